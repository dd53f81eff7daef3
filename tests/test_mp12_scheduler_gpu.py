"""MPEG Layer II behind the batch scheduler (csrc/pipeline.cpp, sk_tick_run_mixed_mpa): a stream whose first confirmed frame is Layer I
or II is parsed on the entropy threads (allocation, scale factors), its frames ride in the tick beside the AAC units and the
Layer III granules, and every Layer II frame becomes two AudioData of 576 frames that take the same apply_output_options path.

* no options: the reference's MP2 fixture alone and beside one ADTS and one Layer III stream -- every stream equals its single decoder;
* 16 kHz mono 16 bit (48 -> 16 k through the FIR): against the oracle's CPU chain on Mp3Decoder's s16;
* a frame whose allocation overruns is dropped, exactly that frame; the clean stream beside it is untouched."""
import os
import threading

import numpy as np
import pytest

from soundkit_amd import pipeline
from test_scheduler_gpu import drain, feed_all
from test_scheduler_mp3_gpu import read, single_decoder

pytestmark = pytest.mark.gpu
MP2 = "mp2/stereo48k_A_Tusk_1s.mp2"
ADTS = "aac/aac-stereo-48k.adts"
MP3 = "mp3/stereo16k_A_Tusk_encoded.mp3"


def run(engine, datas, chunks, options=None, **config):
    sched = pipeline.BatchScheduler(engine, entropy_threads=3, max_streams=8, **config)
    try:
        handles = [sched.spawn(options) if options is not None else sched.spawn() for _ in datas]
        feeder = threading.Thread(target=feed_all, args=(handles, datas, chunks))
        feeder.start()
        outs = drain(handles, 60)
        feeder.join()
        for h in handles:
            h.cancel()
    finally:
        sched.close()
    for got in outs:
        assert got and not any(isinstance(a, Exception) for a in got), [a for a in got if isinstance(a, Exception)][:1]
    return outs


def samples_of(outs):
    return np.concatenate([np.frombuffer(a.data.tobytes(), "<i2") for a in outs])


@pytest.fixture(scope="module")
def mp2_alone(engine):
    rate, channels, samples = single_decoder(engine, "mp2", read(MP2))
    assert (rate, channels, samples.size) == (48000, 2, 42 * 1152 * 2) and np.abs(samples.astype(np.int32)).max() > 500
    return samples


@pytest.mark.parametrize("front_end", [0, 3], ids=["host_front_end", "gpu_front_end_with_mp3_huffman_in_the_tick"])
def test_the_fixture_alone_and_beside_an_adts_and_a_layer_three_stream(engine, mp2_alone, front_end):
    names = [MP2, ADTS, MP3, MP2]
    datas = [read(n) for n in names]
    want = [mp2_alone, single_decoder(engine, ADTS, datas[1])[2], single_decoder(engine, MP3, datas[2])[2], mp2_alone]
    alone = run(engine, [datas[0]], [100000], gpu_entropy=front_end)[0]
    assert np.array_equal(samples_of(alone), mp2_alone)
    # small per-stream and per-tick budgets: many ticks, every one with frames of all three kinds; odd chunk sizes
    outs = run(engine, datas, [113, 1500, 777, 4096], max_frames_per_tick=24, max_stream_frames_per_tick=5, gpu_entropy=front_end)
    for name, got, samples in zip(names, outs, want):
        if name == MP2:
            assert len(got) == 84  # two AudioData per Layer II frame
            assert all((a.sampling_rate, a.channel_count, a.bits_per_sample, a.data.size) == (48000, 2, 16, 576 * 2 * 2) for a in got)
        assert np.array_equal(samples_of(got), samples), name


def test_sixteen_kilohertz_mono_meets_the_cpu_chain(engine, oracle, mp2_alone):
    q = mp2_alone.reshape(-1, 2)  # Mp3Decoder's i16 AudioData
    rs = oracle.StreamingResampler(48000, 16000, 2)
    outs = []
    for g in range(0, q.shape[0], 576):  # the worker resamples AudioData by AudioData
        res = rs.process(np.ascontiguousarray(q[g:g + 576].T.astype(np.float32) / np.float32(32768.0)))
        if res.shape[1]:
            outs.append(oracle.planar_f32_to_s16_interleaved(oracle.downmix_mono(res)[None]))
    tail = rs.flush()
    if tail.shape[1]:
        outs.append(oracle.planar_f32_to_s16_interleaved(oracle.downmix_mono(tail)[None]))
    want = np.concatenate([o.reshape(-1) for o in outs]).astype(np.int32)
    assert np.abs(want).max() > 300

    data = read(MP2)
    got = run(engine, [data] * 3, [777, 4096, 100000], pipeline.DecodeOptions(16, 16000, 1))
    for outs in got:
        assert all(a.sampling_rate == 16000 and a.channel_count == 1 and a.bits_per_sample == 16 for a in outs)
        mine = samples_of(outs).astype(np.int32)
        assert mine.size == want.size, (mine.size, want.size)
        d = np.abs(mine - want)
        print("largest difference %d, %.4f %% of the samples differ" % (int(d.max()), 100 * float((d > 0).mean())))
        assert d.max() <= 1 and (d > 0).mean() < 0.01, (int(d.max()), float((d > 0).mean()))


def test_a_damaged_frame_loses_exactly_its_samples(engine, mp2_alone):
    good = read(MP2)
    bad = bytearray(good)
    k = 17
    bad[576 * k + 4:576 * k + 24] = b"\xff" * 20  # every allocation of frame 17 at its widest class: the samples would overrun the frame
    bad = bytes(bad)
    want_bad = single_decoder(engine, "mp2", bad)[2]
    assert want_bad.size == 41 * 2304
    outs = run(engine, [good, bad, good], [1500, 1500, 333], max_stream_frames_per_tick=4)
    assert np.array_equal(samples_of(outs[0]), mp2_alone) and np.array_equal(samples_of(outs[2]), mp2_alone)
    mine = samples_of(outs[1])
    assert len(outs[1]) == 82 and mine.size == 41 * 2304
    assert np.array_equal(mine, want_bad)
    assert np.array_equal(mine[:k * 2304], mp2_alone[:k * 2304])  # untouched up to the damage; behind it the FIFO has missed a frame

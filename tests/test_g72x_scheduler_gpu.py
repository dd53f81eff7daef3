"""Headerless telephony streams through the batch scheduler (sk_pipeline_spawn_g711 / _g722 / _g726): the decoder's parameters at the spawn,
every non-empty send one decode and one AudioData, the empty send the end; decoded by the telephony tick in the PCM family's shared path.

Expected values: tests/g72x_model.py's samples send by send (the reference's recordings where a fixture is sent); with output options,
what a raw PCM stream makes of those samples sent in the same pieces -- the path tests/test_pcm_pipeline_gpu.py pins to the CPU chain."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import g72x_model as M
from soundkit_amd import pipeline
from test_flac_scheduler_gpu import cut, feed
from test_pcm_pipeline_gpu import drain, read

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = "A_Tusk_is_used_to_make_costly_gifts"


def load(path):
    with open(os.path.join(GOLDEN, path), "rb") as f:
        return f.read()


def twin(path):
    w = load(path)
    return w[w.index(b"data") + 8:]


def spawn(sched, kind, options):
    what = kind[0]
    if what == "g711":
        return sched.spawn_g711(kind[1], kind[2], kind[3], options)
    if what == "g722":
        return sched.spawn_g722(options)
    return sched.spawn_g726(kind[1], kind[2], options)


def model_sends(kind, sends):
    """-> the model's s16le bytes per send (empty where a G.726 send completes no group)"""
    if kind[0] == "g711":
        return [M.g711_decode(s, kind[1]).astype("<i2").tobytes() for s in sends]
    dec = M.G722Decoder() if kind[0] == "g722" else M.G726Decoder(kind[1], kind[2])
    return [dec.decode(s).astype("<i2").tobytes() for s in sends]


def shape(kind):
    return (kind[2], kind[3]) if kind[0] == "g711" else ((16000, 1) if kind[0] == "g722" else (8000, 1))


def run(engine, streams, others=(), raw=(), budget=0):
    """streams: (kind, DecodeOptions, [sends]); others: chunk lists of detected streams; raw: (RawPcmFormat, DecodeOptions, [pieces])
    -> per stream its outputs, in that order"""
    sched = pipeline.BatchScheduler(engine, entropy_threads=4, max_streams=len(streams) + len(others) + len(raw) + 4, max_stream_frames_per_tick=budget)
    try:
        handles = [spawn(sched, k, o) for k, o, _ in streams] + [sched.spawn() for _ in others] + [sched.spawn_raw_pcm(f, o) for f, o, _ in raw]
        # fed from a thread of its own while this one drains: a stream of more sends than the input and output queues hold together
        # (128 + 16) is never taken whole while nothing is received
        feeder = threading.Thread(target=feed, args=(handles, [s for _, _, s in streams] + list(others) + [p for _, _, p in raw]))
        feeder.start()
        outs = drain(handles)
        feeder.join()
        for h in handles:
            h.cancel()
    finally:
        sched.close()
    return outs


def audio(outs):
    assert all(not isinstance(o, pipeline.DecodeError) for o in outs), [str(o) for o in outs if isinstance(o, pipeline.DecodeError)]
    return b"".join(o.data.tobytes() for o in outs)


@pytest.mark.parametrize("budget", [0, 3])
def test_all_three_spawns_beside_a_wav_and_an_adts_stream(engine, budget):
    from soundkit_amd import engine as E
    rng = np.random.default_rng(11)
    stereo = rng.integers(0, 256, 2 * 6000, dtype=np.uint8).tobytes()
    plain = [(("g711", M.ULAW, 8000, 1), None, cut(load("g711/%s.ulaw" % NAME), 160)),
             (("g711", M.ALAW, 8000, 2), None, cut(stereo, 320)),
             (("g722",), None, cut(load("g722/%s.g722" % NAME), 160)),
             (("g726", 32000, M.LEFT), None, cut(load("g726/%s_32.g726" % NAME), 80)),
             (("g726", 24000, M.LEFT), None, cut(load("g726/%s_24.g726" % NAME), 100)),  # 100 is no multiple of 3: groups wait between sends
             (("g726", 40000, M.RIGHT), None, cut(M.g726_encode(np.frombuffer(twin("g726/%s_40.decoded.wav" % NAME), "<i2")[:1600], 40000, M.RIGHT), 1)),
             (("g726", 16000, M.RIGHT), None, cut(rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), 77))]
    to16k, to8k, mono24 = pipeline.DecodeOptions(16, 16000, 1), pipeline.DecodeOptions(16, 8000, 1), pipeline.DecodeOptions(24, None, 1)
    converted = [(plain[3][0], to16k, plain[3][2]), (plain[4][0], to16k, plain[4][2]), (plain[0][0], to16k, plain[0][2]), (plain[2][0], to8k, plain[2][2]),
                 (plain[1][0], mono24, plain[1][2]), (plain[1][0], to16k, plain[1][2])]
    others = [cut(read("aac/aac-stereo-48k.adts"), 4096), cut(load("g722/%s.decoded.wav" % NAME), 5000)]  # an ADTS and a WAV stream
    alone = run(engine, [], others, budget=budget)
    # what the raw PCM path makes of the model's samples, sent in the same pieces
    raw = [(pipeline.RawPcmFormat(shape(k)[0], shape(k)[1], E.FMT_S16LE), o, [p for p in model_sends(k, s) if p]) for k, o, s in converted]
    outs = run(engine, plain + converted, others, raw, budget=budget)
    n, m = len(plain), len(converted)
    for i, (kind, _, sends) in enumerate(plain):  # one AudioData per send that decodes something, the model's bytes, the spawn's shape
        want = [p for p in model_sends(kind, sends) if p]
        assert [o.data.tobytes() for o in outs[i]] == want, kind
        rate, ch = shape(kind)
        assert all((o.bits_per_sample, o.channel_count, o.sampling_rate) == (16, ch, rate) for o in outs[i]), kind
    # (of the 1000 one-byte sends at 40 kbit/s only every fifth completes a group; a 100-byte send always does, with 1 or 2 bytes left over)
    assert len(outs[0]) == 148 and len(outs[5]) == 1600 // 8 and len(plain[5][2]) == 1000 and len(outs[4]) == len(plain[4][2]) == 89
    # the fixtures are the reference's recordings
    assert audio(outs[0]) == twin("aiff/g711_ulaw.decoded.wav") and audio(outs[2]) == twin("g722/%s.decoded.wav" % NAME)
    assert audio(outs[3]) == twin("g726/%s_32.decoded.wav" % NAME) and audio(outs[4]) == twin("g726/%s_24.decoded.wav" % NAME)
    for j, (kind, opts, _) in enumerate(converted):
        got, want = outs[n + j], outs[n + m + len(others) + j]
        assert audio(got) == audio(want) and len(audio(got)) > 8000, (kind, j)
        assert all((o.bits_per_sample, o.channel_count, o.sampling_rate) == (opts.output_bits_per_sample, 1, opts.output_sample_rate or shape(kind)[0])
                   for o in got), (kind, j)
    # the neighbours are what they are alone
    assert [audio(o) for o in outs[n + m:n + m + len(others)]] == [audio(o) for o in alone]


def test_a_trailing_partial_group_ends_only_its_own_stream(engine):
    data = load("g726/%s_40.g726" % NAME)
    good = cut(load("g726/%s_32.g726" % NAME), 400)
    streams = [(("g726", 32000, M.LEFT), None, good),
               (("g726", 40000, M.LEFT), None, [data[:10], data[10:17]]),
               (("g726", 40000, M.LEFT), pipeline.DecodeOptions(16, 16000, 1), cut(data[:5 * 2000 + 3], 500)),
               (("g726", 24000, M.LEFT), None, [load("g726/%s_24.g726" % NAME)[:301]]),
               (("g722",), None, cut(load("g722/%s.g722" % NAME)[:4001], 1000))]
    outs = run(engine, streams)
    assert audio(outs[0]) == twin("g726/%s_32.decoded.wav" % NAME)
    want = twin("g726/%s_40.decoded.wav" % NAME)
    assert [o.data.tobytes() for o in outs[1][:-1]] == [want[:32], want[32:48]]
    for i, left in ((1, 2), (2, 3), (3, 1)):
        assert isinstance(outs[i][-1], pipeline.DecodeError)
        assert str(outs[i][-1]) == "Decoding failed: G.726 stream ended with %d trailing partial-packet byte(s)" % left
    assert len(audio(outs[2][:-1])) > 2 * 2 * 8000  # what came before the end went out, at twice the rate
    assert audio(outs[3][:-1]) == twin("g726/%s_24.decoded.wav" % NAME)[:1600]
    assert audio(outs[4]) == twin("g722/%s.decoded.wav" % NAME)[:4 * 4001]  # G.722 has no partial anything: it ends with an empty decode


def test_a_stereo_send_that_splits_a_frame(engine):
    """as decoded the samples leave as they came; behind a conversion the stream ends with the reference's conversion text"""
    sends = [bytes(range(100)), bytes(range(101)), bytes(range(99))]
    outs = run(engine, [(("g711", M.ULAW, 8000, 2), None, sends), (("g711", M.ULAW, 8000, 2), pipeline.DecodeOptions(16, None, 1), sends)])
    assert [o.data.tobytes() for o in outs[0]] == model_sends(("g711", M.ULAW), sends)
    assert len(outs[1]) == 2 and len(outs[1][0].data.tobytes()) == 100
    assert str(outs[1][1]) == "Decoding failed: Output conversion failed: PCM data is unsupported or contains a partial frame"


def test_the_spawn_parameter_errors_are_returned(engine):
    from soundkit_amd import SoundkitError, telephony
    from soundkit_amd._lib import lib
    sched = pipeline.BatchScheduler(engine, max_streams=4)
    try:
        with pytest.raises(telephony.TelephonyError, match=r"^G\.711 sample rate must be > 0$"):
            sched.spawn_g711(telephony.ULAW, 0, 1)
        with pytest.raises(telephony.TelephonyError, match=r"^G\.711 channel count must be > 0$"):
            sched.spawn_g711(telephony.ALAW, 8000, 0)
        with pytest.raises(ValueError, match="rate must be one of"):
            sched.spawn_g726(8000)
        with pytest.raises(ValueError, match="law must be"):
            sched.spawn_g711(telephony.G722, 8000, 1)
        handle = C.c_uint32(77)
        assert lib.sk_pipeline_spawn_g726(sched._h, 8000, 0, None, C.byref(handle)) == -1
        assert lib.sk_pipeline_spawn_g726(sched._h, 32000, 2, None, C.byref(handle)) == -1
        assert lib.sk_pipeline_spawn_g711(sched._h, 2, 8000, 1, None, C.byref(handle), None, 0) == -1 and handle.value == 77
        with pytest.raises(SoundkitError) as e:  # apply_output_options' own check, as for every spawn
            sched.spawn_g722(pipeline.DecodeOptions(12, None, None))
        assert e.value.status == -6
        # nothing of this took a slot
        hs = [sched.spawn_g722() for _ in range(4)]
        for h in hs:
            h.cancel()
    finally:
        sched.close()


def test_cancel_mid_stream(engine):
    data = load("g722/%s.g722" % NAME)
    sched = pipeline.BatchScheduler(engine, max_streams=4)
    try:
        gone, stays = sched.spawn_g722(pipeline.DecodeOptions(16, 8000, 1)), sched.spawn_g726(32000, M.LEFT)
        for k in range(0, 8000, 160):
            send(gone, data[k:k + 160])
        first = drain_one(gone)
        assert (first.bits_per_sample, first.channel_count, first.sampling_rate) == (16, 1, 8000)
        gone.cancel()
        with pytest.raises(pipeline.DecodeError):
            gone.send(data[:160])
        feed([stays], [cut(load("g726/%s_32.g726" % NAME), 160)])
        assert audio(drain([stays])[0]) == twin("g726/%s_32.decoded.wav" % NAME)
        again = sched.spawn_g722()  # the slot is free again and starts from a fresh carry
        feed([again], [cut(data, 4000)])
        assert audio(drain([again])[0]) == twin("g722/%s.decoded.wav" % NAME)
        stays.cancel()
        again.cancel()
    finally:
        sched.close()


def send(handle, data):
    import time
    while True:
        try:
            return handle.send(data)
        except pipeline.DecodeError as e:
            assert e.kind == "InputBufferFull", e
            time.sleep(0.0005)


def drain_one(handle, deadline_s=60):
    import time
    t0 = time.time()
    while time.time() - t0 < deadline_s:
        got = handle.try_recv()
        if got is not None:
            return got
        time.sleep(0.0005)
    raise AssertionError("no output")

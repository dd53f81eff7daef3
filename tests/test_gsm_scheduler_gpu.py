"""GSM 06.10 streams through the batch scheduler (sk_pipeline_spawn_gsm): the variant at the spawn, every send that completes at least
one packet one decode and one AudioData, the empty send the end; decoded by the GSM tick in the PCM family's shared path.

Expected values: the reference's recording where the fixture is sent, tests/gsm_model.py's samples send by send elsewhere; with output
options, what a raw PCM stream makes of those samples sent in the same pieces -- the path tests/test_pcm_pipeline_gpu.py pins to the
CPU chain."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import gsm_model as M
from soundkit_amd import pipeline
from test_flac_scheduler_gpu import cut, feed
from test_pcm_pipeline_gpu import drain

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gsm")
NAME = "A_Tusk_is_used_to_make_costly_gifts"


def load(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def twin():
    w = load(NAME + ".decoded.wav")
    return w[w.index(b"data") + 8:]


def model_sends(variant, sends):
    """-> the model's s16le bytes per send (empty where a send completes no packet)"""
    dec = M.GsmDecoder(variant)
    return [dec.decode(s).astype("<i2").tobytes() for s in sends]


def run(engine, streams, raw=(), budget=0):
    """streams: (variant, DecodeOptions, [sends]); raw: (RawPcmFormat, DecodeOptions, [pieces]) -> per stream its outputs, in that order"""
    sched = pipeline.BatchScheduler(engine, entropy_threads=4, max_streams=len(streams) + len(raw) + 4, max_stream_frames_per_tick=budget)
    try:
        handles = [sched.spawn_gsm(v, o) for v, o, _ in streams] + [sched.spawn_raw_pcm(f, o) for f, o, _ in raw]
        feeder = threading.Thread(target=feed, args=(handles, [s for _, _, s in streams] + [p for _, _, p in raw]))
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
def test_the_fixture_equals_the_recording_in_pieces_and_whole_in_both_framings(engine, budget):
    from soundkit_amd import engine as E
    data = load(NAME + ".gsm")
    ms = M.standard_to_microsoft(data)
    plain = [(M.STANDARD, None, cut(data, 41)), (M.STANDARD, None, [data]), (M.MICROSOFT, None, cut(ms, 41)), (M.MICROSOFT, None, [ms]),
             (M.STANDARD, None, cut(data, 19))]
    to16k, stereo24 = pipeline.DecodeOptions(16, 16000, 1), pipeline.DecodeOptions(24, None, 2)
    converted = [(M.STANDARD, to16k, plain[0][2]), (M.MICROSOFT, stereo24, plain[2][2])]
    # what the raw PCM path makes of the model's samples, sent in the same pieces
    raw = [(pipeline.RawPcmFormat(8000, 1, E.FMT_S16LE), o, [p for p in model_sends(v, s) if p]) for v, o, s in converted]
    outs = run(engine, plain + converted, raw, budget=budget)
    for i, (variant, _, sends) in enumerate(plain):
        assert audio(outs[i]) == twin(), i
        # one AudioData per send that completes a packet, the model's bytes send by send: 8 kHz, mono, 16 bits
        assert [o.data.tobytes() for o in outs[i]] == [p for p in model_sends(variant, sends) if p], i
        assert all((o.bits_per_sample, o.channel_count, o.sampling_rate) == (16, 1, 8000) for o in outs[i]), i
    assert len(outs[0]) == 120 and len(outs[1]) == 1 and len(outs[3]) == 1 and len(outs[4]) == 148  # 19-byte sends: 258, of which 148 complete a frame
    n = len(plain)
    for j, (variant, opts, _) in enumerate(converted):
        got, want = outs[n + j], outs[n + len(converted) + j]
        assert audio(got) == audio(want) and len(audio(got)) > 2 * 23680, j
        # the AudioData's shape is what the raw PCM stream's is (a mono source asked for two channels stays what apply_output_options makes of it)
        assert {(o.bits_per_sample, o.channel_count, o.sampling_rate) for o in got} == {(o.bits_per_sample, o.channel_count, o.sampling_rate) for o in want}, j
        assert all((o.bits_per_sample, o.sampling_rate) == (opts.output_bits_per_sample, opts.output_sample_rate or 8000) for o in got), j


def test_three_streams_end_alone_while_their_neighbours_go_on(engine):
    data = load(NAME + ".gsm")
    want = twin()
    rejected = bytearray(data[:33 * 20])
    rejected[33 * 13] = 0x90 | (rejected[33 * 13] & 15)  # the fourteenth frame: the second of the fifth 99-byte send
    streams = [(M.STANDARD, None, cut(data, 330)),
               (M.STANDARD, None, cut(data[:33 * 10 + 3], 100)),                        # a trailing partial packet
               (M.STANDARD, None, cut(bytes(rejected), 99)),                            # a rejected frame
               (M.STANDARD, None, [data[:66], data[:33] * 1639, data[66:99]]),          # an oversized send
               (M.MICROSOFT, pipeline.DecodeOptions(16, 16000, 1), cut(M.standard_to_microsoft(data)[:65 * 30 + 64], 500)),
               (M.MICROSOFT, None, cut(M.standard_to_microsoft(data), 650))]
    outs = run(engine, streams)
    assert audio(outs[0]) == want and audio(outs[5]) == want
    texts = {1: "Decoding failed: GSM stream ended with 3 trailing partial-frame byte(s)",
             2: "Decoding failed: GSM decoder rejected frame",
             3: "Decoding failed: Output buffer too small for GSM decode: need 262240, have 262144",
             4: "Decoding failed: GSM stream ended with 64 trailing partial-frame byte(s)"}
    for i, text in texts.items():
        assert isinstance(outs[i][-1], pipeline.DecodeError) and str(outs[i][-1]) == text, i
    # what came before the end went out
    assert audio(outs[1][:-1]) == want[:320 * 10]
    assert audio(outs[2][:-1]) == want[:320 * 12] and len(outs[2]) == 5  # four whole sends, then the error
    assert audio(outs[3][:-1]) == want[:320 * 2] and len(outs[3]) == 2
    assert len(audio(outs[4][:-1])) > 2 * 2 * 160 * 50  # at twice the rate


def test_the_spawn_checks_its_variant(engine):
    from soundkit_amd._lib import lib
    sched = pipeline.BatchScheduler(engine, max_streams=2)
    try:
        with pytest.raises(ValueError, match="variant must be"):
            sched.spawn_gsm(2)
        handle = C.c_uint32(77)
        assert lib.sk_pipeline_spawn_gsm(sched._h, 2, None, C.byref(handle)) == -1
        assert lib.sk_pipeline_spawn_gsm(sched._h, -1, None, C.byref(handle)) == -1 and handle.value == 77
        # nothing of this took a slot, and a slot that is used again starts from a fresh carry
        data = load(NAME + ".gsm")
        for _ in range(2):
            hs = [sched.spawn_gsm(), sched.spawn_gsm(M.MICROSOFT)]
            feed(hs, [[data[:330]], [M.standard_to_microsoft(data[:330])]])
            got = drain(hs)
            assert audio(got[0]) == audio(got[1]) == twin()[:3200]
            for h in hs:
                h.cancel()
    finally:
        sched.close()

"""AIFF / AIFF-C streams through the batch scheduler: found by their FORM header behind the detection buffer, or spawned with their
decoder (spawn_aiff); every AudioData against the model of the reference's decoder (tests/aiff_model.py) fed the way the reference's
worker feeds it; with output options, against a raw PCM stream that is fed the model's decoded PCM; tiled beside ADTS and WAV
streams; failing streams end alone with the reference's text; and the channel limits of a conversion."""
import os
import threading

import numpy as np
import pytest

import aiff_builder as B
import aiff_model as M
from soundkit_amd import pipeline
from soundkit_amd import engine as E
from test_aiff_stream_cpu import FIXTURES, load
from test_pcm_pipeline_gpu import as_model, drain, feed, read

pytestmark = pytest.mark.gpu

MIN_DETECTION, MAX_DETECTION = 8192, 65536


def worker_model(chunks, auto):
    """what the reference's pipeline worker makes of an AIFF stream: (list of Audio, error text or None).  auto: the detection buffer
    (chunks gathered until 8192 bytes are there or the stream ends, at most 65536 of them) is one add, the rest of the chunk that
    completed it a second one; then one add per chunk; the end of the stream is the finalising empty add."""
    m = M.AiffModel()
    adds = []
    rest = list(chunks)
    if auto:
        buf = b""
        while rest and len(buf) < MIN_DETECTION:
            buf += rest.pop(0)
        adds.append(buf[:MAX_DETECTION])
        if len(buf) > MAX_DETECTION:
            adds.append(buf[MAX_DETECTION:])
    adds += rest + [b""]
    outs = []
    for a in adds:
        try:
            got = m.add(a)
        except ValueError as exc:
            return outs, "Decoding failed: " + str(exc)
        if got is not None:
            outs.append(got)
    return outs, None


def run(engine, streams, lanes=1):
    """streams: (kind, DecodeOptions, chunks), kind = "auto" (spawn), "aiff" (spawn_aiff) or a RawPcmFormat -> per stream its outputs"""
    sched = pipeline.BatchScheduler(engine, entropy_threads=4, max_streams=len(streams) + 4, lanes=lanes)
    try:
        handles = []
        for kind, opt, _ in streams:
            handles.append(sched.spawn(opt) if kind == "auto" else sched.spawn_aiff(opt) if kind == "aiff" else sched.spawn_raw_pcm(kind, opt))
        lists = [c for _, _, c in streams]
        half = len(handles) // 2
        feeders = [threading.Thread(target=feed, args=(handles[:half], lists[:half])), threading.Thread(target=feed, args=(handles[half:], lists[half:]))]
        for t in feeders:
            t.start()
        outs = drain(handles)
        for t in feeders:
            t.join()
        for h in handles:
            h.cancel()
    finally:
        sched.close()
    return outs


def cut(data, n):
    return [data[at:at + n] for at in range(0, len(data), n)]


def check_against_model(got_raw, chunks, auto, label):
    got, err = as_model(got_raw)
    want, want_err = worker_model(chunks, auto)
    assert err == want_err, (label, err, want_err)
    assert len(got) == len(want), (label, len(got), len(want))
    for g, w in zip(got, want):
        assert g[:5] == (w.bits, w.channels, w.sample_rate, w.is_float, False), label
        assert g[5] == w.data, label


def test_fixtures_detected_and_spawned(engine):
    streams, checks = [], []
    for name in FIXTURES:
        data = load(name)
        streams.append(("auto", pipeline.DecodeOptions(), [data]))  # the whole file in one send
        checks.append(([data], True, name + " detected"))
        parts = cut(data, 997)
        streams.append(("aiff", pipeline.DecodeOptions(), parts))
        checks.append((parts, False, name + " spawned"))
    outs = run(engine, streams)
    for o, (chunks, auto, label) in zip(outs, checks):
        check_against_model(o, chunks, auto, label)
        if auto:  # one AudioData for the detection buffer, one more where the file is longer than that
            assert len(o) == (1 if len(chunks[0]) <= MAX_DETECTION else 2), label


def contract_format(audio):
    return {(16, False): E.FMT_S16LE, (24, False): E.FMT_S24LE, (32, False): E.FMT_S32LE, (32, True): E.FMT_F32LE}[(audio.bits, audio.is_float)]


def stereo_ima4(groups, seed):
    p = B.ima4_packets(np.random.default_rng(seed), groups, 2)
    p[:, :, 2:] &= 0x37  # small nibbles: a signal that stays away from the rails
    return B.simple(b"ima4", 2, 16, 44100.0, p.tobytes(), frames=groups)


def test_options_equal_a_raw_pcm_stream_of_the_decoded_pcm(engine):
    cases = [(load(FIXTURES[0]), pipeline.DecodeOptions(None, 16000, None)),                     # 8 -> 16 kHz
             (load("stream-s24be.aifc"), pipeline.DecodeOptions(16, None, None)),                 # s24be -> 16 bit (the exact path)
             (load("stream-f64be.aifc"), pipeline.DecodeOptions(16, None, 1)),                    # f64 -> s16 mono
             (stereo_ima4(700, 5), pipeline.DecodeOptions(16, 16000, 1))]                         # IMA4 stereo -> 16 kHz mono
    streams = []
    for data, opt in cases:
        parts = cut(data, 9973)
        decoded, err = worker_model(parts, False)
        assert err is None and decoded
        a = decoded[0]
        streams.append(("aiff", opt, parts))
        streams.append(("auto", opt, parts))
        streams.append((pipeline.RawPcmFormat(a.sample_rate, a.channels, contract_format(a)), opt, [d.data for d in decoded]))
    outs = [as_model(o) for o in run(engine, streams)]
    for k, (data, opt) in enumerate(cases):
        (spawned, e1), (detected, e2), (raw, e3) = outs[3 * k:3 * k + 3]
        assert e1 is None and e2 is None and e3 is None and raw, k
        want = b"".join(r[5] for r in raw)
        assert len(want) > 1000 and any(want)
        for got in (spawned, detected):
            assert {g[:5] for g in got} == {r[:5] for r in raw}, k
            assert b"".join(g[5] for g in got) == want, k


_ALONE = []


@pytest.mark.parametrize("lanes", [1, 2])
def test_65_tiled_streams_beside_adts_and_wav(engine, lanes):
    rng = np.random.default_rng(60 + lanes)
    kinds = []
    for name in FIXTURES:
        data = load(name)
        kinds.append(("aiff", pipeline.DecodeOptions(), cut(data, 4001)))
        kinds.append(("auto", pipeline.DecodeOptions(16, 16000, None), cut(data, 30011)))
    kinds.append(("aiff", pipeline.DecodeOptions(16, 16000, 1), cut(stereo_ima4(300, 9), 5003)))
    others = [("auto", pipeline.DecodeOptions(), cut(read("aac/aac-stereo-48k.adts"), 3000)),
              ("auto", pipeline.DecodeOptions(16, None, 1), cut(read("wav_stereo_A_Tusk.wav"), 20000))]
    if not _ALONE:  # every kind of stream by itself, once for both cases
        _ALONE.extend(as_model(run(engine, [k])[0]) for k in kinds + others)
    alone = _ALONE
    assert all(err is None and outs for outs, err in alone)
    order = [int(x) for x in rng.permutation(65) % len(kinds)]
    streams = [kinds[i] for i in order] + others
    outs = run(engine, streams, lanes)
    for k, i in enumerate(order + [len(kinds), len(kinds) + 1]):
        got, err = as_model(outs[k])
        want, _ = alone[i]
        assert err is None, (k, err)
        if streams[k][1].output_sample_rate:  # AudioData boundaries of a resampled stream are the resampler's chunks: the same either way
            assert [g[:5] for g in got] == [w[:5] for w in want], k
        assert b"".join(g[5] for g in got) == b"".join(w[5] for w in want), (k, i)
        assert len(got) == len(want), k


def test_failing_streams_end_alone(engine):
    good = load("stream-ulaw.aifc")
    ima = load("stream-ima4.aifc")
    cases = [("aiff", cut(load("stream-s24be.aifc")[:30000], 997)),           # truncated inside the sound
             ("auto", [load(FIXTURES[0])[:20001]]),                            # ... and found by detection, inside a sample
             ("aiff", cut(good + b"trailing", 5000)),                          # bytes after the FORM
             ("auto", [good + b"x"]),
             ("aiff", [ima[:12 + 30]]),                                        # truncated in a chunk
             ("aiff", [B.form([B.comm(1, 0, 16, 8000.0)], kind=b"8SVX")]),
             ("aiff", [B.form([B.fver(), B.comm(3, 0, 16, 8000.0, b"ima4"), B.ssnd(b"")], aifc=True)])]
    streams = [(kind, pipeline.DecodeOptions(), chunks) for kind, chunks in cases]
    streams += [("aiff", pipeline.DecodeOptions(), cut(good, 997)), ("auto", pipeline.DecodeOptions(16, 16000, None), [ima])]
    outs = run(engine, streams)
    for k, (kind, chunks) in enumerate(cases):
        _, want_err = worker_model(chunks, kind == "auto")
        assert want_err is not None, k
        check_against_model(outs[k], chunks, kind == "auto", "case %d" % k)
        assert outs[k][-1].status == -401
    check_against_model(outs[len(cases)], cut(good, 997), False, "neighbour")
    got, err = as_model(outs[len(cases) + 1])  # ... and the resampled neighbour gives what it gives alone
    alone, alone_err = as_model(run(engine, [streams[-1]])[0])
    assert err is None and alone_err is None and alone and got == alone


def test_channel_limits(engine):
    import soundkit_amd
    rng = np.random.default_rng(70)
    four = B.simple(None, 4, 16, 44100.0, rng.integers(-20000, 20000, 4 * 9000).astype(">i2").tobytes(), frames=9000)
    many = B.simple(None, 32, 24, 48000.0, rng.integers(0, 256, 32 * 3 * 500, dtype=np.uint8).tobytes(), frames=500)
    opt = pipeline.DecodeOptions(16, 16000, 2)
    parts, many_parts = cut(four, 7001), cut(many, 7001)
    outs = run(engine, [("aiff", opt, parts), ("aiff", pipeline.DecodeOptions(), many_parts), ("aiff", pipeline.DecodeOptions(None, None, 1), parts)])
    got, err = as_model(outs[0])
    assert got == [] and err == "Decoding failed: conversion of PCM with more than 2 channels is not supported" and outs[0][-1].status == -6
    check_against_model(outs[1], many_parts, False, "32 channels, decode only")  # s24be reversed on the device, no conversion
    assert as_model(outs[2])[1] == err
    wide = soundkit_amd.Engine(0, 64)
    try:
        wide.enable_wide_pcm(8)
        whole = [four[:54 + 8000]] + cut(four[54 + 8000:], 8000)  # sends that end on frames (the header is 54 bytes)
        decoded, _ = worker_model(whole, False)
        outs = [as_model(o) for o in run(wide, [("aiff", opt, whole), (pipeline.RawPcmFormat(44100, 4, E.FMT_S16LE), opt, [d.data for d in decoded]),
                                                ("aiff", opt, parts)])]
        (got, e1), (raw, e2), (_, e3) = outs
        assert e1 is None and e2 is None and raw and {g[:5] for g in got} == {(16, 2, 16000, False, False)}
        assert b"".join(g[5] for g in got) == b"".join(r[5] for r in raw)
        # a send that ends inside a frame: the decoder emits the whole samples, and the conversion refuses them as the reference's does
        assert e3 == "Decoding failed: Output conversion failed: PCM data is unsupported or contains a partial frame"
    finally:
        wide.close()

"""5.1 WAV files and headerless 8-channel PCM through the batch scheduler on an engine with the pool of wide streams
(sk_engine_enable_wide_pcm): boundaries, info and bytes of wide_pcm_model's worker, beside a stereo WAV and an AAC stream; one
stream more than the pool holds fails alone; and an engine without the pool answers as it always did."""
import numpy as np
import pytest

import pcm_worker_model as M
import wide_pcm_model as W
from soundkit_amd import pipeline
from test_pcm_pipeline_gpu import as_model, hashes, lsb_check, read, through_scheduler, wav_file
from test_pcm_tick_formats_gpu import wav_extensible
from test_wide_pcm_gpu import encode

pytestmark = pytest.mark.gpu

OLD_MESSAGE = "Decoding failed: conversion of PCM with more than 2 channels is not supported"


@pytest.fixture(scope="module")
def wide(engine):
    import soundkit_amd
    eng = soundkit_amd.Engine(0, 64)
    eng.enable_wide_pcm(32)
    yield eng
    eng.close()


def wav_worker(oracle, chunks, out_bits, out_rate, out_ch):
    """pcm_worker_model.wav_worker with the output stage for any channel count"""
    outs = []
    wav, pieces, err = M.wav_pieces(chunks)
    assert err is None and pieces
    stage = W.WideOutputStage(oracle, wav.rate, wav.channels, wav.bits, wav.is_float, False, out_bits, out_rate, out_ch)
    for p in pieces:
        outs += stage.piece(p)
    return outs + stage.flush()


def raw_worker(oracle, chunks, rate, channels, fmt, out_bits, out_rate, out_ch):
    bits = 16 if fmt <= M.FMT_S16BE else (24 if fmt <= M.FMT_S24BE else 32)
    raw = M.RawModel(bits // 8 * channels)
    stage = W.WideOutputStage(oracle, rate, channels, bits, fmt >= M.FMT_F32LE, bool(fmt & 1), out_bits, out_rate, out_ch)
    outs = []
    for chunk in chunks:
        piece = raw.add(chunk) if chunk else None
        if piece:
            outs += stage.piece(piece)
    raw.flush()
    return outs + stage.flush()


def pcm(fmt, channels, frames, seed):
    return encode(np.random.default_rng(seed).uniform(-1.0, 1.0, (frames, channels)), fmt)


# -> 16 kHz mono s16 | stereo 24-bit | 16 bits with the channels kept (the fast path for the 16-bit files, the exact path on eight
# channels for the 24-bit stream)
OPTIONS = [(16, 16000, 1), (24, None, 2), (16, None, None)]


@pytest.mark.parametrize("lanes", [1, 2])
def test_wide_streams_through_the_scheduler(wide, oracle, lanes):
    rng = np.random.default_rng(200 + lanes)
    frames = 4096 * 2 + 1777
    six = pcm(M.FMT_S16LE, 6, frames, 1)
    sources = [("wav", wav_file(6, 48000, 16, six)), ("wav", wav_extensible(6, 48000, 16, six)),
               (M.FMT_S24BE, pcm(M.FMT_S24BE, 8, frames, 2))]
    streams, want, opts = [], [], []
    for kind, data in sources:
        for bits, out_rate, out_ch in OPTIONS:
            chunks = M.ragged(data, rng, 1, 30000)
            opt = pipeline.DecodeOptions(bits, out_rate, out_ch)
            if kind == "wav":
                streams.append((None, opt, chunks))
                want.append(wav_worker(oracle, chunks, bits, out_rate, out_ch))
            else:
                streams.append((pipeline.RawPcmFormat(44100, 8, kind), opt, chunks))
                want.append(raw_worker(oracle, chunks, 44100, 8, kind, bits, out_rate, out_ch))
            opts.append((bits, out_rate, out_ch))
    stereo = M.ragged(read("wav_stereo_A_Tusk.wav"), rng, 1, 30000)
    streams.append((None, pipeline.DecodeOptions(24, None, 1), stereo))
    want.append(M.wav_worker(oracle, stereo, 24, None, 1)[0])
    opts.append((24, None, 1))
    extra = [M.ragged(read("aac/aac-stereo-48k.adts"), rng, 200, 6000)]
    alone = [hashes(o) for o in through_scheduler(wide, [], 1, extra)]
    outs = through_scheduler(wide, streams, lanes, extra)
    for k, exp in enumerate(want):
        got, err = as_model(outs[k])
        assert err is None, (k, err)
        assert exp and [g[:5] + (len(g[5]),) for g in got] == [w[:5] + (len(w[5]),) for w in exp], k
        if opts[k][1]:
            lsb_check(b"".join(g[5] for g in got), b"".join(w[5] for w in exp), "stream %d" % k)
        else:
            assert all(g[5] == w[5] for g, w in zip(got, exp)), k
    assert hashes(outs[len(want)]) == alone[0] and alone[0]


def test_one_stream_more_than_the_pool_holds(oracle):
    import soundkit_amd
    eng = soundkit_amd.Engine(0, 64)
    try:
        eng.enable_wide_pcm(2)
        data = wav_file(6, 48000, 16, pcm(M.FMT_S16LE, 6, 9000, 3))
        opt = pipeline.DecodeOptions(16, 16000, 1)
        parts = [data[k:k + 16000] for k in range(0, len(data), 16000)]  # several sends each: all three are open before one ends
        assert len(parts) >= 6
        streams = [(None, opt, parts) for _ in range(3)]
        streams.append((None, pipeline.DecodeOptions(24, None, 2), parts))  # no rate change: needs no slot
        outs = [as_model(o) for o in through_scheduler(eng, streams)]
        failed = [k for k in range(3) if outs[k][1] is not None]
        assert len(failed) == 1, [o[1] for o in outs]
        assert outs[failed[0]][0] == [] and outs[failed[0]][1].startswith("Decoding failed: engine stream: capacity exhausted")
        exp = wav_worker(oracle, parts, 16, 16000, 1)
        for k in range(3):
            if k != failed[0]:
                got = outs[k][0]
                assert [g[:5] + (len(g[5]),) for g in got] == [w[:5] + (len(w[5]),) for w in exp], k
        got, err = outs[3]
        exp = wav_worker(oracle, parts, 24, None, 2)
        assert err is None and [g[5] for g in got] == [w[5] for w in exp]
    finally:
        eng.close()


def test_without_the_pool_the_answer_is_the_old_one(engine):
    data = wav_file(6, 48000, 16, pcm(M.FMT_S16LE, 6, 5000, 4))
    streams = [(None, pipeline.DecodeOptions(16, 16000, 1), [data]), (None, pipeline.DecodeOptions(24, None, 2), [data]),
               (pipeline.RawPcmFormat(44100, 8, M.FMT_S24BE), pipeline.DecodeOptions(16, None, None), [pcm(M.FMT_S24BE, 8, 3000, 5)])]
    raw = through_scheduler(engine, streams)
    for k, o in enumerate(raw):
        got, err = as_model(o)
        assert got == [] and err == OLD_MESSAGE and o[-1].status == -6, k

"""WAV and raw PCM streams through batched GPU ticks (sk_tick_run_pcm: k_pcm_direct, k_pcm_ingest) and through the scheduler.

* the tick against the one-stream path (decoder.apply_output_options unit by unit + flush_resampler_frames): every record and its
  bytes, count and order included, for the five fixtures and their big-endian forms over the OPTIONS grid of test_tick_gpu.py;
* against the CPU chain (tests/pcm_worker_model.py on the oracle): bit-exact without a rate change; through the FIR / sinc
  resampler to 16 bits at most one LSB on at most 1 % of the samples (another order of summation: the bound
  test_tick_against_oracle_with_resampling and test_reference_twins_gpu.py::_check_s16 hold this resampler to);
* the reference's twin recordings through the scheduler: depth reduction bit for bit, resampled pairs within tests/twin_fit.py's pins;
* 64 WAV / raw PCM streams in ragged chunks from two threads beside AAC and MP3 streams, one and two lanes;
* isolation and limits; both kernels at full-device size, every stream identical to the one-stream path."""
import os
import struct
import threading
import time

import numpy as np
import pytest

import pcm_worker_model as M
import twin_fit
from soundkit_amd import decoder, pipeline
from soundkit_amd.audio_types import AudioData, EncodingFlag, Endianness
from test_tick_gpu import OPTIONS

pytestmark = pytest.mark.gpu
GOLD = twin_fit.GOLDEN


def read(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


def sources():
    """name -> (SK_FMT_*, rate, channels, bytes): the five fixtures and their byte-swapped big-endian forms"""
    tw = twin_fit.pcm_twins()
    little = {
        "s16_stereo_16k": (M.FMT_S16LE, 16000, 2, twin_fit.read_wav(twin_fit.golden("wav_stereo_A_Tusk.wav"))[1]),
        "s24_mono_16k": (M.FMT_S24LE, 16000, 1, tw["s24"].tobytes()),
        "f32_mono_16k": (M.FMT_F32LE, 16000, 1, tw["f32"].tobytes()),
        "s32_mono_16k": (M.FMT_S32LE, 16000, 1, tw["s32"].tobytes()),
        "s16_mono_48k": (M.FMT_S16LE, 48000, 1, read(twin_fit.TWIN_FILES[48000])),
    }
    out = dict(little)
    for name, (fmt, rate, ch, data) in little.items():
        width = 2 if fmt <= 1 else (3 if fmt <= 3 else 4)
        out[name + "_be"] = (fmt + 1, rate, ch, twin_fit.swap_bytes(np.frombuffer(data, np.uint8), width).tobytes())
    return out


def fmt_fields(fmt):
    bits = 16 if fmt <= 1 else (24 if fmt <= 3 else 32)
    return bits, fmt >= M.FMT_F32LE, bool(fmt & 1)


def split_units(data, frame_bytes, rng, hi_frames):
    """`data` cut into seeded ragged units of whole frames"""
    out, pos = [], 0
    while pos < len(data):
        n = int(rng.integers(1, hi_frames + 1)) * frame_bytes
        out.append(data[pos:pos + n])
        pos += n
    return out


def fast_path(fmt, rate, ch, bits, out_rate, out_ch):
    src_bits = fmt_fields(fmt)[0]
    return (out_rate or rate) == rate and (bits or src_bits) == src_bits and (out_ch or ch) == ch


def one_at_a_time(fmt, rate, ch, units, bits, out_rate, out_ch):
    """the one-stream path: apply_output_options unit by unit, then the resampler's flush"""
    src_bits, is_float, be = fmt_fields(fmt)
    rs, out = None, []
    for u in units:
        audio = AudioData(src_bits, ch, rate, u, EncodingFlag.PCMFloat if is_float else EncodingFlag.PCMSigned,
                          Endianness.BigEndian if be else Endianness.LittleEndian)
        got, rs = decoder.apply_output_options(audio, bits, out_rate, out_ch, rs)
        out += [(a.bits_per_sample, a.channel_count, a.audio_format == EncodingFlag.PCMFloat, a.data.tobytes()) for a in got]
    if rs is not None:
        b = bits or src_bits
        fl = EncodingFlag.PCMFloat if (b == 32 and is_float) else EncodingFlag.PCMSigned
        out += [(a.bits_per_sample, a.channel_count, a.audio_format == EncodingFlag.PCMFloat, a.data.tobytes())
                for a in decoder.flush_resampler_frames(rs, b, out_ch or ch, fl)]
        rs.close()
    return out


def run_pcm_ticks(engine, specs, per_tick):
    """specs: (fmt, rate, ch, units, bits, out_rate, out_ch); stream i brings per_tick[i] units per tick.  -> outputs per stream"""
    sids, outs, pos = [], [[] for _ in specs], [0] * len(specs)
    for fmt, rate, ch, units, bits, out_rate, out_ch in specs:
        sid = None
        if out_rate and out_rate != rate:
            sid = engine.open_stream(rate, ch)
            engine.resampler_open(sid, rate, out_rate)
        sids.append(sid)
    done = [False] * len(specs)
    while not all(done):
        table, pieces, index = [], [], []
        for i, (fmt, rate, ch, units, bits, out_rate, out_ch) in enumerate(specs):
            if done[i]:
                continue
            take = units[pos[i]:pos[i] + per_tick[i]]
            pos[i] += len(take)
            done[i] = pos[i] >= len(units)
            table.append({"stream": sids[i] or 0, "n_units": len(take), "format": fmt, "channels": ch, "out_bits": bits or fmt_fields(fmt)[0],
                          "out_channels": out_ch or ch, "resample": sids[i] is not None, "flush": done[i] and sids[i] is not None})
            pieces += take
            index.append(i)
        for idx, status, frames, ch_o, bits_o, data, is_float in engine.tick_run_pcm(table, pieces):
            assert status == 0 and len(data) == frames * ch_o * bits_o // 8
            outs[index[idx]].append((bits_o, ch_o, is_float, data))
    for sid in sids:
        if sid is not None:
            engine.close_stream(sid)
    return outs


@pytest.mark.parametrize("bits,out_rate,out_ch", OPTIONS)
def test_tick_matches_the_one_stream_path(engine, bits, out_rate, out_ch):
    """all ten sources side by side in the same ticks, ragged units (some larger than a resampler row holds), uneven unit counts
    per tick: every output record and its bytes equal the one-stream path's, count and order included"""
    from soundkit_amd._lib import SoundkitError
    rng = np.random.default_rng(17)
    specs, names = [], []
    for name, (fmt, rate, ch, data) in sorted(sources().items()):
        if fast_path(fmt, rate, ch, bits, out_rate, out_ch):
            # nothing to convert: the scheduler delivers such pieces as they are, and the tick refuses the stream
            with pytest.raises(SoundkitError) as exc:
                engine.tick_run_pcm([{"n_units": 1, "format": fmt, "channels": ch, "out_bits": fmt_fields(fmt)[0], "out_channels": ch}], [data[:4800]])
            assert exc.value.status == -1
            continue
        width = fmt_fields(fmt)[0] // 8 * ch
        specs.append((fmt, rate, ch, split_units(data, width, rng, 30000 if len(specs) % 2 else 5000), bits, out_rate if out_rate != rate else None, out_ch))
        names.append(name)
    got = run_pcm_ticks(engine, specs, [1 + (3 * i) % 4 for i in range(len(specs))])
    for name, spec, mine in zip(names, specs, got):
        want = one_at_a_time(*spec)
        assert [(m[0], m[1], m[2], len(m[3])) for m in mine] == [(w[0], w[1], w[2], len(w[3])) for w in want], name
        for k, (m, w) in enumerate(zip(mine, want)):
            assert m[3] == w[3], (name, k)


def test_tick_refuses_what_it_does_not_do(engine):
    from soundkit_amd._lib import SoundkitError
    ok = {"n_units": 1, "format": M.FMT_S24LE, "channels": 1, "out_bits": 16, "out_channels": 1}
    unit = bytes(3 * 32)
    assert len(engine.tick_run_pcm([ok], [unit])) == 1
    for bad, status in (({"out_bits": 24}, -1), ({"channels": 3, "out_channels": 3}, -6), ({"out_bits": 20}, -1), ({"format": 8}, -1),
                        ({"resample": 1, "stream": 8191}, -5), ({"flush": 1}, -1), ({"n_units": 2}, -1)):
        with pytest.raises(SoundkitError) as exc:
            engine.tick_run_pcm([dict(ok, **bad)], [unit])
        assert exc.value.status == status, (bad, exc.value.status)
    with pytest.raises(SoundkitError):
        engine.tick_run_pcm([ok], [unit[:-1]])  # not whole frames


def lsb_check(mine, want, label):
    mine, want = np.frombuffer(mine, "<i2").astype(np.int32), np.frombuffer(want, "<i2").astype(np.int32)
    assert mine.size == want.size, (label, mine.size, want.size)
    d = np.abs(mine - want)
    print("\n%s: worst |d| %d, share of samples off by one %.5f of %d" % (label, d.max(), (d > 0).mean(), d.size))
    assert d.max() <= 1 and (d > 0).mean() <= 0.01, (label, int(d.max()), float((d > 0).mean()))


def test_tick_against_the_cpu_chain(engine, oracle):
    rng = np.random.default_rng(23)
    src = sources()
    # without a rate change: bit-exact, every source and every such option
    for name, (fmt, rate, ch, data) in sorted(src.items()):
        for bits, out_rate, out_ch in OPTIONS:
            if (out_rate and out_rate != rate) or fast_path(fmt, rate, ch, bits, None, out_ch):
                continue
            src_bits, is_float, be = fmt_fields(fmt)
            units = split_units(data, src_bits // 8 * ch, rng, 9000)
            mine = run_pcm_ticks(engine, [(fmt, rate, ch, units, bits, None, out_ch)], [3])[0]
            stage = M.OutputStage(oracle, rate, ch, src_bits, is_float, be, bits, None, out_ch)
            want = [o for u in units for o in stage.piece(u)]
            assert [(m[0], m[1], m[2], m[3]) for m in mine] == [(w[0], w[1], w[3], w[5]) for w in want], (name, bits, out_ch)
    # through the resampler to 16 bits: one LSB on at most 1 % of the samples
    cases = [("s16_mono_48k", 16000, None), ("s16_mono_48k", 8000, None), ("s16_stereo_16k", 8000, 1)]
    mono16 = (M.FMT_S16LE, 16000, 1, read(twin_fit.TWIN_FILES[16000]))
    for name, out_rate, out_ch in cases + [("s16_mono_16k", 8000, None)]:
        fmt, rate, ch, data = mono16 if name == "s16_mono_16k" else src[name]
        units = split_units(data, 2 * ch, rng, 30000)
        mine = run_pcm_ticks(engine, [(fmt, rate, ch, units, 16, out_rate, out_ch)], [2])[0]
        stage = M.OutputStage(oracle, rate, ch, 16, False, False, 16, out_rate, out_ch)
        want = [o for u in units for o in stage.piece(u)] + stage.flush()
        assert [(m[0], m[1], len(m[3])) for m in mine] == [(w[0], w[1], len(w[5])) for w in want], name
        lsb_check(b"".join(m[3] for m in mine), b"".join(w[5] for w in want), "%s -> %d Hz, %s channel(s)" % (name, out_rate, out_ch or ch))


# ---- through the scheduler ----------------------------------------------------------------------------------------------------

def feed(handles, chunk_lists):
    pos = [0] * len(handles)
    pending = set(range(len(handles)))
    while pending:
        for i in list(pending):
            try:
                if pos[i] >= len(chunk_lists[i]):
                    handles[i].finish()
                    pending.discard(i)
                else:
                    handles[i].send(chunk_lists[i][pos[i]])
                    pos[i] += 1
            except pipeline.DecodeError as e:
                assert e.kind == "InputBufferFull", e
        time.sleep(0.0002)


def drain(handles, deadline_s=180):
    outs, t0, live = [[] for _ in handles], time.time(), set(range(len(handles)))
    while live:
        assert time.time() - t0 < deadline_s, "scheduler stalled"
        for i in list(live):
            got = handles[i].try_recv()
            if got is not None:
                outs[i].append(got)
            elif handles[i].ended():
                live.discard(i)
        time.sleep(0.0005)
    return outs


def through_scheduler(engine, streams, lanes=1, extra=()):
    """streams: (raw format or None for WAV, DecodeOptions, chunks); extra: (chunks) of AAC / MP3 streams beside them.  -> outputs"""
    sched = pipeline.BatchScheduler(engine, entropy_threads=4, max_streams=len(streams) + len(extra) + 4, lanes=lanes)
    try:
        handles = [sched.spawn_raw_pcm(f, o) if f is not None else sched.spawn(o) for f, o, _ in streams] + [sched.spawn() for _ in extra]
        lists = [c for _, _, c in streams] + list(extra)
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


def as_model(outs):
    """scheduler outputs in the model's form; the error's text last (or None)"""
    err = None
    if outs and isinstance(outs[-1], Exception):
        err, outs = str(outs[-1]), outs[:-1]
    assert not any(isinstance(a, Exception) for a in outs)
    return [(a.bits_per_sample, a.channel_count, a.sampling_rate, a.audio_format == EncodingFlag.PCMFloat, a.endianness == Endianness.BigEndian,
             a.data.tobytes()) for a in outs], err


def test_twins_through_the_scheduler(engine):
    rng = np.random.default_rng(31)
    want16 = read(twin_fit.TWIN_FILES[16000])
    o16 = pipeline.DecodeOptions(output_bits_per_sample=16)
    streams = [(None, o16, M.ragged(read("wav_24_A_Tusk.wav"), rng, 1, 40000)),
               (pipeline.RawPcmFormat(16000, 1, M.FMT_S32LE), o16, M.ragged(read("linear32_A_Tusk.s32le"), rng, 1, 40000))]
    for in_hz, out_hz in twin_fit.PAIRS:
        streams.append((pipeline.RawPcmFormat.linear16(in_hz, 1), pipeline.DecodeOptions(16, out_hz, None),
                        M.ragged(read(twin_fit.TWIN_FILES[in_hz]), rng, 1, 50000)))
    outs = [as_model(o) for o in through_scheduler(engine, streams)]
    for k in (0, 1):
        got, err = outs[k]
        assert err is None and all(g[:5] == (16, 1, 16000, False, False) for g in got)
        assert b"".join(g[5] for g in got) == want16, k
    for (in_hz, out_hz), (got, err) in zip(twin_fit.PAIRS, outs[2:]):
        assert err is None and all(g[:5] == (16, 1, out_hz, False, False) for g in got)
        y = np.frombuffer(b"".join(g[5] for g in got), "<i2").astype(np.float64) / 32768.0
        twin_fit.assert_twin(y, in_hz, out_hz, kind="s16", label="scheduler")


def hashes(outs):
    import hashlib
    assert not any(isinstance(a, Exception) for a in outs)
    return [(a.bits_per_sample, a.channel_count, a.sampling_rate, hashlib.sha1(a.data.tobytes()).hexdigest()) for a in outs]


@pytest.mark.parametrize("lanes", [1, 2])
def test_scheduler_end_to_end(engine, oracle, lanes):
    """64 WAV / raw PCM streams in seeded ragged chunks (1 byte ... the whole file) from two threads beside AAC and MP3 streams:
    every PCM stream's outputs are the model's -- boundaries, info, bytes (resampled 16-bit cases within one LSB on 1 %) -- and the
    AAC / MP3 streams give what they give alone"""
    rng = np.random.default_rng(100 + lanes)
    src = sources()
    wavs = ["wav_stereo_A_Tusk.wav", "wav_24_A_Tusk.wav", "wav_32f_A_Tusk.wav"]
    raws = ["s16_mono_48k", "s32_mono_16k", "s16_stereo_16k_be", "f32_mono_16k", "s24_mono_16k_be"]
    options = [(None, None, None), (16, None, None), (16, 8000, 1), (24, None, 1), (32, None, None), (16, 16000, None), (None, None, 1)]
    streams, want, src_rate = [], [], []
    for k in range(64):
        bits, out_rate, out_ch = options[k % len(options)]
        opt = pipeline.DecodeOptions(bits, out_rate, out_ch)
        hi = [7, 300, 5000, 70000, None][k % 5]
        if k % 2 == 0:
            data = read(wavs[(k // 2) % 3])
            if hi == 7:
                data = data[:2500]  # (a WAV whose data chunk ends early is no error; one-byte sends of a whole file only test the input bound)
            chunks = M.ragged(data, rng, 1, hi)
            streams.append((None, opt, chunks))
            src_rate.append(16000)
            want.append(M.wav_worker(oracle, chunks, bits, out_rate, out_ch))
        else:
            fmt, rate, ch, data = src[raws[(k // 2) % 5]]
            if hi == 7:
                data = data[:2400]
            chunks = M.ragged(data, rng, 1, hi)
            streams.append((pipeline.RawPcmFormat(rate, ch, fmt), opt, chunks))
            src_rate.append(rate)
            want.append(M.raw_worker(oracle, chunks, rate, ch, fmt, bits, out_rate, out_ch))
    coded = [read("aac/aac-stereo-48k.adts"), read("mp3/stereo16k_A_Tusk_encoded.mp3"), read("aac/mono16k_A_Tusk.aac"), read("mp3/mono16k_A_Tusk.mp3")]
    extra = [M.ragged(d, rng, 200, 6000) for d in coded]
    alone = [hashes(o) for o in through_scheduler(engine, [], 1, extra)]
    outs = through_scheduler(engine, streams, lanes, extra)
    for k, (exp, exp_err) in enumerate(want):
        got, err = as_model(outs[k])
        assert err == exp_err, (k, err, exp_err)
        assert [g[:5] + (len(g[5]),) for g in got] == [w[:5] + (len(w[5]),) for w in exp], k
        out_rate = options[k % len(options)][1]
        if out_rate is not None and out_rate != src_rate[k] and got:  # (every such option asks for 16 bits)
            lsb_check(b"".join(g[5] for g in got), b"".join(w[5] for w in exp), "stream %d" % k)
        else:
            assert all(g[5] == w[5] for g, w in zip(got, exp)), k
    for k in range(len(extra)):
        assert hashes(outs[64 + k]) == alone[k] and alone[k], k


def wav_file(channels, rate, bits, pcm, tag=1):
    fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    return b"RIFF" + struct.pack("<I", 36 + len(pcm)) + b"WAVEfmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(pcm)) + pcm


def test_isolation_and_limits(engine, oracle):
    src = sources()
    fmt, rate, ch, stereo = src["s16_stereo_16k"]
    three = np.arange(3 * 5000, dtype="<i2").tobytes()
    be = src["s16_mono_48k_be"][3][:40000]
    f32 = read("wav_32f_A_Tusk.wav")
    streams = [
        (pipeline.RawPcmFormat.linear16(rate, 2), pipeline.DecodeOptions(24, None, None), [stereo[:20000], stereo[20000:40001]]),  # a trailing byte
        (None, pipeline.DecodeOptions(), [wav_file(3, 16000, 16, three)]),
        (None, pipeline.DecodeOptions(output_channels=1), [wav_file(3, 16000, 16, three)]),
        (pipeline.RawPcmFormat.l16(48000, 1), pipeline.DecodeOptions(), [be]),
        (None, pipeline.DecodeOptions(32, 8000, None), [f32[:50000], f32[50000:]]),
        (None, pipeline.DecodeOptions(output_bits_per_sample=16), [wav_file(1, 8000, 8, bytes(1000))]),
        (None, pipeline.DecodeOptions(16, None, None), [read("wav_24_A_Tusk.wav")]),
    ]
    raw = through_scheduler(engine, streams)
    outs = [as_model(o) for o in raw]
    got, err = outs[0]
    assert err == "Decoding failed: Raw PCM stream ended with 1 trailing partial-frame byte(s)"
    assert [g[:5] + (len(g[5]),) for g in got] == [(24, 2, 16000, False, False, 30000), (24, 2, 16000, False, False, 30000)]
    got, err = outs[1]
    assert err is None and [g[:5] for g in got] == [(16, 3, 16000, False, False)] and got[0][5] == three
    got, err = outs[2]
    assert got == [] and err == "Decoding failed: conversion of PCM with more than 2 channels is not supported" and raw[2][-1].status == -6
    got, err = outs[3]
    assert err is None and [g[:5] for g in got] == [(16, 1, 48000, False, True)] and got[0][5] == be
    got, err = outs[4]
    assert err is None and got and all(g[:5] == (32, 1, 8000, True, False) for g in got)
    y = np.frombuffer(b"".join(g[5] for g in got), "<f4")
    want, _ = M.wav_worker(oracle, streams[4][2], 32, 8000, None)  # the CPU chain: same boundaries, floats within the resampler's rounding
    assert [g[:5] + (len(g[5]),) for g in got] == [w[:5] + (len(w[5]),) for w in want]
    w = np.frombuffer(b"".join(o[5] for o in want), "<f4")
    assert np.isfinite(y).all() and np.abs(w).max() > 0.001 and np.abs(y.astype(np.float64) - w).max() < 1e-5  # a third of a 16-bit step
    got, err = outs[5]
    assert got == [] and err == "Decoding failed: Output conversion failed: PCM data is unsupported or contains a partial frame"
    got, err = outs[6]
    assert err is None and b"".join(g[5] for g in got) == read(twin_fit.TWIN_FILES[16000])


# ---- full device ------------------------------------------------------------------------------------------------------------------

def fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def full_device(engine, fmt, rate, ch, data, bits, out_rate, out_ch, n_streams=2048):
    """n_streams copies of `data` in one tick, two seeded unit splits alternating: every stream's bytes equal the one-stream path's"""
    width = fmt_fields(fmt)[0] // 8 * ch
    rng = np.random.default_rng(41)
    splits = [split_units(data, width, rng, 9000), split_units(data, width, rng, 3000)]
    want = b"".join(o[3] for o in one_at_a_time(fmt, rate, ch, [data], bits, out_rate, out_ch))
    sids = []
    if out_rate:
        for _ in range(n_streams):
            sids.append(engine.open_stream(rate, ch))
            engine.resampler_open(sids[-1], rate, out_rate)
    table, pieces = [], []
    for s in range(n_streams):
        units = splits[s & 1]
        table.append({"stream": sids[s] if sids else 0, "n_units": len(units), "format": fmt, "channels": ch, "out_bits": bits, "out_channels": out_ch,
                      "resample": bool(out_rate), "flush": bool(out_rate)})
        pieces += units
    per_stream = [[] for _ in range(n_streams)]
    for idx, status, frames, ch_o, bits_o, out, is_float in engine.tick_run_pcm(table, pieces):
        assert status == 0 and (ch_o, bits_o, is_float) == (out_ch, bits, False)
        per_stream[idx].append(out)
    for sid in sids:
        engine.close_stream(sid)
    first = b"".join(per_stream[0])
    assert len(first) == len(want) and fnv1a(first) == fnv1a(want)
    bad = [s for s in range(n_streams) if b"".join(per_stream[s]) != first]
    assert not bad, (len(bad), bad[:8])


def test_full_device_ingest(engine):
    """2048 streams x 16 384 frames of the 48 kHz fixture -> 16 kHz mono s16 in one tick: thousands of k_pcm_ingest workgroups"""
    data = read(twin_fit.TWIN_FILES[48000])[20000:20000 + 2 * 16384]
    full_device(engine, M.FMT_S16LE, 48000, 1, data, 16, 16000, 1)


def test_full_device_direct(engine):
    """the stereo WAV's data tiled to 2048 streams x 16 384 frames -> 24-bit mono in one tick: thousands of k_pcm_direct workgroups"""
    data = twin_fit.read_wav(twin_fit.golden("wav_stereo_A_Tusk.wav"))[1][:4 * 16384]
    assert len(data) == 4 * 16384
    full_device(engine, M.FMT_S16LE, 16000, 2, data, 24, None, 1)

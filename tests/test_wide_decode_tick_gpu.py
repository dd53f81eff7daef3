"""FLAC and AIFF sources of 3 ... 8 channels with something to convert: behind the decode they reach the wide path of the PCM tick
(csrc/pcm_wide.hip, sk_engine_enable_wide_pcm) through flac_tick_derive / aiff_tick_derive, which was built and tested for WAV / raw PCM.

The decoded PCM is the models' (tests/flac_model.py, tests/aiff_model.py), asserted equal to the source samples on the CPU first; the
expected records are sk_tick_run_pcm's on the same engine, fed that PCM -- test_wide_pcm_gpu.py pins that path to the reference's
downmix_channels.  Every comparison is bit for bit.  The sources carry, in every block, a full-scale sample alone in each channel in
turn over quiet noise that differs from channel to channel: every channel lands in the output with its own coefficient, so a swapped
channel index in the decode or in the derived table cannot cancel out.

On the engine without the pool the same tables are refused as a whole, the streams with nothing to change still deliver, and through
the scheduler a 5.1 stream with a conversion ends alone with the reference's text."""
import functools
import random

import numpy as np
import pytest

import aiff_builder as AB
import aiff_model as AM
import flac_builder as FB
import flac_model as FM
from test_flac_tick_rates_gpu import KINDS, checked_frames

gpu = pytest.mark.gpu

BLOCKS = [192, 4100, 17]  # frames per FLAC block / AIFF unit: more than a 4096-sample slice, and less than a lane's 16 samples times two
RATE = 48000
# what a stream does behind its decode: (out_rate or None, out_channels or None for "as the source", change the depth?)
CONVERSIONS = [("downmix to 2", None, 2), ("downmix to 1", None, 1), ("depth only", None, None), ("48000 to 16000 Hz with a downmix", 16000, None)]
DEALS = [[3], [1, 0, 2]]


@pytest.fixture(scope="module")
def wide(engine):
    """the module's engine with the pool of wide streams (the session's `engine` first: it stays the decoder mirrors' default)"""
    import soundkit_amd
    eng = soundkit_amd.Engine(0, 64)
    try:
        eng.enable_wide_pcm(8)
        yield eng
    finally:
        eng.close()


def source(seed, nch, frames, bits):
    """[frames][nch] integers of `bits` bits: quiet noise, different in every channel, and at frame 2c + 1 (inside the shortest block's
    17 frames for every c < 8) a full-scale sample in channel c alone, positive in the even channels, negative in the odd ones"""
    rng = np.random.default_rng([seed, nch, frames, bits])
    full = 1 << (bits - 1)
    v = rng.integers(-(full // 20), full // 20, (frames, nch), dtype=np.int64)
    for c in range(nch):
        v[2 * c + 1, :] = 0
        v[2 * c + 1, c] = full - 1 if c % 2 == 0 else -full
    for a in range(nch):
        for b in range(a):
            assert (v[:, a] != v[:, b]).sum() > frames // 2
    return v


def le_bytes(v, bits):
    """[frames][nch] integers -> interleaved little-endian samples of the contract's width"""
    if bits == 16:
        return v.astype("<i2").tobytes()
    return np.ascontiguousarray((v & 0xffffff).astype("<u4")).view(np.uint8).reshape(-1, 4)[:, :3].tobytes()


def conversion_of(k, nch, bits, is_float=False):
    """-> (name, out_rate, out_bits, out_channels) of the k-th stream of a table"""
    name, out_rate, out_ch = CONVERSIONS[k % 4]
    if name == "depth only":
        return name, None, 24 if bits == 16 else 16, nch
    if out_rate:
        return name, out_rate, 16, 1 if nch == 7 else 2
    return name, None, 32 if is_float else 16, out_ch


# ---- FLAC ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def flac_stream(nch, bits, damage=None, seed=1):
    """-> ([(frame dict, frame bytes)], [the contract's bytes per frame]); the model has decoded every frame back to its source"""
    blocks_np = [source(seed * 10 + i, nch, n, bits) for i, n in enumerate(BLOCKS)]
    blocks = [[[int(x) for x in b[:, c]] for c in range(nch)] for b in blocks_np]

    def specs(i, ch):
        out = [KINDS[(i + c) % 3] for c in range(len(ch))]
        if damage == i:
            out[0] = dict(KINDS[2], raw_shift=0x1F)  # a negative LPC shift: the framer passes it, the device rejects it
        return out
    data, _ = FB.stream(blocks, bits, RATE, specs)
    if damage is None:
        frames = checked_frames(data, blocks)
    else:  # the frames beside the damaged one are the undamaged stream's
        from soundkit_amd import flac
        r = flac.FlacReader()
        frames = r.add(data) + r.add(b"")
        r.close()
        good = flac_stream(nch, bits, None, seed)[0]
        assert len(frames) == len(BLOCKS) and all(frames[i][1] == good[i][1] for i in range(len(BLOCKS)) if i != damage) and frames[damage][1] != good[damage][1]
    pcm = [le_bytes(b, bits) for b in blocks_np]
    for p, ch in zip(pcm, blocks):  # (the two short blocks: the long one's bytes are made the same way)
        assert len(ch[0]) > 192 or p == FM.contract_bytes({"bits_per_sample": bits, "block_size": len(ch[0])}, ch)
    return frames, pcm


def flac_table():
    """-> [(channels, bits, (conversion name, out_rate, out_bits, out_channels))]: 3 ... 8 channels at 16 and 24 bits"""
    return [(nch, bits, conversion_of(nch + (2 if bits == 24 else 0), nch, bits)) for bits in (16, 24) for nch in range(3, 9)]


def test_flac_sources_decode_in_the_model():
    table = flac_table()
    assert len(table) == 12 and {t[2][0] for t in table if t[0] == 6} == {"downmix to 2", "depth only"}
    for name, _, _ in CONVERSIONS:
        assert sum(t[2][0] == name for t in table) == 3
    for nch, bits, _ in table:
        frames, pcm = flac_stream(nch, bits)
        assert [d["block_size"] for d, _ in frames] == BLOCKS and [len(p) for p in pcm] == [n * nch * bits // 8 for n in BLOCKS]
    flac_stream(6, 16, 1)
    scheduler_sources()


def pcm_fmt(bits, is_float=False):
    import soundkit_amd.engine as E
    return E.FMT_F32LE if is_float else {16: E.FMT_S16LE, 24: E.FMT_S24LE, 32: E.FMT_S32LE}[bits]


def flac_ticks(engine, kind, table, units_of, deals):
    """the streams of `table` through tick_run_flac (kind "flac", units: frames) or tick_run_pcm (kind "pcm", units: the decoded PCM),
    their units dealt out as `deals` says (per tick, how many every stream gets), then a tick that flushes the resamplers
    -> the records' (frames, channels, bits, bytes) per stream"""
    sids, entries = [], []
    for nch, bits, (_, out_rate, out_bits, out_ch) in table:
        entry = {"channels": nch, "out_bits": out_bits, "out_channels": out_ch}
        entry.update({"bits_per_sample": bits} if kind == "flac" else {"format": pcm_fmt(bits)})
        sid = None
        if out_rate:
            sid = engine.open_stream(RATE, nch)
            engine.resampler_open(sid, RATE, out_rate)
            entry.update(stream=sid, resample=1)
        sids.append(sid)
        entries.append(entry)
    out, at = [[] for _ in table], [0] * len(table)
    try:
        for tick in range(len(deals[0]) + 1):
            units = []
            for i, entry in enumerate(entries):
                n = 0 if tick == len(deals[0]) else deals[i][tick]
                entry.update(n_units=n, flush=1 if tick == len(deals[0]) and sids[i] is not None else 0)
                units += units_of[i][at[i]:at[i] + n]
                at[i] += n
            if kind == "flac":
                recs, status = engine.tick_run_flac(entries, units)
                assert not any(status)
            else:
                recs = engine.tick_run_pcm(entries, units)
            for r in recs:
                assert r[1] == 0 and not r[6]
                out[r[0]].append(r[2:6])
    finally:
        for sid in sids:
            if sid is not None:
                engine.resampler_close(sid)
                engine.close_stream(sid)
    assert at == [len(u) for u in units_of]
    return out


def check_outputs(got, want, table, frames_in, label):
    for k, (nch, bits, (name, out_rate, out_bits, out_ch)) in enumerate(table):
        what = (label, nch, bits, name)
        assert want[k] and all((r[1], r[2]) == (out_ch, out_bits) and len(r[3]) == r[0] * out_ch * out_bits // 8 for r in want[k]), what
        frames = sum(r[0] for r in want[k])
        if out_rate:  # the resampler's chunks: the same whatever the deal, and about a third of the frames
            assert 0.9 * frames_in * out_rate / RATE < frames < 1.1 * frames_in * out_rate / RATE + 300, what
            assert b"".join(r[3] for r in got[k]) == b"".join(r[3] for r in want[k]), what
        else:
            assert frames == frames_in, what
        assert got[k] == want[k], what
        assert any(b"".join(r[3] for r in want[k])), what


@gpu
def test_flac_of_3_to_8_channels_behind_a_conversion_equals_the_pcm_tick(wide):
    table = flac_table()
    built = [flac_stream(nch, bits) for nch, bits, _ in table]
    frames, pcm = [b[0] for b in built], [b[1] for b in built]
    one_tick = [DEALS[0]] * len(table)
    want = flac_ticks(wide, "pcm", table, pcm, one_tick)
    check_outputs(flac_ticks(wide, "flac", table, frames, one_tick), want, table, sum(BLOCKS), "one tick")
    # dealt out another way: the resampled streams' chunks do not move; the others get one record per frame either way
    dealt = [DEALS[1] if i % 2 == 0 else [2, 1, 0] for i in range(len(table))]
    check_outputs(flac_ticks(wide, "flac", table, frames, dealt), want, table, sum(BLOCKS), "three ticks")


@gpu
def test_flac_tables_without_the_pool_are_refused_and_decode_only_streams_deliver(engine):
    import soundkit_amd
    table = flac_table()
    stereo, stereo_pcm = flac_stream(2, 16)
    whole, units = [], []
    for nch, bits, (name, out_rate, out_bits, out_ch) in table:
        frames, _ = flac_stream(nch, bits)
        entry = {"channels": nch, "bits_per_sample": bits, "out_bits": out_bits, "out_channels": out_ch, "n_units": 3}
        if out_rate:
            entry.update(stream=0, resample=1)  # (no such stream can be opened here: the channel count is refused before it is looked at)
        with pytest.raises(soundkit_amd.SoundkitError) as exc:
            engine.tick_run_flac([entry], frames)
        assert exc.value.status == -6, (nch, bits, name)
        whole.append(entry)
        units += frames
    with pytest.raises(soundkit_amd.SoundkitError) as exc:
        engine.tick_run_flac(whole, units)
    assert exc.value.status == -6
    # one such stream behind streams that are fine: the whole tick is refused
    fine = {"channels": 2, "bits_per_sample": 16, "out_bits": 16, "out_channels": 1, "n_units": 3}
    with pytest.raises(soundkit_amd.SoundkitError) as exc:
        engine.tick_run_flac([fine, whole[0]], stereo + flac_stream(table[0][0], table[0][1])[0])
    assert exc.value.status == -6
    # with nothing to change, every channel count from 3 to 8 delivers the decoded bytes, one record per frame
    entries, units, want = [], [], []
    for i, (nch, bits, _) in enumerate(table):
        frames, pcm = flac_stream(nch, bits)
        entries.append({"channels": nch, "bits_per_sample": bits, "out_bits": bits, "out_channels": nch, "n_units": 3})
        units += frames
        want += [(i, 0, n, nch, bits, p, False) for n, p in zip(BLOCKS, pcm)]
    recs, status = engine.tick_run_flac(entries + [fine], units + stereo)
    assert status == [0] * (len(units) + 3) and recs[:len(want)] == want and len(recs) == len(want) + 3


@gpu
def test_a_rejected_frame_in_a_6_channel_stream_behind_a_downmix(wide):
    damaged, _ = flac_stream(6, 16, 1)
    good, pcm = flac_stream(6, 16, None, 2)
    entry = {"channels": 6, "bits_per_sample": 16, "out_bits": 16, "out_channels": 2, "n_units": 3}
    recs, status = wide.tick_run_flac([entry, entry, dict(entry, out_channels=6)], damaged + good + damaged)
    assert status == [0, -506, 0, 0, 0, 0, 0, -506, 0]
    assert [(r[0], r[1]) for r in recs] == [(0, -506)] * 3 + [(1, 0)] * 3 + [(2, 0), (2, -506), (2, 0)]
    want = wide.tick_run_pcm([{"format": pcm_fmt(16), "channels": 6, "out_bits": 16, "out_channels": 2, "n_units": 3}], pcm)
    assert len(want) == 3 and [r[2:] for r in recs[3:6]] == [r[2:] for r in want]
    first = flac_stream(6, 16)[1]
    assert recs[6][5] == first[0] and recs[8][5] == first[2]  # as decoded, the frames beside the rejected one are the source's


# ---- AIFF ---------------------------------------------------------------------------------------------------------------------------

AIFF_ENCODINGS = [AM.S16BE, AM.S24BE, AM.F32BE]


@functools.lru_cache(maxsize=None)
def aiff_stream(enc, nch):
    """-> (source units, the model's decoded PCM per unit), the decode asserted equal to the source samples"""
    bits, is_float = AM.contract(enc)
    units, pcm = [], []
    for i, n in enumerate(BLOCKS):
        v = source(100 + i, nch, n, 24 if is_float else bits)
        if is_float:
            f = (v / float(1 << 23)).astype(np.float32)  # exact: 24-bit integers over 2^23
            assert float(np.abs(f).max()) == 1.0
            src, want = f.astype(">f4").tobytes(), f.astype("<f4").tobytes()
        elif bits == 16:
            src, want = v.astype(">i2").tobytes(), le_bytes(v, 16)
        else:
            want = le_bytes(v, 24)
            src = np.frombuffer(want, np.uint8).reshape(-1, 3)[:, ::-1].tobytes()
        got = AM.decode(enc, nch, src)
        assert got == want and len(got) == n * nch * bits // 8
        units.append(src)
        pcm.append(got)
    return units, pcm


def aiff_table():
    """-> [(encoding, channels, rate, out_rate, out_bits, out_channels)] in test_aiff_tick_gpu.run_ticks' form, and the conversions' names"""
    table, names = [], []
    for e, enc in enumerate(AIFF_ENCODINGS):
        for c, nch in enumerate((3, 6, 8)):
            bits, is_float = AM.contract(enc)
            name, out_rate, out_bits, out_ch = conversion_of(e + c + (1 if e == 2 else 0), nch, bits, is_float)
            table.append((enc, nch, RATE, out_rate, 16 if is_float and name == "depth only" else out_bits, out_ch))
            names.append(name)
    return table, names


def test_aiff_sources_decode_in_the_model():
    table, names = aiff_table()
    assert len(table) == 9 and set(names) == {c[0] for c in CONVERSIONS}
    for enc, nch, *_ in table:
        units, pcm = aiff_stream(enc, nch)
        assert len(units) == 3 and len(pcm) == 3
    for nch in range(3, 9):
        aiff_stream(AM.S16BE, nch)


@gpu
def test_aiff_of_3_6_and_8_channels_behind_a_conversion_equals_the_pcm_tick(wide):
    from test_aiff_tick_gpu import run_ticks
    table, names = aiff_table()
    built = [aiff_stream(t[0], t[1]) for t in table]
    units, pcm = [b[0] for b in built], [b[1] for b in built]
    want, _ = run_ticks(wide, "pcm", table, pcm, [[3] * len(table)])
    for k, (enc, nch, rate, out_rate, out_bits, out_ch) in enumerate(table):
        frames = len(want[k]) // (out_bits // 8 * out_ch)
        if out_rate:
            assert 0.9 * sum(BLOCKS) / 3 < frames < 1.1 * sum(BLOCKS) / 3 + 300, table[k]
        else:
            assert frames == sum(BLOCKS), table[k]
        assert any(want[k])
    ways = {"one tick": [[3] * len(table)],
            "three ticks": [[DEALS[1][t] if i % 2 == 0 else [2, 1, 0][t] for i in range(len(table))] for t in range(3)]}
    for way, deals in ways.items():
        got, _ = run_ticks(wide, "aiff", table, units, deals)
        for k, t in enumerate(table):
            assert got[k] == want[k], (way, AM.NAMES[t[0]], t[1], names[k])


@gpu
def test_aiff_tables_without_the_pool_are_refused_and_decode_only_streams_deliver(engine):
    import soundkit_amd
    table, names = aiff_table()
    whole, units = [], []
    for (enc, nch, rate, out_rate, out_bits, out_ch), name in zip(table, names):
        entry = {"encoding": enc, "channels": nch, "out_bits": out_bits, "out_channels": out_ch, "n_units": 3}
        if out_rate:
            entry.update(stream=0, resample=1)
        with pytest.raises(soundkit_amd.SoundkitError) as exc:
            engine.tick_run_aiff([entry], aiff_stream(enc, nch)[0])
        assert exc.value.status == -6, (AM.NAMES[enc], nch, name)
        whole.append(entry)
        units += aiff_stream(enc, nch)[0]
    with pytest.raises(soundkit_amd.SoundkitError) as exc:
        engine.tick_run_aiff(whole, units)
    assert exc.value.status == -6
    entries, units, want = [], [], []
    cases = [(AM.S16BE, nch) for nch in range(3, 9)] + [(enc, nch) for enc in (AM.S24BE, AM.F32BE) for nch in (3, 6, 8)]
    for i, (enc, nch) in enumerate(cases):
        bits, is_float = AM.contract(enc)
        src, pcm = aiff_stream(enc, nch)
        entries.append({"encoding": enc, "channels": nch, "out_bits": bits, "out_channels": nch, "n_units": 3})
        units += src
        want += [(i, 0, n, nch, bits, p, is_float) for n, p in zip(BLOCKS, pcm)]
    assert engine.tick_run_aiff(entries, units) == want


# ---- the scheduler ------------------------------------------------------------------------------------------------------------------

SCHED_BLOCKS = [1152, 4096, 192, 17, 4100]
TEXT = "Decoding failed: conversion of PCM with more than 2 channels is not supported"


@functools.lru_cache(maxsize=None)
def scheduler_sources():
    """the same 9557 frames of 5.1 as a FLAC stream, as an AIFF stream and decoded -> (flac bytes, aiff bytes, the decoded PCM)"""
    blocks_np = [source(500 + i, 6, n, 16) for i, n in enumerate(SCHED_BLOCKS)]
    blocks = [[[int(x) for x in b[:, c]] for c in range(6)] for b in blocks_np]
    flac, _ = FB.stream(blocks, 16, RATE, lambda i, ch: [KINDS[(i + c) % 3] for c in range(6)])
    pcm = b"".join(le_bytes(b, 16) for b in blocks_np)
    info, frames = FM.decode_stream(flac)
    assert (info["sample_rate"], info["channels"], info["bits_per_sample"]) == (RATE, 6, 16)
    assert b"".join(FM.contract_bytes(h, ch) for h, ch in frames) == pcm
    sound = np.concatenate(blocks_np).astype(">i2").tobytes()
    aiff = AB.simple(None, 6, 16, float(RATE), sound, frames=sum(SCHED_BLOCKS))
    outs, _ = AM.decode_file(aiff)
    assert len(aiff) == 54 + len(sound) and b"".join(o.data for o in outs) == pcm and outs[0][:4] == (RATE, 6, 16, False)
    return flac, aiff, pcm


def cut(data, n):
    return [data[at:at + n] for at in range(0, len(data), n)]


def run(engine, streams):
    """streams: (kind, DecodeOptions, chunks), kind = "auto" (spawn), "aiff" (spawn_aiff) or a RawPcmFormat -> per stream its outputs.
    The feeder is the FLAC scheduler test's: a stream that has ended with an error takes no more, and the others go on."""
    import threading

    from soundkit_amd import pipeline
    from test_flac_scheduler_gpu import feed
    from test_pcm_pipeline_gpu import drain
    sched = pipeline.BatchScheduler(engine, entropy_threads=4, max_streams=len(streams) + 4, lanes=1)
    try:
        handles = [sched.spawn(opt) if kind == "auto" else sched.spawn_aiff(opt) if kind == "aiff" else sched.spawn_raw_pcm(kind, opt)
                   for kind, opt, _ in streams]
        feeder = threading.Thread(target=feed, args=(handles, [c for _, _, c in streams]))
        feeder.start()
        outs = drain(handles, deadline_s=30)
        feeder.join()
        for h in handles:
            h.cancel()
    finally:
        sched.close()
    return outs


@gpu
def test_5_1_flac_and_6_channel_aiff_through_the_scheduler_equal_a_raw_pcm_stream(wide):
    from soundkit_amd import pipeline
    from soundkit_amd import engine as E
    from test_pcm_pipeline_gpu import as_model
    flac, aiff, pcm = scheduler_sources()
    opt = pipeline.DecodeOptions(16, 16000, 2)
    # AIFF sends must end on frames: a send that ends inside one is refused as the reference refuses it, and 1 KiB is no multiple of
    # the 12-byte frame -- so 85 frames (1020 bytes) a piece here, and the 1 KiB pieces beside it, with the reference's answer
    on_frames = [aiff[:54 + 1020]] + cut(aiff[54 + 1020:], 1020)
    outs = [as_model(o) for o in run(wide, [("auto", opt, cut(flac, 1024)), ("aiff", opt, on_frames),
                                            (pipeline.RawPcmFormat(RATE, 6, E.FMT_S16LE), opt, cut(pcm, 1020)), ("aiff", opt, cut(aiff, 1024))])]
    (got_flac, e1), (got_aiff, e2), (raw, e3), (_, e4) = outs
    assert e1 is None and e2 is None and e3 is None and raw
    want = b"".join(r[5] for r in raw)
    assert {r[:5] for r in raw} == {(16, 2, 16000, False, False)} and len(want) // 4 > 3000 and any(want)
    for got in (got_flac, got_aiff):
        assert {g[:5] for g in got} == {(16, 2, 16000, False, False)}
        assert b"".join(g[5] for g in got) == want
    assert e4 == "Decoding failed: Output conversion failed: PCM data is unsupported or contains a partial frame"


@gpu
def test_5_1_flac_without_the_pool_ends_alone_with_the_references_text(engine):
    from soundkit_amd import pipeline
    from test_pcm_pipeline_gpu import as_model
    flac, _, pcm = scheduler_sources()
    rng = random.Random(7)
    blocks = [[[rng.randrange(-20000, 20000) for _ in range(n)] for _ in range(2)] for n in (1152, 300, 1152)]
    stereo, _ = FB.stream(blocks, 16, 44100, lambda i, ch: [KINDS[(i + c) % 3] for c in range(2)], assignment=10)
    stereo_pcm = [FM.contract_bytes(h, ch) for h, ch in FM.decode_stream(stereo)[1]]
    assert stereo_pcm == [FM.contract_bytes({"bits_per_sample": 16, "block_size": len(ch[0])}, ch) for ch in blocks]
    outs = run(engine, [("auto", pipeline.DecodeOptions(16, 16000, 2), cut(flac, 1024)), ("auto", pipeline.DecodeOptions(), cut(stereo, 1024)),
                        ("auto", pipeline.DecodeOptions(), cut(flac, 1024))])
    got, err = as_model(outs[0])
    assert got == [] and err == TEXT and outs[0][-1].status == -6
    got, err = as_model(outs[1])
    assert err is None and [g[5] for g in got] == stereo_pcm and all(g[:5] == (16, 2, 44100, False, False) for g in got)
    got, err = as_model(outs[2])  # ... and as decoded the 5.1 stream itself is taken
    assert err is None and b"".join(g[5] for g in got) == pcm and all(g[:5] == (16, 6, RATE, False, False) for g in got)

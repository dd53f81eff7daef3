"""The tick of the WAV ADPCM streams (sk_tick_run_wav_adpcm through Engine.tick_run_wav_adpcm): every unit decoded on the device, then
what sk_tick_run_pcm runs on an s16le source.  Checked against the PCM tick on the model's decode (tests/wav_adpcm_model.py), bit for
bit, however the blocks are split into units and dealt over ticks; the fact cap inside a block, on a block edge and past the end; a
refused tick; a bad block; and, as the PCM tick's own tests do, against the CPU chain (tests/pcm_worker_model.py OutputStage): exact
without a rate change, within test_pcm_pipeline_gpu.lsb_check's bound through the resampler."""
import numpy as np
import pytest

import wav_adpcm_model as M
from pcm_worker_model import OutputStage

gpu = pytest.mark.gpu
IMA, MS = M.TAG_IMA, M.TAG_MS
FMT_S16LE = 0
COEF3 = [(256, 0), (460, -208), (392, -232)]


def speech_like(rng, frames, ch):
    t = np.arange(frames)[:, None]
    x = 9000 * np.sin(2 * np.pi * t * (np.array([170.0, 233.0])[:ch] / 8000)) + rng.normal(0, 600, (frames, ch))
    return np.clip(x, -32768, 32767).astype(np.int16)


# (tag, channels, block_align, blocks, coef, rate, out_rate, out_bits, out_channels)
TABLE = [(IMA, 1, 256, 21, None, 8000, 16000, 16, 1),
         (MS, 1, 256, 21, M.MS_COEF, 8000, 16000, 16, 1),
         (IMA, 2, 64, 40, None, 44100, None, 16, 2),      # nothing to change: the decoded bytes are the outputs
         (MS, 2, 39, 50, COEF3, 8000, None, 24, 2),
         (IMA, 1, 36, 70, None, 8000, None, 24, 1),
         (MS, 2, 128, 30, M.MS_COEF, 44100, 16000, 16, 1),
         (MS, 1, 7, 9, M.MS_COEF, 8000, None, 16, 1)]      # two frames a block, as decoded


def plain(k):
    return TABLE[k][6] is None and TABLE[k][7] == 16 and TABLE[k][8] == TABLE[k][1]


def build(k):
    tag, ch, align, blocks = TABLE[k][:4]
    rng = np.random.default_rng(100 + k)
    pcm = speech_like(rng, M.block_frames(tag, ch, align) * blocks, ch)
    data = M.ima_encode(pcm, align) if tag == IMA else M.ms_encode(pcm, align, TABLE[k][4])
    assert len(data) == blocks * align
    return data


def units_of(data, align, sizes):
    """the stream's blocks as units of `sizes` blocks, the last one taking the rest"""
    out, at = [], 0
    for n in sizes:
        out.append(data[at:at + n * align])
        at += n * align
    if at < len(data):
        out.append(data[at:])
    return [u for u in out if u]


def model_units(k, units, cap=None):
    """the model's s16 of every unit, cut to the cap"""
    tag, ch, align = TABLE[k][:3]
    out, left = [], cap
    for u in units:
        pcm = M.decode(tag, ch, align, u, TABLE[k][4])[0].astype("<i2").tobytes()
        if left is not None:
            pcm = pcm[:left * ch * 2]
            left -= len(pcm) // (ch * 2)
        out.append(pcm)
    return out


def run_ticks(engine, kind, rows, units, deals, caps=None):
    """rows: indices into TABLE; units[i]: the stream's units ("wav": blocks; "pcm": s16); deals: per tick how many units each stream
    gets, then a tick that takes the rest and flushes the resamplers -> (bytes per stream, [records per stream], frames_left per stream)"""
    sids, entries = [], []
    for i, k in enumerate(rows):
        tag, ch, align, _, coef, rate, out_rate, out_bits, out_ch = TABLE[k]
        entry = {"channels": ch, "out_bits": out_bits, "out_channels": out_ch}
        if kind == "wav":
            entry.update(tag=tag, block_align=align, coef=coef, frames_left=None if caps is None else caps[i])
        else:
            entry["format"] = FMT_S16LE
        sid = None
        if out_rate is not None:
            sid = engine.open_stream(rate, ch)
            engine.resampler_open(sid, rate, out_rate)
            entry.update(stream=sid, resample=1)
        sids.append(sid)
        entries.append(entry)
    out, recs_of, at = [b""] * len(rows), [[] for _ in rows], [0] * len(rows)
    try:
        for deal in list(deals) + [None]:
            # (the PCM tick has no place for a stream with nothing to change: that is the caller's fast path)
            batch, live = [], [i for i, k in enumerate(rows) if kind == "wav" or not plain(k)]
            for i in live:
                entry = entries[i]
                n = len(units[i]) - at[i] if deal is None else min(deal[i], len(units[i]) - at[i])
                entry["n_units"] = n
                entry["flush"] = 1 if deal is None and sids[i] is not None else 0
                batch += units[i][at[i]:at[i] + n]
                at[i] += n
            if kind == "wav":
                recs, status = engine.tick_run_wav_adpcm([entries[i] for i in live], batch)
                assert not any(status)
            else:
                recs = engine.tick_run_pcm([entries[i] for i in live], batch) if live else []
            for r in recs:
                i = live[r[0]]
                assert r[1] == 0 and (r[3], r[4]) == (TABLE[rows[i]][8], TABLE[rows[i]][7])
                out[i] += r[5]
                recs_of[i].append((r[2], len(r[5])))
    finally:
        for sid in sids:
            if sid is not None:
                engine.resampler_close(sid)
                engine.close_stream(sid)
    return out, recs_of, [e.get("frames_left") for e in entries]


SPLITS = {"one block a unit": lambda n: [1] * n, "1 + rest": lambda n: [1], "all at once": lambda n: [n], "ragged": lambda n: [2, 1, 5, 3, 1]}
DEALS = {"all at once": lambda n: [], "one per tick": lambda n: [[1]] * n, "1 + rest": lambda n: [[1]]}


@gpu
@pytest.mark.parametrize("k", [0, 1, 3, 4, 5], ids=lambda k: "row%d" % k)
def test_a_converted_stream_is_the_pcm_tick_on_the_models_decode_whatever_the_deal(engine, k):
    """streams behind a conversion: the bytes do not depend on how the blocks are split into units or dealt over ticks, and they are
    what sk_tick_run_pcm gives on the model's s16"""
    data, align = build(k), TABLE[k][2]
    whole = [data]
    want, _, _ = run_ticks(engine, "pcm", [k], [model_units(k, whole)], [])
    assert any(want[0])
    for split, sizes in SPLITS.items():
        units = units_of(data, align, sizes(len(data) // align))
        for deal, of in DEALS.items():
            got, _, left = run_ticks(engine, "wav", [k], [units], of(len(units)))
            assert got[0] == want[0], (split, deal)
            assert left == [None]


@gpu
@pytest.mark.parametrize("k", [2, 6], ids=lambda k: "row%d" % k)
def test_a_stream_with_nothing_to_change_gets_the_models_decode_one_record_per_unit(engine, k):
    data, (tag, ch, align) = build(k), TABLE[k][:3]
    for split, sizes in SPLITS.items():
        units = units_of(data, align, sizes(len(data) // align))
        want = model_units(k, units)
        for deal, of in DEALS.items():
            got, recs, _ = run_ticks(engine, "wav", [k], [units], of(len(units)))
            assert got[0] == b"".join(want), (split, deal)
            assert recs[0] == [(len(w) // (2 * ch), len(w)) for w in want], (split, deal)


@gpu
def test_all_rows_side_by_side_in_the_same_ticks(engine):
    rows = list(range(len(TABLE)))
    datas = [build(k) for k in rows]
    units = [units_of(d, TABLE[k][2], [3, 1, 2]) for k, d in zip(rows, datas)]
    want, want_recs, _ = run_ticks(engine, "pcm", rows, [model_units(k, u) for k, u in zip(rows, units)], [[2] * len(rows), [1] * len(rows)])
    got, recs, _ = run_ticks(engine, "wav", rows, units, [[2] * len(rows), [1] * len(rows)])
    for k in rows:
        if plain(k):
            assert got[k] == b"".join(model_units(k, units[k]))
        else:
            assert got[k] == want[k] and recs[k] == want_recs[k], TABLE[k]


@gpu
@pytest.mark.parametrize("k", [0, 2, 3, 6], ids=lambda k: "row%d" % k)
def test_the_fact_cap(engine, k):
    """frames_left inside a block, on a block edge, in a unit's first block, and past the end (no cut): the frames behind the cap are
    not there, frames_left goes down by what was given"""
    data, (tag, ch, align, blocks) = build(k), TABLE[k][:4]
    per = M.block_frames(tag, ch, align)
    for cap in (per * blocks - 1, per * (blocks - 1), per * (blocks - 1) + 1, per * blocks, per * blocks + 5, per + 1):
        # units of two blocks, as many blocks as hold `cap` frames: a stream brings no unit behind its cap
        n_blocks = min(blocks, -(-cap // per))
        live = units_of(data[:n_blocks * align], align, [2] * (n_blocks // 2))
        want_pcm = model_units(k, live, cap)
        assert sum(len(w) for w in want_pcm) == min(cap, per * blocks) * ch * 2 and all(want_pcm)
        got, recs, left = run_ticks(engine, "wav", [k], [live], [[1]], caps=[cap])
        if plain(k):
            assert got[0] == b"".join(want_pcm), cap
            assert [r[1] for r in recs[0]] == [len(w) for w in want_pcm]
        else:
            want, _, _ = run_ticks(engine, "pcm", [k], [want_pcm], [[1]])
            assert got[0] == want[0], cap
        assert left == [cap - min(cap, per * blocks)]


@gpu
def test_a_stream_whose_cap_is_used_up_brings_no_more_units(engine):
    from soundkit_amd._lib import SoundkitError
    k = 2
    data, align = build(k), TABLE[k][2]
    entry = {"tag": IMA, "channels": 2, "block_align": align, "out_bits": 16, "out_channels": 2, "n_units": 2, "frames_left": 57}
    with pytest.raises(SoundkitError):
        engine.tick_run_wav_adpcm([entry], [data[:align], data[align:2 * align]])  # 57 frames are the first block's
    assert entry["frames_left"] == 57
    for bad in ({"tag": 1}, {"channels": 3}, {"block_align": 63}, {"out_bits": 8}, {"tag": MS, "block_align": 64, "coef": []}):
        with pytest.raises(SoundkitError):
            engine.tick_run_wav_adpcm([dict(entry, frames_left=None, n_units=1, **bad)], [data[:64]])
    assert engine.tick_run_wav_adpcm([], []) == ([], [])


@gpu
@pytest.mark.parametrize("k", [0, 5], ids=lambda k: "row%d" % k)
def test_a_refused_tick_leaves_frames_left_and_the_resampler_as_they_were(engine, k):
    from soundkit_amd._lib import SoundkitError
    tag, ch, align, blocks, coef, rate, out_rate, out_bits, out_ch = TABLE[k]
    data = build(k)
    units = units_of(data, align, [blocks // 2])
    cap = M.block_frames(tag, ch, align) * blocks - 3
    outs = []
    for refuse in (False, True):
        sid = engine.open_stream(rate, ch)
        engine.resampler_open(sid, rate, out_rate)
        entry = {"tag": tag, "channels": ch, "block_align": align, "coef": coef, "out_bits": out_bits, "out_channels": out_ch, "stream": sid, "resample": 1,
                 "frames_left": cap}
        try:
            got = b""
            for t, u in enumerate(units):
                entry.update(n_units=1, flush=int(t == len(units) - 1))
                if refuse and t == 1:
                    before = entry["frames_left"]
                    with pytest.raises(SoundkitError):
                        engine.tick_run_wav_adpcm([entry], [u], out_cap=64)
                    assert entry["frames_left"] == before
                recs, status = engine.tick_run_wav_adpcm([entry], [u])
                assert status == [0] and all(r[1] == 0 for r in recs)
                got += b"".join(r[5] for r in recs)
            assert entry["frames_left"] == 0
            outs.append(got)
        finally:
            engine.resampler_close(sid)
            engine.close_stream(sid)
    assert outs[0] == outs[1] and any(outs[0])


@gpu
def test_a_bad_block_marks_its_unit_and_leaves_the_other_streams_alone(engine):
    """one invalid block of each kind: its unit's status names it, the records of its unit (as decoded) or of its stream in this tick
    (behind a conversion) carry SK_WAV_BAD_BLOCK, and the streams beside it are what they are without it"""
    rows = [2, 3, 4, 6]
    datas = [bytearray(build(k)) for k in rows]
    clean = [bytes(d) for d in datas]
    datas[0][2 * 64 + 4 + 2] = 89       # row 2: IMA stereo, block 2, the right channel's step index
    datas[1][5 * 39 + 0] = 3            # row 3: MS with three sets, block 5, the left channel's predictor
    units = [units_of(bytes(d), TABLE[k][2], [2, 2, 2]) for k, d in zip(rows, datas)]
    entries = []
    for k, u in zip(rows, units):
        tag, ch, align, _, coef, _, _, out_bits, out_ch = TABLE[k]
        entries.append({"tag": tag, "channels": ch, "block_align": align, "coef": coef, "out_bits": out_bits, "out_channels": out_ch, "n_units": len(u)})
    recs, status = engine.tick_run_wav_adpcm(entries, [x for u in units for x in u])
    assert status == [0, 1, 0, 0] + [0, 0, 2, 0] + [0] * 8
    by_stream = [[r for r in recs if r[0] == i] for i in range(4)]
    assert [r[1] for r in by_stream[0]] == [0, M.BAD_BLOCK, 0, 0]          # as decoded: the unit's own record
    assert all(r[1] == M.BAD_BLOCK for r in by_stream[1]) and by_stream[1]  # behind a conversion: every record of the stream
    assert [r[5] for r in by_stream[0]] == model_units(2, units[0])
    bad = np.frombuffer(by_stream[0][1][5], "<i2").reshape(2, 57, 2)
    assert not bad[0].any() and bad[1].any()  # block 2 is zeros, block 3 beside it in the same unit is not
    ref, _ = engine.tick_run_wav_adpcm([dict(e) for e in entries[2:]], [x for k, c in zip(rows[2:], clean[2:]) for x in units_of(c, TABLE[k][2], [2, 2, 2])])
    assert [r[1:] for r in by_stream[2]] == [r[1:] for r in ref if r[0] == 0] and [r[1:] for r in by_stream[3]] == [r[1:] for r in ref if r[0] == 1]


def lsb_check(mine, want, label):
    """tests/test_pcm_pipeline_gpu.py lsb_check, the PCM tick's bound through the resampler: one step, on at most 1 % of the samples"""
    mine, want = np.frombuffer(mine, "<i2").astype(np.int32), np.frombuffer(want, "<i2").astype(np.int32)
    assert mine.size == want.size, (label, mine.size, want.size)
    d = np.abs(mine - want)
    print("\n%s: worst |d| %d, share of samples off by one %.5f of %d" % (label, d.max(), (d > 0).mean(), d.size))
    assert d.max() <= 1 and (d > 0).mean() <= 0.01, (label, int(d.max()), float((d > 0).mean()))


@gpu
@pytest.mark.parametrize("k", [0, 1, 3, 4], ids=lambda k: "row%d" % k)
def test_against_the_cpu_chain_on_the_models_s16(engine, oracle, k):
    """8 -> 16 kHz mono s16 (rows 0, 1) and a 24-bit output (rows 3, 4): the oracle and the tolerance of the PCM tick's own tests"""
    tag, ch, align, blocks, coef, rate, out_rate, out_bits, out_ch = TABLE[k]
    data = build(k)
    units = units_of(data, align, [5, 4, 7])
    got, recs, _ = run_ticks(engine, "wav", [k], [units], [[1], [2]])
    stage = OutputStage(oracle, rate, ch, 16, False, False, out_bits, out_rate, out_ch)
    cpu = [o for u in model_units(k, units) for o in stage.piece(u)] + stage.flush()
    assert all(o[:3] == (out_bits, out_ch, out_rate or rate) for o in cpu)
    assert [n for _, n in recs[0]] == [len(o[5]) for o in cpu]
    want = b"".join(o[5] for o in cpu)
    if out_rate is None:
        assert got[0] == want
    else:
        lsb_check(got[0], want, "row %d" % k)

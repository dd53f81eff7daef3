"""Telephony streams through the tick (sk_tick_run_g72x, Engine.tick_run_g72x).

Expected values are never the code under test: the decoded samples are tests/g72x_model.py's, and whatever stands behind the decode -- a
rate change, a depth or channel change -- is sk_tick_run_pcm fed those samples as s16le units, which the PCM tick's own tests pin to the
CPU chain of tests/pcm_worker_model.py (test_pcm_tick_formats_gpu.py, test_rate_pairs_gpu.py).  That is the comparison
tests/test_aiff_tick_gpu.py makes for its resampled streams, and like there every comparison is bit for bit.

* plain streams: the outputs are the decoded bytes, one per unit;
* 8 -> 16 kHz for G.726 and G.711, G.722 at 16 -> 8 kHz and to 48 kHz, 24-bit output, stereo G.711 to mono (with and without a rate change);
* the units dealt out over ticks in several ways: the carries and the resamplers go out of one launch and into the next;
* refused ticks leave the carries and the resamplers as they were."""
import ctypes as C
import functools

import numpy as np
import pytest

import g72x_model as M

gpu = pytest.mark.gpu

UNIT_SAMPLES = [2, 30, 32, 34, 3000, 3400, 1400, 66, 2000, 4, 1022, 514]  # frames per unit, before rounding up to whole groups
DEALS = {"all at once": lambda i: [12],
         "one unit a tick": lambda i: [1] * 12,
         "uneven": lambda i: [[5, 0, 0, 6, 1], [0, 1, 10, 0, 1], [2, 7, 0, 0, 3]][i % 3],
         "uneven, the other way": lambda i: [[0, 0, 11, 1], [4, 4, 0, 4], [1, 0, 1, 10]][i % 3]}
# (codec, G.726 rate, packing, channels, rate, out_rate or None, out_bits, out_channels)
TABLE = [(M.G726, 32000, M.LEFT, 1, 8000, 16000, 16, 1),
         (M.G726, 24000, M.RIGHT, 1, 8000, 16000, 16, 1),
         (M.ULAW, 0, 0, 1, 8000, 16000, 16, 1),
         (M.G722, 0, 0, 1, 16000, 8000, 16, 1),
         (M.G722, 0, 0, 1, 16000, 48000, 16, 1),
         (M.G726, 40000, M.LEFT, 1, 8000, None, 24, 1),
         (M.ALAW, 0, 0, 2, 8000, None, 16, 1),
         (M.ALAW, 0, 0, 2, 8000, 16000, 16, 1),
         (M.G726, 16000, M.RIGHT, 1, 8000, 16000, 24, 1),
         # nothing to change behind the decode
         (M.G726, 16000, M.LEFT, 1, 8000, None, 16, 1),
         (M.G726, 40000, M.RIGHT, 1, 8000, None, 16, 1),
         (M.G722, 0, 0, 1, 16000, None, 16, 1),
         (M.ULAW, 0, 0, 2, 8000, None, 16, 2)]
PLAIN = [k for k, t in enumerate(TABLE) if t[5] is None and t[6] == 16 and t[7] == t[3]]


def unit_bytes(codec, rate, channels, frames):
    if codec == M.G726:
        gs, gb = M.G726_GROUP_SAMPLES[rate], M.G726_GROUP_BYTES[rate]
        return (frames + gs - 1) // gs * gb
    return (frames + 1) // 2 if codec == M.G722 else frames * channels


@functools.lru_cache(maxsize=None)
def dealt_streams():
    """-> per stream of TABLE (source units, the model's s16le bytes per unit, the model's final state words or None)"""
    out = []
    for k, (codec, rate, packing, ch, hz, out_hz, out_bits, out_ch) in enumerate(TABLE):
        rng = np.random.default_rng(700 + k)
        units = [rng.integers(0, 256, unit_bytes(codec, rate, ch, f), dtype=np.uint8).tobytes() for f in UNIT_SAMPLES]
        if codec == M.G726:
            dec = M.G726Decoder(rate, packing)
            pcm = [dec.decode(u).astype("<i2").tobytes() for u in units]
            words = dec.core.words()
        elif codec == M.G722:
            dec = M.G722Decoder()
            pcm = [dec.decode(u).astype("<i2").tobytes() for u in units]
            words = dec.words()
        else:
            pcm, words = [M.g711_decode(u, codec).astype("<i2").tobytes() for u in units], None
        frames = sum(len(p) for p in pcm) // (2 * ch)
        assert out_hz is None or frames > 2 * 4096 + 256  # two resampler chunks and a tail for the flush
        out.append((units, pcm, words))
    return out


def test_the_dealt_streams_decode_in_the_model():
    streams = dealt_streams()
    assert len(streams) == len(TABLE) and all(len(u) == 12 and len(p) == 12 for u, p, _ in streams)
    assert len(PLAIN) == 4
    for of in DEALS.values():
        assert all(sum(of(i)) == 12 for i in range(3))


def run_ticks(engine, kind, streams, units_of, deals):
    """every stream's records over the ticks of `deals` (lists of how many units each stream gets per tick), then a tick that takes what is
    left and flushes the resamplers.  kind "g72x": the source units through tick_run_g72x, the carry threaded through the stream dicts;
    kind "pcm": the model's samples through tick_run_pcm.  -> ([record bytes] per stream, final state words per stream)"""
    import soundkit_amd.engine as E
    from soundkit_amd import telephony
    sids, entries = [], []
    for codec, rate, packing, ch, hz, out_hz, out_bits, out_ch in streams:
        entry = {"channels": ch, "out_bits": out_bits, "out_channels": out_ch}
        if kind == "g72x":
            entry.update(codec=codec, rate=rate or 32000, packing=packing, state=telephony.new_state(codec))
        else:
            entry["format"] = E.FMT_S16LE
        sid = None
        if out_hz is not None:
            sid = engine.open_stream(hz, ch)
            engine.resampler_open(sid, hz, out_hz)
            entry.update(stream=sid, resample=1)
        sids.append(sid)
        entries.append(entry)
    out = [[] for _ in streams]
    at = [0] * len(streams)
    try:
        for deal in list(deals) + [None]:
            units = []
            for i, entry in enumerate(entries):
                n = len(units_of[i]) - at[i] if deal is None else deal[i]
                entry["n_units"] = n
                entry["flush"] = 1 if deal is None and sids[i] is not None else 0
                units += units_of[i][at[i]:at[i] + n]
                at[i] += n
            recs = engine.tick_run_g72x(entries, units) if kind == "g72x" else engine.tick_run_pcm(entries, units)
            for r in recs:
                assert r[1] == 0 and (r[3], r[4]) == (streams[r[0]][7], streams[r[0]][6]) and not r[6]
                out[r[0]].append(r[5])
    finally:
        for sid in sids:
            if sid is not None:
                engine.resampler_close(sid)
                engine.close_stream(sid)
    return out, [telephony.state_words(e["state"]) if e.get("state") is not None else None for e in entries]


def deal_of(of, n_streams):
    per = [of(i) for i in range(n_streams)]
    ticks = max(len(p) for p in per)
    return [[p[t] if t < len(p) else 0 for p in per] for t in range(ticks)]


_WANT = {}


def wanted(engine):
    """the PCM tick on the model's samples, all units in one tick: computed once, shared"""
    cache = _WANT
    if "want" not in cache:
        pcm = [b[1] for b in dealt_streams()]
        cache["want"] = run_ticks(engine, "pcm", [t for k, t in enumerate(TABLE) if k not in PLAIN], [p for k, p in enumerate(pcm) if k not in PLAIN],
                                  deal_of(DEALS["all at once"], len(TABLE) - len(PLAIN)))[0]
    full, it = [], iter(cache["want"])
    for k in range(len(TABLE)):
        full.append(None if k in PLAIN else next(it))
    return full


@gpu
def test_plain_streams_get_the_decoded_bytes_one_record_per_unit(engine):
    built = dealt_streams()
    got, states = run_ticks(engine, "g72x", [TABLE[k] for k in PLAIN], [built[k][0] for k in PLAIN], deal_of(DEALS["uneven"], len(PLAIN)))
    for j, k in enumerate(PLAIN):
        assert got[j] == built[k][1], TABLE[k]  # record for record
        assert states[j] == built[k][2], TABLE[k]


@gpu
@pytest.mark.parametrize("name", list(DEALS))
def test_every_deal_gives_the_pcm_tick_on_the_models_samples(engine, name):
    built = dealt_streams()
    want = wanted(engine)
    for k, (codec, rate, packing, ch, hz, out_hz, out_bits, out_ch) in enumerate(TABLE):  # the output is there
        if k in PLAIN:
            continue
        frames_in = sum(len(p) for p in built[k][1]) // (2 * ch)
        frames_out = sum(len(r) for r in want[k]) // (out_bits // 8 * out_ch)
        if out_hz is None:
            assert frames_out == frames_in
        else:
            assert 0.9 * frames_in * out_hz / hz < frames_out < 1.1 * frames_in * out_hz / hz + 300, TABLE[k]
        assert any(b"".join(want[k]))
    got, states = run_ticks(engine, "g72x", TABLE, [b[0] for b in built], deal_of(DEALS[name], len(TABLE)))
    for k, t in enumerate(TABLE):
        if k in PLAIN:
            assert got[k] == built[k][1], (name, t)
        else:
            assert b"".join(got[k]) == b"".join(want[k]), (name, t)
        assert states[k] == built[k][2], (name, t)


# ---- refused ticks ------------------------------------------------------------------------------------------------------------------

def raw_tick(engine, streams, units, out_cap=None, outs_cap=256):
    """sk_tick_run_g72x as Engine.tick_run_g72x calls it, but the status comes back instead of an exception and the caller's records are
    read back whatever the status -> (status, [state words per stream], n_outs, the records' bytes one after the other)"""
    from soundkit_amd import telephony
    from soundkit_amd._lib import G722State, G726State, G72xTickStream, PcmUnit, TickOutput, lib
    ts = (G72xTickStream * max(len(streams), 1))()
    s726, s722 = (G726State * len(streams))(), (G722State * len(streams))()
    for i, s in enumerate(streams):
        ts[i].stream, ts[i].n_units = int(s.get("stream", 0)), int(s["n_units"])
        ts[i].codec, ts[i].channels = int(s["codec"]), int(s.get("channels", 1))
        ts[i].g726_rate, ts[i].g726_packing, ts[i].state = int(s.get("rate", 32000)), int(s.get("packing", 0)), i
        ts[i].out_bits, ts[i].out_channels = int(s["out_bits"]), int(s["out_channels"])
        ts[i].resample, ts[i].flush = int(bool(s.get("resample", 0))), int(bool(s.get("flush", 0)))
        if s["codec"] == M.G726:
            s726[i] = s["state"]
        elif s["codec"] == M.G722:
            s722[i] = s["state"]
    table = (PcmUnit * max(len(units), 1))()
    total = 0
    for k, u in enumerate(units):
        table[k].byte_offset, table[k].byte_len = total, len(u)
        total += (len(u) + 15) & ~15
    blob = np.zeros(max(total, 16), np.uint8)
    for k, u in enumerate(units):
        blob[table[k].byte_offset:table[k].byte_offset + len(u)] = np.frombuffer(bytes(u), np.uint8)
    out = np.zeros(1 << 20 if out_cap is None else max(out_cap, 16), np.uint8)
    recs = (TickOutput * 256)()
    n_out, used = C.c_uint32(77), C.c_size_t(77)
    rc = lib.sk_tick_run_g72x(engine._h, ts, len(streams), table, len(units), blob.ctypes.data, total, out.ctypes.data,
                              out.size if out_cap is None else out_cap, recs, outs_cap, C.byref(n_out), C.byref(used), s726, len(streams), s722, len(streams))
    payload = b"".join(out[r.byte_offset:r.byte_offset + r.bytes].tobytes() for r in recs[:n_out.value])
    words = [telephony.state_words(s726[i]) if s["codec"] == M.G726 else (telephony.state_words(s722[i]) if s["codec"] == M.G722 else None)
             for i, s in enumerate(streams)]
    return rc, words, n_out.value, payload


@gpu
@pytest.mark.parametrize("k", [1, 3], ids=["g726-24 to 16000", "g722 to 8000"])
def test_a_refused_tick_leaves_the_carry_and_the_resampler_as_they_were(engine, k):
    from soundkit_amd import telephony
    codec, rate, packing, ch, hz, out_hz, out_bits, out_ch = TABLE[k]
    units, pcm, final = dealt_streams()[k]
    # the PCM tick on the model's samples, this stream alone as below
    want = b"".join(run_ticks(engine, "pcm", [TABLE[k]], [pcm], [[12]])[0][0])
    sid = engine.open_stream(hz, ch)
    engine.resampler_open(sid, hz, out_hz)
    try:
        entry = {"codec": codec, "rate": rate or 32000, "packing": packing, "channels": ch, "out_bits": out_bits, "out_channels": out_ch, "stream": sid,
                 "resample": 1, "n_units": 5, "state": telephony.new_state(codec)}
        got = engine.tick_run_g72x([entry], units[:5])
        mid = telephony.state_words(entry["state"])
        assert mid != telephony.state_words(telephony.new_state(codec))
        nxt = dict(entry, n_units=2)
        two = np.random.default_rng(5).integers(0, 256, 200, dtype=np.uint8).tobytes()
        ok_neighbour = {"codec": M.ULAW, "channels": 2, "out_bits": 24, "out_channels": 1, "n_units": 1}
        refusals = [  # (label, table, units, output capacity in bytes, in records)
            ("a flush without a resampler", [nxt, dict(ok_neighbour, flush=1)], units[5:7] + [two], None, 256),
            ("a neighbour's depth the PCM body does not take", [nxt, dict(ok_neighbour, out_bits=12)], units[5:7] + [two], None, 256),
            ("a neighbour that is no codec", [nxt, dict(ok_neighbour, codec=9)], units[5:7] + [two], None, 256),
            ("a stereo unit of half a frame behind a conversion", [nxt, ok_neighbour], units[5:7] + [two[:-1]], None, 256),
            ("an empty unit", [nxt], [units[5], b""], None, 256),
            ("an output too small in bytes", [nxt, ok_neighbour], units[5:7] + [two], 64, 256),
            ("an output too small in records", [nxt, ok_neighbour], units[5:7] + [two], None, 1)]
        if codec == M.G726:
            refusals.append(("a unit that is no whole group", [nxt], [units[5], units[6][:-1]], None, 256))
        for label, table, us, cap, outs_cap in refusals:
            rc, words, n_outs, _ = raw_tick(engine, table, us, cap, outs_cap)
            assert rc == -1 and n_outs == 0, label
            assert words[0] == mid, label  # the caller's record keeps the carry it came with
        # the same units sent again give the right answer
        rest = dict(entry, n_units=7, flush=1)
        got += engine.tick_run_g72x([rest], units[5:])
        assert telephony.state_words(rest["state"]) == final
    finally:
        engine.resampler_close(sid)
        engine.close_stream(sid)
    assert all(r[1] == 0 for r in got)
    assert b"".join(r[5] for r in got) == want and len(want) > 2 * 4096  # (16 -> 8 kHz halves the 8 k frames that went in)

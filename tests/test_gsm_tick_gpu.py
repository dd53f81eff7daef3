"""GSM 06.10 streams through the tick (sk_tick_run_gsm, Engine.tick_run_gsm).

Expected values are never the code under test: the decoded samples are tests/gsm_model.py's, and whatever stands behind the decode -- a
rate change, a depth or channel change -- is sk_tick_run_pcm fed those samples as 8 kHz mono s16le units, which the PCM tick's own tests
pin to the CPU chain (test_pcm_tick_formats_gpu.py, test_rate_pairs_gpu.py).  That is the comparison tests/test_g72x_tick_gpu.py makes,
and like there every comparison is bit for bit.

* plain streams: the outputs are the decoded bytes, one per unit;
* 8 -> 16 kHz, 24-bit output, a stereo output asked for (whatever the PCM tick makes of a mono source then), in both framings;
* the units dealt out over ticks in several ways: the carries and the resamplers go out of one launch and into the next;
* refused ticks leave the carries and the resamplers as they were."""
import ctypes as C
import functools

import numpy as np
import pytest

import gsm_model as M

gpu = pytest.mark.gpu

UNIT_FRAMES = [2, 4, 12, 2, 20, 6, 2, 10]  # frames per unit (even: both framings); 58 frames = 9 280 samples, two resampler chunks and a tail
DEALS = {"all at once": lambda i: [8],
         "one unit a tick": lambda i: [1] * 8,
         "uneven": lambda i: [[3, 0, 0, 4, 1], [0, 1, 6, 0, 1], [2, 5, 0, 0, 1]][i % 3],
         "uneven, the other way": lambda i: [[0, 0, 7, 1], [2, 2, 0, 4], [1, 0, 1, 6]][i % 3]}
# (variant, out_rate or None, out_bits, out_channels)
TABLE = [(M.STANDARD, 16000, 16, 1),
         (M.MICROSOFT, 16000, 16, 1),
         (M.STANDARD, None, 24, 1),
         (M.MICROSOFT, None, 16, 2),
         (M.STANDARD, 16000, 24, 2),
         # nothing to change behind the decode
         (M.STANDARD, None, 16, 1),
         (M.MICROSOFT, None, 16, 1)]
PLAIN = [k for k, t in enumerate(TABLE) if t[1] is None and t[2] == 16 and t[3] == 1]


@functools.lru_cache(maxsize=None)
def dealt_streams():
    """-> per stream of TABLE (source units, the model's s16le bytes per unit, the model's final state words)"""
    out = []
    for k, (variant, out_hz, out_bits, out_ch) in enumerate(TABLE):
        core = M.GsmCore()
        units, pcm = [], []
        for j, n in enumerate(UNIT_FRAMES):
            units.append(M.build_stream(M.random_frames(7000 + 16 * k + j, n), variant))
            pcm.append(M.decode_packets(core, units[-1], variant).astype("<i2").tobytes())
        assert sum(len(p) for p in pcm) // 2 > 2 * 4096 + 256
        out.append((units, pcm, core.words()))
    return out


def test_the_dealt_streams_decode_in_the_model():
    streams = dealt_streams()
    assert len(streams) == len(TABLE) and all(len(u) == 8 and len(p) == 8 for u, p, _ in streams)
    assert len(PLAIN) == 2
    for of in DEALS.values():
        assert all(sum(of(i)) == 8 for i in range(3))


def run_ticks(engine, kind, streams, units_of, deals):
    """every stream's records over the ticks of `deals` (lists of how many units each stream gets per tick), then a tick that takes what is
    left and flushes the resamplers.  kind "gsm": the source units through tick_run_gsm, the carry threaded through the stream dicts;
    kind "pcm": the model's samples through tick_run_pcm.  -> ([(channels, bits, record bytes)] per stream, final state words per stream)"""
    import soundkit_amd.engine as E
    from soundkit_amd import telephony
    sids, entries = [], []
    for variant, out_hz, out_bits, out_ch in streams:
        entry = {"channels": 1, "out_bits": out_bits, "out_channels": out_ch}
        if kind == "gsm":
            entry.update(variant=variant, state=telephony.new_state(telephony.GSM))
        else:
            entry["format"] = E.FMT_S16LE
        sid = None
        if out_hz is not None:
            sid = engine.open_stream(8000, 1)
            engine.resampler_open(sid, 8000, out_hz)
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
            recs = engine.tick_run_gsm(entries, units) if kind == "gsm" else engine.tick_run_pcm(entries, units)
            for r in recs:
                assert r[1] == 0 and r[4] == streams[r[0]][2] and not r[6]
                out[r[0]].append((r[3], r[4], r[5]))
    finally:
        for sid in sids:
            if sid is not None:
                engine.resampler_close(sid)
                engine.close_stream(sid)
    return out, [telephony.state_words(e["state"]) if "state" in e else None for e in entries]


def deal_of(of, n_streams):
    per = [of(i) for i in range(n_streams)]
    ticks = max(len(p) for p in per)
    return [[p[t] if t < len(p) else 0 for p in per] for t in range(ticks)]


_WANT = {}


def wanted(engine):
    """the PCM tick on the model's samples, all units in one tick: computed once, shared"""
    if "want" not in _WANT:
        pcm = [b[1] for b in dealt_streams()]
        _WANT["want"] = run_ticks(engine, "pcm", [t for k, t in enumerate(TABLE) if k not in PLAIN], [p for k, p in enumerate(pcm) if k not in PLAIN],
                                  deal_of(DEALS["all at once"], len(TABLE) - len(PLAIN)))[0]
    full, it = [], iter(_WANT["want"])
    for k in range(len(TABLE)):
        full.append(None if k in PLAIN else next(it))
    return full


@gpu
def test_plain_streams_get_the_decoded_bytes_one_record_per_unit(engine):
    built = dealt_streams()
    got, states = run_ticks(engine, "gsm", [TABLE[k] for k in PLAIN], [built[k][0] for k in PLAIN], deal_of(DEALS["uneven"], len(PLAIN)))
    for j, k in enumerate(PLAIN):
        assert got[j] == [(1, 16, p) for p in built[k][1]], TABLE[k]  # record for record
        assert states[j] == built[k][2], TABLE[k]


@gpu
@pytest.mark.parametrize("name", list(DEALS))
def test_every_deal_gives_the_pcm_tick_on_the_models_samples(engine, name):
    built = dealt_streams()
    want = wanted(engine)
    for k, (variant, out_hz, out_bits, out_ch) in enumerate(TABLE):  # the output is there
        if k in PLAIN:
            continue
        frames_in = sum(len(p) for p in built[k][1]) // 2
        assert len({r[:2] for r in want[k]}) == 1  # one shape throughout
        frames_out = sum(len(r[2]) for r in want[k]) // (out_bits // 8 * want[k][0][0])
        if out_hz is None:
            assert frames_out == frames_in
        else:
            assert 0.9 * frames_in * out_hz / 8000 < frames_out < 1.1 * frames_in * out_hz / 8000 + 300, TABLE[k]
        assert any(b"".join(r[2] for r in want[k]))
    got, states = run_ticks(engine, "gsm", TABLE, [b[0] for b in built], deal_of(DEALS[name], len(TABLE)))
    for k, t in enumerate(TABLE):
        if k in PLAIN:
            assert got[k] == [(1, 16, p) for p in built[k][1]], (name, t)
        else:  # the same shape, the same bytes
            assert {r[:2] for r in got[k]} == {r[:2] for r in want[k]} and b"".join(r[2] for r in got[k]) == b"".join(r[2] for r in want[k]), (name, t)
        assert states[k] == built[k][2], (name, t)


# ---- refused ticks ------------------------------------------------------------------------------------------------------------------

def raw_tick(engine, streams, units, out_cap=None, outs_cap=256, n_states=None):
    """sk_tick_run_gsm as Engine.tick_run_gsm calls it, but the status comes back instead of an exception and the caller's records are
    read back whatever the status -> (status, [state words per stream], n_outs)"""
    from soundkit_amd import telephony
    from soundkit_amd._lib import GsmState, GsmTickStream, PcmUnit, TickOutput, lib
    ts = (GsmTickStream * max(len(streams), 1))()
    states = (GsmState * len(streams))()
    for i, s in enumerate(streams):
        ts[i].stream, ts[i].n_units, ts[i].state = int(s.get("stream", 0)), int(s["n_units"]), int(s.get("names", i))
        ts[i].variant, ts[i].channels = int(s.get("variant", 0)), int(s.get("channels", 1))
        ts[i].out_bits, ts[i].out_channels = int(s["out_bits"]), int(s["out_channels"])
        ts[i].resample, ts[i].flush = int(bool(s.get("resample", 0))), int(bool(s.get("flush", 0)))
        states[i] = s["state"]
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
    rc = lib.sk_tick_run_gsm(engine._h, ts, len(streams), table, len(units), blob.ctypes.data, total, out.ctypes.data, out.size if out_cap is None else out_cap,
                             recs, outs_cap, C.byref(n_out), C.byref(used), states, len(streams) if n_states is None else n_states)
    return rc, [telephony.state_words(states[i]) for i in range(len(streams))], n_out.value


@gpu
def test_a_refused_tick_leaves_the_carry_and_the_resampler_as_they_were(engine):
    from soundkit_amd import telephony
    variant, out_hz, out_bits, out_ch = TABLE[0]
    units, pcm, final = dealt_streams()[0]
    # the PCM tick on the model's samples, this stream alone as below
    want = b"".join(r[2] for r in run_ticks(engine, "pcm", [TABLE[0]], [pcm], [[8]])[0][0])
    sid = engine.open_stream(8000, 1)
    engine.resampler_open(sid, 8000, out_hz)
    try:
        entry = {"variant": variant, "out_bits": out_bits, "out_channels": out_ch, "stream": sid, "resample": 1, "n_units": 3,
                 "state": telephony.new_state(telephony.GSM)}
        got = engine.tick_run_gsm([entry], units[:3])
        mid = telephony.state_words(entry["state"])
        assert mid != telephony.state_words(telephony.new_state(telephony.GSM))
        nxt = dict(entry, n_units=2)
        other = M.build_stream(M.random_frames(5, 2))
        neighbour = {"variant": 0, "out_bits": 24, "out_channels": 1, "n_units": 1, "state": telephony.new_state(telephony.GSM)}
        bad_magic = other[:33] + bytes([0x70 | (other[33] & 15)]) + other[34:]
        refusals = [  # (label, table, units, output capacity in bytes, in records, states)
            ("a flush without a resampler", [nxt, dict(neighbour, flush=1)], units[3:5] + [other], None, 256, None),
            ("a neighbour's depth the PCM body does not take", [nxt, dict(neighbour, out_bits=12)], units[3:5] + [other], None, 256, None),
            ("a neighbour whose variant is none", [nxt, dict(neighbour, variant=2)], units[3:5] + [other], None, 256, None),
            ("a neighbour that is not mono", [nxt, dict(neighbour, channels=2)], units[3:5] + [other], None, 256, None),
            ("a neighbour's frame without the magic nibble", [nxt, neighbour], units[3:5] + [bad_magic], None, 256, None),
            ("an empty unit", [nxt], [units[3], b""], None, 256, None),
            ("a unit that is no whole packet", [nxt], [units[3], units[4][:-1]], None, 256, None),
            ("a Microsoft unit of standard size", [nxt, dict(neighbour, variant=1)], units[3:5] + [other], None, 256, None),
            ("a state named twice", [nxt, dict(neighbour, names=0)], units[3:5] + [other], None, 256, None),
            ("a state that is not there", [nxt, neighbour], units[3:5] + [other], None, 256, 1),
            ("an output too small in bytes", [nxt, neighbour], units[3:5] + [other], 64, 256, None),
            ("an output too small in records", [nxt, neighbour], units[3:5] + [other], None, 1, None)]
        for label, table, us, cap, outs_cap, n_states in refusals:
            rc, words, n_outs = raw_tick(engine, table, us, cap, outs_cap, n_states)
            assert rc == -1 and n_outs == 0, label
            assert words[0] == mid, label  # the caller's record keeps the carry it came with
            assert len(words) == 1 or words[1] == M.GsmCore().words(), label
        # the same units sent again give the right answer
        rest = dict(entry, n_units=5, flush=1)
        got += engine.tick_run_gsm([rest], units[3:])
        assert telephony.state_words(rest["state"]) == final
    finally:
        engine.resampler_close(sid)
        engine.close_stream(sid)
    assert all(r[1] == 0 for r in got)
    assert b"".join(r[5] for r in got) == want and len(want) > 2 * 2 * 4096

"""AIFF through the tick (sk_tick_run_aiff, Engine.tick_run_aiff) across tick boundaries: the IMA4 state and the resampler's state go
out of one launch and into the next, so the units are dealt out over ticks in several ways and every deal must give the same bytes.

Expected values are never the code under test: the decoded PCM is tests/aiff_model.py's (the IMA4 state threaded by the model), and
whatever stands behind the decode -- a depth or channel change, a resampler -- is sk_tick_run_pcm fed that PCM as little-endian
units of the contract's format, which the PCM tick's own tests pin to the reference.  Every comparison is bit for bit.

* units dealt out over ticks (all at once, one a tick, unevenly with ticks that give a stream nothing), with and without a resampler;
* QuickTime's carry rule at the first packet of a tick: a header 0x7f away from the carried predictor, 0x80 away, the step index off
  by one, a chain on the +32767 rail -- delivered as decoded and behind a stereo-to-mono conversion;
* refused ticks -- by the table, by a neighbour, by an output too small for what the resampler rounds would deliver -- leave the
  caller's IMA4 state and the resampler where they were;
* empty and flush-only ticks."""
import ctypes as C
import functools

import numpy as np
import pytest

import aiff_builder as B
import aiff_model as M

gpu = pytest.mark.gpu

GROUP_UNITS = [1, 63, 64, 65, 31, 32, 33, 7, 29, 2, 40, 13]  # groups per IMA4 unit: both sides of the kernel's 64-packet round, mono and stereo
FRAME_UNITS = [1, 15, 16, 17, 4095, 4097, 700, 33, 1000, 2, 511, 257]  # frames per unit of the elementwise encodings
DEALS = {"all at once": lambda i: [12],
         "one unit a tick": lambda i: [1] * 12,
         "uneven": lambda i: [[5, 0, 0, 6, 1], [0, 1, 10, 0, 1], [2, 7, 0, 0, 3]][i % 3],
         "uneven, the other way": lambda i: [[0, 0, 11, 1], [4, 4, 0, 4], [1, 0, 1, 10]][i % 3]}
# (encoding, channels, rate, out_rate or None, out_bits, out_channels)
TABLE = [(M.IMA4, 1, 22050, 16000, 16, 1),
         (M.IMA4, 2, 44100, 16000, 16, 1),
         (M.S24BE, 2, 48000, 16000, 16, 1),
         (M.ULAW, 1, 8000, 16000, 16, 1),
         (M.F32BE, 1, 32000, 8000, 32, 1),
         (M.IMA4, 2, 44100, None, 24, 1)]


def fmt_of(enc):
    import soundkit_amd.engine as E
    return {(16, False): E.FMT_S16LE, (24, False): E.FMT_S24LE, (32, False): E.FMT_S32LE, (32, True): E.FMT_F32LE}[M.contract(enc)]


def header(pred, idx):
    word = (pred & 0xff80) | idx
    return [(word >> 8) & 0xff, word & 0xff]


def chained_ima4(rng, groups, channels, state):
    """random packets of which two in three continue from the carried state (their header agrees with it); `state` is advanced"""
    p = B.ima4_packets(rng, groups, channels)
    p[:, :, 2:] &= 0x37  # small steps: the signal stays off the rails most of the time
    for g in range(groups):
        for c in range(channels):
            if rng.integers(0, 3):
                p[g, c, 0], p[g, c, 1] = header(state[c][0], state[c][1])
            M.ima4_packet(p[g, c].tolist(), state[c])
    return p.tobytes()


@functools.lru_cache(maxsize=None)
def dealt_streams():
    """-> per stream of TABLE (source units, the model's decoded PCM per unit, the model's final IMA4 state)"""
    out = []
    for k, (enc, ch, rate, out_rate, out_bits, out_ch) in enumerate(TABLE):
        rng = np.random.default_rng(200 + k)
        build_state = [[0, 0], [0, 0]]
        units = []
        for u in range(12):
            if enc == M.IMA4:
                units.append(chained_ima4(rng, GROUP_UNITS[u], ch, build_state))
            elif enc == M.F32BE:
                units.append(rng.uniform(-1.1, 1.1, ch * FRAME_UNITS[u]).astype(">f4").tobytes())
            else:
                units.append(rng.integers(0, 256, ch * FRAME_UNITS[u] * M.group_bytes(enc, 1), dtype=np.uint8).tobytes())
        state = [[0, 0], [0, 0]]
        pcm = [M.decode(enc, ch, u, state) for u in units]
        if enc == M.IMA4:  # the builder's own chain and the model's decode end in the same place, and the whole equals the parts
            assert state == build_state and any(s[0] for s in state[:ch])
            whole = [[0, 0], [0, 0]]
            assert M.decode(enc, ch, b"".join(units), whole) == b"".join(pcm) and whole == state
            carried = [[0, 0], [0, 0]]
            assert M.decode(enc, ch, b"".join(units), carried, carry=False) != b"".join(pcm)  # the carry matters in this stream
        frames = sum(len(p) for p in pcm) // (ch * M.contract(enc)[0] // 8)
        assert frames == (64 * sum(GROUP_UNITS) if enc == M.IMA4 else sum(FRAME_UNITS))
        assert out_rate is None or frames > 2 * 4096 + 256  # two resampler chunks and a tail for the flush
        out.append((units, pcm, [tuple(s) for s in state]))
    return out


def test_the_dealt_streams_decode_in_the_model():
    streams = dealt_streams()
    assert len(streams) == len(TABLE) and all(len(u) == 12 and len(p) == 12 for u, p, _ in streams)
    for of in DEALS.values():
        assert all(sum(of(i)) == 12 for i in range(3))


def run_ticks(engine, kind, streams, units_of, deals):
    """every stream's concatenated output over the ticks of `deals` (lists of how many units each stream gets per tick), then a tick
    that takes what is left and flushes the resamplers.  streams: (encoding, channels, rate, out_rate, out_bits, out_channels);
    kind "aiff": the source units through tick_run_aiff, the IMA4 state threaded through the stream dicts from tick to tick;
    kind "pcm": the decoded units through tick_run_pcm.  -> (bytes per stream, final IMA4 state per stream)"""
    sids, entries = [], []
    for k, (enc, ch, rate, out_rate, out_bits, out_ch) in enumerate(streams):
        entry = {"channels": ch, "out_bits": out_bits, "out_channels": out_ch}
        if kind == "aiff":
            entry["encoding"] = enc
            if enc == M.IMA4:
                entry["ima_state"] = [(0, 0), (0, 0)]
        else:
            entry["format"] = fmt_of(enc)
        sid = None
        if out_rate is not None:
            sid = engine.open_stream(rate, ch)
            engine.resampler_open(sid, rate, out_rate)
            entry.update(stream=sid, resample=1)
        sids.append(sid)
        entries.append(entry)
    out = [b""] * len(streams)
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
            recs = engine.tick_run_aiff(entries, units) if kind == "aiff" else engine.tick_run_pcm(entries, units)
            for r in recs:
                assert r[1] == 0 and (r[3], r[4]) == (streams[r[0]][5], streams[r[0]][4])
                out[r[0]] += r[5]
    finally:
        for sid in sids:
            if sid is not None:
                engine.resampler_close(sid)
                engine.close_stream(sid)
    return out, [tuple(e["ima_state"]) if "ima_state" in e else None for e in entries]


def deal_of(of, n_streams):
    per = [of(i) for i in range(n_streams)]
    ticks = max(len(p) for p in per)
    return [[p[t] if t < len(p) else 0 for p in per] for t in range(ticks)]


@gpu
def test_every_deal_gives_the_pcm_tick_on_the_models_decode(engine):
    built = dealt_streams()
    sources, pcm = [b[0] for b in built], [b[1] for b in built]
    want, _ = run_ticks(engine, "pcm", TABLE, pcm, deal_of(DEALS["all at once"], len(TABLE)))
    for k, (enc, ch, rate, out_rate, out_bits, out_ch) in enumerate(TABLE):  # the output is there
        frames_in = sum(len(p) for p in pcm[k]) // (ch * M.contract(enc)[0] // 8)
        frames_out = len(want[k]) // (out_bits // 8 * out_ch)
        if out_rate is None:
            assert frames_out == frames_in
        else:
            assert 0.9 * frames_in * out_rate / rate < frames_out < 1.1 * frames_in * out_rate / rate + 300, TABLE[k]
        assert any(want[k])
    for name, of in DEALS.items():
        got, states = run_ticks(engine, "aiff", TABLE, sources, deal_of(of, len(TABLE)))
        for k, t in enumerate(TABLE):
            assert got[k] == want[k], (name, t)
            if t[0] == M.IMA4:
                assert list(states[k])[:t[1]] == built[k][2][:t[1]], (name, t)


# ---- the carry rule at the first packet of a tick -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def first_packets():
    """test_ima4_rule_edges' construction: packets (from a zero state) whose end predictor lies 0x7f, 1 or 0 above a multiple of 128
    -> {low seven bits: (packet, (predictor, step index))}"""
    found = {}
    for seed in range(4000):
        first = [0x03, 0x94] + list(np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8) & 0x33)
        st = [0, 0]
        M.ima4_packet(first, st)
        found.setdefault(st[0] & 0x7f, (first, tuple(st)))
        if all(k in found for k in (0x7f, 1, 0)):
            break
    assert all(k in found for k in (0x7f, 1, 0))
    return found


# what the first packet of the second tick does with the state the first tick left: (low bits of that state's predictor, header
# predictor - carried predictor, header index - carried index, continues?)
EDGES = {"agrees, exactly 0x7f below": (0x7f, -0x7f, 0, True),
         "agrees, one above": (0x7f, 1, 0, True),
         "agrees, exactly 0x7f above": (1, 0x7f, 0, True),
         "disagrees by 0x80 below": (0, -0x80, 0, False),
         "disagrees by 0x80 above": (0, 0x80, 0, False),
         "agrees in the predictor, not in the step index": (0x7f, -0x7f, 1, False),
         "the same predictor, another step index": (0, 0, 1, False)}
# stereo: (left, right); in the second only the right channel disagrees
EDGE_PAIRS = [("agrees, exactly 0x7f below", "agrees, exactly 0x7f above"),
              ("agrees, exactly 0x7f below", "disagrees by 0x80 above"),
              ("disagrees by 0x80 below", "agrees, one above"),
              ("agrees in the predictor, not in the step index", "disagrees by 0x80 below"),
              ("agrees, one above", "the same predictor, another step index")]


def edge_stream(pair, rng):
    """-> (the units of tick one and of tick two, stereo) for the two channels' edges; the rule is checked on the model here"""
    ticks = [[], []]
    tail = [list(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(2)]
    for c, name in enumerate(pair):
        low, d, di, keeps = EDGES[name]
        first, (pred, idx) = first_packets()[low]
        second = header(pred + d, idx + di) + tail[c]
        ticks[0].append(first)
        ticks[1].append(second)
        st = [pred, idx]
        first_sample = int(M.ima4_packet(second, st)[0])
        hp = (pred + d) & 0xff80
        hp = hp - 0x10000 if hp & 0x8000 else hp
        assert hp == pred + d and abs(d) in (0, 1, 0x7f, 0x80)
        step, n = M.STEP[idx + di], tail[c][0] & 15
        delta = (step >> 3) + (step >> 2 if n & 1 else 0) + (step >> 1 if n & 2 else 0) + (step if n & 4 else 0)
        start = pred if keeps else hp
        assert first_sample == max(-32768, min(32767, start - delta if n & 8 else start + delta)), name  # the rule as DESIGN states it
    more = B.ima4_packets(rng, 3, 2).tobytes()
    return [bytes(ticks[0][0] + ticks[0][1])], [bytes(ticks[1][0] + ticks[1][1]) + more]


def rail_stream(rng):
    """a chain that reaches +32767 in tick one and stays there: the first packet of tick two agrees with the carried state (its header
    can only say 0x7f80, 0x7f below), steps down once from the carried 32767 and runs into the rail again -- the clamped serial walk
    on a packet that starts from carried state"""
    up = [0x00, 88] + [0x77] * 32
    down_up = header(32767, 88) + [0x78] + [0x77] * 31
    held = header(32767, 88) + [0x77] * 32
    st = [0, 0]
    M.ima4_packet(up, st)
    assert st == [32767, 88]
    w = M.ima4_packet(down_up, st)
    assert int(w[0]) == 32767 - (32767 >> 3) and int(w[-1]) == 32767 and st == [32767, 88]
    assert int(M.ima4_packet(down_up, [32640, 88])[0]) != int(w[0])  # from the header it would be another signal
    more = B.ima4_packets(rng, 2, 2).tobytes()
    return [bytes(up + up)], [bytes(down_up + held) + bytes(held + down_up) + more]


def edge_cases():
    rng = np.random.default_rng(300)
    """-> (name, (units of tick one, units of tick two), whether tick two depends on the state tick one left)"""
    return [("%s | %s" % p, edge_stream(p, rng), any(EDGES[n][3] for n in p)) for p in EDGE_PAIRS] + [("on the +32767 rail", rail_stream(rng), True)]


def test_the_edge_streams_follow_the_rule_in_the_model():
    for name, (one, two), depends in edge_cases():
        st = [[0, 0], [0, 0]]
        a = M.decode(M.IMA4, 2, one[0], st)
        b = M.decode(M.IMA4, 2, two[0], st)
        fresh = M.decode(M.IMA4, 2, two[0], [[0, 0], [0, 0]])
        assert len(a) == 256 and len(b) == len(two[0]) // 68 * 256
        assert (b != fresh) == depends, name  # a packet that continues depends on what tick one left behind, one that restarts does not


@gpu
@pytest.mark.parametrize("out_channels", [2, 1], ids=["as decoded", "stereo to mono"])
def test_the_carry_rule_at_the_first_packet_of_a_tick(engine, out_channels):
    import soundkit_amd.engine as E
    cases = edge_cases()
    entries = [{"encoding": M.IMA4, "channels": 2, "out_bits": 16, "out_channels": out_channels, "n_units": 1, "ima_state": [(0, 0), (0, 0)]}
               for _ in cases]
    states = [[[0, 0], [0, 0]] for _ in cases]
    for tick in (0, 1):
        units = [units_of[tick][0] for _, units_of, _ in cases]
        decoded = [M.decode(M.IMA4, 2, u, st) for u, st in zip(units, states)]
        recs = engine.tick_run_aiff(entries, units)
        if out_channels == 2:
            want = [(i, 0, len(d) // 4, 2, 16, d, False) for i, d in enumerate(decoded)]
        else:
            want = engine.tick_run_pcm([{"format": E.FMT_S16LE, "channels": 2, "out_bits": 16, "out_channels": 1, "n_units": 1} for _ in cases], decoded)
        assert len(recs) == len(cases)
        for (name, _, _), got, w in zip(cases, recs, want):
            assert got == w, (name, "tick %d" % tick)
        for (name, _, _), e, st in zip(cases, entries, states):
            assert e["ima_state"] == [tuple(s) for s in st], (name, "tick %d" % tick)


# ---- refused ticks ------------------------------------------------------------------------------------------------------------------

def raw_tick(engine, streams, units, out_cap=None, outs_cap=256):
    """sk_tick_run_aiff as Engine.tick_run_aiff calls it, but the status comes back instead of an exception and the caller's table
    is read back whatever the status -> (status, [IMA4 state per stream], n_outs, the records' bytes one after the other)"""
    from soundkit_amd._lib import AiffTickStream, PcmUnit, TickOutput, lib
    ts = (AiffTickStream * max(len(streams), 1))()
    for i, s in enumerate(streams):
        ts[i].stream, ts[i].n_units = int(s.get("stream", 0)), int(s["n_units"])
        ts[i].encoding, ts[i].channels = int(s["encoding"]), int(s["channels"])
        ts[i].out_bits, ts[i].out_channels = int(s["out_bits"]), int(s["out_channels"])
        ts[i].resample, ts[i].flush = int(bool(s.get("resample", 0))), int(bool(s.get("flush", 0)))
        for c, (p, x) in enumerate(s.get("ima_state") or []):
            ts[i].ima_state[c].predictor, ts[i].ima_state[c].step_index = int(p), int(x)
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
    rc = lib.sk_tick_run_aiff(engine._h, ts, len(streams), table, len(units), blob.ctypes.data, total, out.ctypes.data,
                              out.size if out_cap is None else out_cap, recs, outs_cap, C.byref(n_out), C.byref(used))
    payload = b"".join(out[r.byte_offset:r.byte_offset + r.bytes].tobytes() for r in recs[:n_out.value])
    return rc, [[(ts[i].ima_state[c].predictor, ts[i].ima_state[c].step_index) for c in range(2)] for i in range(len(streams))], n_out.value, payload


def out_bound(engine, streams, units):
    """sk_tick_aiff_out_bound_on's bytes for this table: what Engine.tick_run_aiff brings as capacity"""
    from soundkit_amd._lib import AiffTickStream, PcmUnit, lib
    ts = (AiffTickStream * len(streams))()
    for i, s in enumerate(streams):
        ts[i].stream, ts[i].n_units, ts[i].encoding, ts[i].channels = int(s.get("stream", 0)), int(s["n_units"]), int(s["encoding"]), int(s["channels"])
        ts[i].out_bits, ts[i].out_channels, ts[i].resample = int(s["out_bits"]), int(s["out_channels"]), int(bool(s.get("resample", 0)))
    table = (PcmUnit * len(units))()
    total = 0
    for k, u in enumerate(units):
        table[k].byte_offset, table[k].byte_len = total, len(u)
        total += (len(u) + 15) & ~15
    return lib.sk_tick_aiff_out_bound_on(engine._h, ts, len(streams), table, len(units), None)


@gpu
@pytest.mark.parametrize("k", [0, 1], ids=["ima4 mono 22050 to 16000", "ima4 stereo 44100 to 16000 mono"])
def test_a_refused_tick_leaves_the_ima4_state_and_the_resampler_as_they_were(engine, k):
    import soundkit_amd
    enc, ch, rate, out_rate, out_bits, out_ch = TABLE[k]
    units, pcm, final = dealt_streams()[k]
    want, _ = run_ticks(engine, "aiff", [TABLE[k]], [units], [[5]])
    sid = engine.open_stream(rate, ch)
    engine.resampler_open(sid, rate, out_rate)
    try:
        entry = {"encoding": enc, "channels": ch, "out_bits": out_bits, "out_channels": out_ch, "stream": sid, "resample": 1, "n_units": 5,
                 "ima_state": [(0, 0), (0, 0)]}
        got = engine.tick_run_aiff([entry], units[:5])
        split = len(got)
        mid = list(entry["ima_state"])
        assert all(p != 0 for p, _ in mid[:ch])  # a state that zeros, or the header's restart, cannot stand in for
        nxt = dict(entry, n_units=2)
        four = np.random.default_rng(5).integers(-9000, 9000, 4 * 100).astype(">i2").tobytes()
        ok_neighbour = {"encoding": M.S16BE, "channels": 2, "out_bits": 24, "out_channels": 1, "n_units": 1}
        refusals = [  # (label, table, units, output capacity in bytes, in records, status)
            ("a unit that is no multiple of the group", [nxt], [units[5], units[6][:-1]], None, 256, -1),
            ("step index 89", [dict(nxt, ima_state=[(mid[0][0], 89), mid[1]])], units[5:7], None, 256, -1),
            ("a flush without a resampler", [nxt, dict(ok_neighbour, flush=1)], units[5:7] + [four], None, 256, -1),
            ("the stream's own flush without its resampler", [dict(nxt, resample=0, flush=1, out_bits=24)], units[5:7], None, 256, -1),
            ("a neighbour's depth the PCM body does not take", [nxt, dict(ok_neighbour, out_bits=12)], units[5:7] + [four], None, 256, -1),
            ("a 4-channel neighbour that wants 2 channels, no pool", [nxt, dict(ok_neighbour, channels=4, out_channels=2, out_bits=16)],
             units[5:7] + [four], None, 256, -6),
            # what the tick would deliver is only known from the resamplers' time index: all the same it is refused before their rounds run
            ("an output too small in bytes", [nxt, ok_neighbour], units[5:7] + [four], 64, 256, -1),
            ("an output too small in records", [nxt, ok_neighbour], units[5:7] + [four], None, 1, -1)]
        for label, table, us, cap, outs_cap, status in refusals:
            rc, states, n_outs, _ = raw_tick(engine, table, us, cap, outs_cap)
            assert rc == status and n_outs == 0, label
            if "89" not in label:
                assert states[0] == mid, label  # the caller's table keeps the state it came with
            else:
                assert states[0][0] == (mid[0][0], 89), label
            assert entry["ima_state"] == mid
        # ... and through Engine.tick_run_aiff the dict keeps it as well
        with pytest.raises(soundkit_amd.SoundkitError) as exc:
            engine.tick_run_aiff([nxt, dict(ok_neighbour, channels=4, out_channels=2, out_bits=16)], units[5:7] + [four])
        assert exc.value.status == -6 and nxt["ima_state"] == mid
        # (the 4-channel neighbour as decoded is no reason to refuse)
        assert raw_tick(engine, [dict(ok_neighbour, channels=4, out_channels=4, out_bits=16)], [four])[0] == 0
        # the remaining units with less room than sk_tick_aiff_out_bound_on asks for: refused kilobyte by kilobyte until they fit -- the
        # tick then works out what it will deliver, chunk by chunk -- and then taken
        rest = dict(entry, n_units=7)
        bound, cap, tries = out_bound(engine, [rest], units[5:]), 0, 0
        while True:
            cap += 1024
            rc, states, n_outs, payload = raw_tick(engine, [rest], units[5:], cap)
            if rc == 0:
                break
            tries += 1
            assert rc == -1 and states[0] == mid and n_outs == 0 and cap < bound, cap
        assert tries >= 3 and cap < bound - 1024 and n_outs >= 1 and cap - 1024 < len(payload) <= cap
        rest["ima_state"] = states[0]
        assert states[0][:ch] == final[:ch]
        last = dict(rest, n_units=0, flush=1)
        got += engine.tick_run_aiff([last], [])
        assert list(last["ima_state"]) == list(rest["ima_state"])
    finally:
        engine.resampler_close(sid)
        engine.close_stream(sid)
    assert all(r[1] == 0 for r in got)
    first, tail = b"".join(r[5] for r in got[:split]), b"".join(r[5] for r in got[split:])
    assert first + payload + tail == want[0] and len(want[0]) > 2 * 8000


# ---- empty and flush-only ticks -------------------------------------------------------------------------------------------------------

@gpu
def test_empty_and_flush_only_ticks(engine):
    enc, ch, rate, out_rate, out_bits, out_ch = TABLE[1]
    units, pcm, final = dealt_streams()[1]
    pcm_entry = {"format": fmt_of(enc), "channels": ch, "out_bits": out_bits, "out_channels": out_ch, "resample": 1}
    outs, states = [], None
    for kind in ("pcm", "aiff"):
        sid = engine.open_stream(rate, ch)
        engine.resampler_open(sid, rate, out_rate)
        try:
            if kind == "pcm":
                entry = dict(pcm_entry, stream=sid)
                run = lambda e, u: engine.tick_run_pcm([e], u)
                src = pcm
            else:
                entry = {"encoding": enc, "channels": ch, "out_bits": out_bits, "out_channels": out_ch, "stream": sid, "resample": 1,
                         "ima_state": [(0, 0), (0, 0)]}
                run = lambda e, u: engine.tick_run_aiff([e], u)
                src = units
            body = run(dict(entry, n_units=0), [])  # nothing in, nothing out, before anything was fed
            assert body == []
            first = dict(entry, n_units=3)
            body = run(first, src[:3])  # 128 groups: 8192 frames, one chunk out, the second held back with the filter's delay
            if kind == "aiff":
                mid = list(first["ima_state"])
                want_mid = [[0, 0], [0, 0]]
                M.decode(enc, ch, b"".join(units[:3]), want_mid)
                assert mid == [tuple(s) for s in want_mid]
                idle = dict(first, n_units=0)
                assert run(idle, []) == [] and idle["ima_state"] == mid  # an empty tick in the middle of the stream
                flush = dict(first, n_units=0, flush=1)
                tail = run(flush, [])
                assert flush["ima_state"] == mid  # a flush-only tick leaves the IMA4 state alone
            else:
                assert run(dict(entry, n_units=0), []) == []
                tail = run(dict(entry, n_units=0, flush=1), [])
            assert tail and all(r[1] == 0 and r[2] > 0 for r in tail)
            outs.append((body, tail))
        finally:
            engine.resampler_close(sid)
            engine.close_stream(sid)
    assert outs[0] == outs[1]

"""Vorbis through the tick (sk_tick_run_vorbis, Engine.tick_run_vorbis): whole packets decoded on the device in front of what
sk_tick_run_pcm runs.  A stream with nothing to change gets the decoded s16, one output per packet that yields frames; every other
stream must give exactly the records sk_tick_run_pcm gives for the same s16 handed in as little-endian units -- which the PCM tick's
own tests pin to the reference's CPU chain -- whichever way its packets are dealt out over ticks (1, 2 and 7 a tick, and a tick that ends
right behind a block-size change); a refused tick leaves the streams as they were; a damaged packet costs its own samples and the
overlap that follows.  The decoded s16 itself is held to the model and the recording in test_vorbis_decode_gpu.py."""
import numpy as np
import pytest

import vorbis_cases as CASES
import vorbis_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setups():
    from soundkit_amd import vorbis
    return {c.name: vorbis.Setup(vorbis.parse_ident(c.headers[0]), c.headers[2]) for c in CASES.all_cases()}


def case(name):
    return next(c for c in CASES.all_cases() if c.name == name)


def decoded(engine, setups, name, packets=None):
    """the decode call's s16 per packet: [(status, bytes)]"""
    from soundkit_amd import vorbis
    c = case(name)
    rows = engine.vorbis_decode_packets([(vorbis.StreamState(setups[name]), c.packets if packets is None else packets)])[0]
    return [(s, pcm.astype("<i2").tobytes()) for s, pcm in rows]


def deal(engine, setups, names, deals, entry):
    """every stream's records over the ticks of `deals` (how many packets each stream gets per tick) -> [records per stream]"""
    from soundkit_amd import vorbis
    states = [vorbis.StreamState(setups[n]) for n in names]
    at, out = [0] * len(names), [[] for _ in names]
    for d in deals:
        table, packets = [], []
        for i, n in enumerate(names):
            table.append(dict(entry(i), state=states[i], n_units=d[i]))
            packets += case(n).packets[at[i]:at[i] + d[i]]
            at[i] += d[i]
        recs, status = engine.tick_run_vorbis(table, packets)
        assert not any(status)
        for r in recs:
            assert r[1] == 0
            out[r[0]].append(r)
    return out


def test_streams_with_nothing_to_change_get_the_decoded_s16_one_output_per_packet(engine, setups):
    names = ["ogg", "webm", "mono-64-128", "three-256-2048", "eight-64-8192"]
    counts = [12, 9, 7, 7, 7]
    got = deal(engine, setups, names, [counts], lambda i: {"out_bits": 16, "out_channels": case(names[i]).ident["channels"]})
    for name, n, recs in zip(names, counts, got):
        ch = case(name).ident["channels"]
        want = [b for _, b in decoded(engine, setups, name, case(name).packets[:n]) if b]
        assert len(want) == n - 1  # the first packet yields nothing
        assert [(r[2], r[3], r[4], r[5]) for r in recs] == [(len(b) // (2 * ch), ch, 16, b) for b in want], name


@pytest.mark.parametrize("deals", [[[1, 1]] * 7, [[2, 2]] * 3 + [[1, 1]], [[7, 7]], [[3, 2], [4, 5]], [[0, 4], [7, 0], [0, 3]]],
                         ids=["one a tick", "two a tick", "seven a tick", "behind a block-size change", "uneven, with empty ticks"])
def test_the_output_does_not_depend_on_how_packets_are_dealt_over_ticks(engine, setups, deals):
    names = ["three-256-2048", "stereo-64-128-type2"]  # FLAGS = S S L L S L S: packet 2 is the first long one
    assert CASES.FLAGS[2] == 1 and CASES.FLAGS[1] == 0
    got = deal(engine, setups, names, deals, lambda i: {"out_bits": 16, "out_channels": case(names[i]).ident["channels"]})
    for name, recs in zip(names, got):
        assert b"".join(r[5] for r in recs) == b"".join(b for _, b in decoded(engine, setups, name)), name


def test_conversions_equal_the_pcm_tick_on_the_decoded_s16(engine, setups):
    """depth and channel changes without a rate change: stereo to mono, 16 to 24 and 32 bits"""
    import soundkit_amd.engine as E
    names = ["webm", "stereo-64-64", "mono-64-128", "ogg"]
    outs = [(16, 1), (24, 1), (32, 1), (24, 1)]
    counts = [10, 7, 7, 20]
    got = deal(engine, setups, names, [counts], lambda i: {"out_bits": outs[i][0], "out_channels": outs[i][1]})
    p_streams, p_units = [], []
    for name, n, (bits, och) in zip(names, counts, outs):
        units = [b for _, b in decoded(engine, setups, name, case(name).packets[:n]) if b]
        p_streams.append({"format": E.FMT_S16LE, "channels": case(name).ident["channels"], "out_bits": bits, "out_channels": och, "n_units": len(units)})
        p_units += units
    want = engine.tick_run_pcm(p_streams, p_units)
    assert [r for recs in got for r in recs] == want and len(want) == sum(counts) - len(counts)


def resampled(engine, kind, setups, specs, deals):
    """every stream's concatenated output over the ticks of `deals`, then a flush.  specs: (name, rate, out_rate, out_bits, out_channels)"""
    import soundkit_amd.engine as E
    from soundkit_amd import vorbis
    sids, states, units_of = [], [], []
    for name, rate, out_rate, _, _ in specs:
        ch = case(name).ident["channels"]
        sid = engine.open_stream(rate, ch)
        engine.resampler_open(sid, rate, out_rate)
        sids.append(sid)
        states.append(vorbis.StreamState(setups[name]))
        units_of.append(case(name).packets if kind == "vorbis" else [b for _, b in decoded(engine, setups, name) if b])
    out, at = [b""] * len(specs), [0] * len(specs)
    try:
        for d in list(deals) + [None]:
            table, units = [], []
            for i, (name, rate, out_rate, bits, och) in enumerate(specs):
                n = len(units_of[i]) - at[i] if d is None else min(d[i], len(units_of[i]) - at[i])
                row = {"out_bits": bits, "out_channels": och, "stream": sids[i], "resample": 1, "flush": 1 if d is None else 0, "n_units": n}
                if kind == "vorbis":
                    row["state"] = states[i]
                else:
                    row.update(format=E.FMT_S16LE, channels=case(name).ident["channels"])
                table.append(row)
                units += units_of[i][at[i]:at[i] + n]
                at[i] += n
            if kind == "vorbis":
                recs, status = engine.tick_run_vorbis(table, units)
                assert not any(status)
            else:
                recs = engine.tick_run_pcm(table, units)
            for r in recs:
                assert r[1] == 0
                out[r[0]] += r[5]
    finally:
        for sid in sids:
            engine.resampler_close(sid)
            engine.close_stream(sid)
    return out


def test_rate_changes_meet_the_pcm_tick_however_the_packets_are_dealt_out(engine, setups):
    """8 -> 16 kHz mono (the Ogg fixture) and 44.1 -> 16 kHz, stereo to mono (the WebM fixture), both to s16"""
    specs = [("ogg", 8000, 16000, 16, 1), ("webm", 44100, 16000, 16, 1)]
    want = resampled(engine, "pcm", setups, specs, [[93, 55]])
    assert len(want[0]) > 2 * 2 * 23000 and len(want[1]) > 2 * 10000
    assert resampled(engine, "vorbis", setups, specs, [[94, 56]]) == want
    assert resampled(engine, "vorbis", setups, specs, [[7, 7]] * 14) == want
    assert resampled(engine, "vorbis", setups, specs, [[1, 2]] * 30 + [[40, 0]]) == want


def test_a_refused_tick_changes_nothing(engine, setups):
    from soundkit_amd import SoundkitError, vorbis
    name = "stereo-64-64"
    st = vorbis.StreamState(setups[name])
    row = {"state": st, "out_bits": 16, "out_channels": 2, "n_units": 3}
    first, _ = engine.tick_run_vorbis([row], case(name).packets[:3])
    before = (st.prev_blocksize, st.overlap.copy())
    assert before[0] == 64 and np.any(before[1])
    with pytest.raises(SoundkitError):
        engine.tick_run_vorbis([dict(row, n_units=4)], case(name).packets[3:7], out_cap=32)  # room for less than the tick delivers
    assert st.prev_blocksize == before[0] and np.array_equal(st.overlap, before[1])
    rest, status = engine.tick_run_vorbis([dict(row, n_units=4)], case(name).packets[3:7])
    assert not any(status)
    assert b"".join(r[5] for r in first + rest) == b"".join(b for _, b in decoded(engine, setups, name))


def test_a_damaged_packet_costs_its_own_samples_and_the_overlap_that_follows(engine, setups):
    from soundkit_amd import vorbis
    name = "mono-64-128"
    c = case(name)
    packets = c.packets[:3] + [bytes([c.packets[3][0] | 1]) + c.packets[3][1:], b""] + c.packets[4:]
    want = decoded(engine, setups, name, packets)
    assert [s for s, _ in want] == [0, 0, 0, M.ST_NOT_AUDIO, M.ST_SHORT, 0, 0, 0]
    for cuts in ([8], [3, 2, 3], [4, 4]):
        st, recs, status, at = vorbis.StreamState(setups[name]), [], [], 0
        for n in cuts:
            r, s = engine.tick_run_vorbis([{"state": st, "out_bits": 16, "out_channels": 1, "n_units": n}], packets[at:at + n])
            recs, status, at = recs + r, status + s, at + n
        assert status == [s for s, _ in want]
        assert [r[5] for r in recs] == [b for _, b in want if b], cuts


def test_an_eight_channel_stream_with_a_conversion_needs_the_wide_pool(engine):
    import soundkit_amd
    import soundkit_amd.engine as E
    from soundkit_amd import vorbis
    c = case("eight-64-8192")

    def rows(eng):
        setup = vorbis.Setup(vorbis.parse_ident(c.headers[0]), c.headers[2])
        return setup, [{"state": vorbis.StreamState(setup), "out_bits": 16, "out_channels": 2, "n_units": 4}]

    _, table = rows(engine)
    with pytest.raises(soundkit_amd.SoundkitError):
        engine.tick_run_vorbis(table, c.packets[:4])  # the session's engine has no pool
    assert table[0]["state"].prev_blocksize == 0  # ... and the refused tick left the carry alone
    wide = soundkit_amd.Engine(0, 64)
    try:
        wide.enable_wide_pcm(8)
        setup, table = rows(wide)
        got, status = wide.tick_run_vorbis(table, c.packets[:4])
        units = [pcm.astype("<i2").tobytes() for _, pcm in wide.vorbis_decode_packets([(vorbis.StreamState(setup), c.packets[:4])])[0] if pcm.size]
        want = wide.tick_run_pcm([{"format": E.FMT_S16LE, "channels": 8, "out_bits": 16, "out_channels": 2, "n_units": 3}], units)
        assert status == [0] * 4 and got == want and len(got) == 3
    finally:
        wide.close()

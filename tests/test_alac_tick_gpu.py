"""ALAC through the tick (sk_tick_run_alac, Engine.tick_run_alac): whole packets decoded on the device in front of what sk_tick_run_pcm
runs.  A stream with nothing to change gets the decoded bytes, one output per packet; every other stream must give exactly the
records sk_tick_run_pcm gives for the model's PCM handed in as little-endian units -- which the PCM tick's own tests pin to the
reference -- whichever way its packets are dealt out over ticks; 3 ... 8 channels with a conversion need the wide pool; a refused tick
leaves the streams as they were; a rejected packet marks its records and leaves the neighbours alone."""
import os

import pytest

import alac_builder as B
import alac_cases as CASES
import alac_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "alac", "A_Tusk_is_used_to_make_costly_gifts.caf")
INVALID = -601


def pcm_fmt(bits):
    import soundkit_amd.engine as E
    return {16: E.FMT_S16LE, 24: E.FMT_S24LE, 32: E.FMT_S32LE}[bits]


def built(seed, bits, nch, rate, sizes, kind="tone", **el):
    """-> (cfg, [packet bytes], [the model's PCM per packet])"""
    cfg = B.config(4096, bits, nch, rate)
    packets, pcm = [], []
    for k, n in enumerate(sizes):
        ch = CASES.signal(kind, n, bits, seed * 100 + k, nch)
        if "elements" not in el:
            p = B.packet(cfg, ch, order=(4, 8, 0, 31)[k % 4], shift=6, mix_weight=k % 3, mix_shift=2, **el)
        else:
            p = B.packet(cfg, ch, **el)
        got, _ = M.decode_packet(cfg, p)
        assert got == ch
        packets.append(p)
        pcm.append(M.pcm_bytes(ch, bits))
    return cfg, packets, pcm


@pytest.fixture(scope="module")
def fixture_stream():
    data = open(FIXTURE, "rb").read()
    cfg, packets, *_ = M.caf_index(data)
    cfg = {k: v for k, v in cfg.items() if k != "caf_frames_per_packet"}
    return cfg, packets, [M.decode_packet_bytes(cfg, p) for p in packets]


def test_streams_with_nothing_to_change_get_the_decoded_bytes_one_output_per_packet(engine, fixture_stream):
    streams, packets, want = [], [], []
    sources = [fixture_stream, built(1, 16, 2, 44100, [4096, 50, 1]), built(2, 24, 1, 48000, [64, 33]), built(3, 32, 1, 48000, [40]),
               built(4, 16, 6, 48000, [48, 17], elements=[B.Element("cpe", mix_weight=1, mix_shift=2), B.Element("sce"), B.Element("cpe"), B.Element("lfe")]),
               built(5, 24, 8, 48000, [20], elements=[B.Element("cpe")] * 4)]
    for i, (cfg, p, pcm) in enumerate(sources):
        width = cfg["bit_depth"] // 8 * cfg["channels"]
        streams.append({"config": cfg, "out_bits": cfg["bit_depth"], "out_channels": cfg["channels"], "n_units": len(p)})
        packets += p
        want += [(i, 0, len(b) // width, cfg["channels"], cfg["bit_depth"], b, False) for b in pcm]
    recs, status = engine.tick_run_alac(streams, packets)
    assert status == [0] * len(packets)
    assert recs == want


def test_conversions_equal_the_pcm_tick_on_the_model_s_pcm(engine, fixture_stream):
    """depth and channel changes without a rate change, the exact 24 / 32 -> 16 path among them"""
    a_streams, a_packets, p_streams, p_units = [], [], [], []
    for i, (bits, nch, out_bits, out_ch) in enumerate([(24, 2, 16, 2), (32, 1, 16, 1), (24, 1, 16, 1), (16, 2, 16, 1), (16, 1, 24, 1), (24, 2, 32, 1),
                                                      (16, 2, 32, 2)]):
        cfg, p, pcm = built(40 + i, bits, nch, 48000, [4096, 192, 17], kind="rand" if bits < 32 else "tone")
        a_streams.append({"config": cfg, "out_bits": out_bits, "out_channels": out_ch, "n_units": len(p)})
        p_streams.append({"format": pcm_fmt(bits), "channels": nch, "out_bits": out_bits, "out_channels": out_ch, "n_units": len(p)})
        a_packets += p
        p_units += pcm
    got, status = engine.tick_run_alac(a_streams, a_packets)
    want = engine.tick_run_pcm(p_streams, p_units)
    assert status == [0] * len(a_packets) and len(got) == 21 and got == want


def resampled(engine, kind, streams, units_of, deals):
    """every stream's concatenated output over the ticks of `deals` (lists of how many units each stream gets per tick), then a flush"""
    sids = []
    for s in streams:
        sid = engine.open_stream(s["rate"], s["channels"])
        engine.resampler_open(sid, s["rate"], s["out_rate"])
        sids.append(sid)
    out = [b""] * len(streams)
    at = [0] * len(streams)
    try:
        for deal in list(deals) + [None]:
            table, units = [], []
            for i, s in enumerate(streams):
                n = len(units_of[i]) - at[i] if deal is None else deal[i]
                table.append(dict(s["entry"], stream=sids[i], resample=1, flush=1 if deal is None else 0, n_units=n))
                units += units_of[i][at[i]:at[i] + n]
                at[i] += n
            if kind == "alac":
                recs, status = engine.tick_run_alac(table, units)
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


@pytest.fixture(scope="module")
def rate_change_streams(fixture_stream):
    """the fixture 8 -> 48 kHz, a 44.1 kHz 16-bit pair to 16 kHz mono s16, a 48 kHz 24-bit mono stream to 16 kHz s16"""
    sources = [fixture_stream, built(60, 16, 2, 44100, [4096, 4096, 1000, 4096, 333]), built(61, 24, 1, 48000, [4096, 2000, 4096, 4096, 77])]
    outs = [(8000, 48000, 16, 1), (44100, 16000, 16, 1), (48000, 16000, 16, 1)]
    alac_streams, pcm_streams = [], []
    for (cfg, _, _), (rate, out_rate, out_bits, out_ch) in zip(sources, outs):
        assert cfg["sample_rate"] == rate
        common = {"rate": rate, "out_rate": out_rate, "channels": cfg["channels"]}
        alac_streams.append(dict(common, entry={"config": cfg, "out_bits": out_bits, "out_channels": out_ch}))
        pcm_streams.append(dict(common, entry={"format": pcm_fmt(cfg["bit_depth"]), "channels": cfg["channels"], "out_bits": out_bits, "out_channels": out_ch}))
    return alac_streams, [s[1] for s in sources], pcm_streams, [s[2] for s in sources]


def test_rate_changes_meet_the_pcm_tick_however_the_packets_are_dealt_out(engine, rate_change_streams):
    alac_streams, alac_units, pcm_streams, pcm_units = rate_change_streams
    in_one_tick = [[6, 5, 5]]
    want = resampled(engine, "pcm", pcm_streams, pcm_units, in_one_tick)
    # 23 680 frames at six times the rate (142 080); 13 621 at 16000 / 44100 (4942); 14 365 at a third (4788): less what the filter holds back
    assert len(want[0]) > 2 * 140000 and len(want[1]) > 2 * 4800 and len(want[2]) > 2 * 4650
    assert resampled(engine, "alac", alac_streams, alac_units, in_one_tick) == want
    assert resampled(engine, "alac", alac_streams, alac_units, [[1, 1, 1]] * 5 + [[1, 0, 0]]) == want  # one packet per tick
    assert resampled(engine, "alac", alac_streams, alac_units, [[2, 0, 1], [0, 3, 0], [3, 0, 0], [0, 1, 4], [1, 1, 0]]) == want  # unevenly, with empty ticks


def test_as_decoded_and_to_16k_mono_s16_in_one_tick_and_packet_by_packet(engine, fixture_stream):
    """without a rate change nothing is carried from tick to tick: one tick and one packet per tick give the same records"""
    cfg, packets, pcm = built(70, 16, 2, 44100, [4096, 333, 4096])
    plain = {"config": cfg, "out_bits": 16, "out_channels": 2}
    mono = {"config": cfg, "out_bits": 16, "out_channels": 1}
    whole, _ = engine.tick_run_alac([dict(plain, n_units=3), dict(mono, n_units=3)], packets + packets)
    single = []
    for p in packets:
        recs, status = engine.tick_run_alac([dict(plain, n_units=1), dict(mono, n_units=1)], [p, p])
        assert status == [0, 0]
        single += recs
    assert sorted(r[0:1] + r[2:] for r in whole) == sorted(r[0:1] + r[2:] for r in single)
    assert [r[5] for r in whole if r[0] == 0] == pcm
    want = engine.tick_run_pcm([{"format": pcm_fmt(16), "channels": 2, "out_bits": 16, "out_channels": 1, "n_units": 3}], pcm)
    assert [r[2:] for r in whole if r[0] == 1] == [r[2:] for r in want]


def test_a_six_channel_stream_needs_the_wide_pool(engine):
    import soundkit_amd
    els = [B.Element("cpe", mix_weight=1, mix_shift=2), B.Element("sce"), B.Element("cpe"), B.Element("lfe")]
    cfg, packets, pcm = built(90, 16, 6, 48000, [192, 4096, 17], elements=els)
    table = [{"config": cfg, "out_bits": 16, "out_channels": 2, "n_units": 3}]
    with pytest.raises(soundkit_amd.SoundkitError):
        engine.tick_run_alac(table, packets)  # the session's engine has no pool
    # ... while the same stream with nothing to change still delivers there
    recs, _ = engine.tick_run_alac([dict(table[0], out_channels=6)], packets)
    assert [r[5] for r in recs] == pcm
    wide = soundkit_amd.Engine(0, 64)
    try:
        wide.enable_wide_pcm(8)
        got, status = wide.tick_run_alac(table, packets)
        want = wide.tick_run_pcm([{"format": pcm_fmt(16), "channels": 6, "out_bits": 16, "out_channels": 2, "n_units": 3}], pcm)
        assert status == [0, 0, 0] and got == want and len(got) == 3
    finally:
        wide.close()


def test_a_refused_tick_leaves_the_streams_as_they_were(engine, rate_change_streams):
    import soundkit_amd
    alac_streams, alac_units, _, _ = rate_change_streams
    want = resampled(engine, "alac", alac_streams[:1], alac_units[:1], [[2], [4]])
    six, six_packets, _ = built(91, 16, 6, 48000, [64], elements=[B.Element("cpe")] * 3)
    sid = engine.open_stream(8000, 1)
    engine.resampler_open(sid, 8000, 48000)
    try:
        entry = dict(alac_streams[0]["entry"], stream=sid, resample=1, n_units=2)
        first, _ = engine.tick_run_alac([entry], alac_units[0][:2])
        # a six-channel stream that wants two channels is refused without the pool, and with it the whole tick: the resampling stream
        # beside it keeps its state
        with pytest.raises(soundkit_amd.SoundkitError):
            engine.tick_run_alac([dict(entry, n_units=4), {"config": six, "out_bits": 16, "out_channels": 2, "n_units": 1}], alac_units[0][2:] + six_packets)
        second, _ = engine.tick_run_alac([dict(entry, n_units=4)], alac_units[0][2:])
        last, _ = engine.tick_run_alac([dict(entry, n_units=0, flush=1)], [])
    finally:
        engine.resampler_close(sid)
        engine.close_stream(sid)
    assert b"".join(r[5] for r in first + second + last) == want[0]


def test_a_rejected_packet_marks_its_records_and_the_neighbours_are_exact(engine):
    cfg, good, pcm = built(80, 16, 2, 44100, [100, 60, 80])
    other_cfg, other, other_pcm = built(81, 24, 1, 44100, [50, 50])
    bad = B.packet(cfg, CASES.signal("tone", 60, 16, 5, 2), ptype=3)  # the host reads its 60 frames, the device rejects it
    damaged = [good[0], bad, good[2]]
    streams = [{"config": cfg, "out_bits": 16, "out_channels": 2, "n_units": 3},              # as decoded
               {"config": other_cfg, "out_bits": 24, "out_channels": 1, "n_units": 2},
               {"config": cfg, "out_bits": 16, "out_channels": 1, "n_units": 3},              # behind a downmix
               {"config": cfg, "out_bits": 16, "out_channels": 1, "n_units": 3}]
    recs, status = engine.tick_run_alac(streams, damaged + other + damaged + good)
    assert status == [0, INVALID, 0, 0, 0, 0, INVALID, 0, 0, 0, 0]
    assert [(r[0], r[1]) for r in recs] == [(0, 0), (0, INVALID), (0, 0), (1, 0), (1, 0), (2, INVALID), (2, INVALID), (2, INVALID), (3, 0), (3, 0), (3, 0)]
    assert recs[0][5] == pcm[0] and recs[2][5] == pcm[2] and [r[5] for r in recs[3:5]] == other_pcm
    want = engine.tick_run_pcm([{"format": pcm_fmt(16), "channels": 2, "out_bits": 16, "out_channels": 1, "n_units": 3}], pcm)
    assert [r[2:] for r in recs[8:]] == [r[2:] for r in want]


def test_bad_tables_are_refused(engine):
    import soundkit_amd
    cfg, p, _ = built(95, 16, 1, 44100, [32, 32])
    ok = {"config": cfg, "out_bits": 16, "out_channels": 1, "n_units": 2}
    for entry, packets in ((dict(ok, n_units=3), p), (dict(ok, n_units=1), p), (dict(ok, config=dict(cfg, channels=9)), p),
                           (dict(ok, config=dict(cfg, bit_depth=20)), p), (dict(ok, config=dict(cfg, frame_length=16)), p),
                           (dict(ok, out_bits=12), p), (dict(ok, flush=1), p), (ok, [p[0], bytes([0xE0])])):
        with pytest.raises(soundkit_amd.SoundkitError):
            engine.tick_run_alac([entry], packets)
    assert engine.tick_run_alac([], []) == ([], [])

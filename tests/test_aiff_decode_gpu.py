"""The AIFF decode stage on the GPU (csrc/aiff_decode.hip through sk_aiff_decode and sk_tick_run_aiff) against the model of the
reference's decode_stream_bytes (tests/aiff_model.py), bit for bit: every elementwise encoding at the sizes where the kernel changes
path (a lane's 16 samples, a workgroup's 4096), the G.711 codes, float edge cases, and IMA4 chains -- rule edges, saturation in the
middle of a chain, calls split at every packet boundary, many streams of unequal length in one tick."""
import os

import numpy as np
import pytest

import aiff_builder as B
import aiff_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ELEMENTWISE = [M.U8, M.S8, M.S16BE, M.S16LE, M.S24BE, M.S32BE, M.S32LE, M.F32BE, M.F64BE, M.ULAW, M.ALAW]


def random_source(rng, enc, samples):
    if enc == M.F64BE:  # finite doubles over the whole f32 range and beyond, a few specials
        v = rng.standard_normal(samples) * np.exp(rng.uniform(-120, 95, samples))
        return v.astype(">f8").tobytes()
    return rng.integers(0, 256, samples * M.group_bytes(enc, 1), dtype=np.uint8).tobytes()


def same_f32(got, want):
    """bit-equal, except that a NaN need only be a NaN"""
    g, w = np.frombuffer(got, "<u4"), np.frombuffer(want, "<u4")
    nan_w = np.isnan(w.view("<f4"))
    return len(g) == len(w) and np.array_equal(np.isnan(g.view("<f4")), nan_w) and np.array_equal(g[~nan_w], w[~nan_w])


@pytest.mark.parametrize("enc", ELEMENTWISE, ids=[M.NAMES[e] for e in ELEMENTWISE])
def test_elementwise_sizes_and_channels(engine, enc):
    rng = np.random.default_rng(100 + enc)
    for ch in (1, 2, 3):
        for frames in (1, 15, 16, 17, 4095, 4097):
            src = random_source(rng, enc, frames * ch)
            got = engine.aiff_decode(enc, ch, src)
            want = M.decode(enc, ch, src)
            if enc == M.F64BE:
                assert same_f32(got, want), (ch, frames)
            else:
                assert got == want, (ch, frames)


def test_empty_and_partial_groups(engine):
    import soundkit_amd
    assert engine.aiff_decode(M.S24BE, 1, b"") == b""
    for enc, ch, n in [(M.S24BE, 1, 4), (M.F64BE, 1, 12), (M.IMA4, 2, 34), (M.S16BE, 1, 3)]:
        with pytest.raises(soundkit_amd.SoundkitError):
            engine.aiff_decode(enc, ch, bytes(n))
    with pytest.raises(soundkit_amd.SoundkitError):
        engine.aiff_decode(M.IMA4, 3, bytes(102))
    with pytest.raises(soundkit_amd.SoundkitError):
        engine.aiff_decode(12, 1, bytes(16))
    with pytest.raises(soundkit_amd.SoundkitError):
        engine.aiff_decode(M.IMA4, 1, bytes(34), [(0, 89), (0, 0)])


def test_all_g711_codes(engine):
    codes = bytes(range(256)) + bytes(range(255, -1, -1)) + bytes(range(7))
    for enc in (M.ULAW, M.ALAW):
        assert engine.aiff_decode(enc, 1, codes) == M.decode(enc, 1, codes)
    u = np.frombuffer(engine.aiff_decode(M.ULAW, 1, bytes(range(256))), "<i2")
    a = np.frombuffer(engine.aiff_decode(M.ALAW, 1, bytes(range(256))), "<i2")
    assert (u[0], u[0x7f], u[0x80], u[0xff]) == (-32124, 0, 32124, 0)      # ITU-T G.711 end points
    assert (a[0x55 ^ 0x80], a[0x55], a[0x2a], a[0xaa]) == (8, -8, -32256, 32256)


def test_f32be_is_a_bit_move(engine):
    bits = np.array([0x7fc00000, 0x7f800001, 0xffffffff, 0x7fa5a5a5, 0xffc12345, 0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x00400000,
                     0x7f800000, 0xff800000, 0x3f800000, 0x7f7fffff] * 3 + [0x7f812345], np.uint32)
    src = bits.astype(">u4").tobytes()
    got = engine.aiff_decode(M.F32BE, 1, src)
    assert np.array_equal(np.frombuffer(got, "<u4"), bits)


def test_f64be_rounding(engine):
    f32 = lambda b: np.array([b], np.uint32).view(np.float32)[0].astype(np.float64)
    one, ulp = 1.0, 2.0 ** -23
    vals = [one + ulp / 2, one + 3 * ulp / 2, one + ulp / 2 + 2.0 ** -50, one + ulp / 2 - 2.0 ** -50,  # ties to even, and just off a tie
            -(one + ulp / 2), -(one + 3 * ulp / 2), 2.0 - 2.0 ** -25, 2.0 - 2.0 ** -24,               # a carry into the exponent
            2.0 ** -149, 2.0 ** -150, 2.0 ** -150 + 2.0 ** -190, 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149, -(2.0 ** -151), 2.0 ** -126 - 2.0 ** -150,
            2.0 ** -126 - 2.0 ** -151, 3.0 * 2.0 ** -140, 2.0 ** -127 + 2.0 ** -150, 5e-324, -5e-324, 2.0 ** -1000, 0.0, -0.0,
            f32(0x7f7fffff), f32(0x7f7fffff) + 2.0 ** 102, f32(0x7f7fffff) + 2.0 ** 103, -(f32(0x7f7fffff) + 2.0 ** 103), 2.0 ** 128, -2.0 ** 128, 1e300, -1e300,
            float("inf"), float("-inf"), float("nan"), -float("nan")]
    vals = np.array(vals, np.float64)
    for pad in (0, 16 - len(vals) % 16, 17):  # through the tail path, the 16-sample path, and both
        v = np.concatenate([vals, np.linspace(-3, 3, pad)])
        src = v.astype(">f8").tobytes()
        with np.errstate(over="ignore", invalid="ignore"):
            want = v.astype("<f4").tobytes()
        assert want == M.decode(M.F64BE, 1, src)
        got = engine.aiff_decode(M.F64BE, 1, src)
        assert same_f32(got, want), pad
        g = np.frombuffer(got, "<f4")
        assert np.isnan(g[len(vals) - 2:len(vals)]).all() and np.isinf(g[len(vals) - 4:len(vals) - 2]).all()
    # NaN payloads of every kind stay NaN
    nans = np.array([0x7ff0000000000001, 0xfff8000000000000, 0x7ff00000ffffffff, 0x7fffffffffffffff], np.uint64).astype(">u8").tobytes()
    assert np.isnan(np.frombuffer(engine.aiff_decode(M.F64BE, 1, nans), "<f4")).all()


# ---- IMA4 -------------------------------------------------------------------------------------------------------------------------

def model_ima(packets, channels, state=None):
    st = [list(s) for s in (state or [(0, 0), (0, 0)])]
    out = M.decode(M.IMA4, channels, packets, st)
    return out, [tuple(s) for s in st]


@pytest.mark.parametrize("channels", [1, 2])
def test_ima4_random_chains(engine, channels):
    rng = np.random.default_rng(7 + channels)
    for groups in (1, 2, 63, 64, 65, 200):
        p = B.ima4_packets(rng, groups, channels)
        p[groups // 2, 0, 1] |= 0x7f  # a header index above 88
        got, st = engine.aiff_decode(M.IMA4, channels, p.tobytes())
        want, wst = model_ima(p.tobytes(), channels)
        assert got == want and st[:channels] == wst[:channels], groups


def header(pred, idx):
    word = (pred & 0xff80) | idx
    return [(word >> 8) & 0xff, word & 0xff]


def test_ima4_rule_edges(engine):
    """headers that agree with the carried state by exactly 0x7f, disagree by 0x80, or by the index only -- with the state handed in,
    and in the middle of a chain"""
    body = [0x19] * 32
    for hp in (0x100, -0x100, 0, 0x7f80, -0x8000):
        for d in (-0x80, -0x7f, -1, 0, 1, 0x7f, 0x80):
            pred = hp + d
            if not -32768 <= pred <= 32767:
                continue
            for idx, hidx in ((30, 30), (30, 31), (88, 88), (88, 0x7f), (0, 0)):
                pk = bytes(header(hp, hidx) + body)
                state = [(pred, idx), (0, 0)]
                got, gst = engine.aiff_decode(M.IMA4, 1, pk, state)
                want, wst = model_ima(pk, 1, state)
                assert got == want and gst[0] == wst[0], (hp, d, idx, hidx)
                first = int(np.frombuffer(want, "<i2")[0])
                step = M.STEP[min(hidx, 88)]
                delta = (step >> 3) + (step >> 2)  # nibble 9: negative, bit 0
                keeps = abs(d) <= 0x7f and idx == min(hidx, 88)
                assert first == max(-32768, (pred if keeps else hp) - delta)  # the model follows the rule as DESIGN states it
    # in a chain: first packets whose end state lies 0x7f, 1 or 0 above a multiple of 128
    rng = np.random.default_rng(11)
    found = {}
    for seed in range(4000):
        first = [0x03, 0x94] + list(np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8) & 0x33)
        _, st = model_ima(bytes(first), 1)
        found.setdefault(st[0][0] & 0x7f, (first, st[0]))
        if all(k in found for k in (0x7f, 1, 0)):
            break
    assert all(k in found for k in (0x7f, 1, 0))
    tail = list(rng.integers(0, 256, 32, dtype=np.uint8))
    for low, deltas in ((0x7f, (-0x7f, 1)), (1, (-1, 0x7f)), (0, (-0x80, 0x80, 0))):
        first, (pred, idx) = found[low]
        for d in deltas:
            for di in (0, 1):
                chain = bytes(first + header(pred + d, idx + di) + tail + header(0, 0) + tail)
                got, gst = engine.aiff_decode(M.IMA4, 1, chain)
                want, wst = model_ima(chain, 1)
                assert got == want and gst[0] == wst[0], (low, d, di)


@pytest.mark.parametrize("channels", [1, 2])
def test_ima4_saturation_in_the_middle_of_a_chain(engine, channels):
    rng = np.random.default_rng(21 + channels)
    for negative in (False, True):
        p = B.ima4_packets(rng, 150, channels, pinned=(40, 110, negative))
        # the pinned run's headers agree with the carried state, so the rail is carried through the packets
        st = [[0, 0], [0, 0]]
        for g in range(150):
            for c in range(channels):
                if 41 <= g < 110:
                    word = (st[c][0] & 0xff80) | 88
                    p[g, c, 0], p[g, c, 1] = (word >> 8) & 0xff, word & 0xff
                M.ima4_packet(p[g, c].tolist(), st[c])
        want, wst = model_ima(p.tobytes(), channels)
        w = np.frombuffer(want, "<i2")
        assert (w == (-32768 if negative else 32767)).sum() > 64 * 60 * channels  # the rail is really held
        got, gst = engine.aiff_decode(M.IMA4, channels, p.tobytes())
        assert got == want and gst[:channels] == wst[:channels]


def test_ima4_split_calls_equal_one_call(engine):
    rng = np.random.default_rng(31)
    for channels in (1, 2):
        p = B.ima4_packets(rng, 70, channels, pinned=(20, 30, False))
        whole, wst = engine.aiff_decode(M.IMA4, channels, p.tobytes())
        assert whole == model_ima(p.tobytes(), channels)[0]
        for cut in range(1, 70):
            a, st = engine.aiff_decode(M.IMA4, channels, p[:cut].tobytes())
            b, st2 = engine.aiff_decode(M.IMA4, channels, p[cut:].tobytes(), st)
            assert a + b == whole and st2[:channels] == wst[:channels], (channels, cut)


def test_ima4_fixture(engine):
    data = open(os.path.join(HERE, "golden", "aiff", "stream-ima4.aifc"), "rb").read()
    outs, m = M.decode_file(data)
    assert len(m.pieces[0]) == 370 * 34
    got, _ = engine.aiff_decode(M.IMA4, 1, m.pieces[0])
    assert got == outs[0].data


# ---- the tick -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_streams", [1, 64, 65, 300])
def test_tick_many_streams_unequal_lengths(engine, n_streams):
    """IMA4 and elementwise streams of unequal lengths in one tick, several units per stream, delivered as decoded: every record equals
    the model's decode of its unit, the IMA4 state chains through a stream's units and comes back in the stream's record"""
    rng = np.random.default_rng(40 + n_streams)
    streams, units, want, states = [], [], [], []
    for i in range(n_streams):
        kind = i % 4
        n_units = 1 + (i * 7) % 3
        if kind < 2:
            ch = 1 + kind
            st = [[int(rng.integers(-2000, 2000)), int(rng.integers(0, 89))] for _ in range(2)]
            streams.append({"encoding": M.IMA4, "channels": ch, "out_bits": 16, "out_channels": ch, "n_units": n_units,
                            "ima_state": [tuple(s) for s in st]})
            for u in range(n_units):
                p = B.ima4_packets(rng, 1 + (i * 13 + u * 29) % 90, ch).tobytes()
                units.append(p)
                want.append((i, M.decode(M.IMA4, ch, p, st), 16, ch, False))
            states.append([tuple(s) for s in st])
        else:
            enc = ELEMENTWISE[(i // 4) % len(ELEMENTWISE)]
            ch = 1 + (i // 8) % 5
            bits, fl = M.contract(enc)
            streams.append({"encoding": enc, "channels": ch, "out_bits": bits, "out_channels": ch, "n_units": n_units})
            for u in range(n_units):
                src = random_source(rng, enc, ch * (1 + (i * 17 + u * 5) % 700))
                units.append(src)
                want.append((i, M.decode(enc, ch, src), bits, ch, fl))
            states.append(None)
    recs = engine.tick_run_aiff(streams, units)
    assert len(recs) == len(want)
    for (si, status, frames, ch, bits, data, fl), (wi, wdata, wbits, wch, wfl) in zip(recs, want):
        assert (si, status, ch, bits, fl) == (wi, 0, wch, wbits, wfl)
        assert frames * ch * bits // 8 == len(wdata)
        assert same_f32(data, wdata) if wfl else data == wdata, si
    for s, st in zip(streams, states):
        if st is not None:
            assert s["ima_state"][:s["channels"]] == st[:s["channels"]]


def test_tick_conversions_equal_the_pcm_tick_on_decoded_pcm(engine):
    """a stream with something to change runs what sk_tick_run_pcm runs on the decoded PCM: same records, same bytes"""
    import soundkit_amd.engine as E
    rng = np.random.default_rng(50)
    fmt_of = {(16, False): E.FMT_S16LE, (24, False): E.FMT_S24LE, (32, False): E.FMT_S32LE, (32, True): E.FMT_F32LE}
    a_streams, a_units, p_streams, p_units = [], [], [], []
    for enc, ch, out_bits, out_ch in [(M.S24BE, 2, 16, 2), (M.S32BE, 1, 16, 1), (M.F64BE, 2, 16, 1), (M.IMA4, 2, 16, 1), (M.ULAW, 2, 24, 1),
                                      (M.U8, 1, 32, 1), (M.S16BE, 2, 16, 1), (M.F32BE, 1, 24, 1), (M.S16LE, 2, 32, 2), (M.S32LE, 2, 16, 2)]:
        n_units = 2
        st = [[0, 0], [0, 0]]
        a_streams.append({"encoding": enc, "channels": ch, "out_bits": out_bits, "out_channels": out_ch, "n_units": n_units})
        bits, fl = M.contract(enc)
        p_streams.append({"format": fmt_of[(bits, fl)], "channels": ch, "out_bits": out_bits, "out_channels": out_ch, "n_units": n_units})
        for u in range(n_units):
            if enc == M.IMA4:
                src = B.ima4_packets(rng, 70 + u, ch).tobytes()
            elif enc == M.F64BE:
                src = rng.uniform(-1.2, 1.2, ch * (4100 + u)).astype(">f8").tobytes()
            elif enc == M.F32BE:
                src = rng.uniform(-1.2, 1.2, ch * (4100 + u)).astype(">f4").tobytes()
            else:
                src = random_source(rng, enc, ch * (4100 + u))
            a_units.append(src)
            p_units.append(M.decode(enc, ch, src, st))
    got = engine.tick_run_aiff(a_streams, a_units)
    want = engine.tick_run_pcm(p_streams, p_units)
    assert got == want and len(got) == 20

"""The FLAC decode stage on the GPU (csrc/flac_decode.hip through sk_flac_decode_frames and FlacDecoder) against tests/flac_model.py,
bit for bit, at the smallest shapes that can still go wrong: every subframe type and predictor order the kernels take another path
for, full-scale material at every depth (the 64-bit accumulate), Rice parameters and partition layouts at their edges, escape
partitions, long unary runs, wasted bits, the stereo modes on odd sums, channel counts, large and one-sample blocks, many frames of
mixed length in one call, every rejection beside intact neighbours, and the reference's fixtures against their twins.

Every frame is written by tests/flac_builder.py from the samples the decoder must return; the model decodes it back to those samples
before the product is asked."""
import os
import random

import numpy as np
import pytest

import flac_builder as B
import flac_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "flac")
INVALID, UNSUPPORTED = -506, -6
RATE = 44100


def full_scale(bits, n):
    """+max, min, +max, ...: every product of the predictor is as large as the depth allows"""
    return [(1 << (bits - 1)) - 1 if i % 2 == 0 else -(1 << (bits - 1)) for i in range(n)]


def rand(rng, bits, n, scale=1.0):
    lim = max(int((1 << (bits - 1)) * scale), 1)
    return [rng.randrange(-lim, lim) for _ in range(n)]


def case(channels, bits, specs, assignment=None, number=0):
    """-> (frame bytes, channels, bits)"""
    return B.frame(channels, bits, RATE, number, specs, assignment=assignment), channels, bits


def expect(cases):
    """the model's decode of every case, checked against what the case was built from -> [(header dict for the product, frame bytes)],
    [contract bytes]"""
    frames, want = [], []
    for frame, channels, bits in cases:
        h, ch = M.decode_frame(frame, {"sample_rate": RATE, "bits_per_sample": bits})
        assert ch == [list(c) for c in channels] and h["frame_bytes"] == len(frame)
        frames.append((h, frame))
        want.append(M.contract_bytes(h, ch))
    return frames, want


def product_headers(frames):
    """the frames' headers as the product's own parser reads them (they agree with the model's)"""
    from soundkit_amd import flac
    out = []
    for h, frame in frames:
        rc, d = flac.parse_header(frame, flac.streaminfo(sample_rate=RATE, channels=h["channels"], bits_per_sample=h["bits_per_sample"]))
        assert rc == 0 and all(d[k] == h[k] for k in ("block_size", "channels", "assignment", "bits_per_sample", "header_bytes"))
        out.append((dict(d, frame_bytes=len(frame)), frame))
    return out


def run(engine, cases):
    frames, want = expect(cases)
    got, status = engine.flac_decode(product_headers(frames))
    assert status == [0] * len(cases)
    at = 0
    for i, w in enumerate(want):
        assert got[at:at + len(w)] == w, "frame %d of %d differs" % (i, len(want))
        at += len(w)
    assert at == len(got)


def lpc(order, precision, shift, coefs, **more):
    return dict({"type": "lpc", "order": order, "precision": precision, "shift": shift, "coefs": coefs, "params": "auto"}, **more)


def test_constant_verbatim_and_fixed_orders(engine):
    rng = random.Random(1)
    cases = [case([[-12345] * 16], 16, [{"type": "constant"}]), case([rand(rng, 16, 17)], 16, [{"type": "verbatim"}]),
             case([[0] * 192], 16, [{"type": "constant"}])]
    for order in range(5):
        for block in (16, 67, 192):
            cases.append(case([full_scale(16, block)], 16, [{"type": "fixed", "order": order, "params": "auto"}]))
            cases.append(case([rand(rng, 24, block)], 24, [{"type": "fixed", "order": order, "params": "auto", "porder": 0}]))
    run(engine, cases)


def test_lpc_orders_precisions_and_shifts(engine):
    """orders 1, 2, 8, 12 (history in registers), 13 and 32 (the general path) x precisions 1, 12, 15 x shifts 0 and 14"""
    rng = random.Random(2)
    cases = []
    for order in (1, 2, 8, 12, 13, 32):
        for precision in (1, 12, 15):
            for shift in (0, 14):
                # shift 0: small coefficients (the residual must fit 32 bits); shift 14: the whole range of the precision
                lim = 1 if precision == 1 else (3 if shift == 0 else 1 << (precision - 1))
                coefs = [rng.randrange(-lim, lim if precision > 1 else 1) for _ in range(order)]
                block = rng.choice((order, order + 1, 33, 64, 191, 192)) if order <= 33 else 64
                block = max(block, order)
                samples = full_scale(24, block) if shift else [rng.choice((-(1 << 23), (1 << 23) - 1, rng.randrange(-100, 100))) for _ in range(block)]
                cases.append(case([samples], 24, [lpc(order, precision, shift, coefs)]))
    assert len(cases) == 36
    run(engine, cases)


def test_every_depth_at_full_scale_needs_the_64_bit_accumulate(engine):
    cases = []
    for bits in (4, 8, 12, 16, 20, 24, 32):
        # the signal alternates, so does its prediction: sum of (-1)^j coef[j] = -16384 = -1.0 at shift 14
        coefs = [-16000, 384] + [0] * 6
        cases.append(case([full_scale(bits, 64)], bits, [lpc(8, 15, 14, coefs)]))
        cases.append(case([full_scale(bits, 48), full_scale(bits, 48)[::-1]], bits, [lpc(2, 15, 14, [-16384, 0]), {"type": "verbatim"}]))
    run(engine, cases)


def test_both_sides_of_the_32_bit_accumulate_bound(engine):
    """depth + precision + ceil(log2(order)) = 31, 32 and 33 with every product at full scale and of one sign"""
    cases = []
    for precision in (13, 14, 15):
        top = (1 << (precision - 1)) - 1
        coefs = [-top if j % 2 == 0 else top for j in range(4)]
        cases.append(case([full_scale(16, 96)], 16, [lpc(4, precision, precision - 1, coefs)]))
        cases.append(case([[-v - 1 for v in full_scale(16, 96)]], 16, [lpc(4, precision, precision - 1, [-c - 1 for c in coefs])]))
    run(engine, cases)


def test_rice_parameters_partitions_and_long_unary_runs(engine):
    rng = random.Random(3)
    cases = []
    fixed0 = {"type": "fixed", "order": 0}
    cases.append(case([[rng.randrange(-3, 4) for _ in range(64)]], 16, [dict(fixed0, params=0)]))
    cases.append(case([[rng.randrange(-9, 9) for _ in range(64)]], 16, [dict(fixed0, params=1)]))
    cases.append(case([rand(rng, 16, 64)], 16, [dict(fixed0, params=14)]))
    cases.append(case([rand(rng, 32, 64)], 32, [dict(fixed0, params=30, method=1)]))
    cases.append(case([rand(rng, 16, 64, 0.01)], 16, [dict(fixed0, params=[0, 3, 7, 10], method=1, porder=2)]))
    # unary runs of 33, 64, 65 and 200 zeros, alone and back to back
    cases.append(case([[0, -17, 32, 0, -33, 100, -100, 1] * 2], 16, [dict(fixed0, params=0)]))
    # partition orders 0, 1 and the largest the block allows (one sample per partition); with order 1 the first partition is empty
    for porder in (0, 1, 4):
        cases.append(case([rand(rng, 16, 16, 0.1)], 16, [{"type": "fixed", "order": 1 if porder == 4 else 2, "porder": porder, "params": "auto"}]))
    cases.append(case([rand(rng, 16, 64, 0.1)], 16, [{"type": "fixed", "order": 0, "porder": 6, "params": "auto"}]))
    cases.append(case([rand(rng, 16, 192, 0.1)], 16, [lpc(3, 12, 10, [1500, -700, 200], porder=6)]))  # first partition = the order
    cases.append(case([rand(rng, 16, 64, 0.1)], 16, [lpc(8, 12, 10, [1500, -700, 200, 10, -10, 5, 0, 1], porder=3)]))
    run(engine, cases)


def test_escape_partitions(engine):
    rng = random.Random(4)
    cases = []
    for method in (0, 1):
        cases.append(case([[77] * 32], 16, [{"type": "fixed", "order": 1, "method": method, "params": ("esc", 0)}]))
        cases.append(case([[rng.randrange(-1, 1) for _ in range(32)]], 16, [{"type": "fixed", "order": 0, "method": method, "params": ("esc", 1)}]))
        cases.append(case([full_scale(16, 32)], 16, [{"type": "fixed", "order": 0, "method": method, "params": ("esc", 16)}]))
        cases.append(case([rand(rng, 24, 64)], 24, [{"type": "fixed", "order": 0, "method": method, "porder": 2, "params": [("esc", 24), 23 if method else 14, ("esc", 24), ("esc", 25)]}]))
    cases.append(case([rand(rng, 32, 32, 0.4)], 32, [{"type": "fixed", "order": 0, "method": 1, "params": ("esc", 31)}]))
    cases.append(case([[0] * 16 + rand(rng, 16, 16)], 16, [{"type": "fixed", "order": 0, "porder": 1, "params": [("esc", 0), ("esc", 16)]}]))
    run(engine, cases)


def test_wasted_bits(engine):
    rng = random.Random(5)
    cases = [case([[v << 1 for v in rand(rng, 15, 48)]], 16, [{"type": "fixed", "order": 2, "params": "auto", "wasted": 1}]),
             case([[rng.choice((-32768, 0)) for _ in range(48)]], 16, [{"type": "verbatim", "wasted": 15}]),
             case([[-32768] * 16], 16, [{"type": "constant", "wasted": 15}]),
             case([[v << 8 for v in rand(rng, 16, 40)]], 24, [lpc(4, 12, 11, [2000, -900, 300, -50], wasted=8)])]
    # wasted bits on the side channel alone, on both, and on mid
    left = rand(rng, 15, 64)
    right = [l - (rng.randrange(-200, 200) << 3) for l in left]
    cases.append(case([left, right], 16, [{"type": "fixed", "order": 1, "params": "auto"}, {"type": "fixed", "order": 1, "params": "auto", "wasted": 3}], assignment=8))
    cases.append(case([left, right], 16, [{"type": "verbatim", "wasted": 3}, {"type": "fixed", "order": 0, "params": "auto"}], assignment=9))
    l4, r4 = [v << 2 for v in rand(rng, 13, 32)], [v << 2 for v in rand(rng, 13, 32)]
    cases.append(case([l4, r4], 16, [{"type": "verbatim", "wasted": 1}, {"type": "verbatim", "wasted": 2}], assignment=10))
    run(engine, cases)


def test_stereo_modes_with_odd_sums(engine):
    rng = random.Random(6)
    cases = []
    for bits in (8, 16, 24):
        left = [v | 1 for v in rand(rng, bits, 96)]          # odd
        right = [v & ~1 for v in rand(rng, bits, 96)]        # even: every sum is odd, the low bit of mid matters
        left[:4] = full_scale(bits, 4)
        right[:4] = full_scale(bits, 4)[::-1]
        fixed1, fixed2 = {"type": "fixed", "order": 1, "params": "auto"}, {"type": "fixed", "order": 2, "params": "auto"}
        for assignment in (1, 8, 9, 10):
            cases.append(case([left, right], bits, [fixed1, {"type": "verbatim"}], assignment=assignment))
        # equal channels: the side channel is all zeros, a CONSTANT subframe beside a predicted one
        cases.append(case([left, left], bits, [fixed2, {"type": "constant"}], assignment=8))
        cases.append(case([left, left], bits, [{"type": "constant"}, fixed2], assignment=9))
        cases.append(case([left, left], bits, [fixed2, {"type": "constant"}], assignment=10))
    run(engine, cases)


def test_channel_counts(engine):
    rng = random.Random(7)
    kinds = [{"type": "verbatim"}, {"type": "fixed", "order": 3, "params": "auto"}, lpc(5, 10, 8, [300, -100, 50, 20, -7]), {"type": "constant"}]
    cases = []
    for nch in (1, 2, 3, 6, 8):
        for bits in (8, 16, 24, 32):
            block = rng.choice((16, 31, 100))
            chans = [[rng.randrange(-100, 100)] * block if kinds[(c + nch) % 4]["type"] == "constant" else rand(rng, bits, block, 0.2 if bits < 32 else 0.02) for c in range(nch)]
            cases.append(case(chans, bits, [kinds[(c + nch) % 4] for c in range(nch)]))
    run(engine, cases)


def test_large_blocks_and_a_block_of_one_sample(engine):
    rng = random.Random(8)
    walk = [0]
    for _ in range(4607):
        walk.append(max(-30000, min(30000, walk[-1] + rng.randrange(-300, 300))))
    cases = [case([walk[:4096], walk[512:4608]], 16, [lpc(8, 13, 11, [3000, -1500, 400, 100, -60, 30, -10, 4], porder=4),
                                                      {"type": "fixed", "order": 2, "params": "auto", "porder": 8}], assignment=10),
             case([walk], 16, [lpc(12, 15, 13, [12000, -6000, 2000, -500, 100, 50, -20, 10, -5, 2, -1, 1], porder=8)]),
             case([[-5]], 16, [{"type": "verbatim"}]), case([[7], [-8]], 24, [{"type": "constant"}, {"type": "fixed", "order": 1, "params": 0}]),
             case([[100]], 8, [{"type": "fixed", "order": 0, "params": 3}])]
    run(engine, cases)


def test_130_frames_of_mixed_lengths_in_one_call_map_back_to_frame_order(engine):
    rng = random.Random(9)
    cases = []
    for i in range(130):
        bits = rng.choice((8, 16, 24))
        block = rng.choice((16, 17, 50, 192, 600)) if i % 13 else 1152
        nch = rng.choice((1, 2))
        kind = rng.choice(({"type": "verbatim"}, {"type": "fixed", "order": 2, "params": "auto"}, lpc(4, 12, 11, [2000, -900, 300, -50])))
        cases.append(case([rand(rng, bits, block, 0.3) for _ in range(nch)], bits, [kind] * nch, number=i))
    run(engine, cases)


def rejected_frames():
    """(name, frame bytes, header override, expected status)"""
    rng = random.Random(10)
    s = rand(rng, 16, 32, 0.1)
    good = lpc(4, 12, 11, [2000, -900, 300, -50])
    out = []
    for name, spec in (("reserved type 2", dict(good, raw_type=2)), ("reserved type 13", dict(good, raw_type=13)), ("reserved type 31", dict(good, raw_type=31)),
                       ("padding bit", dict(good, pad_bit=1)), ("negative shift", dict(good, raw_shift=0x1F)), ("precision code 15", dict(good, precision_code=15)),
                       ("reserved residual method", dict(good, method=2, params=3))):
        out.append((name, B.frame([s], 16, RATE, 0, [spec]), {}, INVALID))
    out.append(("partition order does not divide", B.frame([s[:24]], 16, RATE, 0, [{"type": "fixed", "order": 1, "porder": 4, "params": 9, "short_partitions": True}]), {}, INVALID))
    out.append(("first partition shorter than the order", B.frame([s[:16]], 16, RATE, 0, [{"type": "fixed", "order": 3, "porder": 3, "params": 9, "short_partitions": True}]), {}, INVALID))
    whole = B.frame([s], 16, RATE, 0, [{"type": "verbatim"}])
    out.append(("samples end beyond the frame", whole[:-10] + whole[-2:], {}, INVALID))
    out.append(("a unary run that leaves the frame", B.frame([[0] * 31 + [20000]], 16, RATE, 0, [{"type": "fixed", "order": 0, "params": 0}])[:40] + b"\0" * 30, {}, INVALID))
    out.append(("samples end 8 bits short of the frame", whole[:-2] + b"\0" + whole[-2:], {}, INVALID))
    odd = B.frame([[1, 2, 3]], 12, RATE, 0, [{"type": "verbatim"}])  # 8 + 36 bits: four padding bits
    out.append(("padding bits not zero", odd[:-3] + bytes([odd[-3] | 1]) + odd[-2:], {}, INVALID))
    out.append(("wasted bits use up the sample", B.frame([[0] * 16], 8, RATE, 0, [{"type": "verbatim", "wasted": 7}])[:7] + b"\x03\x01" + b"\0" * 8, {}, INVALID))
    out.append(("side channel with one channel", B.frame([s], 16, RATE, 0, [{"type": "verbatim"}]), {"assignment": 8}, INVALID))
    out.append(("mid/side with three channels", B.frame([s, s, s], 16, RATE, 0, [{"type": "verbatim"}] * 3), {"assignment": 10}, INVALID))
    big = rand(rng, 32, 16, 0.2)
    out.append(("32 bits with a side channel", B.frame([big, [v // 2 for v in big]], 32, RATE, 0, [{"type": "verbatim"}] * 2, assignment=8), {}, UNSUPPORTED))
    return out


def test_each_rejection_has_its_status_and_the_neighbours_stay_exact(engine):
    from soundkit_amd import flac
    rng = random.Random(11)
    good = [case([rand(rng, 16, 50)], 16, [{"type": "fixed", "order": 2, "params": "auto"}]) for _ in range(3)]
    good_frames, good_want = expect(good)
    good_frames = product_headers(good_frames)
    bad = rejected_frames()
    frames, want, want_status = [], [], []
    for i, (name, frame, override, status) in enumerate(bad):
        rc, d = flac.parse_header(frame, flac.streaminfo(sample_rate=RATE, channels=1, bits_per_sample=16))
        assert rc == 0, name
        if not override:  # the model rejects it too, or finds that the frame ends elsewhere
            try:
                assert M.decode_frame(frame, {"sample_rate": RATE, "bits_per_sample": 16}, check_crc=False)[0]["frame_bytes"] != len(frame), name
            except M.FlacError:
                pass
        d = dict(d, frame_bytes=len(frame), **override)
        frames += [good_frames[i % 3], (d, frame)]
        want += [good_want[i % 3], b"\xa5" * flac.out_bytes([(d, frame)])]
        want_status += [0, status]
    frames.append(good_frames[0])
    want.append(good_want[0])
    want_status.append(0)
    got, status = flac.decode_frames(frames, engine=engine, fill=0xA5)
    assert [(n, s) for (n, _, _, _), s in zip(bad, status[1::2])] == [(n, s) for n, _, _, s in bad]
    assert status == want_status
    assert got == b"".join(want)  # a rejected frame wrote nothing, its neighbours everything


def test_bad_frame_tables_are_refused_before_anything_runs(engine):
    import soundkit_amd
    from soundkit_amd import flac
    frames, _ = expect([case([[1] * 16], 16, [{"type": "constant"}])])
    (d, b), = product_headers(frames)
    for override in ({"channels": 0}, {"channels": 9}, {"bits_per_sample": 3}, {"bits_per_sample": 33}, {"block_size": 0}, {"block_size": 65537},
                     {"header_bytes": len(b)}):
        with pytest.raises(soundkit_amd.SoundkitError):
            flac.decode_frames([(dict(d, **override), b)], engine=engine)
    assert flac.decode_frames([], engine=engine) == (b"", [])


@pytest.fixture(scope="module")
def twin():
    return open(os.path.join(HERE, "golden", "linear16_A_Tusk.s16le"), "rb").read()


def test_the_fixture_against_its_twin(engine, twin):
    from soundkit_amd import flac
    data = open(os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts.flac"), "rb").read()
    r = flac.FlacReader()
    frames = r.add(data) + r.add(b"")
    r.close()
    got, status = engine.flac_decode(frames)
    assert len(frames) == 42 and status == [0] * 42 and got == twin


def test_the_headerless_fixtures_against_their_twins(engine, twin):
    from soundkit_amd import flac
    stereo = open(os.path.join(HERE, "golden", "wav_stereo_A_Tusk.wav"), "rb").read()
    stereo = stereo[stereo.index(b"data") + 8:]
    shifted = (np.frombuffer(twin[:45056 * 2], "<i2").astype(np.int32) << 8).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    for name, want in (("16bit", stereo[:45056 * 4]), ("24bit", shifted), ("32float", None)):
        data = open(os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts_%s.flac" % name), "rb").read()
        rc, found, used = flac.scan(data, final=True)  # no STREAMINFO: the headers describe themselves
        assert rc == 0 and len(found) == 11 and used == len(data)
        got, status = engine.flac_decode([(d, data[d["offset"]:d["offset"] + d["frame_bytes"]]) for d in found])
        assert status == [0] * 11
        if want is None:  # no twin: the model, which the CRCs and the other fixtures pin
            want = b"".join(M.contract_bytes(h, ch) for h, ch in M.decode_frames(data))
        assert got == want, name


# ---- FlacDecoder ---------------------------------------------------------------------------------------------------------------------------

def decode_all(dec, data, piece, dtype, cap):
    out = np.zeros(cap, dtype)
    fn = dec.decode_i16 if dtype == np.int16 else dec.decode_i32
    got = []
    for at in range(0, len(data), piece):
        n = fn(data[at:at + piece], out)
        got.append(out[:n].copy())
    while True:
        n = fn(b"", out)
        if n == 0:
            break
        got.append(out[:n].copy())
    return np.concatenate(got) if got else np.zeros(0, dtype)


def test_decoder_on_the_fixture_at_any_chunking(engine, twin):
    from soundkit_amd import flac
    data = open(os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts.flac"), "rb").read()
    want = np.frombuffer(twin, "<i2")
    dec = flac.FlacDecoder(engine=engine)
    assert dec.sample_rate() is None and dec.channels() is None and dec.bits_per_sample() is None
    assert np.array_equal(decode_all(dec, data, len(data), np.int16, 1 << 16), want)
    assert (dec.sample_rate(), dec.channels(), dec.bits_per_sample(), dec.frames_decoded()) == (16000, 1, 16, 42)
    for piece, cap, dtype in ((4096, 1 << 16, np.int32), (777, 1152, np.int16), (len(data), 2500, np.int32)):
        dec.reset()
        assert dec.sample_rate() is None
        assert np.array_equal(decode_all(dec, data, piece, dtype, cap), want.astype(dtype)), (piece, cap)
    dec.close()


def test_decoder_fetches_waiting_frames_in_the_middle_of_a_stream(engine, twin):
    """an output that holds one frame, pieces that bring several: the frames that wait are fetched with empty calls, and more input follows"""
    from soundkit_amd import flac
    data = open(os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts.flac"), "rb").read()
    dec, out, got, most = flac.FlacDecoder(engine=engine), np.zeros(1152, np.int16), [], 0
    for at in range(0, len(data), 6000):
        n = dec.decode_i16(data[at:at + 6000], out)
        got.append(out[:n].copy())
        most = max(most, dec.pending_samples())
        while dec.pending_samples():
            n = dec.decode_i16(b"", out)
            assert n > 0
            got.append(out[:n].copy())
    assert most >= 3 * 1152
    while True:  # nothing waits: the empty call is the finalising one
        n = dec.decode_i16(b"", out)
        if n == 0:
            break
        got.append(out[:n].copy())
    assert dec.frames_decoded() == 42 and np.array_equal(np.concatenate(got), np.frombuffer(twin, "<i2"))
    dec.close()


def test_decoder_i16_is_i32_clamped_and_small_outputs_are_refused(engine):
    import soundkit_amd
    from soundkit_amd import flac
    rng = random.Random(12)
    blocks = [[full_scale(24, 40), rand(rng, 24, 40)], [rand(rng, 24, 64, 0.001), full_scale(24, 64)[::-1]]]
    data, _ = B.stream(blocks, 24, 48000, lambda i, ch: [{"type": "fixed", "order": 1, "params": "auto"}, {"type": "verbatim"}], assignment=10)
    want = np.array([v for ch in blocks for v in M.interleave(ch)], np.int32)
    dec = flac.FlacDecoder(engine=engine)
    assert np.array_equal(decode_all(dec, data, 100, np.int32, 4096), want)
    assert (dec.sample_rate(), dec.channels(), dec.bits_per_sample()) == (48000, 2, 24)
    dec.reset()
    assert np.array_equal(decode_all(dec, data, len(data), np.int16, 4096), np.clip(want, -32768, 32767).astype(np.int16))
    dec.reset()
    with pytest.raises(soundkit_amd.SoundkitError) as exc:  # the first frame has 80 samples
        dec.decode_i32(data, np.zeros(79, np.int32))
    assert exc.value.status == -7
    assert dec.decode_i32(b"", np.zeros(80, np.int32)) == 80  # nothing was lost
    dec.close()


def test_decoder_errors_carry_a_text(engine):
    import soundkit_amd
    from soundkit_amd import flac
    rng = random.Random(13)
    blocks = [[rand(rng, 16, 32)] for _ in range(3)]
    data, frames = B.stream(blocks, 16, 16000, lambda i, ch: [dict(lpc(4, 12, 11, [2000, -900, 300, -50]), **({"raw_shift": 0x1F} if i == 1 else {}))])
    dec = flac.FlacDecoder(engine=engine)
    with pytest.raises(soundkit_amd.SoundkitError) as exc:
        decode_all(dec, data, len(data), np.int32, 4096)
    assert exc.value.status == flac.ERR_STREAM and "frame 1" in dec.last_error()
    with pytest.raises(soundkit_amd.SoundkitError):
        dec.decode_i32(b"", np.zeros(64, np.int32))
    dec.reset()
    bad = bytearray(data)
    bad[-5] ^= 4  # the framer's CRC-16
    with pytest.raises(soundkit_amd.SoundkitError) as exc:
        decode_all(dec, bytes(bad), len(bad), np.int32, 4096)
    assert exc.value.status == flac.ERR_STREAM and dec.last_error()
    dec.close()

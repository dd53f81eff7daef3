"""tests/f64_ref.py pinned against the C oracle: every float64 reference agrees with the oracle's f32 restatement of the same
operation to f32 accuracy (the IMDCT with the oracle's own f64 evaluation to 1e-12, the s16 narrowing bit for bit), and a
negative control -- one window coefficient or tap changed, or the FIR's alignment moved by one input sample -- fails the
same bound.  CPU only."""
import numpy as np
import pytest

import f64_ref as R


def test_imdct_equals_the_oracle_f64_direct_form(oracle):
    for n, seed in ((1024, 3), (1024, 0x9E3779B9), (128, 11), (128, 12)):
        x = oracle.seeded_spectrum(n, seed) * np.float32(2500.0)
        want = oracle.imdct_direct_f64(x)
        got = R.imdct(x)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), n
    batch = np.stack([oracle.seeded_spectrum(1024, s) for s in range(5)])
    assert np.array_equal(R.imdct(batch)[3], R.imdct(batch[3]))


def _mixed_batch(oracle, channels, frames):
    """every window sequence and shape pair: LongStart, one to three EightShort, LongStop in brackets, both shapes in turn"""
    rng = np.random.default_rng(8)
    coeffs = np.stack([[oracle.seeded_spectrum(1024, 0x51 + 131 * c + f) * np.float32(4000.0) for f in range(frames)]
                       for c in range(channels)])
    brackets = [[0], [1, 2, 3], [1, 2, 2, 3], [0, 0], [1, 2, 2, 2, 3]]
    seqs = np.zeros((channels, frames), np.uint8)
    for c in range(channels):
        row = []
        while len(row) < frames:
            row += brackets[(c + len(row)) % len(brackets)]
        seqs[c] = row[:frames]
    shapes = rng.integers(0, 2, (channels, frames)).astype(np.uint8)
    return coeffs, seqs, shapes


def _oracle_synth(oracle, coeffs, seqs, shapes, state=None):
    out = np.empty(coeffs.shape, np.float32)
    for c in range(coeffs.shape[0]):
        ch = oracle.Channel()
        if state is not None:
            ch.set_state(state[0][c].astype(np.float32), int(state[1][c]))
        for f in range(coeffs.shape[1]):
            out[c, f] = ch.synthesize(coeffs[c, f], seqs[c, f], shapes[c, f])
    return out


def test_synthesis_within_f32_accuracy_of_the_oracle(oracle):
    coeffs, seqs, shapes = _mixed_batch(oracle, 10, 14)
    assert set(np.unique(seqs)) == {0, 1, 2, 3} and set(np.unique(shapes)) == {0, 1}
    want = _oracle_synth(oracle, coeffs, seqs, shapes)
    got, delay, prev = R.synthesize(coeffs, seqs, shapes)
    for c in range(coeffs.shape[0]):
        assert R.rel_rms(want[c], got[c]) < 2e-7, c
    # a given initial state (the carried delay and window shape), and the state handed on: two halves equal the whole
    a, da, pa = R.synthesize(coeffs[:, :6], seqs[:, :6], shapes[:, :6])
    b, db, pb = R.synthesize(coeffs[:, 6:], seqs[:, 6:], shapes[:, 6:], da, pa)
    assert np.array_equal(np.concatenate([a, b], 1), got) and np.array_equal(db, delay) and np.array_equal(pb, prev)
    start = (np.random.default_rng(3).uniform(-0.5, 0.5, (10, 1024)), np.arange(10) & 1)
    want_s = _oracle_synth(oracle, coeffs[:, 6:], seqs[:, 6:], shapes[:, 6:],
                           (start[0].astype(np.float32), start[1]))
    got_s, _, _ = R.synthesize(coeffs[:, 6:], seqs[:, 6:], shapes[:, 6:], start[0].astype(np.float32), start[1])
    assert max(R.rel_rms(want_s[c], got_s[c]) for c in range(10)) < 2e-7


@pytest.mark.parametrize("which", ["long_first", "long_second", "short", "long_start"])
def test_synthesis_negative_control(oracle, which):
    """one window coefficient changed by 1 % fails the 2e-7 bound"""
    coeffs, seqs, shapes = _mixed_batch(oracle, 10, 14)
    want = _oracle_synth(oracle, coeffs, seqs, shapes)
    first, second, short = (w.copy() for w in R.windows())
    if which == "long_first":
        first[0, 1, 700] *= 1.01
    elif which == "long_second":
        second[0, 0, 300] *= 1.01
    elif which == "short":
        short[1, 200] *= 1.01
    else:
        second[1, :, 500] *= 1.01
    got, _, _ = R.synthesize(coeffs, seqs, shapes, win=(first, second, short))
    assert max(R.rel_rms(want[c], got[c]) for c in range(coeffs.shape[0])) > 2e-7


def test_float_sample_to_i16_bit_for_bit(oracle):
    pins = [1.0, -1.0, 2.0, -2.0, np.nan, np.inf, -np.inf, 0.5, -0.5, 0.25, -0.25, 1.0e-6, 0.0, -0.0, 1e-30, -1e-30]
    halves = (np.arange(-32768, 32768) + 0.5)
    x = np.concatenate([np.array(pins, np.float32),
                        (halves / 32767.0).astype(np.float32), (halves / 32768.0).astype(np.float32),
                        np.nextafter((halves / 32767.0).astype(np.float32), np.float32(0)),
                        np.random.default_rng(5).uniform(-1.3, 1.3, 1 << 20).astype(np.float32),
                        np.random.default_rng(6).integers(0, 1 << 32, 1 << 18, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    got = R.float_sample_to_i16(x)
    assert np.array_equal(got, oracle.pcm_convert("FLOAT_TO_I16_ROUND", x))
    assert all(R.float_sample_to_i16(np.float32(p)) == oracle.float_sample_to_i16(p) for p in pins)
    assert R.float_sample_to_i16(np.float32(0.5)) == 16384 and R.float_sample_to_i16(np.float32(-0.5)) == -16384


def test_fir_within_f32_accuracy_of_the_oracle(oracle):
    x = np.random.default_rng(2024).uniform(-1, 1, (6, 7001)).astype(np.float32)
    want = oracle.downsample_planar(x, 48000, 16000)
    got = R.fir_48k_16k(x, want.shape[1])
    assert R.rel_rms(want, got) < 2e-7 and np.abs(want - got).max() < 1e-6
    # the same result for rows given as s16, through s / 32768
    q = (x * 32767).astype(np.int16)
    assert np.array_equal(R.s16_chain(q, want.shape[1]), R.fir_48k_16k(q.astype(np.float64) / 32768.0, want.shape[1]))


@pytest.mark.parametrize("which", ["delay-1", "delay+1", "tap"])
def test_fir_negative_control(oracle, which):
    x = np.random.default_rng(2024).uniform(-1, 1, (6, 7001)).astype(np.float32)
    want = oracle.downsample_planar(x, 48000, 16000)
    if which == "tap":
        taps = oracle.resampler_taps(16000 / 48000).astype(np.float64)
        taps[131] *= 1.001
        got = R.fir_48k_16k(x, want.shape[1], taps=taps)
    else:
        got = R.fir_48k_16k(x, want.shape[1], delay=R.FIR_DELAY + (1 if which == "delay+1" else -1))
    assert R.rel_rms(want, got) > 2e-7


RATIOS = [(44100, 16000), (16000, 48000), (48000, 44100)]


@pytest.mark.parametrize("in_hz,out_hz", RATIOS)
def test_sinc_walk_within_f32_accuracy_of_the_oracle(oracle, in_hz, out_hz):
    x = np.random.default_rng(in_hz + out_hz).uniform(-1, 1, (3, 12000)).astype(np.float32)
    want = oracle.downsample_planar(x, in_hz, out_hz)
    got = R.sinc_resample(x, in_hz, out_hz)
    assert got.shape == want.shape
    assert R.rel_rms(want, got) < 2e-7 and np.abs(want - got).max() < 1e-6


@pytest.mark.parametrize("in_hz,out_hz", RATIOS)
def test_sinc_walk_negative_control(oracle, in_hz, out_hz):
    x = np.random.default_rng(in_hz + out_hz).uniform(-1, 1, (3, 12000)).astype(np.float32)
    want = oracle.downsample_planar(x, in_hz, out_hz)
    sincs = oracle.resampler_sincs(out_hz / in_hz).astype(np.float64)
    sincs[:, 128] *= 1.001  # the centre tap of every sub-filter
    got = R.sinc_resample(x, in_hz, out_hz, sincs=sincs)
    assert R.rel_rms(want, got) > 2e-7


def test_fir_at_columns_equals_the_whole_filter(oracle):
    x = np.random.default_rng(9).uniform(-1, 1, (300, 5000)).astype(np.float32)
    want = R.fir_48k_16k(x, 1623)
    cols = np.array([0, 1, 31, 700, 1590, 1622])
    got = R.fir_48k_16k_at(x, cols, block=128)
    assert np.abs(got - want[:, cols]).max() < 1e-12


def test_float_sample_to_i16_torch_form_bit_for_bit(oracle):
    import torch
    x = np.concatenate([np.array([1.0, -1.0, 2.0, np.nan, np.inf, -np.inf, 0.5, -0.5, 1e-30], np.float32),
                        ((np.arange(-32768, 32768) + 0.5) / 32767.0).astype(np.float32),
                        np.random.default_rng(4).uniform(-1.3, 1.3, 1 << 18).astype(np.float32)])
    got = R.float_sample_to_i16_torch(torch.from_numpy(x)).numpy()
    assert np.array_equal(got, oracle.pcm_convert("FLOAT_TO_I16_ROUND", x))


def _mp3_batch(channels=8, granules=6):
    rng = np.random.default_rng(0)
    xr = rng.standard_normal((channels, granules, 576)) * 0.05
    bts = np.array([[0, 1, 2, 2, 3, 0], [2] * 6, [1, 3, 1, 3, 0, 0], [3, 2, 1, 0, 2, 3], [0] * 6, [2, 3, 0, 1, 2, 2],
                    [1, 2, 3, 0, 1, 2], [2, 2, 3, 3, 2, 2]])[:channels, :granules]
    mixed = np.zeros((channels, granules), int)
    mixed[1], mixed[5, 4:], mixed[7, :2] = 1, 1, 1
    return xr, bts, mixed * (bts == 2)


def _mp3_oracle(xr, bts, mixed, d512):
    from oracle import mp3_hybrid as M
    out = np.empty(xr.shape)
    for c in range(xr.shape[0]):
        ch = M.Channel()
        for g in range(xr.shape[1]):
            out[c, g] = ch.granule(xr[c, g], bts[c, g], mixed[c, g], d512)
    return out


def test_mp3_hybrid_equals_the_oracle_filterbank():
    """every block type, mixed blocks, the state carried over six granules: the vectorised form is oracle/mp3_hybrid.py to 1e-12"""
    from oracle import mp3_hybrid as M
    d512 = M.synthetic_window(7)
    xr, bts, mixed = _mp3_batch()
    want = _mp3_oracle(xr, bts, mixed, d512)
    got, _, _ = R.mp3_hybrid(xr, bts, mixed, d512)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    a, ov, v = R.mp3_hybrid(xr[:, :3], bts[:, :3], mixed[:, :3], d512)
    b, _, _ = R.mp3_hybrid(xr[:, 3:], bts[:, 3:], mixed[:, 3:], d512, ov, v)
    assert np.array_equal(np.concatenate([a, b], 1), got)


@pytest.mark.parametrize("which", ["window_d", "mixed_flag"])
def test_mp3_hybrid_negative_control(which):
    from oracle import mp3_hybrid as M
    d512 = M.synthetic_window(7)
    xr, bts, mixed = _mp3_batch()
    want = _mp3_oracle(xr, bts, mixed, d512)
    if which == "window_d":
        d512 = d512.copy()
        d512[300] *= 1.0001
    else:
        mixed = np.zeros_like(mixed)
    got, _, _ = R.mp3_hybrid(xr, bts, mixed, d512)
    assert np.abs(got - want).max() > 1e-9 * np.abs(want).max()


def test_mp3_requant_is_the_oracle_granule_by_granule():
    """the process-pool form returns requantize_granule's values in order (mid/side, intensity, mixed short blocks)"""
    from oracle import mp3_bitstream
    rng = np.random.default_rng(3)
    long_o = np.array([0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 52, 62, 74, 90, 110, 134, 162, 196, 238, 288, 342, 418, 576], np.uint16)
    short_o = np.array([0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 54, 66, 80, 192], np.uint16)
    pretab = rng.integers(0, 5, 22).astype(np.uint8)
    granules, quant = [], []
    for k in range(12):
        bt = k % 4
        chans = [{"global_gain": int(rng.integers(120, 220)), "scalefac_scale": k & 1, "preflag": 0, "block_type": bt,
                  "mixed_block_flag": int(bt == 2 and k >= 6), "subblock_gain": [1, 0, 2],
                  "scalefac_l": [int(v) for v in rng.integers(0, 8, 21)] + [0],
                  "scalefac_s": [[int(v) for v in rng.integers(0, 8, 3)] for _ in range(12)] + [[0, 0, 0]]} for _ in range(2)]
        granules.append({"sample_rate": 44100, "channels": 2, "ms_stereo": k % 3 == 1, "intensity_stereo": k % 3 == 2, "ch": chans})
        q = rng.integers(-20, 21, (2, 576))
        q[1, 300 + 10 * k:] = 0
        quant.append(q)
    quant = np.concatenate(quant).astype(np.int16)
    got = R.mp3_requant(granules, quant, long_o, short_o, pretab, processes=2)
    want = np.concatenate([mp3_bitstream.requantize_granule(g, quant[2 * i:2 * i + 2], long_o, short_o, pretab)
                           for i, g in enumerate(granules)])
    assert np.array_equal(got, want) and np.abs(want).max() > 0

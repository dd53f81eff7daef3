"""The generic-ratio matrix-core resampler on the decode tail's own data: planar s16 frames in (the layout
sk_aac_plan_run_s16_planar_dev writes), interleaved s16 or f32 rows out, any pair of the common rates the matrix form takes.

  sk_downsample_frames_s16_to_f32_dev   k_sinc_taps<f16> + k_sinc_mfma_s16: two f16 planes per operand, three products per window
  sk_downsample_frames_s16_to_s16_dev   the same with float_sample_to_i16 and the interleave in the epilogue

The f64 reference below is the exact operation (one-shot downsample_audio: rubato's index walk from -128, the two nearest of 256
sub-filters of the oracle's table blended by the sub-phase), with every sum in float64.
"""
import numpy as np
import pytest

import soundkit_amd
from soundkit_amd._lib import SoundkitError

pytestmark = pytest.mark.gpu

RATES = [8000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000]
UNSUPPORTED, INVALID_ARG = -6, -1
PLANTED = [32767, -32768, 0, 1, -1, 255]

_SINCS = {}


def sincs_of(oracle, in_hz, out_hz):
    if (in_hz, out_hz) not in _SINCS:
        _SINCS[(in_hz, out_hz)] = oracle.resampler_sincs(out_hz / in_hz).astype(np.float64)
    return _SINCS[(in_hz, out_hz)]


def walk(frames, in_hz, out_hz):
    """the f64 index of every output: advanced by in_hz / out_hz from -128 before each one, while below frames - 257 - ceil(step)"""
    ratio = out_hz / in_hz
    step = 1.0 / ratio
    end = frames - 257 - int(np.ceil(step))
    idx, out = -128.0, []
    while idx < end:
        idx += step
        out.append(idx)
    return np.array(out, np.float64)


def f64_reference(x16, in_hz, out_hz, sincs, block=512):
    """x16 [R][T] int16 -> [R][n] float64: want = (1 - frac) sum_p sincs[sub][p] x[i0 + p] + frac sum_p sincs[sub + 1][p] x[i0 + p]
    (sub = 255: sincs[0] on x[i0 + 1 + p]), x = s / 32768, zero outside the input"""
    x16 = np.asarray(x16)
    r, t = x16.shape
    idx = walk(t, in_hz, out_hz)
    n = idx.size
    i0 = np.floor(idx).astype(np.int64)
    ph = (idx - np.floor(idx)) * 256.0
    sub = np.floor(ph).astype(np.int64)
    frac = ph - sub
    pad = 640
    xp = np.concatenate([np.zeros((r, pad)), x16.astype(np.float64) / 32768.0, np.zeros((r, pad))], axis=1)
    out = np.empty((r, n))
    p = np.arange(256)
    for a in range(0, n, block):
        b = min(n, a + block)
        lo, hi = int(i0[a]), int(i0[b - 1]) + 258
        g = np.zeros((b - a, hi - lo))
        rows = np.arange(b - a)[:, None]
        s0, s1 = sub[a:b], sub[a:b] + 1
        shift = (s1 >= 256).astype(np.int64)
        s1 = s1 & 255
        g[rows, (i0[a:b] - lo)[:, None] + p] += (1.0 - frac[a:b])[:, None] * sincs[s0]
        g[rows, (i0[a:b] - lo + shift)[:, None] + p] += frac[a:b][:, None] * sincs[s1]
        out[:, a:b] = xp[:, lo + pad:hi + pad] @ g.T
    return out


def rel_rms(got, want):
    return float(np.sqrt(np.mean((np.asarray(got, np.float64) - want) ** 2) / np.mean(want ** 2)))


def pack(x, layout):
    """x [streams][frames][ch][1024] -> the device image and (stream_stride, frame_stride)"""
    n_streams, n_frames, ch, _ = x.shape
    if layout == "frame":
        return np.ascontiguousarray(x.transpose(1, 0, 2, 3)), (ch * 1024, n_streams * ch * 1024)
    return np.ascontiguousarray(x), (n_frames * ch * 1024, ch * 1024)


def rows_of(x):
    """[streams][frames][ch][1024] -> [streams * ch][frames * 1024]: row s * ch + c"""
    n_streams, n_frames, ch, _ = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(n_streams * ch, n_frames * 1024)


def full_range_rows(ch, n_streams, n_frames):
    rng = np.random.default_rng(101 + 7 * ch + n_streams + n_frames)
    x = rng.integers(-32768, 32768, (n_streams, n_frames, ch, 1024), dtype=np.int64).astype(np.int16)
    x[0, 0, 0, :6] = PLANTED
    x[n_streams - 1, :, ch - 1, :] = -32768   # one row is all -32768
    return x


def run_both(engine, x, layout, in_hz, out_hz, o_pad=8, f_pad=4):
    """both forms on the same input and arguments -> (n_out, f32 [rows][f_stride], s16 [streams][o_stride][ch]) on the host"""
    import torch
    n_streams, n_frames, ch, _ = x.shape
    packed, strides = pack(x, layout)
    d_in = torch.from_numpy(packed).cuda()
    n_out = engine.downsample_out_frames(n_frames * 1024, in_hz, out_hz)
    f_stride = (n_out + f_pad - 1) // f_pad * f_pad + (0 if f_pad > 1 else 3)
    o_stride = (n_out + o_pad - 1) // o_pad * o_pad + (0 if o_pad > 1 else 5)
    d_f32 = torch.zeros((n_streams * ch, f_stride), device="cuda")
    d_s16 = torch.zeros((n_streams, o_stride, ch), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    assert engine.downsample_frames_s16_to_f32_dev(d_in, strides[0], strides[1], ch, n_streams, n_frames, in_hz, out_hz, d_f32, f_stride) == n_out
    assert engine.downsample_frames_s16_to_s16_dev(d_in, strides[0], strides[1], ch, n_streams, n_frames, in_hz, out_hz, d_s16, o_stride) == n_out
    engine.synchronize()
    return n_out, d_f32.cpu().numpy(), d_s16.cpu().numpy()


# (ch, streams, frames, layout): 74 rows (no multiple of 32); one frame (a partial last tile, every staged span past the input's
# end); 150 rows (several 32-row blocks per workgroup run, the last one partial); both layouts (a staged span crosses frame
# boundaries whose stride differs)
SHAPES = [(2, 37, 5, "stream"), (1, 21, 3, "frame"), (2, 16, 1, "frame"), (1, 150, 2, "stream")]
# 44.1 -> 16: fractional step; 48 -> 8: step 6, phase always 0, the most windows per tile; 22.05 -> 16: the fewest windows;
# 32 -> 16; 16 -> 24: up-sampling
PAIRS = [(44100, 16000), (48000, 8000), (22050, 16000), (32000, 16000), (16000, 24000)]


@pytest.mark.parametrize("ch,n_streams,n_frames,layout", SHAPES)
@pytest.mark.parametrize("in_hz,out_hz", PAIRS)
def test_against_f64_and_the_s16_form_is_the_rounded_f32_form(engine, oracle, in_hz, out_hz, ch, n_streams, n_frames, layout):
    """full-range s16 rows with the extremes planted, one row all -32768: the f32 form <= 1e-6 relative RMS per stream against the
    f64 evaluation; the s16 form = float_sample_to_i16 (the oracle's) of the f32 form of the same call arguments, bit for bit;
    nothing written at or beyond n_out.  The mono shapes use output strides that leave rows at 4-byte and at odd-sample boundaries
    (the narrower store paths of the epilogue)."""
    x = full_range_rows(ch, n_streams, n_frames)
    o_pad, f_pad = {(2, 37): (8, 4), (1, 21): (2, 1), (2, 16): (8, 4), (1, 150): (1, 4)}[(ch, n_streams)]
    n_out, f32, s16 = run_both(engine, x, layout, in_hz, out_hz, o_pad, f_pad)
    assert n_out == len(walk(n_frames * 1024, in_hz, out_hz)) == soundkit_amd.Engine.downsample_out_frames(n_frames * 1024, in_hz, out_hz)
    assert n_out > 0
    assert not f32[:, n_out:].any() and not s16[:, n_out:].any()
    want = f64_reference(rows_of(x), in_hz, out_hz, sincs_of(oracle, in_hz, out_hz)).reshape(n_streams, ch, n_out)
    got = f32[:, :n_out].reshape(n_streams, ch, n_out)
    worst = max(rel_rms(got[s], want[s]) for s in range(n_streams))
    print("rel. RMS against f64, worst stream: %.3g (%d -> %d Hz, %s)" % (worst, in_hz, out_hz, (ch, n_streams, n_frames, layout)))
    for s in range(n_streams):
        assert np.array_equal(s16[s, :n_out], oracle.planar_f32_to_s16_interleaved(got[s]).reshape(n_out, ch)), s
    assert worst <= 1e-6, worst
    # the all -32768 row: its pass band gain is one -- it reaches -32768 without wrapping
    last = s16[n_streams - 1, :n_out, ch - 1].astype(np.int32)
    assert last.min() == -32768 and last[n_out // 4:n_out // 2].max() < -32000


def test_every_pair_of_the_common_rates_at_the_smallest_shape(engine, oracle):
    """every pair of the nine common rates on 16 stereo streams of one frame: a pair the entry accepts meets the f64 bound and the
    s16 identity, a pair it refuses is SK_ERR_UNSUPPORTED with nothing written -- never a wrong answer"""
    import torch
    ch, n_streams, n_frames, layout = 2, 16, 1, "frame"
    x = full_range_rows(ch, n_streams, n_frames)
    packed, strides = pack(x, layout)
    d_in = torch.from_numpy(packed).cuda()
    refused = []
    for in_hz in RATES:
        for out_hz in RATES:
            if (in_hz, out_hz) in PAIRS or (in_hz, out_hz) == (48000, 16000):
                continue
            n_out = engine.downsample_out_frames(n_frames * 1024, in_hz, out_hz)
            stride = (n_out + 7) // 8 * 8
            d_f32 = torch.zeros((n_streams * ch, stride), device="cuda")
            d_s16 = torch.zeros((n_streams, stride, ch), dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            try:
                got_n = engine.downsample_frames_s16_to_f32_dev(d_in, strides[0], strides[1], ch, n_streams, n_frames, in_hz, out_hz, d_f32, stride)
            except SoundkitError as err:
                assert err.status == UNSUPPORTED, (in_hz, out_hz, err.status)
                with pytest.raises(SoundkitError) as err2:
                    engine.downsample_frames_s16_to_s16_dev(d_in, strides[0], strides[1], ch, n_streams, n_frames, in_hz, out_hz, d_s16, stride)
                assert err2.value.status == UNSUPPORTED
                engine.synchronize()
                assert not d_f32.any() and not d_s16.any()
                refused.append((in_hz, out_hz))
                continue
            assert engine.downsample_frames_s16_to_s16_dev(d_in, strides[0], strides[1], ch, n_streams, n_frames, in_hz, out_hz, d_s16, stride) == n_out
            engine.synchronize()
            assert got_n == n_out == len(walk(n_frames * 1024, in_hz, out_hz)) and n_out > 0
            f32, s16 = d_f32.cpu().numpy(), d_s16.cpu().numpy()
            assert not f32[:, n_out:].any() and not s16[:, n_out:].any()
            want = f64_reference(rows_of(x), in_hz, out_hz, sincs_of(oracle, in_hz, out_hz)).reshape(n_streams, ch, n_out)
            got = f32[:, :n_out].reshape(n_streams, ch, n_out)
            worst = max(rel_rms(got[s], want[s]) for s in range(n_streams))
            assert worst <= 1e-6, (in_hz, out_hz, worst)
            for s in range(n_streams):
                assert np.array_equal(s16[s, :n_out], oracle.planar_f32_to_s16_interleaved(got[s]).reshape(n_out, ch)), (in_hz, out_hz, s)
    # the steps the matrix form does not take (beyond about 6.9), as the header says
    assert refused == [(88200, 8000), (96000, 8000)], refused


@pytest.mark.parametrize("ch,n_streams,n_frames,layout", SHAPES)
@pytest.mark.parametrize("in_hz,out_hz", [(44100, 16000), (48000, 8000), (22050, 16000)])
def test_against_the_oracles_f32_chain(engine, oracle, in_hz, out_hz, ch, n_streams, n_frames, layout):
    """rows drawn from +-8192 (this kernel's own permitted f32 error several times under the cap): the s16 form against
    float_sample_to_i16(downsample_audio(s / 32768)) of the oracle -- every sample within 1 LSB, fewer than 1 % differing"""
    rng = np.random.default_rng(55 + ch + n_streams)
    x = rng.integers(-8192, 8193, (n_streams, n_frames, ch, 1024), dtype=np.int64).astype(np.int16)
    n_out, _, s16 = run_both(engine, x, layout, in_hz, out_hz)
    rows = rows_of(x).reshape(n_streams, ch, n_frames * 1024)
    differing = total = 0
    for s in range(n_streams):
        want32 = oracle.downsample_planar(rows[s].astype(np.float32) / np.float32(32768.0), in_hz, out_hz)
        assert want32.shape[1] == n_out
        want = oracle.planar_f32_to_s16_interleaved(want32).reshape(n_out, ch)
        d = np.abs(s16[s, :n_out].astype(np.int32) - want.astype(np.int32))
        assert d.max() <= 1, (s, int(d.max()))
        differing, total = differing + int((d > 0).sum()), total + d.size
    print("differing from the oracle's chain: %.4f %%" % (100.0 * differing / total))
    assert differing < 0.01 * total


def make_batch_44k1(engine, oracle, layout, ch, n_streams, n_frames, gain=2500.0):
    """test_s16_chain_gpu.make_batch with the streams opened at 44.1 kHz: every window sequence, both shapes"""
    coeffs = np.empty((n_streams, n_frames, ch, 1024), np.float32)
    for s in range(n_streams):
        for f in range(n_frames):
            for c in range(ch):
                coeffs[s, f, c] = oracle.seeded_spectrum(1024, 0x12345678 + 977 * s + 2 * f + c) * np.float32(gain)
    seq_chain = [0, 1, 2, 3, 0, 0]
    seqs = np.zeros((n_streams, n_frames, 2), np.uint8)
    shapes = np.zeros((n_streams, n_frames, 2), np.uint8)
    for s in range(n_streams):
        for f in range(n_frames):
            seqs[s, f] = seq_chain[(f + s) % 6] if s % 2 else 0
            shapes[s, f] = (f + s) & 1
    sids = np.array([engine.open_stream(44100, ch) for _ in range(n_streams)], np.uint32)
    if layout == "frame":
        order = [(s, f) for f in range(n_frames) for s in range(n_streams)]
        strides = (ch * 1024, n_streams * ch * 1024)
    else:
        order = [(s, f) for s in range(n_streams) for f in range(n_frames)]
        strides = (n_frames * ch * 1024, ch * 1024)
    packed = np.stack([coeffs[s, f] for s, f in order])
    descs, n = soundkit_amd.descs_from_arrays([sids[s] for s, f in order], ch, [seqs[s, f] for s, f in order],
                                              [shapes[s, f] for s, f in order])
    return coeffs, seqs, shapes, sids, strides, packed, descs, n


@pytest.mark.parametrize("layout", ["frame", "stream"])
@pytest.mark.parametrize("ch", [1, 2])
def test_44k1_decode_tail_matches_the_oracle_chain(engine, oracle, layout, ch):
    """synthesis to planar s16 on streams opened at 44.1 kHz, then the new entry with the same strides, against the oracle:
    synthesis -> float_sample_to_i16 -> / 32768 -> downsample_audio(44100, 16000) -> s16"""
    import torch
    n_streams, n_frames = 5, 6
    coeffs, seqs, shapes, sids, strides, packed, descs, n = make_batch_44k1(engine, oracle, layout, ch, n_streams, n_frames)
    plan = engine.plan(descs, n)
    d_coeffs = torch.from_numpy(packed).cuda()
    d_pcm16 = torch.zeros(d_coeffs.shape, dtype=torch.int16, device="cuda")
    n_out = engine.downsample_out_frames(n_frames * 1024, 44100, 16000)
    o_stride = (n_out + 7) // 8 * 8
    d_out = torch.zeros((n_streams, o_stride, ch), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    plan.run_s16_planar(d_coeffs, d_pcm16)
    assert engine.downsample_frames_s16_to_s16_dev(d_pcm16, strides[0], strides[1], ch, n_streams, n_frames, 44100, 16000, d_out, o_stride) == n_out
    engine.synchronize()
    out = d_out.cpu().numpy()
    differing = total = 0
    for s in range(n_streams):
        pcm, _ = oracle.synthesize_stream(coeffs[s], seqs[s], shapes[s])
        planar = np.ascontiguousarray(pcm.transpose(1, 0, 2).reshape(ch, n_frames * 1024))
        q = oracle.pcm_convert("FLOAT_TO_I16_ROUND", planar.ravel()).reshape(planar.shape).astype(np.float32) / np.float32(32768.0)
        want = oracle.planar_f32_to_s16_interleaved(oracle.downsample_planar(q, 44100, 16000)).reshape(n_out, ch)
        d = np.abs(out[s, :n_out].astype(np.int32) - want.astype(np.int32))
        assert d.max() <= 1, (s, int(d.max()))
        differing, total = differing + int((d > 0).sum()), total + d.size
        assert np.abs(want).max() > 100
    assert differing < 0.01 * total
    assert not out[:, n_out:].any()
    plan.destroy()
    for sid in sids:
        engine.close_stream(int(sid))


def test_48k_to_16k_is_the_fixed_filters_entry(engine):
    import torch
    ch, n_streams, n_frames = 2, 9, 3
    x = full_range_rows(ch, n_streams, n_frames)
    packed, strides = pack(x, "stream")
    d_in = torch.from_numpy(packed).cuda()
    n_out = engine.downsample_out_frames(n_frames * 1024)
    stride = (n_out + 7) // 8 * 8
    outs = [torch.zeros((n_streams, stride, ch), dtype=torch.int16, device="cuda") for _ in range(2)]
    f32s = [torch.zeros((n_streams * ch, stride), device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    assert engine.downsample_48k_16k_frames_s16_to_s16_dev(d_in, strides[0], strides[1], ch, n_streams, n_frames, outs[0], stride) == n_out
    assert engine.downsample_frames_s16_to_s16_dev(d_in, strides[0], strides[1], ch, n_streams, n_frames, 48000, 16000, outs[1], stride) == n_out
    assert engine.downsample_48k_16k_frames_s16_to_f32_dev(d_in, strides[0], strides[1], ch, n_streams, n_frames, f32s[0], stride) == n_out
    assert engine.downsample_frames_s16_to_f32_dev(d_in, strides[0], strides[1], ch, n_streams, n_frames, 48000, 16000, f32s[1], stride) == n_out
    engine.synchronize()
    assert outs[0].any() and torch.equal(outs[0], outs[1]) and torch.equal(f32s[0], f32s[1])


def test_refusals_write_nothing_and_empty_calls_are_ok(engine):
    import ctypes as C
    import torch
    from soundkit_amd._lib import lib
    ch, n_streams, n_frames = 2, 4, 2
    x = full_range_rows(ch, n_streams, n_frames)
    packed, strides = pack(x, "stream")
    d_in = torch.from_numpy(packed).cuda()
    n_out = engine.downsample_out_frames(n_frames * 1024, 44100, 16000)
    stride = (n_out + 7) // 8 * 8
    d_s16 = torch.zeros((n_streams, stride, ch), dtype=torch.int16, device="cuda")
    d_f32 = torch.zeros((n_streams * ch, stride), device="cuda")
    torch.cuda.synchronize()
    h = engine._h
    fns = [(lib.sk_downsample_frames_s16_to_s16_dev, d_s16), (lib.sk_downsample_frames_s16_to_f32_dev, d_f32)]

    def call(fn, out, pcm=d_in.data_ptr(), channels=ch, streams=n_streams, frames=n_frames, in_hz=44100, out_hz=16000, out_stride=stride, null_out=False):
        got = C.c_uint32(0xdeadbeef)
        rc = fn(h, pcm, strides[0], strides[1], channels, streams, frames, in_hz, out_hz, None if null_out else out.data_ptr(), out_stride, C.byref(got))
        return rc, got.value

    for fn, out in fns:
        assert call(fn, out, channels=3)[0] == INVALID_ARG
        assert call(fn, out, pcm=None)[0] == INVALID_ARG
        assert call(fn, out, null_out=True)[0] == INVALID_ARG
        assert call(fn, out, out_stride=n_out - 1)[0] == INVALID_ARG
        assert call(fn, out, in_hz=44000)[0] == UNSUPPORTED
        assert call(fn, out, out_hz=11025)[0] == UNSUPPORTED
        assert call(fn, out, in_hz=96000, out_hz=8000)[0] == UNSUPPORTED
        engine.set_resampler_exact(True)
        try:
            assert call(fn, out)[0] == UNSUPPORTED
        finally:
            engine.set_resampler_exact(False)
        assert call(fn, out, frames=0) == (0, engine.downsample_out_frames(0, 44100, 16000))
        assert call(fn, out, streams=0) == (0, n_out)
        assert call(fn, out, streams=0, pcm=None, null_out=True) == (0, n_out)
        engine.synchronize()
        assert not out.any()
        assert call(fn, out) == (0, n_out)   # and the same arguments unchanged do the work
        engine.synchronize()
        assert out.any()


def test_repeatable_at_device_width(oracle):
    """8192 rows x 43 frames of 44.1 -> 16 kHz (well over two workgroups per CU's worth of row blocks: a kernel that mixes pipes
    has its parity test at a full device): two runs bit-identical, three spot rows within the f64 bound.  Run once."""
    import torch
    ch, n_streams, n_frames = 2, 4096, 43
    eng = soundkit_amd.Engine(0, 8)
    try:
        g = torch.Generator(device="cuda").manual_seed(20)
        d_in = torch.randint(-32768, 32768, (n_streams, n_frames, ch, 1024), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
        strides = (n_frames * ch * 1024, ch * 1024)
        n_out = eng.downsample_out_frames(n_frames * 1024, 44100, 16000)
        stride = (n_out + 3) // 4 * 4
        outs = [torch.zeros((n_streams * ch, stride), device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for out in outs:
            assert eng.downsample_frames_s16_to_f32_dev(d_in, strides[0], strides[1], ch, n_streams, n_frames, 44100, 16000, out, stride) == n_out
        eng.synchronize()
        assert torch.equal(outs[0], outs[1]), int((outs[0] != outs[1]).sum())
        sincs = sincs_of(oracle, 44100, 16000)
        for row in (0, 4097, 8191):
            x = d_in[row // ch, :, row % ch, :].reshape(1, -1).cpu().numpy()
            want = f64_reference(x, 44100, 16000, sincs)
            err = rel_rms(outs[0][row, :n_out].cpu().numpy()[None], want)
            assert err <= 1e-6, (row, err)
        assert not outs[0][:, n_out:].any()
    finally:
        eng.close()

"""The GPU kernels at the size they are measured at, against the float64 references of tests/f64_ref.py: the AAC synthesis
(every window sequence and task class), the s16 chain and one-launch tail, the 48 -> 16 kHz FIR forms, the generic-ratio
resampler on the matrix cores, MP3 requantisation + hybrid synthesis, and the PCM conversion.

"Full device" is bench.py's own size for its workloads (4096 stereo streams x 64 frames for the decode tail, 8192 rows x 1 s for
the FIR and the generic-ratio resampler, 512 Mi samples for the PCM conversion) and a grid of at least 2048 waves elsewhere.
Each case runs its launch twice on the same inputs and asserts bit-identical outputs (one repeat, never a loop; bench.py runs
once, in its own process), then compares every stream or row -- or, where the float64 work would not fit the time budget, a
seeded sample of rows including both ends -- with float64.  The round-4 defect this guards against
(profiles/r04_lanes_corruption.md) was wrong in 3.4 % of the samples at 4096 x 64 and invisible at ten streams.

The bounds are at most twice the worst value measured on MI355X with the unmodified build and never above 1e-6; each
docstring gives the measured figure.  (The SK_FIR_S16_BF16=1 form has an absolute error floor instead, bounded in 16-bit
steps.)  The float64 work runs on a pool of at most 16 host threads, the MP3 requantisation oracle on 16 processes."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import f64_ref as R
import soundkit_amd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS, FRAMES, CH = 4096, 64, 2
POOL = R.WORKERS
F32_SYNTH_BOUND = 3e-7  # measured 1.57e-7 (A) and 1.58e-7 (B) relative RMS against float64


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _pool_map(fn, items):
    with ThreadPoolExecutor(POOL) as ex:
        return list(ex.map(fn, items))


def _chain_check(pcm64, out16, n_out):
    """pcm64 [C][F*1024] f64 synthesis of the channels of some streams (channel-major per stream), out16 [S][n_out][CH] the
    kernels' 16 kHz s16: the float64 chain narrows, resamples s / 32768 and narrows again.  -> (worst |d| per stream,
    fraction of samples with |d| = 1 per stream)"""
    q = R.float_sample_to_i16(pcm64.astype(np.float32))
    y = R.s16_chain(q, n_out, workers=1)
    want = R.float_sample_to_i16(y.astype(np.float32))
    s = out16.shape[0]
    want = want.reshape(s, -1, n_out).transpose(0, 2, 1)
    d = np.abs(out16.astype(np.int32) - want.astype(np.int32)).reshape(s, -1)
    return d.max(1), (d == 1).mean(1), np.abs(want).reshape(s, -1).max(1)


# ---- A. the decode tail as bench.py runs it ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tail_case():
    """bench.py's pipeline batch (seeded spectra x SPECTRUM_GAIN, frame-major, Sine / KBD alternating), a seeded 1/16 of the
    streams at 400 x that gain (~1e6) so that both s16 stages clamp.  Every launch twice from a reset state; the outputs on the
    host; the float64 synthesis and chain of every stream, compared chunk by chunk."""
    import torch
    from soundkit_amd._lib import lib
    bench = _bench()
    dev = torch.device("cuda")
    eng = soundkit_amd.Engine(0, STREAMS + 8)
    res = {}
    try:
        coeffs = bench.seeded_spectra(torch, dev, STREAMS, FRAMES, CH) * bench.SPECTRUM_GAIN
        loud = np.sort(np.random.default_rng(0xA11).choice(STREAMS, STREAMS // 16, replace=False))
        by_stream = coeffs.view(STREAMS, FRAMES, CH, 1024)
        by_stream[torch.from_numpy(loud).to(dev)] *= 400.0
        packed = by_stream.transpose(0, 1).contiguous().view(-1, CH, 1024)  # [frame][stream]
        del coeffs, by_stream
        sids = np.array([eng.open_stream(48000, CH) for _ in range(STREAMS)], np.uint32)
        shape_of_frame = (np.arange(FRAMES) & 1).astype(np.uint8)
        descs, n = soundkit_amd.descs_from_arrays(np.tile(sids, FRAMES), CH, np.zeros((STREAMS * FRAMES, 2), np.uint8),
                                                  np.repeat(shape_of_frame, STREAMS)[:, None].repeat(2, 1))
        plan = eng.plan(descs, n)
        n_out = eng.downsample_out_frames(FRAMES * 1024)
        stride = (n_out + 7) // 8 * 8

        def reset():
            for sid in sids:
                eng.reset_stream(int(sid))

        torch.cuda.synchronize()
        f32 = []
        for _ in range(2):
            reset()
            f32.append(torch.empty_like(packed))
            torch.cuda.synchronize()
            plan.run_f32(packed, f32[-1])
            eng.synchronize()
        res["f32_repeat"] = torch.equal(f32[0], f32[1])
        del f32[1]
        pcm16 = []
        for _ in range(2):
            reset()
            pcm16.append(torch.zeros(packed.shape, dtype=torch.int16, device=dev))
            torch.cuda.synchronize()  # torch's memset runs on its own stream, the engine on another
            plan.run_s16_planar(packed, pcm16[-1])
            eng.synchronize()
        res["s16_repeat"] = torch.equal(pcm16[0], pcm16[1])
        del pcm16[1]
        res["s16_rounding_mismatches"] = int((pcm16[0] != R.float_sample_to_i16_torch(f32[0])).sum())
        res["s16_clamped"] = int((pcm16[0] == 32767).sum() + (pcm16[0] == -32768).sum())
        chain = []
        for _ in range(2):
            chain.append(torch.zeros((STREAMS, stride, CH), dtype=torch.int16, device=dev))
            torch.cuda.synchronize()
            assert eng.downsample_48k_16k_frames_s16_to_s16_dev(pcm16[0], CH * 1024, STREAMS * CH * 1024, CH, STREAMS, FRAMES,
                                                                 chain[-1], stride) == n_out
            eng.synchronize()
        res["chain_repeat"] = torch.equal(chain[0], chain[1])
        res["chain_pad_zero"] = not chain[0][:, n_out:].any().item()
        res["packed_f32_build"] = lib.sk_kernels_use_packed_f32() != 0
        if not res["packed_f32_build"]:
            tails = []
            for _ in range(2):
                reset()
                tails.append(torch.zeros((STREAMS, stride, CH), dtype=torch.int16, device=dev))
                torch.cuda.synchronize()
                assert plan.run_tail_s16(packed, CH * 1024, CH, FRAMES, tails[-1], stride) == n_out
                eng.synchronize()
            res["tail_repeat"] = torch.equal(tails[0], tails[1])
            res["tail_mismatches"] = int((tails[0] != chain[0]).sum())
            del tails
        plan.destroy()
        # float64, every stream: chunks of 16 streams on the host pool
        coeff_h = packed.view(FRAMES, STREAMS, CH, 1024)
        f32_h = f32[0].view(FRAMES, STREAMS, CH, 1024)
        chunks = [(a, min(STREAMS, a + 16)) for a in range(0, STREAMS, 16)]
        host = [(coeff_h[:, a:b].cpu().numpy(), f32_h[:, a:b].cpu().numpy(), chain[0][a:b, :n_out].cpu().numpy()) for a, b in chunks]
        del packed, f32, pcm16, chain, coeff_h, f32_h

        def one(k):
            c, p, o = host[k]
            b = c.shape[1]
            cc = c.transpose(1, 2, 0, 3).reshape(b * CH, FRAMES, 1024)
            p64, _, _ = R.synthesize(cc, np.zeros((b * CH, FRAMES), np.uint8), np.tile(shape_of_frame, (b * CH, 1)), workers=1)
            got = p.transpose(1, 2, 0, 3).reshape(b, -1).astype(np.float64)
            w = p64.reshape(b, -1)
            rel = np.sqrt(((got - w) ** 2).mean(1) / (w ** 2).mean(1))
            dmax, ones, peak = _chain_check(p64.reshape(b * CH, -1), o, n_out)
            host[k] = None
            return rel, dmax, ones, peak

        t = _pool_map(one, range(len(chunks)))
        res["rel"] = np.concatenate([x[0] for x in t])
        res["dmax"] = np.concatenate([x[1] for x in t])
        res["ones"] = np.concatenate([x[2] for x in t])
        res["peak"] = np.concatenate([x[3] for x in t])
        res["loud"] = loud
        print("\nA: f32 synthesis rel RMS vs f64: worst %.3g (quiet streams %.3g, loud %.3g); chain: worst |d| %d, worst 1-LSB "
              "fraction %.4f, mean %.5f; s16 clamped samples %d" % (
                  res["rel"].max(), np.delete(res["rel"], loud).max(), res["rel"][loud].max(), res["dmax"].max(), res["ones"].max(),
                  res["ones"].mean(), res["s16_clamped"]))
    finally:
        eng.close()
    return res


def test_a_f32_synthesis_every_stream_against_f64(tail_case):
    """plan.run_f32 at bench size: every stream within 3e-7 relative RMS of the float64 synthesis (measured on MI355X:
    1.57e-7 worst, the same in the quiet and the loud streams).  Repeated launch bit-identical."""
    assert tail_case["f32_repeat"]
    assert tail_case["rel"].size == STREAMS
    assert tail_case["rel"].max() < F32_SYNTH_BOUND, tail_case["rel"].max()


def test_a_s16_synthesis_is_the_rounded_f32_synthesis(tail_case):
    """run_s16_planar at bench size: every sample is float_sample_to_i16 of the f32 kernel's output of the same frames, clamped
    samples included (the loud 1/16 clamps)"""
    assert tail_case["s16_repeat"]
    assert tail_case["s16_rounding_mismatches"] == 0
    assert tail_case["s16_clamped"] > 1000


def test_a_two_launch_chain_every_stream_against_f64(tail_case):
    """synthesis to planar s16 + k_fir_48k_16k_bf16 s16 -> s16 at bench size: in every stream no sample is more than 1 LSB from
    the float64 chain and fewer than 1 % differ by 1 (measured: worst stream 0.76 %, mean 0.05 %)"""
    assert tail_case["chain_repeat"] and tail_case["chain_pad_zero"]
    assert tail_case["dmax"].max() <= 1, np.argwhere(tail_case["dmax"] > 1)[:8].ravel().tolist()
    assert tail_case["ones"].max() < 0.01, tail_case["ones"].max()
    assert tail_case["peak"].min() > 100 and tail_case["peak"][tail_case["loud"]].min() == 32767


def test_a_one_launch_tail_at_bench_size(tail_case):
    """run_tail_s16 at 4096 x 64 (the existing check runs 4096 x 8): bit-equal to the two-launch chain, repeated launch too"""
    if tail_case["packed_f32_build"]:
        pytest.skip("packed-f32 build: the one-launch tail is withdrawn")
    assert tail_case["tail_repeat"]
    assert tail_case["tail_mismatches"] == 0


def test_a_bench_dump_against_f64(tmp_path):
    """bench.py itself (--steps 1 --warmup 0 --dump-outputs): the rows of pcm_s16_16k.npy it samples, against the float64 chain
    of the same streams -- the benchmark's timed output tied to a reference"""
    bench = _bench()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=80)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(str(tmp_path / "pcm_s16_16k.npy"))
    n_out = got.shape[1]
    k = max(1, min(STREAMS, bench.DUMP_BYTES // (n_out * CH * 4)))
    rows = np.sort(np.random.default_rng(bench.SEED0).choice(STREAMS, k, replace=False))
    assert got.shape == (rows.size, n_out, CH) and rows.size >= 64
    import torch
    shape_of_frame = (np.arange(FRAMES) & 1).astype(np.uint8)

    def one(s):
        c = (bench.seeded_spectra(torch, torch.device("cpu"), 1, FRAMES, CH, stream0=int(s)) * bench.SPECTRUM_GAIN).numpy()
        p64, _, _ = R.synthesize(c.transpose(1, 0, 2), np.zeros((CH, FRAMES), np.uint8), np.tile(shape_of_frame, (CH, 1)), workers=1)
        return p64.reshape(CH, -1)

    pcm = np.concatenate(_pool_map(one, rows))
    dmax, ones, peak = _chain_check(pcm, got.astype(np.int16), n_out)
    print("\nbench dump: %d rows, worst |d| %d, worst 1-LSB fraction %.4f" % (rows.size, dmax.max(), ones.max()))
    assert dmax.max() <= 1 and ones.max() < 0.01 and peak.min() > 100



# ---- B. mixed window sequences, all four task classes in one plan -------------------------------------------------------

def _mixed_batch(n_streams, n_frames):
    """bench.py --mix's sequences (per ten frames LongStart, EightShort, LongStop, shifted by the stream index; brackets cut by the
    batch's edges fall back to OnlyLong).  Every 8th stream mono; stereo streams with s % 3 == 0 carry their right channel's
    brackets five frames later (EightShort on other frame numbers than the left: one-channel walks or pairs across streams);
    s % 16 == 5 all OnlyLong (pairs), the last stream (mono) all OnlyLong as well (an odd long channel: the straight-line
    one-channel kernel), stream 4087 (mono) with a bracket of three EightShort frames no other channel has (a walk)."""
    pattern = np.array([0, 1, 2, 3, 0, 0, 0, 0, 0, 0], np.uint8)

    def row(shift):
        r = pattern[(np.arange(n_frames) + shift) % 10].copy()
        k = 0
        while k < n_frames and r[k] in (2, 3):
            r[k] = 0
            k += 1
        k = n_frames - 1
        while k >= 0 and r[k] in (1, 2):
            r[k] = 0
            k -= 1
        return r

    chans = np.where(np.arange(n_streams) % 8 == 7, 1, 2)
    seqs = np.zeros((n_streams, n_frames, 2), np.uint8)
    shapes = np.zeros((n_streams, n_frames, 2), np.uint8)
    for s in range(n_streams):
        seqs[s, :, 0] = row(s)
        seqs[s, :, 1] = row(s + 5) if s % 3 == 0 else seqs[s, :, 0]
        if s % 16 == 5 or s == n_streams - 1:
            seqs[s] = 0
        shapes[s, :, 0] = (np.arange(n_frames) + s) & 1
        shapes[s, :, 1] = (np.arange(n_frames) // 2 + s) & 1
    special = n_streams - 9
    seqs[special, :, 0] = 0
    seqs[special, 2:7, 0] = [1, 2, 2, 2, 3]
    return chans, seqs, shapes


def test_b_mixed_sequences_every_stream_against_f64():
    """4096 streams x 16 frames of the mixed batch, frame-major, every launch twice: the f32 output of every stream within 3e-7 relative RMS of the
    float64 synthesis (measured 1.58e-7 worst), the s16 output float_sample_to_i16 of the f32 output (and its repeat) bit for bit"""
    import torch
    n_streams, n_frames = 4096, 16
    chans, seqs, shapes = _mixed_batch(n_streams, n_frames)
    rng = np.random.default_rng(0xB0B)
    eng = soundkit_amd.Engine(0, n_streams + 8)
    try:
        sids = np.array([eng.open_stream(48000, int(c)) for c in chans], np.uint32)
        offs = np.concatenate([[0], np.cumsum(chans)])[:-1]  # a frame's channels, packed: [frame][stream's channels]
        coeffs = (rng.uniform(-1, 1, (n_frames, int(chans.sum()), 1024)) * 2.5e4).astype(np.float32)
        coeffs[:, :, ::7] = 0.0
        order_s = np.tile(np.arange(n_streams), n_frames)
        order_f = np.repeat(np.arange(n_frames), n_streams)
        descs, n = soundkit_amd.descs_from_arrays(sids[order_s], chans[order_s], seqs[order_s, order_f], shapes[order_s, order_f])
        plan = eng.plan(descs, n)
        assert plan.frames_ok == n
        d_in = torch.from_numpy(coeffs.reshape(-1, 1024)).cuda()
        outs = {}
        for kind in ("f32", "f32b", "s16", "s16b"):
            for sid in sids:
                eng.reset_stream(int(sid))
            if kind.startswith("f32"):
                outs[kind] = torch.empty_like(d_in)
                torch.cuda.synchronize()
                plan.run_f32(d_in, outs[kind])
            else:
                outs[kind] = torch.zeros(d_in.shape, dtype=torch.int16, device="cuda")
                torch.cuda.synchronize()
                plan.run_s16_planar(d_in, outs[kind])
            eng.synchronize()
        assert torch.equal(outs["f32"], outs["f32b"]) and torch.equal(outs["s16"], outs["s16b"])
        assert torch.equal(outs["s16"], R.float_sample_to_i16_torch(outs["f32"]))
        plan.destroy()
        f32 = outs["f32"].cpu().numpy().reshape(n_frames, -1, 1024)
    finally:
        eng.close()
    # every channel as its own sequence: [channel][frame]
    ch_seqs = np.concatenate([seqs[s, :, :chans[s]].T for s in range(n_streams)])
    ch_shapes = np.concatenate([shapes[s, :, :chans[s]].T for s in range(n_streams)])
    assert ch_seqs.shape[0] == chans.sum() and set(np.unique(ch_seqs)) == {0, 1, 2, 3}
    cc = coeffs.transpose(1, 0, 2)
    got = f32.transpose(1, 0, 2)
    parts = [(a, min(cc.shape[0], a + 256)) for a in range(0, cc.shape[0], 256)]

    def one(ab):
        a, b = ab
        p64, _, _ = R.synthesize(cc[a:b], ch_seqs[a:b], ch_shapes[a:b], workers=1)
        return ((got[a:b] - p64) ** 2).sum((1, 2)), (p64 ** 2).sum((1, 2))
    t = _pool_map(one, parts)
    err, pw = np.concatenate([x[0] for x in t]), np.concatenate([x[1] for x in t])
    # per stream (its channels together)
    stream_of = np.repeat(np.arange(n_streams), chans)
    rel = np.sqrt(np.bincount(stream_of, err) / np.bincount(stream_of, pw))
    print("\nB: mixed sequences rel RMS vs f64: worst %.3g, median %.3g" % (rel.max(), np.median(rel)))
    assert rel.max() < F32_SYNTH_BOUND, (rel.max(), np.argsort(rel)[-5:].tolist())


# ---- C. the 48 -> 16 kHz FIR forms on 8192 rows x 48000 -------------------------------------------------------------------

def _fir_columns(n_out, rng):
    return np.unique(np.concatenate([np.arange(32), np.arange(n_out - 32, n_out), rng.choice(n_out, 64, replace=False)]))


def _full_rows(n_rows, rng, group=16):
    """256 seeded rows, among them the first and last rows of the first and last 16-row groups"""
    ends = [0, group - 1, n_rows - group, n_rows - 1]
    return np.unique(np.concatenate([ends, rng.choice(n_rows, 256 - len(ends), replace=False)]))


def _check_rows(got, x, n_out, rng, f32_bound, label, to_s16=None, scale=1.0):
    """got [rows][n_out] (f32, or s16 when to_s16); x [rows][T] the input, whose values are x * scale (scale a power of two).  Full rows: relative RMS of each row
    (f32) / the 1-LSB rule (s16); every other row at the edge and seeded columns."""
    full = _full_rows(x.shape[0], rng)
    cols = _fir_columns(n_out, rng)
    parts = [full[i:i + 16] for i in range(0, full.size, 16)]
    y_full = np.concatenate(_pool_map(lambda rows: R.fir_48k_16k(x[rows].astype(np.float64) * scale, n_out, workers=1), parts))
    rest = np.setdiff1d(np.arange(x.shape[0]), full)
    parts = [rest[i:i + 128] for i in range(0, rest.size, 128)]  # 16 threads x 128 rows: about 2 GB of f64 live at most
    y_cols = np.concatenate(_pool_map(lambda rows: R.fir_48k_16k_at(x[rows], cols, block=64) * scale, parts))
    if to_s16:
        w_full = R.float_sample_to_i16(y_full.astype(np.float32)).astype(np.int32)
        w_cols = R.float_sample_to_i16(y_cols.astype(np.float32)).astype(np.int32)
        d_full = np.abs(got[full].astype(np.int32) - w_full)
        d_cols = np.abs(got[rest][:, cols].astype(np.int32) - w_cols)
        ones = (d_full == 1).mean(1)
        print("\nC %s: worst |d| %d (full rows) %d (columns), worst 1-LSB fraction %.4f" % (label, d_full.max(), d_cols.max(), ones.max()))
        assert d_full.max() <= 1 and d_cols.max() <= 1 and ones.max() < 0.01
        return
    g_full = got[full].astype(np.float64)
    rel = np.sqrt(((g_full - y_full) ** 2).mean(1) / (y_full ** 2).mean(1))
    absmax = max(np.abs(g_full - y_full).max(), np.abs(got[rest][:, cols] - y_cols).max())
    print("\nC %s: rel RMS vs f64 worst %.3g over %d full rows; max |err| %.3g (all rows, edge + seeded columns)" % (
        label, rel.max(), full.size, absmax))
    assert rel.max() < f32_bound and absmax < FIR_F32_ABS


FIR_F32_BOUND = 4.5e-7  # measured 2.3e-7 (f32 rows) and 1.7e-7 (s16 -> f32) relative RMS against float64
FIR_F32_ABS = 2e-6  # measured 1.03e-6 largest error of any checked output


@pytest.mark.parametrize("stride_pad", [0, 3], ids=["aligned", "stride48003"])
def test_c_fir_f32_rows(stride_pad):
    """downsample_48k_16k_dev on 8192 f32 rows x 48000 (bench.py --workload fir), rows 16-byte aligned and with a stride of
    48003 floats (the unaligned load path): every row's edges and seeded columns, 256 full rows, against the float64 filter
    (measured: 2.3e-7 worst relative RMS, 1.03e-6 largest error; bounds 4.5e-7 and 2e-6)"""
    import torch
    rows, frames = 8192, 48000
    eng = soundkit_amd.Engine(0, 16)
    try:
        n_out = eng.downsample_out_frames(frames)
        g = torch.Generator(device="cuda").manual_seed(0xC1 + stride_pad)
        x = torch.rand((rows, frames + stride_pad), generator=g, device="cuda") * 2 - 1
        ys = [torch.empty((rows, n_out), device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for y in ys:
            assert eng.downsample_48k_16k_dev(x, frames + stride_pad, rows, frames, y, n_out) == n_out
        eng.synchronize()
        assert torch.equal(ys[0], ys[1])
        got = ys[0].cpu().numpy()
        xh = x[:, :frames].cpu().numpy()
    finally:
        eng.close()
    _check_rows(got, xh, n_out, np.random.default_rng(0xC1), FIR_F32_BOUND, "f32 rows stride %d" % (frames + stride_pad))


@pytest.mark.parametrize("form", ["f32_to_s16_ch1", "f32_to_s16_ch2", "s16_to_s16", "s16_to_f32"])
def test_c_fir_frame_packed_forms(form):
    """the frame-packed forms (frame-major batch of 1024-sample frames, 47 frames per stream, 8192 channel rows): f32 -> s16 with
    one and two channels, s16 -> s16, s16 -> f32 (k_fir_48k_16k_bf16's distinct instantiations); s16 outputs obey the 1-LSB rule
    against float_sample_to_i16 of the float64 filter (measured: worst row 0.28 % off by one), f32 outputs its relative RMS
    bound (measured 1.7e-7)"""
    import torch
    ch = 1 if form.endswith("ch1") else 2
    n_streams, n_frames = 8192 // ch, 47
    eng = soundkit_amd.Engine(0, 16)
    try:
        n_out = eng.downsample_out_frames(n_frames * 1024)
        g = torch.Generator(device="cuda").manual_seed(0xC2 + len(form))
        if form.startswith("f32"):
            x = (torch.rand((n_frames, n_streams, ch, 1024), generator=g, device="cuda") * 2.2 - 1.1) * 0.999
        else:
            x = torch.randint(-32768, 32768, (n_frames, n_streams, ch, 1024), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
        strides = (ch * 1024, n_streams * ch * 1024)
        outs = []
        for _ in range(2):
            if form.endswith("to_f32"):
                f_stride = (n_out + 3) // 4 * 4
                y = torch.zeros((n_streams * ch, f_stride), device="cuda")
                torch.cuda.synchronize()
                assert eng.downsample_48k_16k_frames_s16_to_f32_dev(x, *strides, ch, n_streams, n_frames, y, f_stride) == n_out
            else:
                o_stride = (n_out + 7) // 8 * 8
                y = torch.zeros((n_streams, o_stride, ch), dtype=torch.int16, device="cuda")
                torch.cuda.synchronize()
                fn = eng.downsample_48k_16k_frames_s16_dev if form.startswith("f32") else eng.downsample_48k_16k_frames_s16_to_s16_dev
                assert fn(x, *strides, ch, n_streams, n_frames, y, o_stride) == n_out
            eng.synchronize()
            outs.append(y)
        assert torch.equal(outs[0], outs[1])
        if form.endswith("to_f32"):
            got = outs[0][:, :n_out].cpu().numpy()
        else:
            assert not outs[0][:, n_out:].any()
            got = outs[0][:, :n_out].permute(0, 2, 1).reshape(n_streams * ch, n_out).cpu().numpy()
        xh = x.permute(1, 2, 0, 3).reshape(n_streams * ch, n_frames * 1024).cpu().numpy()
    finally:
        eng.close()
    _check_rows(got, xh, n_out, np.random.default_rng(0xC2), FIR_F32_BOUND, form, to_s16=not form.endswith("to_f32"),
                scale=1.0 / 32768.0 if xh.dtype == np.int16 else 1.0)


# ---- D. the generic ratio on the matrix cores ------------------------------------------------------------------------------

SINC_F64_BOUND = 4.5e-7  # measured 2.25e-7 worst (44.1 -> 16 kHz) relative RMS against float64


@pytest.mark.parametrize("in_hz,out_hz", [(44100, 16000), (16000, 48000), (48000, 44100)])
def test_d_sinc_mfma_every_row(in_hz, out_hz):
    """4096 x 2 rows x 1 s: k_sinc_mfma (twice, bit-identical) against the exact scalar form (set_resampler_exact, bit-equal to
    the oracle) in every row within 1e-6 relative RMS and 4e-6 at most (measured 2.5e-7 and 1.67e-6); 64 seeded rows (first
    and last included) against the float64 sinc walk (measured 2.25e-7 worst, bound 4.5e-7)"""
    import torch
    rows = 8192
    eng = soundkit_amd.Engine(0, 16)
    try:
        n_out = eng.downsample_out_frames(in_hz, in_hz, out_hz)
        g = torch.Generator(device="cuda").manual_seed(in_hz + out_hz)
        x = torch.rand((rows, in_hz), generator=g, device="cuda") * 2 - 1
        ys = [torch.empty((rows, n_out), device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        for k, y in enumerate(ys):
            eng.set_resampler_exact(k == 2)
            assert eng.downsample_dev(x, in_hz, rows, in_hz, in_hz, out_hz, y, n_out) == n_out
            eng.synchronize()
        eng.set_resampler_exact(False)
        assert torch.equal(ys[0], ys[1])
        diff = (ys[0].double() - ys[2].double())
        rel = (diff.pow(2).mean(1) / ys[2].double().pow(2).mean(1)).sqrt()
        worst_rel, worst_abs = rel.max().item(), diff.abs().max().item()
        pick = np.unique(np.concatenate([[0, rows - 1], np.random.default_rng(in_hz).choice(rows, 62, replace=False)]))
        got = ys[0][torch.from_numpy(pick).cuda()].cpu().numpy()
        xh = x[torch.from_numpy(pick).cuda()].cpu().numpy()
    finally:
        eng.close()
    parts = [np.arange(i, min(pick.size, i + 4)) for i in range(0, pick.size, 4)]
    want = np.concatenate(_pool_map(lambda p: R.sinc_resample(xh[p], in_hz, out_hz), parts))
    assert want.shape == got.shape
    rel64 = np.sqrt(((got - want) ** 2).mean(1) / (want ** 2).mean(1))
    print("\nD %d->%d: vs scalar form worst rel RMS %.3g, max |d| %.3g; vs f64 worst rel RMS %.3g" % (
        in_hz, out_hz, worst_rel, worst_abs, rel64.max()))
    assert worst_rel < 1e-6 and worst_abs < 4e-6
    assert rel64.max() < SINC_F64_BOUND


# ---- E. MP3 requantisation + hybrid synthesis ------------------------------------------------------------------------------

MP3_BOUND = 6.5e-7  # measured 3.3e-7 worst stream (median 1.5e-7) relative RMS against float64
MP3_LINE_BOUND = 4.7e-7  # measured 2.37e-7 worst requantised line, relative to its scale


def _mp3_batch(n_streams, n_gran, rng):
    """4096 stereo streams x 4 granules, distinct seeded lines in every stream; per stream a block-type sequence (long,
    start / short / stop, all short, mixed short blocks in every other group of six streams) and its joint stereo: none, mid/side, intensity,
    or both (intensity positions 0..7 in the right channel's scale factors)"""
    from test_mp3_requant_gpu import random_channel, random_quant
    seqs = [[0, 0, 0, 0], [0, 1, 2, 3], [1, 2, 2, 3], [2, 2, 2, 2], [3, 0, 1, 2], [2, 3, 0, 1]]
    granules, quant, bts, mixed = [], [], np.zeros((n_streams, n_gran), np.uint8), np.zeros((n_streams, n_gran), np.uint8)
    for s in range(n_streams):
        bts[s] = seqs[s % len(seqs)]
        mixed[s] = (bts[s] == 2) & ((s // 6) % 2 == 1)
    for g in range(n_gran):  # granule-major, the order the streams' state advances in
        for s in range(n_streams):
            bt, mx = int(bts[s, g]), int(mixed[s, g])
            left, right = random_channel(rng, bt, mx), random_channel(rng, bt, mx)
            right["scalefac_l"] = [int(v) for v in rng.integers(0, 8, 21)] + [0]
            right["scalefac_s"] = [[int(v) for v in rng.integers(0, 8, 3)] for _ in range(12)] + [[0, 0, 0]]
            ms, intensity = [(0, 0), (1, 0), (0, 1), (1, 1)][s % 4]
            granules.append({"sample_rate": 44100, "channels": 2, "ms_stereo": ms, "intensity_stereo": intensity, "ch": [left, right]})
            quant.append(random_quant(rng))
            quant.append(random_quant(rng, int(rng.integers(100, 577))))
    return granules, np.stack(quant), bts, mixed


def test_e_mp3_requant_and_hybrid_every_granule_against_f64():
    """k_mp3_requant + k_mp3_hybrid on 4096 stereo streams x 4 granules, each launch twice (bit-identical, the streams reset
    in between): every line of the requantisation within 4.7e-7 of the float64 oracle (relative to the larger channel of a
    joint-stereo pair, as tests/test_mp3_requant_gpu.py has it; measured 2.37e-7), and every stream's PCM within 6.5e-7
    relative RMS of the float64 hybrid filterbank applied to the float64 lines (measured 3.3e-7 worst, 1.5e-7 median), with the
    synthetic window D of tests/test_mp3_gpu.py"""
    from oracle import mp3_hybrid as M
    from soundkit_amd import mp3
    from test_mp3_requant_gpu import tables
    n_streams, n_gran = 4096, 4
    d512 = M.synthetic_window(7)
    long_o, short_o, pretab = tables(4)
    granules, quant, bts, mixed = _mp3_batch(n_streams, n_gran, np.random.default_rng(0xE3))
    eng = soundkit_amd.Engine(0, n_streams + 8)
    try:
        mp3.set_synthesis_window(d512, eng)
        assert mp3.set_band_tables(44100, long_o, short_o, pretab, eng) == 0
        xr, status = mp3.requantize(granules, quant, eng)
        xr2, status2 = mp3.requantize(granules, quant, eng)
        assert not status.any() and not status2.any() and np.array_equal(xr, xr2)
        sids = [eng.open_stream(44100, 2) for _ in range(n_streams)]
        hyb = [(sids[s], 2, [int(bts[s, g])] * 2, [int(mixed[s, g])] * 2) for g in range(n_gran) for s in range(n_streams)]
        pcm, status = mp3.hybrid_synthesize(hyb, xr.reshape(-1, 2, 576), eng)
        for sid in sids:
            eng.reset_stream(sid)
        pcm2, status2 = mp3.hybrid_synthesize(hyb, xr.reshape(-1, 2, 576), eng)
        assert not status.any() and not status2.any() and np.array_equal(pcm, pcm2)
    finally:
        eng.close()
    want_xr = R.mp3_requant(granules, quant, long_o, short_o, pretab).reshape(-1, 2, 576)
    got_xr = xr.reshape(-1, 2, 576).astype(np.float64)
    joint = np.array([bool(g["ms_stereo"] or g["intensity_stereo"]) for g in granules])
    scale = np.abs(want_xr)
    scale[joint] = np.abs(want_xr[joint]).max(axis=1, keepdims=True)
    line_err = np.abs(got_xr - want_xr)
    assert (line_err <= MP3_LINE_BOUND * scale).all(), float(np.max(line_err / np.maximum(scale, 1e-300)))
    assert not got_xr[want_xr == 0].any()
    # [stream channel][granule][576]: granules are granule-major, channels interleaved
    lines = want_xr.reshape(n_gran, n_streams, 2, 576).transpose(1, 2, 0, 3).reshape(n_streams * 2, n_gran, 576)
    parts = [(a, min(2 * n_streams, a + 512)) for a in range(0, 2 * n_streams, 512)]
    dd = d512.astype(np.float32).astype(np.float64)
    w = np.concatenate(_pool_map(lambda ab: R.mp3_hybrid(lines[ab[0]:ab[1]], np.repeat(bts, 2, 0)[ab[0]:ab[1]],
                                                         np.repeat(mixed, 2, 0)[ab[0]:ab[1]], dd)[0], parts))
    got = pcm.reshape(n_gran, n_streams, 576, 2).transpose(1, 3, 0, 2).reshape(n_streams, -1).astype(np.float64)
    w = w.reshape(n_streams, -1)
    rel = np.sqrt(((got - w) ** 2).mean(1) / (w ** 2).mean(1))
    print("\nE: MP3 requant worst line error %.3g of its scale; hybrid PCM rel RMS vs f64 worst %.3g, median %.3g" % (
        float(np.max(line_err / np.maximum(scale, 1e-300))), rel.max(), np.median(rel)))
    assert rel.max() < MP3_BOUND, (rel.max(), np.argsort(rel)[-5:].tolist())


# ---- F. PCM conversions past 2^31 bytes ------------------------------------------------------------------------------------

def _s24(b):
    v = b[..., 0].astype(np.int32) | (b[..., 1].astype(np.int32) << 8) | (b[..., 2].astype(np.int32) << 16)
    return np.where(v & 0x800000, v - (1 << 24), v)


PCM_CASES = {
    # name: (input bytes per sample, output bytes, numpy restatement of raw input bytes [k][ib] -> output values)
    "F32LE_TO_I16": (4, 2, lambda b: np.nan_to_num(np.clip(b.copy().view(np.float32)[:, 0], np.float32(-1), np.float32(1))
                                                    * np.float32(32767.0), nan=0.0).astype(np.int16)),
    "S24LE_TO_I16": (3, 2, lambda b: (_s24(b) >> 8).astype(np.int16)),
    "I16LE_TO_F32": (2, 4, lambda b: b.copy().view(np.int16)[:, 0].astype(np.float32) / np.float32(32768.0)),
    "exact_S32LE": (4, 2, lambda b: (b.copy().view(np.int32)[:, 0] >> 16).astype(np.int16)),
}


@pytest.mark.parametrize("name", list(PCM_CASES))
def test_f_pcm_conversion_past_2_31_bytes(name):
    """one op per input width with n % 4 == 3 and more than 2^31 + 12 input bytes, 16-byte aligned and with one buffer moved by
    2 bytes (k_convert<OP, false>; the buffer that keeps its elements naturally aligned): the samples around the 2^31-byte
    input offset, the tail and 256 seeded blocks of 4096 samples against a numpy restatement, bit for bit; the repeat
    bit-identical.  Only contiguous slices are copied back (no device-side gather over a tensor of more than 2^31 elements)."""
    import torch
    from soundkit_amd._lib import check, lib
    ib, ob, ref = PCM_CASES[name]
    n = ((1 << 31) + 13 + ib - 1) // ib
    n += (3 - n % 4) % 4
    assert n % 4 == 3 and n * ib > (1 << 31) + 12
    boundary = (1 << 31) // ib
    starts = np.concatenate([[min(boundary - 2048, n - 4096), n - 4096],  # (the 2^31-byte offset lies in the last block)
                             np.sort(np.random.default_rng(ib).choice(n // 4096 - 1, 256, replace=False)) * 4096])
    eng = soundkit_amd.Engine(0, 16)
    try:
        g = torch.Generator(device="cuda").manual_seed(0xF0 + ib)
        raw = torch.randint(0, 256, (n * ib + 16,), generator=g, device="cuda", dtype=torch.uint8)
        if name.startswith("F32"):
            raw[:n * 4].view(torch.float32).copy_(torch.rand(n, generator=g, device="cuda") * 2.4 - 1.2)
        in_shift = 2 if ib in (2, 3) else 0  # 2- and 4-byte elements stay naturally aligned (the API's contract)
        results = []
        for moved in (False, True, True):
            src = raw[in_shift:in_shift + n * ib] if moved else raw[:n * ib]
            out = torch.zeros(n * ob + 16, dtype=torch.uint8, device="cuda")
            dst = out[2:2 + n * ob] if moved and not in_shift else out[:n * ob]
            torch.cuda.synchronize()
            if name.startswith("exact"):
                check(lib.sk_pcm_exact_to_i16_dev(eng._h, soundkit_amd.engine.FMT_S32LE, src.data_ptr(), n, dst.data_ptr()),
                      "sk_pcm_exact_to_i16_dev", eng._h)
            else:
                eng.pcm_convert_dev(name, src, dst, n)
            eng.synchronize()
            got = np.stack([dst[int(a) * ob:(int(a) + 4096) * ob].cpu().numpy() for a in starts])
            inp = np.stack([src[int(a) * ib:(int(a) + 4096) * ib].cpu().numpy() for a in starts])
            results.append((got, inp))
            del out
        del raw
    finally:
        eng.close()
    for k, (got, inp) in enumerate(results):
        want = ref(inp.reshape(-1, ib)).view(np.uint8)
        assert np.array_equal(got.reshape(-1), want), (name, k, int((got.reshape(-1, ob) != want.reshape(-1, ob)).any(1).sum()))
    assert np.array_equal(results[1][0], results[2][0])


# ---- 3. the env-switch forms, each in a child process ------------------------------------------------------------------------

def _child(out_dir):
    """reduced case A (4096 x 8) in a fresh process: f32 and planar s16 synthesis, then the s16 -> s16 and s16 -> f32 FIR forms"""
    import torch
    bench = _bench()
    streams, frames = 4096, 8
    eng = soundkit_amd.Engine(0, streams + 8)
    try:
        coeffs = bench.seeded_spectra(torch, torch.device("cuda"), streams, frames, CH) * bench.SPECTRUM_GAIN
        packed = coeffs.view(streams, frames, CH, 1024).transpose(0, 1).contiguous().view(-1, CH, 1024)
        sids = np.array([eng.open_stream(48000, CH) for _ in range(streams)], np.uint32)
        shapes = np.repeat((np.arange(frames) & 1).astype(np.uint8), streams)[:, None].repeat(2, 1)
        seqs = np.zeros((streams * frames, 2), np.uint8)
        seqs[::7] = [1, 1]  # a few LongStart / LongStop frames among the long ones
        seqs[1::7] = [3, 3]
        descs, n = soundkit_amd.descs_from_arrays(np.tile(sids, frames), CH, seqs, shapes)
        plan = eng.plan(descs, n)
        pcm32 = torch.empty_like(packed)
        pcm16 = torch.zeros(packed.shape, dtype=torch.int16, device="cuda")
        n_out = eng.downsample_out_frames(frames * 1024)
        o_stride = (n_out + 7) // 8 * 8
        f_stride = (n_out + 3) // 4 * 4
        s16 = torch.zeros((streams, o_stride, CH), dtype=torch.int16, device="cuda")
        f32 = torch.zeros((streams * CH, f_stride), device="cuda")
        torch.cuda.synchronize()
        plan.run_f32(packed, pcm32)
        eng.synchronize()
        for sid in sids:
            eng.reset_stream(int(sid))
        plan.run_s16_planar(packed, pcm16)
        strides = (CH * 1024, streams * CH * 1024)
        assert eng.downsample_48k_16k_frames_s16_to_s16_dev(pcm16, *strides, CH, streams, frames, s16, o_stride) == n_out
        assert eng.downsample_48k_16k_frames_s16_to_f32_dev(pcm16, *strides, CH, streams, frames, f32, f_stride) == n_out
        eng.synchronize()
        np.save(os.path.join(out_dir, "pcm32.npy"), pcm32.cpu().numpy())
        np.save(os.path.join(out_dir, "pcm16.npy"), pcm16.cpu().numpy())
        np.save(os.path.join(out_dir, "s16.npy"), s16[:, :n_out].cpu().numpy())
        np.save(os.path.join(out_dir, "f32.npy"), f32[:, :n_out].cpu().numpy())
        plan.destroy()
    finally:
        eng.close()


def _run_child(tmp_path, name, env_extra):
    out = tmp_path / name
    out.mkdir()
    env = dict(os.environ)
    env.pop("SK_SYNTH_PAIRS", None)
    env.pop("SK_FIR_S16_BF16", None)
    env.update(env_extra)
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(os.path.abspath(__file__)), ROOT, env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(out)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return {k: np.load(str(out / (k + ".npy"))) for k in ("pcm32", "pcm16", "s16", "f32")}


def test_switch_synth_pairs_off_gives_the_same_samples(tmp_path):
    """SK_SYNTH_PAIRS=0 (one channel per wave, README: "same samples") against the default, 4096 x 8 in two fresh processes:
    the f32 and the planar s16 synthesis and both FIR outputs bit-identical"""
    a = _run_child(tmp_path, "default", {})
    b = _run_child(tmp_path, "nopairs", {"SK_SYNTH_PAIRS": "0"})
    for k in a:
        assert np.array_equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))


BF16_FLOOR_LSB = 0.003  # absolute RMS error of the SK_FIR_S16_BF16=1 form in 16-bit steps: measured 1.57e-3 worst row


def test_switch_fir_s16_bf16_accuracy(tmp_path):
    """SK_FIR_S16_BF16=1 (the bf16 form of the FIR on s16 rows).  Its sample x = x1 + x2 is split into bf16 planes
    x1 = 256 (s >> 8) and x2 = s & 255, and its product set (fir_bf16.hip products_of) leaves out x2 * h3 (and x2 * h2 in
    windows 1, 7 and 8): pruning meant for the f32 split, where |x2| ~ 2^-8 |x|, but here x2 is the whole low byte.  The
    error is therefore an absolute floor, independent of the level, and the relative error grows as the signal gets quieter.
    This test bounds the floor: the s16 -> f32 output's RMS error against the float64 filter, per row, in 16-bit steps
    (measured on MI355X: 1.45e-3 to 1.57e-3 steps in every row; bound 3e-3).  At the bench's level (signal RMS 184-198 steps)
    that is 8.4e-6 relative; at +-300 steps it would be about 1.6e-5.  The s16 -> s16 output stays within 1 LSB of the float64
    chain (measured 0.14 % of samples off by one)."""
    b = _run_child(tmp_path, "bf16", {"SK_FIR_S16_BF16": "1"})
    pcm16, s16, f32 = b["pcm16"], b["s16"], b["f32"]
    frames, streams = pcm16.shape[0] // 4096, 4096
    rows = pcm16.reshape(frames, streams, CH, 1024).transpose(1, 2, 0, 3).reshape(streams * CH, -1)
    n_out = f32.shape[1]
    parts = [(a, a + 512) for a in range(0, rows.shape[0], 512)]
    y = np.concatenate(_pool_map(lambda ab: R.s16_chain(rows[ab[0]:ab[1]], n_out, workers=1), parts))
    err_lsb = np.sqrt(((f32 - y) ** 2).mean(1)) * 32768.0
    level_lsb = np.sqrt((y ** 2).mean(1)) * 32768.0
    rel = err_lsb / level_lsb
    want = R.float_sample_to_i16(y.astype(np.float32)).reshape(streams, CH, n_out).transpose(0, 2, 1)
    d = np.abs(s16.astype(np.int32) - want.astype(np.int32))
    print("\nSK_FIR_S16_BF16=1: s16 -> f32 RMS error %.4g LSB worst row (%.4g best), signal RMS %.4g..%.4g LSB, relative %.3g worst; "
          "s16 -> s16 worst |d| %d, 1-LSB fraction %.4f" % (err_lsb.max(), err_lsb.min(), level_lsb.min(), level_lsb.max(), rel.max(),
                                                             d.max(), (d == 1).mean()))
    assert err_lsb.max() < BF16_FLOOR_LSB
    assert d.max() <= 1 and (d.reshape(streams, -1) == 1).mean(1).max() < 0.01


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "child":
    _child(sys.argv[2])

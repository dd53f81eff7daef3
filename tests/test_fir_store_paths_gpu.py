"""The 48 -> 16 kHz FIR on s16 frame rows at the shapes where its store and addressing paths change (profiles/fir_interior.md).

sk_downsample_48k_16k_frames_s16_to_s16_dev and the _to_f32 form run k_fir_48k_16k_bf16<true, true, OUT, true, true, A32>.  Its interior
bodies store with every lane (for interleaved stereo each lane of a row pair writes two of the pair's four frames) and, with A32,
address rows and outputs through buffer descriptors with 32-bit offsets; bodies at the edges of a segment, of the rows and of a
partly filled group of sixteen rows keep the branching stores.  Seeded s16 noise at full scale and at +-3 steps, for

  1, 2, 15, 16, 17 and 34 streams, mono and stereo (rows: less than a group, exactly one, one and a part, two and a part),
  1, 2, 3, 7 and 12 frames per stream (one segment of a few bodies up to several segments),
  frame-major and stream-major strides,

each result compared two ways:

  against the oracle's downsample_planar (+ its s16 conversion), with the bound tests/test_s16_chain_gpu.py::test_fir_on_s16_rows
  holds for that comparison: per stream at most one step apart, under 1 % of the samples apart at all; the f32 rows within 1e-6
  relative RMS of the oracle's, and the s16 output = the oracle's conversion of the f32 output, bit for bit;

  bit for bit against the same call under SK_FIR_ADDR64=1 in a fresh child process: 64-bit pointers, the addressing this kernel
  had before the descriptors.

The outputs lie between poisoned guard bands (and the padding of every output row is poisoned too): all of it stays untouched.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = [1, 2, 15, 16, 17, 34]
FRAMES = [1, 2, 3, 7, 12]
LAYOUTS = ["frame", "stream"]
LEVELS = ["full", "quiet"]
GUARD = 4096          # elements of poison in front of and behind each output
POISON16 = 0x5A5B
POISON32 = np.float32(-7.25e11)


def noise(level):
    """[34 streams][12 frames][2 channels][1024] s16; every case takes the leading part of it"""
    rng = np.random.default_rng(77 if level == "full" else 78)
    if level == "full":
        x = rng.integers(-32768, 32768, (max(STREAMS), max(FRAMES), 2, 1024), dtype=np.int64).astype(np.int16)
        x[0, 0, 0, :6] = [32767, -32768, 0, 1, -1, 255]
        return x
    return rng.integers(-3, 4, (max(STREAMS), max(FRAMES), 2, 1024), dtype=np.int64).astype(np.int16)


def key(ch, n_streams, n_frames, layout, level, form):
    return "%s_%s_c%d_s%d_f%d_%s" % (form, level, ch, n_streams, n_frames, layout)


def run_case(engine, torch, x, ch, n_streams, n_frames, layout):
    """both forms on x[:n_streams, :n_frames, :ch]; returns (s16 [streams][n_out][ch], f32 [rows][n_out]) after checking the guards"""
    part = np.ascontiguousarray(x[:n_streams, :n_frames, :ch])
    if layout == "frame":
        packed = np.ascontiguousarray(part.transpose(1, 0, 2, 3))
        strides = (ch * 1024, n_streams * ch * 1024)
    else:
        packed = part
        strides = (n_frames * ch * 1024, ch * 1024)
    d_in = torch.from_numpy(packed).cuda()
    n_out = engine.downsample_out_frames(n_frames * 1024)
    o_stride = (n_out + 7) // 8 * 8
    f_stride = (n_out + 3) // 4 * 4
    buf16 = torch.full((2 * GUARD + n_streams * o_stride * ch,), POISON16, dtype=torch.int16, device="cuda")
    buf32 = torch.full((2 * GUARD + n_streams * ch * f_stride,), float(POISON32), dtype=torch.float32, device="cuda")
    d_s16 = buf16[GUARD:GUARD + n_streams * o_stride * ch].view(n_streams, o_stride, ch)
    d_f32 = buf32[GUARD:GUARD + n_streams * ch * f_stride].view(n_streams * ch, f_stride)
    torch.cuda.synchronize()
    assert engine.downsample_48k_16k_frames_s16_to_s16_dev(d_in, strides[0], strides[1], ch, n_streams, n_frames, d_s16, o_stride) == n_out
    assert engine.downsample_48k_16k_frames_s16_to_f32_dev(d_in, strides[0], strides[1], ch, n_streams, n_frames, d_f32, f_stride) == n_out
    engine.synchronize()
    h16, h32 = buf16.cpu().numpy(), buf32.cpu().numpy()
    assert (h16[:GUARD] == POISON16).all() and (h16[-GUARD:] == POISON16).all(), "s16 output: a guard band was written"
    assert (h32[:GUARD] == POISON32).all() and (h32[-GUARD:] == POISON32).all(), "f32 output: a guard band was written"
    s16 = h16[GUARD:-GUARD].reshape(n_streams, o_stride, ch)
    f32 = h32[GUARD:-GUARD].reshape(n_streams * ch, f_stride)
    assert (s16[:, n_out:] == POISON16).all(), "s16 output: the padding of a row was written"
    assert (f32[:, n_out:] == POISON32).all(), "f32 output: the padding of a row was written"
    return s16[:, :n_out].copy(), f32[:, :n_out].copy()


def child(out_path):
    import torch
    import soundkit_amd
    eng = soundkit_amd.Engine(0, 64)
    got = {}
    try:
        for level in LEVELS:
            x = noise(level)
            for ch in (1, 2):
                for n_streams in STREAMS:
                    for n_frames in FRAMES:
                        for layout in LAYOUTS:
                            s16, f32 = run_case(eng, torch, x, ch, n_streams, n_frames, layout)
                            got[key(ch, n_streams, n_frames, layout, level, "s16")] = s16
                            got[key(ch, n_streams, n_frames, layout, level, "f32")] = f32
    finally:
        eng.close()
    np.savez(out_path, **got)


@pytest.fixture(scope="module")
def addr64(tmp_path_factory):
    """every case once more in a fresh process with SK_FIR_ADDR64=1 (the switch is read once per process)"""
    out = str(tmp_path_factory.mktemp("addr64") / "results.npz")
    env = dict(os.environ)
    env["SK_FIR_ADDR64"] = "1"
    env.pop("SK_FIR_S16_BF16", None)
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(os.path.abspath(__file__)), ROOT, env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", out], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def inputs():
    return {level: noise(level) for level in LEVELS}


@pytest.fixture(scope="module")
def oracle_rows(oracle, inputs):
    """the oracle's f32 result for all 68 rows of the full input, once per level and frame count: row 2 s + c = (stream s, channel c)"""
    want = {}
    for level in LEVELS:
        for n_frames in FRAMES:
            rows = inputs[level][:, :n_frames].transpose(0, 2, 1, 3).reshape(-1, n_frames * 1024).astype(np.float32) / np.float32(32768.0)
            want[level, n_frames] = oracle.downsample_planar(rows, 48000, 16000)
    return want


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_streams", STREAMS)
@pytest.mark.parametrize("ch", [1, 2])
def test_store_paths(engine, oracle, inputs, oracle_rows, addr64, ch, n_streams, layout):
    import torch
    assert os.environ.get("SK_FIR_ADDR64") != "1", "this process must run the default addressing"
    for level in LEVELS:
        for n_frames in FRAMES:
            s16, f32 = run_case(engine, torch, inputs[level], ch, n_streams, n_frames, layout)
            n_out = s16.shape[1]
            # bit for bit against the 64-bit pointer path
            for form, got in (("s16", s16), ("f32", f32)):
                ref = addr64[key(ch, n_streams, n_frames, layout, level, form)]
                assert got.shape == ref.shape and np.array_equal(got.view(np.uint8), ref.view(np.uint8)), \
                    (form, level, n_frames, int((got != ref).sum()), np.argwhere(got != ref)[:5].tolist())
            # against the oracle, with the bounds of test_s16_chain_gpu.py::test_fir_on_s16_rows
            all_rows = oracle_rows[level, n_frames]
            assert all_rows.shape[1] == n_out
            worst32 = 0.0
            for s in range(n_streams):
                want32 = all_rows[2 * s:2 * s + ch]
                mine = f32[s * ch:(s + 1) * ch]
                rms = np.sqrt(np.mean(want32.astype(np.float64) ** 2))
                worst32 = max(worst32, np.sqrt(np.mean((mine.astype(np.float64) - want32.astype(np.float64)) ** 2)) / rms)
                want16 = oracle.planar_f32_to_s16_interleaved(want32).reshape(n_out, ch)
                assert np.array_equal(s16[s], oracle.planar_f32_to_s16_interleaved(mine).reshape(n_out, ch)), (level, n_frames, s)
                d = np.abs(s16[s].astype(np.int32) - want16.astype(np.int32))
                assert d.max() <= 1 and (d > 0).mean() < 0.01, (level, n_frames, s, int(d.max()), float((d > 0).mean()))
            print("%s ch %d streams %d frames %d %s: f32 rel. RMS error %.3g" % (layout, ch, n_streams, n_frames, level, worst32))
            assert worst32 < 1e-6, (level, n_frames, worst32)
        if level == "full":
            assert np.abs(s16.astype(np.int32)).max() > 5000   # loud enough to mean something


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "child":
    child(sys.argv[2])

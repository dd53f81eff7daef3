"""bench.py on the GPU at a small size: a plain run prints the line without what --full adds, and two runs with the same
arguments dump the same outputs of their last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(out_dir, *extra):
    argv = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--streams", "64",
            "--frames", "8", "--dump-outputs", str(out_dir)] + list(extra)
    r = subprocess.run(argv, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_line_and_repeatable_outputs(tmp_path, engine):
    line = bench(tmp_path / "a")
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "frames/s" and line["higher_is_better"] is True
    assert line["value"] > 0 and abs(line["ms_per_step"] - 1000.0 * 64 * 8 * 3 / line["value"] / 3) < 1e-6 * line["ms_per_step"]
    assert not {"cpu_baseline", "cpu_baseline_single_core", "end_to_end", "mix"} & set(line)
    assert "same_kernel_f32_out" not in line["kernels"]["k_aac_synth"]
    bench(tmp_path / "b")
    a, b = np.load(str(tmp_path / "a" / "pcm_s16_16k.npy")), np.load(str(tmp_path / "b" / "pcm_s16_16k.npy"))
    assert a.dtype == np.float32 and a.shape == (64, engine.downsample_out_frames(8 * 1024), 2)
    assert np.array_equal(a, b) and np.all(a == np.round(a)) and np.abs(a).max() > 10 and np.abs(a).max() <= 32768

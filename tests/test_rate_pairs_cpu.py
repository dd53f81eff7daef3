"""The reference side of tests/test_rate_pairs_gpu.py, on the CPU: before a kernel is held to the CPU chain at every rate pair, the
chain itself is measured at every rate pair, on the same signal (tests/rate_pairs.py).

* The f32 chain against float64: oracle.downsample_planar and f64_ref.sinc_resample, both rounded to s16 by
  oracle.planar_f32_to_s16_interleaved, differ by one step on at most 0.5 % of the samples -- half of the 1 % the ticks are allowed
  against the f32 chain, so a kernel keeps as much room as the reference itself uses.  Measured: 0.14 % at most (96 -> 8 kHz), 0.09 % and less elsewhere;
  relative RMS between the two 0.6 - 1.1e-7 (profiles/rate_pairs.md).
* pcm_worker_model.OutputStage, the expected value of the PCM tick, gives at every pair exactly the records rate_pairs.chunk_counts
  derives from the index walk alone: one per whole chunk and the flush's, 16 bits, one channel, so many bytes each.
* The peak of the resampled signal stays below 1.0: no comparison in either file runs into the clamp."""
import numpy as np
import pytest

import f64_ref
import pcm_worker_model as M
import rate_pairs as R


@pytest.mark.parametrize("pair", R.PAIRS, ids=R.label)
def test_the_f32_chain_rounds_like_float64(oracle, pair):
    in_hz, out_hz = pair
    x = R.signal(in_hz, 2).astype(np.float32)
    f32 = oracle.downsample_planar(x, in_hz, out_hz)
    f64 = f64_ref.sinc_resample(x, in_hz, out_hz)
    assert f32.shape == f64.shape and f32.shape[1] > 0.9 * (R.FRAMES - 400) * out_hz / in_hz
    peak = float(np.abs(f64).max())
    a = oracle.planar_f32_to_s16_interleaved(f32).astype(np.int32)
    b = oracle.planar_f32_to_s16_interleaved(f64.astype(np.float32)).astype(np.int32)
    d = np.abs(a - b)
    print("\nrate_pairs part0 %d %d share=%.5f worst=%d rel_rms=%.3e peak=%.3f" % (in_hz, out_hz, (d > 0).mean(), d.max(), R.rel_rms(f32, f64), peak))
    assert peak < 1.0
    assert d.max() <= 1 and (d > 0).mean() <= 0.005, (pair, int(d.max()), float((d > 0).mean()))


def test_the_output_stage_gives_the_records_of_the_index_walk(oracle):
    specs = R.pcm_specs()
    assert len(specs) == 40
    for fmt, rate, ch, units, bits, out_rate, out_ch in specs:
        counts = R.chunk_counts(rate, out_rate)
        assert len(counts) == 3 and all(counts), (rate, out_rate, counts)  # two chunks and a flush that has something to give
        # about frames * out / in of it, less the delay of 128 input frames; the walk ends within two steps of that, the trim is rounded
        assert abs(sum(counts) - (R.FRAMES - 128) * out_rate / rate) <= 2 + 2 * out_rate / rate, (rate, out_rate, counts)
        got = R.cpu_chain(oracle, fmt, rate, ch, units, bits, out_rate, out_ch)
        assert R.structure(got) == [(16, 1, False, 2 * n) for n in counts], (rate, out_rate, ch)
        assert all(np.abs(np.frombuffer(g[3], "<i2").astype(np.int32)).max() < 32767 for g in got)
    # the two kinds of a pair are different signals, and so are the two channels of the stereo one
    for k in range(0, 40, 2):
        mono, stereo = specs[k], specs[k + 1]
        left = np.frombuffer(b"".join(stereo[3]), np.uint8).reshape(-1, 2, 3)
        assert not np.array_equal(left[:, 0], left[:, 1])
        assert len(b"".join(mono[3])) == 2 * R.FRAMES and left.shape[0] == R.FRAMES


def test_chunk_counts_is_the_streaming_resampler(oracle):
    """chunk_counts against oracle.StreamingResampler at sizes on both sides of a chunk: 0 ... 2 chunks and what the flush then pads"""
    for in_hz, out_hz in R.PAIRS:
        for frames in (1, 4095, 4096, 4097, R.FRAMES, 3 * 4096):
            rs = oracle.StreamingResampler(in_hz, out_hz, 1)
            x = np.zeros((1, frames), np.float32)
            got = [rs.process(x[:, p:p + 4096]).shape[1] for p in range(0, frames, 4096)]
            got = [g for g in got if g] + [g for g in [rs.flush().shape[1]] if g]
            assert got == R.chunk_counts(in_hz, out_hz, frames), (in_hz, out_hz, frames)

"""Test infrastructure: downmix_channels of the reference's worker (soundkit-decoder/src/lib.rs:3492-3561) in numpy float32, every
operation separately rounded and in the reference's order, and pcm_worker_model.OutputStage with that downmix in its _emit, so
that sources of more than two channels have a CPU chain to be compared with.  (The C oracle's bytes <-> f32, its mono downmix and
its StreamingResampler take any channel count already.)"""
import numpy as np

import pcm_worker_model as M
from pcm_worker_model import FMT_F32LE, FMT_S16LE, FMT_S24LE, FMT_S32LE

F = np.float32
K = F(0.707)  # center_coef = surround_coef, lib.rs:3519-3520


def surround_pair(x):
    """lib.rs:3522-3538: (left, right) before the normalisation.  x: [C > 2][frames] float32"""
    C = x.shape[0]
    with np.errstate(all="ignore"):
        left, right = x[0].copy(), x[1].copy()
        left = left + K * x[2]
        right = right + K * x[2]
        if C > 4:
            left = left + K * x[4]
            if C > 5:
                right = right + K * x[5]
    return left.astype(F), right.astype(F)


def peak(left, right):
    """lib.rs:3541-3545: fold(0.0, f32::max) over |left| then |right|: a NaN never raises it (f32::max returns the other operand)"""
    a = np.abs(np.concatenate([left, right]))
    a = a[~np.isnan(a)]
    return F(a.max()) if a.size else F(0.0)


def downmix_channels(x, target):
    """-> [min(target, C)][frames] float32"""
    x = np.ascontiguousarray(x, F)
    C, n = x.shape
    assert target >= 1
    if target == 1:  # lib.rs:3500-3508
        scale = F(1.0) / F(C)
        mono = np.zeros(n, F)
        with np.errstate(all="ignore"):
            for c in range(C):
                mono = (mono + (x[c] * scale).astype(F)).astype(F)
        return mono[None, :]
    if target == 2 and C > 2:
        left, right = surround_pair(x)
        m = peak(left, right)
        if m > F(1.0):  # lib.rs:3546-3554
            with np.errstate(all="ignore"):
                s = F(1.0) / m
                left, right = (left * s).astype(F), (right * s).astype(F)
        return np.stack([left, right])
    return x[:target].copy()  # lib.rs:3560


class WideOutputStage(M.OutputStage):
    """OutputStage for any channel count.  peaks: the m of every AudioData that went through the stereo branch, in order."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.peaks = []

    def _emit(self, planar, out_float):  # emit_resampled_chunks, lib.rs:3261-3290
        ch = planar.shape[0]
        if self.t_ch < ch:
            if self.t_ch == 2 and ch > 2:
                self.peaks.append(float(peak(*surround_pair(np.ascontiguousarray(planar, F)))))
            planar = downmix_channels(planar, self.t_ch)
            ch = planar.shape[0]
        fmt = FMT_F32LE if out_float else {16: FMT_S16LE, 24: FMT_S24LE, 32: FMT_S32LE}[self.t_bits]
        return (self.t_bits, ch, self.t_rate, out_float, False, self.O.f32_planar_to_bytes(fmt, planar).tobytes())

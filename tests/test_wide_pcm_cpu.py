"""Sources of 3 ... 8 channels, the part that needs no GPU: the new entry points are declared and exported, and the test model of
downmix_channels (wide_pcm_model, written from soundkit-decoder/src/lib.rs:3492-3561) gives hand-computed values.

The hand computation: Python floats are binary64, and a sum, product or quotient of two binary32 values computed in binary64 and
then rounded to binary32 is the correctly rounded binary32 result (53 >= 2 * 24 + 2), so r32() below restates the reference's f32
arithmetic one operation at a time without numpy's float32 in the loop."""
import struct
import subprocess

import numpy as np
import pytest

import soundkit_amd
import wide_pcm_model as W
from soundkit_amd import _lib

NEW = ["sk_engine_enable_wide_pcm", "sk_engine_wide_pcm_streams", "sk_pcm_downmix", "sk_pcm_downmix_dev"]


def r32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


K = r32(0.707)


def by_hand(frame, target):
    """one frame through lib.rs:3492-3538 (before the normalisation) -> list of outputs"""
    C = len(frame)
    if target == 1:
        scale, acc = r32(1.0 / C), 0.0
        for v in frame:
            acc = r32(acc + r32(v * scale))
        return [acc]
    if target == 2 and C > 2:
        left, right = frame[0], frame[1]
        left = r32(left + r32(K * frame[2]))
        right = r32(right + r32(K * frame[2]))
        if C > 4:
            left = r32(left + r32(K * frame[4]))
        if C > 5:
            right = r32(right + r32(K * frame[5]))
        return [left, right]
    return list(frame[:target])


def test_header_and_library_have_the_new_entry_points():
    declared = soundkit_amd.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", soundkit_amd.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert name in declared and name in exported and hasattr(_lib.lib, name), name
    text = open(_lib.HEADER_PATH).read()
    assert "#define SK_MAX_PCM_CHANNELS 8u" in text and "#define SK_MAX_CHANNELS 2u" in text


def test_exact_literals():
    """values whose arithmetic is exact: 0.707f times a power of two, and three quarters of it (its significand 11861492 is a
    multiple of four)"""
    assert K == 11861492 * 2.0 ** -24
    x = np.array([[0.0], [0.0], [0.5], [9.0], [0.25], [-0.5], [7.0], [-3.0]], np.float32)
    for C, want in ((3, (K / 2, K / 2)), (4, (K / 2, K / 2)), (5, (0.75 * K, K / 2)), (6, (0.75 * K, 0.0)), (8, (0.75 * K, 0.0))):
        y = W.downmix_channels(x[:C], 2)
        assert y.shape == (2, 1) and (float(y[0, 0]), float(y[1, 0])) == want, C
    # mono of four: every product and partial sum is exact
    y = W.downmix_channels(np.array([[1.0], [0.5], [-0.25], [2.0]], np.float32), 1)
    assert y.shape == (1, 1) and float(y[0, 0]) == 0.8125
    # neither mono nor stereo: the first channels as they are; and there is no upmix
    x5 = np.arange(10, dtype=np.float32).reshape(5, 2)
    assert np.array_equal(W.downmix_channels(x5, 3), x5[:3]) and np.array_equal(W.downmix_channels(x5, 7), x5)


@pytest.mark.parametrize("C", [3, 4, 5, 6, 8])
def test_surround_branch_by_hand(C):
    rng = np.random.default_rng(C)
    x = rng.uniform(-0.3, 0.3, (C, 40)).astype(np.float32)  # |L|, |R| <= 0.3 * (1 + 2 * 0.707) < 1: no scale
    want = np.array([by_hand([float(v) for v in x[:, i]], 2) for i in range(40)], np.float32).T
    assert np.array_equal(W.downmix_channels(x, 2), want)
    x *= np.float32(4.0)  # some |L| or |R| beyond 1: scaled by 1 / max
    pre = [by_hand([float(v) for v in x[:, i]], 2) for i in range(40)]
    m = max(abs(v) for f in pre for v in f)
    assert m > 1.0
    s = r32(1.0 / m)
    want = np.array([[r32(v * s) for v in f] for f in pre], np.float32).T
    got = W.downmix_channels(x, 2)
    assert np.array_equal(got, want) and np.abs(got).max() <= 1.0
    want1 = np.array([by_hand([float(v) for v in x[:, i]], 1) for i in range(40)], np.float32).T
    assert np.array_equal(W.downmix_channels(x, 1), want1)


def test_the_peak_decides_strictly_above_one():
    above = float(np.nextafter(np.float32(1), np.float32(2)))
    x = np.zeros((6, 5), np.float32)
    x[0] = [1.0, -0.5, 0.25, 0.0, 0.125]
    y = W.downmix_channels(x, 2)
    assert np.array_equal(y[0], x[0]) and not y[1].any()  # m == 1.0: unscaled
    x[1, 3] = -above  # the peak in R, from a negative sample
    y = W.downmix_channels(x, 2)
    s = r32(1.0 / above)
    assert s < 1.0 and [float(v) for v in y[0]] == [r32(float(v) * s) for v in x[0]]
    assert float(y[1, 3]) == r32(-above * s)


def test_nan_and_infinity():
    x = np.zeros((5, 4), np.float32)
    x[0] = [np.nan, 2.0, -0.5, 0.25]
    x[1] = [0.5, 0.5, np.nan, 0.5]
    y = W.downmix_channels(x, 2)  # the NaNs do not raise m: m = 2, everything halved, the NaNs stay
    assert np.isnan(y[0, 0]) and np.isnan(y[1, 2])
    assert [float(v) for v in y[0, 1:]] == [1.0, -0.25, 0.125] and [float(y[1, i]) for i in (0, 1, 3)] == [0.25, 0.25, 0.25]
    x[0, 0] = -np.inf  # m = inf: the scale is 0, inf * 0 = NaN, everything else 0 with its sign
    y = W.downmix_channels(x, 2)
    assert np.isnan(y[0, 0]) and np.isnan(y[1, 2])
    assert not y[0, 1:].any() and np.signbit(y[0, 2]) and not np.signbit(y[0, 1])
    only_nan = np.full((3, 2), np.nan, np.float32)
    assert np.isnan(W.downmix_channels(only_nan, 2)).all()  # m stays 0.0

"""Test infrastructure for tests/test_rate_pairs_cpu.py and tests/test_rate_pairs_gpu.py: the 20 rate pairs, the signal every stream
carries, its source bytes, the CPU chain's expected records, and the figures the comparisons share.

The signal is 8594 frames, two resampler chunks of 4096 and a tail for the flush, cut into units of UNITS frames.  Per channel it is
0.45 * uniform(-1, 1) + 0.25 * sin(2 pi 440 t / rate) with a seed of its own, so a swapped or doubled channel shows; its peak is
below 0.7, and below 1.0 behind every resampler for every channel a test uses (0.99 at most, after 44.1 -> 48 kHz; the seed is chosen
for that, most seeds overshoot 1.0 by a few per cent somewhere among eight channels and twenty pairs): nothing clips on the way.

chunk_counts() restates the output count of the reference's StreamingResampler (soundkit-decoder lib.rs:1970-2058 over rubato's
SincFixedIn::process) on its own: the f64 time index walked step by step from -128, one chunk of 4096 at a time, and the flush's
trim of round(padding * out / in).  The CPU test holds pcm_worker_model.OutputStage to it, and OutputStage is what the ticks meet."""
import functools
import math

import numpy as np

import pcm_worker_model as M
from test_flac_tick_rates_gpu import PAIRS, SIZES as UNITS

FRAMES = sum(UNITS)
CHUNK = M.CHUNK
BLOCKS = [997, 4096, 1, 3497]  # the streaming entry's calls; what is left of the signal after them goes in as a last call
WIDTH = {M.FMT_S16LE: 2, M.FMT_S24LE: 3, M.FMT_S32LE: 4, M.FMT_F32LE: 4}
assert FRAMES == 8594 and len(PAIRS) == 20 and len(set(PAIRS)) == 20


def label(pair):
    return "%g -> %g kHz" % (pair[0] / 1000.0, pair[1] / 1000.0)


@functools.lru_cache(maxsize=None)
def signal(rate, channels, silent=None):
    """[channels][FRAMES] float64; channel `silent` is zeros"""
    tone = 0.25 * np.sin(2.0 * np.pi * 440.0 * np.arange(FRAMES) / rate)
    x = np.stack([0.45 * np.random.default_rng([23, rate, c]).uniform(-1.0, 1.0, FRAMES) + tone for c in range(channels)])
    if silent is not None:
        x[silent] = 0.0
    x.setflags(write=False)
    return x


def encode(x, fmt):
    """planar [C][frames] float64 -> the interleaved little-endian bytes of a source in `fmt`, rounded to that format"""
    v = np.ascontiguousarray(x.T)
    if fmt == M.FMT_F32LE:
        return v.astype("<f4").tobytes()
    bits = 8 * WIDTH[fmt]
    q = np.round(v * (2.0 ** (bits - 1) - 1)).astype(np.int64)
    assert np.abs(q).max() < 2 ** (bits - 1)
    if bits == 24:
        return np.ascontiguousarray((q & 0xffffff).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()
    return q.astype("<i%d" % (bits // 8)).tobytes()


def cut(data, frame_bytes, unit_frames=UNITS):
    out, pos = [], 0
    for f in unit_frames:
        out.append(data[pos:pos + f * frame_bytes])
        pos += f * frame_bytes
    assert pos == len(data)
    return out


@functools.lru_cache(maxsize=None)
def source_units(rate, channels, fmt, silent=None):
    return tuple(cut(encode(signal(rate, channels, silent), fmt), WIDTH[fmt] * channels))


def chunk_counts(in_hz, out_hz, frames=FRAMES):
    """the frames of every output a stream of `frames` input frames gives: one per whole chunk, then the flush's (left out when empty)"""
    t_ratio = 1.0 / (out_hz / in_hz)
    end_idx = CHUNK - 257 - math.ceil(t_ratio)
    idx = -128.0
    counts = []

    def chunk():
        nonlocal idx
        n = 0
        while idx < end_idx:
            idx += t_ratio
            n += 1
        idx -= CHUNK
        return n
    whole, rest = divmod(frames, CHUNK)
    counts = [chunk() for _ in range(whole)]
    tail = chunk()
    if rest:
        tail = max(tail - int(math.floor((CHUNK - rest) * out_hz / in_hz + 0.5)), 0)  # C's round(): half away from zero
    return counts + ([tail] if tail else [])


def cpu_chain(oracle, fmt, rate, channels, units, out_bits, out_rate, out_channels, stage=M.OutputStage):
    """the CPU chain's records for a PCM stream in the tick's form: (bits, channels, is_float, bytes)"""
    st = stage(oracle, rate, channels, 8 * WIDTH[fmt], fmt == M.FMT_F32LE, False, out_bits, out_rate, out_channels)
    outs = [o for u in units for o in st.piece(u)] + st.flush()
    assert all(o[2] == out_rate and not o[4] for o in outs)
    return [(o[0], o[1], o[3], o[5]) for o in outs]


def structure(records):
    return [(r[0], r[1], r[2], len(r[3])) for r in records]


# the two streams of every pair in the PCM tick: (format, channels, out_bits, out_channels)
PCM_KINDS = [(M.FMT_S16LE, 1, 16, 1), (M.FMT_S24LE, 2, 16, 1)]


def pcm_specs():
    """run_pcm_ticks' specs, pair by pair and kind by kind: 40 streams"""
    return [(fmt, rate, ch, list(source_units(rate, ch, fmt)), bits, out_rate, out_ch)
            for rate, out_rate in PAIRS for fmt, ch, bits, out_ch in PCM_KINDS]


def rel_rms(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.sqrt(np.mean((got - want) ** 2)) / np.sqrt(np.mean(want ** 2)))


def lsb_share(mine, want):
    """-> (worst |d| in steps, share of samples that differ) of two s16 byte strings of equal length"""
    a, b = np.frombuffer(mine, "<i2").astype(np.int32), np.frombuffer(want, "<i2").astype(np.int32)
    assert a.size == b.size and a.size
    d = np.abs(a - b)
    return int(d.max()), float((d > 0).mean())


def as_floats(record):
    """a record's samples as float64 of full scale 1: floats as they are, integers divided by 2^(bits - 1)"""
    bits, _, is_float, data = record
    if is_float:
        return np.frombuffer(data, "<f4").astype(np.float64)
    if bits == 24:
        b = np.frombuffer(data, np.uint8).reshape(-1, 3).astype(np.int64)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
    else:
        v = np.frombuffer(data, "<i%d" % (bits // 8)).astype(np.int64)
    return v.astype(np.float64) / 2.0 ** (bits - 1)

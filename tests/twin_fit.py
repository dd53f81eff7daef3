"""The reference's twin recordings of one clip ("A_Tusk...", 2.96 s mono) and what the tests pin with them.

TEST INFRASTRUCTURE ONLY (a plain module, imported by tests/test_oracle_pins.py, tests/test_pcm_gpu.py and
tests/test_reference_twins_gpu.py).  The reference's testdata/ holds the clip at 48, 16 and 8 kHz (s16), at 16 kHz as s32, as a
24-bit WAV and as a float32 WAV (tests/golden/README.md).  The files were made outside this project, so they are the one check
of the resampler's gain, delay and pass-band that does not go back to oracle/sk_oracle.c's restatement of rubato: a resampled
higher-rate file must meet its lower-rate twin.  What they cannot pin is tap identity: another good low-pass at the same cut
and delay scores the same below 6 kHz, because the twins' own 16-bit rounding (the clip's RMS is 281 steps) bounds the figures.

read_wav        the RIFF walk of WavStreamProcessor::add (soundkit/src/wav.rs:95-262), with the EXTENSIBLE fields
fit_gain_delay  least-squares gain and fractional delay of a resampled signal against its twin, and the SNR per band
assert_twin     the one assertion every twin test (CPU oracle, GPU kernels, negative controls) goes through
"""
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TWIN_FILES = {48000: "linear16_48k_A_Tusk.s16le", 16000: "linear16_A_Tusk.s16le", 8000: "linear16_8k_A_Tusk.s16le"}
PAIRS = [(48000, 16000), (48000, 8000), (16000, 8000)]


def golden(name):
    return os.path.join(GOLDEN, name)


def twin_s16(rate):
    """the clip at `rate` as the reference holds it: int16 samples (142 080 / 47 360 / 23 680)"""
    return np.fromfile(golden(TWIN_FILES[rate]), "<i2")


def pcm_twins():
    """the 16 kHz clip in its four sample formats, as bytes (uint8 arrays): s16 and s32 files, the 24-bit and float32 WAVs' data"""
    out = {"s16": np.fromfile(golden(TWIN_FILES[16000]), np.uint8), "s32": np.fromfile(golden("linear32_A_Tusk.s32le"), np.uint8)}
    for key, name in (("s24", "wav_24_A_Tusk.wav"), ("f32", "wav_32f_A_Tusk.wav")):
        out[key] = np.frombuffer(read_wav(golden(name))[1], np.uint8).copy()
    return out


def swap_bytes(raw, width):
    """little-endian samples of `width` bytes -> the same samples big-endian"""
    return np.ascontiguousarray(np.asarray(raw, np.uint8).reshape(-1, width)[:, ::-1]).ravel()


def read_wav(path):
    """Walk the RIFF chunks as WavStreamProcessor::add does (soundkit/src/wav.rs:95-262): no 44-byte assumption.
    -> (fmt, pcm, ext): fmt = (tag, channels, rate, byte rate, block align, container bits), pcm = the data chunk's bytes,
    ext = None for a 16-byte `fmt `, else {"fmt_size", "valid_bits", "channel_mask", "sub_format"} of WAVE_FORMAT_EXTENSIBLE
    (sub_format: the leading format code of the sub-format GUID, 1 = PCM, 3 = IEEE float)."""
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and data[8:12] == b"WAVE"
    pos, fmt, pcm, ext = 12, None, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = struct.unpack("<HHIIHH", body[:16])
            if size >= 40:
                cb, valid, mask, code = struct.unpack("<HHIH", body[16:26])
                assert cb >= 22
                ext = {"fmt_size": size, "valid_bits": valid, "channel_mask": mask, "sub_format": code}
        elif cid == b"data":
            pcm = body
        pos += 8 + size + (size & 1)
    return fmt, pcm, ext


# ---- the fit -----------------------------------------------------------------------------------------------------------------

def _best_delay(cross, k, n, lo, hi, step):
    d = np.arange(lo, hi + step / 2, step)
    score = (cross[None, :] * np.exp(2j * np.pi * d[:, None] * k[None, :] / n)).real.sum(1)
    return d, score


def fit_gain_delay(y, twin, fs, band_edges):
    """y: a resampler's output at `fs` Hz, twin: the recording it should equal (same scale).  Over their whole overlap (the
    first min(len) samples of each), in the rfft bins below band_edges[0]: the real gain g and the delay d, in samples of `fs`,
    that minimise sum |g Y_k e^{-2 pi i k d / n} - T_k|^2: the phase ramp delays y by d (circularly; the clip starts and ends
    near silence), so d > 0 says that y runs d samples ahead of the twin.
    -> (d, g, [10 log10(sum |T|^2 / sum |g Y_d - T|^2) over the bins below each edge]).

    For a fixed delay the best gain is closed-form, and the residual falls as Re sum conj(Y_k) T_k e^{2 pi i k d / n} rises, so
    the delay is searched alone: a 0.05-sample grid over +-4 samples, then 0.002, then 0.0001, then the vertex of the parabola
    through the best point and its neighbours (resolution far below 0.001 sample; a 0.01 grid alone costs up to 5 dB)."""
    n = min(len(y), len(twin))
    yf = np.fft.rfft(np.asarray(y[:n], np.float64))
    tf = np.fft.rfft(np.asarray(twin[:n], np.float64))
    freq = np.arange(yf.size) * (fs / n)
    w = np.full(yf.size, 2.0)  # a real signal's bins stand for themselves and their mirror image, except DC (and Nyquist)
    w[0] = 1.0
    if n % 2 == 0:
        w[-1] = 1.0
    sel = freq < band_edges[0]
    k = np.arange(yf.size)[sel].astype(np.float64)
    cross = (w * np.conj(yf) * tf)[sel]
    lo, hi = -4.0, 4.0
    for step in (0.05, 0.002, 0.0001):
        d, score = _best_delay(cross, k, n, lo, hi, step)
        i = int(np.argmax(score))
        lo, hi = d[i] - step, d[i] + step
    i = min(max(i, 1), d.size - 2)
    s0, s1, s2 = score[i - 1], score[i], score[i + 1]
    curve = s0 - 2.0 * s1 + s2
    delay = d[i] + (0.5 * step * (s0 - s2) / curve if curve < 0.0 else 0.0)
    y_d = yf * np.exp(-2j * np.pi * delay * np.arange(yf.size) / n)
    gain = float((w[sel] * (np.conj(y_d[sel]) * tf[sel]).real).sum() / (w[sel] * np.abs(yf[sel]) ** 2).sum())
    snr = []
    for edge in band_edges:
        b = freq < edge
        snr.append(float(10.0 * np.log10((w[b] * np.abs(tf[b]) ** 2).sum() / (w[b] * np.abs(gain * y_d[b] - tf[b]) ** 2).sum())))
    return float(delay), gain, snr


# ---- what the twins pin --------------------------------------------------------------------------------------------------------
# Every figure below was measured with fit_gain_delay on the CPU oracle (oracle.downsample_planar of the higher-rate file / 32768
# against the lower-rate file / 32768; StreamingResampler in any chunking gives the same figures).  Floors are 1 dB under the
# measured SNR.  "f32": the resampler's float output; "s16": that output through float_sample_to_i16 (the worker's full step),
# divided by 32768 again.  None of them comes from a GPU run.

BAND_EDGES = {16000: (3000.0, 6000.0, 7000.0), 8000: (1500.0, 3000.0, 3500.0)}
GAIN_TOL = 1.0e-4   # 5 x the worst |gain - 1| measured (1.9e-5), 10 x under a filter scaled by 1.001
DELAY_TOL = 0.02    # output samples; one input sample of misalignment at 48 -> 16 kHz is 0.33
TWIN_PINS = {
    # (in_hz, out_hz): expected delay, {kind: SNR floors per band edge}
    # measured: delay 0.6680, gain 1.000019 (s16 1.000033), SNR f32 70.67 / 67.82 / 56.49 dB, s16 63.33 / 60.43 / 55.07 dB
    (48000, 16000): dict(delay=0.668, f32=(69.67, 66.82, 55.49), s16=(62.33, 59.43, 54.07)),
    # measured: delay 0.8340, gain 0.999986 (s16 0.999996), SNR f32 63.16 / 60.28 / 53.17 dB, s16 60.64 / 57.77 / 52.46 dB
    (48000, 8000): dict(delay=0.834, f32=(62.16, 59.28, 52.17), s16=(59.64, 56.77, 51.46)),
    # measured: delay 0.5020, gain 1.000001 (s16 1.000028), SNR f32 63.68 / 60.81 / 59.12 dB, s16 60.70 / 57.80 / 56.57 dB
    (16000, 8000): dict(delay=0.502, f32=(62.68, 59.81, 58.12), s16=(59.70, 56.80, 55.57)),
}


def twin_findings(y, in_hz, out_hz, kind="f32"):
    """fit y (the clip at in_hz resampled to out_hz, full scale 1.0) against the out_hz twin -> (tripped, text): the names of
    the pinned quantities that miss ("snr<3000", "gain", "delay"), and the figures in words"""
    pin, edges = TWIN_PINS[(in_hz, out_hz)], BAND_EDGES[out_hz]
    delay, gain, snr = fit_gain_delay(y, twin_s16(out_hz).astype(np.float64) / 32768.0, out_hz, edges)
    tripped = ["snr<%d" % e for e, s, f in zip(edges, snr, pin[kind]) if not s >= f]
    if not abs(gain - 1.0) <= GAIN_TOL:
        tripped.append("gain")
    if not abs(delay - pin["delay"]) <= DELAY_TOL:
        tripped.append("delay")
    text = "%d->%d %s: delay %.4f (pinned %.3f), gain %.6f, SNR %s dB (floors %s)" % (
        in_hz, out_hz, kind, delay, pin["delay"], gain, " / ".join("%.2f" % s for s in snr), " / ".join("%.2f" % f for f in pin[kind]))
    return tripped, text


def assert_twin(y, in_hz, out_hz, kind="f32", label=""):
    tripped, text = twin_findings(y, in_hz, out_hz, kind)
    print("\ntwin %s %s" % (label, text))
    if tripped:
        raise AssertionError("twin fit misses %s: %s %s" % (", ".join(tripped), label, text))

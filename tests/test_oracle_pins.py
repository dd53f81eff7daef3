"""Pins the CPU oracle against the reference's own in-file known answers.

Every case cites the reference test it restates.  No GPU.
"""
import os

import numpy as np
import pytest

import f64_ref as R
import twin_fit as T


def test_imdct_zero_input(oracle):  # dsp.rs:616-624
    out = oracle.imdct_direct_f32(np.zeros(8, np.float32))
    assert np.all(out == 0.0)


def test_imdct_fast_small_block(oracle):  # dsp.rs:626-651, tol 1e-10
    x = np.array([0.0, 1.0, -2.0, 0.5, 3.0, -4.0, 0.25, -0.75], np.float32)
    assert np.abs(oracle.imdct_fast(x) - oracle.imdct_direct_f32(x)).max() < 1.0e-10


@pytest.mark.parametrize("n", [128, 1024])
def test_imdct_fast_aac_blocks(oracle, n):  # dsp.rs:653-692, tol 2e-8
    pat = [0.0, 1.0, -2.0, 0.5, -0.25, 4.0, -8.0, 0.125, -0.75]
    x = np.array([pat[i % 9] for i in range(n)], np.float32)
    assert np.abs(oracle.imdct_fast(x) - oracle.imdct_direct_f32(x)).max() < 2.0e-8


@pytest.mark.parametrize("n", [8, 16, 128, 1024])
@pytest.mark.parametrize("seed", [0x12345678, 0xA5A50101, 0xDEADBEEF])
def test_imdct_fast_seeded_spectra(oracle, n, seed):  # dsp.rs:694-738, tol 4e-8
    x = oracle.seeded_spectrum(n, seed)
    fast = oracle.imdct_fast(x)
    assert np.abs(fast - oracle.imdct_direct_f32(x)).max() < 4.0e-8
    # and against the mathematical definition in f64
    assert np.abs(fast - oracle.imdct_direct_f64(x)).max() < 4.0e-8


def test_seeded_spectrum_shape(oracle):  # dsp.rs:725-738
    x = oracle.seeded_spectrum(1024, 0x12345678)
    assert np.all(x[::7] == 0.0)
    assert np.abs(x).max() <= 12.0
    state = (0x12345678 * 1664525 + 1013904223) & 0xFFFFFFFF
    state = (state * 1664525 + 1013904223) & 0xFFFFFFFF  # index 1
    assert x[1] == np.float32((np.float32((state >> 8) & 0xFFFF) / np.float32(32768.0) - np.float32(1.0)) * np.float32(12.0))


def test_sine_window_princen_bradley(oracle):  # dsp.rs:593-602
    w = oracle.sine_window(2048).astype(np.float32)
    s = w[:1024] * w[:1024] + w[1024:] * w[1024:]
    assert np.abs(s - 1.0).max() < 2.0e-6


def test_kbd_window_symmetric_complementary(oracle):  # dsp.rs:604-614
    w = oracle.kbd_window(2048, 4.0)
    assert np.abs(w - w[::-1]).max() < 1.0e-6
    s = w[:1024] * w[:1024] + w[1024:] * w[1024:]
    assert np.abs(s - 1.0).max() < 2.0e-6


def test_long_synthesis_zero_coefficients(oracle):  # dsp.rs:751-769
    ch = oracle.Channel()
    out = ch.synthesize(np.zeros(1024, np.float32), oracle.ONLY_LONG, oracle.SINE)
    assert np.abs(out).max() < 1.0e-6 and np.abs(ch.delay).max() < 1.0e-6


def test_sequence_windows_use_previous_shape(oracle):  # dsp.rs:771-795 through the synthesis itself
    # an impulse-free check: with unit "imdct" we cannot poke the window directly, so check the
    # documented selections via two syntheses that differ only in the previous shape
    x = oracle.seeded_spectrum(1024, 0xA5A50101)
    a, b = oracle.Channel(), oracle.Channel()
    b.set_state(np.zeros(1024, np.float32), oracle.KBD)
    ya = a.synthesize(x, oracle.ONLY_LONG, oracle.KBD)
    yb = b.synthesize(x, oracle.ONLY_LONG, oracle.KBD)
    imd = oracle.imdct_fast(x)
    ls, lk = oracle.sine_window(2048), oracle.kbd_window(2048, 4.0)
    assert np.array_equal(ya, imd[:1024] * ls[:1024])       # previous shape (Sine) on the left half
    assert np.array_equal(yb, imd[:1024] * lk[:1024])       # previous shape (KBD)
    assert np.array_equal(a.delay, imd[1024:] * lk[1024:])  # current shape on the right half
    # LongStop: 0 | prev short[0..128] | 1 at 448/576 ; LongStart: 1 | cur short[128..256] | 0
    c = oracle.Channel()
    y = c.synthesize(x, oracle.LONG_STOP, oracle.KBD)
    ss = oracle.sine_window(256)
    assert np.all(y[:448] == 0.0)
    assert np.array_equal(y[448:576], imd[448:576] * ss[:128])
    assert np.array_equal(y[576:], imd[576:1024])
    d = oracle.Channel()
    d.synthesize(x, oracle.LONG_START, oracle.KBD)
    sk = oracle.kbd_window(256, 6.0)
    assert np.array_equal(d.delay[:448], imd[1024:1472])
    assert np.array_equal(d.delay[448:576], imd[1472:1600] * sk[128:])
    assert np.all(d.delay[576:] == 0.0)


def test_channel_tracks_previous_shape(oracle):  # dsp.rs:797-807, decoder.rs:371
    ch = oracle.Channel()
    assert ch.prev_shape == oracle.SINE
    ch.synthesize(np.zeros(1024, np.float32), oracle.ONLY_LONG, oracle.KBD)
    assert ch.prev_shape == oracle.KBD


def test_dequantize_known_answers(oracle):  # dsp.rs:809-822
    L = oracle.lib()
    assert L.sko_dequantize_signed(0, 100) == 0.0
    assert abs(L.sko_dequantize_signed(1, 100) - 1.0) < 1e-6
    assert abs(L.sko_dequantize_signed(-1, 100) + 1.0) < 1e-6
    assert abs(L.sko_dequantize_signed(8, 100) - 16.0) < 1e-5
    assert abs(L.sko_scalefactor_multiplier(100) - 1.0) < 1e-6
    assert abs(L.sko_scalefactor_multiplier(104) - 2.0) < 1e-6
    assert abs(L.sko_scalefactor_multiplier(96) - 0.5) < 1e-6


# ---- audio_bytes.rs:380-468 -------------------------------------------------------------------

def test_deinterleave_vecs_i16(oracle):
    out = oracle.deinterleave("i16", np.array([1, 0, 2, 0, 3, 0, 4, 0, 5, 0, 6, 0], np.uint8), 2)
    assert out.tolist() == [[1, 3, 5], [2, 4, 6]]


def test_interleave_vecs_i16(oracle):
    out = oracle.interleave_i16(np.array([[1, 3, 5], [2, 4, 6]], np.int16))
    assert out.tolist() == [1, 0, 2, 0, 3, 0, 4, 0, 5, 0, 6, 0]


def test_deinterleave_vecs_s24(oracle):
    data = np.array([1, 0, 0, 2, 0, 0, 3, 0, 0, 4, 0, 0, 5, 0, 0, 6, 0, 0], np.uint8)
    assert oracle.deinterleave("s24", data, 2).tolist() == [[1, 3, 5], [2, 4, 6]]


def test_deinterleave_vecs_f32(oracle):
    data = np.array([0, 0, 128, 63, 0, 0, 0, 64, 0, 0, 64, 64, 0, 0, 128, 64, 0, 0, 160, 64, 0, 0, 192, 64], np.uint8)
    assert oracle.deinterleave("f32", data, 2).tolist() == [[1.0, 3.0, 5.0], [2.0, 4.0, 6.0]]


def test_i16le_to_f32(oracle):
    data = np.array([0, 0, 0, 64, 255, 127, 0, 192, 0, 128], np.uint8)
    got = oracle.pcm_convert("I16LE_TO_F32", data)
    assert np.abs(got - np.array([0.0, 0.5, 0.9999694, -0.5, -1.0])).max() < 1e-4


def test_stereo_to_mono(oracle):
    assert oracle.pcm_convert("STEREO_TO_MONO_TAKE_LEFT", np.array([10, 20, -30, -40, 50, 60], np.int16)).tolist() == [10, -30, 50]
    assert oracle.pcm_convert("STEREO_TO_MONO_AVG", np.array([100, -100, 50, 150, -200, 200], np.int16)).tolist() == [0, 100, 0]


# ---- audio_pipeline.rs:698-763 ----------------------------------------------------------------

def test_audio_to_mono_f32_averages_channels(oracle):  # :698-713
    data = oracle.interleave_i16(np.array([[32767, -32768], [-32768, 32767]], np.int16))
    ch = oracle.core_bytes_to_f32_planar(oracle.FMT_S16LE, data, 2)
    mono = (ch[0] + ch[1]) * np.float32(0.5)
    assert np.abs(mono).max() < 0.01


def test_decoder_side_scales(oracle):  # audio_pipeline.rs:715-755 values, decoder lib.rs:3563-3617 scales
    be = np.array([0x7F, 0xFF, 0x80, 0x00], np.uint8)  # i16::MAX, i16::MIN big-endian
    ch = oracle.decoder_bytes_to_f32_planar(oracle.FMT_S16BE, be, 2)
    assert abs(ch[0, 0] - 32767.0 / 32768.0) < np.finfo(np.float32).eps and ch[1, 0] == -1.0
    s24 = np.array([0xFF, 0xFF, 0x7F, 0x00, 0x00, 0x80], np.uint8)
    ch = oracle.decoder_bytes_to_f32_planar(oracle.FMT_S24LE, s24, 2)
    assert abs(ch[0, 0] - 8388607.0 / 8388608.0) < np.finfo(np.float32).eps and ch[1, 0] == -1.0
    nan = np.array([np.nan], np.float32).view(np.uint8)
    assert oracle.decoder_bytes_to_f32_planar(oracle.FMT_F32LE, nan, 1)[0, 0] == 0.0


def test_float_sample_to_i16_semantics(oracle):  # soundkit-decoder lib.rs:1815-1827
    f = oracle.float_sample_to_i16
    assert f(1.0) == 32767 and f(-1.0) == -32768 and f(2.0) == 32767 and f(-2.0) == -32768
    assert f(float("nan")) == 0 and f(float("inf")) == 0
    assert f(0.5) == 16384   # 16383.5 rounds half away from zero
    assert f(-0.5) == -16384
    assert f(0.25) == 8192 and f(-0.25) == -8192 and f(1.0e-6) == 0


def test_rust_cast_semantics(oracle):  # audio_bytes.rs:167-220 (`as` casts saturate, NaN -> 0, truncate)
    x = np.array([np.nan, np.inf, -np.inf, 0.99999, -0.99999, 1.0, -1.0, 3.0e-5], np.float32)
    assert oracle.pcm_convert("F32LE_TO_I16", x).tolist() == [0, 32767, -32767, 32766, -32766, 32767, -32767, 0]
    got = oracle.pcm_convert("F32LE_TO_I32", x).tolist()
    assert got[0] == 0 and got[1] == 2147483647 and got[2] == -2147483648 and got[5] == 2147483647 and got[6] == -2147483648
    got = oracle.pcm_convert("F32LE_TO_S24", x).tolist()
    assert got[5] == 8388607 and got[6] == -8388608 and got[0] == 0


# ---- resampler: the reference pins lengths only (soundkit-decoder lib.rs:5188-5238) -------------

def test_streaming_resampler_matches_single_pass_length(oracle):
    n = 44100
    x = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / 44100.0)).astype(np.float32)[None]
    s = oracle.StreamingResampler(44100, 16000, 1)
    chunks = [s.process(x[:, i:i + 997]) for i in range(0, n, 997)]
    chunks.append(s.flush())
    one = oracle.StreamingResampler(44100, 16000, 1)
    single = [one.process(x), one.flush()]
    a, b = np.concatenate(chunks, 1), np.concatenate(single, 1)
    assert a.shape == b.shape and a.shape[1] > 0
    assert np.array_equal(a, b)


def test_downsample_48k_16k_is_phase0_fir(oracle):
    """At ratio 1/3 rubato's time step is exactly 3 and the fractional phase 0."""
    rng = np.random.default_rng(7)
    x = rng.uniform(-1, 1, (2, 3000)).astype(np.float32)
    y = oracle.downsample_planar(x, 48000, 16000)
    assert y.shape[1] == (3000 - 132 + 2) // 3
    taps = oracle.resampler_taps(16000 / 48000).astype(np.float64)
    m = 400
    ref = sum(taps[p] * x[0, 3 * m - 125 + p] for p in range(256))
    assert abs(y[0, m] - ref) < 1e-6
    assert abs(taps.sum() - 1.0) < 1e-4


def test_pcm_stats_fnv(oracle):  # aac-wasm-bench lib.rs:73-100
    st = oracle.pcm_stats(np.zeros(0, np.float32))
    assert st["checksum"] == 0xCBF29CE484222325 and st["rms"] == 0.0
    st = oracle.pcm_stats(np.array([1.0], np.float32))
    assert st["checksum"] == ((0xCBF29CE484222325 ^ 0x3F800000) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    assert st["rms"] == 1.0 and st["peak_abs"] == 1.0


def test_f64_free_rounding_equals_the_reference_form(tmp_path):
    """The device computes float_sample_to_i16 (soundkit-decoder lib.rs:1815-1827) without f64
    (csrc/sk_device.h dev_float_sample_to_i16_f32).  tools/check_f32_rounding.c holds both forms in C; this sweeps
    every f32 with |x| in [2^-20, 2] (all rounding boundaries), both signs, zeros, infinities and NaNs: 0 mismatches.
    (All 2^32 patterns were swept once: also 0.)"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "check_f32_rounding")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(root, "tools", "check_f32_rounding.c"), "-lm"])
    out = subprocess.run([exe, "boundaries"], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout
    # the C copy and the device source must stay the same expression
    dev = open(os.path.join(root, "soundkit_amd", "csrc", "sk_device.h")).read()
    for line in ("const float a = m * 32768.0f;", "const float k = floorf(a);", "const float d = a - k;",
                 "const int neg = ki + (d >= 0.5f ? 1 : 0);",
                 "const int pos = ki + ((d - 0.5f >= m) ? 1 : 0) - ((d + 0.5f < m) ? 1 : 0);"):
        assert line in dev, line


def test_config1_wav_stereo_plumbing_on_the_cpu_path(oracle):
    """BASELINE configs[0] ("plumbing, no GPU"): the reference's testdata/wav_stereo file (fixture copy) through
    s16le_to_i16 -> deinterleave_vecs_i16 -> vec_i16_to_f32 -> vec_f32_to_i16 -> interleave_vecs_i16 as restated by
    the oracle, checked against the definitions (audio_bytes.rs:231, :264, :250; audio_pipeline.rs:17-38).  The GPU
    suite runs the same chain through the product (tests/test_pcm_gpu.py::test_config1_wav_stereo_plumbing)."""
    path = T.golden("wav_stereo_A_Tusk.wav")
    assert os.path.getsize(path) == 189518
    fmt, pcm, ext = T.read_wav(path)  # the chunk walk of WavStreamProcessor::add (wav.rs:95-262): no 44-byte assumption
    assert ext is None
    assert fmt == (1, 2, 16000, 64000, 4, 16) and len(pcm) == 189440
    src = np.frombuffer(pcm, "<i2")
    i16 = oracle.pcm_convert("S16LE_TO_I16", pcm)
    assert np.array_equal(i16, src)
    planes = oracle.deinterleave("i16", pcm, 2)
    assert planes.shape == (2, 47360) and np.array_equal(planes[0], src[0::2]) and np.array_equal(planes[1], src[1::2])
    f = np.stack([oracle.pcm_convert("VEC_I16_TO_F32", planes[c]) for c in range(2)])
    assert f.dtype == np.float32 and np.array_equal(f, planes.astype(np.float32) / np.float32(32768.0))
    back = np.stack([oracle.pcm_convert("VEC_F32_TO_I16", f[c]) for c in range(2)])
    # (x / 32768) * 32767 truncated toward zero: never larger in magnitude than the source, off by at most one
    want = np.trunc(f.astype(np.float64) * 32767.0).astype(np.int16)
    assert np.all(np.abs(back.astype(np.int32)) <= np.abs(planes.astype(np.int32)))
    assert np.abs(back.astype(np.int32) - planes.astype(np.int32)).max() <= 1
    assert np.abs(back.astype(np.int32) - want.astype(np.int32)).max() <= 1
    inter = np.asarray(oracle.interleave_i16(back)).view("<i2")  # interleave_vecs_i16 returns little-endian bytes
    assert inter.shape == (2 * 47360,) and np.array_equal(inter[0::2], back[0]) and np.array_equal(inter[1::2], back[1])


# ---- the reference's twin recordings (tests/twin_fit.py, tests/golden/README.md) ---------------------------------------------
# The resampler part of the oracle is a restatement of rubato that everything else in this suite takes its taps,
# alignment and gain from.  These pins hold it against recordings the reference keeps of one clip at 48, 16 and 8 kHz: gain,
# delay and pass-band.  Tap identity stays unpinned (another good low-pass at the same cut and delay scores the same).

def _clip_f32(rate):
    return (T.twin_s16(rate).astype(np.float32) / np.float32(32768.0))[None]


@pytest.mark.parametrize("in_hz,out_hz", T.PAIRS)
def test_twin_downsample_planar(oracle, in_hz, out_hz):
    """downsample_audio (audio_pipeline.rs:438-493) of the higher-rate file meets the lower-rate file: every band's SNR, the
    gain and the delay (floors and measured figures: twin_fit.TWIN_PINS); so does the worker's full step, the same output
    through float_sample_to_i16 (soundkit-decoder lib.rs:1815-1827), at the floors of its own"""
    y = oracle.downsample_planar(_clip_f32(in_hz), in_hz, out_hz)[0]
    assert y.size == {(48000, 16000): 47316, (48000, 8000): 23658, (16000, 8000): 23615}[(in_hz, out_hz)]
    T.assert_twin(y, in_hz, out_hz, "f32", "oracle one-shot")
    q = oracle.pcm_convert("FLOAT_TO_I16_ROUND", y)
    assert np.array_equal(q, R.float_sample_to_i16(y))
    T.assert_twin(q.astype(np.float64) / 32768.0, in_hz, out_hz, "s16", "oracle one-shot, rounded")


def _chunk_sizes(chunking, total):
    if chunking == "ones":  # the first 2 000 samples one at a time, then larger chunks
        return [1] * 2000 + [4096] * ((total - 2000 + 4095) // 4096)
    size = total if chunking == "whole" else int(chunking)
    return [size] * ((total + size - 1) // size)


@pytest.mark.parametrize("chunking", ["ones", "417", "4800", "whole"])
@pytest.mark.parametrize("in_hz,out_hz", T.PAIRS)
def test_twin_streaming_resampler(oracle, in_hz, out_hz, chunking):
    """StreamingResampler (soundkit-decoder lib.rs:1917-2060) fed the higher-rate file in chunks and flushed: the same pins,
    and the samples do not depend on the chunking (they are the one-shot call's, which pads and trims the same way)"""
    x = _clip_f32(in_hz)
    s = oracle.StreamingResampler(in_hz, out_hz, 1)
    parts, pos = [], 0
    for size in _chunk_sizes(chunking, x.shape[1]):
        parts.append(s.process(x[:, pos:pos + size]))
        pos += size
    assert pos >= x.shape[1]
    parts.append(s.flush())
    y = np.concatenate(parts, 1)[0]
    T.assert_twin(y, in_hz, out_hz, "f32", "oracle streaming %s" % chunking)
    assert np.array_equal(y, oracle.downsample_planar(x, in_hz, out_hz)[0])


def _cut_taps(cut, like):
    """phase 0 of a Blackman-Harris^2 windowed sinc cut at `cut` of the output Nyquist, laid out and normalised as the
    oracle's 48 -> 16 kHz taps are (tap p sits at 256 p + 255 of the 65 536-point prototype, centre 32 768), in f64"""
    pos = 256.0 * np.arange(256) + 255.0
    a = 2.0 * np.pi * pos / 65536.0
    win = (0.35875 - 0.48829 * np.cos(a) + 0.14128 * np.cos(2 * a) - 0.01168 * np.cos(3 * a)) ** 2
    taps = win * np.sinc((pos - 32768.0) * (cut / 3.0) / 256.0)
    return taps * (like.sum() / taps.sum())


def _bf16_truncate(taps):
    return (np.asarray(taps, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def test_twin_fit_negative_controls(oracle):
    """What the pins tell apart, at 48 -> 16 kHz with the float64 FIR of tests/f64_ref.py: the unaltered filter passes, and each
    altered one fails the same assertion for its own reason (the quantity named in the message)."""
    x = _clip_f32(48000)
    taps = oracle.resampler_taps(16000 / 48000).astype(np.float64)
    n_out = 47316

    def run(label, **kw):
        return T.twin_findings(R.fir_48k_16k(x, n_out, **kw)[0], 48000, 16000)[0], label

    assert run("unaltered") == ([], "unaltered")
    T.assert_twin(R.fir_48k_16k(x, n_out)[0], 48000, 16000, "f32", "f64 FIR, the oracle's taps")
    # the 0.95 cut restated here is the oracle's filter to f32 rounding: the 0.80 control below differs in the cut alone
    assert np.abs(_cut_taps(0.95, taps) - taps).max() < 1e-6
    assert run("0.95 restated", taps=_cut_taps(0.95, taps)) == ([], "0.95 restated")

    zeroed = taps.copy()
    zeroed[100] = 0.0
    controls = [
        ("cut at 0.80 of Nyquist", dict(taps=_cut_taps(0.80, taps)), "snr<7000"),
        ("tap 100 zeroed", dict(taps=zeroed), "gain"),
        ("taps x 1.001", dict(taps=taps * 1.001), "gain"),
        ("alignment 3m - 126", dict(delay=R.FIR_DELAY + 1), "delay"),
        ("taps truncated to bf16", dict(taps=_bf16_truncate(taps)), "gain"),
    ]
    for label, kw, reason in controls:
        y = R.fir_48k_16k(x, n_out, **kw)[0]
        with pytest.raises(AssertionError, match=reason):
            T.assert_twin(y, 48000, 16000, "f32", label)
        tripped = T.twin_findings(y, 48000, 16000)[0]
        assert reason in tripped, (label, tripped)
        if label in ("taps x 1.001", "alignment 3m - 126"):  # SNR alone misses these two: the same filter otherwise
            assert tripped == [reason], (label, tripped)
    assert "snr<3000" in T.twin_findings(R.fir_48k_16k(x, n_out, taps=zeroed)[0], 48000, 16000)[0]


def test_twin_wav_headers():
    """the 24-bit and float32 WAVs are WAVE_FORMAT_EXTENSIBLE; the walk is WavStreamProcessor::add's (soundkit/src/wav.rs:95-262)"""
    for name, size, bits, align, code, data_len in (("wav_24_A_Tusk.wav", 142182, 24, 3, 1, 142080),
                                                    ("wav_32f_A_Tusk.wav", 189554, 32, 4, 3, 189440)):
        assert os.path.getsize(T.golden(name)) == size
        fmt, pcm, ext = T.read_wav(T.golden(name))
        assert fmt == (0xFFFE, 1, 16000, 16000 * align, align, bits), name
        assert ext == {"fmt_size": 40, "valid_bits": bits, "channel_mask": 4, "sub_format": code}, name
        assert len(pcm) == data_len == 47360 * align


def _s24_values(raw):
    b = np.asarray(raw, np.uint8).reshape(-1, 3).astype(np.int32)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    return np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.int32)


def test_twin_files_are_one_clip():
    """file to file, no code of ours between: the s32 file is the s16 file << 16, the 24-bit WAV is the s32 file >> 8, the float
    WAV is the s16 file / 32768; the 48 and 8 kHz files are exactly 3 x and 1/2 the length"""
    tw = T.pcm_twins()
    s16, s32, f32 = tw["s16"].view("<i2"), tw["s32"].view("<i4"), tw["f32"].view("<f4")
    assert s16.size == s32.size == f32.size == 47360 and tw["s24"].size == 3 * 47360
    assert T.twin_s16(48000).size == 142080 and T.twin_s16(8000).size == 23680
    assert np.array_equal(s32 >> 16, s16) and not np.any(s32 & 0xFFFF)
    assert np.array_equal(s32 >> 8, _s24_values(tw["s24"]))
    assert np.array_equal(f32.astype(np.float64) * 32768.0, s16.astype(np.float64))


def test_twin_pcm_relations_exact(oracle):
    """every conversion between the clip's four sample formats lands on the twin file bit for bit, whole file
    (audio_bytes.rs:3-373, audio_pipeline.rs:17-98, soundkit-decoder lib.rs:1815-1827, :3458, :3563-3660)"""
    tw = T.pcm_twins()
    s16, s32, f32 = tw["s16"].view("<i2"), tw["s32"].view("<i4"), tw["f32"].view("<f4")
    same = np.array_equal
    assert same(oracle.pcm_convert("S32LE_TO_I16", tw["s32"]), s16)
    assert same(oracle.exact_signed_pcm_to_i16(oracle.FMT_S32LE, tw["s32"]), tw["s16"])
    assert same(oracle.pcm_convert("S24LE_TO_I16", tw["s24"]), s16)
    assert same(oracle.exact_signed_pcm_to_i16(oracle.FMT_S24LE, tw["s24"]), tw["s16"])
    assert same(oracle.pcm_convert("I16LE_TO_F32", tw["s16"]).view(np.uint32), f32.view(np.uint32))
    assert same(oracle.pcm_convert("VEC_I16_TO_F32", s16).view(np.uint32), f32.view(np.uint32))
    assert same(oracle.pcm_convert("S32LE_TO_F32", tw["s32"]).view(np.uint32), f32.view(np.uint32))
    assert same(oracle.decoder_bytes_to_f32_planar(oracle.FMT_S32LE, tw["s32"], 1)[0].view(np.uint32), f32.view(np.uint32))
    assert same(oracle.core_bytes_to_f32_planar(oracle.FMT_S32LE, tw["s32"], 1)[0].view(np.uint32), f32.view(np.uint32))
    assert same(oracle.pcm_convert("FLOAT_TO_I16_ROUND", f32), s16)
    assert same(oracle.f32_planar_to_bytes(oracle.FMT_S16LE, f32[None]), tw["s16"])
    assert same(oracle.planar_f32_to_s16_interleaved(f32[None]), s16)
    assert same(oracle.pcm_convert("S24LE_TO_I32", tw["s24"]), s32 >> 8)


def _check_scaled_by_32767(got, s16):
    """F32LE_TO_I16 / VEC_F32_TO_I16 scale by 32767 and truncate (audio_bytes.rs:167-175): on x = s / 32768 they cannot give s
    back, but never exceed it in magnitude and miss it by one step at most"""
    got, s = got.astype(np.int32), s16.astype(np.int32)
    assert np.all(np.abs(got) <= np.abs(s)) and np.abs(got - s).max() <= 1
    assert np.array_equal(got, np.trunc(s.astype(np.float64) / 32768.0 * 32767.0).astype(np.int32))  # exact in f64, and f32 agrees


def test_twin_pcm_relations_that_are_not_identities(oracle):
    tw = T.pcm_twins()
    s16, s32, f32 = tw["s16"].view("<i2"), tw["s32"].view("<i4"), tw["f32"].view("<f4")
    _check_scaled_by_32767(oracle.pcm_convert("F32LE_TO_I16", tw["f32"]), s16)
    _check_scaled_by_32767(oracle.pcm_convert("VEC_F32_TO_I16", f32), s16)
    # S32LE_TO_S24 keeps the low 24 bits (audio_bytes.rs:101-110), which is not the 24-bit file's sample
    assert np.array_equal(oracle.pcm_convert("S32LE_TO_S24", tw["s32"]), s32 & 0x00FFFFFF)


def test_twin_big_endian_ops_equal_their_little_endian_forms(oracle):
    tw = T.pcm_twins()
    for be, le, key, width in (("S32BE_TO_I16", "S32LE_TO_I16", "s32", 4), ("S24BE_TO_I16", "S24LE_TO_I16", "s24", 3),
                               ("S32BE_TO_F32", "S32LE_TO_F32", "s32", 4), ("S32BE_TO_S24", "S32LE_TO_S24", "s32", 4),
                               ("S16BE_TO_I16", "S16LE_TO_I16", "s16", 2), ("F32BE_TO_I16", "F32LE_TO_I16", "f32", 4)):
        got = oracle.pcm_convert(be, T.swap_bytes(tw[key], width))
        want = oracle.pcm_convert(le, tw[key])
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), be
    assert np.array_equal(oracle.pcm_convert("S16BE_TO_I16", T.swap_bytes(tw["s16"], 2)), tw["s16"].view("<i2"))

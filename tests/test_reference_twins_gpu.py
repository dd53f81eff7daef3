"""The GPU resampler and PCM kernels on the reference's twin recordings of one clip (tests/twin_fit.py, tests/golden/README.md).

Every other resampler test compares a kernel with oracle/sk_oracle.c's restatement of rubato, or with tests/f64_ref.py, which
takes its taps, alignment and gain from that restatement.  Here the product's entry points resample the reference's 48 kHz (or
16 kHz) file and must meet its 16 kHz (or 8 kHz) file: gain, delay and pass-band, at the floors measured on the CPU oracle
(twin_fit.TWIN_PINS; none comes from a GPU run -- float32 error is some 60 dB below them).  Sample values are held against
float64 at the bounds tests/test_full_device_gpu.py measured and DESIGN.md records (FIR_F32_BOUND, FIR_F32_ABS, SINC_F64_BOUND),
on a signal unlike the seeded noise used there: the clip is quiet (RMS 281 of 32 768) with long near-silent stretches.
The PCM conversions must land on the twin *file* of the other sample format, bit for bit, over the whole 47 360 samples (not a
multiple of any kernel's vector width times its block size, so the tail path runs).

Tap identity with rubato stays unpinned: another good low-pass at the same cut and delay would pass the twin fit too.
Each test is a handful of short launches on the session's engine; nothing is retried."""
import numpy as np
import pytest

import f64_ref as R
import twin_fit as T
from soundkit_amd import audio_bytes, audio_pipeline, decoder
from soundkit_amd import engine as E
from soundkit_amd.audio_types import AudioData, EncodingFlag
from test_full_device_gpu import FIR_F32_ABS, FIR_F32_BOUND, SINC_F64_BOUND  # measured on MI355X at bench size

pytestmark = pytest.mark.gpu

OUT_FRAMES = {(48000, 16000): 47316, (48000, 8000): 23658, (16000, 8000): 23615}  # the oracle's, whole file (test_oracle_pins.py)


def _clip_f32(rate):
    return T.twin_s16(rate).astype(np.float32) / np.float32(32768.0)


def _f64_ref(x, in_hz, out_hz, n_out):
    """x [rows][T] f32 -> the float64 resampler of tests/f64_ref.py, [rows][n_out]"""
    if (in_hz, out_hz) == (48000, 16000):
        return R.fir_48k_16k(x, n_out)
    y = R.sinc_resample(x, in_hz, out_hz)
    assert y.shape[1] == n_out
    return y


def _bound(in_hz, out_hz):
    return FIR_F32_BOUND if (in_hz, out_hz) == (48000, 16000) else SINC_F64_BOUND


def _check_f32(got, want, in_hz, out_hz, label):
    """every row: relative RMS against float64 under the project's bound, largest error under FIR_F32_ABS"""
    assert got.shape == want.shape, (label, got.shape, want.shape)
    rel = np.sqrt(((got.astype(np.float64) - want) ** 2).mean(1) / (want ** 2).mean(1))
    worst_abs = np.abs(got - want).max()
    print("\n%s %d->%d: rel RMS vs f64 worst %.3g (row %d), max |err| %.3g over %d rows" % (
        label, in_hz, out_hz, rel.max(), int(rel.argmax()), worst_abs, got.shape[0]))
    assert rel.max() < _bound(in_hz, out_hz) and worst_abs < FIR_F32_ABS, (label, rel.max(), worst_abs)


def _check_s16(got, want64, label):
    """the 1-LSB rule of test_c_fir_frame_packed_forms: against float_sample_to_i16 of the float64 result, at most one step, and
    fewer than 1 % of a row's samples off by one"""
    want = R.float_sample_to_i16(want64.astype(np.float32)).astype(np.int32)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    d = np.abs(got.astype(np.int32) - want)
    ones = (d == 1).mean(1)
    print("\n%s: worst |d| %d, worst 1-LSB fraction %.5f over %d rows" % (label, d.max(), ones.max(), got.shape[0]))
    assert d.max() <= 1 and ones.max() < 0.01, (label, d.max(), ones.max())


def _shifted_rows(clip, n_rows, length):
    """row r = the clip from sample r on: every phase of 3 and every 16-byte misalignment of a row start occurs"""
    return np.stack([clip[r:r + length] for r in range(n_rows)])


# ---- the one-shot call ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_hz,out_hz", T.PAIRS)
def test_downsample_audio_meets_the_twin(engine, in_hz, out_hz):
    """audio_pipeline.downsample_audio on the file's bytes (one row: the MFMA FIR at 48 -> 16 kHz, the generic kernels otherwise,
    in their default and their exact scalar form): the oracle's output length, the twin fit, float64 sample values"""
    raw = np.fromfile(T.golden(T.TWIN_FILES[in_hz]), np.uint8)
    x = _clip_f32(in_hz)[None]
    want = _f64_ref(x, in_hz, out_hz, OUT_FRAMES[(in_hz, out_hz)])
    for exact in (False, True):
        engine.set_resampler_exact(exact)
        try:
            got = audio_pipeline.downsample_audio(AudioData(16, 1, in_hz, raw), out_hz)
        finally:
            engine.set_resampler_exact(False)
        label = "downsample_audio%s" % (" (exact form)" if exact else "")
        assert got.shape == (1, OUT_FRAMES[(in_hz, out_hz)])
        T.assert_twin(got[0], in_hz, out_hz, "f32", label)
        _check_f32(got, want, in_hz, out_hz, label)


# ---- batches: unaligned row starts and the kernels' row tiling -------------------------------------------------------------------

def test_batch_48k_16k_f32_rows(engine):
    """512 rows through engine.downsample (the MFMA FIR on f32 rows of odd length, so row starts fall on every 4-byte offset of a
    16-byte line): twice, bit-identical; every row against float64; row 0 meets the twin"""
    length = 142080 - 511
    x = _shifted_rows(_clip_f32(48000), 512, length)
    got, again = engine.downsample(x, 48000, 16000), engine.downsample(x, 48000, 16000)
    assert np.array_equal(got, again)
    n_out = engine.downsample_out_frames(length)
    assert got.shape == (512, n_out)
    _check_f32(got, R.fir_48k_16k(x, n_out), 48000, 16000, "batch f32 rows")
    T.assert_twin(got[0], 48000, 16000, "f32", "batch f32 rows, row 0")


@pytest.mark.parametrize("form", ["s16_to_s16", "s16_to_f32"])
def test_batch_48k_16k_frame_packed(engine, form):
    """the forms the tick uses, laid out as test_c_fir_frame_packed_forms lays them out: 512 mono streams x 138 frames of 1024
    s16 samples, stream r = the 48 kHz file from sample r on.  s16 -> s16 obeys the 1-LSB rule against the rounded float64
    filter, s16 -> f32 the float bounds; twice, bit-identical; stream 0 meets the twin (s16 output: at the rounded floors)"""
    import torch
    n_streams, n_frames, ch = 512, 138, 1
    rows = _shifted_rows(T.twin_s16(48000), n_streams, n_frames * 1024)
    x = torch.from_numpy(np.ascontiguousarray(rows.reshape(n_streams, n_frames, ch, 1024).transpose(1, 0, 2, 3))).cuda()
    strides = (ch * 1024, n_streams * ch * 1024)
    n_out = engine.downsample_out_frames(n_frames * 1024)
    outs = []
    for _ in range(2):
        if form == "s16_to_f32":
            stride = (n_out + 3) // 4 * 4
            y = torch.zeros((n_streams * ch, stride), device="cuda")
            torch.cuda.synchronize()  # inputs are produced on torch's stream, the engine runs on its own
            assert engine.downsample_48k_16k_frames_s16_to_f32_dev(x, *strides, ch, n_streams, n_frames, y, stride) == n_out
        else:
            stride = (n_out + 7) // 8 * 8
            y = torch.zeros((n_streams, stride, ch), dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            assert engine.downsample_48k_16k_frames_s16_to_s16_dev(x, *strides, ch, n_streams, n_frames, y, stride) == n_out
        engine.synchronize()
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    assert not outs[0][:, n_out:].any()  # nothing written past the outputs
    got = outs[0][:, :n_out].reshape(n_streams, n_out).cpu().numpy()
    want = R.s16_chain(rows, n_out)
    if form == "s16_to_f32":
        _check_f32(got, want, 48000, 16000, "frame-packed s16 -> f32")
        T.assert_twin(got[0], 48000, 16000, "f32", "frame-packed s16 -> f32, stream 0")
    else:
        _check_s16(got, want, "frame-packed s16 -> s16")
        T.assert_twin(got[0].astype(np.float64) / 32768.0, 48000, 16000, "s16", "frame-packed s16 -> s16, stream 0")


@pytest.mark.parametrize("exact", [False, True], ids=["mfma", "exact"])
@pytest.mark.parametrize("in_hz,out_hz", [(48000, 8000), (16000, 8000)])
def test_batch_generic_pairs(engine, oracle, in_hz, out_hz, exact):
    """64 rows through engine.downsample: k_sinc_taps + k_sinc_mfma (the default for batches) and the exact scalar form, which
    is the oracle's f32 restatement bit for bit (test_fir_gpu.py demands that of it).  Twice, bit-identical; every row against
    the float64 sinc walk; row 0 meets the twin"""
    clip = _clip_f32(in_hz)
    x = _shifted_rows(clip, 64, clip.size - 63)
    engine.set_resampler_exact(exact)
    try:
        got, again = engine.downsample(x, in_hz, out_hz), engine.downsample(x, in_hz, out_hz)
    finally:
        engine.set_resampler_exact(False)
    assert np.array_equal(got, again)
    if exact:
        assert np.array_equal(got, oracle.downsample_planar(x, in_hz, out_hz))
    label = "batch %s" % ("exact form" if exact else "mfma form")
    _check_f32(got, _f64_ref(x, in_hz, out_hz, got.shape[1]), in_hz, out_hz, label)
    T.assert_twin(got[0], in_hz, out_hz, "f32", label + ", row 0")


# ---- the streaming resampler and the worker's full step ---------------------------------------------------------------------------

@pytest.mark.parametrize("in_hz,out_hz", T.PAIRS)
def test_streaming_resampler_meets_the_twin(engine, in_hz, out_hz):
    """decoder.StreamingResampler (sk_resampler_open / process / flush) fed the file in chunks of 417, 4 800 and whole, flushed:
    the samples do not depend on the chunking (bit for bit, as test_fir_gpu.py demands), each passes the twin fit, and they
    are the one-shot call's samples within the float bounds (length included)"""
    x = _clip_f32(in_hz)[None]
    outs = []
    for chunk in (417, 4800, x.shape[1]):
        s = decoder.StreamingResampler(in_hz, out_hz, 1, engine)
        try:
            parts = [s.process(x[:, a:a + chunk]) for a in range(0, x.shape[1], chunk)] + [s.flush()]
        finally:
            s.close()
        y = np.concatenate(parts, 1)
        assert y.shape == (1, OUT_FRAMES[(in_hz, out_hz)]), chunk
        T.assert_twin(y[0], in_hz, out_hz, "f32", "streaming, chunks of %d" % chunk)
        outs.append(y)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    _check_f32(outs[0], _f64_ref(x, in_hz, out_hz, outs[0].shape[1]), in_hz, out_hz, "streaming")


@pytest.mark.parametrize("in_hz,out_hz", T.PAIRS)
def test_worker_step_to_s16_meets_the_twin(engine, in_hz, out_hz):
    """the worker's full step (soundkit-decoder lib.rs:3324-3456): apply_output_options with another rate and 16 bits resamples
    chunk by chunk and narrows each with float_sample_to_i16 on the device, flush_resampler_frames brings the rest.  The s16
    stream obeys the 1-LSB rule against the rounded float64 reference and meets the twin at the floors measured on the rounded
    CPU oracle output (rounding costs up to 7 dB in the lowest band, so the f32 floors do not apply)"""
    raw = np.fromfile(T.golden(T.TWIN_FILES[in_hz]), np.uint8)
    outs, rs = decoder.apply_output_options(AudioData(16, 1, in_hz, raw), output_sample_rate=out_hz)
    try:
        outs = outs + decoder.flush_resampler_frames(rs, 16, 1)
    finally:
        rs.close()
    assert all(o.bits_per_sample == 16 and o.channel_count == 1 and o.sampling_rate == out_hz
               and o.audio_format == EncodingFlag.PCMSigned for o in outs)
    got = np.concatenate([np.asarray(o.data, np.uint8) for o in outs]).view("<i2")[None]
    n_out = OUT_FRAMES[(in_hz, out_hz)]
    assert got.shape == (1, n_out)
    _check_s16(got, _f64_ref(_clip_f32(in_hz)[None], in_hz, out_hz, n_out), "worker step %d->%d" % (in_hz, out_hz))
    T.assert_twin(got[0].astype(np.float64) / 32768.0, in_hz, out_hz, "s16", "worker step")


# ---- PCM conversions: each lands on the twin file ---------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_pcm_relations_exact(engine):
    """every conversion between the clip's four sample formats, through the product's entry points, gives the twin file's bytes"""
    tw = T.pcm_twins()
    s16, s32, f32 = tw["s16"].view("<i2"), tw["s32"].view("<i4"), tw["f32"].view("<f4")
    same = np.array_equal
    assert same(audio_bytes.s32le_to_i16(tw["s32"]), s16)
    assert same(engine.exact_to_i16(E.FMT_S32LE, tw["s32"]), tw["s16"])
    assert same(audio_bytes.s24le_to_i16(tw["s24"]), s16)
    assert same(engine.exact_to_i16(E.FMT_S24LE, tw["s24"]), tw["s16"])
    for got in (audio_bytes.i16le_to_f32(tw["s16"]), audio_pipeline.vec_i16_to_f32(s16), audio_bytes.s32le_to_f32(tw["s32"]),
                engine.bytes_to_f32_planar(0, E.FMT_S32LE, tw["s32"], 1)[0], engine.bytes_to_f32_planar(1, E.FMT_S32LE, tw["s32"], 1)[0],
                engine.bytes_to_f32_planar(0, E.FMT_S16LE, tw["s16"], 1)[0], engine.bytes_to_f32_planar(1, E.FMT_S16LE, tw["s16"], 1)[0]):
        assert got.dtype == np.float32 and same(_bits(got), tw["f32"])
    assert same(decoder.float_sample_to_i16(f32), s16)
    assert same(engine.f32_planar_to_bytes(E.FMT_S16LE, f32[None]), tw["s16"])
    assert same(decoder.f32_channels_to_bytes(f32[None], 16, EncodingFlag.PCMSigned), tw["s16"])
    assert same(audio_bytes.s24le_to_i32(tw["s24"]), s32 >> 8)
    assert same(audio_bytes.s32le_to_i32(tw["s32"]), s32)


def test_pcm_relations_that_are_not_identities(engine, oracle):
    """F32LE_TO_I16 / VEC_F32_TO_I16 scale by 32767 and truncate (audio_bytes.rs:167-175): never larger in magnitude than the s16
    twin, one step off at most, and the oracle's bytes.  S32LE_TO_S24 keeps the low 24 bits (audio_bytes.rs:101-110)"""
    tw = T.pcm_twins()
    s16, s32, f32 = tw["s16"].view("<i2").astype(np.int32), tw["s32"].view("<i4"), tw["f32"].view("<f4")
    for got, op, data in ((audio_bytes.f32le_to_i16(tw["f32"]), "F32LE_TO_I16", tw["f32"]), (audio_pipeline.vec_f32_to_i16(f32), "VEC_F32_TO_I16", f32)):
        g = got.astype(np.int32)
        assert np.all(np.abs(g) <= np.abs(s16)) and np.abs(g - s16).max() <= 1
        assert np.array_equal(g, np.trunc(s16.astype(np.float64) / 32768.0 * 32767.0).astype(np.int32))
        assert np.array_equal(got, oracle.pcm_convert(op, data))
    got = audio_bytes.s32le_to_s24(tw["s32"])
    assert np.array_equal(got, s32 & 0x00FFFFFF) and np.array_equal(got, oracle.pcm_convert("S32LE_TO_S24", tw["s32"]))


def test_pcm_big_endian_ops_equal_their_little_endian_forms(engine):
    tw = T.pcm_twins()
    s16 = tw["s16"].view("<i2")
    for be, le, key, width in ((audio_bytes.s32be_to_i16, audio_bytes.s32le_to_i16, "s32", 4), (audio_bytes.s24be_to_i16, audio_bytes.s24le_to_i16, "s24", 3),
                               (audio_bytes.s32be_to_f32, audio_bytes.s32le_to_f32, "s32", 4), (audio_bytes.s32be_to_s24, audio_bytes.s32le_to_s24, "s32", 4),
                               (audio_bytes.s16be_to_i16, audio_bytes.s16le_to_i16, "s16", 2), (audio_bytes.f32be_to_i16, audio_bytes.f32le_to_i16, "f32", 4)):
        got, want = be(T.swap_bytes(tw[key], width)), le(tw[key])
        assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want)), be.__name__
    # and the twin itself where the relation is an identity
    assert np.array_equal(audio_bytes.s32be_to_i16(T.swap_bytes(tw["s32"], 4)), s16)
    assert np.array_equal(audio_bytes.s24be_to_i16(T.swap_bytes(tw["s24"], 3)), s16)
    assert np.array_equal(audio_bytes.s16be_to_i16(T.swap_bytes(tw["s16"], 2)), s16)
    assert np.array_equal(_bits(audio_bytes.s32be_to_f32(T.swap_bytes(tw["s32"], 4))), tw["f32"])
    for fmt, key, width in ((E.FMT_S32BE, "s32", 4), (E.FMT_S24BE, "s24", 3)):
        assert np.array_equal(engine.exact_to_i16(fmt, T.swap_bytes(tw[key], width)), tw["s16"])


def test_apply_output_options_lands_on_the_s16_twin(engine):
    """decoder.apply_output_options(output_bits_per_sample=16): the 24-bit and 32-bit integer files by exact narrowing
    (lib.rs:3458), the float file through the float path (float_sample_to_i16) -- each gives exactly the bytes of the s16 file"""
    tw = T.pcm_twins()
    for bits, key, flag in ((24, "s24", EncodingFlag.PCMSigned), (32, "s32", EncodingFlag.PCMSigned), (32, "f32", EncodingFlag.PCMFloat)):
        out, _ = decoder.apply_output_options(AudioData(bits, 1, 16000, tw[key], flag), output_bits_per_sample=16)
        assert len(out) == 1 and (out[0].bits_per_sample, out[0].channel_count, out[0].sampling_rate) == (16, 1, 16000)
        assert out[0].audio_format == EncodingFlag.PCMSigned
        assert np.array_equal(np.asarray(out[0].data, np.uint8), tw["s16"]), key

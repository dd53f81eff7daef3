"""Engine: thin object wrapper over the C ABI (include/soundkit_amd.h).

Host entry points take/return numpy arrays; the *_dev entry points take device addresses
(ints, or anything with .data_ptr() such as a torch tensor) and enqueue on the engine's
HIP stream.  All compute happens in libsoundkit_amd.so on the GPU.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import FrameDesc, check, lib

ONLY_LONG, LONG_START, EIGHT_SHORT, LONG_STOP = 0, 1, 2, 3
SINE, KBD = 0, 1

FMT_S16LE, FMT_S16BE, FMT_S24LE, FMT_S24BE, FMT_S32LE, FMT_S32BE, FMT_F32LE, FMT_F32BE = range(8)
# enum sk_aiff_encoding: how an AIFF / AIFF-C file encodes its samples
(AIFF_U8, AIFF_S8, AIFF_S16BE, AIFF_S16LE, AIFF_S24BE, AIFF_S32BE, AIFF_S32LE, AIFF_F32BE, AIFF_F64BE, AIFF_ULAW, AIFF_ALAW,
 AIFF_IMA4, _, AIFF_F64LE, AIFF_DVD_S24) = range(15)  # 12 is unassigned and refused; AIFF_F64LE = 13: container PCM only (QuickTime `fl64` with enda = 1); no AIFF-C file holds it; AIFF_DVD_S24 = 14: DVD LPCM's 24-bit groups (12 bytes = four samples), MPEG program streams only
AIFF_GROUP_BYTES = {AIFF_U8: 1, AIFF_S8: 1, AIFF_S16BE: 2, AIFF_S16LE: 2, AIFF_S24BE: 3, AIFF_S32BE: 4, AIFF_S32LE: 4, AIFF_F32BE: 4,
                    AIFF_F64BE: 8, AIFF_ULAW: 1, AIFF_ALAW: 1, AIFF_F64LE: 8, AIFF_DVD_S24: 12}  # IMA4: 34 bytes per channel

# enum sk_wav_tag: the format tags the coded WAV walker takes; WAV_BAD_BLOCK = SK_WAV_BAD_BLOCK, a block's status
WAV_TAG_PCM, WAV_TAG_MS_ADPCM, WAV_TAG_FLOAT, WAV_TAG_ALAW, WAV_TAG_ULAW, WAV_TAG_IMA_ADPCM = 1, 2, 3, 6, 7, 0x11
WAV_BAD_BLOCK = -1201
WAV_NO_FRAME_CAP = 0xFFFFFFFFFFFFFFFF


def wav_adpcm_block_frames(tag, channels, block_align):
    """Frames of one ADPCM block of nBlockAlign bytes; 0 where the size is no block of the tag."""
    if channels not in (1, 2):
        return 0
    if tag == WAV_TAG_IMA_ADPCM:
        return 0 if block_align < 4 * channels or block_align % (4 * channels) else (block_align - 4 * channels) * 2 // channels + 1
    if tag == WAV_TAG_MS_ADPCM:
        return 0 if block_align < 7 * channels else (block_align - 7 * channels) * 2 // channels + 2
    return 0


PCM_OPS = [
    "I16LE_TO_F32", "I16_TO_I16LE", "I16LE_TO_I16", "S24LE_TO_I32", "S24LE_TO_I16", "S24BE_TO_I16",
    "S32LE_TO_I32", "S32BE_TO_I32", "S32LE_TO_S24", "S32BE_TO_S24", "S32LE_TO_F32", "S32BE_TO_F32",
    "S32LE_TO_I16", "S32BE_TO_I16", "F32LE_TO_I16", "F32BE_TO_I16", "F32LE_TO_I32", "F32LE_TO_S24",
    "S16BE_TO_I16", "S16LE_TO_I16", "S16LE_TO_I32", "STEREO_TO_MONO_TAKE_LEFT", "STEREO_TO_MONO_AVG",
    "VEC_F32_TO_I16", "VEC_I16_TO_F32", "VEC_I32_TO_F32", "FLOAT_TO_I16_ROUND", "MP3_F32_TO_I16",
    "MP3_F32_TO_I32",
]
PCM_OP = {name: i for i, name in enumerate(PCM_OPS)}


def _ptr(x):
    """Device or host address of x (torch tensor, numpy array, int or None)."""
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    if isinstance(x, np.ndarray):
        return C.c_void_p(x.ctypes.data)
    raise TypeError("cannot take the address of %r" % type(x))


def make_descs(frames):
    """frames: iterable of (stream, channels, (seq...), (shape...)) -> ctypes array of sk_aac_frame_desc."""
    frames = list(frames)
    arr = (FrameDesc * max(len(frames), 1))()
    for i, (stream, ch, seqs, shapes) in enumerate(frames):
        d = arr[i]
        d.stream = stream
        d.channels = ch
        for c in range(min(ch, 2)):
            d.window_sequence[c] = seqs[c]
            d.window_shape[c] = shapes[c]
    return arr, len(frames)


def descs_from_arrays(streams, channels, seqs, shapes):
    """Vectorised builder: streams [n], channels scalar or [n], seqs/shapes [n][2] -> (ctypes array, n)."""
    streams = np.asarray(streams, np.uint32)
    n = streams.size
    raw = np.zeros(n, dtype=np.dtype([("stream", "<u4"), ("channels", "u1"), ("seq", "u1", (2,)),
                                      ("shape", "u1", (2,)), ("reserved", "u1", (3,))]))
    assert raw.dtype.itemsize == C.sizeof(FrameDesc)
    raw["stream"] = streams
    raw["channels"] = channels
    raw["seq"] = np.asarray(seqs, np.uint8).reshape(n, 2)
    raw["shape"] = np.asarray(shapes, np.uint8).reshape(n, 2)
    arr = (FrameDesc * max(n, 1)).from_buffer_copy(raw.tobytes() if n else bytes(C.sizeof(FrameDesc)))
    return arr, n


class Plan:
    """A validated, device-resident schedule of AAC frames (sk_aac_plan)."""

    def __init__(self, engine, descs, n):
        self.engine = engine
        self.n = n
        self.status = np.zeros(max(n, 1), np.int32)
        h = C.c_void_p()
        check(lib.sk_aac_plan_create(engine._h, descs, n, _ptr(self.status), C.byref(h)), "sk_aac_plan_create", engine._h)
        self._h = h
        self.status = self.status[:n]
        self.elements = int(lib.sk_aac_plan_elements(h))
        self.frames_ok = int(lib.sk_aac_plan_frames_ok(h))

    def run_f32(self, d_coeffs, d_pcm):
        check(lib.sk_aac_plan_run_f32_dev(self.engine._h, self._h, _ptr(d_coeffs), _ptr(d_pcm)),
              "sk_aac_plan_run_f32_dev", self.engine._h)

    def run_s16_planar(self, d_coeffs, d_pcm16):
        """planar s16 PCM (float_sample_to_i16 of every sample), same packing as run_f32's output"""
        check(lib.sk_aac_plan_run_s16_planar_dev(self.engine._h, self._h, _ptr(d_coeffs), _ptr(d_pcm16)),
              "sk_aac_plan_run_s16_planar_dev", self.engine._h)

    def run_tail_s16(self, d_coeffs, stream_stride, channels, frames_per_stream, d_out, out_stride):
        """sk_aac_plan_run_tail_s16_dev: run_s16_planar + the one-shot 48k->16k FIR to interleaved s16 as one launch.  WITHDRAWN:
        raises SoundkitError -6 (unsupported) unless SK_AAC_TAIL_ONE_LAUNCH=1 is set -- the kernel is computed wrongly by the platform
        once several workgroups share a CU (include/soundkit_amd.h); also -6 for plans the fused kernel does not cover"""
        got = C.c_uint32()
        check(lib.sk_aac_plan_run_tail_s16_dev(self.engine._h, self._h, _ptr(d_coeffs), stream_stride, channels, frames_per_stream,
                                               _ptr(d_out), out_stride, C.byref(got)), "sk_aac_plan_run_tail_s16_dev", self.engine._h)
        return got.value

    def run_s16(self, d_coeffs, d_pcm):
        check(lib.sk_aac_plan_run_s16_dev(self.engine._h, self._h, _ptr(d_coeffs), _ptr(d_pcm)),
              "sk_aac_plan_run_s16_dev", self.engine._h)

    def destroy(self):
        if self._h:
            lib.sk_aac_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Engine:
    def __init__(self, device=0, max_streams=4096):
        h = C.c_void_p()
        check(lib.sk_engine_create(device, max_streams, C.byref(h)), "sk_engine_create")
        self._h = h
        self.device = device
        self.max_streams = max_streams
        self._channels = {}

    # ---- lifetime ---------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            lib.sk_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def hip_stream(self):
        return lib.sk_engine_hip_stream(self._h)

    def synchronize(self):
        check(lib.sk_engine_synchronize(self._h), "sk_engine_synchronize", self._h)

    # ---- streams ----------------------------------------------------------------------
    def enable_wide_pcm(self, max_wide_streams):
        """Reserve slots for PCM streams of 3 ... 8 channels (sk_engine_enable_wide_pcm): once, before the first resampler_open."""
        check(lib.sk_engine_enable_wide_pcm(self._h, int(max_wide_streams)), "sk_engine_enable_wide_pcm", self._h)

    @property
    def wide_pcm_streams(self):
        return int(lib.sk_engine_wide_pcm_streams(self._h))

    def open_stream(self, sample_rate=48000, channels=2):
        sid = C.c_uint32()
        check(lib.sk_stream_open(self._h, sample_rate, channels, C.byref(sid)), "sk_stream_open", self._h)
        self._channels[sid.value] = channels
        return sid.value

    def close_stream(self, sid):
        check(lib.sk_stream_close(self._h, sid), "sk_stream_close", self._h)

    def reset_stream(self, sid):
        check(lib.sk_stream_reset(self._h, sid), "sk_stream_reset", self._h)

    def get_state(self, sid, channels):
        delay = np.zeros((channels, 1024), np.float32)
        shape = np.zeros(channels, np.uint8)
        check(lib.sk_stream_get_state(self._h, sid, _ptr(delay), _ptr(shape)), "sk_stream_get_state", self._h)
        return delay, shape

    def set_state(self, sid, delay, shape):
        delay = np.ascontiguousarray(delay, np.float32)
        shape = np.ascontiguousarray(shape, np.uint8)
        check(lib.sk_stream_set_state(self._h, sid, _ptr(delay), _ptr(shape)), "sk_stream_set_state", self._h)

    # ---- AAC synthesis ----------------------------------------------------------------
    def plan(self, descs, n):
        return Plan(self, descs, n)

    def aac_synthesize(self, descs, n, coeffs, out="f32", pcm=None):
        """Host-buffer batch synthesis.  coeffs: packed f32 (sum(ch) * 1024).  Returns (pcm, status)."""
        coeffs = np.ascontiguousarray(coeffs, np.float32).ravel()
        status = np.zeros(max(n, 1), np.int32)
        if out == "f32":
            if pcm is None:
                pcm = np.zeros(coeffs.size, np.float32)
            rc = lib.sk_aac_synthesize_f32(self._h, descs, _ptr(coeffs), _ptr(pcm), n, _ptr(status))
        else:
            if pcm is None:
                pcm = np.zeros(coeffs.size, np.int16)
            rc = lib.sk_aac_synthesize_s16(self._h, descs, _ptr(coeffs), _ptr(pcm), n, _ptr(status))
        check(rc, "sk_aac_synthesize_" + out, self._h)
        return pcm, status[:n]

    def dequantize(self, quant, scalefactor):
        quant = np.ascontiguousarray(quant, np.int16).ravel()
        scalefactor = np.ascontiguousarray(scalefactor, np.int16).ravel()
        assert quant.size == scalefactor.size
        out = np.zeros(quant.size, np.float32)
        check(lib.sk_aac_dequantize(self._h, _ptr(quant), _ptr(scalefactor), _ptr(out), quant.size),
              "sk_aac_dequantize", self._h)
        return out

    # ---- PCM ---------------------------------------------------------------------------
    @staticmethod
    def _op_out_dtype(op):
        name = PCM_OPS[op]
        ob = lib.sk_pcm_op_out_bytes(op)
        if ob == 2:
            return np.int16
        return np.float32 if name.endswith("_F32") else np.int32

    def pcm_convert(self, op, data, n=None):
        if isinstance(op, str):
            op = PCM_OP[op]
        raw = np.ascontiguousarray(data).view(np.uint8).ravel()
        if n is None:
            n = raw.size // lib.sk_pcm_op_in_bytes(op)
        out = np.zeros(n, self._op_out_dtype(op))
        check(lib.sk_pcm_convert(self._h, op, _ptr(raw), _ptr(out), n), "sk_pcm_convert", self._h)
        return out

    def pcm_convert_dev(self, op, d_in, d_out, n):
        if isinstance(op, str):
            op = PCM_OP[op]
        check(lib.sk_pcm_convert_dev(self._h, op, _ptr(d_in), _ptr(d_out), n), "sk_pcm_convert_dev", self._h)

    def interleave_i16(self, planar):
        planar = np.ascontiguousarray(planar, np.int16)
        ch, frames = planar.shape
        out = np.zeros(ch * frames * 2, np.uint8)
        check(lib.sk_pcm_interleave_i16(self._h, _ptr(planar), frames, ch, _ptr(out)), "sk_pcm_interleave_i16", self._h)
        return out

    def deinterleave(self, kind, data, ch):
        raw = np.ascontiguousarray(data).view(np.uint8).ravel()
        bps = {"i16": 2, "s24": 3, "f32": 4}[kind]
        dt = {"i16": np.int16, "s24": np.int32, "f32": np.float32}[kind]
        frames = raw.size // (bps * ch)
        out = np.zeros((ch, frames), dt)
        fn = getattr(lib, "sk_pcm_deinterleave_" + kind)
        check(fn(self._h, _ptr(raw), frames, ch, _ptr(out)), "sk_pcm_deinterleave_" + kind, self._h)
        return out

    def interleave_f32(self, planar):
        planar = np.ascontiguousarray(planar, np.float32)
        ch, frames = planar.shape
        out = np.zeros(ch * frames * 4, np.uint8)
        check(lib.sk_pcm_interleave_f32(self._h, _ptr(planar), frames, ch, _ptr(out)), "sk_pcm_interleave_f32", self._h)
        return out

    def bytes_to_f32_planar(self, variant, fmt, data, ch):
        raw = np.ascontiguousarray(data).view(np.uint8).ravel()
        frames = raw.size // (lib.sk_pcm_fmt_bytes(fmt) * ch)
        out = np.zeros((ch, frames), np.float32)
        check(lib.sk_pcm_bytes_to_f32_planar(self._h, variant, fmt, _ptr(raw), frames, ch, _ptr(out)),
              "sk_pcm_bytes_to_f32_planar", self._h)
        return out

    def f32_planar_to_bytes(self, fmt, planar):
        planar = np.ascontiguousarray(planar, np.float32)
        ch, frames = planar.shape
        out = np.zeros(ch * frames * lib.sk_pcm_fmt_bytes(fmt), np.uint8)
        check(lib.sk_pcm_f32_planar_to_bytes(self._h, fmt, _ptr(planar), frames, ch, _ptr(out)),
              "sk_pcm_f32_planar_to_bytes", self._h)
        return out

    def downmix_mono(self, planar):
        planar = np.ascontiguousarray(planar, np.float32)
        ch, frames = planar.shape
        out = np.zeros(frames, np.float32)
        check(lib.sk_pcm_downmix_mono(self._h, _ptr(planar), frames, ch, _ptr(out)), "sk_pcm_downmix_mono", self._h)
        return out

    def downmix(self, planar, target):
        """downmix_channels (soundkit-decoder lib.rs:3492-3561): [ch][frames] f32, ch <= 8 -> [min(target, ch)][frames]."""
        planar = np.ascontiguousarray(planar, np.float32)
        ch, frames = planar.shape
        out = np.zeros((min(int(target), ch), frames), np.float32)
        check(lib.sk_pcm_downmix(self._h, _ptr(planar), frames, ch, int(target), _ptr(out)), "sk_pcm_downmix", self._h)
        return out

    def exact_to_i16(self, fmt, data):
        raw = np.ascontiguousarray(data).view(np.uint8).ravel()
        n = raw.size // lib.sk_pcm_fmt_bytes(fmt)
        out = np.zeros(n * 2, np.uint8)
        check(lib.sk_pcm_exact_to_i16(self._h, fmt, _ptr(raw), n, _ptr(out)), "sk_pcm_exact_to_i16", self._h)
        return out

    # ---- resampling ---------------------------------------------------------------------
    @staticmethod
    def downsample_out_frames(frames, in_hz=48000, out_hz=16000):
        if (in_hz, out_hz) == (48000, 16000):
            return int(lib.sk_downsample_48k_16k_out_frames(frames))
        return int(lib.sk_downsample_out_frames(frames, in_hz, out_hz))

    def taps(self):
        t = np.zeros(256, np.float32)
        check(lib.sk_downsample_48k_16k_taps(self._h, _ptr(t)), "sk_downsample_48k_16k_taps", self._h)
        return t

    def downsample_48k_16k(self, rows):
        """rows: [n_rows][frames] f32 -> [n_rows][out_frames]"""
        rows = np.ascontiguousarray(rows, np.float32)
        n_rows, frames = rows.shape
        n_out = self.downsample_out_frames(frames)
        out = np.zeros((n_rows, n_out), np.float32)
        got = C.c_uint32()
        check(lib.sk_downsample_48k_16k_f32(self._h, _ptr(rows), n_rows, frames, _ptr(out), C.byref(got)),
              "sk_downsample_48k_16k_f32", self._h)
        assert got.value == n_out
        return out

    def downsample_48k_16k_dev(self, d_in, in_stride, rows, frames, d_out, out_stride):
        got = C.c_uint32()
        check(lib.sk_downsample_48k_16k_f32_dev(self._h, _ptr(d_in), in_stride, rows, frames, _ptr(d_out), out_stride,
                                                C.byref(got)), "sk_downsample_48k_16k_f32_dev", self._h)
        return got.value

    def downsample_dev(self, d_in, in_stride, rows, frames, in_hz, out_hz, d_out, out_stride):
        """sk_downsample_f32_dev: one-shot downsample_audio of device rows, any pair of the reference's common rates"""
        got = C.c_uint32()
        check(lib.sk_downsample_f32_dev(self._h, _ptr(d_in), in_stride, rows, frames, in_hz, out_hz, _ptr(d_out), out_stride, C.byref(got)),
              "sk_downsample_f32_dev", self._h)
        return got.value

    def downsample(self, rows, in_hz, out_hz):
        """rows: [n_rows][frames] f32 -> [n_rows][out_frames], any pair of the reference's common rates."""
        rows = np.ascontiguousarray(rows, np.float32)
        n_rows, frames = rows.shape
        n_out = int(lib.sk_downsample_out_frames(frames, in_hz, out_hz))
        out = np.zeros((n_rows, n_out), np.float32)
        got = C.c_uint32()
        check(lib.sk_downsample_f32(self._h, _ptr(rows), n_rows, frames, in_hz, out_hz, _ptr(out), n_out, C.byref(got)),
              "sk_downsample_f32", self._h)
        assert got.value == n_out
        return out

    def downsample_48k_16k_frames_s16_dev(self, d_pcm, stream_stride, frame_stride, channels, n_streams, frames_per_stream,
                                          d_out, out_stride):
        """FIR with the s16 output stage fused: d_out [n_streams][out_stride][channels] int16."""
        got = C.c_uint32()
        check(lib.sk_downsample_48k_16k_frames_s16_dev(self._h, _ptr(d_pcm), stream_stride, frame_stride, channels, n_streams,
                                                       frames_per_stream, _ptr(d_out), out_stride, C.byref(got)),
              "sk_downsample_48k_16k_frames_s16_dev", self._h)
        return got.value

    def downsample_48k_16k_frames_s16_to_s16_dev(self, d_pcm16, stream_stride, frame_stride, channels, n_streams, frames_per_stream,
                                                 d_out, out_stride):
        """the worker's resample step on planar s16 PCM (Plan.run_s16_planar): d_out [n_streams][out_stride][channels] int16"""
        got = C.c_uint32()
        check(lib.sk_downsample_48k_16k_frames_s16_to_s16_dev(self._h, _ptr(d_pcm16), stream_stride, frame_stride, channels,
                                                              n_streams, frames_per_stream, _ptr(d_out), out_stride, C.byref(got)),
              "sk_downsample_48k_16k_frames_s16_to_s16_dev", self._h)
        return got.value

    def downsample_48k_16k_frames_s16_to_f32_dev(self, d_pcm16, stream_stride, frame_stride, channels, n_streams, frames_per_stream,
                                                 d_out, out_stride):
        got = C.c_uint32()
        check(lib.sk_downsample_48k_16k_frames_s16_to_f32_dev(self._h, _ptr(d_pcm16), stream_stride, frame_stride, channels,
                                                              n_streams, frames_per_stream, _ptr(d_out), out_stride, C.byref(got)),
              "sk_downsample_48k_16k_frames_s16_to_f32_dev", self._h)
        return got.value

    def downsample_frames_s16_to_s16_dev(self, d_pcm16, stream_stride, frame_stride, channels, n_streams, frames_per_stream,
                                         in_hz, out_hz, d_out, out_stride):
        """the same resample step at any pair of the common rates the matrix-core resampler takes (one-shot, planar s16 frames in):
        d_out [n_streams][out_stride][channels] int16; returns downsample_out_frames(frames_per_stream * 1024, in_hz, out_hz)"""
        got = C.c_uint32()
        check(lib.sk_downsample_frames_s16_to_s16_dev(self._h, _ptr(d_pcm16), stream_stride, frame_stride, channels, n_streams,
                                                      frames_per_stream, in_hz, out_hz, _ptr(d_out), out_stride, C.byref(got)),
              "sk_downsample_frames_s16_to_s16_dev", self._h)
        return got.value

    def downsample_frames_s16_to_f32_dev(self, d_pcm16, stream_stride, frame_stride, channels, n_streams, frames_per_stream,
                                         in_hz, out_hz, d_out, out_stride):
        """the filter output before the 16-bit stage: d_out [n_streams * channels][out_stride] float32"""
        got = C.c_uint32()
        check(lib.sk_downsample_frames_s16_to_f32_dev(self._h, _ptr(d_pcm16), stream_stride, frame_stride, channels, n_streams,
                                                      frames_per_stream, in_hz, out_hz, _ptr(d_out), out_stride, C.byref(got)),
              "sk_downsample_frames_s16_to_f32_dev", self._h)
        return got.value

    def downsample_48k_16k_frames_dev(self, d_pcm, stream_stride, frame_stride, channels, n_streams, frames_per_stream,
                                      d_out, out_stride):
        got = C.c_uint32()
        check(lib.sk_downsample_48k_16k_frames_dev(self._h, _ptr(d_pcm), stream_stride, frame_stride, channels, n_streams,
                                                   frames_per_stream, _ptr(d_out), out_stride, C.byref(got)),
              "sk_downsample_48k_16k_frames_dev", self._h)
        return got.value

    def f32_planar_to_bytes_batch_dev(self, fmt, d_planar, batch, plane_stride, frames, ch, d_out):
        check(lib.sk_pcm_f32_planar_to_bytes_batch_dev(self._h, fmt, _ptr(d_planar), batch, plane_stride, frames, ch,
                                                       _ptr(d_out)), "sk_pcm_f32_planar_to_bytes_batch_dev", self._h)

    _rs_ratio_max = 96000 / 8000  # largest ratio among the common rates: sizes host output buffers

    def resampler_open(self, sid, in_hz=48000, out_hz=16000):
        check(lib.sk_resampler_open(self._h, sid, in_hz, out_hz), "sk_resampler_open", self._h)

    def resampler_close(self, sid):
        check(lib.sk_resampler_close(self._h, sid), "sk_resampler_close", self._h)

    def resampler_process(self, sids, data, channels):
        """data: [n_streams][channels][frames] f32 -> list of [channels][out_frames] arrays."""
        sids = np.ascontiguousarray(sids, np.uint32)
        data = np.ascontiguousarray(data, np.float32)
        n, ch, frames = data.shape
        assert ch == channels
        cap = int((frames + 4096) * self._rs_ratio_max + 64)
        out = np.zeros((n, ch, cap), np.float32)
        got = np.zeros(n, np.uint32)
        check(lib.sk_resampler_process_f32(self._h, _ptr(sids), n, _ptr(data), frames, _ptr(out), cap, _ptr(got)),
              "sk_resampler_process_f32", self._h)
        return [out[i, :, :got[i]].copy() for i in range(n)]

    def resampler_flush(self, sids, channels):
        sids = np.ascontiguousarray(sids, np.uint32)
        n = sids.size
        cap = int(4096 * self._rs_ratio_max + 64)
        out = np.zeros((n, channels, cap), np.float32)
        got = np.zeros(n, np.uint32)
        check(lib.sk_resampler_flush_f32(self._h, _ptr(sids), n, _ptr(out), cap, _ptr(got)),
              "sk_resampler_flush_f32", self._h)
        return [out[i, :, :got[i]].copy() for i in range(n)]


    def tick_run(self, streams, descs, n_frames, coeffs):
        """One scheduler tick (sk_tick_run).  streams: list of dicts {stream, n_frames, out_bits, out_channels,
        resample, flush}; descs / coeffs as aac_synthesize.  -> list of (stream_index, status, frames, channels,
        bits, bytes) in the order the reference's worker would have sent them."""
        import ctypes as C
        from ._lib import TickStream, TickOutput
        ts = (TickStream * max(len(streams), 1))()
        for i, s in enumerate(streams):
            ts[i].stream, ts[i].n_frames = int(s["stream"]), int(s["n_frames"])
            ts[i].out_bits, ts[i].out_channels = int(s.get("out_bits", 16)), int(s["out_channels"])
            ts[i].resample, ts[i].flush = int(bool(s.get("resample", 0))), int(bool(s.get("flush", 0)))
        max_out = C.c_uint32()
        cap = lib.sk_tick_out_bound_on(self._h, ts, len(streams), C.byref(max_out))
        out = np.zeros(max(cap, 16), np.uint8)
        recs = (TickOutput * max(max_out.value, 1))()
        n_out, used = C.c_uint32(), C.c_size_t()
        coeffs = np.ascontiguousarray(coeffs, np.float32)
        check(lib.sk_tick_run(self._h, ts, len(streams), descs, _ptr(coeffs) if n_frames else None, n_frames, _ptr(out),
                              out.size, recs, max_out.value, C.byref(n_out), C.byref(used)), "sk_tick_run", self._h)
        res = []
        for r in recs[:n_out.value]:
            res.append((r.stream_index, r.status, r.frames, r.channels, r.bits,
                        out[r.byte_offset:r.byte_offset + r.bytes].tobytes()))
        return res


    def tick_run_q(self, streams, descs, n_units, sides, quant):
        """sk_tick_run_q: as tick_run, fed by AacLcFrontEnd.parse_q -- sides [n_units][SK_AAC_UNIT_SIDE_BYTES] u8, quant the
        units' i16 values packed like tick_run's coeffs"""
        import ctypes as C
        from ._lib import TickStream, TickOutput
        ts = (TickStream * max(len(streams), 1))()
        for i, s in enumerate(streams):
            ts[i].stream, ts[i].n_frames = int(s["stream"]), int(s["n_frames"])
            ts[i].out_bits, ts[i].out_channels = int(s.get("out_bits", 16)), int(s["out_channels"])
            ts[i].resample, ts[i].flush = int(bool(s.get("resample", 0))), int(bool(s.get("flush", 0)))
        max_out = C.c_uint32()
        cap = lib.sk_tick_out_bound_on(self._h, ts, len(streams), C.byref(max_out))
        out = np.zeros(max(cap, 16), np.uint8)
        recs = (TickOutput * max(max_out.value, 1))()
        n_out, used = C.c_uint32(), C.c_size_t()
        sides = np.ascontiguousarray(sides, np.uint8)
        quant = np.ascontiguousarray(quant, np.int16)
        check(lib.sk_tick_run_q(self._h, ts, len(streams), descs, _ptr(sides) if n_units else None, _ptr(quant) if n_units else None,
                                n_units, _ptr(out), out.size, recs, max_out.value, C.byref(n_out), C.byref(used)), "sk_tick_run_q", self._h)
        return [(r.stream_index, r.status, r.frames, r.channels, r.bits, out[r.byte_offset:r.byte_offset + r.bytes].tobytes())
                for r in recs[:n_out.value]]

    def tick_run_pcm(self, streams, units):
        """One tick of WAV / raw PCM streams (sk_tick_run_pcm).  streams: list of dicts {format (FMT_*), channels, out_bits,
        out_channels, n_units, and for a rate change: stream, resample, flush}; units: the pieces (bytes) of all streams, stream by
        stream in the order of `streams`.  Each is packed at a 16-byte aligned offset of one buffer, as the scheduler does it.
        -> list of (stream_index, status, frames, channels, bits, bytes, is_float)."""
        import ctypes as C
        from ._lib import PcmTickStream, PcmUnit, TickOutput
        ts = (PcmTickStream * max(len(streams), 1))()
        for i, s in enumerate(streams):
            ts[i].stream, ts[i].n_units = int(s.get("stream", 0)), int(s["n_units"])
            ts[i].format, ts[i].channels = int(s["format"]), int(s["channels"])
            ts[i].out_bits, ts[i].out_channels = int(s["out_bits"]), int(s["out_channels"])
            ts[i].resample, ts[i].flush = int(bool(s.get("resample", 0))), int(bool(s.get("flush", 0)))
        n = len(units)
        table = (PcmUnit * max(n, 1))()
        total = 0
        for k, u in enumerate(units):
            table[k].byte_offset, table[k].byte_len = total, len(u)
            total += (len(u) + 15) & ~15
        blob = np.zeros(max(total, 16), np.uint8)
        for k, u in enumerate(units):
            blob[table[k].byte_offset:table[k].byte_offset + len(u)] = np.frombuffer(bytes(u), np.uint8)
        max_out = C.c_uint32()
        cap = lib.sk_tick_pcm_out_bound_on(self._h, ts, len(streams), table, n, C.byref(max_out))
        out = np.zeros(max(cap, 16), np.uint8)
        recs = (TickOutput * max(max_out.value, 1))()
        n_out, used = C.c_uint32(), C.c_size_t()
        check(lib.sk_tick_run_pcm(self._h, ts, len(streams), table, n, _ptr(blob), total, _ptr(out), out.size, recs, max_out.value,
                                  C.byref(n_out), C.byref(used)), "sk_tick_run_pcm", self._h)
        return [(r.stream_index, r.status, r.frames, r.channels, r.bits, out[r.byte_offset:r.byte_offset + r.bytes].tobytes(), bool(r.reserved & 1))
                for r in recs[:n_out.value]]

    def aiff_decode(self, encoding, channels, data, ima_state=None):
        """sk_aiff_decode: whole sample groups of an AIFF / AIFF-C stream in the file's encoding (AIFF_*) -> the little-endian PCM
        of the output contract, as bytes.  IMA4: ima_state = [(predictor, step_index)] * 2 carried in (None: a fresh stream); the
        return is then (bytes, state)."""
        import ctypes as C
        from ._lib import AiffImaState
        data = np.frombuffer(bytes(data), np.uint8)
        group = 34 * channels if encoding == AIFF_IMA4 else AIFF_GROUP_BYTES.get(encoding, 1)  # (an unknown encoding is the library's to refuse)
        per_group = 128 * channels if encoding == AIFF_IMA4 else 12 if encoding == AIFF_DVD_S24 else (3 if encoding == AIFF_S24BE else (4 if AIFF_S32BE <= encoding <= AIFF_F64BE or encoding == AIFF_F64LE else 2))
        out = np.zeros(max(data.size // max(group, 1) * per_group, 16), np.uint8)
        st = (AiffImaState * 2)()
        for c, (p, i) in enumerate(ima_state or []):
            st[c].predictor, st[c].step_index = int(p), int(i)
        n = C.c_size_t()
        check(lib.sk_aiff_decode(self._h, int(encoding), int(channels), _ptr(data) if data.size else None, data.size, _ptr(out), out.size,
                                 C.byref(n), st), "sk_aiff_decode", self._h)
        got = out[:n.value].tobytes()
        if encoding == AIFF_IMA4:
            return got, [(st[c].predictor, st[c].step_index) for c in range(2)]
        return got

    def wav_adpcm_decode(self, tag, channels, block_align, data, coef=None):
        """sk_wav_adpcm_decode: whole blocks of a WAV stream of tag WAV_TAG_IMA_ADPCM / WAV_TAG_MS_ADPCM -> (interleaved little-endian
        s16 as bytes, frames_per_block x channels samples a block; [status per block]: 0, or WAV_BAD_BLOCK for a block its header
        rules out, whose samples are zeros).  coef: the fmt chunk's [(iCoef1, iCoef2)] (Microsoft ADPCM only)."""
        data = np.frombuffer(bytes(data), np.uint8)
        block_align, channels = int(block_align), int(channels)
        table = np.asarray(coef if coef is not None else [], np.int16).reshape(-1, 2)
        n_blocks = data.size // block_align if block_align > 0 else 0
        per_block = 2 * channels * wav_adpcm_block_frames(int(tag), channels, block_align)  # 0: the library refuses that geometry
        out = np.zeros(max(n_blocks * per_block, 16), np.uint8)
        status = np.zeros(max(n_blocks, 1), np.int32)
        n = C.c_size_t()
        check(lib.sk_wav_adpcm_decode(self._h, int(tag), channels, block_align, _ptr(table) if table.size else None, table.shape[0],
                                      _ptr(data) if data.size else None, data.size, _ptr(out), n_blocks * per_block, C.byref(n), _ptr(status)),
              "sk_wav_adpcm_decode", self._h)
        return out[:n.value].tobytes(), status[:n_blocks].tolist()

    def flac_decode(self, frames):
        """sk_flac_decode_frames: [(frame dict, frame bytes)] as flac.FlacReader.add / flac.scan cut them -> (the contract's interleaved
        little-endian PCM as bytes, [status per frame])"""
        from . import flac
        return flac.decode_frames(frames, engine=self)

    def vorbis_decode_packets(self, groups, as_f32=False):
        """sk_vorbis_decode_packets: [(vorbis.StreamState, [audio packet bytes])], every stream's packets in one launch sequence; the
        states are updated.  -> [per stream: [per packet: (status, samples as [frames][channels], s16 or -- as_f32 -- the f32 before
        narrowing)]]"""
        from . import vorbis
        return vorbis.decode_packets(groups, as_f32=as_f32, engine=self)

    def vorbis_entropy_decode(self, groups):
        """sk_vorbis_entropy_decode: [(vorbis.Setup, [audio packet bytes])] -> per stream, per packet a dict of what the entropy stage
        left: status, mode, window flags, per channel used / final_y / step2, and the residue vectors"""
        from . import vorbis
        return vorbis.entropy_decode(groups, engine=self)

    def tick_run_vorbis(self, streams, packets, out_cap=None, skip_frames=None, keep_frames=None):
        """One tick of Vorbis streams (sk_tick_run_vorbis).  streams: list of dicts {state (a vorbis.StreamState: the carry, updated when
        the tick succeeded), out_bits, out_channels, n_units, and for a rate change: stream, resample, flush}; packets: [audio packet
        bytes] of all streams, stream by stream.  out_cap: an output size other than the bound's (to have a tick refused).
        skip_frames / keep_frames: per packet, the frames dropped at its front and how many of the rest stay at most (None: 0 / all).
        -> (the same list of records as tick_run_pcm, [status per packet])."""
        import ctypes as C
        from . import vorbis
        from ._lib import TickOutput, VorbisTickPacket, VorbisTickStream
        ts = (VorbisTickStream * max(len(streams), 1))()
        for i, s in enumerate(streams):
            st = s["state"]
            ts[i].setup, ts[i].overlap, ts[i].prev_blocksize = st.setup._h, st.overlap.ctypes.data, st.prev_blocksize
            ts[i].stream, ts[i].n_units = int(s.get("stream", 0)), int(s["n_units"])
            ts[i].out_bits, ts[i].out_channels = int(s["out_bits"]), int(s["out_channels"])
            ts[i].resample, ts[i].flush = int(bool(s.get("resample", 0))), int(bool(s.get("flush", 0)))
        n = len(packets)
        table, blob = (VorbisTickPacket * max(n, 1))(), bytearray()
        for k, p in enumerate(packets):
            blob += bytes(-len(blob) % 16)
            table[k].offset, table[k].size = len(blob), len(p)
            table[k].keep_frames = 0xffffffff if keep_frames is None else int(keep_frames[k])
            table[k].skip_frames = 0 if skip_frames is None else int(skip_frames[k])
            blob += p
        src = np.frombuffer(bytes(blob) + bytes(16), np.uint8)
        max_out = C.c_uint32()
        cap = lib.sk_tick_vorbis_out_bound_on(self._h, ts, len(streams), table, n, _ptr(src), len(blob), C.byref(max_out))
        out = np.zeros(max(cap if out_cap is None else out_cap, 16), np.uint8)
        recs = (TickOutput * max(max_out.value, 1))()
        status = np.zeros(max(n, 1), np.int32)
        n_out, used = C.c_uint32(), C.c_size_t()
        check(lib.sk_tick_run_vorbis(self._h, ts, len(streams), table, n, _ptr(src), len(blob), _ptr(out), out.size if out_cap is None else out_cap, recs,
                                     max_out.value, C.byref(n_out), C.byref(used), _ptr(status)), "sk_tick_run_vorbis", self._h)
        for i, s in enumerate(streams):
            s["state"].prev_blocksize = int(ts[i].prev_blocksize)
        return ([(r.stream_index, r.status, r.frames, r.channels, r.bits, out[r.byte_offset:r.byte_offset + r.bytes].tobytes(), bool(r.reserved & 1))
                 for r in recs[:n_out.value]], status[:n].tolist())

    def tick_run_flac(self, streams, frames):
        """One tick of FLAC streams (sk_tick_run_flac).  streams: list of dicts {channels, bits_per_sample, out_bits, out_channels, n_units,
        and for a rate change: stream, resample, flush}; frames: [(frame dict, frame bytes)] of all streams, stream by stream, each
        packed at a 16-byte aligned offset.  -> (the same list of records as tick_run_pcm, [status per frame])."""
        import ctypes as C
        from . import flac
        from ._lib import FlacTickStream, TickOutput
        ts = (FlacTickStream * max(len(streams), 1))()
        for i, s in enumerate(streams):
            ts[i].stream, ts[i].n_units = int(s.get("stream", 0)), int(s["n_units"])
            ts[i].channels, ts[i].bits_per_sample = int(s["channels"]), int(s["bits_per_sample"])
            ts[i].out_bits, ts[i].out_channels = int(s["out_bits"]), int(s["out_channels"])
            ts[i].resample, ts[i].flush = int(bool(s.get("resample", 0))), int(bool(s.get("flush", 0)))
        table, blob = flac.pack_frames(frames)
        n = len(frames)
        src = np.frombuffer(blob + bytes(16), np.uint8)
        max_out = C.c_uint32()
        cap = lib.sk_tick_flac_out_bound_on(self._h, ts, len(streams), table, n, C.byref(max_out))
        out = np.zeros(max(cap, 16), np.uint8)
        recs = (TickOutput * max(max_out.value, 1))()
        status = np.zeros(max(n, 1), np.int32)
        n_out, used = C.c_uint32(), C.c_size_t()
        check(lib.sk_tick_run_flac(self._h, ts, len(streams), table, n, _ptr(src), len(blob), _ptr(out), out.size, recs, max_out.value,
                                   C.byref(n_out), C.byref(used), _ptr(status)), "sk_tick_run_flac", self._h)
        return ([(r.stream_index, r.status, r.frames, r.channels, r.bits, out[r.byte_offset:r.byte_offset + r.bytes].tobytes(), bool(r.reserved & 1))
                 for r in recs[:n_out.value]], status[:n].tolist())

    def tick_run_alac(self, streams, packets):
        """One tick of ALAC streams (sk_tick_run_alac).  streams: list of dicts {config (the cookie as alac.parse_cookie gives it), out_bits,
        out_channels, n_units, and for a rate change: stream, resample, flush}; packets: [packet bytes] of all streams, stream by stream,
        each packed at a 16-byte aligned offset; their frame counts are read with sk_alac_packet_frames, as the scheduler does it.
        -> (the same list of records as tick_run_pcm, [status per packet])."""
        import ctypes as C
        from . import alac
        from ._lib import AlacTickPacket, AlacTickStream, TickOutput
        ts = (AlacTickStream * max(len(streams), 1))()
        counts, at = [], 0
        for i, s in enumerate(streams):
            ts[i].stream, ts[i].n_units = int(s.get("stream", 0)), int(s["n_units"])
            for name in ("frame_length", "channels", "bit_depth", "pb", "mb", "kb"):
                setattr(ts[i], name, int(s["config"][name]))
            ts[i].out_bits, ts[i].out_channels = int(s["out_bits"]), int(s["out_channels"])
            ts[i].resample, ts[i].flush = int(bool(s.get("resample", 0))), int(bool(s.get("flush", 0)))
            counts += [alac.packet_frames(s["config"], p)[1] for p in packets[at:at + int(s["n_units"])]]
            at += int(s["n_units"])
        counts += [0] * (len(packets) - len(counts))
        placed, blob = alac.pack_packets(packets)
        n = len(packets)
        table = (AlacTickPacket * max(n, 1))()
        for k in range(n):
            table[k].offset, table[k].size, table[k].frames = placed[k].offset, placed[k].size, counts[k]
        src = np.frombuffer(blob + bytes(16), np.uint8)
        max_out = C.c_uint32()
        cap = lib.sk_tick_alac_out_bound_on(self._h, ts, len(streams), table, n, C.byref(max_out))
        out = np.zeros(max(cap, 16), np.uint8)
        recs = (TickOutput * max(max_out.value, 1))()
        status = np.zeros(max(n, 1), np.int32)
        n_out, used = C.c_uint32(), C.c_size_t()
        check(lib.sk_tick_run_alac(self._h, ts, len(streams), table, n, _ptr(src), len(blob), _ptr(out), out.size, recs, max_out.value,
                                   C.byref(n_out), C.byref(used), _ptr(status)), "sk_tick_run_alac", self._h)
        return ([(r.stream_index, r.status, r.frames, r.channels, r.bits, out[r.byte_offset:r.byte_offset + r.bytes].tobytes(), bool(r.reserved & 1))
                 for r in recs[:n_out.value]], status[:n].tolist())

    def g72x_decode(self, codec, data, state=None, rate=32000, packing=0):
        """sk_g72x_decode: one telephony stream's bytes (telephony.ULAW / ALAW / G722 / G726; G.726 in whole groups) -> s16le bytes.
        state: a telephony.new_state(codec) record carried from call to call and updated in place (None: a fresh stream)."""
        import ctypes as C
        from . import telephony
        data = np.frombuffer(bytes(data), np.uint8)
        st = state if state is not None else telephony.new_state(codec)
        out = np.zeros(max(telephony.decoded_samples(codec, data.size, rate) * 2, 16), np.uint8)
        n = C.c_size_t()
        text = C.create_string_buffer(256)
        rc = lib.sk_g72x_decode(self._h, int(codec), int(rate), int(packing), _ptr(data) if data.size else None, data.size, _ptr(out), out.size, C.byref(n),
                                C.byref(st) if st is not None else None, text, 256)
        if rc == telephony.ERR_STREAM:
            raise telephony.TelephonyError(text.value.decode())
        check(rc, "sk_g72x_decode", self._h)
        return out[:n.value].tobytes()

    def g72x_decode_batch(self, streams, units):
        """sk_g72x_decode_batch.  streams: list of dicts {codec, n_units, and for G.726: rate, packing; for G.722 / G.726: state (a
        telephony.new_state record, updated in place)}; units: the pieces (bytes) of all streams, stream by stream, each packed at a
        16-byte aligned offset.  -> [s16le bytes per unit]."""
        import ctypes as C
        from . import telephony
        from ._lib import G722State, G726State, G72xStream, G72xUnit
        ts = (G72xStream * max(len(streams), 1))()
        of726, of722 = [], []
        for i, s in enumerate(streams):
            ts[i].codec, ts[i].n_units = int(s["codec"]), int(s["n_units"])
            ts[i].g726_rate, ts[i].g726_packing = int(s.get("rate", 32000)), int(s.get("packing", 0))
            if ts[i].codec == telephony.G726:
                ts[i].state = len(of726)
                of726.append(s)
            elif ts[i].codec == telephony.G722:
                ts[i].state = len(of722)
                of722.append(s)
        s726, s722 = (G726State * max(len(of726), 1))(), (G722State * max(len(of722), 1))()
        for k, s in enumerate(of726):
            s726[k] = s["state"]
        for k, s in enumerate(of722):
            s722[k] = s["state"]
        n = len(units)
        table = (G72xUnit * max(n, 1))()
        total, need = 0, 0
        for k, u in enumerate(units):
            table[k].offset, table[k].size = total, len(u)
            total += (len(u) + 15) & ~15
            need += (len(u) * 16 + 15) & ~15  # no codec gives more than 8 samples a byte
        blob = np.zeros(max(total, 16), np.uint8)
        for k, u in enumerate(units):
            blob[table[k].offset:table[k].offset + len(u)] = np.frombuffer(bytes(u), np.uint8)
        out = np.zeros(max(need, 16), np.uint8)
        used = C.c_size_t()
        check(lib.sk_g72x_decode_batch(self._h, ts, len(streams), table, n, _ptr(blob), total, _ptr(out), out.size, C.byref(used), s726, len(of726),
                                       s722, len(of722)), "sk_g72x_decode_batch", self._h)
        for k, s in enumerate(of726):
            C.memmove(C.byref(s["state"]), C.byref(s726[k]), C.sizeof(G726State))
        for k, s in enumerate(of722):
            C.memmove(C.byref(s["state"]), C.byref(s722[k]), C.sizeof(G722State))
        return [out[table[k].out_offset:table[k].out_offset + table[k].out_len].tobytes() for k in range(n)]

    def tick_run_g72x(self, streams, units):
        """One tick of telephony streams (sk_tick_run_g72x).  As tick_run_pcm, with `codec` (telephony.ULAW / ALAW / G722 / G726) in
        the place of `format`, `rate` and `packing` for G.726, `channels` for G.711 (1 when absent) and "state": a telephony.new_state
        record for G.722 / G.726, which is updated in place.  -> the same list of records."""
        import ctypes as C
        from . import telephony
        from ._lib import G722State, G726State, G72xTickStream, PcmUnit, TickOutput
        ts = (G72xTickStream * max(len(streams), 1))()
        of726, of722 = [], []
        for i, s in enumerate(streams):
            ts[i].stream, ts[i].n_units = int(s.get("stream", 0)), int(s["n_units"])
            ts[i].codec, ts[i].channels = int(s["codec"]), int(s.get("channels", 1))
            ts[i].g726_rate, ts[i].g726_packing = int(s.get("rate", 32000)), int(s.get("packing", 0))
            ts[i].out_bits, ts[i].out_channels = int(s["out_bits"]), int(s["out_channels"])
            ts[i].resample, ts[i].flush = int(bool(s.get("resample", 0))), int(bool(s.get("flush", 0)))
            if ts[i].codec == telephony.G726:
                ts[i].state = len(of726)
                of726.append(s)
            elif ts[i].codec == telephony.G722:
                ts[i].state = len(of722)
                of722.append(s)
        s726, s722 = (G726State * max(len(of726), 1))(), (G722State * max(len(of722), 1))()
        for k, s in enumerate(of726):
            s726[k] = s["state"]
        for k, s in enumerate(of722):
            s722[k] = s["state"]
        n = len(units)
        table = (PcmUnit * max(n, 1))()
        total = 0
        for k, u in enumerate(units):
            table[k].byte_offset, table[k].byte_len = total, len(u)
            total += (len(u) + 15) & ~15
        blob = np.zeros(max(total, 16), np.uint8)
        for k, u in enumerate(units):
            blob[table[k].byte_offset:table[k].byte_offset + len(u)] = np.frombuffer(bytes(u), np.uint8)
        max_out = C.c_uint32()
        cap = lib.sk_tick_g72x_out_bound_on(self._h, ts, len(streams), table, n, C.byref(max_out))
        out = np.zeros(max(cap, 16), np.uint8)
        recs = (TickOutput * max(max_out.value, 1))()
        n_out, used = C.c_uint32(), C.c_size_t()
        check(lib.sk_tick_run_g72x(self._h, ts, len(streams), table, n, _ptr(blob), total, _ptr(out), out.size, recs, max_out.value,
                                   C.byref(n_out), C.byref(used), s726, len(of726), s722, len(of722)), "sk_tick_run_g72x", self._h)
        for k, s in enumerate(of726):
            C.memmove(C.byref(s["state"]), C.byref(s726[k]), C.sizeof(G726State))
        for k, s in enumerate(of722):
            C.memmove(C.byref(s["state"]), C.byref(s722[k]), C.sizeof(G722State))
        return [(r.stream_index, r.status, r.frames, r.channels, r.bits, out[r.byte_offset:r.byte_offset + r.bytes].tobytes(), bool(r.reserved & 1))
                for r in recs[:n_out.value]]

    def gsm_decode(self, data, state=None, variant=0):
        """sk_gsm_decode: one GSM stream's whole packets (telephony.GSM_STANDARD / GSM_MICROSOFT) -> s16le bytes.  state: a
        telephony.new_state(telephony.GSM) record carried from call to call and updated in place (None: a fresh stream)."""
        import ctypes as C
        from . import telephony
        data = np.frombuffer(bytes(data), np.uint8)
        st = state if state is not None else telephony.new_state(telephony.GSM)
        out = np.zeros(max(telephony.gsm_decoded_samples(variant, data.size) * 2, 16), np.uint8)
        n = C.c_size_t()
        text = C.create_string_buffer(256)
        rc = lib.sk_gsm_decode(self._h, int(variant), _ptr(data) if data.size else None, data.size, _ptr(out), out.size, C.byref(n), C.byref(st), text, 256)
        if rc == telephony.ERR_STREAM:
            raise telephony.TelephonyError(text.value.decode())
        check(rc, "sk_gsm_decode", self._h)
        return out[:n.value].tobytes()

    @staticmethod
    def _gsm_tables(streams, units, row_type, unit_type, offset_field, size_field):
        """the stream rows, the state records and the unit table with every unit packed at a 16-byte aligned offset of one blob"""
        from ._lib import GsmState
        ts = (row_type * max(len(streams), 1))()
        states = (GsmState * max(len(streams), 1))()
        for i, s in enumerate(streams):
            ts[i].variant, ts[i].n_units, ts[i].state = int(s.get("variant", 0)), int(s["n_units"]), i
            states[i] = s["state"]
        table = (unit_type * max(len(units), 1))()
        total = 0
        for k, u in enumerate(units):
            setattr(table[k], offset_field, total)
            setattr(table[k], size_field, len(u))
            total += (len(u) + 15) & ~15
        blob = np.zeros(max(total, 16), np.uint8)
        at = 0
        for u in units:
            blob[at:at + len(u)] = np.frombuffer(bytes(u), np.uint8)
            at += (len(u) + 15) & ~15
        return ts, states, table, blob, total

    def gsm_decode_batch(self, streams, units):
        """sk_gsm_decode_batch.  streams: list of dicts {n_units, variant (0 when absent), state (a telephony.new_state(telephony.GSM)
        record, updated in place)}; units: the pieces (bytes, whole packets) of all streams, stream by stream.  -> [s16le bytes per unit]."""
        import ctypes as C
        from . import telephony
        from ._lib import GsmState, GsmStream, G72xUnit
        ts, states, table, blob, total = self._gsm_tables(streams, units, GsmStream, G72xUnit, "offset", "size")
        need = sum((len(u) * 10 + 15) & ~15 for u in units)  # 320 bytes out of 33, 640 out of 65
        out = np.zeros(max(need, 16), np.uint8)
        used = C.c_size_t()
        rc = lib.sk_gsm_decode_batch(self._h, ts, len(streams), table, len(units), _ptr(blob), total, _ptr(out), out.size, C.byref(used), states, len(streams))
        if rc == telephony.ERR_STREAM:
            raise telephony.TelephonyError("GSM decoder rejected frame")
        check(rc, "sk_gsm_decode_batch", self._h)
        for i, s in enumerate(streams):
            C.memmove(C.byref(s["state"]), C.byref(states[i]), C.sizeof(GsmState))
        return [out[table[k].out_offset:table[k].out_offset + table[k].out_len].tobytes() for k in range(len(units))]

    def tick_run_gsm(self, streams, units):
        """One tick of GSM streams (sk_tick_run_gsm).  As tick_run_pcm, with `variant` in the place of `format` and "state": a
        telephony.new_state(telephony.GSM) record, which is updated in place.  -> the same list of records."""
        import ctypes as C
        from ._lib import GsmState, GsmTickStream, PcmUnit, TickOutput
        ts, states, table, blob, total = self._gsm_tables(streams, units, GsmTickStream, PcmUnit, "byte_offset", "byte_len")
        for i, s in enumerate(streams):
            ts[i].stream, ts[i].channels = int(s.get("stream", 0)), 1
            ts[i].out_bits, ts[i].out_channels = int(s["out_bits"]), int(s["out_channels"])
            ts[i].resample, ts[i].flush = int(bool(s.get("resample", 0))), int(bool(s.get("flush", 0)))
        max_out = C.c_uint32()
        cap = lib.sk_tick_gsm_out_bound_on(self._h, ts, len(streams), table, len(units), C.byref(max_out))
        out = np.zeros(max(cap, 16), np.uint8)
        recs = (TickOutput * max(max_out.value, 1))()
        n_out, used = C.c_uint32(), C.c_size_t()
        check(lib.sk_tick_run_gsm(self._h, ts, len(streams), table, len(units), _ptr(blob), total, _ptr(out), out.size, recs, max_out.value,
                                  C.byref(n_out), C.byref(used), states, len(streams)), "sk_tick_run_gsm", self._h)
        for i, s in enumerate(streams):
            C.memmove(C.byref(s["state"]), C.byref(states[i]), C.sizeof(GsmState))
        return [(r.stream_index, r.status, r.frames, r.channels, r.bits, out[r.byte_offset:r.byte_offset + r.bytes].tobytes(), bool(r.reserved & 1))
                for r in recs[:n_out.value]]

    def tick_run_aiff(self, streams, units):
        """One tick of AIFF streams (sk_tick_run_aiff).  As tick_run_pcm, with `encoding` (AIFF_*) in the place of `format` and, for
        IMA4, "ima_state": [(predictor, step_index)] * 2, which is updated in the dict.  -> the same list of records."""
        import ctypes as C
        from ._lib import AiffTickStream, PcmUnit, TickOutput
        ts = (AiffTickStream * max(len(streams), 1))()
        for i, s in enumerate(streams):
            ts[i].stream, ts[i].n_units = int(s.get("stream", 0)), int(s["n_units"])
            ts[i].encoding, ts[i].channels = int(s["encoding"]), int(s["channels"])
            ts[i].out_bits, ts[i].out_channels = int(s["out_bits"]), int(s["out_channels"])
            ts[i].resample, ts[i].flush = int(bool(s.get("resample", 0))), int(bool(s.get("flush", 0)))
            for c, (p, x) in enumerate(s.get("ima_state") or []):
                ts[i].ima_state[c].predictor, ts[i].ima_state[c].step_index = int(p), int(x)
        n = len(units)
        table = (PcmUnit * max(n, 1))()
        total = 0
        for k, u in enumerate(units):
            table[k].byte_offset, table[k].byte_len = total, len(u)
            total += (len(u) + 15) & ~15
        blob = np.zeros(max(total, 16), np.uint8)
        for k, u in enumerate(units):
            blob[table[k].byte_offset:table[k].byte_offset + len(u)] = np.frombuffer(bytes(u), np.uint8)
        max_out = C.c_uint32()
        cap = lib.sk_tick_aiff_out_bound_on(self._h, ts, len(streams), table, n, C.byref(max_out))
        out = np.zeros(max(cap, 16), np.uint8)
        recs = (TickOutput * max(max_out.value, 1))()
        n_out, used = C.c_uint32(), C.c_size_t()
        check(lib.sk_tick_run_aiff(self._h, ts, len(streams), table, n, _ptr(blob), total, _ptr(out), out.size, recs, max_out.value,
                                   C.byref(n_out), C.byref(used)), "sk_tick_run_aiff", self._h)
        for i, s in enumerate(streams):
            if int(s["encoding"]) == AIFF_IMA4:
                s["ima_state"] = [(ts[i].ima_state[c].predictor, ts[i].ima_state[c].step_index) for c in range(2)]
        return [(r.stream_index, r.status, r.frames, r.channels, r.bits, out[r.byte_offset:r.byte_offset + r.bytes].tobytes(), bool(r.reserved & 1))
                for r in recs[:n_out.value]]

    def _wav_adpcm_tick_tables(self, streams, units):
        from ._lib import PcmUnit, WavAdpcmTickStream
        ts = (WavAdpcmTickStream * max(len(streams), 1))()
        for i, s in enumerate(streams):
            ts[i].stream, ts[i].n_units = int(s.get("stream", 0)), int(s["n_units"])
            ts[i].tag, ts[i].channels, ts[i].block_align = int(s["tag"]), int(s["channels"]), int(s["block_align"])
            ts[i].out_bits, ts[i].out_channels = int(s["out_bits"]), int(s["out_channels"])
            ts[i].resample, ts[i].flush = int(bool(s.get("resample", 0))), int(bool(s.get("flush", 0)))
            ts[i].frames_left = WAV_NO_FRAME_CAP if s.get("frames_left") is None else int(s["frames_left"])
            coef = s.get("coef") or []
            ts[i].n_coef = len(coef)
            for k, (a, b) in enumerate(coef):
                ts[i].coef[k][0], ts[i].coef[k][1] = int(a), int(b)
        table = (PcmUnit * max(len(units), 1))()
        total = 0
        for k, u in enumerate(units):
            table[k].byte_offset, table[k].byte_len = total, len(u)
            total += (len(u) + 15) & ~15
        blob = np.zeros(max(total, 16), np.uint8)
        for k, u in enumerate(units):
            blob[table[k].byte_offset:table[k].byte_offset + len(u)] = np.frombuffer(bytes(u), np.uint8)
        return ts, table, blob, total

    def tick_wav_adpcm_out_bound(self, streams, units):
        """sk_tick_wav_adpcm_out_bound_on for the tables tick_run_wav_adpcm would build -> (bytes, records)"""
        ts, table, _, _ = self._wav_adpcm_tick_tables(streams, units)
        max_out = C.c_uint32()
        return lib.sk_tick_wav_adpcm_out_bound_on(self._h, ts, len(streams), table, len(units), C.byref(max_out)), max_out.value

    def tick_run_wav_adpcm(self, streams, units, out_cap=None):
        """One tick of WAV ADPCM streams (sk_tick_run_wav_adpcm).  As tick_run_pcm, with the stream's description in the place of
        `format`: tag (WAV_TAG_IMA_ADPCM / WAV_TAG_MS_ADPCM), block_align, coef ([(iCoef1, iCoef2)], Microsoft ADPCM), and frames_left,
        the fact chunk's cap (None: no cap), which is updated in the dict when the tick succeeded.  units: whole blocks.  out_cap: an
        output size other than the bound's (to have a tick refused).  -> (the same list of records, [status per unit: 0, or 1 + the
        index of the unit's first bad block])."""
        from ._lib import TickOutput
        ts, table, blob, total = self._wav_adpcm_tick_tables(streams, units)
        n = len(units)
        max_out = C.c_uint32()
        cap = lib.sk_tick_wav_adpcm_out_bound_on(self._h, ts, len(streams), table, n, C.byref(max_out))
        out = np.zeros(max(cap, 16), np.uint8)
        recs = (TickOutput * max(max_out.value, 1))()
        status = np.zeros(max(n, 1), np.int32)
        n_out, used = C.c_uint32(), C.c_size_t()
        check(lib.sk_tick_run_wav_adpcm(self._h, ts, len(streams), table, n, _ptr(blob), total, _ptr(out), out.size if out_cap is None else out_cap, recs,
                                        max_out.value, C.byref(n_out), C.byref(used), _ptr(status)), "sk_tick_run_wav_adpcm", self._h)
        for i, s in enumerate(streams):
            s["frames_left"] = None if ts[i].frames_left == WAV_NO_FRAME_CAP else int(ts[i].frames_left)
        return ([(r.stream_index, r.status, r.frames, r.channels, r.bits, out[r.byte_offset:r.byte_offset + r.bytes].tobytes(), bool(r.reserved & 1))
                 for r in recs[:n_out.value]], status[:n].tolist())

    def tick_run_mpa(self, streams, frames=None):
        """One tick of MPEG Layer I / II streams alone (sk_tick_run_mixed_mpa with no AAC unit and no Layer III granule).  streams:
        list of dicts {stream, channels, out_bits, out_channels (the source's `channels` when absent), resample, flush, frames};
        a stream's frames are (MpaFrameRecord, frame bytes) pairs as mp3.mpa_parse_frame gives them.  They are packed as
        mp3.mpa_pack_frames packs them (4-byte aligned, at least 8 zero bytes behind each), stream by stream in the order of
        `streams`.  `frames`, when given, is that packing done by the caller -- (record array, n, uint8 buffer) -- and every
        stream's dict then says how many of its records are its own with n_frames; nothing is checked here, so a table that does
        not add up reaches the library, which refuses it.
        -> list of (stream_index, status, frames, channels, bits, bytes), as tick_run."""
        import ctypes as C
        from . import mp3
        from ._lib import SK_TICK_MPA, TickInput, TickMpaFrames, TickOutput, TickStream
        if frames is None:
            frames = mp3.mpa_pack_frames([f for s in streams for f in s["frames"]])
        recs, n, buf = frames
        ts = (TickStream * max(len(streams), 1))()
        for i, s in enumerate(streams):
            ts[i].stream, ts[i].n_frames = int(s["stream"]), int(s["n_frames"]) if "n_frames" in s else len(s["frames"])
            ts[i].out_bits, ts[i].out_channels = int(s.get("out_bits", 16)), int(s.get("out_channels") or s["channels"])
            ts[i].resample, ts[i].flush = int(bool(s.get("resample", 0))), int(bool(s.get("flush", 0)))
            ts[i].codec = SK_TICK_MPA
        buf = np.ascontiguousarray(buf, np.uint8)
        mpa = TickMpaFrames(C.cast(recs, C.c_void_p), n, _ptr(buf), buf.size if n else 0)
        tin = TickInput()
        max_out = C.c_uint32()
        cap = lib.sk_tick_out_bound_on(self._h, ts, len(streams), C.byref(max_out))
        out = np.zeros(max(cap, 16), np.uint8)
        outs = (TickOutput * max(max_out.value, 1))()
        n_out, used = C.c_uint32(), C.c_size_t()
        check(lib.sk_tick_run_mixed_mpa(self._h, ts, len(streams), C.byref(tin), None, C.byref(mpa), _ptr(out), out.size, outs, max_out.value,
                                        C.byref(n_out), C.byref(used)), "sk_tick_run_mixed_mpa", self._h)
        return [(r.stream_index, r.status, r.frames, r.channels, r.bits, out[r.byte_offset:r.byte_offset + r.bytes].tobytes())
                for r in outs[:n_out.value]]

    def tick_run_au(self, streams, access_units):
        """sk_tick_run_au: as tick_run, but the entropy front-end runs on the GPU.  access_units: the raw access
        units (bytes) of all streams, stream by stream in the order of `streams`."""
        import ctypes as C
        from ._lib import TickStream, TickOutput
        ts = (TickStream * max(len(streams), 1))()
        for i, s in enumerate(streams):
            ts[i].stream, ts[i].n_frames = int(s["stream"]), int(s["n_frames"])
            ts[i].out_bits, ts[i].out_channels = int(s.get("out_bits", 16)), int(s["out_channels"])
            ts[i].resample, ts[i].flush = int(bool(s.get("resample", 0))), int(bool(s.get("flush", 0)))
        n = len(access_units)
        items = np.zeros((max(n, 1), 2), np.uint32)
        blob = bytearray()
        for k, au in enumerate(access_units):
            items[k] = (len(blob), len(au))
            blob += bytes(au) + b"\0" * (8 + (-len(au)) % 4)   # >= 8 zero bytes, next unit 4-byte aligned
        blob = np.frombuffer(bytes(blob) + b"\0" * 8, np.uint8)
        max_out = C.c_uint32()
        cap = lib.sk_tick_out_bound_on(self._h, ts, len(streams), C.byref(max_out))
        out = np.zeros(max(cap, 16), np.uint8)
        recs = (TickOutput * max(max_out.value, 1))()
        n_out, used = C.c_uint32(), C.c_size_t()
        check(lib.sk_tick_run_au(self._h, ts, len(streams), _ptr(items), n, _ptr(blob), blob.size, _ptr(out), out.size, recs,
                                 max_out.value, C.byref(n_out), C.byref(used)), "sk_tick_run_au", self._h)
        return [(r.stream_index, r.status, r.frames, r.channels, r.bits, out[r.byte_offset:r.byte_offset + r.bytes].tobytes())
                for r in recs[:n_out.value]]


    def entropy_decode(self, streams, access_units):
        """sk_aac_entropy_decode: the AAC-LC front-end alone, on the GPU.  streams: [(stream id, unit count)];
        access_units: the raw units of all streams, stream by stream.  -> [(status, coeffs [ch][1024] f32,
        window_sequence[ch], window_shape[ch])] per unit."""
        import ctypes as C
        n = len(access_units)
        ids = np.array([s for s, _ in streams], np.uint32)
        counts = np.array([c for _, c in streams], np.uint32)
        assert int(counts.sum()) == n
        items = np.zeros((max(n, 1), 2), np.uint32)
        blob = bytearray()
        for k, au in enumerate(access_units):
            items[k] = (len(blob), len(au))
            blob += bytes(au) + b"\0" * (8 + (-len(au)) % 4)
        blob = np.frombuffer(bytes(blob) + b"\0" * 8, np.uint8)
        ch = np.repeat(np.array([self._channels[int(s)] for s in ids], np.uint32), counts) if n else np.zeros(0, np.uint32)
        coeffs = np.zeros(max(int(ch.sum()) * 1024, 1), np.float32)
        descs = (FrameDesc * max(n, 1))()
        status = np.zeros(max(n, 1), np.int32)
        check(lib.sk_aac_entropy_decode(self._h, _ptr(ids), _ptr(counts), len(streams), _ptr(items), n, _ptr(blob), blob.size,
                                        _ptr(coeffs), descs, _ptr(status)), "sk_aac_entropy_decode", self._h)
        out, off = [], 0
        for k in range(n):
            c = int(ch[k])
            out.append((int(status[k]), coeffs[off:off + c * 1024].reshape(c, 1024).copy(),
                        [int(descs[k].window_sequence[i]) for i in range(c)], [int(descs[k].window_shape[i]) for i in range(c)]))
            off += c * 1024
        return out


    def expand_q_decode(self, streams, parsed):
        """sk_aac_expand_q_decode: the device half of the quantised hand-over alone.  streams: [(stream id, unit count)];
        parsed: AacLcFrontEnd.parse_q's results (quant, side, sequences, shapes) of all units, stream by stream.
        -> [(status, coeffs [ch][1024] f32, window_sequence[ch], window_shape[ch])] per unit."""
        from ._lib import AAC_UNIT_SIDE_BYTES
        n = len(parsed)
        ids = np.array([s for s, _ in streams], np.uint32)
        counts = np.array([c for _, c in streams], np.uint32)
        assert int(counts.sum()) == n
        ch = np.repeat(np.array([self._channels[int(s)] for s in ids], np.uint32), counts) if n else np.zeros(0, np.uint32)
        owner = np.repeat(ids, counts) if n else np.zeros(0, np.uint32)
        descs_in = (FrameDesc * max(n, 1))()
        for k, (q, side, seqs, shapes) in enumerate(parsed):
            descs_in[k].stream, descs_in[k].channels = int(owner[k]), int(ch[k])
            for c in range(int(ch[k])):
                descs_in[k].window_sequence[c], descs_in[k].window_shape[c] = int(seqs[c]), int(shapes[c])
        sides = np.ascontiguousarray(np.stack([p[1] for p in parsed]) if n else np.zeros((1, AAC_UNIT_SIDE_BYTES)), np.uint8)
        quant = np.ascontiguousarray(np.concatenate([p[0].ravel() for p in parsed]) if n else np.zeros(1), np.int16)
        coeffs = np.zeros(max(int(ch.sum()) * 1024, 1), np.float32)
        descs = (FrameDesc * max(n, 1))()
        status = np.zeros(max(n, 1), np.int32)
        check(lib.sk_aac_expand_q_decode(self._h, _ptr(ids), _ptr(counts), len(streams), descs_in, _ptr(sides), _ptr(quant), n,
                                         _ptr(coeffs), descs, _ptr(status)), "sk_aac_expand_q_decode", self._h)
        out, off = [], 0
        for k in range(n):
            c = int(ch[k])
            out.append((int(status[k]), coeffs[off:off + c * 1024].reshape(c, 1024).copy(),
                        [int(descs[k].window_sequence[i]) for i in range(c)], [int(descs[k].window_shape[i]) for i in range(c)]))
            off += c * 1024
        return out

    def where(self):
        """sk_engine_where: the stage of the engine's current tick ("idle" outside one)"""
        return lib.sk_engine_where(self._h).decode()

    def set_resampler_exact(self, exact=True):
        """generic-ratio resampling in rubato's own order of operations (bit-identical to the restated reference) instead of
        the matrix-core form"""
        check(lib.sk_engine_set_resampler_exact(self._h, 1 if exact else 0), "sk_engine_set_resampler_exact", self._h)

    def set_wait_bound(self, seconds):
        check(lib.sk_engine_set_wait_bound(self._h, float(seconds)), "sk_engine_set_wait_bound")

    def debug_fail_after(self, n_hip_calls):
        """error-path tests: the n-th HIP call from now fails as a launch failure"""
        check(lib.sk_engine_debug_fail_after(self._h, int(n_hip_calls)), "sk_engine_debug_fail_after")


_default = None


def default_engine():
    """Process-wide engine on HIP device 0 (LOCAL_RANK if set), created on first use."""
    global _default
    if _default is None:
        import os
        _default = Engine(int(os.environ.get("LOCAL_RANK", "0")), 8192)
    return _default

"""Host-side mirror of soundkit-decoder's streaming pipeline handle (soundkit-decoder/src/lib.rs:2590-2889) on
top of the batch scheduler (csrc/pipeline.cpp): `DecodePipeline.spawn_with_options(..)` returns a handle with
`send / finish / try_recv / recv / cancel / queued_input_bytes`, but instead of one worker thread per stream every
handle feeds one shared scheduler per GPU (entropy decode on host threads, everything after it batched on the GPU).

Input: ADTS AAC-LC and MPEG Layer III (the stream's first bytes choose), WAV / RF64 (`RIFF....WAVE`: the walker of
soundkit/src/wav.rs, then the reference's output stage -- sample width, mono downmix, rate -- in one batched GPU tick for all such
streams; a stream with nothing to change is passed through as it is, any width and channel count), and headerless PCM through
`spawn_raw_pcm[_with_options](RawPcmFormat)`, and AIFF / AIFF-C (`FORM....AIFF|AIFC`, or `spawn_aiff[_with_options]`: the walker of
soundkit-aiff, its per-sample decode -- byte order, widening, f64, G.711, IMA4 -- and the same output stage in the batched tick).
AudioData from WAV / raw PCM / AIFF streams carries the real `audio_format` and `endianness`.
MP4 / M4A (`....ftyp`) with an AAC-LC track, regular (`moov` in front of `mdat`) or fragmented: demuxed on the entropy thread
(csrc/mp4_stream.h), then exactly an ADTS stream; whole files in any box order, and ALAC tracks, go through `mp4.decode_file`.
WebM / Matroska (`1A 45 DF A3`) with one A_VORBIS, A_AAC or A_FLAC track: demuxed on the entropy thread (csrc/webm_stream.h), then
exactly a Vorbis-packet, ADTS or native FLAC stream; anything else in it: `unsupported or disabled WebM codec: ID`.
MPEG transport stream (`.ts`, `.m2ts`: three syncs at stride 188 or 192, or `spawn_mpeg_ts` for a join in mid-segment) with an ADTS AAC,
MPEG Layer I / II / III or stereo Blu-ray LPCM track: demuxed on the entropy thread (csrc/ts_stream.h), then exactly an ADTS, MPEG audio
or big-endian raw PCM stream; LATM, AC-3, DTS: `unsupported MPEG-TS audio codec NAME`.
The reference's other formats stay with their CPU decoders (out of scope)."""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._lib import AudioInfo, DecodeOptionsC, PipelineConfig, PipelineStats, RawPcmFormatC, SoundkitError, check, lib
from .audio_types import AudioData, EncodingFlag, Endianness
from .engine import FMT_F32LE, FMT_S16BE, FMT_S16LE, default_engine

SK_PIPE_INPUT_FULL, SK_PIPE_CLOSED, SK_PIPE_CHUNK_TOO_LARGE, SK_ERR_CAPACITY = -201, -202, -203, -7


@dataclass
class DecodeOptions:  # lib.rs:147-151
    output_bits_per_sample: Optional[int] = None
    output_sample_rate: Optional[int] = None
    output_channels: Optional[int] = None


@dataclass
class RawPcmFormat:  # soundkit/src/raw_pcm.rs:39-126; `format` is one of engine.FMT_*
    sample_rate: int
    channels: int
    format: int = FMT_S16LE

    def __post_init__(self):  # validate, raw_pcm.rs:117-125
        if self.sample_rate == 0:
            raise ValueError("Raw PCM sample rate must be > 0")
        if self.channels == 0:
            raise ValueError("Raw PCM channel count must be > 0")

    @classmethod
    def linear16(cls, sample_rate, channels):  # signed 16-bit little-endian, raw_pcm.rs:62-69
        return cls(sample_rate, channels, FMT_S16LE)

    @classmethod
    def l16(cls, sample_rate, channels):  # RFC 3551 L16: signed 16-bit big-endian, raw_pcm.rs:71-78
        return cls(sample_rate, channels, FMT_S16BE)

    @classmethod
    def linear32(cls, sample_rate, channels):  # 32-bit float little-endian, raw_pcm.rs:80-87
        return cls(sample_rate, channels, FMT_F32LE)


class DecodeError(Exception):  # lib.rs:108-141
    def __init__(self, kind, message="", status=0):
        self.kind, self.status = kind, status
        super().__init__(message or {"InputBufferFull": "Input buffer full", "PipelineClosed": "Decode pipeline is closed"}.get(kind, kind))


class BatchScheduler:
    """One per GPU.  Keyword arguments are the fields of sk_pipeline_config (0 / missing = default)."""

    def __init__(self, engine=None, **config):
        """config: the fields of sk_pipeline_config.  gpu_entropy: 0 host front-end, 1 AAC front-end on the GPU, 2 host Huffman decode +
        device rest, 3 = 1 with the MP3 streams' scale factors and Huffman decode in the tick as well"""
        self.engine = engine or default_engine()
        cfg = PipelineConfig()
        for k, v in config.items():
            if not hasattr(cfg, k):
                raise TypeError("unknown scheduler option %r" % k)
            setattr(cfg, k, int(v))
        h = C.c_void_p()
        check(lib.sk_pipeline_create(self.engine._h, C.byref(cfg), C.byref(h)), "sk_pipeline_create", self.engine._h)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib.sk_pipeline_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def spawn(self, options=None):
        options = options or DecodeOptions()
        o = DecodeOptionsC(options.output_sample_rate or 0, options.output_bits_per_sample or 0, options.output_channels or 0, 0)
        handle = C.c_uint32()
        rc = lib.sk_pipeline_spawn(self._h, C.byref(o), C.byref(handle))
        if rc != 0:
            raise SoundkitError(rc, "sk_pipeline_spawn")
        return DecodePipelineHandle(self, handle.value)

    def spawn_raw_pcm(self, format, options=None):
        """DecodePipeline::spawn_raw_pcm_with_options (lib.rs:2475-2486): a stream of headerless PCM"""
        options = options or DecodeOptions()
        o = DecodeOptionsC(options.output_sample_rate or 0, options.output_bits_per_sample or 0, options.output_channels or 0, 0)
        f = RawPcmFormatC(format.sample_rate, format.channels, format.format, 0)
        handle = C.c_uint32()
        rc = lib.sk_pipeline_spawn_raw_pcm(self._h, C.byref(f), C.byref(o), C.byref(handle))
        if rc != 0:
            raise SoundkitError(rc, "sk_pipeline_spawn_raw_pcm")
        return DecodePipelineHandle(self, handle.value)

    def spawn_mpeg_ts(self, options=None):
        """a stream known to be an MPEG transport stream (sk_pipeline_spawn_mpeg_ts): nothing is detected, the demuxer finds the first
        sync itself -- for a join in mid-segment; `spawn` takes a stream that begins at a packet by itself"""
        options = options or DecodeOptions()
        o = DecodeOptionsC(options.output_sample_rate or 0, options.output_bits_per_sample or 0, options.output_channels or 0, 0)
        handle = C.c_uint32()
        rc = lib.sk_pipeline_spawn_mpeg_ts(self._h, C.byref(o), C.byref(handle))
        if rc != 0:
            raise SoundkitError(rc, "sk_pipeline_spawn_mpeg_ts")
        return DecodePipelineHandle(self, handle.value)

    def spawn_aiff(self, options=None):
        """DecodePipeline::spawn_aiff_with_options (lib.rs:2714-2724): an AIFF / AIFF-C stream, its decoder there from the start"""
        options = options or DecodeOptions()
        o = DecodeOptionsC(options.output_sample_rate or 0, options.output_bits_per_sample or 0, options.output_channels or 0, 0)
        handle = C.c_uint32()
        rc = lib.sk_pipeline_spawn_aiff(self._h, C.byref(o), C.byref(handle))
        if rc != 0:
            raise SoundkitError(rc, "sk_pipeline_spawn_aiff")
        return DecodePipelineHandle(self, handle.value)

    def spawn_alac_packets(self, magic_cookie, options=None):
        """a stream of ALAC packets (sk_pipeline_spawn_alac_packets): the cookie once, then every `send` is exactly one packet; the
        empty send ends the stream and flushes the resampler"""
        options = options or DecodeOptions()
        o = DecodeOptionsC(options.output_sample_rate or 0, options.output_bits_per_sample or 0, options.output_channels or 0, 0)
        cookie = bytes(magic_cookie)
        handle = C.c_uint32()
        rc = lib.sk_pipeline_spawn_alac_packets(self._h, cookie, len(cookie), C.byref(o), C.byref(handle))
        if rc != 0:
            raise SoundkitError(rc, "sk_pipeline_spawn_alac_packets")
        return DecodePipelineHandle(self, handle.value)

    def spawn_vorbis_packets(self, ident, comment, setup, options=None):
        """a stream of demuxed Vorbis packets (sk_pipeline_spawn_vorbis_packets, the A_VORBIS case): the three header packets once, then
        every `send` is exactly one audio packet; the empty send ends the stream and flushes the resampler"""
        options = options or DecodeOptions()
        o = DecodeOptionsC(options.output_sample_rate or 0, options.output_bits_per_sample or 0, options.output_channels or 0, 0)
        ident, comment, setup = bytes(ident), bytes(comment), bytes(setup)
        handle, text = C.c_uint32(), C.create_string_buffer(256)
        rc = lib.sk_pipeline_spawn_vorbis_packets(self._h, ident, len(ident), comment, len(comment), setup, len(setup), C.byref(o), C.byref(handle), text, 256)
        if rc != 0:
            raise SoundkitError(rc, "sk_pipeline_spawn_vorbis_packets", text.value.decode())
        return DecodePipelineHandle(self, handle.value)

    def spawn_g711(self, law, sample_rate, channels, options=None):
        """a headerless G.711 stream (sk_pipeline_spawn_g711): law = telephony.ULAW / ALAW; every non-empty `send` gives one AudioData"""
        from . import telephony
        if law not in (telephony.ULAW, telephony.ALAW):
            raise ValueError("law must be telephony.ULAW or telephony.ALAW, not %r" % (law,))
        options = options or DecodeOptions()
        o = DecodeOptionsC(options.output_sample_rate or 0, options.output_bits_per_sample or 0, options.output_channels or 0, 0)
        handle, text = C.c_uint32(), C.create_string_buffer(128)
        rc = lib.sk_pipeline_spawn_g711(self._h, int(law), int(sample_rate), int(channels), C.byref(o), C.byref(handle), text, 128)
        if rc == telephony.ERR_STREAM:
            raise telephony.TelephonyError(text.value.decode())
        if rc != 0:
            raise SoundkitError(rc, "sk_pipeline_spawn_g711")
        return DecodePipelineHandle(self, handle.value)

    def spawn_g722(self, options=None):
        """a headerless G.722 stream at 64 kbit/s, 16 kHz mono (sk_pipeline_spawn_g722)"""
        options = options or DecodeOptions()
        o = DecodeOptionsC(options.output_sample_rate or 0, options.output_bits_per_sample or 0, options.output_channels or 0, 0)
        handle = C.c_uint32()
        rc = lib.sk_pipeline_spawn_g722(self._h, C.byref(o), C.byref(handle))
        if rc != 0:
            raise SoundkitError(rc, "sk_pipeline_spawn_g722")
        return DecodePipelineHandle(self, handle.value)

    def spawn_g726(self, rate=32000, packing=0, options=None):
        """a headerless G.726 stream, 8 kHz mono (sk_pipeline_spawn_g726): rate 16000 / 24000 / 32000 / 40000, packing telephony.LEFT /
        RIGHT; a `send` that completes no group gives nothing, a partial group at the end is the stream's error"""
        from . import telephony
        telephony._check_codec(telephony.G726, rate, packing)
        options = options or DecodeOptions()
        o = DecodeOptionsC(options.output_sample_rate or 0, options.output_bits_per_sample or 0, options.output_channels or 0, 0)
        handle = C.c_uint32()
        rc = lib.sk_pipeline_spawn_g726(self._h, int(rate), int(packing), C.byref(o), C.byref(handle))
        if rc != 0:
            raise SoundkitError(rc, "sk_pipeline_spawn_g726")
        return DecodePipelineHandle(self, handle.value)

    def spawn_gsm(self, variant=0, options=None):
        """a GSM 06.10 full-rate stream, 8 kHz mono (sk_pipeline_spawn_gsm): variant telephony.GSM_STANDARD (33-byte frames) /
        GSM_MICROSOFT (65-byte pairs); a `send` that completes no packet gives nothing, a partial packet at the end or a frame without
        the magic nibble is the stream's error"""
        from . import telephony
        telephony._check_gsm_variant(variant)
        options = options or DecodeOptions()
        o = DecodeOptionsC(options.output_sample_rate or 0, options.output_bits_per_sample or 0, options.output_channels or 0, 0)
        handle = C.c_uint32()
        rc = lib.sk_pipeline_spawn_gsm(self._h, int(variant), C.byref(o), C.byref(handle))
        if rc != 0:
            raise SoundkitError(rc, "sk_pipeline_spawn_gsm")
        return DecodePipelineHandle(self, handle.value)

    def wait_outputs(self, timeout_ms=100, cap=256):
        """Handles (as spawned: `handle.id`) that have outputs or have ended; blocks up to timeout_ms.  For callers that
        serve many streams from one thread."""
        arr = (C.c_uint32 * cap)()
        n = lib.sk_pipeline_wait_outputs(self._h, arr, cap, timeout_ms)
        if n < 0:
            raise SoundkitError(n, "sk_pipeline_wait_outputs")
        return list(arr[:n])

    def stats(self):
        st = PipelineStats()
        check(lib.sk_pipeline_get_stats(self._h, C.byref(st)), "sk_pipeline_get_stats")
        return {name: getattr(st, name) for name, _ in st._fields_ if name != "reserved"}


class DecodePipelineHandle:
    """lib.rs:2788-2889"""

    def __init__(self, scheduler, handle):
        self._s, self._id = scheduler, handle
        self.id = handle
        self._buf = np.empty(1 << 16, np.uint8)
        self._info = AudioInfo()

    def send(self, data):
        if self._id is None:
            raise DecodeError("PipelineClosed")
        data = bytes(data)
        rc = lib.sk_pipeline_send(self._s._h, self._id, data if data else None, len(data))
        if rc == SK_PIPE_INPUT_FULL:
            raise DecodeError("InputBufferFull")
        if rc == SK_PIPE_CLOSED:
            raise DecodeError("PipelineClosed")
        if rc == SK_PIPE_CHUNK_TOO_LARGE:
            raise DecodeError("InputChunkTooLarge", "Input chunk of %d bytes exceeds the 4 MiB limit" % len(data))
        if rc != 0:
            raise SoundkitError(rc, "sk_pipeline_send")

    def finish(self):
        self.send(b"")

    def _take(self, call, on_empty=None):
        if self._id is None:
            raise DecodeError("PipelineClosed")
        for _ in range(2):
            rc = call()
            if rc == SK_ERR_CAPACITY:
                self._buf = np.empty(int(self._info.bytes) * 2, np.uint8)
                continue
            break
        if rc == SK_PIPE_CLOSED:
            return None
        if rc == 0:
            if on_empty is not None:
                raise on_empty
            return None
        if rc != 1:
            raise SoundkitError(rc, "sk_pipeline_recv")
        i = self._info
        payload = self._buf[:i.bytes].tobytes()
        if i.is_error:
            return DecodeError("DecodingFailed", payload.decode("utf-8", "replace"), i.status)
        return AudioData(i.bits_per_sample, i.channel_count, i.sampling_rate, payload,
                         EncodingFlag.PCMFloat if i.reserved & 1 else EncodingFlag.PCMSigned,
                         Endianness.BigEndian if i.reserved & 2 else Endianness.LittleEndian)

    def try_recv(self):
        """None when nothing is ready (or the stream has ended and is drained); else AudioData or a DecodeError value."""
        return self._take(lambda: lib.sk_pipeline_try_recv(self._s._h, self._id, self._buf.ctypes.data, self._buf.size,
                                                           C.byref(self._info)))

    def recv(self, timeout_ms=10000):
        """Blocks for the next output: AudioData or a DecodeError value; None only when the stream has ended and is
        drained.  A wait that runs out raises TimeoutError -- it never looks like the end of the stream."""
        return self._take(lambda: lib.sk_pipeline_recv(self._s._h, self._id, self._buf.ctypes.data, self._buf.size,
                                                       C.byref(self._info), timeout_ms),
                          TimeoutError("no output within %d ms" % timeout_ms))

    def ended(self):
        """True once the worker side has ended and every output has been taken."""
        if self._id is None:
            return True
        rc = lib.sk_pipeline_try_recv(self._s._h, self._id, self._buf.ctypes.data, 0, C.byref(self._info))
        return rc == SK_PIPE_CLOSED

    def cancel(self):
        if self._id is not None and self._s._h:
            lib.sk_pipeline_cancel(self._s._h, self._id)
        self._id = None

    def queued_input_bytes(self):
        if self._id is None:
            raise DecodeError("PipelineClosed")
        return lib.sk_pipeline_queued_input_bytes(self._s._h, self._id)

    def __del__(self):  # Drop, lib.rs:2884-2888
        try:
            self.cancel()
        except Exception:
            pass


_scheduler = None


def default_scheduler():
    global _scheduler
    if _scheduler is None:
        _scheduler = BatchScheduler()
    return _scheduler


class DecodePipeline:
    """lib.rs:2590-2786"""

    @staticmethod
    def spawn():
        return default_scheduler().spawn(DecodeOptions())

    @staticmethod
    def spawn_with_options(options):
        return default_scheduler().spawn(options)

    @staticmethod
    def spawn_mpeg_ts(options=None):
        return default_scheduler().spawn_mpeg_ts(options)

    @staticmethod
    def spawn_aiff():
        return default_scheduler().spawn_aiff(DecodeOptions())

    @staticmethod
    def spawn_aiff_with_options(options):
        return default_scheduler().spawn_aiff(options)

    @staticmethod
    def spawn_alac_packets(magic_cookie, options=None):
        return default_scheduler().spawn_alac_packets(magic_cookie, options)

    @staticmethod
    def spawn_vorbis_packets(ident, comment, setup, options=None):
        return default_scheduler().spawn_vorbis_packets(ident, comment, setup, options)

    @staticmethod
    def spawn_g711(law, sample_rate, channels, options=None):
        return default_scheduler().spawn_g711(law, sample_rate, channels, options)

    @staticmethod
    def spawn_g722(options=None):
        return default_scheduler().spawn_g722(options)

    @staticmethod
    def spawn_g726(rate=32000, packing=0, options=None):
        return default_scheduler().spawn_g726(rate, packing, options)

    @staticmethod
    def spawn_gsm(variant=0, options=None):
        return default_scheduler().spawn_gsm(variant, options)

    @staticmethod
    def spawn_raw_pcm(format):
        return default_scheduler().spawn_raw_pcm(format, DecodeOptions())

    @staticmethod
    def spawn_raw_pcm_with_options(format, options):
        return default_scheduler().spawn_raw_pcm(format, options)

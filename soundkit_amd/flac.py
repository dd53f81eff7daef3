"""FLAC (RFC 9639): the host's header parser, framer and stream reader (csrc/flac_stream.h), the GPU decode stage
(csrc/flac_decode.hip) and soundkit-flac's FlacDecoder (soundkit-flac/src/lib.rs:122-219) on top of them.

Not built: Ogg FLAC, FLAC in MP4, decode_f32, 32-bit frames with a side channel, MD5 / total-sample verification."""
import ctypes as C

import numpy as np

from ._lib import FlacFrameInfo, FlacInfo, FlacStreamInfo, SoundkitError, check, lib
from .engine import _ptr, default_engine

NEED_MORE, NO_SYNC, RESERVED, BAD_CRC, NEED_STREAMINFO, INVALID, ERR_STREAM = -501, -502, -503, -504, -505, -506, -507
FRAME_FIELDS = ("number", "offset", "frame_bytes", "sample_rate", "block_size", "header_bytes", "channels", "assignment", "bits_per_sample",
                "variable_blocksize")


def _bytes(data):
    return np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)


def frame_dict(f):
    return {n: int(getattr(f, n)) for n in FRAME_FIELDS}


def frame_info(d):
    f = FlacFrameInfo()
    for n in FRAME_FIELDS:
        setattr(f, n, int(d.get(n, 0)))
    return f


def streaminfo(sample_rate=0, channels=0, bits_per_sample=0, max_framesize=0, **more):
    """a sk_flac_streaminfo for parse_header / scan"""
    s = FlacStreamInfo()
    s.sample_rate, s.channels, s.bits_per_sample, s.max_framesize = sample_rate, channels, bits_per_sample, max_framesize
    for k, v in more.items():
        setattr(s, k, v)
    return s


def streaminfo_dict(s):
    d = {n: int(getattr(s, n)) for n in ("min_blocksize", "max_blocksize", "min_framesize", "max_framesize", "sample_rate", "channels",
                                        "bits_per_sample", "total_samples")}
    d["md5"] = bytes(s.md5)
    return d


def parse_header(data, info=None):
    """one frame header -> (status, dict)"""
    b, f = _bytes(data), FlacFrameInfo()
    rc = lib.sk_flac_parse_header(_ptr(b), len(data), C.byref(info) if info is not None else None, C.byref(f))
    return rc, frame_dict(f)


def scan(data, info=None, final=False, cap=4096):
    """whole frames out of bytes that begin at a frame -> (status, [dict], consumed)"""
    b = _bytes(data)
    frames = (FlacFrameInfo * max(cap, 1))()
    n, used = C.c_uint32(0), C.c_size_t(0)
    rc = lib.sk_flac_scan(_ptr(b), len(data), C.byref(info) if info is not None else None, 1 if final else 0, frames, cap, C.byref(n), C.byref(used))
    return rc, [frame_dict(frames[i]) for i in range(n.value)], used.value


class FlacReader:
    """sk_flac_reader: a stream from its fLaC marker on, cut anywhere -> whole frames"""

    def __init__(self):
        self._h = C.c_void_p()
        check(lib.sk_flac_reader_create(C.byref(self._h)), "sk_flac_reader_create")

    def close(self):
        if self._h:
            lib.sk_flac_reader_destroy(self._h)
            self._h = C.c_void_p()

    def add(self, data, cap=4096):
        """-> [(dict, frame bytes)]; an empty add is the finalising one.  Raises SoundkitError with the reader's text."""
        b = _bytes(data)
        frames = (FlacFrameInfo * max(cap, 1))()
        n, base = C.c_uint32(0), C.c_void_p()
        rc = lib.sk_flac_reader_add(self._h, _ptr(b), len(data), frames, cap, C.byref(n), C.byref(base))
        if rc != 0:
            raise SoundkitError(rc, "sk_flac_reader_add", self.last_error())
        return [(frame_dict(frames[i]), C.string_at(base.value + frames[i].offset, frames[i].frame_bytes)) for i in range(n.value)]

    def info(self):
        i = FlacInfo()
        check(lib.sk_flac_reader_info(self._h, C.byref(i)), "sk_flac_reader_info")
        return {"streaminfo": streaminfo_dict(i.streaminfo) if i.have_streaminfo else None, "frames": int(i.frames),
                "buffered_bytes": int(i.buffered_bytes)}

    def last_error(self):
        return lib.sk_flac_reader_last_error(self._h).decode()


def pack_frames(frames):
    """[(dict, frame bytes)] -> (FlacFrameInfo array with offsets into the packed bytes, the bytes; every frame at a 16-byte aligned offset)"""
    table = (FlacFrameInfo * max(len(frames), 1))()
    blob = bytearray()
    for i, (d, b) in enumerate(frames):
        blob += bytes(-len(blob) % 16)
        table[i] = frame_info(dict(d, offset=len(blob), frame_bytes=len(b)))
        blob += b
    return table, bytes(blob)


def out_bytes(frames):
    return sum(d["block_size"] * d["channels"] * (1 if d["bits_per_sample"] <= 8 else 2 if d["bits_per_sample"] <= 16 else
                                                  3 if d["bits_per_sample"] <= 24 else 4) for d, _ in frames)


def decode_frames(frames, engine=None, fill=0):
    """sk_flac_decode_frames over [(dict, frame bytes)] -> (the contract's PCM as bytes, [status per frame]).  A rejected frame's place
    keeps `fill`."""
    engine = engine or default_engine()
    table, blob = pack_frames(frames)
    src = _bytes(blob)
    out = np.full(max(out_bytes(frames), 16), fill, np.uint8)
    status = np.zeros(max(len(frames), 1), np.int32)
    n = C.c_size_t(0)
    check(lib.sk_flac_decode_frames(engine._h, table, len(frames), _ptr(src), _ptr(out), out.size, C.byref(n), _ptr(status)),
          "sk_flac_decode_frames", engine._h)
    return out[:n.value].tobytes(), status[:len(frames)].tolist()


class FlacDecoder:
    """soundkit-flac's FlacDecoder (soundkit-flac/src/lib.rs:122-219): sample_rate / channels / bits_per_sample / reset / decode_i16 /
    decode_i32; bytes in at any chunking, interleaved samples out.  A call with no bytes fetches frames an earlier call had no room for (pending_samples) and, once none
    waits, finalises the stream and drains what is left (0 = nothing is).  Errors
    raise SoundkitError with the decoder's text.  decode_f32 is not built."""

    def __init__(self, engine=None):
        self._engine = engine or default_engine()
        self._h = C.c_void_p()
        check(lib.sk_flac_decoder_create(self._engine._h, C.byref(self._h)), "sk_flac_decoder_create", self._engine._h)

    def close(self):
        if self._h:
            lib.sk_flac_decoder_destroy(self._h)
            self._h = C.c_void_p()

    def _info(self):
        rate, ch, bits, frames = C.c_uint32(0), C.c_uint8(0), C.c_uint8(0), C.c_uint64(0)
        check(lib.sk_flac_decoder_info(self._h, C.byref(rate), C.byref(ch), C.byref(bits), C.byref(frames)), "sk_flac_decoder_info")
        return rate.value, ch.value, bits.value, frames.value

    def sample_rate(self):
        return self._info()[0] or None

    def channels(self):
        return self._info()[1] or None

    def bits_per_sample(self):
        return self._info()[2] or None

    def frames_decoded(self):
        return self._info()[3]

    def pending_samples(self):
        """samples of the frames that wait for room in `out`: while not 0, a call with no bytes only fetches them"""
        return lib.sk_flac_decoder_pending_samples(self._h)

    def reset(self):
        check(lib.sk_flac_decoder_reset(self._h), "sk_flac_decoder_reset")

    def last_error(self):
        return lib.sk_flac_decoder_last_error(self._h).decode()

    def _decode(self, fn, data, out):
        b = _bytes(data)
        n = C.c_size_t(0)
        rc = fn(self._h, _ptr(b), len(data), _ptr(out), out.size, C.byref(n))
        if rc != 0:
            detail = self.last_error() if rc == ERR_STREAM else (lib.sk_engine_last_hip_error(self._engine._h).decode() if rc in (-3, -4, -8) else "")
            raise SoundkitError(rc, "sk_flac_decoder_decode", detail)
        return n.value

    def decode_i16(self, data, out):
        assert out.dtype == np.int16
        return self._decode(lib.sk_flac_decoder_decode_i16, data, out)

    def decode_i32(self, data, out):
        assert out.dtype == np.int32
        return self._decode(lib.sk_flac_decoder_decode_i32, data, out)

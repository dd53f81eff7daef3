"""Apple Lossless: the host's cookie parser, packet header reader and CAF packet index (csrc/alac_stream.h), the GPU decode stage
(csrc/alac_decode.hip), soundkit-alac's AlacPacketDecoder and CafAlacPacketIndex (soundkit-alac/src/lib.rs:24-300) on top of them, and
decode_caf: soundkit-decoder's decode_seekable_caf_audio (lib.rs:1029-1092) for an ALAC file.

Channels leave in bitstream order.  ALAC in MP4: mp4.py (its demuxer hands cookie and packets to the same calls)."""
import ctypes as C

import numpy as np

from ._lib import AlacConfig, AlacPacket, CafAlacInfo, SoundkitError, check, lib
from .engine import _ptr, default_engine

INVALID, ERR_STREAM, UNSUPPORTED_ELEMENT = -601, -602, -603
MAX_PACKET_BYTES = 16 * 1024 * 1024
CONFIG_FIELDS = ("frame_length", "sample_rate", "max_frame_bytes", "avg_bit_rate", "max_run", "compatible_version", "bit_depth", "pb", "mb",
                 "kb", "channels")


def _bytes(data):
    return np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)


def config_dict(c):
    return {n: int(getattr(c, n)) for n in CONFIG_FIELDS}


def config(d):
    """a sk_alac_config from a dict (or one already made)"""
    if isinstance(d, AlacConfig):
        return d
    c = AlacConfig()
    for n in CONFIG_FIELDS:
        setattr(c, n, int(d.get(n, 0)))
    return c


def parse_cookie(cookie):
    """the bare ALACSpecificConfig, the MP4 `alac` FullBox payload or the QuickTime `frma` + `alac` form -> dict.  Raises SoundkitError
    with the parser's text."""
    b, c, text = _bytes(cookie), AlacConfig(), C.create_string_buffer(256)
    rc = lib.sk_alac_parse_cookie(_ptr(b), len(cookie), C.byref(c), text, len(text))
    if rc != 0:
        raise SoundkitError(rc, "sk_alac_parse_cookie", text.value.decode())
    return config_dict(c)


def packet_frames(cfg, packet):
    """-> (status, the frame count the packet's first audio element states)"""
    b, n = _bytes(packet), C.c_uint32(0)
    rc = lib.sk_alac_packet_frames(C.byref(config(cfg)), _ptr(b), len(packet), C.byref(n))
    return rc, n.value


class CafAlacPacketIndex:
    """CafAlacPacketIndex (soundkit-alac/src/lib.rs:24-154): config, valid / priming / remainder frames, frames_per_packet and
    packets = [(absolute offset, size)]"""

    def __init__(self, handle):
        try:
            info = CafAlacInfo()
            check(lib.sk_caf_alac_index_info(handle, C.byref(info)), "sk_caf_alac_index_info")
            self.config = config_dict(info.config)
            self.sample_rate, self.channels, self.bit_depth = self.config["sample_rate"], self.config["channels"], self.config["bit_depth"]
            self.valid_frames, self.priming_frames, self.remainder_frames = int(info.valid_frames), int(info.priming_frames), int(info.remainder_frames)
            self.frames_per_packet = int(info.frames_per_packet)
            n = int(info.n_packets)
            offsets, sizes = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32)
            check(lib.sk_caf_alac_index_packets(handle, _ptr(offsets), _ptr(sizes), n), "sk_caf_alac_index_packets")
            self.packets = [(int(offsets[i]), int(sizes[i])) for i in range(n)]
        finally:
            lib.sk_caf_alac_index_destroy(handle)

    @classmethod
    def new(cls, description, magic_cookie, packet_table, data_payload_offset, data_payload_size):
        d, k, t = _bytes(description), _bytes(magic_cookie), _bytes(packet_table)
        h, text = C.c_void_p(), C.create_string_buffer(256)
        rc = lib.sk_caf_alac_index_create(_ptr(d), len(description), _ptr(k), len(magic_cookie), _ptr(t), len(packet_table), data_payload_offset,
                                          data_payload_size, C.byref(h), text, len(text))
        if rc != 0:
            raise SoundkitError(rc, "sk_caf_alac_index_create", text.value.decode())
        return cls(h)

    @classmethod
    def from_file(cls, data):
        b = _bytes(data)
        h, text = C.c_void_p(), C.create_string_buffer(256)
        rc = lib.sk_caf_alac_index_from_file(_ptr(b), len(data), C.byref(h), text, len(text))
        if rc != 0:
            raise SoundkitError(rc, "sk_caf_alac_index_from_file", text.value.decode())
        return cls(h)

    def packet_bytes(self, data):
        """the packets of the file the index was made from"""
        return [bytes(data[o:o + s]) for o, s in self.packets]

    def trim(self, index, decoded_frames):
        """pcm_packet_trim (soundkit-audio-demux/src/caf.rs:365-393): the frames of packet `index` that lie in the programme ->
        (first frame, count) or None.  A packet's place on the timeline is index * frames_per_packet."""
        start = index * self.frames_per_packet
        lo, hi = max(start, self.priming_frames), min(start + decoded_frames, self.priming_frames + self.valid_frames)
        return (lo - start, hi - lo) if hi > lo else None


def pack_packets(packets):
    """[packet bytes] -> (AlacPacket array with offsets into the packed bytes, the bytes; every packet at a 16-byte aligned offset)"""
    table = (AlacPacket * max(len(packets), 1))()
    blob = bytearray()
    for i, p in enumerate(packets):
        blob += bytes(-len(blob) % 16)
        table[i].offset, table[i].size = len(blob), len(p)
        blob += p
    return table, bytes(blob)


def decode_packets(cfg, packets, engine=None, fill=0):
    """sk_alac_decode_packets over [packet bytes] -> (the PCM as bytes, [status per packet], [frames per packet]).  A rejected packet's
    place keeps `fill`."""
    engine = engine or default_engine()
    c = config(cfg)
    table, blob = pack_packets(packets)
    src = _bytes(blob)
    n = len(packets)
    cap = n * int(c.frame_length) * int(c.channels) * (int(c.bit_depth) // 8)
    out = np.full(max(cap, 16), fill, np.uint8)
    status, frames = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint32)
    used = C.c_size_t(0)
    check(lib.sk_alac_decode_packets(engine._h, C.byref(c), table, n, _ptr(src), _ptr(out), out.size, C.byref(used), _ptr(status), _ptr(frames)),
          "sk_alac_decode_packets", engine._h)
    return out[:used.value].tobytes(), status[:n].tolist(), frames[:n].tolist()


class AlacPacketDecoder:
    """soundkit-alac's AlacPacketDecoder (lib.rs:217-300): a magic cookie once, one packet per decode_packet -> AudioData.  Errors raise
    SoundkitError with the decoder's text; the decoder goes on with the next packet."""

    def __init__(self, magic_cookie, engine=None):
        self._engine = engine or default_engine()
        self._h = C.c_void_p()
        b, text = _bytes(magic_cookie), C.create_string_buffer(256)
        rc = lib.sk_alac_packet_decoder_create(self._engine._h, _ptr(b), len(magic_cookie), C.byref(self._h), text, len(text))
        if rc != 0:
            raise SoundkitError(rc, "sk_alac_packet_decoder_create", text.value.decode())
        rate, ch, depth, most = C.c_uint32(0), C.c_uint8(0), C.c_uint8(0), C.c_size_t(0)
        check(lib.sk_alac_packet_decoder_info(self._h, C.byref(rate), C.byref(ch), C.byref(depth), C.byref(most)), "sk_alac_packet_decoder_info")
        self._info = (rate.value, ch.value, depth.value, most.value)
        self._out = np.zeros(max(most.value * (depth.value // 8), 16), np.uint8)

    def close(self):
        if self._h:
            lib.sk_alac_packet_decoder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sample_rate(self):
        return self._info[0]

    def channels(self):
        return self._info[1]

    def bit_depth(self):
        return self._info[2]

    def maximum_pcm_samples(self):
        return self._info[3]

    def last_error(self):
        return lib.sk_alac_packet_decoder_last_error(self._h).decode()

    def decode_packet(self, packet):
        from .audio_types import AudioData, Endianness, EncodingFlag
        if len(packet) > MAX_PACKET_BYTES:  # said here, so that 16 MiB need not be copied to be refused
            raise SoundkitError(ERR_STREAM, "sk_alac_packet_decoder_decode_packet", "ALAC packet exceeds the %d byte budget" % MAX_PACKET_BYTES)
        b, n = _bytes(packet), C.c_size_t(0)
        rc = lib.sk_alac_packet_decoder_decode_packet(self._h, _ptr(b), len(packet), _ptr(self._out), self._out.size, C.byref(n))
        if rc != 0:
            detail = self.last_error() if rc == ERR_STREAM else (lib.sk_engine_last_hip_error(self._engine._h).decode() if rc in (-3, -4, -8) else "")
            raise SoundkitError(rc, "sk_alac_packet_decoder_decode_packet", detail)
        rate, ch, depth, _ = self._info
        return AudioData(depth, ch, rate, self._out[:n.value].tobytes(), EncodingFlag.PCMSigned, Endianness.LittleEndian)


def decode_caf(data, options=None, scheduler=None, engine=None):
    """decode_seekable_caf_audio (soundkit-decoder/src/lib.rs:1029-1092) for an ALAC CAF file: index -> every packet decoded in one call
    -> each trimmed by priming / valid frames -> the output options -> the resampler's flush.  -> (the index, [AudioData]).
    Without options that change anything the AudioData are the trimmed packets themselves; otherwise they are what the scheduler's raw
    PCM stream of the file's format makes of them (the same conversion stage every PCM-family input ends in)."""
    index = CafAlacPacketIndex.from_file(data)
    packets = index.packet_bytes(data)
    pcm, status, frames = decode_packets(index.config, packets, engine)
    width = index.channels * (index.bit_depth // 8)
    pieces, at = [], 0
    for i, (st, n) in enumerate(zip(status, frames)):
        if st != 0:
            raise SoundkitError(ERR_STREAM, "decode_caf", "Decoding failed: ALAC packet %d: %s" % (i, lib.sk_strerror(st).decode()))
        t = index.trim(i, n)
        if t:
            pieces.append(pcm[at + t[0] * width:at + (t[0] + t[1]) * width])
        at += n * width
    if not pieces:
        raise SoundkitError(ERR_STREAM, "decode_caf", "Decoding failed: CAF track emitted no audio frames")
    return index, output_stage(pieces, index.sample_rate, index.channels, index.bit_depth, options, scheduler)


def output_stage(pieces, sample_rate, channels, bit_depth, options=None, scheduler=None, is_float=False, big_endian=False):
    """[PCM bytes: signed little-endian, or as is_float / big_endian say] -> [AudioData] under the output options, the resampler flushed
    at the end (what decode_caf, mp4.decode_file and caf.decode_file end in).  Without options that change anything the AudioData are the
    pieces themselves, in the byte order they came in; otherwise they are what the scheduler's raw PCM stream of that format makes of
    them (the same conversion stage every PCM-family input ends in)."""
    from .audio_types import AudioData, Endianness, EncodingFlag
    from .engine import FMT_F32BE, FMT_F32LE, FMT_S16BE, FMT_S16LE, FMT_S24BE, FMT_S24LE, FMT_S32BE, FMT_S32LE
    from .pipeline import DecodeError, DecodeOptions, RawPcmFormat, default_scheduler
    o = options or DecodeOptions()
    same = ((o.output_sample_rate or sample_rate) == sample_rate and (o.output_channels or channels) == channels and
            (o.output_bits_per_sample or bit_depth) == bit_depth)
    if same:
        return [AudioData(bit_depth, channels, sample_rate, p, EncodingFlag.PCMFloat if is_float else EncodingFlag.PCMSigned,
                          Endianness.BigEndian if big_endian else Endianness.LittleEndian) for p in pieces]
    if is_float:
        fmt = {32: FMT_F32BE if big_endian else FMT_F32LE}[bit_depth]
    else:
        fmt = {16: (FMT_S16LE, FMT_S16BE), 24: (FMT_S24LE, FMT_S24BE), 32: (FMT_S32LE, FMT_S32BE)}[bit_depth][1 if big_endian else 0]
    h = (scheduler or default_scheduler()).spawn_raw_pcm(RawPcmFormat(sample_rate, channels, fmt), o)
    out = []

    def take():
        a = h.recv()
        if a is not None and not isinstance(a, AudioData):
            raise a
        if a is not None:
            out.append(a)
        return a

    try:
        for p in pieces + [b""]:  # the empty send ends the stream and flushes the resampler
            while True:
                try:
                    h.send(p)
                    break
                except DecodeError as e:
                    if e.kind != "InputBufferFull":
                        raise
                    take()
        while take() is not None:
            pass
    finally:
        h.cancel()
    return out

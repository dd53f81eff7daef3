"""Ogg Vorbis: the host's Ogg page parser (csrc/ogg_stream.h), the three header parsers and the stream's device tables
(csrc/vorbis_stream.h), the GPU decode stage (csrc/vorbis_decode.hip), and on top of them soundkit's OggPacketParser
(soundkit/src/ogg.rs), VorbisPacketDecoder and VorbisDecoder (soundkit-vorbis/src/lib.rs; sk_vorbis_packet_decoder_*, sk_vorbis_decoder_*).

The tick is Engine.tick_run_vorbis (sk_tick_run_vorbis).  In the scheduler: DecodePipeline.spawn() takes an Ogg Vorbis stream by
its first bytes, DecodePipeline.spawn_vorbis_packets takes demuxed packets.  Not built: floor type 0, more than 8 channels."""
import ctypes as C

import numpy as np

from ._lib import (OggPacketInfo, SoundkitError, VorbisIdent, VorbisPacket, VorbisPacketInfo, VorbisSetupInfo, VorbisStream, check, lib)
from .engine import _ptr, default_engine

NOT_AUDIO, BAD_MODE, SHORT, ERR_STREAM = -801, -802, -803, -804
IDENT_FIELDS = ("sample_rate", "bitrate_maximum", "bitrate_nominal", "bitrate_minimum", "blocksize_0", "blocksize_1", "channels")


def _bytes(data):
    return np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)


def ogg_page_crc(page):
    b = _bytes(page)
    return int(lib.sk_ogg_page_crc(_ptr(b), len(page)))


class OggPacket:
    __slots__ = ("data", "serial", "first_in_stream", "last_in_page", "last_in_stream", "granule_position")

    def __init__(self, data, info):
        self.data, self.serial = data, int(info.serial)
        self.first_in_stream, self.last_in_page, self.last_in_stream = bool(info.first_in_stream), bool(info.last_in_page), bool(info.last_in_stream)
        self.granule_position = int(info.granule_position) if info.has_granule else None

    def __eq__(self, other):
        return all(getattr(self, n) == getattr(other, n) for n in self.__slots__)

    def __repr__(self):
        return "OggPacket(%d bytes, serial %d, first %d, last in page %d, last %d, granule %r)" % (
            len(self.data), self.serial, self.first_in_stream, self.last_in_page, self.last_in_stream, self.granule_position)


class OggPacketParser:
    """OggPacketParser (soundkit/src/ogg.rs): add(bytes) -> [OggPacket], finish() -> [OggPacket].  Refusals raise SoundkitError with the
    reference's text."""

    def __init__(self):
        self._h = C.c_void_p()
        check(lib.sk_ogg_parser_create(C.byref(self._h)), "sk_ogg_parser_create")

    def close(self):
        if self._h:
            lib.sk_ogg_parser_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _drain(self):
        out, info = [], OggPacketInfo()
        while lib.sk_ogg_parser_pending(self._h):
            rc = lib.sk_ogg_parser_take(self._h, C.byref(info), None, 0)
            buf = np.zeros(max(int(info.size), 1), np.uint8)
            if rc != 0:
                check(lib.sk_ogg_parser_take(self._h, C.byref(info), _ptr(buf), buf.size), "sk_ogg_parser_take")
            out.append(OggPacket(buf[:info.size].tobytes(), info))
        return out

    def _checked(self, rc, what):
        if rc != 0:
            raise SoundkitError(rc, what, lib.sk_ogg_parser_last_error(self._h).decode() if rc == ERR_STREAM else "")

    def add(self, data):
        if len(data) > 4 * 1024 * 1024:  # said here, so that the bytes need not be copied to be refused
            raise SoundkitError(ERR_STREAM, "sk_ogg_parser_add", "Ogg input chunk exceeds the 4194304 byte streaming budget")
        b = _bytes(data)
        self._checked(lib.sk_ogg_parser_add(self._h, _ptr(b), len(data)), "sk_ogg_parser_add")
        return self._drain()

    def finish(self):
        self._checked(lib.sk_ogg_parser_finish(self._h), "sk_ogg_parser_finish")
        return self._drain()


def parse_ident(packet):
    """-> dict of the identification header; raises SoundkitError with the parser's text"""
    b, ident, text = _bytes(packet), VorbisIdent(), C.create_string_buffer(256)
    rc = lib.sk_vorbis_parse_ident(_ptr(b), len(packet), C.byref(ident), text, len(text))
    if rc != 0:
        raise SoundkitError(rc, "sk_vorbis_parse_ident", text.value.decode())
    return {n: int(getattr(ident, n)) for n in IDENT_FIELDS}


def parse_comment(packet):
    b, text = _bytes(packet), C.create_string_buffer(256)
    rc = lib.sk_vorbis_parse_comment(_ptr(b), len(packet), text, len(text))
    if rc != 0:
        raise SoundkitError(rc, "sk_vorbis_parse_comment", text.value.decode())


class Setup:
    """a parsed, validated setup header with the stream's device tables (sk_vorbis_setup)"""

    def __init__(self, ident, packet):
        self.ident = dict(ident)
        c = VorbisIdent()
        for n in IDENT_FIELDS:
            setattr(c, n, int(ident.get(n, 0)))
        b, text = _bytes(packet), C.create_string_buffer(256)
        self._h = C.c_void_p()
        rc = lib.sk_vorbis_setup_create(C.byref(c), _ptr(b), len(packet), C.byref(self._h), text, len(text))
        if rc != 0:
            self._h = C.c_void_p()
            raise SoundkitError(rc, "sk_vorbis_setup_create", text.value.decode())
        info = VorbisSetupInfo()
        check(lib.sk_vorbis_setup_get_info(self._h, C.byref(info)), "sk_vorbis_setup_get_info")
        self.info = {n: int(getattr(info, n)) for n, _ in VorbisSetupInfo._fields_ if n != "reserved"}
        self.channels, self.blocksizes = self.info["channels"], (self.info["blocksize_0"], self.info["blocksize_1"])

    def close(self):
        if getattr(self, "_h", None):
            lib.sk_vorbis_setup_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def packet_blocksize(self, packet):
        """-> (status, block size) from the packet's first bits"""
        b, n = _bytes(packet), C.c_uint32(0)
        rc = lib.sk_vorbis_packet_blocksize(self._h, _ptr(b), len(packet), C.byref(n))
        return rc, n.value


class StreamState:
    """what a stream carries from call to call: the block size of its previous accepted packet and that packet's windowed right half"""

    def __init__(self, setup):
        self.setup, self.prev_blocksize = setup, 0
        self.overlap = np.zeros((setup.channels, setup.blocksizes[1] // 2), np.float32)

    def copy(self):
        c = StreamState(self.setup)
        c.prev_blocksize, c.overlap = self.prev_blocksize, self.overlap.copy()
        return c


def _pack(groups):
    """[(state or setup, [packet bytes])] -> (VorbisStream array, VorbisPacket array, the packed bytes, packet count)"""
    n = sum(len(p) for _, p in groups)
    streams, table, blob = (VorbisStream * max(len(groups), 1))(), (VorbisPacket * max(n, 1))(), bytearray()
    k = 0
    for i, (st, packets) in enumerate(groups):
        setup = st.setup if isinstance(st, StreamState) else st
        streams[i].setup, streams[i].n_packets = setup._h, len(packets)
        if isinstance(st, StreamState):
            streams[i].overlap, streams[i].prev_blocksize = st.overlap.ctypes.data, st.prev_blocksize
        for p in packets:
            blob += bytes(-len(blob) % 16)
            table[k].offset, table[k].size = len(blob), len(p)
            blob += p
            k += 1
    return streams, table, bytes(blob), n


def decode_packets(groups, as_f32=False, engine=None):
    """sk_vorbis_decode_packets over [(StreamState, [packet bytes])]: every stream's packets in one launch sequence; the states are
    updated.  -> ([per stream: [per packet: (status, interleaved samples as an array of [frames][channels])]])"""
    engine = engine or default_engine()
    streams, table, blob, n = _pack(groups)
    src = _bytes(blob)
    cap = sum(len(p) * st.setup.blocksizes[1] // 2 * st.setup.channels for st, p in groups)
    out = np.zeros(max(cap, 8), np.float32 if as_f32 else np.int16)
    status, frames, used = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint32), C.c_size_t(0)
    check(lib.sk_vorbis_decode_packets(engine._h, streams, len(groups), table, n, _ptr(src), len(blob), 1 if as_f32 else 0, _ptr(out), out.nbytes,
                                       C.byref(used), _ptr(status), _ptr(frames)), "sk_vorbis_decode_packets", engine._h)
    res, k, at = [], 0, 0
    for i, (st, packets) in enumerate(groups):
        st.prev_blocksize = int(streams[i].prev_blocksize)
        ch, rows = st.setup.channels, []
        for _ in packets:
            f = int(frames[k])
            rows.append((int(status[k]), out[at:at + f * ch].reshape(f, ch).copy()))
            at += f * ch
            k += 1
        res.append(rows)
    return res


def entropy_decode(groups, engine=None):
    """sk_vorbis_entropy_decode over [(Setup, [packet bytes])] -> [per stream: [per packet: dict(status, mode, blockflag, prev_flag,
    next_flag, blocksize, used[ch], final_y[ch][65], step2[ch][65], residue[ch][blocksize / 2])]]"""
    engine = engine or default_engine()
    streams, table, blob, n = _pack(groups)
    src = _bytes(blob)
    cap = sum(len(p) * (st.setup if isinstance(st, StreamState) else st).blocksizes[1] // 2 * (st.setup if isinstance(st, StreamState) else st).channels
              for st, p in groups)
    residue, info, used = np.zeros(max(cap, 8), np.float32), (VorbisPacketInfo * max(n, 1))(), C.c_size_t(0)
    check(lib.sk_vorbis_entropy_decode(engine._h, streams, len(groups), table, n, _ptr(src), len(blob), info, _ptr(residue), residue.size, C.byref(used)),
          "sk_vorbis_entropy_decode", engine._h)
    raw = np.frombuffer(bytes(info), np.uint8).reshape(max(n, 1), C.sizeof(VorbisPacketInfo))
    res, k, at = [], 0, 0
    for st, packets in groups:
        ch = (st.setup if isinstance(st, StreamState) else st).channels
        rows = []
        for _ in packets:
            r, o = info[k], raw[k]
            d = dict(status=int(r.status), mode=int(r.mode), blockflag=int(r.blockflag), prev_flag=int(r.prev_flag), next_flag=int(r.next_flag),
                     blocksize=int(r.blocksize), used=list(r.used)[:ch],
                     final_y=o[20:20 + 1040].view("<i2").reshape(8, 65)[:ch].astype(np.int32), step2=o[1060:1580].reshape(8, 65)[:ch].copy())
            half = d["blocksize"] // 2 if d["status"] == 0 else 0
            d["residue"] = residue[at:at + ch * half].reshape(ch, half).copy()
            at += ch * half
            rows.append(d)
            k += 1
        res.append(rows)
    return res


class _Handle:
    _destroy = None

    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _info(self):
        rate, ch = C.c_uint32(0), C.c_uint8(0)
        return (rate.value, ch.value) if self._info_fn(self._h, C.byref(rate), C.byref(ch), *self._info_more) == 0 else (None, None)

    def sample_rate(self):
        return self._info()[0]

    def channels(self):
        return self._info()[1]


class VorbisPacketDecoder(_Handle):
    """soundkit-vorbis's VorbisPacketDecoder (sk_vorbis_packet_decoder_*): the three header packets, then raw audio packets (Matroska /
    WebM A_VORBIS), one per decode_packet -> None for a header, else the packet's interleaved s16 samples (an empty array for the first
    audio packet).  A header or a packet that is refused raises SoundkitError; after a refused audio packet the decoder goes on with
    the next."""
    _destroy, _info_fn, _info_more = lib.sk_vorbis_packet_decoder_destroy, lib.sk_vorbis_packet_decoder_info, (None,)

    def __init__(self, engine=None):
        self._engine, self._h = engine or default_engine(), C.c_void_p()
        check(lib.sk_vorbis_packet_decoder_create(self._engine._h, C.byref(self._h)), "sk_vorbis_packet_decoder_create")
        self._out = np.zeros(8 * 4096, np.int16)  # 8 channels x blocksize 8192 / 2

    def decode_packet(self, packet):
        b, n, produced = _bytes(packet), C.c_size_t(0), C.c_int(0)
        rc = lib.sk_vorbis_packet_decoder_decode_packet(self._h, _ptr(b), len(packet), _ptr(self._out), self._out.size, C.byref(n), C.byref(produced))
        if rc != 0:
            detail = lib.sk_engine_last_hip_error(self._engine._h).decode() if rc in (-3, -4, -8) else lib.sk_vorbis_packet_decoder_last_error(self._h).decode()
            raise SoundkitError(rc, "sk_vorbis_packet_decoder_decode_packet", detail)
        return self._out[:n.value].copy() if produced.value else None


class VorbisDecoder(_Handle):
    """soundkit-vorbis's VorbisDecoder (sk_vorbis_decoder_*): Ogg bytes in any pieces through add, then finish; each returns an AudioData
    (16 bits, interleaved, little-endian) when the packets that became complete produced samples, else None -- all of a call's audio
    packets in one launch sequence.  The serial check, the truncation of the stream's last packet to the final granule position and
    the error texts are the reference's process_packet's."""
    _destroy, _info_fn, _info_more = lib.sk_vorbis_decoder_destroy, lib.sk_vorbis_decoder_info, ()

    def __init__(self, engine=None):
        self._engine, self._h = engine or default_engine(), C.c_void_p()
        check(lib.sk_vorbis_decoder_create(self._engine._h, C.byref(self._h)), "sk_vorbis_decoder_create")
        self._out = np.zeros(1 << 16, np.int16)

    def _call(self, what, fn, *args):
        from .audio_types import AudioData, Endianness, EncodingFlag
        n = C.c_size_t(0)
        rc = fn(self._h, *args, _ptr(self._out), self._out.size, C.byref(n))
        if rc == -7:  # SK_ERR_CAPACITY: the samples wait; fetch them with room
            self._out = np.zeros(n.value, np.int16)
            rc = lib.sk_vorbis_decoder_add(self._h, None, 0, _ptr(self._out), self._out.size, C.byref(n))
        if rc != 0:
            detail = lib.sk_engine_last_hip_error(self._engine._h).decode() if rc in (-3, -4, -8) else lib.sk_vorbis_decoder_last_error(self._h).decode()
            raise SoundkitError(rc, what, detail)
        if n.value == 0:
            return None
        rate, ch = self._info()
        return AudioData(16, ch, rate, self._out[:n.value].astype("<i2").tobytes(), EncodingFlag.PCMSigned, Endianness.LittleEndian)

    def add(self, data):
        if len(data) > 4 * 1024 * 1024:  # said here, so that the bytes need not be copied to be refused
            raise SoundkitError(ERR_STREAM, "sk_vorbis_decoder_add", "Ogg input chunk exceeds the 4194304 byte streaming budget")
        b = _bytes(data)
        return self._call("sk_vorbis_decoder_add", lib.sk_vorbis_decoder_add, _ptr(b), len(data))

    def finish(self):
        return self._call("sk_vorbis_decoder_finish", lib.sk_vorbis_decoder_finish)

"""Writes MPEG program streams for the tests: pack headers in the MPEG-2 and the MPEG-1 layout, a system header, padding and video
packets, PES packets with MPEG-2 and MPEG-1 headers, DVD LPCM in private_stream_1 and MPEG audio PES.  The DVD LPCM packer is written
from the layout's description (csrc/ps_stream.h, include/soundkit_amd.h: SK_AIFF_DVD_S24), not from tests/ps_model.py, which unpacks.
The audio comes from tests/golden/ (avi_builder's sources)."""
import struct

import avi_builder as A

RATE_CODES = {48000: 0, 96000: 1, 44100: 2, 32000: 3}


def stamp(prefix, value):
    """the five bytes of a PTS / DTS"""
    return bytes([(prefix << 4) | (((value >> 30) & 7) << 1) | 1, (value >> 22) & 0xFF, (((value >> 15) & 0x7F) << 1) | 1, (value >> 7) & 0xFF,
                  ((value & 0x7F) << 1) | 1])


def pack_header(mpeg2=True, stuffing=0):
    if mpeg2:  # 00 00 01 BA, `01` + SCR ... 10 bytes, the last one's low three bits: the stuffing count
        return b"\x00\x00\x01\xba" + bytes([0x44, 0x00, 0x04, 0x00, 0x04, 0x01, 0x01, 0x89, 0xC3, 0xF8 | stuffing]) + b"\xff" * stuffing
    return b"\x00\x00\x01\xba" + bytes([0x21, 0x00, 0x01, 0x00, 0x01, 0x80, 0x1B, 0x91])  # `0010` + SCR, mux rate: 12 bytes


def packet(stream_id, body):
    """a start code, the 16-bit length, the bytes"""
    return b"\x00\x00\x01" + bytes([stream_id]) + struct.pack(">H", len(body)) + body


def system_header():
    return packet(0xBB, bytes([0x80, 0xC4, 0xE1, 0x04, 0xE1, 0x7F, 0xB9, 0xE0, 0xE8, 0xBD, 0xC0, 0x20]))


def padding(n=40):
    return packet(0xBE, b"\xff" * n)


def pes2(stream_id, payload, pts=None, dts=None, stuffing=0):
    """a PES packet with the MPEG-2 header: `10` flags, the PTS / DTS flags, the header's data length"""
    fields = b""
    if pts is not None and dts is not None:
        fields = stamp(3, pts) + stamp(1, dts)
    elif pts is not None:
        fields = stamp(2, pts)
    flags = 0xC0 if dts is not None and pts is not None else (0x80 if pts is not None else 0)
    return packet(stream_id, bytes([0x81, flags, len(fields) + stuffing]) + fields + b"\xff" * stuffing + payload)


def pes1(stream_id, payload, pts=None, dts=None, stuffing=0, std=False):
    """a PES packet with the MPEG-1 header: FF stuffing, the 2-byte `01` STD buffer field, then `0010` PTS, `0011` PTS + DTS or 0F"""
    head = b"\xff" * stuffing + (b"\x60\x20" if std else b"")
    if pts is not None and dts is not None:
        head += stamp(3, pts) + stamp(1, dts)
    elif pts is not None:
        head += stamp(2, pts)
    else:
        head += b"\x0f"
    return packet(stream_id, head + payload)


def video(n=300, length_zero=False):
    body = bytes([0x81, 0x00, 0x00]) + b"\x00\x00\x01\xb3" + bytes([0x55]) * n  # (a sequence header's start code inside the payload)
    return b"\x00\x00\x01\xe0\x00\x00" + body if length_zero else packet(0xE0, body)


# ---- DVD LPCM -------------------------------------------------------------------------------------------------------------------------

def lpcm_header(bits, rate, channels, substream=0xA0, frames=0, first_access=4):
    """substream id, the three bytes of the DVD substream header, then the three bytes the decoder reads: emphasis / mute / frame number,
    quantisation (top two bits) + rate code (two bits) + channels - 1 (low three bits), dynamic range"""
    return bytes([substream, frames & 0xFF, first_access >> 8, first_access & 0xFF, 0x00, (((bits - 16) // 4) << 6) | (RATE_CODES[rate] << 4) | (channels - 1), 0x80])


def pack16(le):
    """interleaved little-endian s16 -> DVD LPCM's big-endian samples"""
    out = bytearray(le)
    out[0::2], out[1::2] = le[1::2], le[0::2]
    return bytes(out)


def pack24(le):
    """interleaved little-endian s24 -> DVD LPCM's 12-byte groups: of every four consecutive samples first the upper 16 bits of each,
    big-endian, then the four low bytes.  The sample count is a multiple of four."""
    assert len(le) % 12 == 0
    out = bytearray()
    for at in range(0, len(le), 12):
        four = [le[at + 3 * i:at + 3 * i + 3] for i in range(4)]
        for s in four:
            out += bytes([s[2], s[1]])
        for s in four:
            out.append(s[0])
    return bytes(out)


def block_bytes(bits, channels):
    if bits == 16:
        return 2 * channels
    return 12 if channels in (1, 2, 4) else (24 if channels == 8 else 12 * channels)


def lpcm_stream(packed, bits, rate, channels, sizes, mpeg1=False, substream=0xA0, noise=True):
    """a program stream whose DVD LPCM packets carry `packed` in pieces of `sizes` bytes (cycled; blocks may straddle packets), between
    pack headers, a system header, padding and video packets"""
    out = [pack_header(not mpeg1), system_header()]
    for k, piece in enumerate(A.split(packed, sizes)):
        body = lpcm_header(bits, rate, channels, substream, k) + piece
        out.append(pack_header(not mpeg1, stuffing=k % 4 if not mpeg1 else 0))
        if noise:
            out.append(video(100 + k % 7, length_zero=k % 5 == 4))
        out.append(pes1(0xBD, body, 90000 + k, stuffing=k % 3, std=k % 2 == 0) if mpeg1 else pes2(0xBD, body, 90000 + k, stuffing=k % 3))
        if noise and k % 3 == 0:
            out.append(padding(20 + k))
    out.append(b"\x00\x00\x01\xb9")
    return b"".join(out)


def mpa_stream(es, sizes, stream_id=0xC0, mpeg1=False, other=None):
    """a program stream whose MPEG audio PES packets (stream_id) carry the elementary stream in pieces; `other`: a second audio stream id
    whose packets lie in between"""
    out = [pack_header(not mpeg1), system_header()]
    for k, piece in enumerate(A.split(es, sizes)):
        out.append(pack_header(not mpeg1))
        out.append(video(80 + k % 9))
        if other is not None:
            out.append(pes2(other, bytes([0x11]) * 64, 5000 + k))
        out.append(pes1(stream_id, piece, 90000 + k, 90000 + k, std=True) if mpeg1 else pes2(stream_id, piece, 90000 + k, 90000 + k))
    out.append(b"\x00\x00\x01\xb9")
    return b"".join(out)


def widen(le16, channels, bits=16):
    """mono little-endian s16 -> `channels` interleaved channels (channel c attenuated by c bits, so the channels differ) at 16 or 24 bits
    (the low byte carries the sample index, so that a misplaced low byte shows)"""
    out = bytearray()
    n = len(le16) // 2
    for k, (s,) in enumerate(struct.iter_unpack("<h", le16)):
        for c in range(channels):
            v = s >> c
            out += struct.pack("<h", v) if bits == 16 else bytes([(k * channels + c) & 0xFF]) + struct.pack("<h", v)
    assert len(out) == n * channels * bits // 8
    return bytes(out)


MP2 = A.golden("mp2", "stereo48k_A_Tusk_1s.mp2")


def cases():
    """name -> (file, kind, the track's bytes as the demuxer hands them out (DVD LPCM: still packed), rate, channels, bits,
    the little-endian PCM the track decodes to or None)"""
    out = {}
    frames = 2400  # a multiple of the frames per block at every channel count below
    for bits in (16, 24):
        for channels in (1, 2, 6, 8):
            pcm = widen(A.S16[2 * 1000:2 * (1000 + frames)], channels, bits)
            packed = pack16(pcm) if bits == 16 else pack24(pcm)
            # packet sizes that are no multiple of any block size: blocks straddle packets
            out["lpcm%d_%dch" % (bits, channels)] = (lpcm_stream(packed, bits, 48000, channels, [2011, 1999, 997]), "pcm-dvd", packed, 48000, channels, bits, pcm)
    mono48 = A.S16_48K
    out["lpcm16_48k_mono_mpeg1"] = (lpcm_stream(pack16(mono48), 16, 48000, 1, [2000, 2014], mpeg1=True), "pcm-dvd", pack16(mono48), 48000, 1, 16, mono48)
    s24 = A.S24[:3 * 5996]  # 5996 frames: a multiple of four
    out["lpcm24_mono_44k"] = (lpcm_stream(pack24(s24), 24, 44100, 1, [1801], noise=False), "pcm-dvd", pack24(s24), 44100, 1, 24, s24)
    out["mp2"] = (mpa_stream(MP2, [2000, 1111]), "mpeg-audio", MP2, None, None, None, None)
    out["mp2_mpeg1_c1"] = (mpa_stream(MP2[:576 * 12], [700], stream_id=0xC1, mpeg1=True), "mpeg-audio", MP2[:576 * 12], None, None, None, None)
    return out

"""Synthetic AIFF / AIFF-C containers for the tests: chunks with their padding, COMM with an 80-bit extended sample rate, SSND with
its offset field, FORM with a size that may be told wrong on purpose, and IMA4 packets."""
import math
import struct

import numpy as np


def extended(rate):
    """IEEE 754 80-bit extended, big-endian, of a positive finite float (or the raw 10 bytes when given bytes)"""
    if isinstance(rate, (bytes, bytearray)):
        assert len(rate) == 10
        return bytes(rate)
    if rate == 0:
        return bytes(10)
    sign = 0x8000 if rate < 0 else 0
    m, e = math.frexp(abs(rate))  # abs = m * 2^e, 0.5 <= m < 1
    mantissa = int(m * (1 << 64))  # exact: m has 53 bits
    return struct.pack(">HQ", sign | (e - 1 + 16383), mantissa)


def chunk(cid, payload, declared=None):
    """one chunk: id, big-endian size (declared overrides it), payload, and the pad byte of an odd payload"""
    size = len(payload) if declared is None else declared
    return bytes(cid) + struct.pack(">I", size) + bytes(payload) + (b"\0" if len(payload) & 1 else b"")


def comm(channels, frames, sample_size, rate, tag=None, name=b"", extra=b""):
    """COMM: AIFF when tag is None, AIFF-C otherwise (compression tag + Pascal-string name, padded to even)"""
    body = struct.pack(">HIH", channels, frames, sample_size) + extended(rate)
    if tag is not None:
        pname = bytes([len(name)]) + bytes(name)
        body += bytes(tag) + pname + (b"\0" if len(pname) & 1 else b"")
    return chunk(b"COMM", body + extra)


def ssnd(audio, offset=0, block=0):
    """SSND: offset, block size, `offset` filler bytes, the sound bytes"""
    return chunk(b"SSND", struct.pack(">II", offset, block) + b"\xee" * offset + bytes(audio))


def form(chunks, aifc=False, kind=None, size=None):
    body = (kind if kind is not None else (b"AIFC" if aifc else b"AIFF")) + b"".join(chunks)
    return b"FORM" + struct.pack(">I", len(body) if size is None else size) + body


def fver():
    return chunk(b"FVER", struct.pack(">I", 0xA2805140))


def simple(enc_tag, channels, sample_size, rate, audio, frames=0, aifc=None, extra_chunks=()):
    """FORM { [FVER] COMM extra... SSND }"""
    aifc = enc_tag is not None if aifc is None else aifc
    head = [fver()] if aifc else []
    return form(head + [comm(channels, frames, sample_size, rate, enc_tag)] + list(extra_chunks) + [ssnd(audio)], aifc)


def ima4_packets(rng, groups, channels, pinned=None):
    """random IMA4 packets: groups x channels x 34 bytes.  pinned = (first, last, sign): those groups hold step index 88 and all-maximal
    nibbles of one sign, so the decoded signal sticks at a rail"""
    p = rng.integers(0, 256, (groups, channels, 34), dtype=np.uint8)
    p[:, :, 1] = (p[:, :, 1] & 0x80) | rng.integers(0, 89, (groups, channels), dtype=np.uint8)  # a valid step index
    if pinned:
        first, last, negative = pinned
        p[first:last, :, 2:] = 0xff if negative else 0x77
        p[first:last, :, 1] = (p[first:last, :, 1] & 0x80) | 88
    return p

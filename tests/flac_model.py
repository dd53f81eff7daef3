"""A plain-Python FLAC decoder (RFC 9639) on big integers, written from the RFC and independent of the product: frame headers,
subframes, Rice partitions, prediction, stereo decorrelation, CRC-8 / CRC-16, STREAMINFO and the MD5 of the samples.  It finds a
frame's end by decoding the frame, not by searching for the next header, so it also checks the product's framer.

tests/test_flac_cpu.py pins it: the reference's fixture decodes to tests/golden/linear16_A_Tusk.s16le, whose MD5 is the one in the
fixture's STREAMINFO, and all CRCs hold."""
import hashlib


class FlacError(Exception):
    pass


def crc8(data):
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


_CRC16 = []
for _i in range(256):
    _c = _i << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x8005) & 0xFFFF if _c & 0x8000 else (_c << 1) & 0xFFFF
    _CRC16.append(_c)


def crc16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _CRC16[(c >> 8) ^ b]
    return c


class Bits:
    def __init__(self, data, pos=0):
        self.n = len(data) * 8
        self.v = int.from_bytes(data, "big")
        self.pos = pos

    def read(self, n):
        if n == 0:
            return 0
        if self.pos + n > self.n:
            raise FlacError("read past the end")
        self.pos += n
        return (self.v >> (self.n - self.pos)) & ((1 << n) - 1)

    def signed(self, n):
        v = self.read(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self):
        count = 0
        while True:
            left = self.n - self.pos
            if left <= 0:
                raise FlacError("unary run past the end")
            w = min(64, left)
            v = (self.v >> (left - w)) & ((1 << w) - 1)
            if v:
                z = w - v.bit_length()
                self.pos += z + 1
                return count + z
            count += w
            self.pos += w


RATES = [None, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000]
DEPTHS = [None, 8, 12, "reserved", 16, 20, 24, 32]


def parse_streaminfo(b):
    assert len(b) == 34
    v = int.from_bytes(b[10:18], "big")
    return {"min_blocksize": int.from_bytes(b[0:2], "big"), "max_blocksize": int.from_bytes(b[2:4], "big"),
            "min_framesize": int.from_bytes(b[4:7], "big"), "max_framesize": int.from_bytes(b[7:10], "big"),
            "sample_rate": v >> 44, "channels": ((v >> 41) & 7) + 1, "bits_per_sample": ((v >> 36) & 31) + 1,
            "total_samples": v & ((1 << 36) - 1), "md5": bytes(b[18:34])}


def parse_header(data, streaminfo=None):
    """-> dict (with header_bytes) or raises FlacError"""
    r = Bits(data[:16])
    if r.read(15) != 0x7FFC:
        raise FlacError("no sync")
    variable = r.read(1)
    bs_code, rate_code, assignment, depth_code = r.read(4), r.read(4), r.read(4), r.read(3)
    if r.read(1) or bs_code == 0 or rate_code == 15 or depth_code == 3 or assignment > 10:
        raise FlacError("reserved")
    first = r.read(8)
    if first < 0x80:
        number, extra = first, 0
    else:
        extra = 0
        while first & (0x80 >> extra):
            extra += 1
        if extra < 2 or extra > 7:
            raise FlacError("reserved coded number")
        number, extra = first & (0x7F >> extra), extra - 1
        for _ in range(extra):
            c = r.read(8)
            if c >> 6 != 2:
                raise FlacError("reserved coded number")
            number = (number << 6) | (c & 0x3F)
    if bs_code == 1:
        block = 192
    elif bs_code <= 5:
        block = 576 << (bs_code - 2)
    elif bs_code == 6:
        block = r.read(8) + 1
    elif bs_code == 7:
        block = r.read(16) + 1
    else:
        block = 256 << (bs_code - 8)
    if rate_code < 12:
        rate = RATES[rate_code]
    elif rate_code == 12:
        rate = r.read(8) * 1000
    elif rate_code == 13:
        rate = r.read(16)
    else:
        rate = r.read(16) * 10
    n = r.pos // 8
    if crc8(data[:n]) != r.read(8):
        raise FlacError("CRC-8")
    bits = DEPTHS[depth_code]
    if rate is None or bits is None:
        if streaminfo is None:
            raise FlacError("needs STREAMINFO")
        rate = rate or streaminfo["sample_rate"]
        bits = bits or streaminfo["bits_per_sample"]
    return {"number": number, "sample_rate": rate, "block_size": block, "header_bytes": n + 1,
            "channels": assignment + 1 if assignment < 8 else 2, "assignment": assignment, "bits_per_sample": bits,
            "variable_blocksize": variable}


FIXED = [[], [1], [2, -1], [3, -3, 1], [4, -6, 4, -1]]


def _residual(r, block, order, out):
    method = r.read(2)
    if method > 1:
        raise FlacError("reserved residual coding method")
    pbits, escape = (5, 31) if method else (4, 15)
    porder = r.read(4)
    if block % (1 << porder) or (block >> porder) < order:
        raise FlacError("partition order")
    per = block >> porder
    for p in range(1 << porder):
        k = r.read(pbits)
        count = per - order if p == 0 else per
        if k == escape:
            width = r.read(5)
            for _ in range(count):
                out.append(r.signed(width))
        else:
            for _ in range(count):
                u = (r.unary() << k) | r.read(k)
                out.append((u >> 1) ^ -(u & 1))


def _subframe(r, block, bps):
    if r.read(1):
        raise FlacError("padding bit")
    kind = r.read(6)
    wasted = r.unary() + 1 if r.read(1) else 0
    if wasted >= bps:
        raise FlacError("wasted bits")
    bps -= wasted
    if kind == 0:
        s = [r.signed(bps)] * block
    elif kind == 1:
        s = [r.signed(bps) for _ in range(block)]
    elif 8 <= kind <= 12 or kind >= 32:
        order = kind - 8 if kind < 32 else kind - 31
        if order > block:
            raise FlacError("order exceeds the block")
        s = [r.signed(bps) for _ in range(order)]
        if kind >= 32:
            precision = r.read(4) + 1
            if precision == 16:
                raise FlacError("precision code 15")
            shift = r.signed(5)
            if shift < 0:
                raise FlacError("negative shift")
            coefs = [r.signed(precision) for _ in range(order)]
        else:
            shift, coefs = 0, FIXED[order]
        res = []
        _residual(r, block, order, res)
        for e in res:
            s.append(e + (sum(c * s[-1 - j] for j, c in enumerate(coefs)) >> shift))
    else:
        raise FlacError("reserved subframe type")
    return [v << wasted for v in s]


def decode_frame(data, streaminfo=None, check_crc=True):
    """one frame at the start of data -> (header dict with frame_bytes, [channel][sample])"""
    h = parse_header(data, streaminfo)
    r = Bits(data, h["header_bytes"] * 8)
    a, bits, block = h["assignment"], h["bits_per_sample"], h["block_size"]
    if a >= 8 and bits >= 32:
        raise FlacError("33-bit side channel")
    ch = []
    for c in range(h["channels"]):
        side = (a == 8 and c == 1) or (a == 9 and c == 0) or (a == 10 and c == 1)
        ch.append(_subframe(r, block, bits + (1 if side else 0)))
    if a == 8:
        ch = [ch[0], [l - s for l, s in zip(ch[0], ch[1])]]
    elif a == 9:
        ch = [[s + x for s, x in zip(ch[0], ch[1])], ch[1]]
    elif a == 10:
        mids = [(m << 1) | (s & 1) for m, s in zip(ch[0], ch[1])]
        ch = [[(m + s) >> 1 for m, s in zip(mids, ch[1])], [(m - s) >> 1 for m, s in zip(mids, ch[1])]]
    pad = -r.pos % 8
    if r.read(pad):
        raise FlacError("padding bits")
    end = r.pos // 8 + 2
    if end > len(data):
        raise FlacError("frame past the end")
    if check_crc and crc16(data[:end]):
        raise FlacError("CRC-16")
    h["frame_bytes"] = end
    return h, ch


def decode_frames(data, streaminfo=None):
    """frames one after the other to the end of data -> [(header, channels)]"""
    out, pos = [], 0
    while pos < len(data):
        h, ch = decode_frame(data[pos:], streaminfo)
        h["offset"] = pos
        out.append((h, ch))
        pos += h["frame_bytes"]
    return out


def split_stream(data):
    """fLaC + metadata -> (streaminfo dict, [(type, body)], offset of the first frame)"""
    if data[:4] != b"fLaC":
        raise FlacError("no marker")
    pos, blocks, info = 4, [], None
    while True:
        last, kind, n = data[pos] >> 7, data[pos] & 127, int.from_bytes(data[pos + 1:pos + 4], "big")
        body = data[pos + 4:pos + 4 + n]
        if info is None:
            if kind != 0 or n != 34:
                raise FlacError("STREAMINFO")
            info = parse_streaminfo(body)
        blocks.append((kind, body))
        pos += 4 + n
        if last:
            return info, blocks, pos


def decode_stream(data):
    info, _, pos = split_stream(data)
    return info, decode_frames(data[pos:], info)


def width(bits):
    return 1 if bits <= 8 else 2 if bits <= 16 else 3 if bits <= 24 else 4


def contract_bytes(h, ch):
    """create_audio_data_i32_with_bits (soundkit-decoder/src/lib.rs:3191-3236): interleaved, little-endian, <= 8 bits as sample + 128"""
    w, out = width(h["bits_per_sample"]), bytearray()
    bias = 128 if w == 1 else 0
    for i in range(h["block_size"]):
        for c in ch:
            out += ((c[i] + bias) & ((1 << (8 * w)) - 1)).to_bytes(w, "little")
    return bytes(out)


def interleave(ch):
    return [c[i] for i in range(len(ch[0])) for c in ch]


def md5_of(frames, bits):
    """the STREAMINFO MD5: every sample interleaved, signed little-endian in ceil(bits / 8) bytes"""
    w, m = (bits + 7) // 8, hashlib.md5()
    for _, ch in frames:
        m.update(b"".join((v & ((1 << (8 * w)) - 1)).to_bytes(w, "little") for v in interleave(ch)))
    return m.digest()

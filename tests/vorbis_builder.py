"""Writes Vorbis headers and audio packets for the tests.  Every code book is a complete prefix code, so any random bit string is a
decodable packet: the end-of-packet paths, unused channels and every partition class come for free.  The books cover ordered and sparse
length lists, lookup types 0, 1 and 2 with and without sequence_p, and the one-entry case; the floors several classes with subclass
books; the residues types 0, 1 and 2; the mappings coupling steps and two submaps; two modes."""
import struct

import numpy as np


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, bits):
        assert 0 <= value < (1 << bits) or bits == 0, (value, bits)
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def ilog(x):
    return int(x).bit_length() if x > 0 else 0


def pack_float(mant, exp, neg=False):
    """mant * 2^exp in the Vorbis float format"""
    return (int(neg) << 31) | ((exp + 788) << 21) | mant


def book(dims, lengths, ordered=False, sparse=False, lookup=0, minimum=0, delta=0, value_bits=1, sequence_p=0, mults=()):
    return dict(dims=dims, lengths=list(lengths), ordered=ordered, sparse=sparse, lookup=lookup, minimum=minimum, delta=delta, value_bits=value_bits,
                sequence_p=sequence_p, mults=list(mults))


def default_books():
    return [
        book(1, [3] * 8),                                                                      # 0 scalar, plain list
        book(1, [1, 2, 3, 3], ordered=True),                                                   # 1 scalar, ordered list
        book(1, [2, 0, 2, 2, 0, 2], sparse=True),                                              # 2 scalar, sparse list
        book(2, [3] * 7 + [4, 4], lookup=1, minimum=pack_float(1, 0, True), delta=pack_float(1, 0), value_bits=2, mults=[0, 1, 2]),  # 3 lookup 1
        book(4, [2] * 4, lookup=2, minimum=pack_float(7, -1, True), delta=pack_float(1, -1), value_bits=4, sequence_p=1,
             mults=[(5 * i + 3) % 16 for i in range(16)]),                                     # 4 lookup 2 with sequence_p
        book(1, [1, 2, 3, 3], ordered=True, lookup=1, minimum=pack_float(3, -2, True), delta=pack_float(3, -3), value_bits=3, sequence_p=1,
             mults=[0, 2, 5, 7]),                                                              # 5 lookup 1, one dimension
        book(2, [4] * 16),                                                                     # 6 the residues' class book: 4 classes, 2 words
        book(1, [7] * 128),                                                                    # 7 scalar, the large Y values
        book(1, [1]),                                                                          # 8 the one-entry case
        book(2, [5] * 32, sparse=True, lookup=2, minimum=pack_float(1, 1, True), delta=pack_float(1, -4), value_bits=6,
             mults=[(7 * i + 1) % 64 for i in range(64)]),                                     # 9 lookup 2 without sequence_p
    ]


def floor(rangebits, multiplier, seed):
    rng = np.random.default_rng(seed)
    partition_class = [0, 1, 1, 2]
    classes = [dict(dim=1, sub=0, master=0, books=[0]), dict(dim=2, sub=1, master=1, books=[0, 7]), dict(dim=3, sub=2, master=0, books=[0, -1, 2, 8])]
    count = sum(classes[c]["dim"] for c in partition_class)
    x = sorted(rng.choice(np.arange(1, 1 << rangebits), count, replace=False).tolist())
    rng.shuffle(x)
    return dict(partition_class=partition_class, classes=classes, multiplier=multiplier, rangebits=rangebits, x=[int(v) for v in x])


def residue(rtype, end, partition_size=8):
    # class 0 adds nothing; 1: one pass; 2: two passes; 3: passes 0 and 2
    return dict(type=rtype, begin=0, end=end, partition_size=partition_size, classifications=4, classbook=6,
                books=[[-1] * 8, [3] + [-1] * 7, [4, 5] + [-1] * 6, [5, -1, 9] + [-1] * 5])


def default_setup(channels, bs0, bs1, rtype=(1, 2), multiplier=(2, 1), seed=0):
    """two floors, two residues, two mappings (short blocks: two submaps when there are two channels or more; long blocks: one), coupling
    when there are two channels or more, two modes"""
    submaps = 2 if channels >= 2 else 1
    coupling = ([(0, 1)] if channels >= 2 else []) + ([(2, 0)] if channels >= 3 else [])
    end = lambda t, bs, nch: (bs // 2) * (nch if t == 2 else 1)
    mux = [c % submaps for c in range(channels)]
    per_sub = [mux.count(i) for i in range(submaps)]
    return dict(
        channels=channels, bs=(bs0, bs1), books=default_books(),
        floors=[floor(ilog(bs0 // 2 - 1), multiplier[0], seed), floor(ilog(bs1 // 2 - 1), multiplier[1], seed + 1)],
        residues=[residue(rtype[0], end(rtype[0], bs0, max(per_sub))), residue(rtype[1], end(rtype[1], bs1, channels)),
                  residue(0, bs0 // 2 - 8)],
        mappings=[dict(submaps=submaps, coupling=coupling, mux=mux, floor=[0] * submaps, residue=[0, 2][:submaps]),
                  dict(submaps=1, coupling=coupling[::-1], mux=[0] * channels, floor=[1], residue=[1])],
        modes=[(0, 0), (1, 1)])


def ident_header(channels, sample_rate, bs0, bs1):
    return (b"\x01vorbis" + struct.pack("<IBIiii", 0, channels, sample_rate, 0, 128000, 0) + bytes([ilog(bs0 - 1) | ilog(bs1 - 1) << 4, 1]))


def comment_header(vendor=b"soundkit tests", comments=(b"TITLE=built",)):
    out = b"\x03vorbis" + struct.pack("<I", len(vendor)) + vendor + struct.pack("<I", len(comments))
    for c in comments:
        out += struct.pack("<I", len(c)) + c
    return out + b"\x01"


def setup_header(s):
    w = BitWriter()
    for b in b"\x05vorbis":
        w.put(b, 8)
    w.put(len(s["books"]) - 1, 8)
    for bk in s["books"]:
        entries = len(bk["lengths"])
        w.put(0x564342, 24)
        w.put(bk["dims"], 16)
        w.put(entries, 24)
        w.put(int(bk["ordered"]), 1)
        if bk["ordered"]:
            cur, ln = 0, bk["lengths"][0]
            w.put(ln - 1, 5)
            while cur < entries:
                num = sum(1 for v in bk["lengths"][cur:] if v == ln)
                w.put(num, ilog(entries - cur))
                cur += num
                ln += 1
        else:
            w.put(int(bk["sparse"]), 1)
            for ln in bk["lengths"]:
                if bk["sparse"]:
                    w.put(int(ln > 0), 1)
                if ln > 0 or not bk["sparse"]:
                    w.put(ln - 1, 5)
        w.put(bk["lookup"], 4)
        if bk["lookup"]:
            w.put(bk["minimum"], 32)
            w.put(bk["delta"], 32)
            w.put(bk["value_bits"] - 1, 4)
            w.put(bk["sequence_p"], 1)
            for m in bk["mults"]:
                w.put(m, bk["value_bits"])
    w.put(0, 6)
    w.put(s.get("time", 0), 16)
    w.put(len(s["floors"]) - 1, 6)
    for f in s["floors"]:
        w.put(f.get("type", 1), 16)
        w.put(len(f["partition_class"]), 5)
        for c in f["partition_class"]:
            w.put(c, 4)
        for c in f["classes"][:max(f["partition_class"]) + 1]:
            w.put(c["dim"] - 1, 3)
            w.put(c["sub"], 2)
            if c["sub"]:
                w.put(c["master"], 8)
            for bk in c["books"][:1 << c["sub"]]:
                w.put(bk + 1, 8)
        w.put(f["multiplier"] - 1, 2)
        w.put(f["rangebits"], 4)
        for v in f["x"]:
            w.put(v, f["rangebits"])
    w.put(len(s["residues"]) - 1, 6)
    for r in s["residues"]:
        w.put(r["type"], 16)
        w.put(r["begin"], 24)
        w.put(r["end"], 24)
        w.put(r["partition_size"] - 1, 24)
        w.put(r["classifications"] - 1, 6)
        w.put(r["classbook"], 8)
        cascades = [sum(1 << j for j in range(8) if row[j] >= 0) for row in r["books"]]
        for c in cascades:
            w.put(c & 7, 3)
            w.put(int(c >> 3 != 0), 1)
            if c >> 3:
                w.put(c >> 3, 5)
        for row in r["books"]:
            for v in row:
                if v >= 0:
                    w.put(v, 8)
    w.put(len(s["mappings"]) - 1, 6)
    for m in s["mappings"]:
        w.put(0, 16)
        w.put(int(m["submaps"] > 1), 1)
        if m["submaps"] > 1:
            w.put(m["submaps"] - 1, 4)
        w.put(int(bool(m["coupling"])), 1)
        if m["coupling"]:
            w.put(len(m["coupling"]) - 1, 8)
            for mag, ang in m["coupling"]:
                w.put(mag, ilog(s["channels"] - 1))
                w.put(ang, ilog(s["channels"] - 1))
        w.put(0, 2)
        if m["submaps"] > 1:
            for v in m["mux"]:
                w.put(v, 4)
        for i in range(m["submaps"]):
            w.put(0, 8)
            w.put(m["floor"][i], 8)
            w.put(m["residue"][i], 8)
    w.put(len(s["modes"]) - 1, 6)
    for flag, mapping in s["modes"]:
        w.put(flag, 1)
        w.put(0, 16)
        w.put(0, 16)
        w.put(mapping, 8)
    w.put(s.get("framing", 1), 1)
    return w.bytes()


def packet(rng, s, mode, prev=0, nxt=0, size=None):
    """an audio packet of random bits behind its first ones: the type bit, the mode number, a long block's window flags"""
    if size is None:
        size = int(rng.integers(8, 40)) + s["bs"][s["modes"][mode][0]] // 16
    body = int.from_bytes(rng.integers(0, 256, size, dtype=np.uint8).tobytes(), "little")
    bits = ilog(len(s["modes"]) - 1)
    head, n = mode << 1, 1 + bits
    if s["modes"][mode][0]:
        head |= prev << n | nxt << (n + 1)
        n += 2
    body = (body >> n << n) | head
    return body.to_bytes(size, "little")


def stream_packets(rng, s, count, long_share=0.5):
    """packets whose window flags agree with their neighbours' block sizes"""
    flags = [int(rng.random() < long_share) for _ in range(count)]
    out = []
    for i, f in enumerate(flags):
        prev = flags[i - 1] if i else 0
        nxt = flags[i + 1] if i + 1 < count else 0
        out.append(packet(rng, s, f, prev, nxt))
    return out

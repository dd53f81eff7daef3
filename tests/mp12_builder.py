"""Writes MPEG Layer I and II frames from chosen allocations, scale factors and sample codes -- what tests/mp3_builder.py is for
Layer III.  The tables are tests/mp12_model.py's (typed independently of the product's).  Every frame comes with what a parser
must find in it: the class byte and the three scale-factor indices of every (channel, subband), where the samples start, how
wide a granule is, and the bit behind the last code."""
import numpy as np

from mp12_model import BITRATES, GROUPED_BITS, ROWS, SAMPLE_RATES, TABLES, class_code, table_name


class BitWriter:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, bits):
        assert 0 <= value < (1 << bits) or bits == 0, (value, bits)
        self.v, self.n = (self.v << bits) | value, self.n + bits

    def bytes(self, total):
        """the first `total` bytes (zero-filled behind the last bit)"""
        pad = (-self.n) % 8
        raw = ((self.v << pad).to_bytes((self.n + pad) // 8, "big") if self.n else b"") + bytes(total)
        return raw[:total]


def header(layer, lsf, rate_index, bitrate_index, mode, mode_ext=0, crc=False, padding=0):
    version_bits = 2 if lsf else 3
    b1 = 0xE0 | (version_bits << 3) | ((4 - layer) << 1) | (0 if crc else 1)
    b2 = (bitrate_index << 4) | (rate_index << 2) | (padding << 1)
    b3 = (mode << 6) | (mode_ext << 4)
    rate, kbps = SAMPLE_RATES[version_bits][rate_index], BITRATES[(int(lsf), layer)][bitrate_index - 1]
    frame_bytes = (12 * kbps * 1000 // rate + padding) * 4 if layer == 1 else 144 * kbps * 1000 // rate + padding
    return bytes([0xFF, b1, b2, b3]), dict(layer=layer, lsf=int(lsf), sample_rate=rate, bitrate_kbps=kbps, mode=mode, mode_ext=mode_ext,
                                           crc=crc, padding=padding, channels=1 if mode == 3 else 2, frame_bytes=frame_bytes)


def geometry(h):
    """(rows per subband or None for Layer I, sblimit, bound)"""
    if h["layer"] == 1:
        rows, sblimit = None, 32
    else:
        rows = TABLES[table_name(h["lsf"], h["bitrate_kbps"], h["channels"], h["sample_rate"])]
        sblimit = len(rows)
    bound = min(4 * (h["mode_ext"] + 1), sblimit) if h["mode"] == 1 else sblimit
    return rows, sblimit, bound


def steps_of(h, rows, sb, alloc):
    if not alloc:
        return 0
    return (1 << (alloc + 1)) - 1 if h["layer"] == 1 else ROWS[rows[sb]][1][alloc - 1]


def build_frame(h4, h, alloc, scfsi, scf, codes, allow_overrun=False):
    """alloc[ch][sb]: allocation indices (above the bound channel 0's counts); scfsi[ch][sb] (Layer II); scf[ch][sb][3]: the indices a
    decoder must END UP with (the writer sends what the pattern sends: they must agree with scfsi); codes[g][sb][ch][k]: sample codes
    (Layer I: k = 0 only).  -> (frame bytes, expectation dict)"""
    layer, ch = h["layer"], h["channels"]
    rows, sblimit, bound = geometry(h)
    w = BitWriter()
    w.put(int.from_bytes(h4, "big"), 32)
    if h["crc"]:
        w.put(0xBEEF, 16)  # not verified by anybody
    steps = np.zeros((2, 32), np.int64)
    for sb in range(sblimit):
        for c in range(ch if sb < bound else 1):
            a = int(alloc[c][sb])
            w.put(a, 4 if layer == 1 else ROWS[rows[sb]][0])
            steps[c][sb] = steps_of(h, rows, sb, a)
            if sb >= bound and ch == 2:
                steps[1][sb] = steps[0][sb]
    want_scf = np.zeros((2, 32, 3), np.int64)
    if layer == 1:
        for sb in range(sblimit):
            for c in range(ch):
                if steps[c][sb]:
                    w.put(int(scf[c][sb][0]), 6)
                    want_scf[c][sb][:] = scf[c][sb][0]
    else:
        for sb in range(sblimit):
            for c in range(ch):
                if steps[c][sb]:
                    w.put(int(scfsi[c][sb]), 2)
        for sb in range(sblimit):
            for c in range(ch):
                if not steps[c][sb]:
                    continue
                f, s = [int(x) for x in scf[c][sb]], int(scfsi[c][sb])
                sent, got = {0: ([f[0], f[1], f[2]], f), 1: ([f[0], f[2]], [f[0], f[0], f[2]]), 2: ([f[0]], [f[0]] * 3),
                             3: ([f[0], f[1]], [f[0], f[1], f[1]])}[s]
                for x in sent:
                    w.put(x, 6)
                want_scf[c][sb] = got
    sample_bit = w.n
    for g in range(12):
        for sb in range(sblimit):
            for c in range(ch if sb < bound else 1):
                st = int(steps[c][sb])
                if not st:
                    continue
                cs = [int(x) for x in codes[g][sb][c]]
                if layer == 1:
                    w.put(cs[0], (st + 1).bit_length() - 1)
                elif st in GROUPED_BITS:
                    assert all(0 <= x < st for x in cs)
                    w.put(cs[0] + st * cs[1] + st * st * cs[2], GROUPED_BITS[st])
                else:
                    for x in cs:
                        w.put(x, (st + 1).bit_length() - 1)
    bits = w.n
    assert allow_overrun or bits <= 8 * h["frame_bytes"], (bits, 8 * h["frame_bytes"])
    cls = np.zeros((2, 32), np.int64)
    for c in range(2):
        for sb in range(32):
            st = int(steps[c][sb])
            cls[c][sb] = 0 if not st else ((st + 1).bit_length() - 1 if layer == 1 else class_code(st))
    return w.bytes(h["frame_bytes"]), dict(cls=cls, scf=want_scf, steps=steps, sample_bit=sample_bit, granule_bits=(bits - sample_bit) // 12, bits=bits,
                                           sblimit=sblimit, bound=bound)


def random_frame(rng, layer, lsf, rate_index, bitrate_index, mode, mode_ext=0, crc=False, padding=0, code_mode="random", fill=0.9, scf_floor=0):
    """A frame with a random allocation that uses about `fill` of its bits, random scale factors (all four scfsi patterns) and codes:
    code_mode "random", "zero", "max" or "middle".  The scale-factor indices are drawn from scf_floor ... 63: index 0 is a factor of
    2.0 per subband, and with every subband at that level the decoded PCM leaves +-1 (fine for a float comparison, useless behind
    an s16 output); from 9 on (a factor of 0.25 at the most) no stream of tests/test_mp12_cpu.py's CONFIGS does."""
    h4, h = header(layer, lsf, rate_index, bitrate_index, mode, mode_ext, crc, padding)
    rows, sblimit, bound = geometry(h)
    ch = h["channels"]
    budget = int(fill * (8 * h["frame_bytes"] - 32 - (16 if crc else 0)))
    alloc = np.zeros((2, 32), np.int64)
    used = sum((4 if layer == 1 else ROWS[rows[sb]][0]) * (ch if sb < bound else 1) for sb in range(sblimit))
    for sb in rng.permutation(sblimit):
        for c in range(ch if sb < bound else 1):
            top = 14 if layer == 1 else len(ROWS[rows[sb]][1])
            a = int(rng.integers(0, top + 1))
            st = steps_of(h, rows, sb, a)
            if not st:
                continue
            nb = (st + 1).bit_length() - 1
            per = 12 * (nb if layer == 1 else (GROUPED_BITS[st] if st in GROUPED_BITS else 3 * nb))
            side = (6 if layer == 1 else 2 + 18) * (1 if sb < bound else ch)
            if used + per + side <= budget:
                alloc[c][sb] = a
                used += per + side
    scfsi = rng.integers(0, 4, (2, 32))
    scf = rng.integers(scf_floor, 64, (2, 32, 3))
    codes = np.zeros((12, 32, 2, 3), np.int64)
    for sb in range(sblimit):
        for c in range(ch if sb < bound else 1):
            st = steps_of(h, rows, sb, int(alloc[c][sb]))
            if not st:
                continue
            grouped = layer == 2 and st in GROUPED_BITS
            top = st - 1 if grouped else st  # an ungrouped code has log2(steps + 1) bits: all of them may be set
            codes[:, sb, c, :] = {"random": rng.integers(0, top + 1, (12, 3)), "zero": 0, "max": top, "middle": top // 2}[code_mode]
    frame, want = build_frame(h4, h, alloc, scfsi, scf, codes)
    want["header"] = h
    return frame, want

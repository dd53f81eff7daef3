"""A float64 decoder of MPEG Layer I and II (ISO/IEC 11172-3 2.4.1.5-6, 2.4.3.2-3; 13818-3 2.4.3.1), the checker of
csrc/mp12_bitstream.cpp and csrc/mp12_synth.hip.  Its tables are typed here, independently of csrc/mp12_tables.h; the polyphase
synthesis is oracle/mp3_hybrid.py's (the one Layer III is checked against), the window D the oracle's Table B.3.

Scale factor 2^(1 - i/3): the standard's table ends at index 62; index 63 continues the closed form here as in the product."""
import numpy as np

from oracle import mp3_hybrid, mp3_iso

SAMPLE_RATES = {3: (44100, 48000, 32000), 2: (22050, 24000, 16000)}  # by version bits: MPEG-1, MPEG-2
BITRATES = {  # (lsf, layer) -> kbit/s of index 1 ... 14
    (0, 1): [32 * i for i in range(1, 15)],
    (0, 2): [32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384],
    (1, 1): [32, 48, 56, 64, 80, 96, 112, 128, 144, 160, 176, 192, 224, 256],
    (1, 2): [8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160],
}

# Layer II allocation rows: (width of the allocation field, steps of allocation 1, 2, ...)
ROWS = {
    "A": (4, [3, 7, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 16383, 32767, 65535]),
    "B": (4, [3, 5, 7, 9, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 65535]),
    "C": (3, [3, 5, 7, 9, 15, 31, 65535]),
    "D": (2, [3, 5, 65535]),
    "E": (4, [3, 5, 9, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 16383, 32767]),
    "F": (3, [3, 5, 9, 15, 31, 63, 127]),
    "G": (4, [3, 5, 7, 9, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 16383]),
    "H": (2, [3, 5, 9]),
}
TABLES = {  # name -> the row of every subband below the subband limit
    "B.2a": "AAA" + "B" * 8 + "C" * 12 + "D" * 4,
    "B.2b": "AAA" + "B" * 8 + "C" * 12 + "D" * 7,
    "B.2c": "EE" + "F" * 6,
    "B.2d": "EE" + "F" * 10,
    "LSF": "GGGG" + "F" * 7 + "H" * 19,
}
assert [len(TABLES[k]) for k in ("B.2a", "B.2b", "B.2c", "B.2d", "LSF")] == [27, 30, 8, 12, 30]
GROUPED_BITS = {3: 5, 5: 7, 9: 10}


def table_name(lsf, bitrate_kbps, channels, sample_rate):
    if lsf:
        return "LSF"
    per_channel = bitrate_kbps if channels == 1 else bitrate_kbps // 2
    if per_channel < 56:
        return "B.2d" if sample_rate == 32000 else "B.2c"
    if per_channel >= 96 and sample_rate != 48000:
        return "B.2b"
    return "B.2a"


def class_code(steps):
    """the product's class byte (include/soundkit_amd.h, sk_mpa_frame_record::cls) of a quantiser of `steps` steps in Layer II"""
    return 0x80 | steps if steps in GROUPED_BITS else (steps + 1).bit_length() - 1


def parse_header(b):
    """4 bytes -> dict, or None if they are no Layer I / II header this project decodes"""
    if len(b) < 4 or b[0] != 0xFF or (b[1] & 0xE0) != 0xE0:
        return None
    version, layer_bits = (b[1] >> 3) & 3, (b[1] >> 1) & 3
    if version not in (2, 3) or layer_bits not in (2, 3):
        return None
    layer = 4 - layer_bits
    bi, si = b[2] >> 4, (b[2] >> 2) & 3
    if bi in (0, 15) or si == 3:
        return None
    lsf = int(version == 2)
    rate, kbps, pad = SAMPLE_RATES[version][si], BITRATES[(lsf, layer)][bi - 1], (b[2] >> 1) & 1
    mode = b[3] >> 6
    h = dict(version=2 if lsf else 1, layer=layer, lsf=lsf, crc=not (b[1] & 1), sample_rate=rate, bitrate_kbps=kbps, padding=pad, mode=mode,
             mode_ext=(b[3] >> 4) & 3, channels=1 if mode == 3 else 2)
    h["frame_bytes"] = (12 * kbps * 1000 // rate + pad) * 4 if layer == 1 else 144 * kbps * 1000 // rate + pad
    h["samples_per_channel"] = 384 if layer == 1 else 1152
    return h


def scan(data):
    """[(offset, header)] of a clean stream of back-to-back frames"""
    out, pos = [], 0
    while pos + 4 <= len(data):
        h = parse_header(data[pos:pos + 4])
        if h is None or pos + h["frame_bytes"] > len(data):
            break
        out.append((pos, h))
        pos += h["frame_bytes"]
    return out


class Bits:
    def __init__(self, data, pos=0):
        self.v, self.n, self.pos = int.from_bytes(data, "big"), 8 * len(data), pos

    def get(self, k):
        if k == 0:
            return 0
        end = self.pos + k
        v = (self.v >> (self.n - end)) & ((1 << k) - 1) if end <= self.n else ((self.v << (end - self.n)) & ((1 << k) - 1))
        self.pos = end
        return v


def parse_frame(frame, h, tables=TABLES):
    """One frame -> dict: steps[ch][sb] (0: nothing), scf[ch][sb][3], samples[ch][slot][sb] as float64 in +-1.0 (36 or 12 slots),
    sblimit, bound, sample_bit, granule_bits, bits (the position behind the last sample code).  `tables`: for the negative control."""
    ch, layer = h["channels"], h["layer"]
    if layer == 1:
        sblimit = 32
    else:
        rows = tables[table_name(h["lsf"], h["bitrate_kbps"], ch, h["sample_rate"])]
        sblimit = len(rows)
    bound = min(4 * (h["mode_ext"] + 1), sblimit) if h["mode"] == 1 else sblimit
    b = Bits(frame[:h["frame_bytes"]], 32 + (16 if h["crc"] else 0))
    steps = np.zeros((2, 32), np.int64)
    for sb in range(sblimit):
        for c in range(ch if sb < bound else 1):
            if layer == 1:
                a = b.get(4)
                if a == 15:
                    raise ValueError("forbidden allocation")
                st = (1 << (a + 1)) - 1 if a else 0
            else:
                width, row = ROWS[rows[sb]]
                a = b.get(width)
                st = row[a - 1] if a else 0
            steps[c][sb] = st
            if sb >= bound and ch == 2:
                steps[1][sb] = st
    scf = np.zeros((2, 32, 3), np.int64)
    if layer == 1:
        for sb in range(sblimit):
            for c in range(ch):
                if steps[c][sb]:
                    scf[c][sb][:] = b.get(6)
    else:
        scfsi = np.zeros((2, 32), np.int64)
        for sb in range(sblimit):
            for c in range(ch):
                if steps[c][sb]:
                    scfsi[c][sb] = b.get(2)
        for sb in range(sblimit):
            for c in range(ch):
                if not steps[c][sb]:
                    continue
                s = scfsi[c][sb]
                if s == 0:
                    scf[c][sb] = [b.get(6), b.get(6), b.get(6)]
                elif s == 1:
                    x, y = b.get(6), b.get(6)
                    scf[c][sb] = [x, x, y]
                elif s == 2:
                    scf[c][sb][:] = b.get(6)
                else:
                    x, y = b.get(6), b.get(6)
                    scf[c][sb] = [x, y, y]
    sample_bit = b.pos
    slots = 12 if layer == 1 else 36
    samples = np.zeros((2, slots, 32))
    factor = lambda i: 2.0 ** (1.0 - i / 3.0)
    requant = lambda code, st: (2 * code - (st - 1)) / st
    for g in range(12):
        for sb in range(sblimit):
            for c in range(ch if sb < bound else 1):
                st = int(steps[c][sb])
                if not st:
                    continue
                if layer == 1:
                    codes = [b.get((st + 1).bit_length() - 1)]
                elif st in GROUPED_BITS:
                    w = b.get(GROUPED_BITS[st])
                    codes = [w % st, (w // st) % st, w // (st * st)]
                else:
                    codes = [b.get((st + 1).bit_length() - 1) for _ in range(3)]
                for cc in ((c,) if sb < bound or ch == 1 else (0, 1)):
                    f = factor(int(scf[cc][sb][0 if layer == 1 else g // 4]))
                    for k, code in enumerate(codes):
                        samples[cc][(g if layer == 1 else 3 * g + k)][sb] = f * requant(code, st)
    return dict(steps=steps, scf=scf, samples=samples, sblimit=sblimit, bound=bound, sample_bit=sample_bit,
                granule_bits=(b.pos - sample_bit) // 12, bits=b.pos, slots=slots)


class Decoder:
    """frames in stream order -> interleaved float64 PCM; the polyphase FIFO is carried from frame to frame"""

    def __init__(self):
        self.chans = [mp3_hybrid.Channel(), mp3_hybrid.Channel()]
        self.window = np.asarray(mp3_iso.tables()["window"], np.float64)

    def frame(self, frame, h):
        p = parse_frame(frame, h)
        if p["bits"] > 8 * h["frame_bytes"]:
            raise ValueError("samples end beyond the frame")
        out = np.zeros((p["slots"] * 32, h["channels"]))
        for c in range(h["channels"]):
            for s in range(p["slots"]):
                out[32 * s:32 * s + 32, c] = self.chans[c].polyphase(p["samples"][c][s], self.window)
        return out

    def stream(self, data):
        return np.concatenate([self.frame(data[off:off + h["frame_bytes"]], h) for off, h in scan(data)])

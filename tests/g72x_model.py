"""Plain-Python models of the telephony decoders: G.711, G.722 (64 kbit/s) and G.726 (16 / 24 / 32 / 40 kbit/s, both packings).

The G.726 model restates the reference's `soundkit-g726` (itself the classic public G.72x arithmetic); the G.722 model is the ITU-T
decoder in its common fixed-point form with both scale factors starting at 0 (profiles/telephony.md says what pins that).  Both are
pinned by fixture = twin in tests/test_g72x_cpu.py.  The encoders exist to write test streams: the G.726 one is the reference's, the
G.722 one is an analysis-by-synthesis search that keeps in step with the model decoder and is held to no recording.

States are plain lists of ints in the order of `sk_g726_state` / `sk_g722_state` (include/soundkit_amd.h), so a GPU test can compare
a returned state word for word.
"""
import numpy as np

from aiff_model import ALAW_TABLE, ULAW_TABLE

ULAW, ALAW, G722, G726 = 0, 1, 2, 3  # enum sk_g72x_codec
LEFT, RIGHT = 0, 1  # enum sk_g726_packing
MAX_SEND_SAMPLES = 262144


def g711_decode(data, law):
    table = ULAW_TABLE if law == ULAW else ALAW_TABLE
    return np.asarray(table, dtype=np.int16)[np.frombuffer(bytes(data), dtype=np.uint8)]


# ---- G.726 -------------------------------------------------------------------------------------------------------------------------

G726_BITS = {16000: 2, 24000: 3, 32000: 4, 40000: 5}
G726_GROUP_BYTES = {16000: 1, 24000: 3, 32000: 1, 40000: 5}
G726_GROUP_SAMPLES = {16000: 4, 24000: 8, 32000: 2, 40000: 8}

_QTAB = {
    16000: [261],
    24000: [8, 218, 331],
    32000: [-124, 80, 178, 246, 300, 349, 400],
    40000: [-122, -16, 68, 139, 198, 250, 298, 339, 378, 413, 445, 475, 502, 528, 553],
}
_DQLN = {
    16000: [116, 365, 365, 116],
    24000: [-2048, 135, 273, 373, 373, 273, 135, -2048],
    32000: [-2048, 4, 135, 213, 273, 323, 373, 425, 425, 373, 323, 273, 213, 135, 4, -2048],
    40000: [-2048, -66, 28, 104, 169, 224, 274, 318, 358, 395, 429, 459, 488, 514, 539, 566,
            566, 539, 514, 488, 459, 429, 395, 358, 318, 274, 224, 169, 104, 28, -66, -2048],
}
_WI = {
    16000: [-22, 439, 439, -22],
    24000: [-4, 30, 137, 582, 582, 137, 30, -4],
    32000: [-12, 18, 41, 64, 112, 198, 355, 1122, 1122, 355, 198, 112, 64, 41, 18, -12],
    40000: [14, 14, 24, 39, 40, 41, 58, 100, 141, 179, 219, 280, 358, 440, 529, 696,
            696, 529, 440, 358, 280, 219, 179, 141, 100, 58, 41, 40, 39, 24, 14, 14],
}
_FI = {
    16000: [0, 0xE00, 0xE00, 0],
    24000: [0, 0x200, 0x400, 0xE00, 0xE00, 0x400, 0x200, 0],
    32000: [0, 0, 0, 0x200, 0x200, 0x200, 0x600, 0xE00, 0xE00, 0x600, 0x200, 0x200, 0x200, 0, 0, 0],
    40000: [0, 0, 0, 0, 0, 0x200, 0x200, 0x200, 0x200, 0x200, 0x400, 0x600, 0x800, 0xA00, 0xC00, 0xC00,
            0xC00, 0xC00, 0xA00, 0x800, 0x600, 0x400, 0x200, 0x200, 0x200, 0x200, 0x200, 0, 0, 0, 0, 0],
}


def quan(value, table):
    """Index of the first threshold above `value`, or the table's length."""
    for i, t in enumerate(table):
        if value < t:
            return i
    return len(table)


_POWER2 = [1 << i for i in range(15)]


def _ilog(value):
    """quan over the powers of two up to 2^14: the bit length, capped at 15."""
    return quan(value, _POWER2)


def fmult(an, srn):
    anmag = an if an > 0 else (-an) & 0x1FFF
    anexp = _ilog(anmag) - 6
    if anmag == 0:
        anmant = 32
    elif anexp >= 0:
        anmant = anmag >> anexp
    else:
        anmant = anmag << -anexp
    wanexp = anexp + ((srn >> 6) & 0xF) - 13
    wanmant = (anmant * (srn & 0x3F) + 0x30) >> 4
    ret = ((wanmant << wanexp) & 0x7FFF) if wanexp >= 0 else (wanmant >> -wanexp)
    return -ret if (an ^ srn) < 0 else ret


def reconstruct(sign, dqln, y):
    dql = dqln + (y >> 2)
    if dql < 0:
        return -0x8000 if sign else 0
    dex = (dql >> 7) & 15
    dqt = 128 + (dql & 127)
    dq = (dqt << 7) >> (14 - dex)
    return dq - 0x8000 if sign else dq


def _float_form(mag):
    exp = _ilog(mag)
    return (exp << 6) + ((mag << 6) >> exp)


class G726Core:
    """The adaptive predictor and quantiser scale of one G.726 stream."""

    def __init__(self, words=None):
        if words is None:
            self.yl, self.yu, self.dms, self.dml, self.ap = 34816, 544, 0, 0, 0
            self.a, self.b, self.pk, self.dq, self.sr, self.td = [0, 0], [0] * 6, [0, 0], [32] * 6, [32, 32], 0
        else:
            w = [int(v) for v in words]
            self.yl, self.yu, self.dms, self.dml, self.ap = w[0:5]
            self.a, self.b, self.pk, self.dq, self.sr, self.td = w[5:7], w[7:13], w[13:15], w[15:21], w[21:23], w[23]

    def words(self):
        """The 24 int32 of sk_g726_state."""
        return [self.yl, self.yu, self.dms, self.dml, self.ap] + self.a + self.b + self.pk + self.dq + self.sr + [self.td]

    def predictor_zero(self):
        return sum(fmult(b >> 2, dq) for b, dq in zip(self.b, self.dq))

    def predictor_pole(self):
        return fmult(self.a[1] >> 2, self.sr[1]) + fmult(self.a[0] >> 2, self.sr[0])

    def step_size(self):
        if self.ap >= 256:
            return self.yu
        y = self.yl >> 6
        dif = self.yu - y
        al = self.ap >> 2
        if dif > 0:
            return y + ((dif * al) >> 6)
        if dif < 0:
            return y + ((dif * al + 0x3F) >> 6)
        return y

    def decode_code(self, code, rate):
        i = code & ((1 << G726_BITS[rate]) - 1)
        sezi = self.predictor_zero()
        sez = sezi >> 1
        se = (sezi + self.predictor_pole()) >> 1
        y = self.step_size()
        dq = reconstruct(bool(i >> (G726_BITS[rate] - 1)), _DQLN[rate][i], y)
        mask = 0x7FFF if rate == 40000 else 0x3FFF
        sr = se - (dq & mask) if dq < 0 else se + dq
        self.update(y, _WI[rate][i] << 5, _FI[rate][i], dq, sr, sr - se + sez, rate)
        return max(-32768, min(32767, sr << 2))

    def encode_sample(self, sample, rate):
        sl = sample >> 2
        sezi = self.predictor_zero()
        sez = sezi >> 1
        se = (sezi + self.predictor_pole()) >> 1
        d = sl - se
        y = self.step_size()
        mask_code = (1 << G726_BITS[rate]) - 1
        dqm = abs(d)
        exp = _ilog(dqm >> 1)
        dl = (exp << 7) + (((dqm << 7) >> exp) & 0x7F)
        q = quan(dl - (y >> 2), _QTAB[rate])
        i = mask_code - q if d < 0 else (mask_code if q == 0 else q)
        dq = reconstruct(bool(i >> (G726_BITS[rate] - 1)), _DQLN[rate][i], y)
        mask = 0x7FFF if rate == 40000 else 0x3FFF
        sr = se - (dq & mask) if dq < 0 else se + dq
        self.update(y, _WI[rate][i] << 5, _FI[rate][i], dq, sr, sr + sez - se, rate)
        return i

    def update(self, y, wi, fi, dq, sr, dqsez, rate):
        pk0 = 1 if dqsez < 0 else 0
        mag = dq & 0x7FFF
        ylint = self.yl >> 15
        ylfrac = (self.yl >> 10) & 0x1F
        thr1 = (32 + ylfrac) << ylint
        thr2 = (31 << 10) if ylint > 9 else thr1
        dqthr = (thr2 + (thr2 >> 1)) >> 1
        tr = self.td != 0 and mag > dqthr

        self.yu = max(544, min(5120, y + ((wi - y) >> 5)))
        self.yl += self.yu + ((-self.yl) >> 6)

        if tr:
            a2p = 0
            self.a = [0, 0]
            self.b = [0] * 6
        else:
            pks1 = pk0 ^ self.pk[0]
            a2p = self.a[1] - (self.a[1] >> 7)
            if dqsez != 0:
                fa1 = self.a[0] if pks1 else -self.a[0]
                if fa1 < -8191:
                    a2p -= 0x100
                elif fa1 > 8191:
                    a2p += 0xFF
                else:
                    a2p += fa1 >> 5
                if pk0 ^ self.pk[1]:
                    if a2p <= -12160:
                        a2p = -12288
                    elif a2p >= 12416:
                        a2p = 12288
                    else:
                        a2p -= 0x80
                elif a2p <= -12416:
                    a2p = -12288
                elif a2p >= 12160:
                    a2p = 12288
                else:
                    a2p += 0x80
            self.a[1] = a2p
            self.a[0] -= self.a[0] >> 8
            if dqsez != 0:
                self.a[0] += 192 if pks1 == 0 else -192
            a1ul = 15360 - a2p
            self.a[0] = max(-a1ul, min(a1ul, self.a[0]))
            shift = 9 if rate == 40000 else 8
            for k in range(6):
                self.b[k] -= self.b[k] >> shift
                if mag != 0:
                    self.b[k] += 128 if (dq ^ self.dq[k]) >= 0 else -128

        self.dq[1:] = self.dq[:5]
        if mag == 0:
            self.dq[0] = 0x20 if dq >= 0 else -0x3E0
        else:
            self.dq[0] = _float_form(mag) if dq >= 0 else _float_form(mag) - 0x400

        self.sr[1] = self.sr[0]
        if sr == 0:
            self.sr[0] = 0x20
        elif sr > 0:
            self.sr[0] = _float_form(sr)
        elif sr > -32768:
            self.sr[0] = _float_form(-sr) - 0x400
        else:
            self.sr[0] = -0x3E0

        self.pk = [pk0, self.pk[0]]
        self.td = 0 if tr else (1 if a2p < -11776 else 0)
        self.dms += (fi - self.dms) >> 5
        self.dml += ((fi << 2) - self.dml) >> 7
        if tr:
            self.ap = 256
        elif y < 1536 or self.td != 0 or abs((self.dms << 2) - self.dml) >= (self.dml >> 3):
            self.ap += (0x200 - self.ap) >> 4
        else:
            self.ap += (-self.ap) >> 4


def unpack_code_group(group, bits, packing):
    """One group of bytes into its codes: LEFT takes the stream MSB first, RIGHT LSB first."""
    n = len(group) * 8 // bits
    if packing == LEFT:
        word = int.from_bytes(bytes(group), "big")
        total = len(group) * 8
        return [(word >> (total - bits * (k + 1))) & ((1 << bits) - 1) for k in range(n)]
    word = int.from_bytes(bytes(group), "little")
    return [(word >> (bits * k)) & ((1 << bits) - 1) for k in range(n)]


def pack_code_group(codes, bits, packing):
    nbytes = len(codes) * bits // 8
    word = 0
    if packing == LEFT:
        for c in codes:
            word = (word << bits) | c
        return word.to_bytes(nbytes, "big")
    for k, c in enumerate(codes):
        word |= c << (bits * k)
    return word.to_bytes(nbytes, "little")


class G726Decoder:
    """`G726Decoder::decode_i16` with its pending partial group, and `flush`."""

    def __init__(self, rate=32000, packing=LEFT):
        self.rate, self.packing, self.core, self.pending = rate, packing, G726Core(), b""

    def decode(self, data):
        gb, bits = G726_GROUP_BYTES[self.rate], G726_BITS[self.rate]
        data = self.pending + bytes(data)
        whole = len(data) // gb * gb
        out = []
        for g in range(0, whole, gb):
            for code in unpack_code_group(data[g:g + gb], bits, self.packing):
                out.append(self.core.decode_code(code, self.rate))
        self.pending = data[whole:]
        return np.asarray(out, dtype=np.int16)

    def flush(self):
        if self.pending:
            raise ValueError("G.726 stream ended with %d trailing partial-packet byte(s)" % len(self.pending))


def g726_encode(samples, rate=32000, packing=LEFT, core=None):
    """Whole groups only: the samples past the last whole group are dropped."""
    core = core or G726Core()
    gs, bits = G726_GROUP_SAMPLES[rate], G726_BITS[rate]
    out = bytearray()
    samples = [int(s) for s in samples]
    for g in range(0, len(samples) // gs * gs, gs):
        out += pack_code_group([core.encode_sample(s, rate) for s in samples[g:g + gs]], bits, packing)
    return bytes(out)


# ---- G.722 -------------------------------------------------------------------------------------------------------------------------

_QM2 = [-7408, -1616, 7408, 1616]
_QM4 = [0, -20456, -12896, -8968, -6288, -4240, -2584, -1200, 20456, 12896, 8968, 6288, 4240, 2584, 1200, 0]
_QM6 = [-136, -136, -136, -136, -24808, -21904, -19008, -16704, -14984, -13512, -12280, -11192, -10232, -9360, -8576, -7856,
        -7192, -6576, -6000, -5456, -4944, -4464, -4008, -3576, -3168, -2776, -2400, -2032, -1688, -1360, -1040, -728,
        24808, 21904, 19008, 16704, 14984, 13512, 12280, 11192, 10232, 9360, 8576, 7856, 7192, 6576, 6000, 5456,
        4944, 4464, 4008, 3576, 3168, 2776, 2400, 2032, 1688, 1360, 1040, 728, 432, 136, -432, -136]
_WL = [-60, -30, 58, 172, 334, 538, 1198, 3042]
_RL42 = [0, 7, 6, 5, 4, 3, 2, 1, 7, 6, 5, 4, 3, 2, 1, 0]
_ILB = [2048, 2093, 2139, 2186, 2233, 2282, 2332, 2383, 2435, 2489, 2543, 2599, 2656, 2714, 2774, 2834,
        2896, 2960, 3025, 3091, 3158, 3228, 3298, 3371, 3444, 3520, 3597, 3676, 3756, 3838, 3922, 4008]
_WH = [0, -214, 798]
_RH2 = [2, 1, 2, 1]
_QMF = [3, -11, 12, 32, -210, 951, 3876, -805, 362, -156, 53, -11]


def _sat16(v):
    return max(-32768, min(32767, v))


def _scale(nb, k):
    w = k - (nb >> 11)
    v = _ILB[(nb >> 6) & 31]
    return (v << -w) if w < 0 else (v >> w)


class G722Band:
    """One band's predictor: s, sz, r[2], p[2], a[2], b[6], d[6], nb, det -- 22 words."""

    def __init__(self, words=None):
        w = [0] * 22 if words is None else [int(v) for v in words]
        self.s, self.sz, self.r, self.p, self.a, self.b, self.d, self.nb, self.det = w[0], w[1], w[2:4], w[4:6], w[6:8], w[8:14], w[14:20], w[20], w[21]

    def words(self):
        return [self.s, self.sz] + self.r + self.p + self.a + self.b + self.d + [self.nb, self.det]

    def block4(self, d):
        r0 = _sat16(self.s + d)  # RECONS
        p0 = _sat16(self.sz + d)  # PARREC
        # UPPOL2
        wd1 = _sat16(self.a[0] << 2)
        wd2 = -wd1 if (p0 < 0) == (self.p[0] < 0) else wd1
        wd2 = min(wd2, 32767)
        wd3 = (128 if (p0 < 0) == (self.p[1] < 0) else -128) + (wd2 >> 7) + ((self.a[1] * 32512) >> 15)
        a2 = max(-12288, min(12288, wd3))
        # UPPOL1
        a1 = _sat16((192 if (p0 < 0) == (self.p[0] < 0) else -192) + ((self.a[0] * 32640) >> 15))
        lim = _sat16(15360 - a2)
        a1 = max(-lim, min(lim, a1))
        # UPZERO
        step = 0 if d == 0 else 128
        self.b = [_sat16((step if (dk < 0) == (d < 0) else -step) + ((bk * 32640) >> 15)) for bk, dk in zip(self.b, self.d)]
        # DELAYA
        self.d = [d] + self.d[:5]
        self.r = [r0, self.r[0]]
        self.p = [p0, self.p[0]]
        self.a = [a1, a2]
        # FILTEP, FILTEZ, PREDIC
        sp = _sat16(((a1 * _sat16(2 * self.r[0])) >> 15) + ((a2 * _sat16(2 * self.r[1])) >> 15))
        self.sz = _sat16(sum((bk * _sat16(2 * dk)) >> 15 for bk, dk in zip(self.b, self.d)))
        self.s = _sat16(sp + self.sz)


class G722Decoder:
    """64 kbit/s, two samples per byte, nothing buffered between calls."""

    def __init__(self, words=None):
        if words is None:
            self.band, self.x = [G722Band(), G722Band()], [0] * 22
        else:
            w = [int(v) for v in words]
            self.band, self.x = [G722Band(w[0:22]), G722Band(w[22:44])], w[44:66]

    def words(self):
        """The 66 int32 of sk_g722_state."""
        return self.band[0].words() + self.band[1].words() + list(self.x)

    def bands(self, code):
        """One byte through both ADPCM bands: (rlow, rhigh)."""
        lo, hi = self.band
        ilow, ihigh = code & 63, code >> 6
        rlow = max(-16384, min(16383, lo.s + ((lo.det * _QM6[ilow]) >> 15)))
        dlowt = (lo.det * _QM4[ilow >> 2]) >> 15
        lo.nb = max(0, min(18432, ((lo.nb * 127) >> 7) + _WL[_RL42[ilow >> 2]]))
        lo.det = _scale(lo.nb, 8) << 2
        lo.block4(dlowt)
        dhigh = (hi.det * _QM2[ihigh]) >> 15
        rhigh = max(-16384, min(16383, dhigh + hi.s))
        hi.nb = max(0, min(22528, ((hi.nb * 127) >> 7) + _WH[_RH2[ihigh]]))
        hi.det = _scale(hi.nb, 10) << 2
        hi.block4(dhigh)
        return rlow, rhigh

    def decode(self, data):
        out = []
        for code in bytes(data):
            rlow, rhigh = self.bands(code)
            x = self.x + [rlow + rhigh, rlow - rhigh]
            x2 = sum(x[2 * i] * _QMF[i] for i in range(12))
            x1 = sum(x[2 * i + 1] * _QMF[11 - i] for i in range(12))
            out += [_sat16(x1 >> 11), _sat16(x2 >> 11)]
            self.x = x[2:]
        return np.asarray(out, dtype=np.int16)


def g722_encode(samples, decoder=None):
    """Pairs of 16 kHz samples to bytes by analysis-by-synthesis against the model decoder: sum / difference split, the nearest
    reconstruction per band.  `decoder` (a G722Decoder) is advanced exactly as decoding the returned bytes would advance it."""
    dec = decoder or G722Decoder()
    out = bytearray()
    samples = [int(s) for s in samples]
    for k in range(0, len(samples) // 2 * 2, 2):
        xlow = max(-16384, min(16383, (samples[k] + samples[k + 1]) >> 1))
        xhigh = max(-16384, min(16383, (samples[k] - samples[k + 1]) >> 1))
        lo, hi = dec.band
        dl, dh = max(lo.det, 32), max(hi.det, 8)  # a zero scale factor tells no two codes apart
        ilow = min(range(4, 64), key=lambda i: abs(xlow - lo.s - ((dl * _QM6[i]) >> 15)))
        ihigh = min(range(4), key=lambda i: abs(xhigh - hi.s - ((dh * _QM2[i]) >> 15)))
        code = ilow | (ihigh << 6)
        out.append(code)
        rlow, rhigh = dec.bands(code)
        dec.x = (dec.x + [rlow + rhigh, rlow - rhigh])[2:]
    return bytes(out)

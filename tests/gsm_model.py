"""GSM 06.10 full-rate (RPE-LTP, 13 kbit/s) in plain Python integers: the decoder the device kernels (csrc/gsm_decode.hip) are held to,
the reference's two framings, its streaming wrapper with its texts, and an encoder-free stream builder that packs any 76 parameters
into a frame.  `word` is 16-bit signed; add / sub saturate; mult_r rounds; shifts of negatives are arithmetic.

The decoder counts what the tests need to know they reached: saturating adds and subtracts, Nc outside 40 ... 120, frames whose
output clipped.
"""
import numpy as np

STANDARD, MICROSOFT = 0, 1
FRAME_BYTES, MS_PACKET_BYTES, FRAME_SAMPLES, FRAME_BITS = 33, 65, 160, 260
PACKET_BYTES = {STANDARD: FRAME_BYTES, MICROSOFT: MS_PACKET_BYTES}
PACKET_SAMPLES = {STANDARD: FRAME_SAMPLES, MICROSOFT: 2 * FRAME_SAMPLES}
MAX_SEND_SAMPLES = 262144

FAC = (18431, 20479, 22527, 24575, 26623, 28671, 30719, 32767)
QLB = (3277, 11469, 21299, 32767)
LAR_B = (0, 0, 2048, -2560, 94, -1792, -341, -1144)
LAR_MIC = (-32, -32, -16, -16, -8, -8, -4, -4)
LAR_INVA = (13107, 13107, 13107, 13107, 19223, 17476, 31454, 29708)
LAR_BITS = (6, 6, 5, 5, 4, 4, 3, 3)
# the 76 parameters in frame order, with their widths: LARc[8], then per subframe Nc, bc, Mc, xmaxc, xMc[13]
PARAM_BITS = LAR_BITS + ((7, 2, 2, 6) + (3,) * 13) * 4
assert len(PARAM_BITS) == 76 and sum(PARAM_BITS) == FRAME_BITS


class Counters:
    def __init__(self):
        self.sat_add = self.sat_sub = self.nc_out_of_range = self.clipped_frames = 0


def word(v):
    """truncation to 16 bits, signed"""
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def mult_r(a, b):
    return word((a * b + 16384) >> 15)


class GsmCore:
    """The carry of a stream (sk_gsm_state) and one frame's decode."""

    def __init__(self):
        self.dp = [0] * 120   # the long-term history, oldest first
        self.v = [0] * 8      # the lattice memory v[0..7] (v[8] is written and never read)
        self.msr = 0
        self.nrp = 40
        self.larpp = [0] * 8  # the previous frame's decoded LARpp
        self.count = Counters()

    def words(self):
        return list(self.dp) + list(self.v) + [self.msr, self.nrp] + list(self.larpp)

    def add(self, a, b):
        s = a + b
        if s > 32767 or s < -32768:
            self.count.sat_add += 1
            return 32767 if s > 0 else -32768
        return s

    def sub(self, a, b):
        s = a - b
        if s > 32767 or s < -32768:
            self.count.sat_sub += 1
            return 32767 if s > 0 else -32768
        return s

    def excite(self, nc, bc, mc, xmaxc, xmc):
        """RPE decoding and long-term synthesis of one subframe -> its 40 wt"""
        exp = (xmaxc >> 3) - 1 if xmaxc > 15 else 0
        mant = xmaxc - (exp << 3)
        if mant == 0:
            exp, mant = -4, 7
        else:
            while mant <= 7:
                mant = mant << 1 | 1
                exp -= 1
            mant -= 8
        t1, t2 = FAC[mant], 6 - exp
        t3 = (1 << (t2 - 1)) if t2 > 0 else 0
        erp = [0] * 40
        for i in range(13):
            t = word(((xmc[i] << 1) - 7) << 12)
            erp[mc + 3 * i] = self.add(mult_r(t1, t), t3) >> t2
        if nc < 40 or nc > 120:
            self.count.nc_out_of_range += 1
            nr = self.nrp
        else:
            nr = nc
        self.nrp = nr
        brp = QLB[bc]
        drp = [self.add(erp[k], mult_r(brp, self.dp[120 + k - nr])) for k in range(40)]  # nr >= 40: all from earlier subframes
        self.dp = self.dp[40:] + drp
        return drp

    def lar_decode(self, larc):
        out = []
        for i in range(8):
            t = word(self.add(larc[i], LAR_MIC[i]) << 10)
            t = self.sub(t, LAR_B[i] << 1)
            t = mult_r(LAR_INVA[i], t)
            out.append(self.add(t, t))
        return out

    def to_rp(self, larp):
        out = []
        for x in larp:
            t = 32767 if x == -32768 else abs(x)
            t = t << 1 if t < 11059 else (t + 11059 if t < 20070 else self.add(t >> 2, 26112))
            assert t < 32768  # the lattice's MIN_WORD x MIN_WORD guard is unreachable
            out.append(-t if x < 0 else t)
        return out

    def frame(self, params):
        """76 parameters -> 160 samples"""
        larc = params[:8]
        wt = []
        for j in range(4):
            nc, bc, mc, xmaxc = params[8 + 17 * j:12 + 17 * j]
            wt += self.excite(nc, bc, mc, xmaxc, params[12 + 17 * j:25 + 17 * j])
        p, c = self.larpp, self.lar_decode(larc)
        segs = ((0, 13, [self.add(self.add(a >> 2, b >> 2), a >> 1) for a, b in zip(p, c)]),
                (13, 27, [self.add(a >> 1, b >> 1) for a, b in zip(p, c)]),
                (27, 40, [self.add(self.add(a >> 2, b >> 2), b >> 1) for a, b in zip(p, c)]),
                (40, 160, c))
        self.larpp = c
        out, clipped = [], False
        for lo, hi, larp in segs:
            rrp = self.to_rp(larp)
            for k in range(lo, hi):
                sri = wt[k]
                v = self.v + [0]
                for i in range(7, -1, -1):
                    sri = self.sub(sri, mult_r(rrp[i], v[i]))
                    v[i + 1] = self.add(v[i], mult_r(rrp[i], sri))
                v[0] = sri
                self.v = v[:8]
                self.msr = self.add(sri, mult_r(self.msr, 28180))
                d = self.msr + self.msr
                clipped |= d > 32767 or d < -32768
                out.append(word(self.add(self.msr, self.msr) & 0xFFF8))
        self.count.clipped_frames += clipped
        return out


def bits_at(data, bit, n):
    """n bits of data, MSB first, from bit index `bit`"""
    v = 0
    for k in range(bit, bit + n):
        v = v << 1 | ((data[k >> 3] >> (7 - (k & 7))) & 1)
    return v


def frame_params(data, bit):
    """the 76 parameters of the frame whose 260 bits begin at bit index `bit`"""
    out = []
    for n in PARAM_BITS:
        out.append(bits_at(data, bit, n))
        bit += n
    return out


def params_bits(params):
    """76 parameters -> their 260 bits as a list"""
    assert len(params) == 76
    bits = []
    for v, n in zip(params, PARAM_BITS):
        assert 0 <= v < (1 << n)
        bits += [(v >> (n - 1 - k)) & 1 for k in range(n)]
    return bits


def pack_bits(bits):
    bits = list(bits) + [0] * (-len(bits) % 8)
    return bytes(sum(b << (7 - k) for k, b in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))


def build_stream(frames, variant=STANDARD):
    """The stream builder: a list of 76-parameter lists -> the stream's bytes.  Standard: 0xD, then the 260 bits.  Microsoft: two runs
    of 260 bits, MSB first, in 65 bytes (an even number of frames)."""
    if variant == STANDARD:
        return b"".join(pack_bits([1, 1, 0, 1] + params_bits(p)) for p in frames)
    assert len(frames) % 2 == 0
    return b"".join(pack_bits(params_bits(frames[i]) + params_bits(frames[i + 1])) for i in range(0, len(frames), 2))


def standard_to_microsoft(data):
    """a standard stream of an even number of frames in the Microsoft framing (the reference's pack_ms_pair)"""
    assert len(data) % (2 * FRAME_BYTES) == 0
    return build_stream([frame_params(data, 8 * at + 4) for at in range(0, len(data), FRAME_BYTES)], MICROSOFT)


def params_of(var):
    """(packet bytes, first frame's bit, bits from one frame to the next): Microsoft packets are 2 x 260 bits with no gap"""
    return (FRAME_BYTES, 4, 8 * FRAME_BYTES) if var == STANDARD else (MS_PACKET_BYTES, 0, FRAME_BITS)


def decode_packets(core, data, variant=STANDARD):
    """whole packets -> samples; a standard frame without the magic nibble: ValueError, as libgsm's -1"""
    packet, base, stride = params_of(variant)
    assert len(data) % packet == 0
    n_frames = len(data) // packet * (PACKET_SAMPLES[variant] // FRAME_SAMPLES)
    if variant == STANDARD:
        for at in range(0, len(data), FRAME_BYTES):
            if data[at] >> 4 != 0xD:
                raise ValueError("GSM decoder rejected frame")
    out = []
    for f in range(n_frames):
        out += core.frame(frame_params(data, base + f * stride))
    return np.array(out, np.int16)


class GsmDecoder:
    """The reference's GsmDecoder: holds a partial packet back, checks the output's room before anything else."""

    def __init__(self, variant=STANDARD):
        self.variant = variant
        self.core = GsmCore()
        self.pending = b""

    def decode(self, data, out_cap=MAX_SEND_SAMPLES):
        packet = PACKET_BYTES[self.variant]
        total = self.pending + bytes(data)
        whole = len(total) // packet * packet
        need = whole // packet * PACKET_SAMPLES[self.variant]
        if need > out_cap:
            raise ValueError("Output buffer too small for GSM decode: need %d, have %d" % (need, out_cap))
        out = decode_packets(self.core, total[:whole], self.variant)
        self.pending = total[whole:]
        return out

    def flush(self):
        if self.pending:
            raise ValueError("GSM stream ended with %d trailing partial-frame byte(s)" % len(self.pending))


def random_frames(seed, n):
    """n frames of random parameters"""
    rng = np.random.default_rng(seed)
    return [[int(rng.integers(0, 1 << b)) for b in PARAM_BITS] for _ in range(n)]


def make_params(larc=(0,) * 8, nc=(40,) * 4, bc=(0,) * 4, mc=(0,) * 4, xmaxc=(0,) * 4, xmc=None):
    """a frame's 76 parameters from its parts; xmc: 4 x 13 values (default: a fixed pattern)"""
    p = list(larc)
    for j in range(4):
        x = xmc[j] if xmc is not None else [(3 * i + 5 * j + 1) % 8 for i in range(13)]
        p += [nc[j], bc[j], mc[j], xmaxc[j]] + list(x)
    return p

"""Writes FLAC frames and streams (RFC 9639) from explicit per-subframe choices.  A writer, not an encoder: nothing is searched for;
the caller says which subframe type, order, coefficients, partition order and Rice parameters to use and gets exactly those bits.

A subframe spec is a dict:
    {"type": "constant" | "verbatim" | "fixed" | "lpc", "wasted": 0,
     "order": n,                                    fixed: 0 ... 4, lpc: 1 ... 32
     "precision": p, "shift": s, "coefs": [...],    lpc; coefs[j] multiplies the sample j + 1 back
     "method": 0 | 1,                               4- or 5-bit Rice parameters
     "porder": o, "params": [k | ("esc", width), ...]}   one entry per partition (a single value is repeated); "auto": 5-bit
                                                    parameters that keep the unary runs short
Raw overrides for damaged frames: "raw_type" (the 6-bit type field), "pad_bit", "precision_code", "raw_shift", and
"short_partitions" for a partition layout that does not add up to the block."""
import hashlib

from flac_model import FIXED, crc8, crc16


class BitWriter:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, bits):
        if bits:
            self.v = (self.v << bits) | (value & ((1 << bits) - 1))
            self.n += bits

    def unary(self, zeros):
        self.put(1, zeros + 1)

    def pad(self):
        self.put(0, -self.n % 8)

    def bytes(self):
        assert self.n % 8 == 0
        return self.v.to_bytes(self.n // 8, "big")


def coded_number(n):
    if n < 0x80:
        return bytes([n])
    for extra in range(1, 7):
        if n < 1 << (6 * extra + 6 - extra):
            lead = (0xFF << (7 - extra)) & 0xFF
            out = [lead | (n >> (6 * extra))]
            return bytes(out + [0x80 | ((n >> (6 * k)) & 0x3F) for k in range(extra - 1, -1, -1)])
    raise ValueError(n)


BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
DEPTH_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}


def header(block, rate, bits, assignment, number, variable=False, bs_code=None, rate_code=None, depth_code=None, reserved_bit=0, sync_reserved=0):
    if bs_code is None:
        bs_code = BS_CODES.get(block) or (6 if block <= 256 else 7)
    if rate_code is None:
        rate_code = RATE_CODES.get(rate)
        if rate_code is None:
            rate_code = 12 if rate % 1000 == 0 and rate < 256000 else 13 if rate < 65536 else 14
    if depth_code is None:
        depth_code = DEPTH_CODES.get(bits, 0)
    h = bytearray([0xFF, 0xF8 | (sync_reserved << 1) | (1 if variable else 0), (bs_code << 4) | rate_code, (assignment << 4) | (depth_code << 1) | reserved_bit])
    h += coded_number(number)
    if bs_code == 6:
        h += bytes([block - 1])
    elif bs_code == 7:
        h += (block - 1).to_bytes(2, "big")
    if rate_code == 12:
        h += bytes([rate // 1000])
    elif rate_code == 13:
        h += rate.to_bytes(2, "big")
    elif rate_code == 14:
        h += (rate // 10).to_bytes(2, "big")
    return bytes(h) + bytes([crc8(h)])


def put_subframe(w, samples, bps, spec):
    block, wasted = len(samples), spec.get("wasted", 0)
    kind = spec["type"]
    order = spec.get("order", 0)
    code = {"constant": 0, "verbatim": 1, "fixed": 8 + order, "lpc": 31 + order}[kind]
    w.put(spec.get("pad_bit", 0), 1)
    w.put(spec.get("raw_type", code), 6)
    w.put(1 if wasted else 0, 1)
    if wasted:
        w.unary(wasted - 1)
        assert all(v % (1 << wasted) == 0 for v in samples), "the samples do not have that many wasted bits"
        samples = [v >> wasted for v in samples]
        bps -= wasted
    assert all(-(1 << (bps - 1)) <= v < (1 << (bps - 1)) for v in samples), "a sample does not fit its subframe's width"
    if kind == "constant":
        assert len(set(samples)) == 1
        w.put(samples[0], bps)
        return
    if kind == "verbatim":
        for v in samples:
            w.put(v, bps)
        return
    for v in samples[:order]:
        w.put(v, bps)
    if kind == "lpc":
        precision, shift, coefs = spec["precision"], spec["shift"], spec["coefs"]
        assert len(coefs) == order and all(-(1 << (precision - 1)) <= c < (1 << (precision - 1)) for c in coefs)
        w.put(spec.get("precision_code", precision - 1), 4)
        w.put(spec.get("raw_shift", shift), 5)
        for c in coefs:
            w.put(c, precision)
    else:
        shift, coefs = 0, FIXED[order]
    res = [samples[i] - (sum(c * samples[i - 1 - j] for j, c in enumerate(coefs)) >> shift) for i in range(order, block)]
    assert all(-(1 << 31) < e < (1 << 31) for e in res), "a residual does not fit 32 bits"
    method, porder = spec.get("method", 0), spec.get("porder", 0)
    params = spec.get("params", 4)
    if params == "auto":  # 5-bit parameters, each partition's large enough for short unary runs
        method, per, params = 1, block >> porder, []
        for p in range(1 << porder):
            part = res[max(p * per - order, 0):(p + 1) * per - order]
            params.append(min(30, max(0, max([abs(e) for e in part] + [0]).bit_length() - 1)))
    if not isinstance(params, list):
        params = [params] * (1 << porder)
    assert len(params) == 1 << porder
    w.put(method, 2)
    w.put(porder, 4)
    per, at = block >> porder, 0
    for p, k in enumerate(params):
        count = per - order if p == 0 else per
        part, at = res[at:at + count], at + count
        if isinstance(k, tuple):
            width = k[1]
            w.put(31 if method else 15, 5 if method else 4)
            w.put(width, 5)
            for e in part:
                assert width == 0 and e == 0 or -(1 << (width - 1)) <= e < (1 << (width - 1))
                w.put(e, width)
        else:
            w.put(k, 5 if method else 4)
            for e in part:
                u = (e << 1) if e >= 0 else ((-e) << 1) - 1
                w.unary(u >> k)
                w.put(u, k)
    assert spec.get("short_partitions") or at == len(res)


def frame(channels, bits, rate, number, specs, assignment=None, variable=False, crc16_xor=0, **head):
    """channels: [channel][sample] as the decoder must return them; assignment 8 / 9 / 10 derive side / mid.  -> the frame's bytes"""
    if assignment is None:
        assignment = len(channels) - 1
    block = len(channels[0])
    coded = [list(c) for c in channels]
    widths = [bits] * len(channels)
    if assignment == 8:
        coded[1], widths[1] = [l - r for l, r in zip(*channels)], bits + 1
    elif assignment == 9:
        coded[0], widths[0] = [l - r for l, r in zip(*channels)], bits + 1
    elif assignment == 10:
        coded = [[(l + r) >> 1 for l, r in zip(*channels)], [l - r for l, r in zip(*channels)]]
        widths[1] = bits + 1
    w = BitWriter()
    for s, bps, spec in zip(coded, widths, specs):
        put_subframe(w, s, bps, spec)
    w.pad()
    body = header(block, rate, bits, assignment, number, variable, **head) + w.bytes()
    return body + (crc16(body) ^ crc16_xor).to_bytes(2, "big")


def streaminfo_block(blocks, channels, bits, rate, frames, max_framesize=None):
    """blocks: [[channel][sample]] of every frame, frames: their bytes"""
    w = (bits + 7) // 8
    m = hashlib.md5()
    total = 0
    for ch in blocks:
        total += len(ch[0])
        m.update(b"".join((c[i] & ((1 << (8 * w)) - 1)).to_bytes(w, "little") for i in range(len(ch[0])) for c in ch))
    sizes = [len(ch[0]) for ch in blocks]
    body = min(max(min(sizes[:-1] or sizes), 16), 65535).to_bytes(2, "big") + min(max(sizes), 65535).to_bytes(2, "big")
    body += min(len(f) for f in frames).to_bytes(3, "big") + (max(len(f) for f in frames) if max_framesize is None else max_framesize).to_bytes(3, "big")
    body += ((rate << 44) | ((channels - 1) << 41) | ((bits - 1) << 36) | total).to_bytes(8, "big") + m.digest()
    return body


def metadata(kind, body, last=False):
    return bytes([(0x80 if last else 0) | kind]) + len(body).to_bytes(3, "big") + body


def stream(blocks, bits, rate, specs_of, assignment=None, variable=False, extra_blocks=(), max_framesize=None):
    """blocks: [[channel][sample]]; specs_of(i, block) -> subframe specs.  -> (stream bytes, [frame bytes])"""
    frames, first = [], 0
    for i, ch in enumerate(blocks):
        frames.append(frame(ch, bits, rate, first if variable else i, specs_of(i, ch), assignment=assignment, variable=variable))
        first += len(ch[0])
    out = b"fLaC" + metadata(0, streaminfo_block(blocks, len(blocks[0]), bits, rate, frames, max_framesize), last=not extra_blocks)
    for k, (kind, body) in enumerate(extra_blocks):
        out += metadata(kind, body, last=k == len(extra_blocks) - 1)
    return out + b"".join(frames), frames

"""A plain-Python Apple Lossless decoder, written from the format's public description and independent of the product: the
ALACSpecificConfig in its three wrappings, the element walk of a packet, the adaptive Golomb residuals, the adapting predictor in
32-bit wrapping arithmetic, pair unmix, extra bits, the output width, and the CAF chunks an ALAC file needs.

tests/test_alac_cpu.py pins it: the reference's fixture decodes to its decoded twin, 23 680 samples, bit for bit."""
import struct

INVALID, UNSUPPORTED, ELEMENT = "invalid", "unsupported", "element"


class AlacError(Exception):
    def __init__(self, kind, text=""):
        super().__init__(text or kind)
        self.kind = kind


def w32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def sx(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def sign(v):
    return (v > 0) - (v < 0)


def floor_log2(v):
    return v.bit_length() - 1 if v else 0


class Bits:
    """reads past the end give zeros and set `over`, as the device does"""

    def __init__(self, data):
        self.n = len(data) * 8
        self.v = int.from_bytes(data, "big")
        self.pos = 0
        self.over = False

    def peek(self, n):
        if n == 0:
            return 0
        left = self.n - self.pos
        if left >= n:
            return (self.v >> (left - n)) & ((1 << n) - 1)
        if left <= 0:
            return 0
        return (self.v & ((1 << left) - 1)) << (n - left)

    def skip(self, n):
        self.pos += n
        if self.pos > self.n:
            self.over = True

    def read(self, n):
        v = self.peek(n)
        self.skip(n)
        return v

    def signed(self, n):
        return sx(self.read(n), n) if n else 0


def parse_cookie(cookie):
    """bare config | MP4 `alac` FullBox payload | QuickTime `frma` + `alac` atoms -> dict"""
    c = bytes(cookie)
    if len(c) >= 24 + 12 + 12 and c[4:8] == b"frma" and c[16:20] == b"alac":
        c = c[24:]
    elif len(c) >= 28 and c[:4] == b"\0\0\0\0":
        c = c[4:]
    if len(c) < 24:
        raise AlacError(INVALID, "ALAC magic cookie is shorter than 24 bytes")
    fl, ver, depth, pb, mb, kb, ch, max_run, max_bytes, rate_avg, rate = struct.unpack(">IBBBBBBHIII", c[:24])
    if rate == 0:
        raise AlacError(INVALID, "ALAC stream reports a zero sample rate")
    if not 1 <= ch <= 8:
        raise AlacError(INVALID, f"ALAC channel count {ch} exceeds the supported range 1-8")
    if depth not in (16, 24, 32):
        raise AlacError(INVALID, f"Unsupported ALAC bit depth: {depth}")
    if not 1 <= fl <= 65536:
        raise AlacError(INVALID, f"ALAC frame length {fl} exceeds the 1-65536 frame budget")
    return dict(frame_length=fl, version=ver, bit_depth=depth, pb=pb, mb=mb, kb=kb, channels=ch, max_run=max_run, max_frame_bytes=max_bytes,
                avg_bit_rate=rate_avg, sample_rate=rate)


def read_scalar(b, k, escape_bits):
    count = 0
    while count < 9 and b.peek(1):
        b.skip(1)
        count += 1
    if count == 9:
        return b.read(escape_bits)
    b.skip(1)
    if k == 1:
        return count
    x = count * ((1 << k) - 1)
    e = b.peek(k)
    if e > 1:
        x += e - 1
        b.skip(k)
    else:
        b.skip(k - 1)
    return x


def read_residuals(b, cfg, n, bps, pb_factor, stats=None):
    m = pb_factor * cfg["pb"] // 4
    kb = cfg["kb"]
    if kb == 0:
        raise AlacError(INVALID, "Rice limit 0")
    history, modifier = cfg["mb"], 0
    out = [0] * n
    i = 0
    while i < n:
        k = min(floor_log2((history >> 9) + 3), kb)
        x = (read_scalar(b, k, bps) + modifier) & 0xFFFFFFFF
        modifier = 0
        out[i] = w32((x >> 1) ^ -(x & 1))
        if x > 0xFFFF:
            history = 0xFFFF
        else:
            history = (history + x * m - (((history * m) & 0xFFFFFFFF) >> 9)) & 0xFFFFFFFF
        if history < 128 and i + 1 < n:
            k = min(7 - floor_log2(history) + ((history + 16) >> 6), kb)
            run = read_scalar(b, k, 16)
            if stats is not None:
                stats["runs"] = stats.get("runs", 0) + 1
            if run >= n - i:
                raise AlacError(INVALID, "zero run past the element's end")
            i += run
            if run <= 0xFFFF:
                modifier = 1
            history = 0
        if b.over:
            raise AlacError(INVALID, "residuals past the packet's end")
        i += 1
    return out


def first_order_sum(e, bps):
    out = list(e)
    for i in range(1, len(e)):
        out[i] = sx(out[i - 1] + e[i], bps)
    return out


def predict(e, bps, ptype, order, shift, coefs):
    """coefs[j] multiplies out[i - order + j] - out[i - order - 1]"""
    if ptype == 15:
        e = first_order_sum(e, bps)
    elif ptype != 0:
        raise AlacError(INVALID, f"prediction type {ptype}")
    n = len(e)
    out = list(e)
    if order == 0 or n <= 1:
        return out
    if order == 31:
        return first_order_sum(e, bps)
    c = list(coefs)
    for i in range(1, min(order, n - 1) + 1):
        out[i] = sx(out[i - 1] + e[i], bps)
    half = (1 << (shift - 1)) if shift else 0
    for i in range(order + 1, n):
        d = out[i - order - 1]
        p = out[i - order:i]
        val = 0
        for j in range(order):
            val += w32(p[j] - d) * c[j]
        val = w32(w32(val) + half) >> shift
        err = e[i]
        out[i] = sx(val + d + err, bps)
        s_e = sign(err)
        if s_e:
            j = 0
            while j < order and w32(err * s_e) > 0:
                v = w32(d - p[j])
                s = sign(v) * s_e
                c[j] = w32(c[j] - s)
                err = w32(err - w32((w32(v * s) >> shift) * (j + 1)))
                j += 1
    return out


def skip_dse(b):
    b.skip(4)
    align = b.read(1)
    count = b.read(8)
    if count == 255:
        count += b.read(8)
    if align:
        b.skip(-b.pos % 8)
    b.skip(8 * count)


def skip_fil(b):
    count = b.read(4)
    if count == 15:
        count += b.read(8) - 1
    b.skip(8 * count)


def element_header(b, cfg, el_ch):
    b.skip(16)
    has_size = b.read(1)
    extra = 8 * b.read(2)
    raw = b.read(1)
    n = b.read(32) if has_size else cfg["frame_length"]
    return n, extra, raw


def packet_frames(cfg, packet):
    """the frame count of the first audio element, as the host reads it"""
    b = Bits(packet)
    while not b.over:
        tag = b.read(3)
        if tag in (0, 1, 3):
            n, _, _ = element_header(b, cfg, 1)
            if b.over or n == 0 or n > cfg["frame_length"]:
                raise AlacError(INVALID, "frame count")
            return n
        if tag == 4:
            skip_dse(b)
        elif tag == 6:
            skip_fil(b)
        elif tag in (2, 5) and not b.over:
            raise AlacError(ELEMENT, f"element {tag}")
        else:
            break
    raise AlacError(INVALID, "no audio element")


def decode_packet(cfg, packet, stats=None):
    """-> (channels x n samples as lists, n)"""
    b = Bits(packet)
    depth, want = cfg["bit_depth"], cfg["channels"]
    if cfg["kb"] == 0:
        raise AlacError(INVALID, "Rice limit 0")
    chans, frames = [], None
    while True:
        tag = b.read(3)
        if b.over:
            raise AlacError(INVALID, "packet ends without END")
        if tag == 7:
            break
        if tag in (2, 5):
            raise AlacError(ELEMENT, f"element {tag}")
        if tag == 4:
            skip_dse(b)
            continue
        if tag == 6:
            skip_fil(b)
            continue
        el_ch = 2 if tag == 1 else 1
        if len(chans) + el_ch > want:
            raise AlacError(INVALID, "more channels than the cookie has")
        n, extra, raw = element_header(b, cfg, el_ch)
        if b.over or n == 0 or n > cfg["frame_length"] or (frames is not None and n != frames):
            raise AlacError(INVALID, "frame count")
        frames = n
        bps = depth - extra + el_ch - 1
        if bps > 32:
            raise AlacError(UNSUPPORTED, "33-bit channel")
        if bps < 1:
            raise AlacError(INVALID, "extra bits")
        if raw:
            flat = [b.signed(depth) for _ in range(n * el_ch)]
            if b.over:
                raise AlacError(INVALID, "samples past the packet's end")
            chans += [flat[c::el_ch] for c in range(el_ch)]
            continue
        mix_shift, mix_weight = b.read(8), b.read(8)
        heads = []
        for _ in range(el_ch):
            ptype, shift, pbf, order = b.read(4), b.read(4), b.read(3), b.read(5)
            coefs = [b.signed(16) for _ in range(order)][::-1]
            heads.append((ptype, shift, pbf, order, coefs))
        extras = [b.read(extra) for _ in range(n * el_ch)] if extra else None
        if b.over:
            raise AlacError(INVALID, "header past the packet's end")
        outs = []
        for ptype, shift, pbf, order, coefs in heads:
            if ptype not in (0, 15):
                raise AlacError(INVALID, f"prediction type {ptype}")
            e = read_residuals(b, cfg, n, bps, pbf, stats)
            outs.append(predict(e, bps, ptype, order, shift, coefs))
        if el_ch == 2 and mix_weight:
            for i in range(n):
                a, bb = outs[0][i], outs[1][i]
                a = w32(a - (w32(bb * mix_weight) >> min(mix_shift, 31)))
                bb = w32(bb + a)
                outs[0][i], outs[1][i] = bb, a
        if extra:
            for c in range(el_ch):
                outs[c] = [w32((outs[c][i] << extra) | extras[i * el_ch + c]) for i in range(n)]
        chans += outs
    if b.over or b.n - b.pos >= 8 or len(chans) != want:
        raise AlacError(INVALID, "packet end")
    return chans, frames


def pcm_bytes(chans, depth):
    """interleaved little-endian in ceil(depth / 8) bytes"""
    width, n = (depth + 7) // 8, len(chans[0]) if chans else 0
    out = bytearray()
    mask = (1 << (8 * width)) - 1
    for i in range(n):
        for c in chans:
            out += (c[i] & mask).to_bytes(width, "little")
    return bytes(out)


def decode_packet_bytes(cfg, packet):
    chans, _ = decode_packet(cfg, packet)
    return pcm_bytes(chans, cfg["bit_depth"])


# ---- CAF ---------------------------------------------------------------------------------------------------------------------------

def caf_chunks(data):
    """-> {type: (payload offset, payload size)} of a `caff` file; a data chunk of size -1 runs to the end"""
    if len(data) < 8 or data[:4] != b"caff":
        raise AlacError(INVALID, "not a CAF file")
    at, found = 8, {}
    while at + 12 <= len(data):
        kind, size = data[at:at + 4], struct.unpack(">q", data[at + 4:at + 12])[0]
        at += 12
        if size < 0:
            size = len(data) - at
        if at + size > len(data):
            raise AlacError(INVALID, "CAF chunk past the end")
        found.setdefault(kind.decode("latin1"), (at, size))
        at += size
    return found


def caf_index(data):
    """-> (cfg, [packet bytes], valid, priming, remainder)"""
    ch = caf_chunks(data)
    desc = data[ch["desc"][0]:ch["desc"][0] + ch["desc"][1]]
    cookie = data[ch["kuki"][0]:ch["kuki"][0] + ch["kuki"][1]]
    cfg = parse_cookie(cookie)
    bytes_per_packet, frames_per_packet = struct.unpack(">II", desc[16:24])
    at, size = ch["data"]
    at, size = at + 4, size - 4
    if bytes_per_packet:
        sizes = [bytes_per_packet] * (size // bytes_per_packet)
        valid, priming, remainder = len(sizes) * frames_per_packet, 0, 0
    else:
        t = data[ch["pakt"][0]:ch["pakt"][0] + ch["pakt"][1]]
        count, valid, priming, remainder = struct.unpack(">qqii", t[:24])
        sizes, p = [], 24
        for _ in range(count):
            v = 0
            while True:
                v = (v << 7) | (t[p] & 0x7F)
                p += 1
                if not t[p - 1] & 0x80:
                    break
            sizes.append(v)
    packets = []
    for s in sizes:
        packets.append(bytes(data[at:at + s]))
        at += s
    return dict(cfg, caf_frames_per_packet=frames_per_packet), packets, valid, priming, remainder


def trim(start, decoded, priming, valid):
    """the packet's frames that lie in [priming, priming + valid): (first frame, count) or None"""
    lo, hi = max(start, priming), min(start + decoded, priming + valid)
    return (lo - start, hi - lo) if hi > lo else None


def decode_caf(data):
    """-> (cfg, PCM bytes after trimming)"""
    cfg, packets, valid, priming, remainder = caf_index(data)
    width = (cfg["bit_depth"] + 7) // 8 * cfg["channels"]
    out, start = bytearray(), 0
    for p in packets:
        chans, n = decode_packet(cfg, p)
        t = trim(start, n, priming, valid)
        if t:
            out += pcm_bytes(chans, cfg["bit_depth"])[t[0] * width:(t[0] + t[1]) * width]
        start += cfg["caf_frames_per_packet"]  # a packet's place on the timeline is its index times the description's count
    return cfg, bytes(out)

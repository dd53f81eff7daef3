"""A lossless Apple Lossless packet writer for the tests: what tests/alac_model.py reads, written.  It does not search for good
parameters -- the caller chooses order, shift, pb_factor, mix, extra bytes and prediction type, so every branch of a decoder can be
reached on purpose -- and whatever it is given it writes exactly: model(builder(x)) == x.

Also the three cookie wrappings and a CAF file in both packet-table forms."""
import struct

from alac_model import floor_log2, sign, sx, w32


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        if n == 0:
            return
        self.acc = (self.acc << n) | (v & ((1 << n) - 1))
        self.n += n
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xFF)
        self.acc &= (1 << self.n) - 1

    @property
    def pos(self):
        return len(self.out) * 8 + self.n

    def bytes(self):
        return bytes(self.out) + (bytes([(self.acc << (8 - self.n)) & 0xFF]) if self.n else b"")


def config(frame_length=4096, bit_depth=16, channels=1, sample_rate=44100, pb=40, mb=10, kb=14, max_run=255):
    return dict(frame_length=frame_length, version=0, bit_depth=bit_depth, pb=pb, mb=mb, kb=kb, channels=channels, max_run=max_run,
                max_frame_bytes=0, avg_bit_rate=0, sample_rate=sample_rate)


def cookie(cfg, wrap="bare"):
    """wrap: bare | mp4 (four zero bytes in front) | qt (`frma` atom, then an `alac` atom)"""
    c = struct.pack(">IBBBBBBHIII", cfg["frame_length"], cfg["version"], cfg["bit_depth"], cfg["pb"], cfg["mb"], cfg["kb"], cfg["channels"],
                    cfg["max_run"], cfg["max_frame_bytes"], cfg["avg_bit_rate"], cfg["sample_rate"])
    if wrap == "mp4":
        return bytes(4) + c
    if wrap == "qt":
        return struct.pack(">I4s4s", 12, b"frma", b"alac") + struct.pack(">I4sI", 36, b"alac", 0) + c
    return c


class Element:
    """one audio element: kind sce | cpe | lfe"""

    def __init__(self, kind="sce", order=4, shift=6, pb_factor=4, mix_shift=0, mix_weight=0, extra_bytes=0, ptype=0, raw=False, coefs=None,
                 n_override=None, has_size=None):
        self.kind, self.order, self.shift, self.pb_factor = kind, order, shift, pb_factor
        self.mix_shift, self.mix_weight, self.extra_bytes, self.ptype, self.raw = mix_shift, mix_weight, extra_bytes, ptype, raw
        self.coefs, self.n_override, self.has_size = coefs, n_override, has_size

    @property
    def channels(self):
        return 2 if self.kind == "cpe" else 1


def default_coefs(order, shift):
    c = [0] * order
    for j in range(order):
        back = order - j  # 1 = the newest sample
        c[j] = ((1 << shift) * 3 // 4 if back == 1 else (-1) ** back * ((1 << shift) >> (back + 1)))
    return c


def errors(out, bps, ptype, order, shift, coefs):
    """the predictor's inverse: the residuals from which alac_model.predict gives `out` back"""
    n = len(out)
    e = list(out)
    if order == 31 or (order and n > 1):
        for i in range(1, n if order == 31 else min(order, n - 1) + 1):
            e[i] = sx(out[i] - out[i - 1], bps)
    if 0 < order < 31:
        c = list(coefs)
        half = (1 << (shift - 1)) if shift else 0
        for i in range(order + 1, n):
            d = out[i - order - 1]
            p = out[i - order:i]
            val = 0
            for j in range(order):
                val += w32(p[j] - d) * c[j]
            val = w32(w32(val) + half) >> shift
            err = e[i] = sx(out[i] - val - d, bps)
            s_e = sign(err)
            j = 0
            while s_e and j < order and w32(err * s_e) > 0:
                v = w32(d - p[j])
                s = sign(v) * s_e
                c[j] = w32(c[j] - s)
                err = w32(err - w32((w32(v * s) >> shift) * (j + 1)))
                j += 1
    if ptype == 15:
        e = [e[0]] + [sx(e[i] - e[i - 1], bps) for i in range(1, n)]
    return e


def write_scalar(w, v, k, escape_bits):
    base = 1 if k == 1 else (1 << k) - 1
    count, rem = divmod(v, base)
    if count >= 9:
        w.put(0x1FF, 9)
        assert v < (1 << escape_bits), (v, escape_bits)
        w.put(v, escape_bits)
        return
    w.put((1 << count) - 1, count)
    w.put(0, 1)
    if k == 1:
        return
    if rem == 0:
        w.put(0, k - 1)
    else:
        w.put(rem + 1, k)


def write_residuals(w, cfg, e, bps, pb_factor, stats=None):
    m = pb_factor * cfg["pb"] // 4
    kb, n = cfg["kb"], len(e)
    history, modifier = cfg["mb"], 0
    i = 0
    while i < n:
        k = min(floor_log2((history >> 9) + 3), kb)
        r = e[i]
        x = ((r << 1) ^ (r >> 31)) & 0xFFFFFFFF
        assert x >= modifier
        write_scalar(w, x - modifier, k, bps)
        modifier = 0
        if stats is not None:
            stats.setdefault("k", set()).add(k)
            if x > 0xFFFF:
                stats["pinned"] = stats.get("pinned", 0) + 1
        if x > 0xFFFF:
            history = 0xFFFF
        else:
            history = (history + x * m - (((history * m) & 0xFFFFFFFF) >> 9)) & 0xFFFFFFFF
        if history < 128 and i + 1 < n:
            k = min(7 - floor_log2(history) + ((history + 16) >> 6), kb)
            run = 0
            while i + 1 + run < n and e[i + 1 + run] == 0 and run < 0xFFFF:
                run += 1
            write_scalar(w, run, k, 16)
            if stats is not None:
                stats.setdefault("runs", []).append(run)
            i += run
            modifier = 1
            history = 0
        i += 1


def write_element(w, cfg, el, chans, stats=None):
    """chans: el.channels lists of n samples of the cookie's depth"""
    depth, ch = cfg["bit_depth"], el.channels
    n = len(chans[0])
    w.put({"sce": 0, "cpe": 1, "lfe": 3}[el.kind], 3)
    w.put(0, 4)
    w.put(0, 12)
    has_size = el.has_size if el.has_size is not None else n != cfg["frame_length"]
    w.put(1 if has_size else 0, 1)
    w.put(el.extra_bytes, 2)
    w.put(1 if el.raw else 0, 1)
    if has_size:
        w.put(el.n_override if el.n_override is not None else n, 32)
    if el.raw:
        for i in range(n):
            for c in range(ch):
                w.put(chans[c][i], depth)
        return
    extra = 8 * el.extra_bytes
    bps = depth - extra + ch - 1
    high = [[v >> extra for v in c] for c in chans]
    low = [[v & ((1 << extra) - 1) for v in c] for c in chans]
    if ch == 2 and el.mix_weight:
        left, right = high
        side = [w32(l - r) for l, r in zip(left, right)]
        high = [[w32(r + (w32(s * el.mix_weight) >> min(el.mix_shift, 31))) for r, s in zip(right, side)], side]
    w.put(el.mix_shift, 8)
    w.put(el.mix_weight, 8)
    coefs = el.coefs if el.coefs is not None else default_coefs(el.order, el.shift)
    assert len(coefs) == el.order
    for _ in range(ch):
        w.put(el.ptype, 4)
        w.put(el.shift, 4)
        w.put(el.pb_factor, 3)
        w.put(el.order, 5)
        for c in reversed(coefs):
            w.put(c, 16)
    if extra:
        if stats is not None:
            stats["extra_pos"] = w.pos
        for i in range(n):
            for c in range(ch):
                w.put(low[c][i], extra)
    ptype = el.ptype if el.ptype in (0, 15) else 0
    for c in range(ch):
        write_residuals(w, cfg, errors(high[c], bps, ptype, el.order, el.shift, coefs), bps, el.pb_factor, stats)


def write_dse(w, payload=b"\x01\x02\x03", align=True):
    w.put(4, 3)
    w.put(0, 4)
    w.put(1 if align else 0, 1)
    if len(payload) >= 255:
        w.put(255, 8)
        w.put(len(payload) - 255, 8)
    else:
        w.put(len(payload), 8)
    if align:
        w.put(0, -w.pos % 8)
    for b in payload:
        w.put(b, 8)


def write_fil(w, count=3):
    w.put(6, 3)
    if count >= 15:
        w.put(15, 4)
        w.put(count - 14, 8)
    else:
        w.put(count, 4)
    for _ in range(count):
        w.put(0xA5, 8)


def layout(channels, lfe=False):
    """an element sequence for 1 ... 8 channels: pairs first, a single last (an LFE when asked)"""
    kinds = ["cpe"] * (channels // 2) + (["lfe" if lfe else "sce"] if channels % 2 else [])
    return kinds if channels != 1 else ["sce"]


def packet(cfg, chans, elements=None, dse=None, fil=None, end=True, stats=None, before=None, **el_args):
    """chans: cfg['channels'] lists of n samples -> one packet.  elements: Element objects in bitstream order (default: layout() with
    el_args); dse / fil: a payload / a byte count to put in front of END; before: a callback(writer) that writes in front of everything"""
    if elements is None:
        elements = [Element(kind, **el_args) for kind in layout(cfg["channels"])]
    w = BitWriter()
    if before:
        before(w)
    at = 0
    for el in elements:
        write_element(w, cfg, el, chans[at:at + el.channels], stats)
        at += el.channels
    if dse is not None:
        write_dse(w, dse)
    if fil is not None:
        write_fil(w, fil)
    if end:
        w.put(7, 3)
    return w.bytes()


def vlq(v):
    out = [v & 0x7F]
    v >>= 7
    while v:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    return bytes(reversed(out))


def chunk(kind, payload, size=None):
    return kind + struct.pack(">q", len(payload) if size is None else size) + payload


def pakt(sizes, valid, priming=0, remainder=0):
    return struct.pack(">qqii", len(sizes), valid, priming, remainder) + b"".join(vlq(s) for s in sizes)


def desc(cfg, bytes_per_packet=0, frames_per_packet=None, bits=0, fmt=b"alac", rate=None, channels=None):
    return struct.pack(">d4sIIIII", float(cfg["sample_rate"] if rate is None else rate), fmt, 0, bytes_per_packet,
                       cfg["frame_length"] if frames_per_packet is None else frames_per_packet, cfg["channels"] if channels is None else channels,
                       bits)


def caf(cfg, packets, valid=None, priming=0, remainder=0, wrap="qt", constant=False, edit_count=1):
    """a CAF file: desc, kuki, data, pakt (constant=True: packets of one size and no table)"""
    total = len(packets) * cfg["frame_length"]
    valid = total - priming - remainder if valid is None else valid
    if constant:
        assert len({len(p) for p in packets}) == 1  # fewer than 8 bits may follow END, so nothing can be padded
    out = b"caff" + struct.pack(">HH", 1, 0)
    out += chunk(b"desc", desc(cfg, bytes_per_packet=len(packets[0]) if constant else 0))
    out += chunk(b"kuki", cookie(cfg, wrap))
    out += chunk(b"data", struct.pack(">I", edit_count) + b"".join(packets))
    if not constant:
        out += chunk(b"pakt", pakt([len(p) for p in packets], valid, priming, remainder))
    return out

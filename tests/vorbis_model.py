"""Vorbis I in numpy: Ogg pages, the three headers, the packet decode (floor 1, residues 0 / 1 / 2, coupling, IMDCT, window, overlap-add)
and the narrowing to s16.  Parameterised by dtype: float64 is the yardstick; float32 follows the operation order that
csrc/vorbis_decode.hip states (VQ value = ((multiplicand * delta) + minimum) + last; residue adds in stream order; floor x residue;
y x window; right half + left half), except inside the FFT, whose butterfly order is the model's own.

Choices where the specification leaves a malformed stream open (the same on the device):
  * a final floor Y outside [0, range) is clamped into it when it is computed;
  * a code book with one used entry reads one bit and returns that entry whatever the bit is;
  * the window slopes follow the packet's flags, the overlap-add follows the sizes of the blocks that actually came."""
import struct

import numpy as np

MAX_CHANNELS = 8


class VorbisError(Exception):
    pass


class Unsupported(VorbisError):
    pass


def ilog(x):
    return int(x).bit_length() if x > 0 else 0


def float32_unpack(x):
    mant = x & 0x1fffff
    if x & 0x80000000:
        mant = -mant
    return float(np.ldexp(np.float64(mant), ((x & 0x7fe00000) >> 21) - 788))


def lookup1_values(entries, dims):
    r = int(np.floor(np.exp(np.log(entries) / dims)))
    while (r + 1) ** dims <= entries:
        r += 1
    while r ** dims > entries:
        r -= 1
    return r


INVERSE_DB = (np.float64(1.0649863e-07) * (np.float64(1.0) / np.float64(1.0649863e-07)) ** (np.arange(256) / 255.0))


def inverse_db(dtype):
    """the floor's table as the device holds it: the geometric series in float64, rounded to float32 (then widened for float64 runs,
    so that both models multiply by the same numbers)"""
    return INVERSE_DB.astype(np.float32).astype(dtype)


# ---- Ogg ------------------------------------------------------------------------------------------------------------------------

def ogg_page_crc(page):
    crc = 0
    for i, b in enumerate(page):
        if 22 <= i < 26:
            b = 0
        crc ^= b << 24
        for _ in range(8):
            crc = ((crc << 1) ^ 0x04C11DB7) & 0xffffffff if crc & 0x80000000 else (crc << 1) & 0xffffffff
    return crc


def ogg_page(header_type, granule, serial, sequence, packets_lacing, body):
    page = bytearray(27 + len(packets_lacing) + len(body))
    page[:4] = b"OggS"
    page[5] = header_type
    page[6:14] = struct.pack("<Q", granule)
    page[14:18] = struct.pack("<I", serial)
    page[18:22] = struct.pack("<I", sequence)
    page[26] = len(packets_lacing)
    page[27:27 + len(packets_lacing)] = bytes(packets_lacing)
    page[27 + len(packets_lacing):] = body
    page[22:26] = struct.pack("<I", ogg_page_crc(page))
    return bytes(page)


def ogg_packets(data):
    """-> [dict(data, serial, first_in_stream, last_in_page, last_in_stream, granule_position)] of a whole, well-formed file"""
    out, at, pending = [], 0, b""
    while at + 27 <= len(data):
        assert data[at:at + 4] == b"OggS"
        htype, granule, serial = data[at + 5], struct.unpack_from("<Q", data, at + 6)[0], struct.unpack_from("<I", data, at + 14)[0]
        nseg = data[at + 26]
        lacing = data[at + 27:at + 27 + nseg]
        body = at + 27 + nseg
        assert ogg_page_crc(data[at:body + sum(lacing)]) == struct.unpack_from("<I", data, at + 22)[0]
        done = []
        for s in lacing:
            pending += data[body:body + s]
            body += s
            if s < 255:
                done.append(dict(data=pending, serial=serial, first_in_stream=bool(htype & 2), last_in_page=False, last_in_stream=False,
                                 granule_position=None))
                pending = b""
        if done:
            done[-1]["last_in_page"], done[-1]["last_in_stream"] = True, bool(htype & 4)
            done[-1]["granule_position"] = None if granule == 2 ** 64 - 1 else granule
        out += done
        at = body
    return out


# ---- bits -----------------------------------------------------------------------------------------------------------------------

class Bits:
    """LSB first.  A read that does not fit returns None, sets eop and consumes nothing more."""

    def __init__(self, data):
        self.v, self.n, self.pos, self.eop = int.from_bytes(data, "little"), 8 * len(data), 0, False

    def read(self, bits):
        if self.eop or self.pos + bits > self.n:
            self.eop = True
            return None
        r = (self.v >> self.pos) & ((1 << bits) - 1)
        self.pos += bits
        return r


class Codebook:
    def __init__(self):
        self.dims = self.entries = 0
        self.lengths = []  # 0: unused
        self.lookup_type, self.minimum, self.delta, self.value_bits, self.sequence_p, self.multiplicands = 0, 0.0, 0.0, 0, 0, []
        self.single = -1

    def assign(self):
        """the specification's code word assignment -> {(length, code): entry}; raises unless the tree is complete (or the one-entry case)"""
        used = [(i, l) for i, l in enumerate(self.lengths) if l]
        if not used:
            raise VorbisError("code book without a used entry")
        if len(used) == 1:
            if used[0][1] != 1:
                raise VorbisError("code book with one entry of length other than 1")
            self.single, self.codes = used[0][0], {}
            return
        avail, codes = [0] * 33, {}
        first = True
        for i, l in used:
            if first:
                code, first = 0, False
                for k in range(1, l + 1):
                    avail[k] = 1 << (32 - k)
            else:
                z = l
                while z > 0 and not avail[z]:
                    z -= 1
                if z == 0:
                    raise VorbisError("over-specified code book")
                res = avail[z]
                avail[z] = 0
                code = res >> (32 - l)
                for y in range(z + 1, l + 1):
                    avail[y] = res + (1 << (32 - y))
            codes[(l, code)] = i
        if any(avail[1:]):
            raise VorbisError("under-specified code book")
        self.codes = codes

    def decode(self, b):
        if self.single >= 0:
            return None if b.read(1) is None else self.single
        code = 0
        for l in range(1, 33):
            bit = b.read(1)
            if bit is None:
                return None
            code = code << 1 | bit
            e = self.codes.get((l, code))
            if e is not None:
                return e
        return None

    def vq_table(self, dtype):
        """[entries][dims] in dtype: ((multiplicand * delta) + minimum) + last"""
        if self.lookup_type == 0:
            return None
        key = np.dtype(dtype).name
        if not hasattr(self, "_vq"):
            self._vq = {}
        if key not in self._vq:
            m = np.asarray(self.multiplicands, np.int64)
            e = np.arange(self.entries, dtype=np.int64)
            t = np.zeros((self.entries, self.dims), dtype)
            last = np.zeros(self.entries, dtype)
            delta, minimum = dtype(np.float32(self.delta)), dtype(np.float32(self.minimum))
            div = 1
            with np.errstate(all="ignore"):
                for i in range(self.dims):
                    if self.lookup_type == 1:
                        lv = len(self.multiplicands)
                        off = (e // div) % lv
                        div *= lv
                    else:
                        off = e * self.dims + i
                    t[:, i] = ((m[off].astype(dtype) * delta) + minimum) + last
                    if self.sequence_p:
                        last = t[:, i].copy()
            self._vq[key] = t
        return self._vq[key]


class Setup:
    pass


def parse_ident(p):
    b = Bits(p)
    if len(p) < 7 or p[:7] != b"\x01vorbis":
        raise VorbisError("not a Vorbis identification header")
    b.pos = 56
    f = {}
    version = b.read(32)
    f["channels"], f["sample_rate"] = b.read(8), b.read(32)
    f["bitrate_maximum"], f["bitrate_nominal"], f["bitrate_minimum"] = b.read(32), b.read(32), b.read(32)
    e0, e1, framing = b.read(4), b.read(4), b.read(1)
    if b.eop:
        raise VorbisError("identification header too short")
    if version != 0 or f["channels"] == 0 or f["sample_rate"] == 0 or not framing:
        raise VorbisError("bad identification header")
    if not (6 <= e0 <= e1 <= 13):
        raise VorbisError("bad block sizes")
    f["blocksize_0"], f["blocksize_1"] = 1 << e0, 1 << e1
    return f


def parse_comment(p):
    if len(p) < 7 or p[:7] != b"\x03vorbis":
        raise VorbisError("not a Vorbis comment header")
    at = 7

    def take(n):
        nonlocal at
        if at + n > len(p):
            raise VorbisError("comment header too short")
        at += n
        return p[at - n:at]

    vendor = take(struct.unpack("<I", take(4))[0])
    comments = [take(struct.unpack("<I", take(4))[0]) for _ in range(struct.unpack("<I", take(4))[0])]
    if not take(1)[0] & 1:
        raise VorbisError("comment header without framing bit")
    return vendor, comments


def parse_setup(p, channels, bs0, bs1):
    if len(p) < 7 or p[:7] != b"\x05vorbis":
        raise VorbisError("not a Vorbis setup header")
    b = Bits(p)
    b.pos = 56

    def rd(n):
        v = b.read(n)
        if v is None:
            raise VorbisError("setup header too short")
        return v

    s = Setup()
    s.books = []
    for _ in range(rd(8) + 1):
        if rd(24) != 0x564342:
            raise VorbisError("code book sync")
        c = Codebook()
        c.dims, c.entries = rd(16), rd(24)
        if c.dims == 0 or c.entries == 0:
            raise VorbisError("empty code book")
        if rd(1):
            cur, ln = 0, rd(5) + 1
            while cur < c.entries:
                num = rd(ilog(c.entries - cur))
                if cur + num > c.entries or ln > 32:
                    raise VorbisError("ordered code book lengths")
                c.lengths += [ln] * num
                cur += num
                ln += 1
        else:
            sparse = rd(1)
            for _ in range(c.entries):
                c.lengths.append(rd(5) + 1 if (not sparse or rd(1)) else 0)
        c.lookup_type = rd(4)
        if c.lookup_type > 2:
            raise VorbisError("code book lookup type")
        if c.lookup_type:
            c.minimum, c.delta, c.value_bits, c.sequence_p = float32_unpack(rd(32)), float32_unpack(rd(32)), rd(4) + 1, rd(1)
            n = lookup1_values(c.entries, c.dims) if c.lookup_type == 1 else c.entries * c.dims
            c.multiplicands = [rd(c.value_bits) for _ in range(n)]
        c.assign()
        s.books.append(c)
    nb = len(s.books)
    for _ in range(rd(6) + 1):
        if rd(16) != 0:
            raise VorbisError("time domain transform")
    s.floors = []
    for _ in range(rd(6) + 1):
        t = rd(16)
        if t == 0:
            raise Unsupported("floor type 0 is not built")
        if t != 1:
            raise VorbisError("floor type")
        f = Setup()
        f.partition_class = [rd(4) for _ in range(rd(5))]
        f.class_dim, f.class_sub, f.class_master, f.sub_books = [], [], [], []
        for _ in range(max(f.partition_class) + 1 if f.partition_class else 0):
            f.class_dim.append(rd(3) + 1)
            f.class_sub.append(rd(2))
            f.class_master.append(rd(8) if f.class_sub[-1] else 0)
            if f.class_sub[-1] and f.class_master[-1] >= nb:
                raise VorbisError("floor master book")
            f.sub_books.append([rd(8) - 1 for _ in range(1 << f.class_sub[-1])])
            if any(x >= nb for x in f.sub_books[-1]):
                raise VorbisError("floor subclass book")
        f.multiplier, f.rangebits = rd(2) + 1, rd(4)
        f.x = [0, 1 << f.rangebits]
        for cl in f.partition_class:
            f.x += [rd(f.rangebits) for _ in range(f.class_dim[cl])]
        if len(f.x) > 65 or len(set(f.x)) != len(f.x):
            raise VorbisError("floor X list")
        f.sorted = sorted(range(len(f.x)), key=lambda i: f.x[i])
        f.low, f.high = [0, 0], [0, 0]
        for i in range(2, len(f.x)):
            f.low.append(max((j for j in range(i) if f.x[j] < f.x[i]), key=lambda j: f.x[j]))
            f.high.append(min((j for j in range(i) if f.x[j] > f.x[i]), key=lambda j: f.x[j]))
        s.floors.append(f)
    s.residues = []
    for _ in range(rd(6) + 1):
        r = Setup()
        r.type = rd(16)
        if r.type > 2:
            raise VorbisError("residue type")
        r.begin, r.end, r.partition_size, r.classifications, r.classbook = rd(24), rd(24), rd(24) + 1, rd(6) + 1, rd(8)
        cascade = []
        for _ in range(r.classifications):
            low = rd(3)
            cascade.append((rd(5) if rd(1) else 0) * 8 + low)
        r.books = [[(rd(8) if cas >> j & 1 else -1) for j in range(8)] for cas in cascade]
        if r.classbook >= nb:
            raise VorbisError("residue class book")
        if r.end < r.begin:
            raise VorbisError("residue begin / end")
        if r.end > bs1 // 2 * (channels if r.type == 2 else 1):
            raise VorbisError("residue end beyond the longest vector")
        if r.classifications ** min(s.books[r.classbook].dims, 32) > s.books[r.classbook].entries:
            raise VorbisError("residue class book has too few entries for its class words")
        for row in r.books:
            for x in row:
                if x >= nb or (x >= 0 and s.books[x].lookup_type == 0):
                    raise VorbisError("residue book")
                if x >= 0 and r.partition_size % s.books[x].dims:
                    raise VorbisError("residue partition size is no multiple of a book's dimensions")
        s.residues.append(r)
    s.mappings = []
    for _ in range(rd(6) + 1):
        if rd(16) != 0:
            raise VorbisError("mapping type")
        m = Setup()
        m.submaps = rd(4) + 1 if rd(1) else 1
        m.coupling = []
        if rd(1):
            for _ in range(rd(8) + 1):
                mag, ang = rd(ilog(channels - 1)), rd(ilog(channels - 1))
                if mag == ang or mag >= channels or ang >= channels:
                    raise VorbisError("coupling channels")
                m.coupling.append((mag, ang))
        if rd(2) != 0:
            raise VorbisError("mapping reserved bits")
        m.mux = [rd(4) for _ in range(channels)] if m.submaps > 1 else [0] * channels
        if any(x >= m.submaps for x in m.mux):
            raise VorbisError("mapping mux")
        m.floor, m.residue = [], []
        for _ in range(m.submaps):
            rd(8)
            m.floor.append(rd(8))
            m.residue.append(rd(8))
            if m.floor[-1] >= len(s.floors) or m.residue[-1] >= len(s.residues):
                raise VorbisError("submap floor / residue")
        s.mappings.append(m)
    s.modes = []
    for _ in range(rd(6) + 1):
        flag, wt, tt, mp = rd(1), rd(16), rd(16), rd(8)
        if wt or tt or mp >= len(s.mappings):
            raise VorbisError("mode")
        s.modes.append((flag, mp))
    if not rd(1):
        raise VorbisError("setup header without framing bit")
    if channels > MAX_CHANNELS:
        raise Unsupported("more than 8 channels are not built")
    s.channels, s.bs = channels, (bs0, bs1)
    return s


# ---- packet decode --------------------------------------------------------------------------------------------------------------

ST_OK, ST_NOT_AUDIO, ST_BAD_MODE, ST_SHORT = 0, -801, -802, -803  # SK_VORBIS_*


class Staged:
    """what the entropy stage leaves of one packet"""


def render_point(x0, y0, x1, y1, x):
    dy, adx = y1 - y0, x1 - x0
    off = abs(dy) * (x - x0) // adx
    return y0 - off if dy < 0 else y0 + off


def floor1_decode(s, f, b):
    """-> (Y list or None when unused)"""
    nz = b.read(1)
    if not nz:
        return None
    rng = [256, 128, 86, 64][f.multiplier - 1]
    y = [b.read(ilog(rng - 1)), b.read(ilog(rng - 1))]
    for cl in f.partition_class:
        cdim, cbits = f.class_dim[cl], f.class_sub[cl]
        cval = s.books[f.class_master[cl]].decode(b) if cbits else 0
        if cval is None:
            return None
        for _ in range(cdim):
            book = f.sub_books[cl][cval & ((1 << cbits) - 1)]
            cval >>= cbits
            y.append(s.books[book].decode(b) if book >= 0 else 0)
    return None if b.eop or any(v is None for v in y) else y


def floor1_unwrap(f, y):
    rng = [256, 128, 86, 64][f.multiplier - 1]
    final, step2 = [y[0], y[1]] + [0] * (len(y) - 2), [True, True] + [False] * (len(y) - 2)
    final[0], final[1] = min(final[0], rng - 1), min(final[1], rng - 1)
    for i in range(2, len(y)):
        lo, hi = f.low[i], f.high[i]
        pred = render_point(f.x[lo], final[lo], f.x[hi], final[hi], f.x[i])
        val, highroom, lowroom = y[i], rng - pred, pred
        room = (highroom if highroom < lowroom else lowroom) * 2
        if val:
            step2[lo] = step2[hi] = step2[i] = True
            if val >= room:
                v = val - lowroom + pred if highroom > lowroom else pred - val + highroom - 1
            else:
                v = pred - (val + 1) // 2 if val & 1 else pred + val // 2
        else:
            v = pred
        final[i] = min(max(v, 0), rng - 1)
    return final, step2


def floor1_curve(f, final, step2, n2):
    """the integer curve: [n2] table indices"""
    out = np.zeros(n2, np.int64)
    lx, ly = 0, final[f.sorted[0]] * f.multiplier
    hx = 0
    for k in range(1, len(f.x)):
        j = f.sorted[k]
        if not step2[j]:
            continue
        hy, hx = final[j] * f.multiplier, f.x[j]
        dy, adx = hy - ly, hx - lx
        kk = np.arange(0, min(hx, n2) - lx, dtype=np.int64)
        if len(kk):
            base = int(dy / adx)  # toward zero
            ady = abs(dy) - abs(base) * adx
            out[lx:lx + len(kk)] = ly + base * kk + (-1 if dy < 0 else 1) * (kk * ady // adx)
        lx, ly = hx, hy
        if lx >= n2:
            break
    if lx < n2:
        out[lx:] = ly
    return np.clip(out, 0, 255)


def residue_decode(s, r, b, n_vec, vec_len, dnd, dtype):
    """the specification's 8.6.2 for n_vec vectors of vec_len -> [n_vec][vec_len]"""
    v = np.zeros((n_vec, vec_len), dtype)
    lb, le = min(r.begin, vec_len), min(r.end, vec_len)
    cb = s.books[r.classbook]
    cw, ps = cb.dims, r.partition_size
    parts = (le - lb) // ps
    if parts == 0 or all(dnd):
        return v
    cls = np.zeros((n_vec, parts + cw), np.int64)
    with np.errstate(all="ignore"):
        for pas in range(8):
            pc = 0
            while pc < parts:
                if pas == 0:
                    for j in range(n_vec):
                        if dnd[j]:
                            continue
                        t = cb.decode(b)
                        if t is None:
                            return v
                        for i in range(cw - 1, -1, -1):
                            cls[j, i + pc] = t % r.classifications
                            t //= r.classifications
                for _ in range(cw):
                    if pc >= parts:
                        break
                    for j in range(n_vec):
                        if dnd[j]:
                            continue
                        book = r.books[cls[j, pc]][pas]
                        if book < 0:
                            continue
                        bk = s.books[book]
                        tab, off = bk.vq_table(dtype), lb + pc * ps
                        if r.type == 0:
                            step = ps // bk.dims
                            for i in range(step):
                                e = bk.decode(b)
                                if e is None:
                                    return v
                                v[j, off + i:off + i + step * bk.dims:step] += tab[e]
                        else:
                            for i in range(0, ps, bk.dims):
                                e = bk.decode(b)
                                if e is None:
                                    return v
                                v[j, off + i:off + i + bk.dims] += tab[e]
                    pc += 1
    return v


def packet_header(s, p):
    """-> (status, mode, blockflag, prev, next, n, the reader behind the header)"""
    b = Bits(p)
    t = b.read(1)
    if t is None:
        return ST_SHORT, 0, 0, 0, 0, 0, b
    if t:
        return ST_NOT_AUDIO, 0, 0, 0, 0, 0, b
    mode = b.read(ilog(len(s.modes) - 1))
    if mode is None:
        return ST_SHORT, 0, 0, 0, 0, 0, b
    if mode >= len(s.modes):
        return ST_BAD_MODE, mode, 0, 0, 0, 0, b
    flag = s.modes[mode][0]
    prv = nxt = 0
    if flag:
        prv, nxt = b.read(1), b.read(1)
        if nxt is None:
            return ST_SHORT, mode, flag, 0, 0, 0, b
    return ST_OK, mode, flag, prv, nxt, s.bs[flag], b


def entropy_decode(s, p, dtype=np.float32):
    """the entropy stage of one packet -> Staged(status, mode, blockflag, prev, next, n, used[ch], final_y[ch][65], step2[ch][65],
    residue[ch][n/2])"""
    o = Staged()
    o.status, o.mode, o.blockflag, o.prev, o.next, o.n, b = packet_header(s, p)
    ch = s.channels
    o.used, o.final_y, o.step2 = [0] * ch, np.zeros((ch, 65), np.int32), np.zeros((ch, 65), np.uint8)
    o.residue = np.zeros((ch, o.n // 2), dtype)
    if o.status != ST_OK:
        return o
    m = s.mappings[s.modes[o.mode][1]]
    n2 = o.n // 2
    for c in range(ch):
        f = s.floors[m.floor[m.mux[c]]]
        y = None if b.eop else floor1_decode(s, f, b)
        if y is not None:
            fy, st = floor1_unwrap(f, y)
            o.used[c] = 1
            o.final_y[c, :len(fy)], o.step2[c, :len(fy)] = fy, st
    no_res = [not u for u in o.used]
    for mag, ang in m.coupling:
        if not (no_res[mag] and no_res[ang]):
            no_res[mag] = no_res[ang] = False
    for sm in range(m.submaps):
        chans = [c for c in range(ch) if m.mux[c] == sm]
        if not chans:
            continue
        r = s.residues[m.residue[sm]]
        dnd = [no_res[c] for c in chans]
        if r.type == 2:
            if all(dnd):
                continue
            v = residue_decode(s, r, b, 1, n2 * len(chans), [False], dtype)
            for k, c in enumerate(chans):
                o.residue[c] = v[0, k::len(chans)]
        else:
            v = residue_decode(s, r, b, len(chans), n2, dnd, dtype)
            for k, c in enumerate(chans):
                o.residue[c] = v[k]
    return o


def spectrum(s, o, dtype):
    """inverse coupling, floor curve, product -> [ch][n/2]"""
    m = s.mappings[s.modes[o.mode][1]]
    res = o.residue.astype(dtype).copy()
    with np.errstate(all="ignore"):
        for mag, ang in reversed(m.coupling):
            M, A = res[mag].copy(), res[ang].copy()
            nm = np.where(M > 0, np.where(A > 0, M, M + A), np.where(A > 0, M, M - A))
            na = np.where(M > 0, np.where(A > 0, M - A, M), np.where(A > 0, M + A, M))
            res[mag], res[ang] = nm, na
        table = inverse_db(dtype)
        out = np.zeros_like(res)
        for c in range(s.channels):
            if o.used[c]:
                f = s.floors[m.floor[m.mux[c]]]
                out[c] = table[floor1_curve(f, list(o.final_y[c]), list(o.step2[c]), o.n // 2)] * res[c]
    return out


def fft_radix2(x, dtype):
    """forward DFT of a power-of-two length in complex arithmetic of dtype: decimation in time, twiddles rounded from float64"""
    cd = np.complex64 if dtype == np.float32 else np.complex128
    n = len(x)
    bits = n.bit_length() - 1
    idx = np.arange(n)
    rev = np.zeros(n, np.int64)
    for k in range(bits):
        rev |= ((idx >> k) & 1) << (bits - 1 - k)
    a = np.asarray(x, cd)[rev]
    half = 1
    while half < n:
        w = np.exp(-2j * np.pi * np.arange(half) / (2 * half)).astype(cd)
        a = a.reshape(-1, 2 * half)
        t = a[:, half:] * w
        a = np.concatenate([a[:, :half] + t, a[:, :half] - t], axis=1)
        half *= 2
    return a.reshape(n)


def imdct(X, dtype):
    """y[m] = sum_k X[k] cos(pi / (2 N) (2 m + 1 + N / 2) (2 k + 1)), N = 2 len(X), through an N / 4 point complex FFT"""
    cd = np.complex64 if dtype == np.float32 else np.complex128
    M = len(X)
    N, n4 = 2 * M, M // 2
    X = np.asarray(X, dtype)
    tw = np.exp(-1j * np.pi * (8 * np.arange(n4) + 1) / (8 * M)).astype(cd)
    with np.errstate(all="ignore"):
        t = (X[0::2] + 1j * X[::-1][0::2]).astype(cd) * tw
        T = np.fft.fft(t) if dtype == np.float64 else fft_radix2(t, dtype)
        v = (T * tw).astype(cd)
    u = np.zeros(M, dtype)
    u[0::2] = v.real
    u[::-1][0::2] = -v.imag
    y = np.empty(N, dtype)
    y[:n4] = u[n4:]
    y[n4:3 * n4] = -u[::-1]
    y[3 * n4:] = -u[:n4]
    return y


def imdct_direct(X):
    M = len(X)
    N = 2 * M
    m, k = np.arange(N)[:, None], np.arange(M)[None, :]
    return (np.cos(np.pi / (2 * N) * (2 * m + 1 + N / 2) * (2 * k + 1)) * np.asarray(X, np.float64)).sum(axis=1)


def slope(n, dtype):
    """the rising half of the Vorbis window of length 2 n"""
    i = np.arange(n)
    return np.sin(np.pi / 2 * np.sin((i + 0.5) / (2 * n) * np.pi) ** 2).astype(np.float32).astype(dtype)


def window(s, blockflag, prv, nxt, dtype):
    n = s.bs[blockflag]
    ln = s.bs[1 if (blockflag and prv) else 0] // 2
    rn = s.bs[1 if (blockflag and nxt) else 0] // 2
    w = np.zeros(n, dtype)
    ls, rs = n // 4 - ln // 2, 3 * n // 4 - rn // 2
    w[ls:ls + ln] = slope(ln, dtype)
    w[ls + ln:rs] = 1
    w[rs:rs + rn] = slope(rn, dtype)[::-1]
    return w


def to_s16(x):
    """lewton's rule, established from the recording (tests/golden/vorbis/README.md): x * 32768, saturated, truncated toward zero"""
    with np.errstate(all="ignore"):
        v = np.asarray(x, np.float32).astype(np.float64) * 32768.0
        v = np.where(np.isnan(v), 0.0, v)
    return np.trunc(np.clip(v, -32768.0, 32767.0)).astype(np.int16)


class Stream:
    """the overlap state of one stream and the whole packet decode in one dtype"""

    def __init__(self, setup, dtype=np.float64):
        self.s, self.dtype, self.prev, self.prev_n = setup, dtype, None, 0

    def decode(self, p):
        """-> (status, [ch][samples] of dtype or None)"""
        o = entropy_decode(self.s, p, self.dtype)
        if o.status != ST_OK:
            return o.status, None
        spec = spectrum(self.s, o, self.dtype)
        w = window(self.s, o.blockflag, o.prev, o.next, self.dtype)
        with np.errstate(all="ignore"):
            y = np.stack([imdct(spec[c], self.dtype) * w for c in range(self.s.channels)])
        n = o.n
        left, right = y[:, :n // 2], y[:, n // 2:]
        out = None
        if self.prev is not None:
            pn = self.prev_n
            if pn == n:
                out = self.prev + left
            elif pn > n:
                a = pn // 4 - n // 4
                out = np.concatenate([self.prev[:, :a], self.prev[:, a:a + n // 2] + left], axis=1)
            else:
                a = n // 4 - pn // 4
                out = np.concatenate([self.prev + left[:, a:a + pn // 2], left[:, a + pn // 2:]], axis=1)
        else:
            out = np.zeros((self.s.channels, 0), self.dtype)
        self.prev, self.prev_n = right.copy(), n
        return ST_OK, out


def decode_ogg(data, dtype=np.float64):
    """VorbisDecoder over a whole file -> (ident, [ch][samples] of dtype), with the reference's granule truncation"""
    pk = ogg_packets(data)
    ident = parse_ident(pk[0]["data"])
    parse_comment(pk[1]["data"])
    s = parse_setup(pk[2]["data"], ident["channels"], ident["blocksize_0"], ident["blocksize_1"])
    st, out, absgp = Stream(s, dtype), [], None
    for p in pk[3:]:
        status, pcm = st.decode(p["data"])
        if status != ST_OK:
            raise VorbisError("packet status %d" % status)
        if absgp is not None and p["last_in_stream"] and p["granule_position"] is not None:
            pcm = pcm[:, :max(p["granule_position"] - absgp, 0)]
        if p["last_in_page"]:
            if p["granule_position"] is not None:
                absgp = p["granule_position"]
        elif absgp is not None:
            absgp += pcm.shape[1]
        out.append(pcm)
    return ident, s, np.concatenate(out, axis=1)

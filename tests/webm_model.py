"""The WebM / Matroska audio demuxer stated in Python, for the tests: what soundkit-webm's WebmAudioDemuxer makes of a whole file.
demux(data) -> (events, error): events are ("config", dict) and ("packet", dict) in order, error is the refusal's text or None.
An element is parsed once all of it is there, so the result does not depend on how the bytes arrive (the per-call budget aside)."""
import math
import struct

AUDIO_IDS = ("A_OPUS", "A_VORBIS", "A_AAC", "A_FLAC", "A_ALAC")
VIDEO_IDS = ("V_VP9", "V_AV1", "V_MPEG4/ISO/AVC", "V_MPEGH/ISO/HEVC")
BLOCKS = (0xA3, 0xA1, 0xA0)


class Refused(Exception):
    pass


def vint(d, at):
    """-> (value, length) or None"""
    if at >= len(d) or d[at] == 0:
        return None
    n = 9 - d[at].bit_length()
    if at + n > len(d):
        return None
    v = d[at] & (0xff >> n) if n < 8 else 0
    for b in d[at + 1:at + n]:
        v = v << 8 | b
    return v, n


def elem_id(d, at):
    if at >= len(d) or d[at] == 0:
        return None
    n = 9 - d[at].bit_length()
    if n > 4 or at + n > len(d):
        return None
    return int.from_bytes(d[at:at + n], "big"), n


def uint(b):
    return int.from_bytes(b[:8], "big")


def flt(b):
    return struct.unpack(">f", b)[0] if len(b) == 4 else struct.unpack(">d", b)[0] if len(b) == 8 else 0.0


def rust_round(v):
    """f64::round: half away from zero"""
    a = abs(v)
    if a >= 2 ** 52:
        return int(v)
    whole = math.floor(a)
    return (whole + (1 if a - whole >= 0.5 else 0)) * (1 if v >= 0 else -1)


def children(d, truncated):
    """the children of a master that is all there -> [(id, payload)]"""
    out, at = [], 0
    while at + 2 <= len(d):
        i = elem_id(d, at)
        s = i and vint(d, at + i[1])
        if not s:
            break
        start = at + i[1] + s[1]
        if start + s[0] > len(d):
            raise Refused(truncated)
        out.append((i[0], d[start:start + s[0]]))
        at = start + s[0]
    return out


def bounded(i, size):
    budget = 64 << 20 if i in BLOCKS else 16 << 20
    if size > budget:
        raise Refused("WebM element 0x%X exceeds the %d byte budget" % (i, budget))


def check_ebml(d):
    v = {0x42F7: 1, 0x42F2: 4, 0x42F3: 8, 0x4285: 1}
    doc = None
    for i, p in children(d, "truncated WebM track settings"):
        if i in v:
            v[i] = uint(p)
        elif i == 0x4282:
            doc = p.decode("utf-8", "replace")
    if v[0x42F7] > 1:
        raise Refused("unsupported EBML read version %d" % v[0x42F7])
    if v[0x42F2] > 4 or v[0x42F3] > 8:
        raise Refused("unsupported EBML element width")
    if doc is None:
        raise Refused("WebM EBML header is missing DocType")
    if doc not in ("webm", "matroska"):
        raise Refused("unsupported EBML DocType %s" % doc)
    if v[0x4285] > 4:
        raise Refused("unsupported Matroska DocTypeReadVersion %d" % v[0x4285])


def content_encodings(d):
    prefix, at = None, 0
    while at + 2 <= len(d):
        i = elem_id(d, at)
        if not i:
            raise Refused("invalid WebM ContentEncodings element")
        s = vint(d, at + i[1])
        if not s:
            raise Refused("truncated WebM ContentEncodings size")
        start = at + i[1] + s[1]
        if start + s[0] > len(d):
            raise Refused("truncated WebM ContentEncoding")
        at = start + s[0]
        if i[0] != 0x6240:
            continue
        if prefix is not None:
            raise Refused("multiple Matroska ContentEncodings are unsupported")
        scope, kind, comp = 1, 0, None
        for j, p in children(d[start:at], "truncated WebM track settings"):
            if j == 0x5032:
                scope = uint(p)
            elif j == 0x5033:
                kind = uint(p)
            elif j == 0x5034:
                comp = p
        if kind != 0:
            raise Refused("encrypted Matroska ContentEncoding is unsupported")
        if not scope & 1:
            raise Refused("Matroska ContentEncoding does not apply to frame data")
        if comp is None:
            raise Refused("Matroska ContentEncoding has no compression settings")
        algo, settings = 0, None
        for j, p in children(comp, "truncated WebM track settings"):
            if j == 0x4254:
                algo = uint(p)
            elif j == 0x4255:
                settings = p
        if algo != 3:
            raise Refused("unsupported Matroska ContentCompAlgo %d; only header stripping is supported" % algo)
        if settings is None:
            raise Refused("Matroska header stripping has no prefix bytes")
        prefix = bytes(settings)
    if prefix is None:
        raise Refused("empty Matroska ContentEncodings is unsupported")
    return prefix


def track_entry(d):
    t = dict(number=None, kind=None, codec_id="", private=b"", rate=None, channels=None, default_duration=None, codec_delay=0, seek_pre_roll=0, scale=1.0,
             prefix=b"")
    for i, p in children(d, "truncated WebM TrackEntry"):
        if i == 0xD7:
            t["number"] = uint(p)
        elif i == 0x83:
            t["kind"] = {2: "audio", 1: "video"}.get(uint(p))
        elif i == 0x86:
            t["codec_id"] = p.decode("utf-8", "replace")
        elif i == 0x63A2:
            t["private"] = bytes(p)
        elif i == 0x23E383:
            t["default_duration"] = uint(p) or None
        elif i == 0x56AA:
            t["codec_delay"] = uint(p)
        elif i == 0x56BB:
            t["seek_pre_roll"] = uint(p)
        elif i == 0x23314F:
            t["scale"] = flt(p)
            if not math.isfinite(t["scale"]) or t["scale"] <= 0:
                raise Refused("WebM TrackTimestampScale must be finite and positive")
        elif i == 0x6D80:
            t["prefix"] = content_encodings(p)
        elif i == 0xE1:
            for j, q in children(p, "truncated WebM track settings"):
                if j == 0xB5:
                    r = flt(q)
                    if math.isfinite(r) and 0 < r <= 0xffffffff:
                        t["rate"] = rust_round(r)
                elif j == 0x9F and 0 < uint(q) <= 255:
                    t["channels"] = uint(q)
        elif i == 0xE0:
            children(p, "truncated WebM track settings")
    if t["number"] is None or t["kind"] is None:
        return None
    return t if t["codec_id"] in (AUDIO_IDS if t["kind"] == "audio" else VIDEO_IDS) else None


def opus_duration(f):
    if not f:
        return None
    cfg = f[0] >> 3
    us = (10000, 20000, 40000, 60000)[cfg & 3] if cfg < 12 else (10000, 20000)[cfg & 1] if cfg < 16 else (2500, 5000, 10000, 20000)[cfg & 3]
    if f[0] & 3 == 3:
        if len(f) < 2:
            return None
        count = f[1] & 0x3f
    else:
        count = 1 if f[0] & 3 == 0 else 2
    return us * count * 1000 if count > 0 and us * count <= 120000 else None


def unlace(flags, d):
    """a block's payload -> its frames"""
    lacing = flags & 6
    if lacing == 0:
        return [d]
    name = {2: "Xiph", 4: "fixed", 6: "EBML"}[lacing]
    if not d:
        raise Refused("Truncated %s-laced block" % name)
    count, at, sizes = d[0] + 1, 1, []
    if lacing == 2:
        for _ in range(count - 1):
            size = 0
            while True:
                if at >= len(d):
                    raise Refused("Truncated Xiph lacing size")
                size, at = size + d[at], at + 1
                if d[at - 1] != 255:
                    break
            sizes.append(size)
        if sum(sizes) > len(d) - at:
            raise Refused("Xiph-laced frame sizes exceed block payload")
        sizes.append(len(d) - at - sum(sizes))
    elif lacing == 4:
        if (len(d) - 1) % count:
            raise Refused("Invalid fixed-laced block size")
        sizes = [(len(d) - 1) // count] * count
    else:
        first = vint(d, at)
        if not first:
            raise Refused("Truncated EBML-laced first frame size")
        at += first[1]
        sizes.append(first[0])
        for _ in range(1, count - 1):
            delta = vint(d, at)
            if not delta:
                raise Refused("Truncated EBML-laced frame size delta")
            at += delta[1]
            size = sizes[-1] + delta[0] - ((1 << (7 * delta[1] - 1)) - 1)
            if size >= 1 << 63:
                raise Refused("EBML-laced frame size overflow")
            if size < 0:
                raise Refused("Negative EBML-laced frame size")
            sizes.append(size)
        if sum(sizes) > len(d) - at:
            raise Refused("EBML-laced frame sizes exceed block payload")
        sizes.append(len(d) - at - sum(sizes))  # also behind a single listed size
    frames = []
    for s in sizes:
        if at + s > len(d):
            raise Refused("Laced frame extends past block payload")
        frames.append(d[at:at + s])
        at += s
    if at != len(d):
        raise Refused("Laced frame sizes do not consume block payload")
    return frames


class Model:
    def __init__(self):
        self.tracks, self.events, self.scale_ns, self.cluster, self.configured = [], [], 1000000, 0, False

    def block(self, d, duration_ticks=None, discard=None):
        n = vint(d, 0)
        if not n:
            raise Refused("invalid WebM block track number")
        if len(d) < n[1] + 3:
            raise Refused("truncated WebM block header")
        t = next((t for t in self.tracks if t["number"] == n[0]), None)
        if t is None:
            return
        ticks = self.cluster + struct.unpack(">h", d[n[1]:n[1] + 2])[0]
        if not -(1 << 63) <= ticks < 1 << 63:
            raise Refused("WebM block timestamp overflow")
        v = float(ticks) * float(self.scale_ns) * t["scale"]
        if not math.isfinite(v) or abs(v) > 2.0 ** 63:
            raise Refused("WebM nanosecond timestamp overflow")
        stamp = min(rust_round(v), (1 << 63) - 1)
        if t["codec_delay"] >= 1 << 63:
            raise Refused("WebM CodecDelay exceeds the signed timeline range")
        stamp -= t["codec_delay"]
        if stamp < -(1 << 63):
            raise Refused("WebM CodecDelay timestamp underflow")
        frames = unlace(d[n[1] + 2], d[n[1] + 3:])
        declared = t["default_duration"]
        if duration_ticks is not None:
            v = float(duration_ticks) * float(self.scale_ns) * t["scale"]
            if not math.isfinite(v) or v > 2.0 ** 64:
                raise Refused("WebM BlockDuration overflow")
            declared = min(rust_round(v), (1 << 64) - 1) // len(frames)
        durations = [declared if declared is not None else opus_duration(f) if t["codec_id"] == "A_OPUS" else None for f in frames]
        if len(frames) > 1 and None in durations:
            raise Refused("laced WebM %s timing cannot be resolved deterministically" % t["codec_id"])
        offset = 0
        for k, f in enumerate(frames):
            if not f:
                continue
            if offset >= 1 << 63 or stamp + offset >= 1 << 63:
                raise Refused("WebM laced frame timestamp overflow")
            if t["kind"] == "audio":
                self.events.append(("packet", dict(track=n[0], codec_id=t["codec_id"], data=t["prefix"] + bytes(f), timestamp_ns=stamp + offset,
                                                   duration_ns=durations[k], discard_padding_ns=discard if k + 1 == len(frames) else None)))
            if durations[k] is not None:
                offset += durations[k]
                if offset >= 1 << 64:
                    raise Refused("WebM laced duration overflow")

    def block_group(self, d):
        block = duration = discard = None
        for i, p in children(d, "truncated WebM BlockGroup"):
            if i == 0xA1:
                block = p
            elif i == 0x9B:
                duration = uint(p)
            elif i == 0x75A2:
                if not 1 <= len(p) <= 8:
                    raise Refused("invalid WebM signed integer size")
                discard = int.from_bytes(p, "big", signed=True)
        if block is not None:
            self.block(block, duration, discard)

    def run(self, d):
        """-> the bytes left unconsumed"""
        if len(d) < 4:
            return len(d)
        i = elem_id(d, 0)
        if not i:
            raise Refused("invalid WebM EBML element ID")
        if i[0] != 0x1A45DFA3:
            raise Refused("invalid WebM: expected EBML header, got 0x%X" % i[0])
        s = vint(d, i[1])
        if not s:
            return len(d)
        bounded(i[0], s[0])
        at = i[1] + s[1] + s[0]
        if len(d) < at:
            return len(d)
        check_ebml(d[i[1] + s[1]:at])
        seg = elem_id(d, at)
        if not seg:
            return len(d)
        if seg[0] != 0x18538067:
            raise Refused("invalid WebM: expected Segment, got 0x%X" % seg[0])
        s = vint(d, at + seg[1])
        if not s:
            return len(d)
        at += seg[1] + s[1]
        while at + 2 <= len(d):
            i = elem_id(d, at)
            s = i and vint(d, at + i[1])
            if not s:
                break
            head = i[1] + s[1]
            if i[0] == 0x1F43B675:
                if not self.configured:
                    if not self.tracks:
                        raise Refused("WebM source has no supported media track")
                    self.configured = True
                    self.events += [("config", dict(t, timecode_scale_ns=self.scale_ns, rate=t["rate"] or 48000, channels=t["channels"] or 2))
                                    for t in self.tracks if t["kind"] == "audio"]
                self.cluster = 0
                at += head
                continue
            if not self.configured and (i[0] == 0x1654AE6B or (i[0] == 0x18538067 and s[0] == (1 << (7 * s[1])) - 1)):
                at += head
                continue
            bounded(i[0], s[0])
            if at + head + s[0] > len(d):
                break
            p = d[at + head:at + head + s[0]]
            if not self.configured:
                if i[0] == 0xAE:
                    t = track_entry(p)
                    if t and all(o["number"] != t["number"] for o in self.tracks):
                        self.tracks.append(t)
                elif i[0] == 0x1549A966:
                    for j, q in children(p, "truncated WebM track settings"):
                        if j == 0x2AD7B1:
                            self.scale_ns = uint(q)
                    if self.scale_ns == 0:
                        raise Refused("WebM TimecodeScale must be positive")
            elif i[0] == 0xE7:
                self.cluster = uint(p)
                if self.cluster >= 1 << 63:
                    raise Refused("WebM cluster timecode exceeds i64")
            elif i[0] in (0xA3, 0xA1):
                self.block(p)
            elif i[0] == 0xA0:
                self.block_group(p)
            at += head + s[0]
        return len(d) - at


def demux(data):
    m = Model()
    try:
        left = m.run(bytes(data))
        if left:
            raise Refused("truncated WebM element: %d buffered bytes remain" % left)
        if not any(kind == "config" for kind, _ in m.events):
            raise Refused("WebM source has no supported audio track")
    except Refused as e:
        return m.events, str(e)
    return m.events, None

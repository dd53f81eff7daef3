"""A plain-Python reading of ISO base media files (ISO/IEC 14496-12, -14 and Apple's ALAC-in-MP4 note), audio only: the first audio track
whose sample entry is `mp4a` or `alac`, its sample table or its fragments, the first media edit and what it leaves of a decoded packet, and
the ADTS header an AAC sample is wrapped in.  Written from the format, whole files only; csrc/mp4_stream.h is checked against it."""
import struct

RATES = [96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 7350]
CONTAINERS = (b"edts", b"mdia", b"minf", b"stbl")


def boxes(data, start=0, end=None):
    """(name, payload start, box end) of every whole box in data[start:end]"""
    end = len(data) if end is None else end
    at = start
    while end - at >= 8:
        size, name = struct.unpack_from(">I4s", data, at)
        head = 8
        if size == 1:
            if end - at < 16:
                return
            size, head = struct.unpack_from(">Q", data, at + 8)[0], 16
        if size < head or at + size > end:
            return
        yield name, at + head, at + size
        at += size


def descriptor(data, at, end, tag):
    """the body of the first descriptor `tag` in data[at:end], looking inside ES (3) and DecoderConfig (4) descriptors"""
    while end - at >= 2:
        t, at = data[at], at + 1
        n = 0
        for _ in range(4):
            b, at = data[at], at + 1
            n = n << 7 | b & 0x7f
            if not b & 0x80:
                break
        body_end = at + n
        assert body_end <= end, "descriptor runs past its box"
        if t == tag:
            return data[at:body_end]
        skip = {3: 3, 4: 13}.get(t, 0)
        if skip and n >= skip:
            found = descriptor(data, at + skip, body_end, tag)
            if found is not None:
                return found
        at = body_end
    return None


def sample_entry(data, at, end):
    """stsd payload -> dict for the first mp4a / alac entry, or None"""
    count = struct.unpack_from(">I", data, at + 4)[0]
    entries = list(boxes(data, at + 8, end))[:count]
    for name, p, e in entries:
        if name not in (b"mp4a", b"alac"):
            continue
        version, = struct.unpack_from(">H", data, p + 8)
        channels, bits = struct.unpack_from(">HH", data, p + 16)
        rate = struct.unpack_from(">I", data, p + 24)[0] >> 16
        kids = p + {0: 28, 1: 44}[version]
        out = {"codec": "aac" if name == b"mp4a" else "alac", "sample_rate": rate, "channels": channels, "private": b""}
        for kid, kp, ke in boxes(data, kids, e):
            if name == b"mp4a" and kid == b"esds":
                asc = descriptor(data, kp + 4, ke, 5) or b""
                out["private"] = bytes(asc)
                if len(asc) >= 2:
                    index = (asc[0] & 7) << 1 | asc[1] >> 7
                    if index < 13:
                        out["sample_rate"], out["channels"] = RATES[index], asc[1] >> 3 & 15
            if name == b"alac" and kid == b"alac":
                out["private"] = bytes(data[kp:ke])
        return out
    return None


def parse_trak(data, at, end, movie_timescale):
    t = {"audio": False, "entry": None, "edit": None, "stts": [], "stsc": [], "sizes": [], "chunks": []}

    def walk(a, e):
        for name, p, q in boxes(data, a, e):
            if name in CONTAINERS:
                walk(p, q)
            elif name == b"tkhd":
                t["track_id"] = struct.unpack_from(">I", data, p + (20 if data[p] == 1 else 12))[0]
            elif name == b"mdhd":
                t["timescale"] = struct.unpack_from(">I", data, p + (20 if data[p] == 1 else 12))[0]
            elif name == b"hdlr":
                t["audio"] = t["audio"] or data[p + 8:p + 12] == b"soun"
            elif name == b"elst":
                n = struct.unpack_from(">I", data, p + 4)[0]
                empty = 0
                for k in range(n):
                    if data[p] == 1:
                        duration, media = struct.unpack_from(">Qq", data, p + 8 + 20 * k)
                    else:
                        duration, media = struct.unpack_from(">Ii", data, p + 8 + 12 * k)
                    if media == -1:
                        empty += duration
                        continue
                    t["edit"] = (empty, media, duration)  # movie timescale; rescaled below
                    break
            elif name == b"stsd":
                t["entry"] = sample_entry(data, p, q)
            elif name == b"stts":
                n = struct.unpack_from(">I", data, p + 4)[0]
                t["stts"] = [struct.unpack_from(">II", data, p + 8 + 8 * k) for k in range(n)]
            elif name == b"stsc":
                n = struct.unpack_from(">I", data, p + 4)[0]
                t["stsc"] = [struct.unpack_from(">III", data, p + 8 + 12 * k) for k in range(n)]
            elif name == b"stsz":
                size, n = struct.unpack_from(">II", data, p + 4)
                t["sizes"] = [size] * n if size else list(struct.unpack_from(">%dI" % n, data, p + 12))
            elif name == b"stco":
                n = struct.unpack_from(">I", data, p + 4)[0]
                t["chunks"] = list(struct.unpack_from(">%dI" % n, data, p + 8))
            elif name == b"co64":
                n = struct.unpack_from(">I", data, p + 4)[0]
                t["chunks"] = list(struct.unpack_from(">%dQ" % n, data, p + 8))

    walk(at, end)
    if not t["audio"] or t["entry"] is None:
        return None
    track = dict(t["entry"], track_id=t["track_id"], timescale=t["timescale"], edit=None)
    if t["edit"]:
        scale = lambda v: (v * t["timescale"] + movie_timescale // 2) // movie_timescale
        track["edit"] = (scale(t["edit"][0]), t["edit"][1], scale(t["edit"][2]))  # (presentation start, media start, duration)
    durations = [d for n, d in t["stts"] for _ in range(n)]
    samples, k, time = [], 0, 0
    for c, offset in enumerate(t["chunks"]):
        per = [e for e in t["stsc"] if e[0] <= c + 1][-1][1]
        for _ in range(per):
            if k == len(t["sizes"]):
                break
            samples.append((offset, t["sizes"][k], durations[k], time))
            offset += t["sizes"][k]
            time += durations[k]
            k += 1
    track["samples"] = samples  # (offset, size, duration, start)
    track["fragmented"] = not samples
    return track


def parse_moov(data, at, end):
    """-> (track, {track id: (default duration, default size)})"""
    movie_timescale, trex, track, mvex = 0, {}, None, False
    for name, p, q in boxes(data, at, end):
        if name == b"mvhd":
            movie_timescale = struct.unpack_from(">I", data, p + (20 if data[p] == 1 else 12))[0]
        if name == b"mvex":
            mvex = True
            for kid, kp, _ in boxes(data, p, q):
                if kid == b"trex":
                    tid, _, duration, size = struct.unpack_from(">IIII", data, kp + 4)
                    trex[tid] = (duration, size)
    for name, p, q in boxes(data, at, end):
        if name == b"trak" and track is None:
            track = parse_trak(data, p, q, movie_timescale)
    if track is not None and mvex:
        track["fragmented"] = True
    return track, trex


def fragment_samples(data, track, trex):
    """the track's samples in every moof of the file, (offset, size, duration, start)"""
    out = []
    for name, p, q in boxes(data):
        if name != b"moof":
            continue
        moof_start = p - 8
        inherited = None
        for kid, kp, kq in boxes(data, p, q):
            if kid != b"traf":
                continue
            base = duration = size = None
            tid, time, base_is_moof, runs = 0, 0, False, []
            for leaf, lp, lq in boxes(data, kp, kq):
                if leaf == b"tfhd":
                    flags = struct.unpack_from(">I", data, lp)[0] & 0xffffff
                    tid = struct.unpack_from(">I", data, lp + 4)[0]
                    a = lp + 8
                    if flags & 1:
                        base, a = struct.unpack_from(">Q", data, a)[0], a + 8
                    if flags & 2:
                        a += 4
                    if flags & 8:
                        duration, a = struct.unpack_from(">I", data, a)[0], a + 4
                    if flags & 0x10:
                        size = struct.unpack_from(">I", data, a)[0]
                    base_is_moof = bool(flags & 0x20000)
                elif leaf == b"tfdt":
                    time = struct.unpack_from(">Q" if data[lp] == 1 else ">I", data, lp + 4)[0]
                elif leaf == b"trun":
                    runs.append((lp, lq))
            d_duration, d_size = trex.get(tid, (0, 0))
            duration = duration if duration is not None else (d_duration or None)
            size = size if size is not None else (d_size or None)
            if base is None:
                base = moof_start if base_is_moof or inherited is None else inherited
            at = base
            for lp, lq in runs:
                flags = struct.unpack_from(">I", data, lp)[0] & 0xffffff
                n = struct.unpack_from(">I", data, lp + 4)[0]
                a = lp + 8
                if flags & 1:
                    at, a = base + struct.unpack_from(">i", data, a)[0], a + 4
                if flags & 4:
                    a += 4
                for _ in range(n):
                    d, s = duration, size
                    if flags & 0x100:
                        d, a = struct.unpack_from(">I", data, a)[0], a + 4
                    if flags & 0x200:
                        s, a = struct.unpack_from(">I", data, a)[0], a + 4
                    a += 4 * (bool(flags & 0x400) + bool(flags & 0x800))
                    if tid == track["track_id"]:
                        out.append((at, s, d, time))
                        time += d
                    at += s
            inherited = at
    return sorted(out)


def index(data):
    """-> the track with its samples (a fragmented file's come from its moofs)"""
    data = bytes(data)
    for name, p, q in boxes(data):
        if name == b"moov":
            track, trex = parse_moov(data, p, q)
            assert track is not None, "no audio track"
            if track["fragmented"]:
                track["samples"] = fragment_samples(data, track, trex)
            return track
    raise AssertionError("no moov")


def demux(data):
    """-> (track, [(sample bytes, start, duration)]) in file order"""
    track = index(data)
    order = sorted(track["samples"]) if track["fragmented"] else track["samples"]
    return track, [(bytes(data[o:o + n]), start, duration) for o, n, duration, start in order]


def trim(track, sample, decoded_frames, decoded_rate):
    """(first frame, count) of the decoded packet that the first edit keeps; rounding: start up, end down; nothing: (decoded_frames, 0)"""
    if track["edit"] is None:
        return 0, decoded_frames
    presentation, media, length = track["edit"]
    _, _, duration, start = sample
    p0 = start - media + presentation
    lo, hi = max(p0, presentation), min(p0 + duration, presentation + length)
    if hi <= lo or decoded_frames == 0:
        return decoded_frames, 0
    scale = track["timescale"]
    a = min(-(-(lo - p0) * decoded_rate // scale), decoded_frames)
    b = min((hi - p0) * decoded_rate // scale, decoded_frames)
    return (a, b - a) if b > a else (decoded_frames, 0)


def adts_header(asc, rate, channels, raw_len):
    profile = min(max((asc[0] >> 3) - 1, 0), 3) if asc else 1
    index_ = RATES.index(rate) if rate in RATES else 15
    ch, n = min(channels, 7), raw_len + 7
    return bytes([0xff, 0xf1, profile << 6 | index_ << 2 | ch >> 2, (ch & 3) << 6 | n >> 11 & 3, n >> 3 & 0xff, (n & 7) << 5 | 0x1f, 0xfc])


def adts_bytes(data):
    """the file's AAC samples as one ADTS stream"""
    track, packets = demux(data)
    assert track["codec"] == "aac"
    return b"".join(adts_header(track["private"], track["sample_rate"], track["channels"], len(p)) + p for p, _, _ in packets)

"""A small EBML walker for the tests: the A_VORBIS track of a WebM file -> its three header packets (CodecPrivate, Xiph-laced) and the
audio packets of its SimpleBlocks / Blocks.  No lacing inside blocks, one audio track: what the fixture has; anything else asserts."""

MASTERS = {0x18538067, 0x1654AE6B, 0xAE, 0x1F43B675, 0xA0}  # Segment, Tracks, TrackEntry, Cluster, BlockGroup


def _vint(data, at, keep_marker):
    first = data[at]
    n = 1
    while n <= 8 and not first & (0x80 >> (n - 1)):
        n += 1
    assert n <= 8, "bad EBML variable-length integer"
    v = first if keep_marker else first & (0xff >> n)
    for b in data[at + 1:at + n]:
        v = v << 8 | b
    unknown = not keep_marker and v == (1 << (7 * n)) - 1
    return v, at + n, unknown


def _walk(data, at, end, out):
    while at < end:
        eid, at, _ = _vint(data, at, True)
        size, at, unknown = _vint(data, at, False)
        stop = end if unknown else min(at + size, end)
        if eid in MASTERS:
            _walk(data, at, stop, out)
        elif eid == 0x63A2:
            out["private"] = data[at:stop]
        elif eid == 0x86:
            out["codec"] = data[at:stop]
        elif eid in (0xA3, 0xA1):
            _, body, _ = _vint(data, at, False)
            assert not data[body + 2] & 0x06, "laced blocks are not handled"
            out["packets"].append(data[body + 3:stop])
        at = stop


def xiph_unlace(private):
    n = private[0] + 1
    at, sizes = 1, []
    for _ in range(n - 1):
        s = 0
        while private[at] == 255:
            s += 255
            at += 1
        sizes.append(s + private[at])
        at += 1
    out = []
    for s in sizes:
        out.append(private[at:at + s])
        at += s
    out.append(private[at:])
    return out


def vorbis_track(data):
    """-> ([ident, comment, setup], [audio packets])"""
    out = {"packets": []}
    _walk(data, 0, len(data), out)
    assert out.get("codec") == b"A_VORBIS"
    headers = xiph_unlace(out["private"])
    assert len(headers) == 3
    return headers, out["packets"]

"""A small EBML / Matroska writer for the tests: tracks and blocks with every lacing, known and unknown sizes, BlockGroups with
BlockDuration / ReferenceBlock / DiscardPadding, header stripping, padding elements, video tracks, track numbers of any vint width.
It writes what it is told, valid or not."""
import struct

EBML, SEGMENT, INFO, TIMECODE_SCALE, TRACKS, TRACK_ENTRY, CLUSTER, TIMECODE = 0x1A45DFA3, 0x18538067, 0x1549A966, 0x2AD7B1, 0x1654AE6B, 0xAE, 0x1F43B675, 0xE7
SIMPLE_BLOCK, BLOCK, BLOCK_GROUP, BLOCK_DURATION, REFERENCE_BLOCK, DISCARD_PADDING = 0xA3, 0xA1, 0xA0, 0x9B, 0xFB, 0x75A2
VOID, CUES, TAGS, SEEK_HEAD = 0xEC, 0x1C53BB6B, 0x1254C367, 0x114D9B74
UNKNOWN = object()  # as a size: all ones in eight bytes


def eid(i):
    return i.to_bytes((i.bit_length() + 7) // 8, "big")


def vint(v, width=None):
    """a size or a track number; width None: the shortest that does not read as the unknown size"""
    if width is None:
        width = 1
        while v >= (1 << (7 * width)) - 1:
            width += 1
    assert v < 1 << (7 * width)
    return ((1 << (7 * width)) | v).to_bytes(width, "big")


def svint(v, width=None):
    """the signed delta of EBML lacing"""
    if width is None:
        width = 1
        while not -((1 << (7 * width - 1)) - 1) <= v <= (1 << (7 * width - 1)) - 1:
            width += 1
    return vint(v + (1 << (7 * width - 1)) - 1, width)


def el(i, payload=b"", size=None, size_width=None):
    """one element; size: a declared size other than the payload's, or UNKNOWN"""
    if size is UNKNOWN:
        return eid(i) + b"\x01" + b"\xff" * 7 + payload
    return eid(i) + vint(len(payload) if size is None else size, size_width) + payload


def uint(i, v, width=None):
    return el(i, v.to_bytes(width or max((v.bit_length() + 7) // 8, 1), "big"))


def sint(i, v, width=None):
    width = width or next(w for w in range(1, 9) if -(1 << (8 * w - 1)) <= v < 1 << (8 * w - 1))
    return el(i, v.to_bytes(width, "big", signed=True))


def ebml_header(doc_type=b"webm", read_version=1, max_id=4, max_size=8, doc_read_version=2, extra=b""):
    body = uint(0x4286, 1) + uint(0x42F7, read_version) + uint(0x42F2, max_id) + uint(0x42F3, max_size)
    if doc_type is not None:
        body += el(0x4282, doc_type)
    return el(EBML, body + uint(0x4287, 4) + uint(0x4285, doc_read_version) + extra)


def header_stripping(prefix, algo=3, scope=None, enc_type=None, settings=True):
    comp = uint(0x4254, algo) + (el(0x4255, prefix) if settings else b"")
    body = (uint(0x5032, scope) if scope is not None else b"") + (uint(0x5033, enc_type) if enc_type is not None else b"") + el(0x5034, comp)
    return el(0x6D80, el(0x6240, body))


def track(number, codec_id, kind=2, private=None, rate=None, rate_width=8, channels=None, default_duration=None, codec_delay=None, seek_pre_roll=None,
          scale=None, encodings=b"", extra=b""):
    body = uint(0xD7, number) + uint(0x73C5, number + 1000) + uint(0x83, kind) + el(0x86, codec_id)
    if private is not None:
        body += el(0x63A2, private)
    if default_duration is not None:
        body += uint(0x23E383, default_duration)
    if codec_delay is not None:
        body += uint(0x56AA, codec_delay)
    if seek_pre_roll is not None:
        body += uint(0x56BB, seek_pre_roll)
    if scale is not None:
        body += el(0x23314F, struct.pack(">d", scale))
    body += encodings + extra
    if kind == 2:
        audio = b""
        if rate is not None:
            audio += el(0xB5, struct.pack(">d" if rate_width == 8 else ">f", rate))
        if channels is not None:
            audio += uint(0x9F, channels)
        body += el(0xE1, audio)
    elif kind == 1:
        body += el(0xE0, uint(0xB0, 320) + uint(0xBA, 240))
    return el(TRACK_ENTRY, body)


def lace(frames, lacing):
    """the frames of one block behind its flags byte -> (lacing bits, payload)"""
    if lacing == "none":
        assert len(frames) == 1
        return 0x00, frames[0]
    head = bytes([len(frames) - 1])
    if lacing == "xiph":
        for f in frames[:-1]:
            head += b"\xff" * (len(f) // 255) + bytes([len(f) % 255])
        return 0x02, head + b"".join(frames)
    if lacing == "fixed":
        assert len({len(f) for f in frames}) == 1
        return 0x04, head + b"".join(frames)
    assert lacing == "ebml"
    head += vint(len(frames[0]))
    for a, b in zip(frames[:-1], frames[1:-1]):
        head += svint(len(b) - len(a))
    return 0x06, head + b"".join(frames)


def block_body(number, relative, frames, lacing="none", flags=0x80, number_width=None):
    bits, payload = lace(frames, lacing)
    return vint(number, number_width) + struct.pack(">h", relative) + bytes([flags | bits]) + payload


def simple_block(number, relative, frames, lacing="none", number_width=None):
    return el(SIMPLE_BLOCK, block_body(number, relative, frames, lacing, 0x80, number_width))


def block_group(number, relative, frames, lacing="none", duration=None, reference=None, discard=None, number_width=None, extra=b""):
    body = el(BLOCK, block_body(number, relative, frames, lacing, 0x00, number_width))
    if duration is not None:
        body += uint(BLOCK_DURATION, duration)
    if reference is not None:
        body += sint(REFERENCE_BLOCK, reference)
    if discard is not None:
        body += sint(DISCARD_PADDING, discard)
    return el(BLOCK_GROUP, body + extra)


def cluster(timecode, blocks, unknown=False):
    body = uint(TIMECODE, timecode) + b"".join(blocks)
    return el(CLUSTER, body, UNKNOWN if unknown else None)


def webm(tracks, clusters, timecode_scale=None, unknown_segment=False, before=b"", between=b"", header=None):
    """EBML header + Segment(before, Info, Tracks, clusters joined by `between`)"""
    info = el(INFO, (uint(TIMECODE_SCALE, timecode_scale) if timecode_scale is not None else b"") + el(0x4D80, b"tests") + el(0x5741, b"tests"))
    body = before + info + el(TRACKS, b"".join(tracks)) + between.join(clusters)
    return (ebml_header() if header is None else header) + el(SEGMENT, body, UNKNOWN if unknown_segment else None)


def xiph_private(headers):
    """three Vorbis headers -> an A_VORBIS CodecPrivate"""
    out = bytes([len(headers) - 1])
    for h in headers[:-1]:
        out += b"\xff" * (len(h) // 255) + bytes([len(h) % 255])
    return out + b"".join(headers)

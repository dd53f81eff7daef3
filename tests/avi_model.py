"""A Python restatement of the reference's AVI reader (soundkit-decoder/src/lib.rs:257-570), for the tests: what csrc/avi_stream.h must
hand out for a whole file.  Function for function, with the line ranges; the two places where the incremental walker is its own are marked.

The reference walks the file twice (parse_avi_audio_format, then collect_avi_audio_chunks); the walker sees it once, so this model is one
walk in file order: the events in front of a refusal are those of the chunks in front of it.  `demux(data)` -> (events, error):
("config", {...}) once `hdrl` names the track, ("packet", bytes) per `##wb` chunk of the track; error: the refusal's text or None."""
import struct

MAX_CHUNKS = 1_000_000             # lib.rs:510
MAX_PAYLOAD = 512 * 1024 * 1024    # lib.rs:552
MAX_HEADER = 16 * 1024 * 1024      # the walker's own: what `hdrl` may buffer


class Refused(Exception):
    pass


def looks_like_avi(data):  # lib.rs:257-259
    return data[:4] == b"RIFF" and data[8:12] == b"AVI "


def avi_stream_id(two):  # lib.rs:560-570
    try:
        return int(two.decode("ascii"), 16) if len(two) == 2 and all(chr(b) in "0123456789abcdefABCDEF" for b in two) else None
    except UnicodeDecodeError:
        return None


def for_each_riff_chunk(b, visit):  # lib.rs:502-534
    offset = chunks = 0
    while offset + 8 <= len(b):
        chunks += 1
        if chunks > MAX_CHUNKS:
            raise Refused("AVI chunk count exceeds budget")
        fourcc, length = b[offset:offset + 4], struct.unpack_from("<I", b, offset + 4)[0]
        start = offset + 8
        if start + length > len(b):
            # a truncated LIST still shows the complete chunks it holds; a truncated leaf is skipped (lib.rs:519-526)
            if fourcc == b"LIST" and len(b) - start >= 4:
                visit(fourcc, b[start:])
            return
        visit(fourcc, b[start:start + length])
        offset = start + length + (length & 1)
    if offset < len(b) and any(b[offset:]):
        raise Refused("AVI chunk table has trailing data")


def parse_avi_stream_list(b, stream_index):  # lib.rs:411-448
    found = {"audio": False, "wave": None}

    def visit(fourcc, payload):
        if fourcc == b"strh":
            found["audio"] = payload[:4] == b"auds"
        elif fourcc == b"strf":
            found["wave"] = payload

    for_each_riff_chunk(b, visit)
    if not found["audio"]:
        return None
    wave = found["wave"]
    if wave is None:
        raise Refused("AVI audio stream has no strf format")
    if len(wave) < 16:
        raise Refused("AVI WAVEFORMAT is truncated")
    tag, channels, rate = struct.unpack_from("<HHI", wave, 0)
    if channels == 0 or channels > 255:
        raise Refused("AVI channel count is invalid")
    if rate == 0:
        raise Refused("AVI sample rate is zero")
    return dict(index=stream_index, tag=tag, channels=channels, rate=rate, bits=min(struct.unpack_from("<H", wave, 14)[0], 255))


def demux(data):
    events, state = [], {"format": None, "streams": 0, "total": 0}

    def collect(b, depth):  # collect_avi_audio_chunks, lib.rs:536-558
        if depth > 8:
            raise Refused("AVI record nesting exceeds budget")

        def visit(fourcc, payload):
            if fourcc == b"LIST" and len(payload) >= 4:
                collect(payload[4:], depth + 1)
            elif fourcc[2:] == b"wb" and avi_stream_id(fourcc[:2]) == state["format"]["index"]:
                if state["total"] + len(payload) > MAX_PAYLOAD:
                    raise Refused("AVI audio payload exceeds budget")
                state["total"] += len(payload)
                if payload:  # (the walker hands out no empty packet)
                    events.append(("packet", bytes(payload)))

        for_each_riff_chunk(b, visit)

    def header(payload):  # parse_avi_audio_format's visit of one hdrl list, lib.rs:394-405
        def visit(fourcc, chunk):
            if fourcc == b"LIST" and chunk[:4] == b"strl":
                this_stream = state["streams"]
                state["streams"] += 1
                if state["format"] is None:
                    state["format"] = parse_avi_stream_list(chunk[4:], this_stream)
                    if state["format"] is not None:
                        events.append(("config", dict(state["format"])))

        for_each_riff_chunk(payload, visit)

    def visit_list(kind, payload):
        if kind == b"hdrl" and state["format"] is None:
            if len(payload) > MAX_HEADER:  # the walker's own bound
                raise Refused("AVI hdrl list exceeds the %d byte header budget" % MAX_HEADER)
            header(payload)
        elif kind == b"movi":
            if state["format"] is None:  # the walker's own: it cannot look behind `movi` for a header
                raise Refused("AVI has no audio stream")
            collect(payload, 0)

    def form_chunk(fourcc, payload):  # lib.rs:482-492
        if fourcc == b"LIST":
            if len(payload) < 4:
                raise Refused("AVI LIST type is truncated")
            visit_list(payload[:4], payload[4:])

    try:
        offset = forms = 0  # for_each_avi_riff, lib.rs:450-500
        while offset + 12 <= len(data):
            if data[offset:offset + 4] != b"RIFF":
                if forms:
                    break
                raise Refused("AVI contains data outside a RIFF form")
            forms += 1
            length = struct.unpack_from("<I", data, offset + 4)[0]
            declared_end = offset + 8 + length
            end = min(declared_end, len(data))
            if data[offset + 8:offset + 12] not in (b"AVI ", b"AVIX"):
                raise Refused("invalid AVI RIFF form type")
            for_each_riff_chunk(data[offset + 12:end], form_chunk)
            if declared_end > len(data):
                break
            offset = end + (length & 1)
        if state["format"] is None:  # lib.rs:408
            raise Refused("AVI has no audio stream")
    except Refused as e:
        return events, str(e)
    return events, None

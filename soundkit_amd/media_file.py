"""decode_audio_file: soundkit-decoder's entry point for a complete audio or video file (lib.rs:171-255).  Unlike a stream handed to
`spawn()`, a whole file can be looked through: that is what a MOV / MP4 file whose `moov` lies behind `mdat` needs, and packet codecs such
as ALAC and FLAC-in-MP4.  The reference's tests in the reference's order; AVI, MPEG-PS and MXF are recognised by its magic and refused
as not built."""
from dataclasses import dataclass, field
from typing import Any, List, Optional

from ._lib import SoundkitError

INVALID_INPUT, UNSUPPORTED = -5, -6  # SK_ERR_BAD_STREAM, SK_ERR_UNSUPPORTED


@dataclass
class DecodedAudioFile:
    """container: "mp4" / "caf" / "mpeg-ts" / "webm" / None (whatever `spawn()` detected); selected_track: the container's config
    (Mp4Config, CafIndex, the transport stream's or WebM's config) or None; frames: [AudioData]"""
    container: Optional[str]
    selected_track: Any
    frames: List[Any] = field(default_factory=list)


def looks_like_iso_bmff(data):
    """looks_like_iso_bmff (lib.rs:1283-1303): `ftyp`, `moov` or `mdat` behind at most 15 `free` / `wide` / `skip` boxes in the first 64 KiB"""
    position, limit = 0, min(len(data), 64 * 1024)
    for _ in range(16):
        head = data[position:position + 8]
        if len(head) < 8:
            return False
        size, name = int.from_bytes(head[:4], "big"), bytes(head[4:8])
        if name in (b"ftyp", b"moov", b"mdat"):
            return True
        if name not in (b"free", b"wide", b"skip"):
            return False
        if size < 8 or position + size > limit:
            return False
        position += size
    return False


def looks_like_avi(data):
    return data[:4] == b"RIFF" and data[8:12] == b"AVI "


def looks_like_mpeg_ps(data):
    return data[:4] == b"\0\0\x01\xba"


def looks_like_mpeg_ts(data):
    return any(all(len(data) > prefix + k * stride and data[prefix + k * stride] == 0x47 for k in range(3)) for stride, prefix in ((188, 0), (192, 4)))


def looks_like_mxf(data):
    return bytes(data[:65540]).find(b"\x06\x0e\x2b\x34") >= 0  # the first 65 537 windows of four bytes


def looks_like_ebml(data):
    return data[:4] == b"\x1a\x45\xdf\xa3"


def decode_audio_file(data, options=None, scheduler=None, engine=None):
    """-> DecodedAudioFile.  Refusals raise SoundkitError: `media file is empty`; `AVI is not built`, `MPEG-PS is not built`, `MXF is not
    built`; whatever the container's decode_file or the stream's decoder says."""
    if len(data) == 0:
        raise SoundkitError(INVALID_INPUT, "decode_audio_file", "media file is empty")
    data = bytes(data)
    if looks_like_iso_bmff(data):
        from . import mp4
        config, frames = mp4.decode_file(data, options, scheduler, engine)
        return DecodedAudioFile("mp4", config, frames)
    if data[:4] == b"caff":
        from . import caf
        index, frames = caf.decode_file(data, options, scheduler, engine)
        return DecodedAudioFile("caf", index, frames)
    if looks_like_avi(data):
        raise SoundkitError(UNSUPPORTED, "decode_audio_file", "AVI is not built")
    if looks_like_mpeg_ps(data):
        raise SoundkitError(UNSUPPORTED, "decode_audio_file", "MPEG-PS is not built")
    if looks_like_mpeg_ts(data):
        from . import ts
        config, frames = ts.decode_file(data, options, scheduler, engine)
        return DecodedAudioFile("mpeg-ts", config, frames)
    if looks_like_mxf(data):
        raise SoundkitError(UNSUPPORTED, "decode_audio_file", "MXF is not built")
    if looks_like_ebml(data):
        from . import webm
        config, frames = webm.decode_file(data, options, scheduler, engine)
        return DecodedAudioFile("webm", config, frames)
    return DecodedAudioFile(None, None, decode_complete_stream(data, options, scheduler))


def decode_complete_stream(data, options=None, scheduler=None):
    """decode_complete_stream: the bytes through spawn() to the end of the stream -> [AudioData]"""
    from .audio_types import AudioData
    from .pipeline import DecodeError, DecodeOptions, default_scheduler
    h = (scheduler or default_scheduler()).spawn(options or DecodeOptions())
    frames = []

    def take():
        a = h.recv()
        if a is not None and not isinstance(a, AudioData):
            raise a
        if a is not None:
            frames.append(a)
        return a

    try:
        for at in list(range(0, len(data), 1 << 20)) + [None]:
            piece = b"" if at is None else data[at:at + (1 << 20)]
            while True:
                try:
                    if at is None:
                        h.finish()
                    else:
                        h.send(piece)
                    break
                except DecodeError as e:
                    if e.kind != "InputBufferFull":
                        raise
                    take()
        while take() is not None:
            pass
    finally:
        h.cancel()
    return frames

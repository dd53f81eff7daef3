"""AVI (`.avi`, OpenDML `AVIX` forms), audio only: the host demuxer (csrc/avi_stream.h) and decode_file (soundkit-decoder's
decode_avi_audio, lib.rs:257-570).  The container is walked on the host; the `##wb` chunks of the first `auds` stream go to what was there
before it: integer PCM at 16 / 24 / 32 bits and 32-bit float are little-endian PCM as they are, 8-bit PCM is widened on the device
(`SK_AIFF_U8`: `(u8 - 128) << 8`), MPEG audio (tag 0x0055) goes through `spawn()` to the end of the stream.

A stream handed to the scheduler needs none of this: `spawn()` takes an AVI by its `RIFF....AVI ` (csrc/pipeline.cpp) and demuxes on an
entropy thread.
Not built: WMA (`AVI WMA decoding is not implemented`, the reference's text), AC-3 (`AVI AC-3 audio is not built`: the reference hands it
to a decoder this project lacks), 8-bit PCM of more than 32 channels (`AVI 8-bit PCM with more than 32 channels is not built`, from
decode_file and from the scheduler alike: the AIFF stage that widens it takes 32), every other coded tag, `idx1` / `indx` seeking, video."""
import ctypes as C

import numpy as np

from ._lib import AviTrackInfo, SoundkitError, check, lib
from .engine import _ptr

ERR_STREAM = -1401
EVENT_NONE, EVENT_CONFIG, EVENT_PACKET = 0, 1, 2
FILE_PIECE = 64 * 1024  # what decode_file feeds the demuxer at a time
MAX_U8_CHANNELS = 32    # 8-bit PCM goes through the AIFF stage, which takes 1 ... 32 channels
RUN_FRAMES = 4096       # a PCM track leaves in runs of at most this many frames; the contract is the concatenated output


def _bytes(data):
    return np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)


def sniff(data):
    """looks_like_avi"""
    return bytes(data[:4]) == b"RIFF" and bytes(data[8:12]) == b"AVI "


class AviAudioConfig:
    """the config event: stream_index (the track's position among all `strl` lists), format_tag, channels, sample_rate,
    bits_per_sample (WAVEFORMAT's, clamped to 255)"""

    def __init__(self, info):
        self.stream_index, self.format_tag = int(info.stream_index), int(info.format_tag)
        self.channels, self.sample_rate, self.bits_per_sample = int(info.channels), int(info.sample_rate), int(info.bits)

    def __eq__(self, other):
        return isinstance(other, AviAudioConfig) and vars(self) == vars(other)

    def __repr__(self):
        return "AviAudioConfig(%s)" % ", ".join("%s=%r" % kv for kv in sorted(vars(self).items()))


class AviPacket:
    """a packet event: the bytes of one `##wb` chunk of the track"""

    def __init__(self, data):
        self.data = data

    def __repr__(self):
        return "AviPacket(%d bytes)" % len(self.data)


class _Demuxer:
    """add(bytes) / finish() -> the events that became complete.  A refusal raises SoundkitError with the demuxer's text (`text`; its
    `events`: what was complete in front of it), after which it stays refused."""
    _prefix, _info, _config, _packet = "sk_avi_demuxer", AviTrackInfo, AviAudioConfig, AviPacket

    def __init__(self, *create_args):
        self._h = C.c_void_p()
        check(getattr(lib, self._prefix + "_create")(*create_args, C.byref(self._h)), self._prefix + "_create")
        self.config = None
        self._out = np.zeros(FILE_PIECE, np.uint8)  # where a packet is taken to; grown to the largest packet met

    def close(self):
        if self._h:
            getattr(lib, self._prefix + "_destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _events(self, rc, what):
        events = []
        event, n, info = C.c_int(0), C.c_size_t(0), self._info()
        while True:
            out = self._out
            got = getattr(lib, self._prefix + "_next")(self._h, C.byref(event), C.byref(info), _ptr(out), out.size, C.byref(n))
            if got == -7 and n.value > out.size:  # SK_ERR_CAPACITY: the packet stays, *len says what it needs
                self._out = np.zeros(n.value, np.uint8)
                continue
            check(got, self._prefix + "_next")
            if event.value == EVENT_NONE:
                break
            if event.value == EVENT_CONFIG:
                self.config = self._config(info)
                events.append(self.config)
            else:
                events.append(self._packet(out[:n.value].tobytes()))
        if rc != 0:
            text = getattr(lib, self._prefix + "_last_error")(self._h).decode()
            error = SoundkitError(rc, what, text)
            error.events, error.text = events, text
            raise error
        return events

    def add(self, data):
        b = _bytes(data)
        return self._events(getattr(lib, self._prefix + "_add")(self._h, _ptr(b), len(data)), self._prefix + "_add")

    def finish(self):
        return self._events(getattr(lib, self._prefix + "_finish")(self._h), self._prefix + "_finish")


class AviAudioDemuxer(_Demuxer):
    """csrc/avi_stream.h: the AviAudioConfig once `hdrl` has been read, then one AviPacket per `##wb` chunk of the track"""


def _refuse(text):
    return SoundkitError(ERR_STREAM, "decode_file", text)


def demux_file(demuxer, data, piece=FILE_PIECE, status=ERR_STREAM):
    """the whole file through `demuxer` in pieces -> (config or None, [packet bytes]); a refusal is `Invalid input format: <its text>`"""
    events = []
    try:
        try:
            for at in range(0, len(data), piece):
                events.extend(demuxer.add(data[at:at + piece]))
            events.extend(demuxer.finish())
        except SoundkitError as e:
            if hasattr(e, "text"):
                raise SoundkitError(status, "decode_file", "Invalid input format: %s" % e.text)
            raise
    finally:
        demuxer.close()
    return demuxer.config, [e.data for e in events if hasattr(e, "data")]


def pcm_runs(pcm, bytes_per_frame):
    """PCM bytes as runs of at most RUN_FRAMES frames"""
    step = RUN_FRAMES * bytes_per_frame
    return [pcm[at:at + step] for at in range(0, len(pcm), step)]


def decode_file(data, options=None, scheduler=None, engine=None):
    """decode_avi_audio: the file through the demuxer -> the format tag is taken or refused -> PCM through the output options
    (alac.output_stage) and the resampler's flush, MPEG audio through spawn() to the end of the stream.  -> (the config, [AudioData])."""
    from . import alac
    from .engine import AIFF_U8, default_engine
    from .media_file import decode_complete_stream
    config, packets = demux_file(AviAudioDemuxer(), bytes(data))
    encoded = b"".join(packets)
    if not encoded:
        raise _refuse("Invalid input format: AVI audio track contains no packets")
    tag, bits, channels = config.format_tag, config.bits_per_sample, config.channels
    if tag == 0x0055:
        frames = decode_complete_stream(encoded, options, scheduler)
    elif tag in (0x0001, 0x0003):
        if tag == 0x0003 and bits != 32:
            raise _refuse("Invalid input format: unsupported AVI float PCM depth %d" % bits)
        if tag == 0x0001 and bits not in (8, 16, 24, 32):
            raise _refuse("Invalid input format: unsupported AVI integer PCM depth %d" % bits)
        if bits == 8 and channels > MAX_U8_CHANNELS:  # the AIFF stage's bound; the scheduler says the same
            raise _refuse("Invalid input format: AVI 8-bit PCM with more than %d channels is not built" % MAX_U8_CHANNELS)
        bytes_per_frame = channels * (bits // 8)
        if len(encoded) % bytes_per_frame:
            raise _refuse("Invalid input format: AVI PCM ends with a partial sample frame")
        if bits == 8:  # (u8 - 128) << 8 on the device
            encoded, bits, bytes_per_frame = (engine or default_engine()).aiff_decode(AIFF_U8, channels, encoded), 16, 2 * channels
        frames = alac.output_stage(pcm_runs(encoded, bytes_per_frame), config.sample_rate, channels, bits, options, scheduler, is_float=tag == 0x0003)
    elif 0x0160 <= tag <= 0x0163:
        raise _refuse("Invalid input format: AVI WMA decoding is not implemented")
    elif tag == 0x2000:
        raise _refuse("Invalid input format: AVI AC-3 audio is not built")
    else:
        raise _refuse("Invalid input format: unsupported AVI audio format tag 0x%04x" % tag)
    if not frames:
        raise _refuse("Decoding failed: AVI audio track emitted no frames")
    return config, frames

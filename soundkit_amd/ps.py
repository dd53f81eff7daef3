"""MPEG program stream (`.vob`, `.mpg`), audio only: the host demuxer (csrc/ps_stream.h) and decode_file (soundkit-decoder's
decode_mpeg_ps_audio, lib.rs:572-804).  The container is walked on the host.  DVD LPCM at 16 bits is big-endian PCM as it is (as Blu-ray
LPCM out of a transport stream is; the reference swaps it on the host), at 24 bits its groups are unpacked on the device
(`SK_AIFF_DVD_S24`); MPEG audio PES goes through `spawn()` to the end of the stream.

Beyond the reference (csrc/ps_stream.h says why): packets are walked by their length field, only the first LPCM substream is the track,
and MPEG audio PES (C0 ... DF) is a track.  decode_file looks through the whole file: DVD LPCM wins where any is present, else the
stream id of the first MPEG audio packet is the track.  A stream handed to the scheduler cannot look ahead: `spawn()` takes a program
stream by its `00 00 01 BA` (csrc/pipeline.cpp), and the first audio packet of either kind decides.
Not built: 20-bit DVD LPCM (`20-bit DVD LPCM decoding is not implemented`, the reference's text), AC-3 / DTS substreams, video."""
from ._lib import PsTrackInfo, SoundkitError
from .avi import _Demuxer, demux_file, pcm_runs

ERR_STREAM = -1501
TRACK_FIRST, TRACK_LPCM, TRACK_MPEG_AUDIO = 0, 1, 2
KINDS = {1: "pcm-dvd", 2: "mpeg-audio"}
NO_TRACK = "MPEG-PS has no supported DVD LPCM track"


def sniff(data):
    """looks_like_mpeg_ps"""
    return bytes(data[:4]) == b"\x00\x00\x01\xba"


class PsAudioConfig:
    """the config event: kind (`pcm-dvd`, `mpeg-audio`), stream_id (0xBD, or 0xC0 ... 0xDF); for DVD LPCM substream_id (0xA0 ... 0xAF),
    sample_rate, channels, bits_per_sample and block_bytes (every packet is a whole number of these), else None"""

    def __init__(self, info):
        self.kind, self.stream_id = KINDS[int(info.kind)], int(info.stream_id)
        lpcm = int(info.kind) == 1
        self.substream_id = int(info.substream_id) if lpcm else None
        self.sample_rate = int(info.sample_rate) if lpcm else None
        self.channels = int(info.channels) if lpcm else None
        self.bits_per_sample = int(info.bits) if lpcm else None
        self.block_bytes = int(info.block_bytes) if lpcm else None

    def __eq__(self, other):
        return isinstance(other, PsAudioConfig) and vars(self) == vars(other)

    def __repr__(self):
        return "PsAudioConfig(%s)" % ", ".join("%s=%r" % kv for kv in sorted(vars(self).items()))


class PsPacket:
    """a packet event: DVD LPCM -- the whole blocks that one PES packet completed; MPEG audio -- one PES payload"""

    def __init__(self, data):
        self.data = data

    def __repr__(self):
        return "PsPacket(%d bytes)" % len(self.data)


class PsAudioDemuxer(_Demuxer):
    """csrc/ps_stream.h: the PsAudioConfig in front of the track's first PsPacket, then PsPackets in stream order.  track_mode:
    TRACK_FIRST -- the first audio packet of either kind names the track; TRACK_LPCM / TRACK_MPEG_AUDIO -- that kind alone"""
    _prefix, _info, _config, _packet = "sk_ps_demuxer", PsTrackInfo, PsAudioConfig, PsPacket

    def __init__(self, track_mode=TRACK_FIRST):
        super().__init__(int(track_mode))


def _refuse(text):
    return SoundkitError(ERR_STREAM, "decode_file", text)


def decode_file(data, options=None, scheduler=None, engine=None):
    """decode_mpeg_ps_audio: the file through the demuxer, DVD LPCM first and MPEG audio where there is none -> DVD LPCM through the
    output options (alac.output_stage) and the resampler's flush, MPEG audio through spawn() to the end of the stream.
    -> (the config, [AudioData])."""
    from . import alac
    from .engine import AIFF_DVD_S24, default_engine
    from .media_file import decode_complete_stream
    data = bytes(data)
    try:
        config, packets = demux_file(PsAudioDemuxer(TRACK_LPCM), data, status=ERR_STREAM)
    except SoundkitError as e:
        if not str(e).endswith(NO_TRACK):
            raise
        config, packets = demux_file(PsAudioDemuxer(TRACK_MPEG_AUDIO), data, status=ERR_STREAM)
    if config.kind == "mpeg-audio":
        frames = decode_complete_stream(b"".join(packets), options, scheduler)
        if not frames:  # (this project's own track kind, so its own text: in the shape of the reference's for DVD LPCM)
            raise _refuse("Decoding failed: MPEG-PS MPEG audio track emitted no frames")
        return config, frames
    pcm, channels, bits = b"".join(packets), config.channels, config.bits_per_sample
    if bits == 24 and pcm:
        pcm = (engine or default_engine()).aiff_decode(AIFF_DVD_S24, channels, pcm)
    frames = alac.output_stage(pcm_runs(pcm, channels * (bits // 8)), config.sample_rate, channels, bits, options, scheduler, big_endian=bits == 16)
    if not frames:
        raise _refuse("Decoding failed: MPEG-PS DVD LPCM track emitted no frames")
    return config, frames

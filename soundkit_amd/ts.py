"""MPEG transport stream (`.ts`, HLS segments, Blu-ray `.m2ts`), audio only: the host demuxer (csrc/ts_stream.h: soundkit-audio-demux's
MpegTsAudioDemuxer) and decode_file (soundkit-decoder's decode_mpeg_ts_audio, lib.rs:898-1005).  The container is walked on the host; the
packets go to the decoders that were there before it: ADTS frames to the ADTS decoder, MPEG audio frames to Mp3Decoder -- all three
layers, where the reference's decode side takes `mpeg-audio` / `mp2` and refuses Layer III and Layer I -- and Blu-ray LPCM payloads are
big-endian PCM as they are.  LATM AAC, AC-3 and DTS: `unsupported MPEG-TS audio codec NAME`.

A stream handed to the scheduler needs none of this: `spawn()` takes a transport stream by `sniff` (csrc/pipeline.cpp), `spawn_mpeg_ts()`
takes one that is joined in mid-segment, and either demuxes on an entropy thread.
Blu-ray LPCM: stereo at 16 or 24 bits.  Mono (with its pad channel), 20 bits, the multichannel assignments and a size field that
disagrees with its payload are refused by the demuxer with texts of this project's own.
Not built: LATM / LOAS decode, AC-3, DTS (reported, every PES payload handed out whole), video, PCR, seeking, data PIDs, program
selection other than the lowest program number."""
import ctypes as C

import numpy as np

from ._lib import SoundkitError, TsPacketInfo, TsTrackInfo, check, lib
from .engine import _ptr

ERR_STREAM = -1101
CODECS = {0: "unknown", 1: "aac", 2: "pcm", 3: "ac3", 4: "dts", 5: "mp3", 6: "mp1", 7: "mp2", 8: "mpeg-audio"}  # AudioCodec::as_str
PACKET_FORMATS = {0: "raw", 1: "adts", 2: "latm"}
FILE_PIECE = 64 * 1024  # what decode_file feeds the demuxer at a time


def _bytes(data):
    return np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)


def sniff(data):
    """looks_like_mpeg_ts: three syncs at stride 188, or at stride 192 behind four bytes"""
    b = _bytes(data)
    return bool(lib.sk_ts_sniff(_ptr(b), len(data)))


class TsAudioConfig:
    """the config event (AudioTrackConfig): codec (`aac`, `pcm`, `ac3`, `dts`, `mp3`, `mp1`, `mp2`), packet_format (`raw`, `adts`,
    `latm`), stream_type, pid, program_number, packet_stride and packet_prefix, sample_rate and channels (None where the first packet
    does not say); for Blu-ray LPCM bits_per_sample, bytes_per_frame, frames_per_packet and the four header bytes, else None"""

    def __init__(self, info):
        self.codec, self.packet_format = CODECS[info.codec], PACKET_FORMATS[info.packet_format]
        self.stream_type, self.pid, self.program_number = int(info.stream_type), int(info.pid), int(info.program_number)
        self.packet_stride, self.packet_prefix = int(info.packet_stride), int(info.packet_prefix)
        self.sample_rate = int(info.sample_rate) if info.has_rate else None
        self.channels = int(info.channels) if info.has_channels else None
        lpcm = info.bits_per_sample != 0
        self.bits_per_sample = int(info.bits_per_sample) if lpcm else None
        self.bytes_per_frame = int(info.bytes_per_frame) if lpcm else None
        self.frames_per_packet = int(info.frames_per_packet) if lpcm else None
        self.lpcm_header = bytes(info.lpcm_header) if lpcm else None

    def __repr__(self):
        return "TsAudioConfig(%s)" % ", ".join("%s=%r" % kv for kv in sorted(vars(self).items()))


class TsPacket:
    """a packet event: one frame's (Blu-ray LPCM, AC-3, DTS: one PES payload's) bytes; pts, dts and duration in 90 kHz units or None;
    the continuity counter of the packet that started its PES; discontinuity on the first frame of a PES that met the flag or a gap"""

    def __init__(self, data, info):
        self.data = data
        self.pts = int(info.pts) if info.has_pts else None
        self.dts = int(info.dts) if info.has_dts else None
        self.duration = int(info.duration) if info.has_duration else None
        self.continuity_counter, self.discontinuity = int(info.continuity_counter), bool(info.discontinuity)

    def __repr__(self):
        return "TsPacket(%d bytes, pts=%r, dts=%r, duration=%r, cc=%d, discontinuity=%r)" % (len(self.data), self.pts, self.dts, self.duration,
                                                                                         self.continuity_counter, self.discontinuity)


class TsAudioDemuxer:
    """add(bytes) / finish() -> the events that became complete: the TsAudioConfig in front of the track's first TsPacket, then TsPackets
    in stream order.  A refusal raises SoundkitError with the demuxer's text (its `events`: what was complete in front of it), after
    which it stays refused."""

    def __init__(self):
        self._h = C.c_void_p()
        check(lib.sk_ts_demuxer_create(C.byref(self._h)), "sk_ts_demuxer_create")
        self.config = None

    def close(self):
        if self._h:
            lib.sk_ts_demuxer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def buffered_bytes(self):
        n = C.c_size_t(0)
        check(lib.sk_ts_demuxer_pending(self._h, None, None, C.byref(n)), "sk_ts_demuxer_pending")
        return n.value

    def _events(self, rc, what):
        events = []
        if self.config is None:
            info = TsTrackInfo()
            if lib.sk_ts_demuxer_config(self._h, C.byref(info)) == 0:
                self.config = TsAudioConfig(info)
                events.append(self.config)
        n, size = C.c_uint32(0), C.c_size_t(0)
        while True:
            check(lib.sk_ts_demuxer_pending(self._h, C.byref(n), C.byref(size), None), "sk_ts_demuxer_pending")
            if n.value == 0:
                break
            out, got, info = np.zeros(max(size.value, 1), np.uint8), C.c_size_t(0), TsPacketInfo()
            check(lib.sk_ts_demuxer_take(self._h, _ptr(out), out.size, C.byref(got), C.byref(info)), "sk_ts_demuxer_take")
            events.append(TsPacket(out[:got.value].tobytes(), info))
        if rc != 0:
            error = SoundkitError(rc, what, lib.sk_ts_demuxer_last_error(self._h).decode())
            error.events = events
            error.text = lib.sk_ts_demuxer_last_error(self._h).decode()
            raise error
        return events

    def add(self, data):
        b = _bytes(data)
        return self._events(lib.sk_ts_demuxer_add(self._h, _ptr(b), len(data)), "sk_ts_demuxer_add")

    def finish(self):
        return self._events(lib.sk_ts_demuxer_finish(self._h), "sk_ts_demuxer_finish")


def _refuse(text):
    return SoundkitError(ERR_STREAM, "decode_file", text)


class _Adts:
    def __init__(self, engine):
        from .aac import AacDecoder
        self.decoder = AacDecoder(engine)

    def decode(self, packets):
        from .aac import decode_i16_with_drain
        out = np.zeros(max((len(packets) + 2) * 2048, 4096), np.int16)
        try:
            got = decode_i16_with_drain(self.decoder, b"".join(p.data for p in packets), out)
        except ValueError as e:
            raise _refuse("Decoding failed: %s" % e)
        self.rate, self.channels = self.decoder.sample_rate(), self.decoder.channels()
        return np.concatenate(got) if got else np.zeros(0, np.int16)


class _MpegAudio:
    def __init__(self, engine):
        from .mp3 import Mp3Decoder
        self.decoder = Mp3Decoder(engine=engine)

    def decode(self, packets):
        out, got = np.zeros(max(len(packets) * 1152 * 2, 4608), np.int16), []
        n = self.decoder.decode_i16(b"".join(p.data for p in packets), out)
        while n:  # frames that found no room
            got.append(out[:n].copy())
            n = self.decoder.decode_i16(b"", out)
        self.rate, self.channels = self.decoder.sample_rate(), self.decoder.channels()
        return np.concatenate(got) if got else np.zeros(0, np.int16)


def _per_packet(samples, packets, rate, channels):
    """the samples of one call as one piece per packet, where every packet gave what its duration says; else one piece"""
    counts = [(p.duration or 0) * rate // 90000 * channels for p in packets]
    if len(packets) > 1 and all(counts) and sum(counts) == samples.size:
        ends = np.cumsum(counts)
        return [samples[e - c:e] for c, e in zip(counts, ends)]
    return [samples] if samples.size else []


def _big_endian_stage(pieces, config, options, scheduler):
    """Blu-ray LPCM payloads -> [AudioData]: as they are without options that change anything, else what the scheduler's raw PCM stream of
    big-endian samples makes of them, the resampler flushed at the end (alac.output_stage for big-endian input)"""
    from .audio_types import AudioData, Endianness, EncodingFlag
    from .engine import FMT_S16BE, FMT_S24BE
    from .pipeline import DecodeError, DecodeOptions, RawPcmFormat, default_scheduler
    o = options or DecodeOptions()
    rate, channels, bits = config.sample_rate, config.channels, config.bits_per_sample
    if (o.output_sample_rate or rate) == rate and (o.output_channels or channels) == channels and (o.output_bits_per_sample or bits) == bits:
        return [AudioData(bits, channels, rate, p, EncodingFlag.PCMSigned, Endianness.BigEndian) for p in pieces]
    h = (scheduler or default_scheduler()).spawn_raw_pcm(RawPcmFormat(rate, channels, FMT_S16BE if bits == 16 else FMT_S24BE), o)
    out = []

    def take():
        a = h.recv()
        if a is not None and not isinstance(a, AudioData):
            raise a
        if a is not None:
            out.append(a)
        return a

    try:
        for p in pieces + [b""]:  # the empty send ends the stream and flushes the resampler
            while True:
                try:
                    h.send(p)
                    break
                except DecodeError as e:
                    if e.kind != "InputBufferFull":
                        raise
                    take()
        while take() is not None:
            pass
    finally:
        h.cancel()
    return out


def decode_file(data, options=None, scheduler=None, engine=None):
    """decode_mpeg_ts_audio: the file in pieces of 64 KiB through the demuxer -> the first configuration is taken or refused -> every
    packet through its decoder -> the output options (alac.output_stage; big-endian for Blu-ray LPCM) -> the resampler's flush.
    -> (the config, [AudioData]).  A demuxer refusal is `Invalid input format: <its text>`."""
    from . import alac
    demuxer, track, config, pieces = TsAudioDemuxer(), None, None, []

    def consume(events):
        nonlocal track, config
        packets = []
        for e in events:
            if isinstance(e, TsPacket):
                packets.append(e)
            elif config is None:
                if e.codec == "aac" and e.packet_format == "adts":
                    track = _Adts(engine)
                elif e.codec in ("mp1", "mp2", "mp3"):
                    track = _MpegAudio(engine)
                elif e.codec != "pcm":
                    raise _refuse("Invalid input format: unsupported MPEG-TS audio codec %s" % e.codec)
                config = e
        if config is None or not packets:
            return
        if track is None:
            pieces.extend(p.data for p in packets)
        else:
            samples = track.decode(packets)
            if samples.size:
                pieces.extend(s.astype("<i2").tobytes() for s in _per_packet(samples, packets, track.rate, track.channels))

    try:
        try:
            for at in range(0, len(data), FILE_PIECE):
                consume(demuxer.add(data[at:at + FILE_PIECE]))
            consume(demuxer.finish())
        except SoundkitError as e:
            if hasattr(e, "text"):
                raise _refuse("Invalid input format: %s" % e.text)
            raise
        if config is None:
            raise _refuse("Invalid input format: MPEG-TS has no supported audio track")
        if not pieces:
            raise _refuse("Decoding failed: MPEG-TS %s track emitted no audio frames" % config.codec)
        if track is None:
            return config, _big_endian_stage(pieces, config, options, scheduler)
        return config, alac.output_stage(pieces, track.rate, track.channels, 16, options, scheduler)
    finally:
        demuxer.close()
        if track is not None:
            track.decoder.close()

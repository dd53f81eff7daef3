"""WebM / Matroska, audio only: the host demuxer (csrc/webm_stream.h: soundkit-webm's WebmAudioDemuxer), WebmDecoder (soundkit-webm's
WebmDecoder, lib.rs:2849-3078) and decode_file.  The container is walked on the host; the frames go to the decoders that were there
before it: A_VORBIS to vorbis.VorbisPacketDecoder, as in the reference; beyond the reference, whose decoder refuses them, A_AAC to the
ADTS decoder (the CodecPrivate is an AudioSpecificConfig: it meets the AAC-LC config check and every frame is wrapped in a 7-byte ADTS
header, as an MP4 sample is) and A_FLAC to FlacDecoder (the CodecPrivate is `fLaC` and the metadata blocks; followed by the frames it
is a native FLAC stream).  A_OPUS, A_ALAC and everything else: `unsupported or disabled WebM codec: ID`.

A stream handed to the scheduler needs none of this: `spawn()` sniffs the EBML magic (csrc/pipeline.cpp) and demuxes on an entropy
thread.  DiscardPadding trims Vorbis packets at either end, as the reference's decode_vorbis does; on the AAC and FLAC paths, where a
block and the decoder's output are not tied one to one, it is reported by the demuxer and not applied.
Not built: Opus, ALAC through the decoder, video, Cues / seeking, chained segments, EBML CRC-32 verification, ContentCompression other
than header stripping, the old A_AAC/MPEG4/... ids."""
import ctypes as C

import numpy as np

from ._lib import SoundkitError, WebmPacketInfo, WebmTrackInfo, check, lib
from .engine import _ptr

ERR_STREAM = -1001
CODEC_IDS = {1: "A_VORBIS", 2: "A_AAC", 3: "A_FLAC", 4: "A_ALAC", 5: "A_OPUS"}
FILE_PIECE = 64 * 1024  # what decode_file feeds its decoder at a time
AAC_RATES = (96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 7350)


def _bytes(data):
    return np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)


class WebmAudioConfig:
    """the config event (WebmAudioConfig): track_number, codec_id, sample_rate (48 000 without one), channels (2 without one),
    codec_private, codec_delay_ns, seek_pre_roll_ns, default_duration_ns (None without one), track_timestamp_scale, timecode_scale_ns,
    header_stripping_prefix; for an OpusHead CodecPrivate pre_skip, output_gain and mapping_family, else None"""

    def __init__(self, info, private, prefix):
        self.track_number, self.codec_id = int(info.track_number), CODEC_IDS[info.codec]
        self.sample_rate, self.channels = int(info.sample_rate), int(info.channels)
        self.codec_private, self.header_stripping_prefix = private, prefix
        self.codec_delay_ns, self.seek_pre_roll_ns = int(info.codec_delay_ns), int(info.seek_pre_roll_ns)
        self.default_duration_ns = int(info.default_duration_ns) or None
        self.track_timestamp_scale, self.timecode_scale_ns = float(info.track_timestamp_scale), int(info.timecode_scale_ns)
        self.pre_skip = self.output_gain = self.mapping_family = None
        if len(private) >= 19 and private[:8] == b"OpusHead":  # parse_opus_head_metadata
            self.pre_skip = int.from_bytes(private[10:12], "little")
            self.output_gain = int.from_bytes(private[16:18], "little", signed=True)
            self.mapping_family = private[18]

    def __repr__(self):
        return "WebmAudioConfig(%s)" % ", ".join("%s=%r" % kv for kv in sorted(vars(self).items()))


class WebmPacket:
    """a packet event: one frame's bytes (the header-stripping prefix put back), its track and codec id, timestamp_ns, and duration_ns
    and discard_padding_ns or None"""

    def __init__(self, data, info):
        self.data, self.track_number, self.codec_id = data, int(info.track_number), CODEC_IDS[info.codec]
        self.timestamp_ns = int(info.timestamp_ns)
        self.duration_ns = int(info.duration_ns) if info.has_duration else None
        self.discard_padding_ns = int(info.discard_padding_ns) if info.has_discard_padding else None

    def __repr__(self):
        return "WebmPacket(track=%d, %d bytes, t=%d, duration=%r, discard=%r)" % (self.track_number, len(self.data), self.timestamp_ns, self.duration_ns,
                                                                                 self.discard_padding_ns)


def vorbis_headers(codec_private):
    """parse_vorbis_codec_private: an A_VORBIS CodecPrivate -> its three header packets"""
    b, offsets, sizes, text = _bytes(codec_private), (C.c_size_t * 3)(), (C.c_size_t * 3)(), C.create_string_buffer(256)
    rc = lib.sk_webm_vorbis_headers(_ptr(b), len(codec_private), C.byref(offsets), C.byref(sizes), text, len(text))
    if rc != 0:
        raise SoundkitError(rc, "sk_webm_vorbis_headers", text.value.decode())
    return [bytes(codec_private[offsets[k]:offsets[k] + sizes[k]]) for k in range(3)]


def discard_frames(padding_ns, sample_rate, decoded_frames):
    """discard_padding_frames -> (frames off the front, frames off the back); None: (0, 0)"""
    if padding_ns is None:
        return 0, 0
    front, back, text = C.c_uint32(0), C.c_uint32(0), C.create_string_buffer(256)
    rc = lib.sk_webm_discard_frames(padding_ns, sample_rate, decoded_frames, C.byref(front), C.byref(back), text, len(text))
    if rc != 0:
        raise SoundkitError(rc, "sk_webm_discard_frames", text.value.decode())
    return front.value, back.value


class WebmAudioDemuxer:
    """add(bytes) / finish() -> the events that became complete: the WebmAudioConfigs (once the first Cluster header has arrived), then
    WebmPackets in file order.  A refusal raises SoundkitError with the demuxer's text (its `events`: what was complete in front of
    it), after which it stays refused."""

    def __init__(self):
        self._h = C.c_void_p()
        check(lib.sk_webm_demuxer_create(C.byref(self._h)), "sk_webm_demuxer_create")
        self.configs = None

    def close(self):
        if self._h:
            lib.sk_webm_demuxer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def buffered_bytes(self):
        n = C.c_size_t(0)
        check(lib.sk_webm_demuxer_pending(self._h, None, None, C.byref(n)), "sk_webm_demuxer_pending")
        return n.value

    def _config(self, index):
        info = WebmTrackInfo()
        rc = lib.sk_webm_demuxer_config(self._h, index, C.byref(info), None, 0, None, 0)
        if rc not in (0, -7):
            check(rc, "sk_webm_demuxer_config")
        private, prefix = np.zeros(max(int(info.private_len), 1), np.uint8), np.zeros(max(int(info.prefix_len), 1), np.uint8)
        check(lib.sk_webm_demuxer_config(self._h, index, C.byref(info), _ptr(private), private.size, _ptr(prefix), prefix.size), "sk_webm_demuxer_config")
        return WebmAudioConfig(info, private[:info.private_len].tobytes(), prefix[:info.prefix_len].tobytes())

    def _events(self, rc, what):
        events = []
        n_tracks = lib.sk_webm_demuxer_n_tracks(self._h)
        if self.configs is None and n_tracks:
            self.configs = [self._config(i) for i in range(n_tracks)]
            events += self.configs
        n, size = C.c_uint32(0), C.c_size_t(0)
        while True:
            check(lib.sk_webm_demuxer_pending(self._h, C.byref(n), C.byref(size), None), "sk_webm_demuxer_pending")
            if n.value == 0:
                break
            out, got, info = np.zeros(max(size.value, 1), np.uint8), C.c_size_t(0), WebmPacketInfo()
            check(lib.sk_webm_demuxer_take(self._h, _ptr(out), out.size, C.byref(got), C.byref(info)), "sk_webm_demuxer_take")
            events.append(WebmPacket(out[:got.value].tobytes(), info))
        if rc != 0:
            error = SoundkitError(rc, what, lib.sk_webm_demuxer_last_error(self._h).decode())
            error.events = events
            raise error
        return events

    def add(self, data):
        b = _bytes(data)
        return self._events(lib.sk_webm_demuxer_add(self._h, _ptr(b), len(data)), "sk_webm_demuxer_add")

    def finish(self):
        return self._events(lib.sk_webm_demuxer_finish(self._h), "sk_webm_demuxer_finish")


def _refuse(text):
    return SoundkitError(ERR_STREAM, "WebmDecoder", text)


class _VorbisTrack:
    def __init__(self, config, engine):
        from .vorbis import VorbisPacketDecoder
        self.headers, self.decoder, self.make = vorbis_headers(config.codec_private), None, lambda: VorbisPacketDecoder(engine)
        self.rate, self.channels = config.sample_rate, config.channels

    def decode(self, packets, final):
        if self.decoder is None:  # (the device is first needed here, so that a second configuration is refused without one)
            self.decoder = self.make()
            for h in self.headers:
                self.decoder.decode_packet(h)
            self.rate, self.channels = self.decoder.sample_rate() or self.rate, self.decoder.channels() or self.channels
        pcm = []
        for p in packets:  # decode_vorbis: [front, max(frames - back, front)) of every packet's frames
            samples = self.decoder.decode_packet(p.data)
            if samples is None:
                continue
            frames = len(samples) // self.channels
            front, back = discard_frames(p.discard_padding_ns, self.rate, frames)
            pcm.append(samples[front * self.channels:max(frames - back, front) * self.channels].astype("<i2").tobytes())
        return b"".join(pcm)


class _AacTrack:
    def __init__(self, config, engine):
        from .aac import AacDecoder
        from .aac_lc import AacLcError, AacLcFrontEnd
        asc = config.codec_private
        index = ((asc[0] & 7) << 1 | asc[1] >> 7) if len(asc) >= 2 else 15
        if index >= len(AAC_RATES):
            raise _refuse("WebM A_AAC CodecPrivate holds no AudioSpecificConfig with a rate of the table")
        try:
            AacLcFrontEnd(asc).close()
        except AacLcError as e:
            raise SoundkitError(e.status, "WebmDecoder", "AAC-LC decoder init: %s" % e)
        self.asc, self.rate, self.channels = asc, AAC_RATES[index], (asc[1] >> 3) & 15
        self.decoder, self.make = None, lambda: AacDecoder(engine)

    def decode(self, packets, final):
        from .mp4 import adts_header
        stream = b"".join(adts_header(self.asc, self.rate, self.channels, len(p.data)) + p.data for p in packets)
        if not stream and not final:
            return b""
        self.decoder = self.decoder or self.make()
        out, got = np.zeros(max((len(packets) + 2) * 1024 * max(self.channels, 1), 4096), np.int16), 0
        try:
            n = self.decoder.decode_i16(stream, out)
            while n:  # decode_i16_with_drain: empty calls until nothing comes
                got += n
                n = self.decoder.decode_i16(b"", out[got:])
        except ValueError as e:
            raise _refuse(str(e))
        self.rate, self.channels = self.decoder.sample_rate() or self.rate, self.decoder.channels() or self.channels
        return out[:got].astype("<i2").tobytes()


class _FlacTrack:
    def __init__(self, config, engine):
        from .flac import FlacDecoder
        if len(config.codec_private) < 42 or config.codec_private[:4] != b"fLaC":
            raise _refuse("WebM A_FLAC CodecPrivate holds no fLaC marker and STREAMINFO block")
        self.decoder, self.make, self.head = None, lambda: FlacDecoder(engine), config.codec_private
        self.rate, self.channels = config.sample_rate, config.channels
        self.out = np.zeros(1 << 18, np.int16)

    def decode(self, packets, final):
        self.decoder = self.decoder or self.make()
        data, self.head = self.head + b"".join(p.data for p in packets), b""
        pcm = []
        if data:
            n = self.decoder.decode_i16(data, self.out)
            pcm.append(self.out[:n].astype("<i2").tobytes())
            while self.decoder.pending_samples():  # frames that found no room
                n = self.decoder.decode_i16(b"", self.out)
                pcm.append(self.out[:n].astype("<i2").tobytes())
        if final:  # a call with no bytes finalises the stream and drains what is left
            while True:
                n = self.decoder.decode_i16(b"", self.out)
                if n == 0:
                    break
                pcm.append(self.out[:n].astype("<i2").tobytes())
        self.rate, self.channels = self.decoder.sample_rate() or self.rate, self.decoder.channels() or self.channels
        return b"".join(pcm)


class WebmDecoder:
    """soundkit-webm's WebmDecoder: add(piece) / finish() -> one AudioData (16 bits, everything the call completed, concatenated) or
    None.  One audio track: a second configuration is `WebM decoder received more than one audio configuration`."""

    def __init__(self, engine=None):
        self._engine, self._demuxer = engine, WebmAudioDemuxer()
        self.config, self._track = None, None

    def close(self):
        self._demuxer.close()
        if self._track is not None and self._track.decoder is not None and hasattr(self._track.decoder, "close"):
            self._track.decoder.close()
        self._track = None

    def sample_rate(self):
        return self._track.rate if self._track else None

    def channels(self):
        return self._track.channels if self._track else None

    def _accept(self, events, final):
        from .audio_types import AudioData, Endianness, EncodingFlag
        packets = []
        for e in events:
            if isinstance(e, WebmPacket):
                packets.append(e)
            elif self.config is not None:
                raise _refuse("WebM decoder received more than one audio configuration")
            else:
                kind = {"A_VORBIS": _VorbisTrack, "A_AAC": _AacTrack, "A_FLAC": _FlacTrack}.get(e.codec_id)
                if kind is None:
                    raise _refuse("unsupported or disabled WebM codec: %s" % e.codec_id)
                self._track = kind(e, self._engine)
                self.config = e
        if self._track is None:
            return None
        pcm = self._track.decode([p for p in packets if p.track_number == self.config.track_number], final)
        if not pcm:
            return None
        return AudioData(16, self._track.channels, self._track.rate, pcm, EncodingFlag.PCMSigned, Endianness.LittleEndian)

    def add(self, data):
        return self._accept(self._demuxer.add(data), False)

    def finish(self):
        return self._accept(self._demuxer.finish(), True)


def decode_file(data, options=None, scheduler=None, engine=None):
    """a whole file through WebmDecoder, in pieces of 64 KiB -> the output options through alac.output_stage -> the resampler's flush,
    as mp4.decode_file ends.  -> (the config, [AudioData])"""
    from . import alac
    decoder, pieces = WebmDecoder(engine), []
    try:
        for at in range(0, len(data), FILE_PIECE):
            got = decoder.add(data[at:at + FILE_PIECE])
            if got is not None:
                pieces.append(got)
        got = decoder.finish()
        if got is not None:
            pieces.append(got)
        if not pieces:
            raise SoundkitError(ERR_STREAM, "decode_file", "Decoding failed: WebM %s track emitted no audio frames" % decoder.config.codec_id)
        rate, channels = pieces[0].sampling_rate, pieces[0].channel_count
        return decoder.config, alac.output_stage([p.data.tobytes() for p in pieces], rate, channels, 16, options, scheduler)
    finally:
        decoder.close()

"""MP4 / M4A / fragmented MP4, audio only: the host demuxer, sample index and edit-list trim (csrc/mp4_stream.h) and decode_file:
soundkit-decoder's decode_seekable_mp4_audio (lib.rs:1429-1537, with its fragmented fall-through 1539 ff.) for `aac` and `alac` tracks.
The container is walked on the host; the packets go to the decoders that were there before it -- the ADTS decoder for AAC-LC
(every sample wrapped in a 7-byte ADTS header, as the reference's AacMp4Demuxer does) and the ALAC packet stage for ALAC.

A stream handed to the scheduler needs none of this: `spawn()` sniffs `ftyp` (csrc/pipeline.cpp) and demuxes on an entropy thread.
Not built: `flac` and `pcm` tracks, version-two sound descriptions, edits behind the first media edit, video."""
import ctypes as C

import numpy as np

from ._lib import Mp4TrackInfo, SoundkitError, check, lib
from .engine import _ptr

ERR_STREAM = -901
CODECS = {1: "aac", 2: "alac"}
FRAGMENT_PIECE = 64 * 1024  # what decode_fragmented_mp4_audio feeds its demuxer at a time


def _bytes(data):
    return np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)


class Mp4Config:
    """the config event: codec ("aac" / "alac"), sample_rate, channels, bits_per_sample, track_id, timescale, sample_count, fragmented,
    codec_private (the AudioSpecificConfig, or the ALAC cookie in its MP4 wrapping) and edit = (presentation start, media start, duration)
    in the track's timescale, or None"""

    def __init__(self, info, private):
        self.codec = CODECS[info.codec]
        for n in ("sample_rate", "channels", "bits_per_sample", "track_id", "timescale", "sample_count"):
            setattr(self, n, int(getattr(info, n)))
        self.fragmented = bool(info.fragmented)
        self.codec_private = private
        self.edit = (int(info.edit_presentation_start), int(info.edit_media_start), int(info.edit_duration)) if info.has_edit else None

    def __repr__(self):
        return "Mp4Config(%s)" % ", ".join("%s=%r" % kv for kv in sorted(vars(self).items()))


class Mp4Packet:
    """a packet event: the sample's raw bytes, its decode time and its duration in the track's timescale"""

    def __init__(self, data, start_time, duration):
        self.data, self.start_time, self.duration = data, start_time, duration


def _config(fn, handle, what):
    info = Mp4TrackInfo()
    rc = fn(handle, C.byref(info), None, 0)
    if rc not in (0, -7):
        check(rc, what)
    if info.codec == 0:
        return None
    private = np.zeros(max(int(info.private_len), 1), np.uint8)
    check(fn(handle, C.byref(info), _ptr(private), private.size), what)
    return Mp4Config(info, private[:info.private_len].tobytes())


def _trim_result(rc, what, text, first, count):
    if rc != 0:
        raise SoundkitError(rc, what, text.value.decode())
    return first.value, count.value


class Mp4Demuxer:
    """add(bytes) / finish() -> the events that became complete: one Mp4Config, then Mp4Packets in file order.  `moov` must come before
    `mdat`; regular and fragmented files alike.  A refusal raises SoundkitError with the demuxer's text, after which it stays refused."""

    def __init__(self):
        self._h = C.c_void_p()
        check(lib.sk_mp4_demuxer_create(C.byref(self._h)), "sk_mp4_demuxer_create")
        self.config = None

    def close(self):
        if self._h:
            lib.sk_mp4_demuxer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def buffered_bytes(self):
        n = C.c_size_t(0)
        check(lib.sk_mp4_demuxer_pending(self._h, None, None, C.byref(n)), "sk_mp4_demuxer_pending")
        return n.value

    def _events(self, rc, what):
        events = []
        if self.config is None:
            self.config = _config(lib.sk_mp4_demuxer_config, self._h, "sk_mp4_demuxer_config")
            if self.config is not None:
                events.append(self.config)
        n, size = C.c_uint32(0), C.c_size_t(0)
        while True:
            check(lib.sk_mp4_demuxer_pending(self._h, C.byref(n), C.byref(size), None), "sk_mp4_demuxer_pending")
            if n.value == 0:
                break
            out, got, start, duration = np.zeros(max(size.value, 1), np.uint8), C.c_size_t(0), C.c_uint64(0), C.c_uint32(0)
            check(lib.sk_mp4_demuxer_take(self._h, _ptr(out), out.size, C.byref(got), C.byref(start), C.byref(duration)), "sk_mp4_demuxer_take")
            events.append(Mp4Packet(out[:got.value].tobytes(), start.value, duration.value))
        if rc != 0:
            error = SoundkitError(rc, what, lib.sk_mp4_demuxer_last_error(self._h).decode())
            error.events = events  # what was complete in front of the refusal
            raise error
        return events

    def add(self, data):
        b = _bytes(data)
        return self._events(lib.sk_mp4_demuxer_add(self._h, _ptr(b), len(data)), "sk_mp4_demuxer_add")

    def finish(self):
        return self._events(lib.sk_mp4_demuxer_finish(self._h), "sk_mp4_demuxer_finish")

    def trim(self, packet, decoded_frames, decoded_rate):
        """Mp4Index.trim for a packet this demuxer gave"""
        first, count, text = C.c_uint32(0), C.c_uint32(0), C.create_string_buffer(256)
        rc = lib.sk_mp4_demuxer_trim(self._h, packet.start_time, packet.duration, decoded_frames, decoded_rate, C.byref(first), C.byref(count), text, len(text))
        return _trim_result(rc, "sk_mp4_demuxer_trim", text, first, count)


class Mp4Index:
    """Mp4MediaIndex::from_file (soundkit-audio-demux/src/lib.rs:925-1080) for the chosen audio track: `moov` anywhere in the file.
    config, and samples = [(absolute offset, size, duration, start time)]; a fragmented file has none (its packets come from Mp4Demuxer)"""

    def __init__(self, handle):
        self._h = handle
        self.config = _config(lib.sk_mp4_index_info, handle, "sk_mp4_index_info")
        n = self.config.sample_count
        offsets, starts = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
        sizes, durations = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        check(lib.sk_mp4_index_samples(handle, _ptr(offsets), _ptr(sizes), _ptr(durations), _ptr(starts), n), "sk_mp4_index_samples")
        self.samples = [(int(offsets[i]), int(sizes[i]), int(durations[i]), int(starts[i])) for i in range(n)]

    def close(self):
        if self._h:
            lib.sk_mp4_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def from_file(cls, data):
        b = _bytes(data)
        h, text = C.c_void_p(), C.create_string_buffer(256)
        rc = lib.sk_mp4_index_from_file(_ptr(b), len(data), C.byref(h), text, len(text))
        if rc != 0:
            raise SoundkitError(rc, "sk_mp4_index_from_file", text.value.decode())
        return cls(h)

    def packet_bytes(self, data):
        """the samples of the file the index was made from"""
        return [bytes(data[o:o + n]) for o, n, _, _ in self.samples]

    def trim(self, sample, decoded_frames, decoded_rate):
        """resolve_pcm_packet_trim (lib.rs:117-174): the frames of sample `sample`'s decoded packet that the first edit keeps ->
        (first frame, count).  The start rounds up, the end down, both clamped to decoded_frames; nothing kept: (decoded_frames, 0);
        no edit list: (0, decoded_frames)"""
        first, count, text = C.c_uint32(0), C.c_uint32(0), C.create_string_buffer(256)
        rc = lib.sk_mp4_index_trim(self._h, sample, decoded_frames, decoded_rate, C.byref(first), C.byref(count), text, len(text))
        return _trim_result(rc, "sk_mp4_index_trim", text, first, count)


def adts_header(asc, sample_rate, channels, raw_len):
    """create_adts_header (lib.rs:4102-4120) -> the 7 bytes in front of a raw AAC sample"""
    b, out = _bytes(asc), np.zeros(7, np.uint8)
    check(lib.sk_mp4_adts_header(_ptr(b), len(asc), sample_rate, channels, raw_len, _ptr(out)), "sk_mp4_adts_header")
    return out.tobytes()


def _decode_aac(config, packets, engine):
    """-> (PCM bytes of every packet one after the other, frames per packet, the decoded rate, channels).  The AudioSpecificConfig goes
    through the AAC-LC config check first: what it refuses is no AAC-LC and ends the call with its text."""
    from .aac import AacDecoder
    from .aac_lc import AacLcError, AacLcFrontEnd
    try:
        AacLcFrontEnd(config.codec_private or b"\0").close()
    except AacLcError as e:
        raise SoundkitError(e.status, "decode_file", "Decoder initialization failed: AAC-LC decoder init: %s" % e)
    stream = b"".join(adts_header(config.codec_private, config.sample_rate, config.channels, len(p)) + p for p in packets)
    decoder = AacDecoder(engine)
    try:
        out = np.zeros(max(len(packets) * 1024 * max(config.channels, 1), 2048), np.int16)
        got, chunk = 0, stream
        while True:
            try:
                n = decoder.decode_i16(chunk, out[got:])
            except ValueError as e:
                raise SoundkitError(ERR_STREAM, "decode_file", "Decoding failed: %s" % e)
            got, chunk = got + n, b""
            if n == 0:
                break
        rate, channels = decoder.sample_rate() or config.sample_rate, decoder.channels() or config.channels
    finally:
        decoder.close()
    frames = got // channels // 1024
    return out[:got].tobytes(), [1024] * frames + [0] * (len(packets) - frames), rate, channels


def decode_file(data, options=None, scheduler=None, engine=None):
    """decode_seekable_mp4_audio for an `aac` or `alac` track, any box order: index the file -> every packet decoded -> each trimmed by
    the edit list (at the rate the decoder gave) -> the output options through alac.output_stage -> the resampler's flush.  A fragmented
    file has no sample table: its packets and their times come from the demuxer's walk.  -> (the config, [AudioData])"""
    from . import alac
    index = Mp4Index.from_file(data)
    config = index.config
    if index.samples:
        packets = index.packet_bytes(data)
        trim = index.trim
    else:
        demuxer, events = Mp4Demuxer(), []
        for at in range(0, len(data), FRAGMENT_PIECE):
            events += demuxer.add(data[at:at + FRAGMENT_PIECE])
        events += demuxer.finish()
        found = [e for e in events if isinstance(e, Mp4Packet)]
        packets = [e.data for e in found]
        trim = lambda i, n, rate: demuxer.trim(found[i], n, rate)  # noqa: E731
    if config.codec == "alac":
        cfg = alac.parse_cookie(config.codec_private)
        pcm, status, frames = alac.decode_packets(cfg, packets, engine)
        for i, st in enumerate(status):
            if st != 0:
                raise SoundkitError(alac.ERR_STREAM, "decode_file", "Decoding failed: ALAC packet %d: %s" % (i, lib.sk_strerror(st).decode()))
        rate, channels, bits = cfg["sample_rate"], cfg["channels"], cfg["bit_depth"]
    else:
        pcm, frames, rate, channels = _decode_aac(config, packets, engine)
        bits = 16
    width = channels * (bits // 8)
    pieces, at = [], 0
    for i, n in enumerate(frames):
        first, count = trim(i, n, rate)
        if count:
            pieces.append(pcm[at + first * width:at + (first + count) * width])
        at += n * width
    if not pieces:
        raise SoundkitError(ERR_STREAM, "decode_file", "Decoding failed: %sMP4 %s track emitted no audio frames" % ("" if index.samples else "fragmented ", config.codec))
    return config, alac.output_stage(pieces, rate, channels, bits, options, scheduler)

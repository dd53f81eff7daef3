"""MP4 / M4A / MOV / fragmented MP4, audio only: the host demuxer, sample index and edit-list trim (csrc/mp4_stream.h) and decode_file:
soundkit-decoder's decode_seekable_mp4_audio (lib.rs:1429-1537, with its fragmented fall-through 1539 ff.) for `aac`, `alac`, `flac`
and `pcm` tracks.  The container is walked on the host; the packets go to the decoders that were there before it -- the ADTS decoder
for AAC-LC (every sample wrapped in a 7-byte ADTS header, as the reference's AacMp4Demuxer does), the ALAC packet stage for ALAC,
FlacDecoder for FLAC (the normalised `dfLa` first, then the packets) and, for PCM, the output stage alone: the runs of frames are the
audio.  64-bit float PCM is rounded to f32 on the GPU first (Engine.aiff_decode), which the reference does not do: it refuses 64 bits.

A stream handed to the scheduler needs none of this: `spawn()` sniffs `ftyp` (csrc/pipeline.cpp) and demuxes on an entropy thread
(an AAC track as ADTS frames, a `fLaC` track as a FLAC stream, an integer or f32 PCM track as a raw PCM stream; no edit trim).  Not built: `flac` and `pcm` tracks of a fragmented file, edits behind the first media edit, video."""
import ctypes as C

import numpy as np

from ._lib import Mp4PcmInfo, Mp4TrackInfo, SoundkitError, check, lib
from .engine import _ptr

ERR_STREAM = -901
CODECS = {1: "aac", 2: "alac", 3: "flac", 4: "pcm"}
FRAGMENT_PIECE = 64 * 1024  # what decode_fragmented_mp4_audio feeds its demuxer at a time


def _bytes(data):
    return np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)


class Mp4Config:
    """the config event: codec ("aac" / "alac"), sample_rate, channels, bits_per_sample, track_id, timescale, sample_count, fragmented,
    codec_private (the AudioSpecificConfig, or the ALAC cookie in its MP4 wrapping) and edit = (presentation start, media start, duration)
    in the track's timescale, or None.  codec "flac": codec_private is `fLaC` and the metadata blocks (what FlacDecoder takes before
    the packets).  codec "pcm": pcm = {codec_id (the sample entry's name), big_endian, is_float, bits_per_sample, bytes_per_frame,
    frames_per_packet (0: not stated)}; None for every other codec"""

    def __init__(self, info, private, pcm=None):
        self.codec = CODECS[info.codec]
        self.pcm = None
        if pcm is not None and info.codec == 4:
            self.pcm = {"codec_id": bytes(pcm.codec_id).decode("latin-1"), "big_endian": bool(pcm.big_endian), "is_float": bool(pcm.is_float),
                        "bits_per_sample": int(pcm.bits_per_sample), "bytes_per_frame": int(pcm.bytes_per_frame),
                        "frames_per_packet": int(pcm.frames_per_packet)}
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


def _config(fn, handle, what, pcm_fn=None):
    info = Mp4TrackInfo()
    rc = fn(handle, C.byref(info), None, 0)
    if rc not in (0, -7):
        check(rc, what)
    if info.codec == 0:
        return None
    private = np.zeros(max(int(info.private_len), 1), np.uint8)
    check(fn(handle, C.byref(info), _ptr(private), private.size), what)
    pcm = Mp4PcmInfo()
    if pcm_fn is not None:
        check(pcm_fn(handle, C.byref(pcm)), what)
    return Mp4Config(info, private[:info.private_len].tobytes(), pcm)


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
            self.config = _config(lib.sk_mp4_demuxer_config, self._h, "sk_mp4_demuxer_config", lib.sk_mp4_demuxer_pcm_info)
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
        self.config = _config(lib.sk_mp4_index_info, handle, "sk_mp4_index_info", lib.sk_mp4_index_pcm_info)
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


def flac_config(data):
    """normalize_mp4_flac_decoder_configuration (soundkit-audio-demux/src/lib.rs:1277-1302): data that begins with `fLaC`, a bare 34-byte
    STREAMINFO or a `dfLa` payload -> `fLaC` and the metadata blocks.  Raises SoundkitError with the reference's text."""
    b, n, text = _bytes(data), C.c_size_t(0), C.create_string_buffer(256)
    out = np.zeros(len(data) + 16, np.uint8)
    rc = lib.sk_mp4_flac_config(_ptr(b), len(data), _ptr(out), out.size, C.byref(n), text, len(text))
    if rc != 0:
        raise SoundkitError(rc, "sk_mp4_flac_config", text.value.decode())
    return out[:n.value].tobytes()


def _decode_flac(config, packets, engine):
    """-> (PCM bytes of every packet one after the other, frames per packet, rate, channels, bits).  The config goes in first and must
    give no samples; a packet is one FLAC frame, whose header states how many sample frames it holds."""
    from . import flac
    decoder = flac.FlacDecoder(engine)
    try:
        out, got = np.zeros(1 << 18, np.int32), []

        def feed(piece):
            try:
                n = decoder.decode_i32(piece, out)
                got.append(out[:n].copy())
                while decoder.pending_samples():  # frames that found no room
                    got.append(out[:decoder.decode_i32(b"", out)].copy())
            except SoundkitError as e:
                raise SoundkitError(e.status, "decode_file", "Decoding failed: %s" % e)

        try:
            n = decoder.decode_i32(config.codec_private, out)
        except SoundkitError as e:
            raise SoundkitError(e.status, "decode_file", "Decoder initialization failed: %s" % e)
        if n != 0 or decoder.pending_samples():
            raise SoundkitError(ERR_STREAM, "decode_file", "Decoder initialization failed: MP4 FLAC configuration unexpectedly contained audio frames")
        rate, channels, bits = decoder.sample_rate(), decoder.channels(), decoder.bits_per_sample()
        if not rate or not channels or not bits:
            raise SoundkitError(ERR_STREAM, "decode_file", "Decoding failed: MP4 FLAC has no sample rate")
        if bits not in (16, 24, 32):
            raise SoundkitError(ERR_STREAM, "decode_file", "Decoding failed: MP4 FLAC of %d bits per sample is not built" % bits)
        info = flac.streaminfo(rate, channels, bits)
        frames = []
        for i, p in enumerate(packets):
            rc, head = flac.parse_header(p, info)
            if rc != 0:
                raise SoundkitError(ERR_STREAM, "decode_file", "Decoding failed: MP4 FLAC packet %d: %s" % (i, lib.sk_strerror(rc).decode()))
            frames.append(head["block_size"])
        for at in range(0, len(packets), 64):
            feed(b"".join(packets[at:at + 64]))
        while True:  # a call with no bytes finalises the stream and drains what is left
            n = decoder.decode_i32(b"", out)
            if n == 0:
                break
            got.append(out[:n].copy())
    finally:
        decoder.close()
    samples = np.concatenate(got) if got else np.zeros(0, np.int32)
    if samples.size != sum(frames) * channels:
        raise SoundkitError(ERR_STREAM, "decode_file", "Decoding failed: MP4 FLAC packets decoded to %d samples where their headers state %d"
                            % (samples.size, sum(frames) * channels))
    if bits == 16:
        pcm = samples.astype("<i2").tobytes()
    elif bits == 24:
        pcm = samples.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    else:
        pcm = samples.astype("<i4").tobytes()
    return pcm, frames, rate, channels, bits


def container_pcm(pcm, sample_rate, channels, bits, is_float, big_endian, engine=None):
    """make_container_pcm_audio's check (soundkit-decoder/src/lib.rs:1829-1863) for the bytes of a container's PCM track ->
    (bytes, bits, big_endian) as the output stage takes them: 16 / 24 / 32 bits as they are; 64-bit float rounded to f32 little-endian on
    the GPU (beyond the reference, which refuses 64 bits); any other width `unsupported container PCM sample depth: N`."""
    from .engine import AIFF_F64BE, AIFF_F64LE, default_engine
    if bits == 64 and is_float:
        return (engine or default_engine()).aiff_decode(AIFF_F64BE if big_endian else AIFF_F64LE, channels, pcm), 32, False
    if bits not in (16, 24, 32) or (is_float and bits != 32):
        raise SoundkitError(ERR_STREAM, "decode_file", "unsupported container PCM sample depth: %d" % bits)
    return pcm, bits, big_endian


def decode_file(data, options=None, scheduler=None, engine=None):
    """decode_seekable_mp4_audio for an `aac`, `alac`, `flac` or `pcm` track, any box order: index the file -> every packet decoded -> each trimmed by
    the edit list (at the rate the decoder gave) -> the output options through alac.output_stage -> the resampler's flush.  A fragmented
    file has no sample table: its packets and their times come from the demuxer's walk.  -> (the config, [AudioData])"""
    from . import alac
    index = Mp4Index.from_file(data)
    config = index.config
    is_float = big_endian = False
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
    elif config.codec == "flac":
        if not index.samples:
            raise SoundkitError(ERR_STREAM, "decode_file", "Decoding failed: fragmented MP4 flac tracks are not built")
        pcm, frames, rate, channels, bits = _decode_flac(config, packets, engine)
    elif config.codec == "pcm":
        if not index.samples:
            raise SoundkitError(ERR_STREAM, "decode_file", "Decoding failed: fragmented MP4 pcm tracks are not built")
        rate, channels, p = config.sample_rate, config.channels, config.pcm
        in_width = channels * ((config.bits_per_sample + 7) // 8)
        if in_width == 0 or p["bytes_per_frame"] != in_width:
            raise SoundkitError(ERR_STREAM, "decode_file", "Decoding failed: MP4 PCM frames of %d bytes are not %d channels of %d packed bits"
                                % (p["bytes_per_frame"], channels, config.bits_per_sample))
        for i, b in enumerate(packets):
            if len(b) % in_width:
                raise SoundkitError(ERR_STREAM, "decode_file", "Decoding failed: decoder returned misaligned PCM")
        frames = [len(b) // in_width for b in packets]
        pcm, bits, big_endian = container_pcm(b"".join(packets), rate, channels, config.bits_per_sample, p["is_float"], big_endian=p["big_endian"], engine=engine)
        is_float = p["is_float"]
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
    return config, alac.output_stage(pieces, rate, channels, bits, options, scheduler, is_float=is_float, big_endian=big_endian)

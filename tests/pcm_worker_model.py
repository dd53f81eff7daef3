"""A small CPU model of the reference worker's WAV / raw PCM path.  TEST INFRASTRUCTURE ONLY (a plain module).

Written from the reference, not from this library's C++: WavStreamProcessor::add with install_fmt / install_ds64
(soundkit/src/wav.rs:95-324), RawPcmStreamProcessor::add / flush (soundkit/src/raw_pcm.rs:150-190), the worker's detection
gathering and one-`process`-per-chunk loop (soundkit-decoder/src/lib.rs:2926-3029) and apply_output_options' routing
(lib.rs:3324-3456, emit_resampled_chunks :3261-3290, flush :3292-3322), with the arithmetic taken from oracle.oracle.

oracle.StreamingResampler.process returns a call's outputs joined, so the model feeds it pieces that end on the 4096-frame
boundaries (as decoder.StreamingResampler.process_chunks does) to get one output per completed chunk."""
import struct

import numpy as np

MIN_DETECTION_BYTES, MAX_DETECTION_BYTES = 8192, 65536  # lib.rs:75-76
MAX_WAV_FMT_BYTES = 4096                                # wav.rs:20
CHUNK = 4096                                            # RESAMPLE_CHUNK_SIZE, lib.rs:79
FMT_S16LE, FMT_S16BE, FMT_S24LE, FMT_S24BE, FMT_S32LE, FMT_S32BE, FMT_F32LE, FMT_F32BE = range(8)


class WavModel:
    """wav.rs:95-324.  add(chunk) -> None or the piece's bytes; ValueError(text) on a rejected stream."""

    def __init__(self):
        self.buf, self.state = bytearray(), "initial"
        self.bits = self.channels = self.rate = 0
        self.is_float = self.rf64 = False
        self.ds64 = None
        self.data_size = 0

    def total_frames(self):
        frame = self.bits // 8 * self.channels
        return self.data_size // frame if frame and self.data_size else 0

    def add(self, chunk):
        self.buf += chunk
        while True:
            state, self.state = self.state, "finished"  # an error return leaves the processor finished
            if state == "initial":
                if len(self.buf) < 12:
                    self.state = "initial"
                    return None
                self.rf64 = self.buf[:4] == b"RF64"
                if (not self.rf64 and self.buf[:4] != b"RIFF") or self.buf[8:12] != b"WAVE":
                    raise ValueError("Not a WAV file")
                del self.buf[:12]
                self.state = "header"
            elif state == "header":
                if len(self.buf) < 8:
                    self.state = "header"
                    return None
                kind, size = bytes(self.buf[:4]), struct.unpack("<I", self.buf[4:8])[0]
                del self.buf[:8]
                if kind == b"data":
                    if not (self.bits and self.channels and self.rate):
                        raise ValueError("WAV data appears before a valid fmt chunk")
                    if self.rf64 and size == 0xffffffff:
                        if self.ds64 is None:
                            raise ValueError("RF64 data chunk appears before a valid ds64 chunk")
                        size = self.ds64
                    self.data_size = self.remaining = size
                    self.state = "data" if size else "finished"
                else:
                    if kind in (b"fmt ", b"ds64") and size > MAX_WAV_FMT_BYTES:
                        raise ValueError("WAV fmt chunk exceeds the %d byte metadata budget" % MAX_WAV_FMT_BYTES)
                    self.kind, self.remaining, self.padding, self.payload = kind, size, bool(size & 1), bytearray()
                    self.state = "payload"
            elif state == "payload":
                n = min(self.remaining, len(self.buf))
                if self.kind in (b"fmt ", b"ds64"):
                    self.payload += self.buf[:n]
                del self.buf[:n]
                self.remaining -= n
                if self.remaining or (self.padding and not self.buf):
                    self.state = "payload"
                    return None
                if self.padding:
                    del self.buf[:1]
                    self.padding = False
                if self.kind == b"fmt ":
                    self._fmt(bytes(self.payload))
                elif self.kind == b"ds64":
                    self._ds64(bytes(self.payload))
                self.state = "header"
            elif state == "data":
                frame = self.bits // 8 * self.channels
                if frame == 0:
                    raise ValueError("WAV fmt has zero bytes per frame")
                n = min(self.remaining, len(self.buf)) // frame * frame
                if n == 0:
                    if len(self.buf) >= self.remaining > 0:
                        raise ValueError("WAV data chunk is not frame-aligned")
                    self.state = "data"
                    return None
                piece = bytes(self.buf[:n])
                del self.buf[:n]
                self.remaining -= n
                self.state = "data" if self.remaining else "finished"
                return piece
            else:
                return None

    def _fmt(self, p):
        if len(p) < 16:
            raise ValueError("WAV fmt chunk must contain at least 16 bytes")
        tag = struct.unpack("<H", p[:2])[0]
        if tag == 0xfffe:
            if len(p) < 40:
                raise ValueError("WAVE_FORMAT_EXTENSIBLE fmt chunk is truncated")
            tag = struct.unpack("<H", p[24:26])[0]
        self.channels, self.rate = struct.unpack("<HI", p[2:8])
        self.bits = struct.unpack("<H", p[14:16])[0]
        if tag not in (1, 3):
            raise ValueError("unsupported WAV format tag %d" % tag)
        self.is_float = tag == 3
        if not (self.channels and self.rate and self.bits):
            raise ValueError("WAV fmt contains invalid audio geometry")
        if self.bits % 8:
            raise ValueError("WAV sample width must be byte-aligned")

    def _ds64(self, p):
        if not self.rf64:
            raise ValueError("ds64 chunk requires an RF64 header")
        if len(p) < 28:
            raise ValueError("RF64 ds64 chunk is truncated")
        size, = struct.unpack("<Q", p[8:16])
        table, = struct.unpack("<I", p[24:28])
        if len(p) < 28 + 12 * table:
            raise ValueError("RF64 ds64 table is truncated")
        self.ds64 = size


class RawModel:
    """raw_pcm.rs:150-190"""

    def __init__(self, bytes_per_frame):
        self.frame, self.buf = bytes_per_frame, bytearray()

    def add(self, chunk):
        self.buf += chunk
        n = len(self.buf) // self.frame * self.frame
        if n == 0:
            return None
        piece = bytes(self.buf[:n])
        del self.buf[:n]
        return piece

    def flush(self):
        if self.buf:
            raise ValueError("Raw PCM stream ended with %d trailing partial-frame byte(s)" % len(self.buf))


def wav_pieces(chunks):
    """the pieces a worker hands on for a WAV stream received in `chunks`: detection gathering (lib.rs:2926-3003), then one
    process per chunk.  -> (WavModel, [piece bytes], the text that ended the stream or None)"""
    wav, pieces, gathered, detected = WavModel(), [], bytearray(), False
    try:
        _wav_pieces(wav, pieces, gathered, detected, chunks)
    except ValueError as e:
        return wav, pieces, str(e)
    return wav, pieces, None


def _wav_pieces(wav, pieces, gathered, detected, chunks):

    def process(data):
        piece = wav.add(data)
        if piece:
            pieces.append(piece)
    for chunk in chunks:
        if not chunk:
            continue
        if detected:
            process(chunk)
            continue
        probe = min(MAX_DETECTION_BYTES - len(gathered), len(chunk))
        gathered += chunk[:probe]
        if len(gathered) >= MIN_DETECTION_BYTES:
            detected = True
            process(bytes(gathered))
            if probe < len(chunk):
                process(chunk[probe:])
    if not detected:  # end of stream while detecting
        process(bytes(gathered))


def fmt_of(bits, is_float, big_endian):
    if is_float:
        if bits != 32:
            raise ValueError("floating-point PCM must contain 32-bit samples")
        return FMT_F32BE if big_endian else FMT_F32LE
    table = {16: FMT_S16LE, 24: FMT_S24LE, 32: FMT_S32LE}
    if bits not in table:
        raise ValueError("PCM data is unsupported or contains a partial frame")
    return table[bits] + (1 if big_endian else 0)


class OutputStage:
    """apply_output_options for one stream (lib.rs:3324-3456): call piece(bytes) per AudioData, then flush().
    Every output is (bits, channels, rate, is_float, big_endian, bytes)."""

    def __init__(self, O, rate, channels, bits, is_float=False, big_endian=False, out_bits=None, out_rate=None, out_channels=None):
        self.O, self.rate, self.channels, self.bits, self.is_float, self.big_endian = O, rate, channels, bits, is_float, big_endian
        self.t_rate, self.t_bits, self.t_ch = out_rate or rate, out_bits or bits, out_channels or channels
        self.rs, self.fill = None, 0

    def _emit(self, planar, out_float):  # emit_resampled_chunks, lib.rs:3261-3290
        O, ch = self.O, planar.shape[0]
        if self.t_ch < ch:
            assert self.t_ch == 1
            planar, ch = O.downmix_mono(planar)[None, :], 1
        fmt = FMT_F32LE if out_float else {16: FMT_S16LE, 24: FMT_S24LE, 32: FMT_S32LE}[self.t_bits]
        return (self.t_bits, ch, self.t_rate, out_float, False, O.f32_planar_to_bytes(fmt, planar).tobytes())

    def piece(self, data):
        O = self.O
        if (self.t_rate, self.t_bits, self.t_ch) == (self.rate, self.bits, self.channels):  # fast path
            return [(self.bits, self.channels, self.rate, self.is_float, self.big_endian, bytes(data))]
        if self.t_rate == self.rate and self.t_ch == self.channels and self.t_bits == 16 and not self.is_float and self.bits in (24, 32):
            fmt = fmt_of(self.bits, False, self.big_endian)
            return [(16, self.channels, self.rate, False, False, O.exact_signed_pcm_to_i16(fmt, np.frombuffer(data, np.uint8)).tobytes())]
        out_float = self.t_bits == 32 and self.is_float
        fmt = fmt_of(self.bits, self.is_float, self.big_endian)
        planar = O.decoder_bytes_to_f32_planar(fmt, np.frombuffer(data, np.uint8), self.channels)
        if self.t_rate == self.rate:
            return [self._emit(planar, out_float)]
        if self.rs is None:
            self.rs = O.StreamingResampler(self.rate, self.t_rate, self.channels)
        outs, pos = [], 0
        while pos < planar.shape[1]:  # pieces that end on the chunk boundaries: one output per completed chunk
            n = min(planar.shape[1] - pos, CHUNK - self.fill)
            got = self.rs.process(planar[:, pos:pos + n])
            self.fill = (self.fill + n) % CHUNK
            pos += n
            if got.shape[1]:
                outs.append(self._emit(got, out_float))
        return outs

    def flush(self):  # lib.rs:3292-3322
        if self.rs is None:
            return []
        got = self.rs.flush()
        self.rs = None
        return [self._emit(got, self.t_bits == 32 and self.is_float)] if got.shape[1] else []


def wav_worker(O, chunks, out_bits=None, out_rate=None, out_channels=None):
    """a WAV stream through the worker -> (outputs, error text or None)"""
    outs = []
    wav, pieces, err = wav_pieces(chunks)
    stage = OutputStage(O, wav.rate, wav.channels, wav.bits, wav.is_float, False, out_bits, out_rate, out_channels) if pieces else None
    for p in pieces:
        outs += stage.piece(p)
    if err is not None:  # an error ends the stream behind the outputs before it; nothing is flushed (lib.rs:3131-3134)
        return outs, "Decoding failed: %s" % err
    return outs + (stage.flush() if stage else []), None


def raw_worker(O, chunks, rate, channels, fmt, out_bits=None, out_rate=None, out_channels=None):
    """a raw PCM stream through the worker -> (outputs, error text or None)"""
    bits = 16 if fmt <= FMT_S16BE else (24 if fmt <= FMT_S24BE else 32)
    raw = RawModel(bits // 8 * channels)
    stage = OutputStage(O, rate, channels, bits, fmt >= FMT_F32LE, bool(fmt & 1), out_bits, out_rate, out_channels)
    outs = []
    for chunk in chunks:
        if chunk:
            piece = raw.add(chunk)
            if piece:
                outs += stage.piece(piece)
    try:
        raw.flush()
    except ValueError as e:
        return outs, "Decoding failed: %s" % e
    return outs + stage.flush(), None


def ragged(data, rng, lo=1, hi=None):
    """`data` cut into seeded ragged chunks of lo ... hi bytes"""
    hi = hi or len(data)
    out, pos = [], 0
    while pos < len(data):
        n = int(rng.integers(lo, hi + 1))
        out.append(bytes(data[pos:pos + n]))
        pos += n
    return out

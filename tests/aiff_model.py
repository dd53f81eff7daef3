"""A model of the reference's incremental AIFF / AIFF-C decoder (soundkit-aiff: AiffDecoder.add, parse_available, parse_stream_info,
parse_extended_sample_rate, decode_stream_bytes), written from its behaviour: the FORM / COMM / SSND walk with every limit and error
text, and the per-sample work (byte reversal, widening, f64 -> f32, G.711 expansion, IMA4 ADPCM with the QuickTime carry rule).

AiffModel.add(chunk) -> None or Audio(rate, channels, bits, is_float, data) and raises ValueError(text); add(b"") finalises.
`pieces` records, per add that produced audio, the source-encoded whole groups it consumed (what sk_aiff_reader_add returns).
decode(encoding, channels, data, state) is the per-sample stage by itself."""
import collections
import math
import struct
from decimal import Decimal

import numpy as np

(U8, S8, S16BE, S16LE, S24BE, S32BE, S32LE, F32BE, F64BE, ULAW, ALAW, IMA4) = range(12)
NAMES = ["U8", "S8", "S16BE", "S16LE", "S24BE", "S32BE", "S32LE", "F32BE", "F64BE", "ULAW", "ALAW", "IMA4"]
MAX_CHANNELS, MAX_COMM_BYTES, MAX_INPUT_CHUNK_BYTES = 32, 4096, 4 * 1024 * 1024

Audio = collections.namedtuple("Audio", "sample_rate channels bits is_float data")

STEP = [7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
        157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552,
        1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487,
        12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767]
INDEX = [-1, -1, -1, -1, 2, 4, 6, 8]


def group_bytes(enc, channels):
    return {U8: 1, S8: 1, ULAW: 1, ALAW: 1, S16BE: 2, S16LE: 2, S24BE: 3, S32BE: 4, S32LE: 4, F32BE: 4, F64BE: 8}.get(enc, 34 * channels)


def contract(enc):
    """(bits, is_float) of what the decoder emits"""
    if enc in (F32BE, F64BE):
        return 32, True
    return (24 if enc == S24BE else 32 if enc in (S32BE, S32LE) else 16), False


def _ulaw_table():
    out = np.zeros(256, np.int16)
    for code in range(256):
        u = ~code & 0xff
        t = (((u & 0x0f) << 3) + 0x84) << ((u >> 4) & 7)
        out[code] = (0x84 - t) if u & 0x80 else (t - 0x84)
    return out


def _alaw_table():
    out = np.zeros(256, np.int16)
    for code in range(256):
        a = code ^ 0x55
        seg = (a >> 4) & 7
        t = (a & 0x0f) << 4
        t = t + 8 if seg == 0 else (t + 0x108) << (seg - 1)
        out[code] = t if a & 0x80 else -t
    return out


ULAW_TABLE, ALAW_TABLE = _ulaw_table(), _alaw_table()


def ima4_packet(packet, state, carry=True):
    """One 34-byte packet -> 64 samples; state = [predictor, step_index] of the channel, updated.  The QuickTime rule: a header with
    the carried step index and a predictor within 0x7f of the carried one continues from the carried predictor; any other restarts."""
    word = (packet[0] << 8) | packet[1]
    hp = word & 0xff80
    hp = hp - 0x10000 if hp & 0x8000 else hp
    hx = min(word & 0x7f, 88)
    p = state[0] if carry and state[1] == hx and abs(hp - state[0]) <= 0x7f else hp
    idx = hx
    out = np.zeros(64, np.int16)
    for t in range(64):
        byte = packet[2 + (t >> 1)]
        n = (byte >> 4) if t & 1 else (byte & 15)
        step = STEP[idx]
        d = step >> 3
        if n & 1:
            d += step >> 2
        if n & 2:
            d += step >> 1
        if n & 4:
            d += step
        p = max(-32768, min(32767, p - d if n & 8 else p + d))
        idx = max(0, min(88, idx + INDEX[n & 7]))
        out[t] = p
    state[0], state[1] = p, idx
    return out


def decode(enc, channels, data, state=None, carry=True):
    """whole groups of `data` -> contract PCM bytes; state = [[predictor, step_index]] * 2 for IMA4, updated"""
    raw = np.frombuffer(bytes(data), np.uint8)
    if enc == U8:
        return ((raw.astype(np.int16) - 128) << 8).astype("<i2").tobytes()
    if enc == S8:
        return (raw.view(np.int8).astype(np.int16) << 8).astype("<i2").tobytes()
    if enc in (S16LE, S32LE):
        return raw.tobytes()
    if enc in (S16BE, S24BE, S32BE, F32BE):
        n = group_bytes(enc, 1)
        return raw.reshape(-1, n)[:, ::-1].tobytes()
    if enc == F64BE:
        with np.errstate(over="ignore", invalid="ignore"):
            return raw.view(">f8").astype("<f4").tobytes()
    if enc == ULAW:
        return ULAW_TABLE[raw].astype("<i2").tobytes()
    if enc == ALAW:
        return ALAW_TABLE[raw].astype("<i2").tobytes()
    groups = raw.reshape(-1, channels, 34)
    out = np.zeros((len(groups), 64, channels), "<i2")
    for g in range(len(groups)):
        for c in range(channels):
            out[g, :, c] = ima4_packet(groups[g, c].tolist(), state[c], carry)
    return out.tobytes()


def display_f64(v):
    """Rust's `{}` of an f64: the shortest digits that read back, never an exponent"""
    if v != v:
        return "NaN"
    if math.isinf(v):
        return "inf" if v > 0 else "-inf"
    text = format(Decimal(repr(v)), "f")
    return text[:-2] if text.endswith(".0") else text


def lossy(b):
    return bytes(b).decode("utf-8", errors="replace")


def parse_extended_sample_rate(d):
    word = (d[0] << 8) | d[1]
    if word & 0x8000:
        raise ValueError("AIFF sample rate is negative")
    exponent = word & 0x7fff
    mantissa = int.from_bytes(d[2:10], "big")
    if exponent == 0 and mantissa == 0:
        raise ValueError("AIFF sample rate is zero")
    if exponent == 0x7fff:
        raise ValueError("AIFF sample rate is not finite")
    # 2f64.powi(n) by repeated multiplication, and 1 / 2^-n for n < 0: inf beyond 2^1023, hence 0 below 2^-1023
    n = exponent - 16383 - 63
    scale = math.inf if n > 1023 else 0.0 if n < -1023 else math.ldexp(1.0, n)
    m = float(mantissa)
    value = m * scale if not (m == 0 and math.isinf(scale)) else math.nan
    if not math.isfinite(value) or value <= 0.0 or value > 4294967295.0:
        raise ValueError("Invalid AIFF sample rate: " + display_f64(value))
    return int(math.floor(value + 0.5)) if value < 2 ** 52 else int(value)  # f64::round: halves away from zero


def parse_stream_info(d, aifc):
    if len(d) < 18:
        raise ValueError("AIFF COMM is shorter than 18 bytes")
    channels = (d[0] << 8) | d[1]
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError("invalid AIFF channel count: %d" % channels)
    sample_size = (d[6] << 8) | d[7]
    rate = parse_extended_sample_rate(d[8:18])

    def signed_be():
        if 1 <= sample_size <= 8:
            return S8
        if sample_size <= 16 and sample_size >= 9:
            return S16BE
        if 17 <= sample_size <= 24:
            return S24BE
        if 25 <= sample_size <= 32:
            return S32BE
        raise ValueError("unsupported AIFF sample size: %d" % sample_size)

    if not aifc:
        enc = signed_be()
    else:
        if len(d) < 22:
            raise ValueError("AIFF-C COMM has no compression type")
        tag = bytes(d[18:22])
        tags = {b"raw ": U8, b"twos": S16BE, b"sowt": S16LE, b"in24": S24BE, b"in32": S32BE, b"23ni": S32LE, b"FL32": F32BE, b"fl32": F32BE,
                b"FL64": F64BE, b"fl64": F64BE, b"ULAW": ULAW, b"ulaw": ULAW, b"ALAW": ALAW, b"alaw": ALAW, b"ima4": IMA4}
        if tag == b"NONE":
            enc = signed_be()
        elif tag in tags:
            enc = tags[tag]
        else:
            raise ValueError("unsupported AIFF-C compression type: " + lossy(tag))
    if enc == IMA4 and channels > 2:
        raise ValueError("AIFF-C IMA4 supports at most two channels")
    return rate, channels, enc


class AiffModel:
    def __init__(self, carry=True):
        self.buffer = bytearray()
        self.pending = bytearray()
        self.state = ("FormHeader",)
        self.aifc = None
        self.info = None  # (rate, channels, encoding)
        self.form_remaining = 0
        self.padding_next = ("ChunkHeader",)
        self.ima = [[0, 0], [0, 0]]
        self.finished = False
        self.carry = carry
        self.pieces = []  # source-encoded whole groups, one entry per add that produced audio
        self.error = None

    def buffered_bytes(self):
        return len(self.buffer) + len(self.pending)

    def debug_state(self):
        s = self.state
        tf = lambda b: "true" if b else "false"
        if s[0] in ("FormHeader", "ChunkHeader", "Padding", "Done"):
            return s[0]
        if s[0] == "Comm":
            return "Comm { size: %d, padded: %s }" % (s[1], tf(s[2]))
        if s[0] == "SsndOffset":
            return "SsndOffset { skip: %d, remaining_audio: %d, padded: %s }" % (s[1], s[2], tf(s[3]))
        return "%s { remaining: %d, padded: %s }" % (s[0], s[1], tf(s[2]))

    def add(self, data):
        if self.error is not None:  # (what a failed decoder does next is not the reference's concern: the stream has ended)
            raise ValueError(self.error)
        try:
            return self._add(bytes(data))
        except ValueError as exc:
            if "streaming budget" not in str(exc):
                self.error = str(exc)
            raise

    def _add(self, data):
        if self.finished:
            return None
        if len(data) > MAX_INPUT_CHUNK_BYTES:
            raise ValueError("AIFF input chunk exceeds the %d byte streaming budget" % MAX_INPUT_CHUNK_BYTES)
        finalizing = len(data) == 0
        self.buffer += data
        self._source = bytearray()
        pcm = self._parse_available()
        if finalizing:
            if self.state[0] != "Done":
                raise ValueError("truncated AIFF stream in state " + self.debug_state())
            if self.pending:
                raise ValueError("AIFF sound data ends inside an encoded sample group")
            self.finished = True
        if not pcm:
            return None
        if self.info is None:
            raise ValueError("AIFF PCM arrived before COMM metadata")
        self.pieces.append(bytes(self._source))
        bits, is_float = contract(self.info[2])
        return Audio(self.info[0], self.info[1], bits, is_float, bytes(pcm))

    def _consume_form(self, n):
        if n > self.form_remaining:
            raise ValueError("AIFF parser crossed the FORM boundary")
        self.form_remaining -= n

    def _next_chunk_state(self):
        return ("Done",) if self.form_remaining == 0 else ("ChunkHeader",)

    def _finish_chunk(self, padded):
        nxt = self._next_chunk_state()
        if padded:
            self.padding_next = nxt
            self.state = ("Padding",)
        else:
            self.state = nxt

    def _decode_stream_bytes(self, data, pcm):
        rate, channels, enc = self.info
        self.pending += data
        g = group_bytes(enc, channels)
        whole = len(self.pending) // g * g
        complete, self.pending = bytes(self.pending[:whole]), bytearray(self.pending[whole:])
        self._source += complete
        pcm += decode(enc, channels, complete, self.ima, self.carry)

    def _parse_available(self):
        pos = 0
        pcm = bytearray()
        buf = self.buffer
        while True:
            avail = len(buf) - pos
            s = self.state
            if s[0] == "FormHeader":
                if avail < 12:
                    break
                h = bytes(buf[pos:pos + 12])
                if h[:4] != b"FORM":
                    raise ValueError("AIFF stream does not start with FORM")
                form_size = int.from_bytes(h[4:8], "big")
                if form_size < 4:
                    raise ValueError("AIFF FORM is shorter than its type field")
                if h[8:12] == b"AIFF":
                    self.aifc = False
                elif h[8:12] == b"AIFC":
                    self.aifc = True
                else:
                    raise ValueError("unsupported FORM type " + lossy(h[8:12]))
                self.form_remaining = form_size - 4
                pos += 12
                self.state = self._next_chunk_state()
            elif s[0] == "ChunkHeader":
                if self.form_remaining == 0:
                    self.state = ("Done",)
                    continue
                if self.form_remaining < 8:
                    raise ValueError("AIFF FORM ends inside a chunk header")
                if avail < 8:
                    break
                cid = bytes(buf[pos:pos + 4])
                size = int.from_bytes(buf[pos + 4:pos + 8], "big")
                self._consume_form(8)
                pos += 8
                padded = bool(size & 1)
                if size + padded > self.form_remaining:
                    raise ValueError("AIFF chunk %s exceeds the FORM boundary" % lossy(cid))
                if cid == b"COMM":
                    if size > MAX_COMM_BYTES:
                        raise ValueError("AIFF COMM exceeds the %d byte budget" % MAX_COMM_BYTES)
                    self.state = ("Comm", size, padded)
                elif cid == b"SSND":
                    if size < 8:
                        raise ValueError("AIFF SSND is shorter than its header")
                    if self.info is None:
                        raise ValueError("AIFF SSND appears before COMM")
                    self.state = ("SsndHeader", size, padded)
                else:
                    self.state = ("Skip", size, padded)
            elif s[0] == "Comm":
                size, padded = s[1], s[2]
                if avail < size:
                    break
                self.info = parse_stream_info(bytes(buf[pos:pos + size]), self.aifc)
                self._consume_form(size)
                pos += size
                self._finish_chunk(padded)
            elif s[0] == "SsndHeader":
                remaining, padded = s[1], s[2]
                if avail < 8:
                    break
                offset = int.from_bytes(buf[pos:pos + 4], "big")
                if offset > remaining - 8:
                    raise ValueError("AIFF SSND offset exceeds its chunk")
                self._consume_form(8)
                pos += 8
                self.state = ("SsndOffset", offset, remaining - 8 - offset, padded)
            elif s[0] == "SsndOffset":
                skip, audio, padded = s[1], s[2], s[3]
                take = min(avail, skip)
                pos += take
                self._consume_form(take)
                if take == skip:
                    self.state = ("Audio", audio, padded)
                else:
                    self.state = ("SsndOffset", skip - take, audio, padded)
                    break
            elif s[0] == "Audio":
                remaining, padded = s[1], s[2]
                take = min(avail, remaining)
                self._decode_stream_bytes(bytes(buf[pos:pos + take]), pcm)
                pos += take
                self._consume_form(take)
                if take == remaining:
                    if self.pending:
                        raise ValueError("AIFF SSND ends inside an encoded sample group")
                    self._finish_chunk(padded)
                else:
                    self.state = ("Audio", remaining - take, padded)
                    break
            elif s[0] == "Skip":
                remaining, padded = s[1], s[2]
                take = min(avail, remaining)
                pos += take
                self._consume_form(take)
                if take == remaining:
                    self._finish_chunk(padded)
                else:
                    self.state = ("Skip", remaining - take, padded)
                    break
            elif s[0] == "Padding":
                if avail == 0:
                    break
                pos += 1
                self._consume_form(1)
                self.state = self.padding_next
            else:  # Done
                if avail != 0:
                    raise ValueError("AIFF stream has bytes after the FORM boundary")
                break
        del buf[:pos]
        return pcm


def decode_file(data, piece=None, carry=True):
    """the whole file through the model in pieces of `piece` bytes (None: one add) plus the finalising add -> (list of Audio, model)"""
    m = AiffModel(carry)
    outs = []
    step = piece or max(len(data), 1)
    for at in range(0, len(data), step):
        a = m.add(data[at:at + step])
        if a is not None:
            outs.append(a)
    a = m.add(b"")
    if a is not None:
        outs.append(a)
    return outs, m

"""A plain-Python restatement of the MPEG-TS audio demuxer (csrc/ts_stream.h), written from the container's rules and the reference's
checks and texts: demux(data) -> ([("config", {...}) | ("packet", {...})], the refusal's text or None).  It sees the whole input at
once; the demuxer under test must give the same events however the bytes are cut.  Events in front of a refusal are kept."""

MAX_CHUNK, MAX_PES = 4 * 1024 * 1024, 1024 * 1024
ADTS_RATES = (96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 7350)
KBPS = {(True, 1): (32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384, 416, 448),
        (True, 2): (32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384),
        (True, 3): (32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320),
        (False, 1): (32, 48, 56, 64, 80, 96, 112, 128, 144, 160, 176, 192, 224, 256),
        (False, 2): (8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160),
        (False, 3): (8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160)}


class Refused(Exception):
    pass


def crc32_mpeg2(data):
    crc = 0xffffffff
    for b in data:
        crc ^= b << 24
        for _ in range(8):
            crc = ((crc << 1) ^ 0x04C11DB7 if crc & 0x80000000 else crc << 1) & 0xffffffff
    return crc


def sniff(data):
    return any(all(prefix + k * stride < len(data) and data[prefix + k * stride] == 0x47 for k in range(3)) for stride, prefix in ((188, 0), (192, 4)))


def detect_layout(data):
    for stride, prefix in ((188, 0), (192, 4), (204, 0)):
        if len(data) >= stride * 5 and all(data[prefix + k * stride] == 0x47 for k in range(5)):
            return stride, prefix
    return None


def descriptors(data):
    out = []
    while len(data) >= 2:
        if len(data) < 2 + data[1]:
            break
        out.append((data[0], data[2:2 + data[1]]))
        data = data[2 + data[1]:]
    return out


def registration(data, name):
    return any(tag == 5 and body[:4] == name for tag, body in descriptors(data))


def stream_codec(stream_type, program, es):
    table = {0x0f: ("aac", "adts"), 0x11: ("aac", "latm"), 0x03: ("mpeg-audio", "raw"), 0x04: ("mpeg-audio", "raw"), 0x81: ("ac3", "raw"),
             0x87: ("ac3", "raw"), 0x80: ("pcm", "raw"), 0x82: ("dts", "raw")}
    if stream_type in table:
        return table[stream_type]
    if stream_type == 0x06:
        if any(tag == 0x6A for tag, _ in descriptors(es)) or registration(es, b"AC-3"):
            return "ac3", "raw"
        if registration(program, b"HDMV"):
            return "aac", "adts"
    return None


def mpeg_audio_header(d):
    """-> (frame length, rate, channels, samples per frame, layer) or None"""
    if len(d) < 4 or d[0] != 0xff or d[1] & 0xe0 != 0xe0:
        return None
    version, layer_bits = (d[1] >> 3) & 3, (d[1] >> 1) & 3
    if version == 1 or layer_bits == 0:
        return None
    layer, bitrate_index, rate_index = 4 - layer_bits, d[2] >> 4, (d[2] >> 2) & 3
    if bitrate_index in (0, 15) or rate_index == 3:
        return None
    mpeg1 = version == 3
    bitrate = KBPS[(mpeg1, layer)][bitrate_index - 1] * 1000
    rate = (44100, 48000, 32000)[rate_index] // {3: 1, 2: 2, 0: 4}[version]
    padding = (d[2] >> 1) & 1
    if layer == 1:
        length, samples = (12 * bitrate // rate + padding) * 4, 384
    elif layer == 2 or mpeg1:
        length, samples = 144 * bitrate // rate + padding, 1152
    else:
        length, samples = 72 * bitrate // rate + padding, 576
    return length, rate, 1 if d[3] >> 6 == 3 else 2, samples, layer


def adts_header(d):
    """-> (frame length, rate, channel configuration, samples per frame) or None"""
    if len(d) < 7 or d[0] != 0xff or d[1] & 0xf0 != 0xf0 or d[1] & 0x06:
        return None
    index = (d[2] >> 2) & 15
    length = (d[3] & 3) << 11 | d[4] << 3 | d[5] >> 5
    if index >= len(ADTS_RATES) or length < 7:
        return None
    return length, ADTS_RATES[index], (d[2] & 1) << 2 | d[3] >> 6, 1024 * ((d[6] & 3) + 1)


def timestamp(d):
    if len(d) < 5 or not (d[0] & 1 and d[2] & 1 and d[4] & 1):
        raise Refused("invalid or truncated MPEG-TS PES timestamp")
    return ((d[0] >> 1) & 7) << 30 | d[1] << 22 | (d[2] >> 1) << 15 | d[3] << 7 | d[4] >> 1


class Assembler:
    def __init__(self):
        self.bytes, self.expected = bytearray(), None

    def reset(self):
        self.bytes, self.expected = bytearray(), None

    def append(self, data, done):
        while data:
            if not self.bytes and data[0] == 0xff:
                return
            if self.expected is None:
                take = min(3 - len(self.bytes), len(data))
                self.bytes += data[:take]
                data = data[take:]
                if len(self.bytes) < 3:
                    return
                expected = 3 + ((self.bytes[1] & 15) << 8 | self.bytes[2])
                if not 4 <= expected <= 1024:
                    self.reset()
                    raise Refused("PSI section size %d is out of range" % expected)
                self.expected = expected
            take = min(self.expected - len(self.bytes), len(data))
            self.bytes += data[:take]
            data = data[take:]
            if len(self.bytes) == self.expected:
                done.append(bytes(self.bytes))
                self.reset()

    def push(self, data, unit_start):
        done = []
        if unit_start:
            if not data:
                raise Refused("truncated PSI pointer field")
            pointer, data = data[0], data[1:]
            if pointer > len(data):
                raise Refused("PSI pointer exceeds payload")
            if self.bytes:
                self.append(data[:pointer], done)
                if self.bytes:
                    raise Refused("PSI pointer starts a new section before the previous section ends")
            data = data[pointer:]
        self.append(data, done)
        return done


class Model:
    def __init__(self):
        self.events, self.layout = [], None
        self.pmt_pid = self.audio_pid = self.program = self.pat_version = self.pmt_version = None
        self.codec = self.format = self.stream_type = None
        self.pes, self.pes_cc, self.pes_disc = bytearray(), 0, False
        self.cc, self.psi = {}, {}
        self.epoch, self.last_pts = 0, None
        self.configured, self.rate, self.channels = False, None, None

    # ---- packets -----------------------------------------------------------------------------------------------------------------------
    def run(self, data):
        if len(data) > MAX_CHUNK:
            raise Refused("MPEG-TS input chunk exceeds the %d byte streaming budget" % MAX_CHUNK)
        at = 0
        while True:
            rest = len(data) - at
            if self.layout is None:
                self.layout = detect_layout(data[at:at + 1020])
                if self.layout is None:
                    if rest >= 1020:
                        at += 1
                        continue
                    break
            stride, prefix = self.layout
            if rest < stride:
                break
            if data[at + prefix] != 0x47:
                self.layout = None
                at += 1
                continue
            packet = data[at + prefix:at + prefix + 188]
            at += stride
            self.packet(packet)
        self.flush()

    def packet(self, p):
        if p[1] & 0x80:
            raise Refused("MPEG-TS packet has the transport-error indicator")
        if p[3] & 0xC0:
            raise Refused("scrambled MPEG-TS packets are unsupported")
        start, pid, afc, cc = bool(p[1] & 0x40), (p[1] & 0x1f) << 8 | p[2], (p[3] >> 4) & 3, p[3] & 15
        if afc == 0:
            raise Refused("MPEG-TS packet has reserved adaptation-field control")
        if afc == 2:
            return
        at, disc = 4, False
        if afc == 3:
            at = 5 + p[4]
            if at > 188:
                raise Refused("MPEG-TS adaptation field exceeds its packet")
            disc = p[4] > 0 and bool(p[5] & 0x80)
        if at >= 188:
            return
        previous, self.cc[pid] = self.cc.get(pid), cc
        if previous is not None:
            if cc == previous:
                return
            if cc != (previous + 1) & 15 and not disc:
                disc = True
                if pid == self.audio_pid:
                    self.pes = bytearray()
        if disc and pid in self.psi:
            self.psi[pid].reset()
        payload = p[at:]
        if pid == 0 or pid == self.pmt_pid:
            for section in self.psi.setdefault(pid, Assembler()).push(payload, start):
                (self.pat if pid == 0 else self.pmt)(section)
        elif pid == self.audio_pid:
            if start:
                self.flush()
                self.pes, self.pes_disc, self.pes_cc = bytearray(), disc, cc
            self.pes_disc = self.pes_disc or disc
            if len(self.pes) + len(payload) > MAX_PES:
                raise Refused("MPEG-TS PES exceeds the %d byte packet budget" % MAX_PES)
            self.pes += payload

    # ---- PSI ---------------------------------------------------------------------------------------------------------------------------
    def section_ok(self, s, table_id, shortest):
        if len(s) < shortest or s[0] != table_id:
            return False
        if crc32_mpeg2(s):
            raise Refused("MPEG-TS PSI CRC mismatch")
        return bool(s[5] & 1)

    def pat(self, s):
        if not self.section_ok(s, 0, 12):
            return
        version = (s[5] >> 1) & 31
        if version == self.pat_version:
            return
        programs = [(s[at] << 8 | s[at + 1], (s[at + 2] & 0x1f) << 8 | s[at + 3]) for at in range(8, len(s) - 7, 4)]
        programs = [p for p in programs if p[0]]
        if not programs:
            return
        number, pid = min(programs, key=lambda p: p[0])
        if pid != self.pmt_pid:
            self.audio_pid = self.codec = self.format = self.stream_type = self.pmt_version = None
        self.program, self.pmt_pid, self.pat_version = number, pid, version

    def pmt(self, s):
        if not self.section_ok(s, 2, 16):
            return
        version = (s[5] >> 1) & 31
        if version == self.pmt_version or (self.program is not None and self.program != (s[3] << 8 | s[4])):
            return
        end, at = len(s) - 4, 12 + ((s[10] & 15) << 8 | s[11])
        if at > end:
            raise Refused("MPEG-TS PMT program descriptors exceed their section")
        program = s[12:at]
        while at + 5 <= end:
            stream_type, pid, nxt = s[at], (s[at + 1] & 0x1f) << 8 | s[at + 2], at + 5 + ((s[at + 3] & 15) << 8 | s[at + 4])
            if nxt > end:
                raise Refused("MPEG-TS PMT descriptor exceeds its section")
            known = stream_codec(stream_type, program, s[at + 5:nxt])
            if known:
                if self.audio_pid is None:
                    self.audio_pid, self.stream_type, (self.codec, self.format) = pid, stream_type, known
                self.pmt_version = version
                return
            at = nxt

    # ---- PES ---------------------------------------------------------------------------------------------------------------------------
    def config(self, rate=None, channels=None, **lpcm):
        if self.configured:
            return
        self.configured = True
        self.rate, self.channels = rate if rate is not None else self.rate, channels if channels is not None else self.channels
        self.events.append(("config", dict(dict(codec=self.codec, format=self.format, stream_type=self.stream_type, pid=self.audio_pid, program=self.program,
                                                 stride=self.layout[0], prefix=self.layout[1], rate=self.rate, channels=self.channels, bits=None,
                                                 bytes_per_frame=None, frames_per_packet=None, header=None), **lpcm)))

    def emit(self, data, pts, dts, duration, disc):
        self.events.append(("packet", dict(data=bytes(data), pts=pts, dts=dts, duration=duration, cc=self.pes_cc, discontinuity=disc)))

    def flush(self):
        if not self.pes:
            return
        pes, self.pes = bytes(self.pes), bytearray()
        if len(pes) < 9 or pes[:3] != b"\x00\x00\x01":
            raise Refused("invalid MPEG-TS PES header")
        start = 9 + pes[8]
        if start > len(pes):
            raise Refused("MPEG-TS PES optional header is truncated")
        flags = pes[7] >> 6
        pts = timestamp(pes[9:14]) if flags & 2 else None
        dts = timestamp(pes[14:19]) if flags == 3 else pts
        declared = pes[4] << 8 | pes[5]
        end = min(6 + declared, len(pes)) if declared else len(pes)
        if end < start:
            raise Refused("MPEG-TS PES length ends inside its header")
        if pts is not None:
            if self.last_pts is not None and self.last_pts - pts > 1 << 32:
                self.epoch += 1 << 33
            self.last_pts = pts
            pts += self.epoch
        if dts is not None:
            dts = dts + self.epoch if flags == 3 else pts
        if self.codec is None:
            return
        payload = pes[start:end]
        plus = lambda t, by: None if t is None else t + by  # noqa: E731
        if self.stream_type == 0x80:
            self.lpcm(payload, pts, dts)
        elif self.format == "adts":
            at = index = 0
            while at + 7 <= len(payload):
                if payload[at] != 0xff or payload[at + 1] & 0xf0 != 0xf0:
                    at += 1
                    continue
                h = adts_header(payload[at:])
                if h is None or at + h[0] > len(payload):
                    break
                self.config(h[1], h[2])
                duration = 90000 * h[3] // h[1]
                self.emit(payload[at:at + h[0]], plus(pts, duration * index), plus(dts, duration * index), duration, self.pes_disc and index == 0)
                index, at = index + 1, at + h[0]
        elif self.format == "latm":
            at, first = 0, True
            while at + 3 <= len(payload):
                if payload[at] != 0x56 or payload[at + 1] & 0xe0 != 0xe0:
                    at += 1
                    continue
                length = 3 + ((payload[at + 1] & 0x1f) << 8 | payload[at + 2])
                if at + length > len(payload):
                    raise Refused("LOAS/LATM access unit is truncated at the PES boundary")
                self.config()
                self.emit(payload[at:at + length], pts, dts, None, self.pes_disc and first)
                at, first = at + length, False
            if payload[at:].strip(b"\xff"):
                raise Refused("LOAS/LATM PES ends with an incomplete access unit")
        elif self.stream_type in (3, 4):
            at = offset = 0
            while at + 4 <= len(payload):
                h = mpeg_audio_header(payload[at:at + 4])
                if h is None:
                    at += 1
                    continue
                if at + h[0] > len(payload):
                    raise Refused("MPEG audio frame is truncated at the PES boundary")
                if not self.configured:
                    self.codec = "mp%d" % h[4]
                self.config(h[1], h[2])
                duration = h[3] * 90000 // h[1]
                self.emit(payload[at:at + h[0]], plus(pts, offset), plus(dts, offset), duration, self.pes_disc and offset == 0)
                offset, at = offset + duration, at + h[0]
            if payload[at:].strip(b"\xff"):
                raise Refused("MPEG audio PES ends with an incomplete frame")
        else:  # AC-3; DTS whole
            self.config()
            if payload:
                self.emit(payload, pts, dts, None, self.pes_disc)

    def lpcm(self, d, pts, dts):
        if len(d) < 4:
            raise Refused("Blu-ray LPCM access unit of %d bytes is shorter than its 4-byte header" % len(d))
        size = d[0] << 8 | d[1]
        if size != len(d) - 4:
            raise Refused("Blu-ray LPCM size field %d disagrees with the %d payload bytes" % (size, len(d) - 4))
        assignment, rate_code, depth_code = d[2] >> 4, d[2] & 15, d[3] >> 6
        rate = {1: 48000, 4: 96000, 5: 192000}.get(rate_code)
        if rate is None:
            raise Refused("unsupported Blu-ray LPCM rate code %d" % rate_code)
        if depth_code == 0:
            raise Refused("unsupported Blu-ray LPCM depth code 0")
        if assignment == 1:
            raise Refused("mono Blu-ray LPCM (channel assignment 1, with its pad channel) is not built")
        if assignment != 3:
            raise Refused("Blu-ray LPCM channel assignment %d is not built: stereo alone is" % assignment)
        if depth_code == 2:
            raise Refused("20-bit Blu-ray LPCM is not built")
        bits = 16 if depth_code == 1 else 24
        frame = bits // 8 * 2
        if size % frame:
            raise Refused("Blu-ray LPCM payload of %d bytes is no whole number of %d-byte frames" % (size, frame))
        self.codec, self.rate, self.channels = "pcm", rate, 2
        self.config(rate, 2, bits=bits, bytes_per_frame=frame, frames_per_packet=size // frame, header=bytes(d[:4]))
        self.emit(d[4:], pts, dts, size // frame * 90000 // rate, self.pes_disc)


def demux(data):
    m = Model()
    try:
        m.run(bytes(data))
    except Refused as e:
        return m.events, str(e)
    return m.events, None

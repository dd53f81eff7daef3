"""A small MPEG transport stream writer for the tests: PSI sections with CRC-32/MPEG-2 (split over packets on demand), a PES packetiser
with adaptation-field stuffing, PCR-only and null packets, and a Mux that keeps the continuity counters and lays the packets out at
stride 188, 192 (a 4-byte arrival time in front) or 204 (16 parity bytes behind)."""
from ts_model import crc32_mpeg2

NULL_PID = 0x1fff


def section(table_id, ext, body, version=0, current=1, crc=None):
    """a long-form section: table id, length, table id extension, version / current_next, section numbers 0 / 0, body, CRC"""
    length = 5 + len(body) + 4
    head = bytes([table_id, 0xb0 | length >> 8, length & 0xff, ext >> 8, ext & 0xff, 0xc0 | version << 1 | current, 0, 0]) + body
    return head + (crc32_mpeg2(head) if crc is None else crc).to_bytes(4, "big")


def pat(programs, version=0, **more):
    """programs: [(program number, PID)] (number 0: the network PID)"""
    return section(0, 1, b"".join(bytes([n >> 8, n & 0xff, 0xe0 | pid >> 8, pid & 0xff]) for n, pid in programs), version, **more)


def descriptor(tag, body):
    return bytes([tag, len(body)]) + body


def registration(name):
    return descriptor(5, name)


def pmt(program, streams, program_descriptors=b"", version=0, pcr_pid=NULL_PID, **more):
    """streams: [(stream type, PID, ES descriptors)]"""
    body = bytes([0xe0 | pcr_pid >> 8, pcr_pid & 0xff, 0xf0 | len(program_descriptors) >> 8, len(program_descriptors) & 0xff]) + program_descriptors
    for stream_type, pid, es in streams:
        body += bytes([stream_type, 0xe0 | pid >> 8, pid & 0xff, 0xf0 | len(es) >> 8, len(es) & 0xff]) + es
    return section(2, program, body, version, **more)


def stamp(marker, t):
    t &= (1 << 33) - 1
    return bytes([marker << 4 | (t >> 30) << 1 | 1, (t >> 22) & 0xff, ((t >> 15) & 0x7f) << 1 | 1, (t >> 7) & 0xff, (t & 0x7f) << 1 | 1])


def pes(payload, pts=None, dts=None, stream_id=0xc0, unbounded=False):
    head = b""
    if pts is not None and dts is not None:
        head = stamp(3, pts) + stamp(1, dts)
    elif pts is not None:
        head = stamp(2, pts)
    flags = 0xc0 if dts is not None else (0x80 if pts is not None else 0)
    length = 3 + len(head) + len(payload)
    if unbounded or length > 0xffff:
        length = 0
    return b"\x00\x00\x01" + bytes([stream_id, length >> 8, length & 0xff, 0x80, flags, len(head)]) + head + payload


def packet(pid, cc, payload=b"", start=False, adaptation=None, error=False, scrambling=0, afc=None):
    """one 188-byte packet.  adaptation: the adaptation field's bytes behind its length byte (flags, then whatever), None for none; a
    payload shorter than the room left is made to fit with adaptation-field stuffing"""
    room = 184 - (0 if adaptation is None else 1 + len(adaptation))
    if len(payload) < room and payload:
        pad = room - len(payload)
        if adaptation is None:
            adaptation = b"" if pad == 1 else b"\x00" + b"\xff" * (pad - 2)
        else:
            adaptation = adaptation + b"\xff" * pad
    elif not payload and adaptation is not None:
        adaptation = adaptation + b"\xff" * (183 - len(adaptation))
    field = b"" if adaptation is None else bytes([len(adaptation)]) + adaptation
    if afc is None:
        afc = (2 if adaptation is not None else 0) | (1 if payload else 0)
    out = bytes([0x47, (0x80 if error else 0) | (0x40 if start else 0) | pid >> 8, pid & 0xff, scrambling << 6 | afc << 4 | cc & 15]) + field + payload
    assert len(out) == 188, len(out)
    return out


class Mux:
    def __init__(self, stride=188):
        self.stride, self.packets, self.cc, self.clock = stride, [], {}, 0

    def next_cc(self, pid):
        self.cc[pid] = (self.cc.get(pid, -1) + 1) & 15
        return self.cc[pid]

    def raw(self, p):
        self.packets.append(p)
        return self

    def psi(self, pid, sections, first=183, pointer_fill=0):
        """sections (one, or a list that shares packets) behind a pointer field; `first`: section bytes in the first packet at most, the
        rest follows in packets of 184; the last packet is filled with FF.  pointer_fill: so many FF bytes behind the pointer field"""
        data = sections if isinstance(sections, bytes) else b"".join(sections)
        head, data = bytes([pointer_fill]) + b"\xff" * pointer_fill + data[:first - pointer_fill], data[first - pointer_fill:]
        pieces = [head] + [data[at:at + 184] for at in range(0, len(data), 184)]
        pieces[-1] += b"\xff" * (184 - len(pieces[-1]))
        for k, piece in enumerate(pieces):  # (a short first piece is made to fit with adaptation-field stuffing)
            self.raw(packet(pid, self.next_cc(pid), piece, start=k == 0))
        return self

    def pes(self, pid, data, discontinuity=False, pcr=False):
        """a PES packet over as many transport packets as it needs; the last one is stuffed"""
        start = True
        while data:
            adaptation = None
            if start and (discontinuity or pcr):
                adaptation = bytes([(0x80 if discontinuity else 0) | (0x10 if pcr else 0)]) + (bytes(6) if pcr else b"")
            room = 184 - (0 if adaptation is None else 1 + len(adaptation))
            piece, data = data[:room], data[room:]
            self.raw(packet(pid, self.next_cc(pid), piece, start=start, adaptation=adaptation))
            start = False
        return self

    def null(self):
        return self.raw(packet(NULL_PID, 0, b"\xff" * 184))

    def pcr_only(self, pid):
        """adaptation field alone: the continuity counter does not advance"""
        return self.raw(packet(pid, self.cc.get(pid, 0), adaptation=b"\x10" + bytes(6)))

    def bytes(self):
        out = bytearray()
        for p in self.packets:
            if self.stride == 192:
                self.clock += 1504
                out += (self.clock & 0x3fffffff).to_bytes(4, "big")
            out += p
            if self.stride == 204:
                out += bytes(16)
        return bytes(out)


def audio_stream(stream_type, pes_payloads, stride=188, audio_pid=0x100, pmt_pid=0x1000, program=1, es_descriptors=b"", program_descriptors=b"",
                 pts0=90000, pts_step=1920, video=True, repeat_psi=3):
    """PAT, PMT, then one PES per payload on the audio PID, with a video PID and null packets between them; the PSI is repeated every
    `repeat_psi` PES packets"""
    m = Mux(stride)
    streams = ([(0x1b, 0x101, b"")] if video else []) + [(stream_type, audio_pid, es_descriptors)]
    for k, payload in enumerate(pes_payloads):
        if k % repeat_psi == 0:
            m.psi(0, pat([(0, 0x10), (program, pmt_pid)])).psi(pmt_pid, pmt(program, streams, program_descriptors, pcr_pid=audio_pid))
        if video:
            m.pes(0x101, pes(b"\x00\x00\x00\x01\x09\xf0" + bytes([k]) * 300 + b"\xff\xfb\x90\x00", pts0 + k * pts_step, pts0 + k * pts_step - 3000, 0xe0))
        m.pes(audio_pid, pes(payload, pts0 + k * pts_step), pcr=k % 2 == 0)
        if k % 2:
            m.null()
    return m.bytes()

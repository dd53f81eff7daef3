"""What the MPEG-TS tests share: the four fixtures, the elementary streams they and the built streams are made of, and the streams
tests/ts_builder.py writes for the demuxer cases.  Host only."""
import os

import numpy as np

import ts_builder as B
import ts_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"aac.ts": "aac-stereo-48k.ts", "aac.m2ts": "aac-stereo-48k.m2ts", "mp2.ts": "mp2-stereo-48k.ts", "lpcm.m2ts": "lpcm-stereo-48k.m2ts"}
PACKETS = {"aac.ts": 48, "aac.m2ts": 48, "mp2.ts": 42, "lpcm.m2ts": 20}
LPCM_SHA256 = "7126a0d8077e0433c1e78df6c0f1074f78daf3800240ef48c936114ef7cbb563"  # the payloads as s16le: FFmpeg's decode
HDMV = B.registration(b"HDMV")


def golden(*path):
    with open(os.path.join(GOLDEN, *path), "rb") as f:
        return f.read()


def fixture(name):
    return golden("ts", FIXTURES[name])


ADTS = golden("aac", "aac-stereo-48k.adts")
MP2 = golden("mp2", "stereo48k_A_Tusk_1s.mp2")


def adts_frames(data):
    out, at = [], 0
    while at + 7 <= len(data):
        length = M.adts_header(data[at:])[0]
        out.append(data[at:at + length])
        at += length
    assert at == len(data)
    return out


def mpa_frames(data, limit=None):
    """the frames of an MPEG audio file, from its first header on, one header after the other"""
    at = next(k for k in range(len(data)) if M.mpeg_audio_header(data[k:k + 4]))
    out = []
    while at + 4 <= len(data) and (limit is None or len(out) < limit):
        h = M.mpeg_audio_header(data[at:at + 4])
        if h is None or at + h[0] > len(data):
            break
        out.append(data[at:at + h[0]])
        at += h[0]
    return out


def layer3_frames():
    return mpa_frames(golden("mp3", "stereo16k_A_Tusk_encoded.mp3"), 40)


def layer1_frames(n=24):
    """Layer I, MPEG-1, 48 kHz, 256 kbit/s stereo: frames of 256 bytes with scale factors that keep the PCM inside s16"""
    import mp12_builder
    rng = np.random.default_rng(1101)
    return [mp12_builder.random_frame(rng, 1, 0, 1, 8, 0, scf_floor=9)[0] for _ in range(n)]


def groups(frames, k):
    return [b"".join(frames[at:at + k]) for at in range(0, len(frames), k)]


def lpcm_unit(frames, bits=16, assignment=3, rate_code=1, seed=0, size=None):
    depth = {16: 1, 20: 2, 24: 3}[bits]
    width = (3 if bits > 16 else 2) * 2
    body = bytes((seed + 3 * k) & 0xff for k in range(frames * width))
    n = len(body) if size is None else size
    return bytes([n >> 8, n & 0xff, assignment << 4 | rate_code, depth << 6]) + body


def loas(n, seed=0):
    return bytes([0x56, 0xe0 | n >> 8, n & 0xff]) + bytes((seed + k) & 0xff for k in range(n))


def with_packets(make, stream_type=0x0f, nulls=6, **pmt):
    """PAT, PMT (one audio stream of `stream_type` on PID 0x100), whatever `make(mux)` adds, null packets, so that a layout is found"""
    m = B.Mux()
    m.psi(0, B.pat([(1, 0x1000)])).psi(0x1000, B.pmt(1, [(stream_type, 0x100, b"")], **pmt))
    make(m)
    for _ in range(nulls):
        m.null()
    return m.bytes()


def two_programs():
    frames = adts_frames(ADTS)
    m = B.Mux()
    m.psi(0, B.pat([(0, 0x10), (5, 0x1000), (2, 0x1001)]))
    m.psi(0x1000, B.pmt(5, [(0x0f, 0x100, b"")])).psi(0x1001, B.pmt(2, [(0x1b, 0x200, b""), (0x0f, 0x201, b"")]))
    for k, payload in enumerate(groups(frames[:12], 3)):
        m.pes(0x100, B.pes(MP2[:576], 1000 + k)).pes(0x201, B.pes(payload, 90000 + 5760 * k)).pes(0x200, B.pes(bytes(400), 7, 3, 0xe0))
    return m.bytes()


def version_change():
    """PAT version 0 names the PMT on 0x1000 (audio on 0x100); PAT version 1 moves the program to the PMT on 0x1001 (audio on 0x102)"""
    frames = adts_frames(ADTS)
    m = B.Mux()
    m.psi(0, B.pat([(1, 0x1000)])).psi(0x1000, B.pmt(1, [(0x0f, 0x100, b"")]))
    for k, payload in enumerate(groups(frames[:8], 4)):
        m.pes(0x100, B.pes(payload, 90000 + 7680 * k))
    m.psi(0, B.pat([(1, 0x1000)])).psi(0x1000, B.pmt(1, [(0x0f, 0x100, b"")]))  # the same versions again: nothing moves
    m.psi(0x1000, B.pmt(1, [(0x0f, 0x103, b"")], version=1))  # a PMT version change alone keeps the audio PID
    m.pes(0x100, B.pes(frames[8], 200000))
    m.psi(0, B.pat([(1, 0x1001)], version=1)).psi(0x1001, B.pmt(1, [(0x0f, 0x102, b"")], version=1))
    for k, payload in enumerate(groups(frames[9:17], 4)):
        m.pes(0x102, B.pes(payload, 300000 + 7680 * k)).pes(0x100, B.pes(frames[20], 5))
    return m.bytes()


def duplicate_and_gap():
    """the second PES has one of its packets twice; the third loses its last packet, and goes as a whole; the fourth carries the gap"""
    frames = adts_frames(ADTS)
    m, marks = B.Mux(), []
    m.psi(0, B.pat([(1, 0x1000)])).psi(0x1000, B.pmt(1, [(0x0f, 0x100, b"")]))
    for k, payload in enumerate(groups(frames[:15], 3)):
        marks.append(len(m.packets))
        m.pes(0x100, B.pes(payload, 90000 + 5760 * k))
    marks.append(len(m.packets))
    packets = list(m.packets)
    del packets[marks[3] - 1]                          # the third PES's last packet
    packets.insert(marks[1] + 2, packets[marks[1] + 1])  # the second PES's second packet once more
    m.packets = packets
    return m.bytes()


def builder_cases():
    """name -> stream, for the comparison with the model: every one demuxes to the end and hands out packets"""
    adts, mp2 = adts_frames(ADTS), mpa_frames(MP2)
    cases = {}
    for stride in (188, 192, 204):
        cases["adts_%d" % stride] = B.audio_stream(0x0f, groups(adts[:18], 4), stride)
    cases["mp2_192"] = B.audio_stream(0x03, groups(mp2[:10], 3), 192, audio_pid=0x1100, pmt_pid=0x100)
    cases["layer3"] = B.audio_stream(0x03, groups(layer3_frames(), 5), pts_step=16200)
    cases["layer1"] = B.audio_stream(0x04, groups(layer1_frames(), 5), pts_step=3600)
    cases["lpcm_16"] = B.audio_stream(0x80, [lpcm_unit(240, seed=k) for k in range(6)], 192, program_descriptors=HDMV, pts_step=450)
    cases["lpcm_24_96k"] = B.audio_stream(0x80, [lpcm_unit(160, 24, rate_code=4, seed=k) for k in range(5)], program_descriptors=HDMV)
    cases["hdmv_private_aac"] = B.audio_stream(0x06, groups(adts[:8], 2), 192, program_descriptors=HDMV, video=False)
    cases["ac3_by_descriptor"] = B.audio_stream(0x06, [bytes([0x0b, 0x77]) + bytes(60)] * 3, es_descriptors=B.descriptor(0x6A, b"\x00"))
    cases["ac3_by_registration"] = B.audio_stream(0x06, [bytes([0x0b, 0x77]) + bytes(60)] * 3, es_descriptors=B.registration(b"AC-3"))
    cases["ac3"] = B.audio_stream(0x81, [bytes([0x0b, 0x77]) + bytes(200)] * 4)
    cases["dts"] = B.audio_stream(0x82, [bytes([0x7f, 0xfe, 0x80, 0x01]) + bytes(300)] * 4, 192, program_descriptors=HDMV)
    cases["latm"] = B.audio_stream(0x11, [loas(100, 1) + loas(7, 2), loas(300, 3) + b"\xff\xff"])
    cases["two_programs"] = two_programs()
    cases["version_change"] = version_change()
    cases["duplicate_and_gap"] = duplicate_and_gap()
    garbage = bytes((37 * k + 11) % 251 for k in range(1500)).replace(b"\x47", b"\x46")
    cases["leading_garbage"] = garbage + cases["adts_188"]
    cases["garbage_in_the_middle"] = cases["adts_204"][:204 * 20] + garbage[:333] + cases["adts_204"][204 * 20:]
    cases["pts_wrap"] = B.audio_stream(0x0f, groups(adts[:12], 2), pts0=(1 << 33) - 3 * 3840, pts_step=3840)
    big = B.pmt(1, [(0x1b, 0x101, B.descriptor(0x28, bytes(4)) * 30), (0x0f, 0x100, B.descriptor(0x0a, b"eng\x00"))], B.descriptor(0x0e, bytes(3)) * 20)
    assert len(big) > 184
    m = B.Mux()
    m.psi(0, B.pat([(1, 0x1000)]), first=2).psi(0x1000, big, first=100).psi(0, [B.pat([(1, 0x1000)]), B.pat([(1, 0x1000)])], pointer_fill=9)
    for k, payload in enumerate(groups(adts[:6], 2)):
        m.pes(0x100, B.pes(payload, 90000 + 3840 * k, 90000 + 3840 * k - 100), discontinuity=k == 1).pcr_only(0x100)
    cases["split_sections_dts_and_flags"] = m.bytes()
    m = B.Mux()
    m.psi(0, B.pat([(1, 0x1000)])).psi(0x1000, B.pmt(1, [(0x0f, 0x100, b"")]))
    m.pes(0x100, B.pes(b"".join(adts[:3]), unbounded=True)).pes(0x100, B.pes(b"junk" + adts[3] + adts[4][:50], 1234)).pes(0x100, B.pes(adts[5] + b"\xff\xf1\x00", 99))
    for _ in range(3):
        m.null()
    cases["no_timestamps_and_partial_tails"] = m.bytes()
    return cases

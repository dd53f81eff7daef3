"""Apple Lossless on the host (csrc/alac_stream.h): the cookie in its three wrappings, a packet's frame count and the CAF packet index,
against tests/alac_model.py -- which is itself pinned here by the reference's fixture and its decoded twin -- the builder's round trip
over every configuration the GPU tests use, every CAF rejection with its text, and a sanitizer fuzz (tests/fuzz_alac.cpp).  No GPU."""
import os
import struct
import subprocess

import pytest

import alac_builder as B
import alac_cases as CASES
import alac_model as M
from soundkit_amd import SoundkitError, alac

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "alac")
FIXTURE = os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts.caf")
TWIN = os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts.decoded.wav")
OK = 0


@pytest.fixture(scope="module")
def fixture_bytes():
    return open(FIXTURE, "rb").read()


def twin_pcm():
    w = open(TWIN, "rb").read()
    at = w.index(b"data")
    return w[at + 8:at + 8 + struct.unpack("<I", w[at + 4:at + 8])[0]]


# ---- the model and the builder are pinned first ---------------------------------------------------------------------------------------

def test_model_decodes_the_fixture_to_its_twin(fixture_bytes):
    twin = twin_pcm()
    assert len(fixture_bytes) == 18353 and len(twin) == 2 * 23680
    cfg, packets, valid, priming, remainder = M.caf_index(fixture_bytes)
    assert (cfg["sample_rate"], cfg["channels"], cfg["bit_depth"], cfg["frame_length"]) == (8000, 1, 16, 4096)
    assert (len(packets), valid, priming, remainder) == (6, 23680, 0, 896)
    assert [M.packet_frames(cfg, p) for p in packets] == [4096] * 5 + [3200]
    _, pcm = M.decode_caf(fixture_bytes)
    assert len(pcm) // 2 == 23680 and pcm == twin


def test_the_fixture_exercises_what_the_issue_lists(fixture_bytes):
    cfg, packets, *_ = M.caf_index(fixture_bytes)
    stats = {}
    for p in packets:
        M.decode_packet(cfg, p, stats)
    assert stats["runs"] == 431


@pytest.mark.parametrize("case", CASES.cases(), ids=lambda c: c[0])
def test_model_gives_back_what_the_builder_wrote(case):
    _, cfg, packets = case
    for packet, chans in packets:
        got, n = M.decode_packet(cfg, packet)
        assert n == len(chans[0]) == M.packet_frames(cfg, packet)
        assert got == chans


def test_the_cases_reach_the_branches_they_are_named_for():
    """k at the Rice limit, escapes, a pinned history, runs of 1 and of 0xFFFF and a run that ends at the last sample"""
    by_name = {c[0]: c for c in CASES.cases()}

    def stats_of(name, **kw):
        _, cfg, [(packet, chans)] = by_name[name]
        stats = {}
        assert B.packet(cfg, chans, stats=stats, **kw) == packet
        return cfg, stats
    cfg, s = stats_of("loud24_k_at_kb", order=0, shift=4)
    assert cfg["kb"] in s["k"] and not s.get("pinned")
    cfg, s = stats_of("loud24_kb5", order=0, shift=4)
    assert max(s["k"]) == 5
    _, s = stats_of("rand24_escapes", order=0, shift=4)
    assert s["pinned"] > 500
    _, s = stats_of("sparse", order=0, shift=4)
    assert 1 in s["runs"] and len(set(s["runs"])) > 10
    _, s = stats_of("run_ffff", order=0, shift=4)
    assert s["runs"] == [0xFFFF]
    _, s = stats_of("tail", order=0, shift=4)
    assert s["runs"][-1] > 500  # the last run ends exactly at the last sample: nothing is coded behind it
    _, s = stats_of("silence", order=0, shift=4)
    assert s["runs"] == [899]


def test_the_many_packets_round_trip():
    cfg, packets = CASES.many()
    assert len(packets) == 130 and len({len(ch[0]) for _, ch in packets}) >= 8
    for packet, chans in packets:
        assert M.decode_packet(cfg, packet)[0] == chans


def test_model_rejections():
    cfg = B.config(4096, 16, 1, 44100)
    ch = CASES.signal("tone", 100, 16)
    for tag in (2, 5):
        with pytest.raises(M.AlacError) as e:
            M.decode_packet(cfg, B.packet(cfg, ch, before=lambda w, tag=tag: w.put(tag, 3)))
        assert e.value.kind == M.ELEMENT
    for packet in (B.packet(cfg, ch, ptype=3), B.packet(cfg, ch, elements=[B.Element(n_override=4097, has_size=True)]),
                   B.packet(cfg, CASES.signal("silence", 100, 16), elements=[B.Element(order=0, n_override=50, has_size=True)]),
                   B.packet(cfg, ch)[:-9], B.packet(cfg, ch, end=False), B.packet(cfg, ch) + b"\0"):
        with pytest.raises(M.AlacError) as e:
            M.decode_packet(cfg, packet)
        assert e.value.kind == M.INVALID
    s32 = B.config(4096, 32, 2, 48000)
    with pytest.raises(M.AlacError) as e:
        M.decode_packet(s32, B.packet(s32, CASES.signal("tone", 50, 32, 0, 2)))
    assert e.value.kind == M.UNSUPPORTED


# ---- the library: cookie, frame count -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wrap", ["bare", "mp4", "qt"])
def test_cookie_in_all_three_wrappings(wrap):
    cfg = B.config(1234, 24, 6, 96000, pb=30, mb=12, kb=11, max_run=77)
    cfg.update(max_frame_bytes=4321, avg_bit_rate=987654, version=0)
    raw = B.cookie(cfg, wrap)
    assert len(raw) == {"bare": 24, "mp4": 28, "qt": 48}[wrap]
    got = alac.parse_cookie(raw)
    assert got == {"frame_length": 1234, "sample_rate": 96000, "max_frame_bytes": 4321, "avg_bit_rate": 987654, "max_run": 77,
                   "compatible_version": 0, "bit_depth": 24, "pb": 30, "mb": 12, "kb": 11, "channels": 6}
    model = M.parse_cookie(raw)
    assert all(model[k] == got[k] for k in ("frame_length", "sample_rate", "bit_depth", "pb", "mb", "kb", "channels", "max_run"))


def test_the_fixture_s_cookie(fixture_bytes):
    at, size = M.caf_chunks(fixture_bytes)["kuki"]
    got = alac.parse_cookie(fixture_bytes[at:at + size])
    assert size == 48 and (got["frame_length"], got["bit_depth"], got["pb"], got["mb"], got["kb"], got["channels"], got["sample_rate"]) == (
        4096, 16, 40, 10, 14, 1, 8000)


@pytest.mark.parametrize("change,text", [
    (dict(sample_rate=0), "ALAC stream reports a zero sample rate"),
    (dict(channels=0), "ALAC channel count 0 exceeds the supported range 1-8"),
    (dict(channels=9), "ALAC channel count 9 exceeds the supported range 1-8"),
    (dict(bit_depth=20), "Unsupported ALAC bit depth: 20"),
    (dict(bit_depth=8), "Unsupported ALAC bit depth: 8"),
    (dict(frame_length=0), "ALAC frame length 0 exceeds the 1-65536 frame budget"),
    (dict(frame_length=65537), "ALAC frame length 65537 exceeds the 1-65536 frame budget"),
])
def test_cookie_rejections(change, text):
    cfg = dict(B.config(4096, 16, 2, 44100), **change)
    for wrap in ("bare", "mp4", "qt"):
        with pytest.raises(SoundkitError) as e:
            alac.parse_cookie(B.cookie(cfg, wrap))
        assert e.value.status == alac.ERR_STREAM and text in str(e.value)
        with pytest.raises(M.AlacError) as m:
            M.parse_cookie(B.cookie(cfg, wrap))
        assert text == str(m.value)
    assert alac.parse_cookie(B.cookie(dict(cfg, frame_length=65536, channels=8, bit_depth=32, sample_rate=1)))["frame_length"] == 65536


def test_cookie_too_short():
    for n in (0, 1, 23):
        with pytest.raises(SoundkitError) as e:
            alac.parse_cookie(B.cookie(B.config())[:n])
        assert "ALAC magic cookie is shorter than 24 bytes" in str(e.value)
    with pytest.raises(SoundkitError):
        alac.parse_cookie(B.cookie(B.config(), "mp4")[:27])  # four zeros and 23 bytes: a frame length of 0 at best


def test_packet_frames_with_and_without_a_size(fixture_bytes):
    cfg, packets, *_ = M.caf_index(fixture_bytes)
    assert [alac.packet_frames(cfg, p) for p in packets] == [(OK, 4096)] * 5 + [(OK, 3200)]
    small = B.config(256, 16, 2, 8000)
    ch = CASES.signal("tone", 256, 16, 0, 2)
    whole, sized = B.packet(small, ch), B.packet(small, ch, elements=[B.Element("cpe", has_size=True)])
    assert len(sized) == len(whole) + 4
    assert alac.packet_frames(small, whole) == (OK, 256) == alac.packet_frames(small, sized)
    assert alac.packet_frames(small, B.packet(small, [c[:77] for c in ch])) == (OK, 77)
    # DSE and FIL in front are stepped over
    front = B.packet(small, [c[:31] for c in ch], before=lambda w: (B.write_dse(w, b"abc"), B.write_fil(w, 20), B.write_dse(w, bytes(300), align=False)))
    assert alac.packet_frames(small, front) == (OK, 31) and M.packet_frames(small, front) == 31
    # refused: a count of 0 or above the cookie's, no audio element, a header beyond the packet
    for bad in (B.packet(small, [c[:5] for c in ch], elements=[B.Element("cpe", n_override=0, has_size=True)]),
                B.packet(small, [c[:5] for c in ch], elements=[B.Element("cpe", n_override=257, has_size=True)]),
                bytes([0xE0]), b"", sized[:5]):
        assert alac.packet_frames(small, bad) == (alac.INVALID, 0)
        with pytest.raises(M.AlacError) as e:
            M.packet_frames(small, bad)
        assert e.value.kind == M.INVALID
    for bad in (bytes([0x40]), B.packet(small, ch, before=lambda w: w.put(5, 3)), B.packet(small, ch, before=lambda w: (B.write_fil(w, 1), w.put(2, 3)))):
        assert alac.packet_frames(small, bad) == (alac.UNSUPPORTED_ELEMENT, 0)
        with pytest.raises(M.AlacError) as e:
            M.packet_frames(small, bad)
        assert e.value.kind == M.ELEMENT
    for name, cfg, packets in CASES.cases():
        for packet, chans in packets:
            assert alac.packet_frames(cfg, packet) == (OK, len(chans[0])), name


# ---- the library: the CAF packet index ------------------------------------------------------------------------------------------------

def test_index_of_the_fixture(fixture_bytes):
    ix = alac.CafAlacPacketIndex.from_file(fixture_bytes)
    cfg, packets, valid, priming, remainder = M.caf_index(fixture_bytes)
    assert (ix.sample_rate, ix.channels, ix.bit_depth, ix.frames_per_packet) == (8000, 1, 16, 4096)
    assert (ix.valid_frames, ix.priming_frames, ix.remainder_frames) == (valid, priming, remainder) == (23680, 0, 896)
    assert ix.packet_bytes(fixture_bytes) == packets
    assert ix.packets[0][0] == M.caf_chunks(fixture_bytes)["data"][0] + 4
    # the last packet carries its own count of 3200: nothing is trimmed
    assert [ix.trim(i, n) for i, n in enumerate([4096] * 5 + [3200])] == [(0, 4096)] * 5 + [(0, 3200)]


def built_file(constant=False, wrap="qt", **kw):
    cfg = B.config(64, 16, 2, 44100)
    chans = [CASES.signal("rand", 64, 16, i, 2) for i in range(5)]
    packets = [B.packet(cfg, ch, raw=constant, order=2, shift=4) for ch in chans]
    return cfg, packets, B.caf(cfg, packets, wrap=wrap, constant=constant, **kw)


@pytest.mark.parametrize("wrap", ["bare", "mp4", "qt"])
@pytest.mark.parametrize("constant", [False, True])
def test_index_of_built_files_in_both_table_forms(constant, wrap):
    cfg, packets, data = built_file(constant, wrap, priming=10, remainder=7) if not constant else built_file(constant, wrap)
    ix = alac.CafAlacPacketIndex.from_file(data)
    assert ix.packet_bytes(data) == packets and M.caf_index(data)[1] == packets
    assert ix.config["frame_length"] == 64 and ix.frames_per_packet == 64
    if constant:
        assert len({len(p) for p in packets}) == 1
        assert (ix.valid_frames, ix.priming_frames, ix.remainder_frames) == (320, 0, 0)
    else:
        assert (ix.valid_frames, ix.priming_frames, ix.remainder_frames) == (303, 10, 7)
        assert [ix.trim(i, 64) for i in range(5)] == [(10, 54), (0, 64), (0, 64), (0, 64), (0, 57)]
        assert [M.trim(64 * i, 64, 10, 303) for i in range(5)] == [ix.trim(i, 64) for i in range(5)]
    assert ix.trim(5, 64) is None


def parts(constant=False):
    cfg, packets, _ = built_file(constant)
    sizes = [len(p) for p in packets]
    return dict(description=B.desc(cfg, bytes_per_packet=sizes[0] if constant else 0), magic_cookie=B.cookie(cfg, "qt"),
                packet_table=b"" if constant else B.pakt(sizes, 320), data_payload_offset=100, data_payload_size=4 + sum(sizes)), cfg, sizes


def rejected(text, **change):
    p, _, _ = parts(change.pop("constant", False))
    p.update(change)
    with pytest.raises(SoundkitError) as e:
        alac.CafAlacPacketIndex.new(**p)
    assert e.value.status == alac.ERR_STREAM and text in str(e.value), str(e.value)


def test_index_from_its_parts():
    p, cfg, sizes = parts()
    ix = alac.CafAlacPacketIndex.new(**p)
    assert [s for _, s in ix.packets] == sizes and ix.packets[0][0] == 104 and ix.valid_frames == 320
    p, cfg, sizes = parts(True)
    assert [s for _, s in alac.CafAlacPacketIndex.new(**p).packets] == sizes


def test_every_caf_rejection_has_its_text():
    p, cfg, sizes = parts()
    total = sum(sizes)
    rejected("CAF desc must contain 32 bytes, got 31", description=p["description"][:31])
    rejected("CAF desc must contain 32 bytes, got 33", description=p["description"] + b"\0")
    rejected("CAF audio description is not ALAC", description=B.desc(cfg, fmt=b"lpcm"))
    rejected("invalid CAF sample rate", description=B.desc(cfg, rate=0.0))
    rejected("invalid CAF sample rate", description=B.desc(cfg, rate=float("nan")))
    rejected("invalid CAF sample rate", description=B.desc(cfg, rate=-44100.0))
    rejected("invalid CAF sample rate", description=B.desc(cfg, rate=1e10))
    rejected("CAF ALAC channel count exceeds the supported range", description=B.desc(cfg, channels=0))
    rejected("CAF ALAC channel count exceeds the supported range", description=B.desc(cfg, channels=9))
    rejected("CAF data chunk is shorter than its edit count", data_payload_size=3)
    rejected("CAF packet offset overflow", data_payload_offset=2 ** 64 - 2)
    rejected("ALAC magic cookie is shorter than 24 bytes", magic_cookie=b"")
    rejected("Unsupported ALAC bit depth: 20", magic_cookie=B.cookie(dict(cfg, bit_depth=20)))
    rejected("CAF desc and ALAC magic cookie disagree", description=B.desc(cfg, rate=48000))
    rejected("CAF desc and ALAC magic cookie disagree", description=B.desc(cfg, channels=1))
    rejected("CAF desc and ALAC magic cookie disagree", description=B.desc(cfg, bits=24))
    rejected("CAF ALAC frames-per-packet 0 exceeds the decoder budget", description=B.desc(cfg, frames_per_packet=0))
    rejected("CAF ALAC frames-per-packet 65537 exceeds the decoder budget", description=B.desc(cfg, frames_per_packet=65537))
    rejected("CAF packet table is shorter than 24 bytes", packet_table=p["packet_table"][:23])
    for field in range(4):
        values = [len(sizes), 320, 0, 0]
        values[field] = -1
        rejected("CAF packet table contains a negative count", packet_table=struct.pack(">qqii", *values) + p["packet_table"][24:])
    rejected("CAF packet count exceeds its variable-length table", packet_table=struct.pack(">qqii", 1000, 320, 0, 0) + p["packet_table"][24:])
    rejected("CAF packet size VLQ is truncated", packet_table=B.pakt(sizes, 320)[:24] + b"\x81" * 5)
    rejected("CAF packet size VLQ exceeds 10 bytes", packet_table=struct.pack(">qqii", 1, 320, 0, 0) + b"\x80" * 10 + b"\x01")
    rejected("CAF packet size exceeds the u32 range", packet_table=struct.pack(">qqii", 1, 320, 0, 0) + B.vlq(2 ** 32))
    rejected("CAF packet table has trailing bytes", packet_table=p["packet_table"] + b"\x05")
    rejected("CAF ALAC packet size 0 exceeds its budget", packet_table=B.pakt([0] + sizes, 320))
    rejected("CAF ALAC packet size 16777217 exceeds its budget", packet_table=B.pakt([16 * 1024 * 1024 + 1], 320), data_payload_size=16 * 1024 * 1024 + 5)
    rejected("CAF packet table describes %d bytes, data contains %d" % (total, total + 1), data_payload_size=total + 5)
    rejected("CAF packet table describes %d bytes, data contains %d" % (total, total - 1), data_payload_size=total + 3)
    rejected("CAF constant packet size does not divide the data chunk", constant=True, data_payload_size=total + 5)
    # the description may leave the depth open, and 16 MiB itself is within the budget
    q = dict(p, description=B.desc(cfg, bits=0))
    assert alac.CafAlacPacketIndex.new(**q).bit_depth == 16
    q = dict(p, packet_table=B.pakt([16 * 1024 * 1024], 64), data_payload_size=16 * 1024 * 1024 + 4)
    assert alac.CafAlacPacketIndex.new(**q).packets == [(104, 16 * 1024 * 1024)]


def test_file_walker_rejections(fixture_bytes):
    def refused(data, text):
        with pytest.raises(SoundkitError) as e:
            alac.CafAlacPacketIndex.from_file(data)
        assert text in str(e.value), str(e.value)
    refused(b"", "not a CAF file")
    refused(b"RIFF" + fixture_bytes[4:], "not a CAF file")
    refused(fixture_bytes[:4] + b"\0\2" + fixture_bytes[6:], "unsupported CAF version")
    refused(fixture_bytes[:15], "CAF chunk header is truncated")
    refused(fixture_bytes[:-1], "CAF chunk extends past the source")
    cfg, packets, data = built_file()
    chunks = M.caf_chunks(data)
    for kind in ("desc", "kuki", "data"):
        at, size = chunks[kind]
        refused(data[:at - 12] + data[at + size:], "CAF source has no %s chunk" % kind)
        refused(data + data[at - 12:at + size], "CAF source contains multiple %s chunks" % kind)
    at, size = chunks["pakt"]
    refused(data[:at - 12], "CAF packet table is shorter than 24 bytes")
    # a data chunk of size -1 runs to the end of the file
    at, size = chunks["data"]
    moved = data[:at - 12] + data[at + size:] + b"data" + struct.pack(">q", -1) + data[at:at + size]
    assert alac.CafAlacPacketIndex.from_file(moved).packet_bytes(moved) == packets
    # unknown chunks are stepped over
    extra = data[:8] + B.chunk(b"free", bytes(37)) + data[8:]
    assert alac.CafAlacPacketIndex.from_file(extra).packet_bytes(extra) == packets


def test_mutated_files_under_sanitizers(tmp_path):
    """tests/fuzz_alac.cpp: csrc/alac_stream.h alone with AddressSanitizer + UBSan on the CPU -- seeded mutations of the fixture through
    the cookie parser, the frame count, the index and the file walker"""
    exe = str(tmp_path / "fuzz_alac")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "fuzz_alac.cpp")], cwd=HERE)
    out = subprocess.run([exe, "4000", FIXTURE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "fuzz_alac ok" in out.stdout

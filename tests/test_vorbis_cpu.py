"""The host side of the Ogg Vorbis path (csrc/ogg_stream.h, csrc/vorbis_stream.h) against the reference's behaviour and texts, the numpy
model (tests/vorbis_model.py) against the reference's decoded recording, the builder against both parsers, and a sanitizer fuzz
(tests/fuzz_vorbis.cpp).  No GPU."""
import copy
import os
import subprocess
import wave

import numpy as np
import pytest

import vorbis_builder as B
import vorbis_model as M
import webm_vorbis
from soundkit_amd import SoundkitError, vorbis

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "vorbis")
OGG = os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts.ogg")
RECORDING = os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts.decoded.wav")
WEBM = os.path.join(GOLDEN, "yt_itag_171_vorbis.webm")


@pytest.fixture(scope="module")
def ogg_bytes():
    return open(OGG, "rb").read()


@pytest.fixture(scope="module")
def recording():
    w = wave.open(RECORDING)
    assert (w.getframerate(), w.getnchannels(), w.getsampwidth()) == (8000, 1, 2)
    return np.frombuffer(w.readframes(w.getnframes()), "<i2")


def parse_all(data, piece):
    p, out = vorbis.OggPacketParser(), []
    for at in range(0, len(data), piece):
        out += p.add(data[at:at + piece])
    return out + p.finish()


# ---- Ogg ---------------------------------------------------------------------------------------------------------------------------

def test_fixture_packets_whole_and_in_pieces(ogg_bytes):
    whole = parse_all(ogg_bytes, len(ogg_bytes))
    assert len(whole) == 97 and [len(p.data) for p in whole[:3]] == [30, 63, 2476] and max(len(p.data) for p in whole[3:]) == 106
    assert whole[0].first_in_stream and not whole[3].first_in_stream and whole[-1].last_in_stream and whole[-1].granule_position == 23680
    assert sum(p.last_in_page for p in whole) == 5
    for piece in (997, 641, 1):
        assert parse_all(ogg_bytes, piece) == whole
    want = M.ogg_packets(ogg_bytes)
    assert [(p.data, p.serial, p.first_in_stream, p.last_in_page, p.last_in_stream, p.granule_position) for p in whole] == [
        (q["data"], q["serial"], q["first_in_stream"], q["last_in_page"], q["last_in_stream"], q["granule_position"]) for q in want]


def test_page_crc(ogg_bytes):
    assert vorbis.ogg_page_crc(b"") == 0 and vorbis.ogg_page_crc(b"OggS") != 0
    assert vorbis.ogg_page_crc(ogg_bytes[:58]) == M.ogg_page_crc(ogg_bytes[:58]) == int.from_bytes(ogg_bytes[22:26], "little")


def refusal(feed):
    p = vorbis.OggPacketParser()
    with pytest.raises(SoundkitError) as e:
        for piece in feed:
            p.add(piece)
        p.finish()
    assert e.value.status == vorbis.ERR_STREAM
    return str(e.value)


def test_ogg_refusals_carry_the_reference_texts(ogg_bytes):
    first, last = M.ogg_page(2, 0, 7, 0, [1], b"\xaa"), M.ogg_page(4, 1, 7, 1, [1], b"\xbb")
    p = vorbis.OggPacketParser()
    assert len(p.add(first)) == 1
    got = p.add(last)
    assert len(got) == 1 and got[0].last_in_stream and p.finish() == []
    corrupt = bytearray(ogg_bytes)
    corrupt[2000] ^= 1
    assert "Ogg CRC mismatch on page" in refusal([bytes(corrupt)])
    assert "chained or multiplexed Ogg streams are unsupported" in refusal([first, M.ogg_page(0, 1, 8, 1, [1], b"\xbb")])
    assert "Ogg page sequence discontinuity: expected 1, got 2" in refusal([first, M.ogg_page(4, 1, 7, 2, [1], b"\xbb")])
    assert "Ogg packet continuation is missing its continued flag" in refusal([M.ogg_page(2, 0, 7, 0, [255], bytes(255)), last])
    assert "Ogg continued-packet flag has no preceding packet" in refusal([first, M.ogg_page(5, 1, 7, 1, [1], b"\xbb")])
    assert "truncated Ogg page: %d bytes remain" % (len(first) - 1) in refusal([first[:-1]])
    assert "Ogg logical stream is missing EOS" in refusal([first])
    assert "Ogg logical stream does not begin with BOS page zero" in refusal([M.ogg_page(0, 0, 7, 0, [1], b"\xaa")])
    assert "Ogg page appears after EOS" in refusal([first, last, M.ogg_page(0, 2, 7, 2, [1], b"\xcc")])
    assert "Ogg granule position moved backwards" in refusal([first, M.ogg_page(0, 5, 7, 1, [1], b"\xbb"), M.ogg_page(4, 4, 7, 2, [1], b"\xcc")])
    assert "invalid Ogg capture pattern at byte 0" in refusal([b"\x55" * 65536])
    assert "Ogg input chunk exceeds the 4194304 byte streaming budget" in refusal([bytes(4 * 1024 * 1024 + 1)])
    assert "unsupported Ogg page version 1" in refusal([first[:4] + b"\x01" + first[5:]])


def test_a_packet_continued_over_three_pages():
    body = bytes(range(256)) * 3  # 768 bytes: 255 + 255 + 255 + 3
    pages = [M.ogg_page(2, 0, 9, 0, [1], b"\x01"), M.ogg_page(0, 2 ** 64 - 1, 9, 1, [255, 255], body[:510]),
             M.ogg_page(1, 2 ** 64 - 1, 9, 2, [255], body[510:765]), M.ogg_page(5, 40, 9, 3, [3, 2], body[765:] + b"zz")]
    got = parse_all(b"".join(pages), 100)
    assert [p.data for p in got] == [b"\x01", body, b"zz"]
    assert got[1].granule_position is None and not got[1].last_in_page and got[2].last_in_page and got[2].last_in_stream and got[2].granule_position == 40


# ---- headers -----------------------------------------------------------------------------------------------------------------------

def fixture_headers():
    pk = M.ogg_packets(open(OGG, "rb").read())
    hdr, _ = webm_vorbis.vorbis_track(open(WEBM, "rb").read())
    return [p["data"] for p in pk[:3]], hdr


@pytest.mark.parametrize("which", [0, 1])
def test_fixture_headers_parse_as_the_model_parses_them(which):
    ident_p, comment_p, setup_p = fixture_headers()[which]
    ident = vorbis.parse_ident(ident_p)
    want = M.parse_ident(ident_p)
    assert {k: ident[k] for k in want} == want
    assert (ident["channels"], ident["sample_rate"], ident["blocksize_0"], ident["blocksize_1"]) == [(1, 8000, 512, 512), (2, 44100, 256, 2048)][which]
    vorbis.parse_comment(comment_p)
    M.parse_comment(comment_p)
    s = vorbis.Setup(ident, setup_p)
    m = M.parse_setup(setup_p, ident["channels"], ident["blocksize_0"], ident["blocksize_1"])
    assert (s.info["books"], s.info["floors"], s.info["residues"], s.info["mappings"], s.info["modes"]) == (
        len(m.books), len(m.floors), len(m.residues), len(m.mappings), len(m.modes))
    assert s.info["blob_bytes"] <= 4 << 20
    # every book of both fixtures is a complete prefix code: the strict reading of the specification refuses neither
    assert all(b.single < 0 for b in m.books)


def test_the_webm_walker_finds_the_track():
    hdr, packets = webm_vorbis.vorbis_track(open(WEBM, "rb").read())
    assert [len(h) for h in hdr] == [30, 93, 4140] and len(packets) >= 5 and hdr[0][:7] == b"\x01vorbis" and hdr[2][:7] == b"\x05vorbis"


def built(channels=2, bs=(64, 128), **kw):
    s = B.default_setup(channels, bs[0], bs[1], **kw)
    return s, vorbis.parse_ident(B.ident_header(channels, 16000, bs[0], bs[1]))


@pytest.mark.parametrize("channels,bs", [(1, (64, 128)), (2, (64, 64)), (3, (256, 2048)), (8, (64, 8192))])
def test_built_headers_parse_in_both_parsers(channels, bs):
    s, ident = built(channels, bs)
    assert (ident["channels"], ident["blocksize_0"], ident["blocksize_1"]) == (channels, bs[0], bs[1])
    vorbis.parse_comment(B.comment_header())
    hdr = B.setup_header(s)
    info = vorbis.Setup(ident, hdr).info
    m = M.parse_setup(hdr, channels, bs[0], bs[1])
    assert (info["books"], info["floors"], info["residues"], info["mappings"], info["modes"]) == (10, 2, 3, 2, 2) == (
        len(m.books), len(m.floors), len(m.residues), len(m.mappings), len(m.modes))
    assert [b.single for b in m.books].count(0) == 1


def mutate(path, value):
    def f(s):
        node = s
        for k in path[:-1]:
            node = node[k]
        node[path[-1]] = value
    return f


REFUSALS = [
    ("residue book number", mutate(("residues", 0, "books", 1, 0), 10), "book 10 does not exist"),
    ("residue book without values", mutate(("residues", 0, "books", 1, 0), 0), "has no values"),
    ("residue class book", mutate(("residues", 1, "classbook"), 77), "class book 77 does not exist"),
    ("class book dimensions", mutate(("residues", 0, "classbook"), 8), "too few entries for its class words"),
    ("partition size against a book's dimensions", mutate(("residues", 0, "partition_size"), 6), "no multiple of the dimensions"),
    ("residue end against the block sizes", mutate(("residues", 2, "end"), 65), "lies beyond the longest vector of this stream"),
    ("type 2 residue end against the block sizes", mutate(("residues", 1, "end"), 129), "lies beyond the longest vector of this stream"),
    ("residue end before begin", mutate(("residues", 0, "begin"), 1 << 20), "end before begin"),
    ("floor class master book", mutate(("floors", 0, "classes", 1, "master"), 10), "class master book 10 does not exist"),
    ("floor subclass book", mutate(("floors", 1, "classes", 2, "books"), [0, -1, 2, 10]), "subclass book 10 does not exist"),
    ("floor X list repeats", mutate(("floors", 0, "x"), [3, 9, 9, 12, 17, 20, 25, 30]), "X list repeats a value"),
    ("coupling channel", mutate(("mappings", 0, "coupling"), [(1, 1)]), "coupling channels 1 / 1"),
    ("submap floor", mutate(("mappings", 1, "floor"), [2]), "floor 2 does not exist"),
    ("submap residue", mutate(("mappings", 1, "residue"), [3]), "residue 3 does not exist"),
    ("mux", mutate(("mappings", 0, "mux"), [0, 2]), "assigned to submap 2"),
    ("mode mapping", mutate(("modes", 1), (1, 2)), "mapping 2 does not exist"),
    ("under-specified code book", mutate(("books", 0, "lengths"), [3] * 7 + [4]), "under-specified code lengths"),
    ("over-specified code book", mutate(("books", 0, "lengths"), [3] * 7 + [2]), "over-specified code lengths"),
    ("single entry of length 2", mutate(("books", 8, "lengths"), [2]), "a single entry must have length 1"),
    ("lookup type 3", mutate(("books", 3, "lookup"), 3), "lookup type 3"),
    ("time domain placeholder", mutate(("time",), 1), "time domain placeholder is not zero"),
    ("framing bit", mutate(("framing",), 0), "lacks its framing bit"),
]


@pytest.mark.parametrize("name,change,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_setup_validation_refuses_one_field_mutations(name, change, text):
    s, ident = built()
    vorbis.Setup(ident, B.setup_header(s))  # as built: accepted
    bad = copy.deepcopy(s)
    change(bad)
    hdr = B.setup_header(bad)
    with pytest.raises(SoundkitError) as e:
        vorbis.Setup(ident, hdr)
    assert e.value.status == vorbis.ERR_STREAM and text in str(e.value), str(e.value)
    with pytest.raises(M.VorbisError):
        M.parse_setup(hdr, 2, 64, 128)


def test_what_is_not_built_is_refused_as_unsupported():
    s, ident = built()
    bad = copy.deepcopy(s)
    bad["floors"][0]["type"] = 0
    with pytest.raises(SoundkitError) as e:
        vorbis.Setup(ident, B.setup_header(bad))
    assert e.value.status == -6 and "floor type 0 is not built" in str(e.value)
    s9 = B.default_setup(9, 64, 128)
    with pytest.raises(SoundkitError) as e:
        vorbis.Setup(vorbis.parse_ident(B.ident_header(9, 16000, 64, 128)), B.setup_header(s9))
    assert e.value.status == -6 and "more than 8 channels" in str(e.value)
    big = copy.deepcopy(s)  # 2^17 entries x 8 dimensions of VQ values: above the table budget
    big["books"][9] = B.book(8, [17] * (1 << 17), lookup=1, minimum=0, delta=B.pack_float(1, 0), value_bits=1, mults=[0, 1, 0, 1])
    with pytest.raises(SoundkitError) as e:
        vorbis.Setup(ident, B.setup_header(big))
    assert e.value.status == -6 and "table budget" in str(e.value)


def test_identification_header_refusals():
    good = B.ident_header(2, 44100, 256, 2048)
    assert vorbis.parse_ident(good)["sample_rate"] == 44100
    for bad, text in ((good[:7] + b"\x01" + good[8:], "unsupported Vorbis version"), (good[:11] + b"\x00" + good[12:], "no channels"),
                      (good[:28] + bytes([0xb5]) + good[29:], "block sizes"), (good[:28] + bytes([0x68]) + good[29:], "block sizes"),
                      (good[:29] + b"\x00", "framing bit"), (good[:20], "too short"), (b"\x03" + good[1:], "not a Vorbis identification header")):
        with pytest.raises(SoundkitError) as e:
            vorbis.parse_ident(bad)
        assert text in str(e.value)
    with pytest.raises(SoundkitError):
        vorbis.parse_comment(B.comment_header()[:-3])


def test_packet_first_bits():
    s, ident = built()
    setup = vorbis.Setup(ident, B.setup_header(s))
    rng = np.random.default_rng(1)
    assert setup.packet_blocksize(B.packet(rng, s, 0)) == (0, 64) and setup.packet_blocksize(B.packet(rng, s, 1, 1, 0)) == (0, 128)
    assert setup.packet_blocksize(b"\x01\x00") == (vorbis.NOT_AUDIO, 0) and setup.packet_blocksize(b"") == (vorbis.SHORT, 0)
    one = copy.deepcopy(s)
    one["modes"] = [(0, 0), (1, 1), (0, 0)]  # three modes: two bits, the fourth number names none
    assert vorbis.Setup(ident, B.setup_header(one)).packet_blocksize(b"\x06\x00") == (vorbis.BAD_MODE, 0)


# ---- the model ---------------------------------------------------------------------------------------------------------------------

def test_fast_imdct_is_the_direct_sum():
    rng = np.random.default_rng(0)
    for half in (32, 64, 256):
        x = rng.standard_normal(half)
        want = M.imdct_direct(x)
        assert np.abs(M.imdct(x, np.float64) - want).max() < 1e-11 * half
        assert np.abs(M.imdct(x, np.float32) - want).max() < 2e-6 * half


def test_inverse_db_table_ends():
    t = M.inverse_db(np.float32)
    assert t[0] == np.float32(1.0649863e-07) and t[255] == np.float32(1.0) and np.all(np.diff(t) > 0)


def test_model_against_the_recording(ogg_bytes, recording):
    """The float64 model of the Ogg fixture, narrowed by truncation, is within 1 LSB of every recorded sample and has the recording's
    length.  This holds the model -- books, floor, residue, window, overlap, the granule truncation -- to the reference's decoder."""
    ident, _, pcm = M.decode_ogg(ogg_bytes, np.float64)
    assert ident["sample_rate"] == 8000 and pcm.shape == (1, 23680) and len(recording) == 23680
    d = np.abs(M.to_s16(pcm[0]).astype(np.int32) - recording.astype(np.int32))
    print("samples that differ by one step: %d of %d (%.2e); by rounding instead of truncation %.3f would differ" % (
        (d > 0).sum(), d.size, (d > 0).mean(), (np.abs(np.rint(np.clip(pcm[0] * 32768, -32768, 32767)) - recording) > 0).mean()))
    assert d.max() <= 1


def test_mutated_files_under_sanitizers(tmp_path):
    """tests/fuzz_vorbis.cpp: csrc/ogg_stream.h and csrc/vorbis_stream.h alone with AddressSanitizer + UBSan on the CPU -- seeded
    mutations of the fixture through the Ogg parser, the three header parsers and the blob builder, every accepted blob walked as the
    kernel walks it"""
    exe = str(tmp_path / "fuzz_vorbis")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "fuzz_vorbis.cpp")], cwd=HERE)
    out = subprocess.run([exe, "1500", OGG], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "fuzz_vorbis ok" in out.stdout

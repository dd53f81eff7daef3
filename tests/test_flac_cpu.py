"""FLAC on the host (csrc/flac_stream.h): the frame-header parser, the CRC-bounded framer and the incremental reader, field exact
against tests/flac_model.py -- which is itself pinned here by the reference's fixture, its 16 kHz twin and the STREAMINFO MD5 -- plus
every rejection and a sanitizer fuzz (tests/fuzz_flac.cpp).  No GPU."""
import hashlib
import os
import random
import subprocess

import pytest

import flac_builder as B
import flac_model as M
from soundkit_amd import SoundkitError, flac

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "flac")
FIXTURE = os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts.flac")
TWIN = os.path.join(HERE, "golden", "linear16_A_Tusk.s16le")
STEREO_TWIN = os.path.join(HERE, "golden", "wav_stereo_A_Tusk.wav")
OK = 0
HEADER_FIELDS = ("number", "sample_rate", "block_size", "header_bytes", "channels", "assignment", "bits_per_sample", "variable_blocksize")


@pytest.fixture(scope="module")
def fixture_bytes():
    return open(FIXTURE, "rb").read()


@pytest.fixture(scope="module")
def fixture_model(fixture_bytes):
    return M.decode_stream(fixture_bytes)


def s16(samples):
    return b"".join((v & 0xFFFF).to_bytes(2, "little") for v in samples)


# ---- the model and the builder are pinned first ---------------------------------------------------------------------------------------

def test_model_decodes_the_fixture_to_its_twin_and_md5(fixture_bytes, fixture_model):
    info, frames = fixture_model
    twin = open(TWIN, "rb").read()
    assert len(fixture_bytes) == 45991 and len(twin) == 94720
    assert (info["sample_rate"], info["channels"], info["bits_per_sample"], info["total_samples"]) == (16000, 1, 16, 47360)
    assert [h["block_size"] for h, _ in frames] == [1152] * 41 + [128]  # every CRC-8 and CRC-16 held, or decode_stream had raised
    assert s16(v for _, ch in frames for v in ch[0]) == twin
    assert info["md5"].hex() == "61823f38c2798c6ee6d41876a55221c0" == hashlib.md5(twin).hexdigest() == M.md5_of(frames, 16).hex()


def test_model_decodes_the_headerless_fixtures_to_their_twins():
    twin = open(TWIN, "rb").read()
    stereo = open(STEREO_TWIN, "rb").read()
    stereo = stereo[stereo.index(b"data") + 8:]
    f16 = M.decode_frames(open(os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts_16bit.flac"), "rb").read())
    assert len(f16) == 11 and all(h["block_size"] == 4096 and h["assignment"] == 8 for h, _ in f16)
    assert s16(v for _, ch in f16 for v in M.interleave(ch)) == stereo[:45056 * 4]
    f24 = M.decode_frames(open(os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts_24bit.flac"), "rb").read())
    assert len(f24) == 11 and all(h["bits_per_sample"] == 24 for h, _ in f24)
    want = [int.from_bytes(twin[2 * i:2 * i + 2], "little", signed=True) << 8 for i in range(45056)]
    assert [v for _, ch in f24 for v in ch[0]] == want
    f32 = M.decode_frames(open(os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts_32float.flac"), "rb").read())
    assert len(f32) == 11 and all(h["bits_per_sample"] == 32 and h["block_size"] == 4096 for h, _ in f32)


def builder_streams():
    """a few streams that use every kind of subframe; (name, stream bytes, frames' bytes, blocks, bits)"""
    rng = random.Random(7)
    out = []
    for name, bits, nch, sizes, variable in (("mono16", 16, 1, [192, 192, 77], False), ("stereo24v", 24, 2, [64, 160, 33, 1], True),
                                              ("six8", 8, 6, [48, 48], False)):
        lim = 1 << (bits - 1)
        blocks = [[[rng.randrange(-lim, lim) for _ in range(n)] for _ in range(nch)] for n in sizes]

        def specs(i, ch, bits=bits):
            kinds = [{"type": "verbatim"}, {"type": "fixed", "order": min(2, len(ch[0])), "params": bits - 1, "method": 1},
                     {"type": "lpc", "order": min(3, len(ch[0])), "precision": 8, "shift": 9, "coefs": [100, -50, 20][:min(3, len(ch[0]))],
                      "params": ("esc", min(bits + 3, 31) if bits < 24 else 27), "method": 1}]
            return [kinds[(i + c) % 3] for c in range(len(ch))]
        data, frames = B.stream(blocks, bits, 44100, specs, variable=variable)
        out.append((name, data, frames, blocks, bits))
    return out


@pytest.fixture(scope="module")
def built():
    return builder_streams()


def test_builder_streams_decode_in_the_model_to_what_they_were_built_from(built):
    for name, data, frames, blocks, bits in built:
        info, got = M.decode_stream(data)
        assert [ch for _, ch in got] == blocks, name
        assert info["md5"] == M.md5_of(got, bits), name
        assert [h["frame_bytes"] for h, _ in got] == [len(f) for f in frames]


# ---- the header parser ------------------------------------------------------------------------------------------------------------------

def agree(head, info=None, model_info=None):
    rc, got = flac.parse_header(head + b"\0\0\0\0", info)
    want = M.parse_header(head, model_info)
    assert rc == OK and {k: got[k] for k in HEADER_FIELDS} == {k: want[k] for k in HEADER_FIELDS}, (head.hex(), got, want)
    assert got["header_bytes"] == len(head)
    return got


def test_every_block_size_code():
    for code, block in [(1, 192), (2, 576), (3, 1152), (4, 2304), (5, 4608)] + [(8 + k, 256 << k) for k in range(8)]:
        assert agree(B.header(block, 44100, 16, 0, 0, bs_code=code))["block_size"] == block
    for block in (1, 17, 256):
        assert agree(B.header(block, 44100, 16, 0, 0, bs_code=6))["block_size"] == block
    for block in (1, 257, 4097, 65535, 65536):
        assert agree(B.header(block, 44100, 16, 0, 0, bs_code=7))["block_size"] == block


def test_every_sample_rate_code():
    for rate in (88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000):
        assert agree(B.header(192, rate, 16, 0, 0))["sample_rate"] == rate
    assert agree(B.header(192, 255000, 16, 0, 0, rate_code=12))["sample_rate"] == 255000
    assert agree(B.header(192, 11025, 16, 0, 0, rate_code=13))["sample_rate"] == 11025
    assert agree(B.header(192, 655350, 16, 0, 0, rate_code=14))["sample_rate"] == 655350
    info = flac.streaminfo(sample_rate=12345, channels=1, bits_per_sample=16)
    assert agree(B.header(192, 0, 16, 0, 0, rate_code=0), info, {"sample_rate": 12345, "bits_per_sample": 16})["sample_rate"] == 12345


def test_every_depth_code_and_assignment():
    for bits in (8, 12, 16, 20, 24, 32):
        assert agree(B.header(192, 44100, bits, 0, 0))["bits_per_sample"] == bits
    info = flac.streaminfo(sample_rate=44100, channels=1, bits_per_sample=5)
    assert agree(B.header(192, 44100, 5, 0, 0), info, {"sample_rate": 44100, "bits_per_sample": 5})["bits_per_sample"] == 5
    for a in range(11):
        got = agree(B.header(192, 44100, 16, a, 0))
        assert (got["assignment"], got["channels"]) == (a, a + 1 if a < 8 else 2)


def test_coded_numbers_up_to_36_bits():
    for n in (0, 0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x1FFFFF, 0x200000, 0x3FFFFFF, 0x4000000, 0x7FFFFFFF):
        assert agree(B.header(192, 44100, 16, 0, n))["number"] == n
    for n in (0x80000000, 0xFFFFFFFFF):
        got = agree(B.header(192, 44100, 16, 0, n, variable=True))
        assert got["number"] == n and got["variable_blocksize"] == 1
    # a 7-byte number is a sample number: not in a fixed-blocksize frame
    assert flac.parse_header(B.header(192, 44100, 16, 0, 0x80000000, variable=False))[0] == flac.RESERVED


def test_header_rejections():
    good = B.header(192, 44100, 16, 0, 5)
    assert flac.parse_header(good)[0] == OK
    assert flac.parse_header(B.header(192, 44100, 16, 0, 5, rate_code=15))[0] == flac.RESERVED
    assert flac.parse_header(B.header(192, 44100, 16, 0, 5, depth_code=3))[0] == flac.RESERVED
    assert flac.parse_header(B.header(192, 44100, 16, 0, 5, bs_code=0))[0] == flac.RESERVED
    assert flac.parse_header(B.header(192, 44100, 16, 0, 5, reserved_bit=1))[0] == flac.RESERVED
    assert flac.parse_header(B.header(192, 44100, 16, 0, 5, sync_reserved=1))[0] == flac.RESERVED
    for a in range(11, 16):
        assert flac.parse_header(B.header(192, 44100, 16, a, 5))[0] == flac.RESERVED
    assert flac.parse_header(good[:-1] + bytes([good[-1] ^ 1]))[0] == flac.BAD_CRC
    assert flac.parse_header(b"\xff\xf0" + good[2:])[0] == flac.NO_SYNC
    assert flac.parse_header(b"\x00" + good[1:])[0] == flac.NO_SYNC
    for cut in range(1, len(good)):
        assert flac.parse_header(good[:cut])[0] == flac.NEED_MORE, cut
    bad_number = bytearray(B.header(192, 44100, 16, 0, 0x800))
    bad_number[5] = 0x40  # a continuation byte that is none
    assert flac.parse_header(bytes(bad_number))[0] == flac.RESERVED
    # a header that refers to STREAMINFO has a status of its own when there is none
    for kw in ({"rate_code": 0}, {"depth_code": 0}):
        h = B.header(192, 44100, 16, 0, 5, **kw)
        assert flac.parse_header(h)[0] == flac.NEED_STREAMINFO
        assert flac.parse_header(h, flac.streaminfo(sample_rate=44100, channels=1, bits_per_sample=16))[0] == OK


# ---- the framer ---------------------------------------------------------------------------------------------------------------------------

def test_scan_of_the_headerless_fixtures_agrees_with_the_model():
    for name in ("16bit", "24bit", "32float"):
        data = open(os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts_%s.flac" % name), "rb").read()
        want = M.decode_frames(data)
        rc, got, used = flac.scan(data, final=True)
        assert rc == OK and used == len(data) and len(got) == 11
        for g, (h, _) in zip(got, want):
            assert {k: g[k] for k in HEADER_FIELDS + ("offset", "frame_bytes")} == {k: h[k] for k in HEADER_FIELDS + ("offset", "frame_bytes")}
        rc, got, used = flac.scan(data, final=False)  # the last frame's end is not known before the data ends
        assert rc == OK and len(got) == 10 and used == want[10][0]["offset"]
        rc, got, used = flac.scan(data, final=True, cap=3)
        assert rc == OK and len(got) == 3 and used == want[3][0]["offset"]


def test_a_false_sync_with_a_valid_crc8_does_not_split_a_frame():
    fake = B.header(16, 44100, 16, 0, 1)  # a whole valid header, CRC-8 and all
    words = [int.from_bytes(fake[i:i + 2].ljust(2, b"\0"), "big", signed=True) for i in range(0, len(fake), 2)]
    samples = [7, -3] + words + [100, -100] * 4
    samples += [0] * (32 - len(samples))
    frames = [B.frame([samples], 16, 44100, 0, [{"type": "verbatim"}]), B.frame([[5] * 32], 16, 44100, 1, [{"type": "constant"}])]
    data = b"".join(frames)
    at = data.index(fake)
    assert 0 < at < len(frames[0]) and flac.parse_header(data[at:])[0] == OK  # the planted header is one
    rc, got, used = flac.scan(data, final=True)
    assert rc == OK and [(g["offset"], g["frame_bytes"]) for g in got] == [(0, len(frames[0])), (len(frames[0]), len(frames[1]))]


def test_a_flipped_payload_bit_is_an_error_not_a_skipped_frame(fixture_bytes):
    info, _, first = M.split_stream(fixture_bytes)
    frames = fixture_bytes[first:]
    si = flac.streaminfo(sample_rate=16000, channels=1, bits_per_sample=16, max_framesize=info["max_framesize"])
    rc, got, _ = flac.scan(frames, si, final=True)
    assert rc == OK and len(got) == 42
    bad = bytearray(frames)
    bad[got[3]["offset"] + 100] ^= 0x10
    for stream_info in (si, None):
        rc, found, used = flac.scan(bytes(bad), stream_info, final=True)
        assert rc == flac.BAD_CRC and len(found) == 3 and used == got[3]["offset"]
    r = flac.FlacReader()
    with pytest.raises(SoundkitError) as exc:
        r.add(fixture_bytes[:first] + bytes(bad))
    assert exc.value.status == flac.ERR_STREAM and "frame 3" in r.last_error() and "CRC" in r.last_error()
    with pytest.raises(SoundkitError):  # and it stays rejected
        r.add(b"")
    r.close()


# ---- the reader ---------------------------------------------------------------------------------------------------------------------------

def read_all(data, piece, cap=4096):
    r = flac.FlacReader()
    out = []
    for at in range(0, len(data), piece):
        out += r.add(data[at:at + piece], cap)
    while True:
        got = r.add(b"", cap)
        out += got
        if not got:
            break
    info = r.info()
    r.close()
    return out, info


def test_reader_chunk_invariance(fixture_bytes, fixture_model):
    minfo, mframes = fixture_model
    whole, info = read_all(fixture_bytes, len(fixture_bytes))
    assert len(whole) == 42 and info["frames"] == 42 and info["buffered_bytes"] == 0
    assert {k: info["streaminfo"][k] for k in minfo} == minfo
    first = M.split_stream(fixture_bytes)[2]
    assert b"".join(b for _, b in whole) == fixture_bytes[first:]
    for (d, b), (h, _) in zip(whole, mframes):
        assert {k: d[k] for k in HEADER_FIELDS} == {k: h[k] for k in HEADER_FIELDS} and len(b) == h["frame_bytes"]
    for piece, cap in ((1, 4096), (7, 4096), (4096, 4096), (4096, 2)):
        got, _ = read_all(fixture_bytes, piece, cap)
        assert [(dict(d, offset=0), b) for d, b in got] == [(dict(d, offset=0), b) for d, b in whole], piece


def test_variable_blocksize_stream_and_builder_streams_through_the_reader(built):
    for name, data, frames, blocks, bits in built:
        for piece in (len(data), 5):
            got, info = read_all(data, piece)
            assert [b for _, b in got] == frames, name
            assert [d["block_size"] for d, _ in got] == [len(ch[0]) for ch in blocks]
        if name == "stereo24v":
            assert all(d["variable_blocksize"] for d, _ in got) and [d["number"] for d, _ in got] == [0, 64, 224, 257]


def test_all_skippable_metadata_kinds_and_a_large_picture_is_not_buffered(built):
    _, data, frames, _, _ = built[0]
    head, tail = data[:4 + 4 + 34], data[4 + 4 + 34:]
    head = head[:4] + bytes([head[4] & 0x7F]) + head[5:]  # STREAMINFO is not the last block any more
    blocks = b"".join(B.metadata(kind, bytes([kind]) * n) for kind, n in ((1, 0), (1, 100), (2, 20), (3, 36), (4, 60), (5, 400), (6, 3000)))
    picture = B.metadata(6, b"\xff\xf8" * (1 << 19), last=True)  # 1 MiB of sync codes
    stream = head + blocks + picture + tail
    r = flac.FlacReader()
    got, worst = [], 0
    for at in range(0, len(stream), 65536):
        got += r.add(stream[at:at + 65536])
        worst = max(worst, r.info()["buffered_bytes"])
    got += r.add(b"")
    assert [b for _, b in got] == frames and worst <= max(len(f) for f in frames) + 65536 and r.info()["buffered_bytes"] == 0
    r.close()
    r = flac.FlacReader()  # and within the picture nothing is held at all
    r.add(stream[:len(head) + len(blocks) + 500000])
    assert r.info()["buffered_bytes"] == 0
    r.close()


@pytest.mark.parametrize("what, text", [("length", "STREAMINFO is 33 bytes"), ("type127", "127"), ("first", "first block"), ("second", "second STREAMINFO"),
                                        ("marker", "marker")])
def test_bad_metadata(built, what, text):
    _, data, _, _, _ = built[0]
    body, tail = data[8:42], data[42:]
    stream = {"length": b"fLaC" + B.metadata(0, body[:33], last=True) + tail,
              "type127": b"fLaC" + B.metadata(0, body) + B.metadata(127, b"xx", last=True) + tail,
              "first": b"fLaC" + B.metadata(4, b"abcd") + B.metadata(0, body, last=True) + tail,
              "second": b"fLaC" + B.metadata(0, body) + B.metadata(0, body, last=True) + tail,
              "marker": b"fLaX" + data[4:]}[what]
    r = flac.FlacReader()
    with pytest.raises(SoundkitError) as exc:
        r.add(stream)
    assert exc.value.status == flac.ERR_STREAM and text in r.last_error()
    r.close()


def test_truncated_tail_is_reported_on_the_finalising_add(fixture_bytes):
    r = flac.FlacReader()
    got = r.add(fixture_bytes[:-20])
    assert len(got) == 41  # nothing wrong yet: more might come
    with pytest.raises(SoundkitError) as exc:
        r.add(b"")
    assert exc.value.status == flac.ERR_STREAM and "truncated" in r.last_error()
    r.close()
    r = flac.FlacReader()
    r.add(fixture_bytes[:30])
    with pytest.raises(SoundkitError):
        r.add(b"")
    assert "truncated" in r.last_error() and "metadata" in r.last_error()
    r.close()


def test_a_frame_that_disagrees_with_streaminfo_ends_the_stream(built):
    _, data, frames, blocks, _ = built[0]
    other = B.frame([[1] * 192, [2] * 192], 16, 44100, 1, [{"type": "constant"}] * 2)
    r = flac.FlacReader()
    with pytest.raises(SoundkitError):
        r.add(data[:42] + frames[0] + other + frames[2])
        r.add(b"")
    assert "disagree with STREAMINFO" in r.last_error()
    r.close()


def test_mutated_streams_under_sanitizers(tmp_path):
    """tests/fuzz_flac.cpp: csrc/flac_stream.h alone with AddressSanitizer + UBSan on the CPU -- seeded mutations of the fixture
    through the parser, the scan and the reader"""
    exe = str(tmp_path / "fuzz_flac")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "fuzz_flac.cpp")], cwd=HERE)
    out = subprocess.run([exe, "2000", FIXTURE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "fuzz_flac ok" in out.stdout

"""MPEG Layer I / II without a GPU: the reference's MP2 fixture against the float64 model (framing, bit use, the source PCM), and
the product's host parse (csrc/mp12_bitstream.cpp through sk_mpa_*) against frames written by tests/mp12_builder.py -- every record
field exact -- plus its rejections and a sanitizer fuzz of the host code (tests/fuzz_mp12.cpp)."""
import os
import subprocess
import wave

import numpy as np
import pytest

import mp12_builder as B
import mp12_model as M
from soundkit_amd import mp3

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "mp2", "stereo48k_A_Tusk_1s.mp2")
SOURCE = os.path.join(HERE, "golden", "wav_stereo_A_Tusk.wav")
ENCODER_DELAY = 481                 # ffmpeg's MP2 encoder: both channels
SNR_FLOOR = (19.97, 19.61)          # measured with the model: 20.97 dB and 20.61 dB (192 kbit/s; the source is 16 kHz material taken to 48 kHz)
OK, NEED_MORE, UNSUPPORTED, INVALID = 0, -301, -303, -304


@pytest.fixture(scope="module")
def fixture_bytes():
    return open(FIXTURE, "rb").read()


@pytest.fixture(scope="module")
def model_pcm(fixture_bytes):
    return M.Decoder().stream(fixture_bytes)


def test_fixture_framing_and_bit_use(fixture_bytes):
    d = fixture_bytes
    assert len(d) == 24192 and d[:4] == bytes([0xFF, 0xFD, 0xA4, 0x04])
    frames, used, layer = mp3.mpa_scan(d)
    assert len(frames) == 42 and used == len(d) and layer == 2
    mine = M.scan(d)
    assert len(mine) == 42
    swapped = dict(M.TABLES, **{"B.2a": "AAA" + "A" * 8 + "C" * 12 + "D" * 4})  # negative control: row B read as row A in subbands 3 ... 10
    for i, (f, (off, h)) in enumerate(zip(frames, mine)):
        assert (f.offset, f.frame_bytes, f.version, f.layer, f.has_crc, f.bitrate_kbps, f.sample_rate, f.mode, f.channels, f.samples_per_channel) == \
            (576 * i, 576, 1, 2, 0, 192, 48000, 0, 2, 1152)
        assert off == 576 * i and (h["version"], h["layer"], h["crc"], h["bitrate_kbps"], h["sample_rate"], h["mode"]) == (1, 2, False, 192, 48000, 0)
        p = M.parse_frame(d[off:off + 576], h)
        assert p["sblimit"] == 27 and p["bits"] == 4608  # allocation, scfsi, scale factors and samples fill the frame to the bit
        assert M.parse_frame(d[off:off + 576], h, swapped)["bits"] != 4608
        rc, rec = mp3.mpa_parse_frame(d[off:off + 576], f)
        assert rc == OK and rec.sample_bit == p["sample_bit"] and rec.granule_bits == p["granule_bits"]
        assert rec.sample_bit + 12 * rec.granule_bits == 4608


def test_fixture_against_the_source(model_pcm):
    from scipy.signal import resample_poly
    with wave.open(SOURCE) as w:
        assert (w.getframerate(), w.getnchannels(), w.getsampwidth()) == (16000, 2, 2)
        x = np.frombuffer(w.readframes(20000), "<i2").reshape(-1, 2).astype(np.float64) / 32768.0
    src = resample_poly(x, 3, 1, axis=0)
    assert model_pcm.shape == (42 * 1152, 2) and np.abs(model_pcm).max() < 1.0
    for c in range(2):
        s = src[:40000, c]
        lag = max(range(0, 1200), key=lambda L: float(np.dot(model_pcm[L:L + 40000, c], s)))
        a = model_pcm[lag:lag + 40000, c]
        gain = np.dot(a, s) / np.dot(s, s)
        snr = 10 * np.log10(np.sum((gain * s) ** 2) / np.sum((a - gain * s) ** 2))
        print("channel %d: lag %d, gain %.4f, SNR %.2f dB" % (c, lag, gain, snr))
        assert lag == ENCODER_DELAY
        assert 0.99 < gain < 1.0
        assert snr > SNR_FLOOR[c], snr


# ---- the host parse against the builder ------------------------------------------------------------------------------------------
# (layer, lsf, rate index, bit-rate index, mode, mode_ext, crc, padding): every Layer II table, mono / stereo / dual, joint stereo
# with each bound, CRC and padding on and off
CONFIGS = {
    "B.2a stereo 48k 192k": (2, 0, 1, 10, 0, 0, False, 0),
    "B.2a dual 44.1k 160k pad": (2, 0, 0, 9, 2, 0, False, 1),
    "B.2b stereo 44.1k 256k crc": (2, 0, 0, 12, 0, 0, True, 0),
    "B.2b mono 32k 128k": (2, 0, 2, 8, 3, 0, False, 0),
    "B.2c mono 48k 48k": (2, 0, 1, 2, 3, 0, False, 0),
    "B.2c stereo 44.1k 64k crc pad": (2, 0, 0, 4, 0, 0, True, 1),
    "B.2d mono 32k 32k": (2, 0, 2, 1, 3, 0, True, 0),
    "B.2d stereo 32k 96k": (2, 0, 2, 6, 0, 0, False, 0),
    "LSF mono 24k 64k": (2, 1, 1, 8, 3, 0, False, 0),
    "LSF stereo 22.05k 128k pad": (2, 1, 0, 12, 0, 0, False, 1),
    "joint bound 4": (2, 0, 1, 10, 1, 0, False, 0),
    "joint bound 8 crc": (2, 0, 1, 10, 1, 1, True, 0),
    "joint bound 12 B.2b": (2, 0, 0, 12, 1, 2, False, 0),
    "joint bound 16 LSF": (2, 1, 2, 10, 1, 3, False, 0),
    "joint bound 16 over sblimit 8": (2, 0, 1, 4, 1, 3, False, 0),
    "Layer I stereo 48k 384k": (1, 0, 1, 12, 0, 0, False, 0),
    "Layer I mono 44.1k 192k pad crc": (1, 0, 0, 6, 3, 0, True, 1),
    "Layer I joint bound 8 32k": (1, 0, 2, 10, 1, 1, False, 0),
    "Layer I LSF dual 16k 128k": (1, 1, 2, 8, 2, 0, False, 0),
}


def check_record(frame, want, label=""):
    h = want["header"]
    rc, info = mp3.mpa_parse_header(frame[:4])
    assert rc == OK, label
    assert (info.layer, info.version, info.sample_rate, info.bitrate_kbps, info.frame_bytes, info.channels, info.mode, info.mode_ext, info.has_crc,
            info.padding, info.samples_per_channel) == (h["layer"], 2 if h["lsf"] else 1, h["sample_rate"], h["bitrate_kbps"], h["frame_bytes"],
                                                        h["channels"], h["mode"], h["mode_ext"], int(h["crc"]), h["padding"],
                                                        384 if h["layer"] == 1 else 1152), label
    assert len(frame) == info.frame_bytes
    rc, rec = mp3.mpa_parse_frame(frame, info)
    assert rc == OK, label
    assert (rec.layer, rec.channels, rec.sblimit, rec.bound, rec.granules, rec.byte_len, rec.sample_rate) == \
        (h["layer"], h["channels"], want["sblimit"], want["bound"], 12, h["frame_bytes"], h["sample_rate"]), label
    assert np.array_equal(np.ctypeslib.as_array(rec.cls), want["cls"]), label
    assert np.array_equal(np.ctypeslib.as_array(rec.scf), want["scf"]), label
    assert rec.sample_bit == want["sample_bit"] and rec.granule_bits == want["granule_bits"], label
    assert rec.sample_bit + rec.granules * rec.granule_bits == want["bits"], label
    # and the model reads the same frame the same way
    p = M.parse_frame(frame, M.parse_header(frame[:4]))
    assert p["bits"] == want["bits"] and np.array_equal(p["steps"], want["steps"]) and np.array_equal(p["scf"], want["scf"]), label
    return rec


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_host_parse_equals_what_the_builder_wrote(name):
    rng = np.random.default_rng(sum(name.encode()))
    for code_mode in ("random", "zero", "max", "middle"):
        frame, want = B.random_frame(rng, *CONFIGS[name], code_mode=code_mode)
        check_record(frame, want, name)
    assert want["bound"] <= want["sblimit"]


def test_all_four_scfsi_patterns_are_read():
    h4, h = B.header(2, 0, 1, 10, 0)
    alloc = np.zeros((2, 32), np.int64)
    alloc[:, :8] = 1
    scfsi = np.zeros((2, 32), np.int64)
    scfsi[0, :8] = [0, 1, 2, 3, 0, 1, 2, 3]
    scfsi[1, :8] = [3, 2, 1, 0, 3, 2, 1, 0]
    scf = np.arange(2 * 32 * 3).reshape(2, 32, 3) % 64
    frame, want = B.build_frame(h4, h, alloc, scfsi, scf, np.ones((12, 32, 2, 3), np.int64))
    want["header"] = h
    rec = check_record(frame, want)
    got = np.ctypeslib.as_array(rec.scf)
    assert got[0][0].tolist() == [0, 1, 2] and got[0][1].tolist() == [3, 3, 5] and got[0][2].tolist() == [6, 6, 6] and got[0][3].tolist() == [9, 10, 10]


@pytest.mark.parametrize("row", sorted(M.ROWS))
@pytest.mark.parametrize("code_mode", ["zero", "max", "middle"])
def test_every_quantisation_class_of_every_row(row, code_mode):
    """one frame per allocation index of the row: every subband of that row (first channel) carries it"""
    # a configuration whose table holds the row, with room for twelve subbands of 48-bit triples
    cfg = {"A": (2, 0, 1, 14, 0), "B": (2, 0, 1, 14, 0), "C": (2, 0, 1, 14, 0), "D": (2, 0, 1, 14, 0), "E": (2, 0, 2, 6, 0), "F": (2, 0, 2, 6, 0),
           "G": (2, 1, 1, 14, 0), "H": (2, 1, 1, 14, 0)}[row]
    h4, h = B.header(*cfg)
    rows, sblimit, _ = B.geometry(h)
    assert row in rows
    for a in range(1, len(M.ROWS[row][1]) + 1):
        alloc = np.zeros((2, 32), np.int64)
        steps = M.ROWS[row][1][a - 1]
        for sb in range(sblimit):
            if rows[sb] == row:
                alloc[0][sb] = a
        top = steps - 1 if steps in M.GROUPED_BITS else steps
        code = {"zero": 0, "max": top, "middle": top // 2}[code_mode]
        frame, want = B.build_frame(h4, h, alloc, np.full((2, 32), a % 4), np.full((2, 32, 3), (7 * a) % 64), np.full((12, 32, 2, 3), code, np.int64))
        want["header"] = h
        rec = check_record(frame, want, "%s/%d" % (row, a))
        assert rec.cls[0][rows.index(row)] == M.class_code(steps)


@pytest.mark.parametrize("nb", range(2, 16))
def test_layer_one_bit_widths(nb):
    h4, h = B.header(1, 0, 1, 14, 0)  # 448 kbit/s at 48 kHz: 448 bytes, room for sixteen 15-bit subband-channels
    alloc = np.zeros((2, 32), np.int64)
    alloc[0, :12] = nb - 1
    alloc[1, :12:3] = nb - 1
    scf = np.arange(2 * 32 * 3).reshape(2, 32, 3) // 3 % 64
    codes = np.random.default_rng(nb).integers(0, (1 << nb) - 1, (12, 32, 2, 3))
    frame, want = B.build_frame(h4, h, alloc, np.zeros((2, 32), np.int64), scf, codes)
    want["header"] = h
    rec = check_record(frame, want)
    assert rec.cls[0][5] == nb and rec.granule_bits == nb * 16


def test_rejections(fixture_bytes):
    # Layer I: allocation 15 is forbidden
    h4, h = B.header(1, 0, 1, 12, 0)
    alloc = np.zeros((2, 32), np.int64)
    alloc[0][3] = 15
    frame, _ = B.build_frame(h4, h, alloc, np.zeros((2, 32), np.int64), np.zeros((2, 32, 3), np.int64), np.zeros((12, 32, 2, 3), np.int64), allow_overrun=True)
    rc, info = mp3.mpa_parse_header(frame[:4])
    assert rc == OK and mp3.mpa_parse_frame(frame, info)[0] == INVALID
    # Layer II: an allocation whose samples would end beyond the frame (every subband at its widest class in 64 kbit/s)
    h4, h = B.header(2, 0, 1, 4, 0)
    rows, sblimit, _ = B.geometry(h)
    alloc = np.zeros((2, 32), np.int64)
    for sb in range(sblimit):
        alloc[:, sb] = len(M.ROWS[rows[sb]][1])
    frame, want = B.build_frame(h4, h, alloc, np.zeros((2, 32), np.int64), np.zeros((2, 32, 3), np.int64), np.zeros((12, 32, 2, 3), np.int64), allow_overrun=True)
    assert want["bits"] > 8 * h["frame_bytes"]
    rc, info = mp3.mpa_parse_header(frame[:4])
    assert rc == OK and mp3.mpa_parse_frame(frame, info)[0] == INVALID
    # the same allocation one class narrower in the top subbands still fits?  no claim; a clean fixture frame does, a truncated one waits
    rc, info = mp3.mpa_parse_header(fixture_bytes[:4])
    assert rc == OK and mp3.mpa_parse_frame(fixture_bytes[:576], info)[0] == OK
    assert mp3.mpa_parse_frame(fixture_bytes[:575], info)[0] == NEED_MORE
    assert mp3.mpa_parse_header(fixture_bytes[:3])[0] == NEED_MORE
    # the Layer III entry point keeps its answer for a Layer II header; free format and MPEG-2.5 stay out
    assert mp3.parse_header(b"\xff\xfd\x90\x00")[0] == UNSUPPORTED
    assert mp3.mpa_parse_header(b"\xff\xfd\x04\x00")[0] == UNSUPPORTED   # Layer II, free format
    assert mp3.mpa_parse_header(b"\xff\xe5\x94\x00")[0] == UNSUPPORTED   # MPEG-2.5 with Layer II
    rc, info = mp3.mpa_parse_header(b"\xff\xfb\x90\x00")
    assert rc == OK and info.layer == 3 and info.frame_bytes == 417
    assert mp3.mpa_parse_frame(b"\xff\xfb\x90\x00" + bytes(413), info)[0] == UNSUPPORTED


def test_a_streams_layer_is_that_of_its_first_confirmed_frame(fixture_bytes):
    d = fixture_bytes
    # one frame alone confirms nothing; with the next header behind it the layer is known
    frames, used, layer = mp3.mpa_scan(d[:576])
    assert (len(frames), used, layer) == (0, 0, 0)
    frames, used, layer = mp3.mpa_scan(d[:580])
    assert (len(frames), used, layer) == (1, 576, 2)
    # inside an established stream a header of another layer is no frame, garbage is stepped over, the last frame needs no follower;
    # the frame in FRONT of the foreign bytes has no consistent header behind it and goes with them (sk_mp3_scan's rule)
    l3 = b"\xff\xfb\x90\x00" + bytes(413)
    frames, used, layer = mp3.mpa_scan(d[:1152] + l3 + b"junk" + d[1152:2304], layer=2)
    assert [f.offset for f in frames] == [0, 1152 + 417 + 4, 1152 + 417 + 4 + 576] and used == 2304 + 421 and layer == 2
    frames, used, layer = mp3.mpa_scan(l3 + l3 + d[:1152])
    assert layer == 3 and [f.offset for f in frames] == [0] and frames[0].layer == 3  # the second has a Layer II header behind it


def test_mutated_frames_under_sanitizers(tmp_path):
    """tests/fuzz_mp12.cpp: csrc/mp12_bitstream.cpp alone with AddressSanitizer + UBSan on the CPU -- the fixture's frames and
    mutants through header parse, scan, frame parse and the check in front of the kernel: no out-of-bounds access, no undefined
    behaviour, and no record is accepted whose samples would end beyond its frame."""
    exe = str(tmp_path / "fuzz_mp12")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "fuzz_mp12.cpp")], cwd=HERE)
    out = subprocess.run([exe, "3000", FIXTURE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "fuzz_mp12 ok" in out.stdout

"""Compressed WAV without a GPU: the walker's coded mode (csrc/pcm_stream.h through sk_wav_coded_reader_*) on the fixtures of
tests/golden/wav_coded and on files built here -- every tag, every refusal text, the fmt extensions, the fact rule, RF64, odd chunks,
any cut of the file -- and what pins tests/wav_adpcm_model.py to the outside world: the reference's G.711 recordings, Python's audioop
for IMA, a hand-worked block for Microsoft ADPCM.  The reference-shaped reader (sk_wav_reader_*) must still refuse all four tags.
tests/fuzz_wav_coded.cpp runs the walker under the sanitizers as a program of its own."""
import os
import struct
import subprocess
import wave

import numpy as np
import pytest

import g72x_model
import wav_adpcm_model as M
import wav_coded_builder as B

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
DIR = os.path.join(GOLD, "wav_coded")
# name: (tag, channels, block_align, frames_per_block, fact, total_frames)
FIXTURES = {"ulaw_A_Tusk.wav": (7, 1, 1, 1, 0, 23680), "alaw_A_Tusk.wav": (6, 1, 1, 1, 0, 23680),
            "ima_mono_8k.wav": (0x11, 1, 256, 505, 3000, 3000), "ima_stereo.wav": (0x11, 2, 1024, 1017, 2500, 2500),
            "ms_mono_8k.wav": (2, 1, 256, 500, 3000, 3000), "ms_stereo.wav": (2, 2, 1024, 1012, 2500, 2500)}
# the model's SNR on the four ADPCM fixtures against the speech they were encoded from, measured when they were written (README.md)
SNR_DB = {"ima_mono_8k.wav": 19.195, "ima_stereo.wav": 22.305, "ms_mono_8k.wav": 19.777, "ms_stereo.wav": 22.541}


def load(name):
    return open(os.path.join(DIR, name), "rb").read()


def speech():
    return np.frombuffer(open(os.path.join(GOLD, "linear16_8k_A_Tusk.s16le"), "rb").read(), "<i2")


def coded_reader():
    from soundkit_amd import pcm_stream
    return pcm_stream.WavCodedReader()


def walk(data, size, make=coded_reader):
    """-> ([(offset, bytes)], info, error text or None); size 0: the file in one add.  An empty add ends every walk: it is what
    meets a data chunk that ended inside a frame or a block when the piece in front of it took the whole add."""
    rd, got, err = make(), [], None
    try:
        for chunk in [data[at:at + (size or len(data))] for at in range(0, len(data), size or len(data))] + [b""]:
            p = rd.add(chunk)
            if p is not None:
                got.append(p)
    except ValueError as e:
        err = str(e)
    return got, rd.info(), err


def check_pieces(got, payload, first_offset, unit):
    """whole units, one after the other, together the payload"""
    at = first_offset
    for off, piece in got:
        assert off == at and len(piece) % unit == 0 and len(piece) > 0
        at += len(piece)
    assert b"".join(p for _, p in got) == payload


# ---- the fixtures --------------------------------------------------------------------------------------------------------------------

def test_the_committed_fixtures_are_what_the_builder_writes():
    made = B.fixtures(GOLD)
    assert sorted(made) == sorted(n for n in os.listdir(DIR) if n not in ("README.md", "ima_mono_8k.audioop.s16le"))
    for name, data in made.items():
        assert load(name) == data, name


@pytest.mark.parametrize("name", sorted(FIXTURES))
@pytest.mark.parametrize("size", [1, 7, 0])
def test_fixtures_through_the_coded_reader(name, size):
    data = load(name)
    tag, ch, align, per_block, fact, total = FIXTURES[name]
    payload = B.data_of(data)
    got, info, err = walk(data, size)
    assert err is None
    check_pieces(got, payload, len(data) - len(payload), align)
    if size == 0:
        assert len(got) == 1
    assert (info["tag"], info["sample_rate"], info["channels"], info["block_align"], info["frames_per_block"]) == (tag, 8000, ch, align, per_block)
    assert (info["fact_frames"], info["total_frames"], info["is_float"]) == (fact, total, False)
    assert info["bits"] == (8 if tag in (6, 7) else 4)
    assert info["coef"] == (M.MS_COEF if tag == 2 else [])


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_the_reference_shaped_reader_still_refuses_every_coded_tag(name):
    from soundkit_amd import pcm_stream
    for size in (1, 0):
        got, _, err = walk(load(name), size, pcm_stream.WavStreamProcessor)
        assert got == [] and err == "unsupported WAV format tag %d" % FIXTURES[name][0]


# ---- files built here ----------------------------------------------------------------------------------------------------------------

RNG = np.random.default_rng(7)
PCM1 = RNG.integers(-3000, 3000, (700, 1)).astype(np.int16)
PCM2 = RNG.integers(-3000, 3000, (300, 2)).astype(np.int16)
IMA36, MS41 = M.ima_encode(PCM1, 36), M.ms_encode(PCM2, 41)  # 65 frames a block mono; 29 frames a block stereo
COEF3 = [(256, 0), (300, -100), (-32768, 32767)]


def ima_fmt(ch=1, align=36, bits=4, ext=b"auto", rate=8000):
    return B.fmt_payload(0x11, ch, rate, align, bits, B.ima_ext(ch, align) if ext == b"auto" else ext)


def ms_fmt(ch=2, align=41, bits=4, coef=M.MS_COEF, ext=None, spb=None):
    return B.fmt_payload(2, ch, 8000, align, bits, B.ms_ext(ch, align, coef, spb) if ext is None else ext)


# (id, file, payload expected in the pieces, unit, error, info fields to check)
CASES = [
    ("ima, 16-byte fmt", B.wav(ima_fmt(ext=None), IMA36), IMA36, 36, None, {"frames_per_block": 65, "total_frames": 11 * 65}),
    ("ima, cbSize 0", B.wav(ima_fmt(ext=b""), IMA36), IMA36, 36, None, {"frames_per_block": 65}),
    ("ima, cbSize 2", B.wav(ima_fmt(), IMA36), IMA36, 36, None, {"frames_per_block": 65, "tag": 0x11}),
    ("ima, cbSize 2 and no field", B.wav(ima_fmt(ext=None) + struct.pack("<H", 2), IMA36), b"", 36, "WAV IMA ADPCM fmt chunk is truncated", {}),
    ("ima, wrong samples per block", B.wav(ima_fmt(ext=struct.pack("<H", 64)), IMA36), b"", 36,
     "WAV ADPCM fmt declares 64 samples per block, the block holds 65", {}),
    ("ima, header-only blocks", B.wav(ima_fmt(align=4), IMA36[:36]), IMA36[:36], 4, None, {"frames_per_block": 1, "total_frames": 9}),
    ("ima, 8 bits", B.wav(ima_fmt(bits=8), IMA36), b"", 36, "WAV ADPCM requires 4 bits per sample, found 8", {}),
    ("ima, 3 channels", B.wav(ima_fmt(ch=3, ext=b""), IMA36), b"", 36, "WAV ADPCM with 3 channels is not built: mono and stereo are", {}),
    ("ima, block of 38", B.wav(ima_fmt(align=38, ext=b""), IMA36), b"", 36, "WAV IMA ADPCM block size 38 is invalid for 1 channels", {}),
    ("ima, stereo block of 36", B.wav(ima_fmt(ch=2, align=36, ext=b""), IMA36), b"", 36, "WAV IMA ADPCM block size 36 is invalid for 2 channels", {}),
    ("ima, block of 0", B.wav(ima_fmt(align=0, ext=b""), IMA36), b"", 36, "WAV IMA ADPCM block size 0 is invalid for 1 channels", {}),
    ("ima, block too large", B.wav(ima_fmt(align=32772, ext=b""), IMA36), b"", 36, "WAV ADPCM block of 65537 samples exceeds the 65536 sample budget", {}),
    ("ima, largest block", B.wav(ima_fmt(align=32768, ext=b""), b""), b"", 36, None, {"frames_per_block": 65529, "block_align": 32768}),
    ("ima, data ends inside a block", B.wav(ima_fmt(), IMA36[:-2]), IMA36[:-36], 36, "WAV data chunk is not block-aligned", {}),
    ("ms, the standard seven", B.wav(ms_fmt(), MS41), MS41, 41, None, {"frames_per_block": 29, "coef": M.MS_COEF, "tag": 2}),
    ("ms, three sets of its own", B.wav(ms_fmt(coef=COEF3), MS41), MS41, 41, None, {"coef": COEF3}),
    ("ms, 32 sets and bytes behind them", B.wav(ms_fmt(ext=B.ms_ext(2, 41, M.MS_COEF * 4 + COEF3 + [(1, 2)]) + b"\1\2\3\4"), MS41), MS41, 41, None,
     {"coef": M.MS_COEF * 4 + COEF3 + [(1, 2)]}),
    ("ms, 33 sets", B.wav(ms_fmt(coef=M.MS_COEF * 4 + COEF3 + [(1, 2)] * 2), MS41), b"", 41, "WAV MS ADPCM fmt declares 33 coefficient sets: 1 to 32 are read", {}),
    ("ms, no sets", B.wav(ms_fmt(coef=[]), MS41), b"", 41, "WAV MS ADPCM fmt declares 0 coefficient sets: 1 to 32 are read", {}),
    ("ms, 16-byte fmt", B.wav(B.fmt_payload(2, 2, 8000, 41, 4), MS41), b"", 41, "WAV MS ADPCM fmt chunk is truncated", {}),
    ("ms, cbSize 2", B.wav(ms_fmt(ext=struct.pack("<H", 29)), MS41), b"", 41, "WAV MS ADPCM fmt chunk is truncated", {}),
    ("ms, table cut short", B.wav(ms_fmt(ext=B.ms_ext(2, 41)[:-2]), MS41), b"", 41, "WAV MS ADPCM fmt chunk is truncated", {}),
    ("ms, wrong samples per block", B.wav(ms_fmt(spb=30), MS41), b"", 41, "WAV ADPCM fmt declares 30 samples per block, the block holds 29", {}),
    ("ms, smallest blocks", B.wav(ms_fmt(ch=1, align=7), MS41[:35]), MS41[:35], 7, None, {"frames_per_block": 2, "total_frames": 10}),
    ("ms, block of 13 for two", B.wav(ms_fmt(align=13, ext=B.ms_ext(2, 14)), MS41), b"", 41, "WAV MS ADPCM block size 13 is invalid for 2 channels", {}),
    ("ms, mono block too large", B.wav(ms_fmt(ch=1, align=32775, ext=B.ms_ext(1, 7)), MS41), b"", 41,
     "WAV ADPCM block of 65538 samples exceeds the 65536 sample budget", {}),
    ("ms, largest mono block", B.wav(ms_fmt(ch=1, align=32773), b""), b"", 41, None, {"frames_per_block": 65534}),
    ("ms, 65536 samples do not fit the 16-bit field", B.wav(ms_fmt(ch=1, align=32774, spb=0), b""), b"", 41,
     "WAV ADPCM fmt declares 0 samples per block, the block holds 65536", {}),
    ("ms, largest stereo block", B.wav(ms_fmt(align=65535), b""), b"", 41, None, {"frames_per_block": 65523}),
    ("ms, 6 channels", B.wav(ms_fmt(ch=6), MS41), b"", 41, "WAV ADPCM with 6 channels is not built: mono and stereo are", {}),
    ("ms, data ends inside a block", B.wav(ms_fmt(), MS41 + b"\0" * 40), MS41, 41, "WAV data chunk is not block-aligned", {}),
    ("ulaw stereo", B.g711_wav(7, IMA36, channels=2), IMA36, 2, None, {"tag": 7, "bits": 8, "block_align": 2, "frames_per_block": 1, "total_frames": 198}),
    ("alaw, 16-byte fmt", B.wav(B.fmt_payload(6, 1, 8000, 1, 8), IMA36), IMA36, 1, None, {"tag": 6}),
    ("alaw, 16 bits", B.wav(B.fmt_payload(6, 1, 8000, 2, 16), IMA36), b"", 1, "WAV G.711 requires 8 bits per sample, found 16", {}),
    ("ulaw, 4 bits", B.wav(B.fmt_payload(7, 1, 8000, 1, 4), IMA36), b"", 1, "WAV G.711 requires 8 bits per sample, found 4", {}),
    ("ulaw stereo, odd data", B.g711_wav(7, IMA36[:-1], channels=2), IMA36[:-2], 2, "WAV data chunk is not frame-aligned", {}),
    ("zero rate", B.wav(ima_fmt(rate=0), IMA36), b"", 36, "WAV fmt contains invalid audio geometry", {}),
    ("gsm tag", B.wav(B.fmt_payload(0x31, 1, 8000, 65, 0, struct.pack("<H", 320)), IMA36), b"", 1, "unsupported WAV format tag 49", {}),
    ("g726 tag", B.wav(B.fmt_payload(0x45, 1, 8000, 1, 4, b""), IMA36), b"", 1, "unsupported WAV format tag 69", {}),
    ("mp3 tag", B.wav(B.fmt_payload(0x55, 1, 8000, 1, 0, b""), IMA36), b"", 1, "unsupported WAV format tag 85", {}),
    ("extensible around ima", B.wav(B.fmt_payload(0xfffe, 1, 8000, 36, 4, struct.pack("<HIH", 4, 0, 0x11) + bytes(14)), IMA36), b"", 1, "unsupported WAV format tag 17", {}),
    ("fact in front of data", B.wav(ima_fmt(), IMA36, fact=700), IMA36, 36, None, {"fact_frames": 700, "total_frames": 700}),
    ("fact on a block edge", B.wav(ima_fmt(), IMA36, fact=650), IMA36, 36, None, {"fact_frames": 650, "total_frames": 650}),
    ("fact of zero", B.wav(ima_fmt(), IMA36, fact=0), IMA36, 36, None, {"fact_frames": 0, "total_frames": 715}),
    ("fact larger than the blocks", B.wav(ima_fmt(), IMA36, fact=716), IMA36, 36, None, {"fact_frames": 716, "total_frames": 715}),
    ("fact of exactly the blocks", B.wav(ima_fmt(), IMA36, fact=715), IMA36, 36, None, {"total_frames": 715}),
    ("no fact", B.wav(ima_fmt(), IMA36), IMA36, 36, None, {"fact_frames": 0, "total_frames": 715}),
    ("fact behind data", B.wav(ima_fmt(), IMA36, after_data=[(b"fact", struct.pack("<I", 5))]), IMA36, 36, None, {"fact_frames": 0, "total_frames": 715}),
    ("fact of 2 bytes", B.wav(ima_fmt(), IMA36, before_data=[(b"fact", b"\5\0")]), IMA36, 36, None, {"fact_frames": 0, "total_frames": 715}),
    ("fact of 4097 bytes", B.wav(ima_fmt(), IMA36, before_data=[(b"fact", bytes(4097))]), b"", 36, "WAV fmt chunk exceeds the 4096 byte metadata budget", {}),
    ("fact for ms", B.wav(ms_fmt(), MS41, fact=300), MS41, 41, None, {"fact_frames": 300, "total_frames": 300}),
    ("fact leaves g711 alone", B.g711_wav(7, IMA36, fact=5), IMA36, 1, None, {"fact_frames": 5, "total_frames": 396}),
    ("RF64", B.wav(ms_fmt(), MS41, fact=300, rf64=True), MS41, 41, None, {"total_frames": 300, "tag": 2}),
    ("RF64, ima", B.wav(ima_fmt(), IMA36, rf64=True), IMA36, 36, None, {"total_frames": 715}),
    ("an odd chunk in front", B.wav(ima_fmt(), IMA36, before_fmt=[(b"LIST", b"abc")], before_data=[(b"junk", bytes(5001))]), IMA36, 36, None, {"total_frames": 715}),
    ("data before fmt", B.wav(ima_fmt(), IMA36)[:12] + b"data\4\0\0\0abcd", b"", 1, "WAV data appears before a valid fmt chunk", {}),
    ("bytes behind the data chunk", B.wav(ima_fmt(), IMA36, after_data=[(b"LIST", b"xyz")]) + b"tail", IMA36, 36, None, {}),
]


@pytest.mark.parametrize("name,file,want,unit,error,fields", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("size", [1, 7, 0])
def test_files_built_here(name, file, want, unit, error, fields, size):
    got, info, err = walk(file, size)
    assert err == error
    if err is None or want:
        check_pieces(got, want, file.index(b"data", 12 + 8) + 8 if want else 0, unit)
    for k, v in fields.items():
        assert info[k] == v, (k, info[k])


def test_pcm_and_float_files_walk_as_in_the_reference_shaped_reader():
    """tags 1, 3 and 0xFFFE: the same pieces, the same description, the same texts from both readers"""
    from soundkit_amd import pcm_stream
    files = [open(os.path.join(GOLD, n), "rb").read()[:20000] for n in ("wav_24_A_Tusk.wav",)]
    pcm = bytes(range(240))
    files += [B.wav(B.fmt_payload(1, 2, 44100, 4, 16), pcm), B.wav(B.fmt_payload(3, 1, 48000, 4, 32, b""), pcm, fact=60),
              B.wav(B.fmt_payload(0xfffe, 2, 48000, 6, 24, struct.pack("<HIH", 24, 3, 1) + bytes(14)), pcm, rf64=True),
              B.wav(B.fmt_payload(1, 2, 44100, 4, 16), pcm[:-1]), B.wav(B.fmt_payload(1, 1, 8000, 1, 12), pcm), B.wav(B.fmt_payload(1, 0, 8000, 1, 8), pcm)]
    for file in files:
        for size in (1, 7, 0):
            a, b = walk(file, size), walk(file, size, pcm_stream.WavStreamProcessor)
            assert a[0] == b[0] and a[2] == b[2]
            if a[2] is None:
                assert all(a[1][k] == b[1][k] for k in ("sample_rate", "channels", "bits", "is_float", "total_frames"))
                assert a[1]["tag"] == (3 if a[1]["is_float"] else 1) and a[1]["frames_per_block"] == 1 and a[1]["block_align"] == a[1]["bits"] // 8 * a[1]["channels"]


def test_the_new_symbols_are_declared_and_exported():
    import soundkit_amd
    names = ["sk_wav_coded_reader_create", "sk_wav_coded_reader_destroy", "sk_wav_coded_reader_add", "sk_wav_coded_reader_info",
             "sk_wav_coded_reader_last_error", "sk_wav_adpcm_decode", "sk_wav_adpcm_decode_dev", "sk_tick_run_wav_adpcm",
             "sk_tick_wav_adpcm_out_bound_on"]
    declared = soundkit_amd.declared_symbols()
    for n in names:
        assert n in declared and hasattr(soundkit_amd.lib, n), n


# ---- what pins the models --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("law", ["ulaw", "alaw"])
def test_g711_fixtures_expand_to_the_references_recordings(law):
    """independent of anything written for the coded walker: the payload is the reference's, so is the recording"""
    payload = B.data_of(load(law + "_A_Tusk.wav"))
    with wave.open(os.path.join(GOLD, "aiff", "g711_%s.decoded.wav" % law)) as w:
        want = np.frombuffer(w.readframes(w.getnframes()), "<i2")
    assert np.array_equal(g72x_model.g711_decode(payload, g72x_model.ULAW if law == "ulaw" else g72x_model.ALAW), want)


def random_ima_blocks(rng, n):
    blocks = rng.integers(0, 256, (n, 256), dtype=np.uint8)
    blocks[:, 2] = rng.integers(0, 89, n)
    for k in range(0, n, 5):  # saturating ones: a rail, the largest step, every nibble the largest move toward the rail
        blocks[k, :2] = np.frombuffer((32767 if k & 1 else -32768).to_bytes(2, "little", signed=True), np.uint8)
        blocks[k, 2], blocks[k, 4:] = 88, 0x77 if k & 1 else 0xff
    return blocks


def test_ima_model_equals_audioop():
    pytest.importorskip("audioop")
    blocks = random_ima_blocks(np.random.default_rng(3), 300)
    got, status = M.ima_decode(blocks.tobytes(), 1, 256)
    assert not any(status)
    for k, blk in enumerate(blocks):
        assert np.array_equal(got[k, 1:, 0], B.audioop_ima_mono_block(blk.tobytes())), k
        assert got[k, 0, 0] == int.from_bytes(blk[:2].tobytes(), "little", signed=True)


def test_ima_model_equals_the_recorded_audioop_output():
    """the same pin where the module is absent: audioop's output for the first blocks of ima_mono_8k.wav, recorded with the fixtures"""
    blocks = B.data_of(load("ima_mono_8k.wav"))[:256 * B.AUDIOOP_BLOCKS]
    want = np.frombuffer(load("ima_mono_8k.audioop.s16le"), "<i2").reshape(B.AUDIOOP_BLOCKS, 504)
    got, _ = M.ima_decode(blocks, 1, 256)
    assert np.array_equal(got[:, 1:, 0], want)
    for k in range(B.AUDIOOP_BLOCKS):
        assert np.array_equal(np.array(M.ima_decode_block(blocks[256 * k:256 * k + 256], 1))[1:, 0], want[k])


def ms_block(pred, delta, s1, s2, nibbles):
    return bytes([pred]) + struct.pack("<hhh", delta, s1, s2) + bytes((a << 4) | b for a, b in zip(nibbles[0::2], nibbles[1::2]))


def test_ms_known_answer_blocks():
    """Worked by hand from the rules; no independent Microsoft ADPCM decoder exists here to run instead.

    Block A, set 3 = (192, 64), iDelta 16, iSamp1 -101, iSamp2 10, nibbles 3 F 8 7:
      out: 10, -101
      n=3 (+3): -101*192 + 10*64 = -18752; / 256 = -73.25 -> -73 (a floor would give -74); -73 + 3*16 = -25; delta 230*16/256 = 14 -> 16
      n=F (-1): -25*192 + -101*64 = -11264; / 256 = -44; -44 - 16 = -60; delta 230*16/256 = 14 -> 16 (the floor again)
      n=8 (-8): -60*192 + -25*64 = -13120; / 256 = -51.25 -> -51 (floor: -52); -51 - 128 = -179; delta 768*16/256 = 48
      n=7 (+7): -179*192 + -60*64 = -38208; / 256 = -149.25 -> -149 (floor: -150); -149 + 7*48 = 187; delta 614*48/256 = 115
    Block B, set 0 = (256, 0), iDelta 2000, iSamp1 32000, iSamp2 0, nibbles 7 8 8 0:
      n=7: 32000 + 14000 -> 32767 (clamped); delta 614*2000/256 = 4796
      n=8: 32767 - 8*4796 = -5601; delta 768*4796/256 = 14388
      n=8: -5601 - 8*14388 -> -32768 (clamped); delta 43164
      n=0: -32768 + 0 = -32768"""
    a, b = ms_block(3, 16, -101, 10, [3, 15, 8, 7]), ms_block(0, 2000, 32000, 0, [7, 8, 8, 0])
    want_a, want_b = [10, -101, -25, -60, -179, 187], [0, 32000, 32767, -5601, -32768, -32768]
    assert [f[0] for f in M.ms_decode_block(a, 1, M.MS_COEF)] == want_a
    assert [f[0] for f in M.ms_decode_block(b, 1, M.MS_COEF)] == want_b
    got, status = M.decode(M.TAG_MS, 1, 9, a + b, M.MS_COEF)
    assert status == [0, 0] and got.tolist() == want_a + want_b
    # the two as one stereo block: left = A, right = B
    st = bytes([3, 0]) + struct.pack("<hhhhhh", 16, 2000, -101, 32000, 10, 0) + bytes([0x37, 0xf8, 0x88, 0x70])
    got, status = M.decode(M.TAG_MS, 2, 18, st, M.MS_COEF)
    assert status == [0] and got.reshape(-1, 2).T.tolist() == [want_a, want_b]


def test_the_two_forms_of_each_model_agree():
    rng = np.random.default_rng(1)
    for tag, ch, align in ((0x11, 1, 36), (0x11, 2, 64), (0x11, 2, 8), (2, 1, 40), (2, 2, 41), (2, 1, 7)):
        blocks = rng.integers(0, 256, (60, align), dtype=np.uint8)
        if tag == 2:
            blocks[:, :ch] %= 9  # some at or past the seven sets
        else:
            for c in range(ch):
                blocks[:, 4 * c + 2] %= 92  # some above 88
        got, status = M.decode(tag, ch, align, blocks.tobytes(), M.MS_COEF)
        got = got.reshape(60, -1, ch)
        assert 0 < sum(1 for s in status if s) < 60
        for k, blk in enumerate(blocks):
            want = M.ima_decode_block(blk.tobytes(), ch) if tag == 0x11 else M.ms_decode_block(blk.tobytes(), ch, M.MS_COEF)
            if want is None:
                assert status[k] == M.BAD_BLOCK and not got[k].any()
            else:
                assert status[k] == 0 and got[k].tolist() == want


@pytest.mark.parametrize("name", sorted(SNR_DB))
def test_adpcm_fixtures_decode_to_their_recordings_and_track_the_speech(name):
    """the builder's round trip: what the model decodes is the recording, and the recording follows the 8 kHz speech it was encoded from"""
    got = B.model_decode_file(load(name))
    assert got.astype("<i2").tobytes() == load(name[:-4] + ".decoded.s16le")
    sp = speech()
    src = sp[4000:7000] if FIXTURES[name][1] == 1 else np.stack([sp[4000:6500], sp[9000:11500]], 1).reshape(-1)
    err = src.astype(np.float64) - got
    snr = 10 * np.log10((src.astype(np.float64) ** 2).sum() / (err ** 2).sum())
    print("%s: SNR %.3f dB" % (name, snr))
    assert abs(snr - SNR_DB[name]) < 0.01


# ---- sanitizer harness -----------------------------------------------------------------------------------------------------------------

def test_walker_under_the_sanitizers(tmp_path):
    """tests/fuzz_wav_coded.cpp: seeded mutations of the fixtures' headers in ragged pieces -- no crash, no sanitizer report, every
    piece whole units in order; a program of its own, nothing is loaded into this process"""
    exe = str(tmp_path / "fuzz_wav_coded")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(HERE, "fuzz_wav_coded.cpp")], cwd=HERE)
    out = subprocess.check_output([exe, "300"] + [os.path.join(DIR, n) for n in sorted(FIXTURES)], text=True)
    ok_n, err_n = int(out.split()[1]), int(out.split()[3])
    assert ok_n + err_n == 300 * len(FIXTURES) and ok_n >= len(FIXTURES) and err_n > 0, out

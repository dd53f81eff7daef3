"""The host side of the scheduler's WAV / raw PCM streams, without a GPU: the WAV walker and the raw PCM framer
(csrc/pcm_stream.h through sk_wav_reader_* / sk_raw_pcm_framer_*) against the reference's twin recordings, headers built here, and
tests/pcm_worker_model.py -- and that model by itself against the outside world, so that the GPU tests compare with something pinned."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pcm_worker_model as M
import twin_fit

HERE = os.path.dirname(os.path.abspath(__file__))
WAVS = {"wav_stereo_A_Tusk.wav": (16000, 2, 16, False), "wav_24_A_Tusk.wav": (16000, 1, 24, False), "wav_32f_A_Tusk.wav": (16000, 1, 32, True)}


def reader():
    from soundkit_amd import pcm_stream
    return pcm_stream.WavStreamProcessor()


def chunk_walk(data):
    """an independent walk of the file's chunks: (fmt payload, offset and length of the data chunk's bytes)"""
    pos, fmt, where = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        if cid == b"fmt ":
            fmt = data[pos + 8:pos + 8 + size]
        elif cid == b"data":
            where = (pos + 8, min(size, len(data) - pos - 8))
            break
        pos += 8 + size + (size & 1)
    return fmt, where


def pieces_of(rd, chunks):
    out = []
    for c in chunks:
        got = rd.add(c)
        if got:
            out.append(got)
    return out


@pytest.mark.parametrize("name", sorted(WAVS))
@pytest.mark.parametrize("size", [1, 7, 4096, 0])
def test_wav_fixtures_through_the_reader(name, size):
    data = open(twin_fit.golden(name), "rb").read()
    rate, ch, bits, is_float = WAVS[name]
    fmt, (off, length) = chunk_walk(data)
    chunks = [data[i:i + size] for i in range(0, len(data), size)] if size else [data]
    rd = reader()
    got = pieces_of(rd, chunks)
    info = rd.info()
    assert (info["sample_rate"], info["channels"], info["bits"], info["is_float"]) == (rate, ch, bits, is_float)
    assert info["total_frames"] == length // (bits // 8 * ch)
    tag = struct.unpack("<H", fmt[:2])[0]
    if name != "wav_stereo_A_Tusk.wav":  # both are WAVE_FORMAT_EXTENSIBLE: the tag comes from the sub-format
        assert tag == 0xfffe and len(fmt) >= 40 and struct.unpack("<H", fmt[24:26])[0] == (3 if is_float else 1)
    # the pieces, end to end, are the data chunk; each lies where it says and is whole frames
    assert got[0][0] == off and b"".join(p for _, p in got) == data[off:off + length]
    at = off
    for o, p in got:
        assert o == at and len(p) % (bits // 8 * ch) == 0 and data[o:o + len(p)] == p
        at += len(p)
    # and the boundaries are the model's (one add per chunk here: the walker alone, without the worker's detection gathering)
    wav = M.WavModel()
    want = [p for p in (wav.add(c) for c in chunks) if p]
    assert [len(p) for _, p in got] == [len(p) for p in want]
    assert (wav.rate, wav.channels, wav.bits, wav.is_float, wav.total_frames()) == (rate, ch, bits, is_float, info["total_frames"])


def fmt_chunk(tag=1, channels=1, rate=8000, bits=16, size=16, ext_tag=None):
    body = struct.pack("<HHIIHH", tag, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    if ext_tag is not None:
        body += struct.pack("<HHIH", 22, bits, 0, ext_tag) + b"\x00" * 14
    body = body[:size] + b"\x00" * max(0, size - len(body))
    return b"fmt " + struct.pack("<I", size) + body + (b"\x00" if size & 1 else b"")


def riff(*chunks, magic=b"RIFF"):
    body = b"WAVE" + b"".join(chunks)
    return magic + struct.pack("<I", len(body) & 0xffffffff) + body


def data_chunk(payload, size=None):
    return b"data" + struct.pack("<I", len(payload) if size is None else size) + payload


PCM = bytes(range(64))
DS64 = b"ds64" + struct.pack("<IQQQI", 28, 0, 40, 20, 0)
CASES = [
    # name, stream, expected pieces joined (None: not checked), error or None
    ("odd chunk with pad byte", riff(fmt_chunk(), b"LIST" + struct.pack("<I", 3) + b"abc\x00", data_chunk(PCM)), PCM, None),
    ("odd fmt chunk with pad byte", riff(fmt_chunk(size=17), data_chunk(PCM)), PCM, None),
    ("data before fmt", riff(data_chunk(PCM), fmt_chunk()), b"", "WAV data appears before a valid fmt chunk"),
    ("fmt of 4097 bytes", riff(fmt_chunk(size=4097), data_chunk(PCM)), b"", "WAV fmt chunk exceeds the 4096 byte metadata budget"),
    ("fmt of 4096 bytes", riff(fmt_chunk(size=4096), data_chunk(PCM)), PCM, None),
    ("fmt of 14 bytes", riff(fmt_chunk(size=14), data_chunk(PCM)), b"", "WAV fmt chunk must contain at least 16 bytes"),
    ("tag 2", riff(fmt_chunk(tag=2), data_chunk(PCM)), b"", "unsupported WAV format tag 2"),
    ("extensible, sub-format 3", riff(fmt_chunk(tag=0xfffe, bits=32, size=40, ext_tag=3), data_chunk(PCM)), PCM, None),
    ("extensible, sub-format 2", riff(fmt_chunk(tag=0xfffe, size=40, ext_tag=2), data_chunk(PCM)), b"", "unsupported WAV format tag 2"),
    ("extensible, truncated", riff(fmt_chunk(tag=0xfffe, size=24), data_chunk(PCM)), b"", "WAVE_FORMAT_EXTENSIBLE fmt chunk is truncated"),
    ("zero channels", riff(fmt_chunk(channels=0), data_chunk(PCM)), b"", "WAV fmt contains invalid audio geometry"),
    ("12-bit width", riff(fmt_chunk(bits=12), data_chunk(PCM)), b"", "WAV sample width must be byte-aligned"),
    ("RF64 with ds64", riff(DS64, fmt_chunk(), data_chunk(PCM[:40], 0xffffffff), magic=b"RF64"), PCM[:40], None),
    ("RF64 without ds64", riff(fmt_chunk(), data_chunk(PCM, 0xffffffff), magic=b"RF64"), b"", "RF64 data chunk appears before a valid ds64 chunk"),
    ("ds64 in a RIFF file", riff(DS64, fmt_chunk(), data_chunk(PCM)), b"", "ds64 chunk requires an RF64 header"),
    ("short data at end of stream", riff(fmt_chunk(), data_chunk(PCM, 1000)), PCM, None),
    ("unaligned data tail", riff(fmt_chunk(channels=2), data_chunk(PCM[:63])), PCM[:60], "WAV data chunk is not frame-aligned"),
    ("a chunk behind data", riff(fmt_chunk(), data_chunk(PCM), b"LIST" + struct.pack("<I", 4) + b"abcd", data_chunk(PCM)), PCM, None),
    ("not a WAV file", b"RIFF\x00\x00\x00\x00WAVX" + b"\x00" * 32, b"", "Not a WAV file"),
]


@pytest.mark.parametrize("name,stream,want,error", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("size", [1, 5, 0])
def test_wav_headers_built_here(name, stream, want, error, size):
    chunks = [stream[i:i + size] for i in range(0, len(stream), size)] if size else [stream]
    for make in (reader, M.WavModel):  # the library and the model agree with the expectation, so with each other
        rd, got, err = make(), [], None
        try:
            for c in chunks:
                p = rd.add(c)
                if p:
                    got.append(p if isinstance(p, bytes) else p[1])
        except ValueError as e:
            err = str(e)
        if name == "unaligned data tail" and size == 0:
            # one add returns the whole frames; the three bytes left are looked at by the NEXT add (wav.rs:226-231), which a
            # stream that arrives in one chunk never makes
            assert err is None and b"".join(got) == want
            with pytest.raises(ValueError, match=error):
                rd.add(b"")
            continue
        assert err == error, (make, err)
        assert b"".join(got) == want, make
        if err is not None:  # a rejected stream stays rejected quietly: the processor is finished
            assert rd.add(b"\x00" * 16) is None


def test_wav_input_chunk_limit():
    rd = reader()
    with pytest.raises(ValueError, match="WAV input chunk exceeds the 4194304 byte streaming budget"):
        rd.add(b"\x00" * (4 * 1024 * 1024 + 1))


def test_raw_pcm_framing():
    from soundkit_amd import pcm_stream
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, 6 * 1000 + 5, dtype=np.uint8).tobytes()
    for frame in (1, 2, 4, 6, 8):
        fr, model = pcm_stream.RawPcmStreamProcessor(frame), M.RawModel(frame)
        got, want, at = [], [], 0
        for c in M.ragged(data, rng, 1, 40):
            p, w = fr.add(c), model.add(c)
            assert (p is None) == (w is None)
            if p:
                assert p[0] == at and p[1] == w and len(w) % frame == 0
                at += len(w)
                got.append(p[1])
        assert b"".join(got) == data[:len(data) // frame * frame]
        left = len(data) % frame
        if left:
            with pytest.raises(ValueError, match=re.escape("Raw PCM stream ended with %d trailing partial-frame byte(s)" % left)):
                fr.flush()
            with pytest.raises(ValueError):
                model.flush()
        else:
            fr.flush(), model.flush()


# ---- the model by itself against the outside world ----------------------------------------------------------------------------

def joined(outs):
    return b"".join(o[5] for o in outs)


def test_model_depth_reduction_equals_the_16_bit_twin(oracle):
    """wav_24 and linear32 -> 16 bit are the 16-bit recording bit for bit (exact_signed_pcm_to_i16)"""
    rng = np.random.default_rng(11)
    want = open(twin_fit.golden("linear16_A_Tusk.s16le"), "rb").read()
    wav = open(twin_fit.golden("wav_24_A_Tusk.wav"), "rb").read()
    outs, err = M.wav_worker(oracle, M.ragged(wav, rng, 1, 30000), out_bits=16)
    assert err is None and joined(outs) == want and all(o[:5] == (16, 1, 16000, False, False) for o in outs)
    s32 = open(twin_fit.golden("linear32_A_Tusk.s32le"), "rb").read()
    outs, err = M.raw_worker(oracle, M.ragged(s32, rng, 1, 30000), 16000, 1, M.FMT_S32LE, out_bits=16)
    assert err is None and joined(outs) == want


@pytest.mark.parametrize("in_hz,out_hz", twin_fit.PAIRS)
def test_model_resampled_twins(oracle, in_hz, out_hz):
    """the twin pairs fed in seeded ragged pieces through the model's streaming chain meet the pins of tests/twin_fit.py"""
    rng = np.random.default_rng(in_hz + out_hz)
    data = open(twin_fit.golden(twin_fit.TWIN_FILES[in_hz]), "rb").read()
    outs, err = M.raw_worker(oracle, M.ragged(data, rng, 1, 50000), in_hz, 1, M.FMT_S16LE, out_bits=16, out_rate=out_hz)
    assert err is None and all(o[:5] == (16, 1, out_hz, False, False) for o in outs)
    y = np.frombuffer(joined(outs), "<i2").astype(np.float64) / 32768.0
    twin_fit.assert_twin(y, in_hz, out_hz, kind="s16", label="worker model, ragged pieces")


def test_model_detection_gathering():
    """the worker's first `process` is the gathered detection buffer (at least 8192 bytes unless the stream ends, at most 65536),
    the rest of the chunk that completed it a second one"""
    data = open(twin_fit.golden("wav_24_A_Tusk.wav"), "rb").read()
    _, pieces, err = M.wav_pieces([data[:100], data[100:5000], data[5000:100000], data[100000:]])
    assert err is None
    head = 102  # the data chunk's offset in this file
    assert [len(p) for p in pieces] == [(65536 - head) // 3 * 3, (100000 - 65536 + (65536 - head) % 3) // 3 * 3,
                                        len(data) - head - (65536 - head) // 3 * 3 - (100000 - 65536 + (65536 - head) % 3) // 3 * 3]
    _, pieces, err = M.wav_pieces([data[:2000], data[2000:4000]])  # the stream ends while detecting: one process
    assert err is None and [len(p) for p in pieces] == [(4000 - head) // 3 * 3]


# ---- sanitizer harness --------------------------------------------------------------------------------------------------------

def test_mutated_headers_under_sanitizers(tmp_path):
    """tests/fuzz_pcm_stream.cpp: seeded mutations of the fixtures' first 256 bytes in ragged pieces -- no crash, no sanitizer
    report, every piece whole frames inside the input"""
    exe = str(tmp_path / "fuzz_pcm_stream")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(HERE, "fuzz_pcm_stream.cpp")], cwd=HERE)
    out = subprocess.run([exe, "4000"] + [twin_fit.golden(n) for n in sorted(WAVS)], capture_output=True, text=True, cwd=HERE)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-2000:])
    ok, err = [int(x) for x in re.findall(r"ok (\d+) err (\d+)", out.stdout)[0]]
    assert ok > 0 and err > 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr

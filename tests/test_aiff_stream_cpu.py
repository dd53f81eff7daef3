"""AIFF / AIFF-C on the host (no GPU): the model of the reference's decoder (tests/aiff_model.py) against the outside world -- the
reference's nine encodings of one clip, whose payloads relate exactly to the 8 kHz twin and to the reference's decoded G.711 files --
and the container walker (csrc/pcm_stream.h through sk_aiff_reader_*) against the model: pieces, description, error texts, and the
bound on what it holds back.  tests/fuzz_aiff_stream.cpp runs the walker under the sanitizers as a program of its own."""
import os
import struct
import subprocess

import numpy as np
import pytest

import aiff_builder as B
import aiff_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
AIFF = os.path.join(GOLD, "aiff")
CLIP = "A_Tusk_is_used_to_make_costly_gifts"
FIXTURES = [CLIP + ".aiff", CLIP + ".aifc"] + ["stream-%s.aifc" % n for n in ("alaw", "ulaw", "ima4", "f32be", "f64be", "s24be", "s32be")]
ENCODING = {CLIP + ".aiff": M.S16BE, CLIP + ".aifc": M.S16LE, "stream-alaw.aifc": M.ALAW, "stream-ulaw.aifc": M.ULAW, "stream-ima4.aifc": M.IMA4,
            "stream-f32be.aifc": M.F32BE, "stream-f64be.aifc": M.F64BE, "stream-s24be.aifc": M.S24BE, "stream-s32be.aifc": M.S32BE}
# IMA4 against the twin, measured with the model (tests/golden/aiff/README.md): the QuickTime carry rule, and every packet from its header
IMA4_SNR_DB, IMA4_SNR_NO_CARRY_DB = 21.354, 10.629
IMA4_FLOOR_DB = IMA4_SNR_DB - 1.0


def load(name):
    return open(os.path.join(AIFF, name), "rb").read()


def twin():
    return np.fromfile(os.path.join(GOLD, "linear16_8k_A_Tusk.s16le"), "<i2")


def wav_payload(name):
    data = load(name)
    at = data.index(b"data")
    n = struct.unpack("<I", data[at + 4:at + 8])[0]
    return data[at + 8:at + 8 + n]


def model_decode(name, piece=None, carry=True):
    outs, m = M.decode_file(load(name), piece, carry)
    assert outs
    a = outs[0]
    assert all((o.sample_rate, o.channels, o.bits, o.is_float) == (a.sample_rate, a.channels, a.bits, a.is_float) for o in outs)
    return a, b"".join(o.data for o in outs), m


def snr_db(ref, got):
    ref, got = ref.astype(np.float64), got.astype(np.float64)
    return 10 * np.log10(np.sum(ref ** 2) / np.sum((ref - got) ** 2))


# ---- the model against the outside world ------------------------------------------------------------------------------------------

def test_model_linear_fixtures_equal_the_twin():
    t = twin()
    for name, bits, fl in [(CLIP + ".aiff", 16, False), (CLIP + ".aifc", 16, False), ("stream-s24be.aifc", 24, False), ("stream-s32be.aifc", 32, False),
                           ("stream-f32be.aifc", 32, True), ("stream-f64be.aifc", 32, True)]:
        a, data, _ = model_decode(name)
        assert (a.sample_rate, a.channels, a.bits, a.is_float) == (8000, 1, bits, fl), name
        if fl:
            got = np.frombuffer(data, "<f4").astype(np.float64) * 32768.0
        elif bits == 24:
            raw = np.frombuffer(data, np.uint8).reshape(-1, 3).astype(np.int32)
            v = raw[:, 0] | (raw[:, 1] << 8) | (raw[:, 2] << 16)
            got = ((v ^ 0x800000) - 0x800000)
            assert np.array_equal(got, t.astype(np.int32) << 8), name
            continue
        elif bits == 32:
            assert np.array_equal(np.frombuffer(data, "<i4"), t.astype(np.int32) << 16), name
            continue
        else:
            got = np.frombuffer(data, "<i2")
        assert np.array_equal(got, t), name


def test_f64_fixture_values_are_f32_values():
    m = M.AiffModel()
    m.add(load("stream-f64be.aifc"))
    v = np.frombuffer(m.pieces[0], ">f8")
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)


def test_model_g711_fixtures_equal_the_reference_decodes():
    for law in ("ulaw", "alaw"):
        a, data, _ = model_decode("stream-%s.aifc" % law)
        assert (a.sample_rate, a.channels, a.bits, a.is_float) == (8000, 1, 16, False)
        assert data == wav_payload("g711_%s.decoded.wav" % law), law


def test_model_ima4_carry_rule_is_visible_in_the_fixture():
    t = twin()
    a, data, m = model_decode("stream-ima4.aifc")
    assert (a.sample_rate, a.channels, a.bits) == (8000, 1, 16) and len(m.pieces[0]) == 370 * 34 and len(data) == 23680 * 2
    got = np.frombuffer(data, "<i2")
    n = min(len(got), len(t))
    with_carry = snr_db(t[:n], got[:n])
    _, data2, _ = model_decode("stream-ima4.aifc", carry=False)
    without = snr_db(t[:n], np.frombuffer(data2, "<i2")[:n])
    print("IMA4 SNR against the twin: carry %.3f dB, every packet from its header %.3f dB" % (with_carry, without))
    assert abs(with_carry - IMA4_SNR_DB) < 0.001 and abs(without - IMA4_SNR_NO_CARRY_DB) < 0.001
    assert with_carry >= IMA4_FLOOR_DB > without


def test_model_pieces_do_not_change_the_decode():
    for name in FIXTURES:
        _, whole, _ = model_decode(name)
        for piece in (113, 997):
            assert model_decode(name, piece)[1] == whole, (name, piece)


# ---- sk_aiff_reader_* against the model ---------------------------------------------------------------------------------------------

def walk_both(data, piece):
    """-> list of per-add results of the reader, after asserting that the model did the same at every add"""
    from soundkit_amd import pcm_stream
    r, m = pcm_stream.AiffReader(), M.AiffModel()
    step = piece or max(len(data), 1)
    chunks = [data[at:at + step] for at in range(0, len(data), step)] + [b""]
    got, offset = [], 0
    try:
        for c in chunks:
            n_before = len(m.pieces)
            want_err = None
            try:
                audio = m.add(c)
            except ValueError as exc:
                want_err, audio = str(exc), None
            if want_err is not None:
                with pytest.raises(ValueError) as ei:
                    r.add(c)
                assert str(ei.value) == want_err
                got.append(("error", want_err))
                return got
            res = r.add(c)
            if audio is None:
                assert res is None
            else:
                assert len(m.pieces) == n_before + 1
                assert res == (offset, m.pieces[-1])
                offset += len(m.pieces[-1])
                i = r.info()
                assert (i["sample_rate"], i["channels"], i["bits"], i["is_float"]) == (audio.sample_rate, audio.channels, audio.bits, audio.is_float)
                assert i["encoding"] == m.info[2]
                assert len(audio.data) * M.group_bytes(i["encoding"], i["channels"]) == len(res[1]) * (
                    128 * i["channels"] if i["encoding"] == M.IMA4 else i["bits"] // 8)
            assert r.buffered_bytes() == m.buffered_bytes()
            assert r.buffered_bytes() < 4096 + max(step, 257) if piece else True
            got.append(res)
        return got
    finally:
        r.close()


@pytest.mark.parametrize("piece", [113, 257, 641, 997, None])
@pytest.mark.parametrize("name", FIXTURES)
def test_reader_matches_model_on_fixtures(name, piece):
    got = walk_both(load(name), piece)
    assert got[-1] is None or got[-1][0] != "error"
    pieces = [g for g in got if g is not None]
    assert pieces and (piece is not None or len(pieces) == 1)
    from soundkit_amd import pcm_stream
    r = pcm_stream.AiffReader()
    r.add(load(name)[:4096])
    assert r.info()["encoding"] == ENCODING[name]
    r.close()


def test_reader_holds_back_less_than_4096_plus_the_chunk():
    from soundkit_amd import pcm_stream
    for name in FIXTURES:
        r = pcm_stream.AiffReader()
        data = load(name)
        for at in range(0, len(data), 257):
            r.add(data[at:at + 257])
            assert r.buffered_bytes() < 4096 + 257
        r.close()


def error_of(data, piece=None):
    got = walk_both(data, piece)
    assert got[-1] is not None and got[-1][0] == "error", got[-1]
    return got[-1][1]


def ok(data, piece=None):
    got = walk_both(data, piece)
    assert not (got[-1] is not None and got[-1][0] == "error"), got[-1]
    return b"".join(g[1] for g in got if g is not None)


S16 = bytes(range(64))


def test_odd_chunks_unknown_chunks_and_ssnd_offset():
    name = B.chunk(b"NAME", b"odd")  # 3 bytes + pad
    anno = B.chunk(b"ANNO", b"x" * 21)
    for piece in (None, 1, 3, 7):
        data = B.form([name, B.comm(2, 16, 16, 44100.0), anno, B.chunk(b"MARK", b""), B.ssnd(S16, offset=5), B.chunk(b"(c) ", b"odd too.")])
        assert ok(data, piece) == S16
    # an odd COMM (AIFF-C with an even-length name: 23 bytes) and an odd SSND
    data = B.form([B.fver(), B.chunk(b"COMM", struct.pack(">HIH", 1, 3, 8) + B.extended(8000.0) + b"raw " + b"\0"), B.ssnd(b"abc")], aifc=True)
    assert ok(data, 2) == b"abc"
    # two SSND chunks: both are sound
    data = B.form([B.comm(1, 4, 16, 8000.0), B.ssnd(S16[:8]), B.chunk(b"NAME", b"n"), B.ssnd(S16[8:16])])
    assert ok(data) == S16[:16] and ok(data, 5) == S16[:16]


def test_structure_errors():
    comm = B.comm(1, 4, 16, 8000.0)
    assert error_of(B.form([B.ssnd(S16), comm])) == "AIFF SSND appears before COMM"
    assert error_of(B.form([comm, B.chunk(b"SSND", S16, declared=1000)])) == "AIFF chunk SSND exceeds the FORM boundary"
    assert error_of(B.form([comm, B.chunk(b"\xff\xfeX ", b"", declared=77)])) == "AIFF chunk ��X  exceeds the FORM boundary"
    body = B.form([comm, B.ssnd(S16)])
    assert error_of(B.form([comm, B.ssnd(S16)], size=len(body) - 8 + 5) + b"12345") == "AIFF FORM ends inside a chunk header"
    assert error_of(body + b"x") == "AIFF stream has bytes after the FORM boundary"
    assert error_of(body + b"x", 7) == "AIFF stream has bytes after the FORM boundary"
    assert error_of(b"RIFF" + body[4:]) == "AIFF stream does not start with FORM"
    assert error_of(B.form([], size=3)) == "AIFF FORM is shorter than its type field"
    assert error_of(B.form([comm], kind=b"8SVX")) == "unsupported FORM type 8SVX"
    assert error_of(B.form([comm], kind=b"A\xc3\x28F")) == "unsupported FORM type A�(F"
    assert error_of(B.form([comm, B.chunk(b"SSND", b"1234")])) == "AIFF SSND is shorter than its header"
    assert error_of(B.form([comm, B.chunk(b"SSND", struct.pack(">II", 9, 0) + b"12345678")])) == "AIFF SSND offset exceeds its chunk"
    assert error_of(B.form([B.comm(1, 4, 16, 8000.0), B.ssnd(S16[:7])])) == "AIFF SSND ends inside an encoded sample group"
    ima = B.form([B.fver(), B.comm(2, 64, 16, 8000.0, b"ima4"), B.ssnd(bytes(68 + 34))], aifc=True)
    assert error_of(ima) == "AIFF SSND ends inside an encoded sample group" and error_of(ima, 11) == "AIFF SSND ends inside an encoded sample group"
    assert ok(B.form([], size=4)) == b""  # an empty FORM is a finished stream without sound


def test_truncation_in_each_state():
    comm = B.comm(1, 32, 16, 8000.0)
    full = B.form([B.chunk(b"NAME", b"abc"), comm, B.ssnd(S16, offset=3), B.chunk(b"ANNO", b"12345")])
    cases = {
        5: "FormHeader",
        12 + 3: "ChunkHeader",
        12 + 8 + 1: "Skip { remaining: 2, padded: true }",
        12 + 8 + 3: "Padding",
        12 + 12 + 8 + 4: "Comm { size: 18, padded: false }",
        12 + 12 + 26 + 8 + 2: "SsndHeader { remaining: 75, padded: true }",
        12 + 12 + 26 + 16 + 1: "SsndOffset { skip: 2, remaining_audio: 64, padded: true }",
        12 + 12 + 26 + 16 + 3 + 10: "Audio { remaining: 54, padded: true }",
    }
    for cut, state in cases.items():
        for piece in (None, 4):
            assert error_of(full[:cut], piece) == "truncated AIFF stream in state " + state, cut
    # an end inside a sample group whose chunk goes on is a truncation in Audio; the group rule is the SSND's end (above)
    assert error_of(full[:12 + 12 + 26 + 16 + 3 + 11]) == "truncated AIFF stream in state Audio { remaining: 53, padded: true }"
    assert ok(full) == S16 and ok(full, 9) == S16


def test_comm_limits():
    def with_comm(body, aifc=False):
        return B.form([B.chunk(b"COMM", body), B.ssnd(b"")], aifc=aifc)
    base = struct.pack(">HIH", 1, 0, 16) + B.extended(8000.0)
    assert error_of(with_comm(base[:17])) == "AIFF COMM is shorter than 18 bytes"
    assert error_of(with_comm(base + b"NON", aifc=True)) == "AIFF-C COMM has no compression type"
    assert error_of(with_comm(base + bytes(4097 - 18))) == "AIFF COMM exceeds the 4096 byte budget"
    assert ok(with_comm(base + bytes(4096 - 18))) == b""
    assert error_of(with_comm(base + b"GSM \0\0", aifc=True)) == "unsupported AIFF-C compression type: GSM "
    assert error_of(with_comm(base + b"\xe2\x82ab\0\0", aifc=True)) == "unsupported AIFF-C compression type: �ab"
    for ch, text in [(0, "invalid AIFF channel count: 0"), (33, "invalid AIFF channel count: 33"), (300, "invalid AIFF channel count: 300")]:
        assert error_of(with_comm(struct.pack(">HIH", ch, 0, 16) + B.extended(8000.0))) == text
    assert error_of(B.form([B.fver(), B.comm(3, 0, 16, 8000.0, b"ima4"), B.ssnd(b"")], aifc=True)) == "AIFF-C IMA4 supports at most two channels"
    for size, enc in [(0, None), (8, M.S8), (9, M.S16BE), (12, M.S16BE), (24, M.S24BE), (25, M.S32BE), (33, None)]:
        data = B.form([B.comm(1, 0, size, 8000.0), B.ssnd(bytes(24))])
        if enc is None:
            assert error_of(data) == "unsupported AIFF sample size: %d" % size
        else:
            from soundkit_amd import pcm_stream
            r = pcm_stream.AiffReader()
            r.add(data)
            assert r.info()["encoding"] == enc, size
            r.close()
            ok(data)
    # 32 channels of s8, and every AIFF-C tag
    assert ok(B.form([B.comm(32, 1, 8, 8000.0), B.ssnd(bytes(range(64)))])) == bytes(range(64))
    for tag, enc in [(b"NONE", M.S16BE), (b"raw ", M.U8), (b"twos", M.S16BE), (b"sowt", M.S16LE), (b"in24", M.S24BE), (b"in32", M.S32BE), (b"23ni", M.S32LE),
                     (b"FL32", M.F32BE), (b"fl32", M.F32BE), (b"FL64", M.F64BE), (b"fl64", M.F64BE), (b"ULAW", M.ULAW), (b"ulaw", M.ULAW),
                     (b"ALAW", M.ALAW), (b"alaw", M.ALAW), (b"ima4", M.IMA4)]:
        from soundkit_amd import pcm_stream
        data = B.form([B.fver(), B.comm(1, 0, 16, 8000.0, tag, b"name"), B.ssnd(bytes(34 * 24))], aifc=True)
        r = pcm_stream.AiffReader()
        r.add(data)
        assert r.info()["encoding"] == enc, tag
        r.close()
        ok(data, 13)


def test_sample_rates():
    from soundkit_amd import pcm_stream

    def rate_of(r):
        data = B.form([B.comm(1, 0, 16, r), B.ssnd(b"")])
        ok(data)
        rd = pcm_stream.AiffReader()
        rd.add(data)
        got = rd.info()["sample_rate"]
        rd.close()
        return got
    assert rate_of(8000.0) == 8000 and rate_of(44100.0) == 44100 and rate_of(22050.5) == 22051 and rate_of(0.5) == 1 and rate_of(4294967295.0) == 4294967295
    bad = lambda r: error_of(B.form([B.comm(1, 0, 16, r), B.ssnd(b"")]))
    assert bad(bytes(10)) == "AIFF sample rate is zero"
    assert bad(B.extended(-8000.0)) == "AIFF sample rate is negative"
    assert bad(struct.pack(">HQ", 0x7fff, 1 << 63)) == "AIFF sample rate is not finite"
    assert bad(struct.pack(">HQ", 0x7fff, 0)) == "AIFF sample rate is not finite"
    assert bad(4294967296.0) == "Invalid AIFF sample rate: 4294967296"
    assert bad(4294967296.5) == "Invalid AIFF sample rate: 4294967296.5"
    assert bad(1e22) == "Invalid AIFF sample rate: 10000000000000000000000"
    assert bad(struct.pack(">HQ", 16383 + 15, 0)) == "Invalid AIFF sample rate: 0"   # an unnormalised zero
    assert bad(struct.pack(">HQ", 0x7ffe, 1 << 63)) == "Invalid AIFF sample rate: inf"
    assert bad(struct.pack(">HQ", 0x7ffe, 0)) == "Invalid AIFF sample rate: NaN"
    assert bad(struct.pack(">HQ", 1, 1 << 63)) == "Invalid AIFF sample rate: 0"


def test_chunk_budget():
    from soundkit_amd import pcm_stream
    r = pcm_stream.AiffReader()
    with pytest.raises(ValueError) as ei:
        r.add(bytes(4 * 1024 * 1024 + 1))
    assert str(ei.value) == "AIFF input chunk exceeds the 4194304 byte streaming budget"
    m = M.AiffModel()
    with pytest.raises(ValueError) as em:
        m.add(bytes(4 * 1024 * 1024 + 1))
    assert str(em.value) == str(ei.value)
    data = B.form([B.comm(1, 0, 8, 8000.0), B.ssnd(bytes(4 * 1024 * 1024 - 64))])
    assert r.add(data)[1] == bytes(4 * 1024 * 1024 - 64)  # the budget's refusal left the walker usable, as the reference's is
    r.close()


# ---- sanitizer harness --------------------------------------------------------------------------------------------------------------

def test_mutated_headers_under_sanitizers(tmp_path):
    """tests/fuzz_aiff_stream.cpp: seeded mutations of the fixtures' first 256 bytes in ragged pieces -- no crash, no sanitizer
    report, every piece whole groups in order; a program of its own, nothing is loaded into this process"""
    exe = str(tmp_path / "fuzz_aiff_stream")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(HERE, "fuzz_aiff_stream.cpp")], cwd=HERE)
    out = subprocess.check_output([exe, "120"] + [os.path.join(AIFF, n) for n in FIXTURES], text=True)
    ok_n, err_n = int(out.split()[1]), int(out.split()[3])
    assert ok_n + err_n == 120 * len(FIXTURES) and ok_n >= len(FIXTURES) and err_n > 0, out

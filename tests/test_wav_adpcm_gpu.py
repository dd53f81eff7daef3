"""WAV's ADPCM blocks on the GPU (csrc/wav_adpcm.hip through sk_wav_adpcm_decode and its _dev form) against tests/wav_adpcm_model.py,
bit for bit.  tests/test_wav_coded_cpu.py pins the model: audioop for IMA, a hand-worked block for Microsoft ADPCM.  Shapes are the
smallest at which a lane can go wrong: the two smallest blocks of each form, a block that is no multiple of anything, the fixtures'
sizes, the largest block once; 1, 63, 64, 65 and 130 blocks (64 lanes a wave, 256 a workgroup, stereo doubling the lanes)."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import wav_adpcm_model as M
import wav_coded_builder as B

gpu = pytest.mark.gpu
IMA, MS = M.TAG_IMA, M.TAG_MS
COEF3 = [(256, 0), (300, -100), (-32768, 32767)]
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wav_coded")


def random_blocks(rng, tag, ch, align, n, n_coef=7):
    """valid headers: IMA step indices 0 ... 88, MS predictors below n_coef"""
    blocks = rng.integers(0, 256, (n, align), dtype=np.uint8)
    if tag == IMA:
        for c in range(ch):
            blocks[:, 4 * c + 2] = rng.integers(0, 89, n)
    else:
        blocks[:, :ch] = rng.integers(0, n_coef, (n, ch))
    return blocks


def run(engine, tag, ch, align, blocks, coef=None):
    data = blocks.tobytes() if isinstance(blocks, np.ndarray) else blocks
    got, status = engine.wav_adpcm_decode(tag, ch, align, data, coef)
    want, want_status = M.decode(tag, ch, align, data, coef)
    assert status == want_status
    assert len(got) == want.size * 2
    assert np.array_equal(np.frombuffer(got, "<i2"), want)
    return status


SHAPES = [(IMA, a) for a in (4, 8, 36, 256, 1024, 2048)] + [(MS, a) for a in (7, 8, 36, 256, 1024, 2048)]


@gpu
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("tag,per_channel", SHAPES, ids=["%s-%d" % ("ima" if t == IMA else "ms", a) for t, a in SHAPES])
def test_random_blocks_equal_the_model(engine, tag, per_channel, ch):
    """the block sizes are per channel where the form asks for a multiple (IMA: 4 x ch; MS 7 x ch and 7 x ch + 1 are its two smallest)"""
    align = per_channel * ch if tag == IMA or per_channel < 36 else per_channel
    if tag == MS and per_channel == 8:
        align = 7 * ch + 1
    rng = np.random.default_rng(1000 * tag + 10 * per_channel + ch)
    for n in ((1, 63, 64, 65, 130) if per_channel <= 256 else (1, 65)):
        run(engine, tag, ch, align, random_blocks(rng, tag, ch, align, n), M.MS_COEF if tag == MS else None)


@gpu
@pytest.mark.parametrize("tag,ch,align", [(IMA, 1, 32768), (IMA, 2, 65528), (MS, 1, 32774), (MS, 2, 65535)])
def test_the_largest_block(engine, tag, ch, align):
    """what the walker admits at most (MS mono: what the 65 536 sample budget admits; its fmt field stops two samples earlier)"""
    rng = np.random.default_rng(align)
    run(engine, tag, ch, align, random_blocks(rng, tag, ch, align, 3), M.MS_COEF if tag == MS else None)


@gpu
@pytest.mark.parametrize("ch", [1, 2])
def test_ima_clamps_at_both_rails_and_both_ends_of_the_step_table(engine, ch):
    """all-0x7 and all-0xF bodies from headers at +-32767 with index 88 and index 0: the predictor clamps, the index clamps at 88 and
    (nibbles 0 and 8, bodies 0x00 / 0x88) at 0"""
    blocks = []
    for pred in (32767, -32767, -32768):
        for idx in (88, 0):
            for body in (0x77, 0xff, 0x00, 0x88, 0x7f):
                blocks.append((struct.pack("<hBB", pred, idx, 0) * ch) + bytes([body]) * (36 * ch - 4 * ch))
    data = b"".join(blocks)
    run(engine, IMA, ch, 36 * ch, data)
    out = np.frombuffer(engine.wav_adpcm_decode(IMA, ch, 36 * ch, data)[0], "<i2")
    assert out.max() == 32767 and out.min() == -32768


@gpu
@pytest.mark.parametrize("ch", [1, 2])
def test_ms_every_standard_set_a_custom_table_the_delta_floor_and_both_rails(engine, ch):
    rng = np.random.default_rng(5 + ch)
    align = 7 * ch + 40
    # every one of the seven sets in turn, on every channel
    blocks = random_blocks(rng, MS, ch, align, 70)
    for c in range(ch):
        blocks[:, c] = (np.arange(70) + 3 * c) % 7
    run(engine, MS, ch, align, blocks, M.MS_COEF)
    # a table of three sets of its own, one of them with the extreme coefficients (the 32-bit sum wraps)
    blocks = random_blocks(rng, MS, ch, align, 66, n_coef=3)
    run(engine, MS, ch, align, blocks, COEF3)
    # delta driven to its floor (nibbles 0 ... 3 and 13 ... 15 shrink it) and up to its ceiling (nibble 8 triples it: 40 x 2 steps)
    hdr = lambda pred, delta, s1, s2: bytes([pred] * ch) + struct.pack("<h", delta) * ch + struct.pack("<h", s1) * ch + struct.pack("<h", s2) * ch  # noqa: E731
    special = [hdr(0, 16, 0, 0) + bytes([0x1f]) * 40, hdr(1, 17, 100, -100) + bytes([0x00]) * 40, hdr(2, -300, 5, 5) + bytes([0xd2]) * 40,
               hdr(0, 32767, 0, 0) + bytes([0x88]) * 40, hdr(4, 32767, 32767, 32767) + bytes([0x77]) * 40, hdr(5, -32768, -32768, -32768) + bytes([0x87]) * 40,
               hdr(0, 2000, 32000, 0) + bytes([0x78, 0x80]) * 20, hdr(6, 16, -32768, 32767) + bytes([0xf1]) * 40]
    data = b"".join(special)
    run(engine, MS, ch, align, data, M.MS_COEF)
    out = np.frombuffer(engine.wav_adpcm_decode(MS, ch, align, data, M.MS_COEF)[0], "<i2")
    assert out.max() == 32767 and out.min() == -32768


@gpu
@pytest.mark.parametrize("tag,ch", [(IMA, 1), (IMA, 2), (MS, 1), (MS, 2)])
def test_an_invalid_block_is_zeros_with_its_status_and_leaves_its_neighbours_alone(engine, tag, ch):
    rng = np.random.default_rng(40 + tag + ch)
    align = 36 * ch if tag == IMA else 7 * ch + 29
    coef = COEF3 if tag == MS else None
    blocks = random_blocks(rng, tag, ch, align, 67, n_coef=3)
    where = {0: 0, 31: ch - 1, 64: 0, 66: ch - 1}  # block: the channel whose header rules it out
    for k, c in where.items():
        if tag == IMA:
            blocks[k, 4 * c + 2] = 89 if k != 31 else 255
        else:
            blocks[k, c] = 3 if k != 31 else 255
    status = run(engine, tag, ch, align, blocks, coef)
    assert [k for k, s in enumerate(status) if s] == sorted(where) and all(status[k] == M.BAD_BLOCK for k in where)
    from soundkit_amd.engine import WAV_BAD_BLOCK
    assert WAV_BAD_BLOCK == M.BAD_BLOCK
    per = M.block_frames(tag, ch, align) * ch
    got = np.frombuffer(engine.wav_adpcm_decode(tag, ch, align, blocks.tobytes(), coef)[0], "<i2").reshape(67, per)
    clean = blocks.copy()
    for k, c in where.items():  # the neighbours are what they are without the bad blocks
        clean[k] = clean[1]
        assert not got[k].any()
    want = M.decode(tag, ch, align, clean.tobytes(), coef)[0].reshape(67, per)
    keep = [k for k in range(67) if k not in where]
    assert np.array_equal(got[keep], want[keep])


@gpu
@pytest.mark.parametrize("name", ["ima_mono_8k", "ima_stereo", "ms_mono_8k", "ms_stereo"])
def test_fixtures_through_decode_wav_equal_their_recordings(engine, name):
    from soundkit_amd import pcm_stream
    info, audio = pcm_stream.decode_wav(open(os.path.join(DIR, name + ".wav"), "rb").read(), engine=engine)
    want = open(os.path.join(DIR, name + ".decoded.s16le"), "rb").read()
    assert b"".join(a.data.tobytes() for a in audio) == want
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, info["channels"], 8000) for a in audio)


@gpu
@pytest.mark.parametrize("law", ["ulaw", "alaw"])
def test_g711_fixtures_through_decode_wav_equal_the_references_recordings(engine, law):
    import wave
    from soundkit_amd import pcm_stream
    _, audio = pcm_stream.decode_wav(open(os.path.join(DIR, law + "_A_Tusk.wav"), "rb").read(), engine=engine)
    with wave.open(os.path.join(DIR, "..", "aiff", "g711_%s.decoded.wav" % law)) as w:
        assert b"".join(a.data.tobytes() for a in audio) == w.readframes(w.getnframes())


@gpu
def test_decode_wav_names_a_bad_block(engine):
    from soundkit_amd import SoundkitError, pcm_stream
    pcm = np.random.default_rng(2).integers(-2000, 2000, (200, 1)).astype(np.int16)
    ima = bytearray(B.ima_wav(pcm, 36))
    ima[ima.index(b"data") + 8 + 36 + 2] = 90
    with pytest.raises(SoundkitError, match="Decoding failed: WAV IMA ADPCM block step index 90 exceeds 88"):
        pcm_stream.decode_wav(bytes(ima), engine=engine)
    ms = bytearray(B.ms_wav(pcm, 40, coef=COEF3))
    ms[ms.index(b"data") + 8 + 80] = 3
    with pytest.raises(SoundkitError, match="Decoding failed: WAV MS ADPCM block predictor 3 exceeds the 3 coefficient sets"):
        pcm_stream.decode_wav(bytes(ms), engine=engine)
    with pytest.raises(ValueError, match="decode_wav reads WAV format tags"):
        pcm_stream.decode_wav(B.wav(B.fmt_payload(1, 1, 8000, 2, 16), bytes(64)), engine=engine)


@gpu
def test_refused_calls(engine):
    from soundkit_amd._lib import SoundkitError
    for tag, ch, align, data, coef in [(1, 1, 36, bytes(36), None), (IMA, 3, 36, bytes(36), None), (IMA, 1, 38, bytes(38), None), (IMA, 2, 36, bytes(36), None),
                                       (MS, 2, 13, bytes(13), M.MS_COEF), (MS, 1, 40, bytes(40), None), (MS, 1, 40, bytes(40), M.MS_COEF * 5),
                                       (IMA, 1, 32772, bytes(32772), None), (MS, 1, 32775, bytes(32775), M.MS_COEF), (IMA, 1, 36, bytes(35), None)]:
        with pytest.raises(SoundkitError):
            engine.wav_adpcm_decode(tag, ch, align, data, coef)
    assert engine.wav_adpcm_decode(IMA, 1, 36, b"") == (b"", [])


@gpu
@pytest.mark.parametrize("tag,ch,align", [(IMA, 1, 36), (IMA, 2, 8), (MS, 1, 41), (MS, 2, 15)])
def test_the_dev_form_equals_the_host_form_and_stays_inside_its_buffers(engine, tag, ch, align):
    """sk_wav_adpcm_decode_dev: input, output and status in device memory, guard bytes around output and status"""
    import torch
    from soundkit_amd._lib import lib
    n = 67
    rng = np.random.default_rng(align)
    blocks = random_blocks(rng, tag, ch, align, n)
    blocks[5, 2 if tag == IMA else 0] = 200  # one invalid block
    coef = np.asarray(M.MS_COEF, np.int16)
    host, host_status = engine.wav_adpcm_decode(tag, ch, align, blocks.tobytes(), M.MS_COEF if tag == MS else None)
    need = len(host)
    src = torch.zeros((blocks.size + 31) // 16 * 16, dtype=torch.uint8, device="cuda")
    src[:blocks.size] = torch.from_numpy(blocks.reshape(-1).copy()).cuda()
    buf = torch.full((256 + need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.full((64 + n + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    got = C.c_size_t(0)
    torch.cuda.synchronize()
    args = (engine._h, tag, ch, align, coef.ctypes.data if tag == MS else None, 7 if tag == MS else 0, src.data_ptr(), blocks.size, buf.data_ptr() + 256)
    assert lib.sk_wav_adpcm_decode_dev(*args, need - 1, C.byref(got), st.data_ptr() + 256) == -1 and got.value == 0
    assert lib.sk_wav_adpcm_decode_dev(*args, need, C.byref(got), st.data_ptr() + 256) == 0 and got.value == need
    engine.synchronize()
    torch.cuda.synchronize()
    out, status = buf.cpu().numpy(), st.cpu().numpy()
    assert (out[:256] == 0xA5).all() and (out[256 + need:] == 0xA5).all()
    assert (status[:64] == 0x5A5A5A5A).all() and (status[64 + n:] == 0x5A5A5A5A).all()
    assert out[256:256 + need].tobytes() == host and status[64:64 + n].tolist() == host_status and host_status[5] == M.BAD_BLOCK

"""GSM 06.10 streams without a GPU: the model (tests/gsm_model.py) against the reference's recording, the two framings, the streaming
wrapper's texts, the state's layout, the exported symbols and the argument checks."""
import ctypes as C
import os
import subprocess
import wave

import numpy as np
import pytest

import gsm_model as M
import soundkit_amd
from soundkit_amd import _lib, telephony

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gsm")
NAME = "A_Tusk_is_used_to_make_costly_gifts"


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, NAME + ".gsm"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def twin():
    with wave.open(os.path.join(GOLDEN, NAME + ".decoded.wav")) as w:
        assert (w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()) == (8000, 1, 2, 23680)
        return np.frombuffer(w.readframes(23680), "<i2")


def test_model_equals_the_recording(fixture, twin):
    assert len(fixture) == 4884 == 148 * 33 and all(fixture[at] >> 4 == 0xD for at in range(0, 4884, 33))
    dec = M.GsmDecoder()
    got = dec.decode(fixture)
    assert got.size == 23680 and np.array_equal(got, twin)
    dec.flush()
    # what the fixture does not reach, and random frames have to (tests/test_gsm_decode_gpu.py)
    c = dec.core.count
    assert (c.sat_add, c.sat_sub, c.nc_out_of_range, c.clipped_frames) == (0, 0, 0, 0)


@pytest.mark.parametrize("chunk", [41, 19])  # 41: the reference's own test of the fixture
def test_split_anywhere_gives_the_same_samples(fixture, twin, chunk):
    dec = M.GsmDecoder()
    got = [dec.decode(fixture[at:at + chunk]) for at in range(0, len(fixture), chunk)]
    assert any(g.size == 0 for g in got) == (chunk < 33)  # a send that completes no packet gives nothing
    assert np.array_equal(np.concatenate(got), twin)
    dec.flush()


def test_microsoft_framing_decodes_to_the_same_samples(fixture, twin):
    ms = M.standard_to_microsoft(fixture)
    assert len(ms) == 74 * 65 and ms != fixture[:len(ms)]
    assert np.array_equal(M.GsmDecoder(M.MICROSOFT).decode(ms), twin)
    # the builder's two framings hold the same parameters, and reading them back gives them again
    frames = M.random_frames(5, 4)
    std, pair = M.build_stream(frames), M.build_stream(frames, M.MICROSOFT)
    assert len(std) == 132 and len(pair) == 130
    assert [M.frame_params(std, 4 + 264 * f) for f in range(4)] == frames == [M.frame_params(pair, 260 * f) for f in range(4)]
    assert M.standard_to_microsoft(std) == pair
    dec = M.GsmDecoder(M.MICROSOFT)
    got = np.concatenate([dec.decode(pair[at:at + 17]) for at in range(0, len(pair), 17)])
    assert np.array_equal(got, M.GsmDecoder().decode(std))


def test_partial_packet_is_reported_at_the_end():
    dec = M.GsmDecoder()
    assert dec.decode(bytes([0xD0, 0, 0])).size == 0
    with pytest.raises(ValueError, match=r"^GSM stream ended with 3 trailing partial-frame byte\(s\)$"):
        dec.flush()


def test_limit_text_at_1639_frames():
    frame = M.build_stream([M.make_params()])
    dec = M.GsmDecoder()
    dec.pending = frame[:5]
    with pytest.raises(ValueError, match=r"^Output buffer too small for GSM decode: need 262240, have 262144$"):
        dec.decode(frame[5:] + frame * 1638)
    assert dec.pending == frame[:5] and dec.core.words() == M.GsmCore().words()  # checked before anything else
    assert 1638 * 160 <= M.MAX_SEND_SAMPLES < 1639 * 160 and M.MAX_SEND_SAMPLES == telephony.MAX_SEND_SAMPLES


def test_rejected_frame_text(fixture):
    bad = bytearray(fixture[:99])
    bad[66] = 0xC0 | (bad[66] & 15)
    with pytest.raises(ValueError, match=r"^GSM decoder rejected frame$"):
        M.GsmDecoder().decode(bytes(bad))
    # a Microsoft packet carries no magic: any 65 bytes decode
    assert M.GsmDecoder(M.MICROSOFT).decode(bytes(range(65))).size == 320


def test_reflection_coefficients_stay_below_32768():
    """The lattice's MIN_WORD x MIN_WORD guard is unreachable: over every LARp the magnitude is at most 32767."""
    core = M.GsmCore()
    rp = core.to_rp(list(range(-32768, 32768)))
    assert max(rp) == 32767 and min(rp) == -32767


def test_state_layout_and_initial_values():
    assert C.sizeof(_lib.GsmState) == 138 * 4 and C.sizeof(_lib.GsmStream) == 12 and C.sizeof(_lib.GsmTickStream) == 20
    st = telephony.new_state(telephony.GSM)
    words = telephony.state_words(st)
    assert words == M.GsmCore().words() and len(words) == 138
    assert st.nrp == 40 and words.count(0) == 137 and words[129] == 40
    assert (_lib.GsmState.dp.offset, _lib.GsmState.v.offset, _lib.GsmState.msr.offset, _lib.GsmState.nrp.offset, _lib.GsmState.larpp.offset) == (0, 480, 512, 516, 520)
    assert telephony.gsm_decoded_samples(telephony.GSM_STANDARD, 70) == 320 and telephony.gsm_decoded_samples(telephony.GSM_MICROSOFT, 70) == 320
    assert telephony.gsm_decoded_samples(telephony.GSM_STANDARD, 32) == 0


def test_new_symbols_are_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", soundkit_amd.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ("sk_gsm_state_init", "sk_gsm_decode", "sk_gsm_decode_dev", "sk_gsm_decode_batch", "sk_gsm_decode_batch_dev", "sk_tick_run_gsm",
                 "sk_tick_gsm_out_bound_on", "sk_pipeline_spawn_gsm", "sk_gsm_decoder_create", "sk_gsm_decoder_destroy", "sk_gsm_decoder_info",
                 "sk_gsm_decoder_decode_i16", "sk_gsm_decoder_decode_i32", "sk_gsm_decoder_decode_f32", "sk_gsm_decoder_flush", "sk_gsm_decoder_reset",
                 "sk_gsm_decoder_last_error"):
        assert name in exported and name in soundkit_amd.declared_symbols(), name


def test_calls_without_an_engine_are_refused():
    n = C.c_size_t(7)
    st = telephony.new_state(telephony.GSM)
    assert _lib.lib.sk_gsm_decode(None, 0, None, 0, None, 0, C.byref(n), C.byref(st), None, 0) == -1
    assert _lib.lib.sk_gsm_decode_batch(None, None, 0, None, 0, None, 0, None, 0, C.byref(n), None, 0) == -1
    m = C.c_uint32(5)
    assert _lib.lib.sk_tick_run_gsm(None, None, 0, None, 0, None, 0, None, 0, None, 0, C.byref(m), None, None, 0) == -1
    assert _lib.lib.sk_tick_gsm_out_bound_on(None, None, 0, None, 0, C.byref(m)) == 0 and m.value == 0
    h = C.c_void_p()
    assert _lib.lib.sk_gsm_decoder_create(None, 0, C.byref(h)) == -1 and not h.value
    assert _lib.lib.sk_gsm_decoder_flush(None) == -1
    assert _lib.lib.sk_gsm_decoder_last_error(None) == b""
    handle = C.c_uint32()
    assert _lib.lib.sk_pipeline_spawn_gsm(None, 0, None, C.byref(handle)) == -1
    assert _lib.lib.sk_pipeline_spawn_gsm(None, 2, None, C.byref(handle)) == -1
    assert telephony.state_words(st) == M.GsmCore().words()


def test_wrappers_check_their_arguments():
    with pytest.raises(ValueError, match="variant must be"):
        telephony.GsmDecoder(None, 2)
    with pytest.raises(ValueError, match="variant must be"):
        telephony.gsm_decoded_samples(7, 33)

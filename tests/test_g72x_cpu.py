"""Telephony streams without a GPU: the models (tests/g72x_model.py) against the reference's recordings, the framing, the packings, the
exported symbols and the Python wrappers' argument checks."""
import ctypes as C
import os
import subprocess
import wave

import numpy as np
import pytest

import g72x_model as M
import soundkit_amd
from soundkit_amd import _lib, telephony

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = "A_Tusk_is_used_to_make_costly_gifts"


def twin(path, rate, frames):
    with wave.open(os.path.join(GOLDEN, path)) as w:
        assert (w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()) == (rate, 1, 2, frames)
        return np.frombuffer(w.readframes(frames), "<i2")


def fixture(path):
    with open(os.path.join(GOLDEN, path), "rb") as f:
        return f.read()


@pytest.mark.parametrize("kbit", [16, 24, 32, 40])
def test_g726_model_equals_the_recording(kbit):
    data = fixture("g726/%s_%d.g726" % (NAME, kbit))
    assert len(data) == 23680 * M.G726_BITS[kbit * 1000] // 8
    dec = M.G726Decoder(kbit * 1000, M.LEFT)
    assert np.array_equal(dec.decode(data), twin("g726/%s_%d.decoded.wav" % (NAME, kbit), 8000, 23680))
    dec.flush()


def test_g722_model_equals_the_recording():
    data = fixture("g722/%s.g722" % NAME)
    assert len(data) == 23680
    assert np.array_equal(M.G722Decoder().decode(data), twin("g722/%s.decoded.wav" % NAME, 16000, 47360))


def test_g722_scale_factors_start_at_zero():
    """What the recording pins: the C library's starting values 32 / 8 miss it, in the first second only."""
    data = fixture("g722/%s.g722" % NAME)
    want = twin("g722/%s.decoded.wav" % NAME, 16000, 47360)
    dec = M.G722Decoder()
    dec.band[0].det, dec.band[1].det = 32, 8
    got = dec.decode(data)
    wrong = np.nonzero(got != want)[0]
    assert wrong.size == 946 and wrong.max() < 8000


@pytest.mark.parametrize("law,name", [(M.ULAW, "ulaw"), (M.ALAW, "alaw")])
def test_g711_model_equals_the_recording(law, name):
    data = fixture("g711/%s.%s" % (NAME, name))
    assert len(data) == 23680
    assert np.array_equal(M.g711_decode(data, law), twin("aiff/g711_%s.decoded.wav" % name, 8000, 23680))


@pytest.mark.parametrize("rate", [16000, 24000, 32000, 40000])
def test_g726_split_anywhere_gives_the_same_samples(rate):
    data = fixture("g726/%s_%d.g726" % (NAME, rate // 1000))[2000:2000 + 6 * M.G726_GROUP_BYTES[rate]]
    whole = M.G726Decoder(rate).decode(data)
    for cut in range(len(data) + 1):  # mid-group for 24 and 40 kbit/s
        dec = M.G726Decoder(rate)
        got = np.concatenate([dec.decode(data[:cut]), dec.decode(data[cut:])])
        assert np.array_equal(got, whole), cut
        dec.flush()


def test_g722_split_anywhere_gives_the_same_samples():
    data = fixture("g722/%s.g722" % NAME)[3000:3030]
    whole = M.G722Decoder().decode(data)
    for cut in range(len(data) + 1):
        dec = M.G722Decoder()
        assert np.array_equal(np.concatenate([dec.decode(data[:cut]), dec.decode(data[cut:])]), whole), cut


def test_g726_partial_group_is_reported_at_the_end():
    dec = M.G726Decoder(40000)
    assert dec.decode(bytes(7)).size == 8
    with pytest.raises(ValueError, match=r"G\.726 stream ended with 2 trailing partial-packet byte\(s\)"):
        dec.flush()


@pytest.mark.parametrize("rate", [16000, 24000, 32000, 40000])
def test_g726_packings_round_trip_through_the_encoder(rate):
    t = np.arange(400)
    pcm = (6000 * np.sin(t * 0.07) + 2000 * np.sin(t * 0.31)).astype(np.int16)
    left, right = M.g726_encode(pcm, rate, M.LEFT), M.g726_encode(pcm, rate, M.RIGHT)
    assert len(left) == len(right) == 400 * M.G726_BITS[rate] // 8 and left != right
    a, b = M.G726Decoder(rate, M.LEFT).decode(left), M.G726Decoder(rate, M.RIGHT).decode(right)
    assert np.array_equal(a, b) and a.size == 400  # the same codes in both packings
    # the encoder's predictor is the decoder's: its state after the last sample is the state the decoder ends in
    core = M.G726Core()
    M.g726_encode(pcm, rate, M.RIGHT, core)
    dec = M.G726Decoder(rate, M.RIGHT)
    dec.decode(right)
    assert core.words() == dec.core.words()
    # and the codes survive a pack / unpack of every group
    bits = M.G726_BITS[rate]
    gb = M.G726_GROUP_BYTES[rate]
    for packing in (M.LEFT, M.RIGHT):
        data = left if packing == M.LEFT else right
        for g in range(0, len(data), gb):
            assert M.pack_code_group(M.unpack_code_group(data[g:g + gb], bits, packing), bits, packing) == data[g:g + gb]


def test_g722_encoder_keeps_in_step_with_the_decoder():
    t = np.arange(640)
    pcm = (5000 * np.sin(t * 0.05)).astype(np.int16)
    enc_side = M.G722Decoder()
    data = M.g722_encode(pcm, enc_side)
    dec = M.G722Decoder()
    out = dec.decode(data)
    assert len(data) == 320 and out.size == 640 and dec.words() == enc_side.words()
    assert len(set(data)) > 16  # a stream that exercises the adaptation, not a constant


def test_state_layouts():
    assert C.sizeof(_lib.G726State) == 96 and C.sizeof(_lib.G722State) == 264
    assert C.sizeof(_lib.G72xStream) == 16 and C.sizeof(_lib.G72xUnit) == 24 and C.sizeof(_lib.G72xTickStream) == 24
    assert telephony.state_words(telephony.new_state(telephony.G726)) == M.G726Core().words()
    assert telephony.state_words(telephony.new_state(telephony.G722)) == M.G722Decoder().words() == [0] * 66
    assert telephony.new_state(telephony.ULAW) is None


def test_new_symbols_are_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", soundkit_amd.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ("sk_g72x_decode", "sk_g72x_decode_dev", "sk_g72x_decode_batch", "sk_g72x_decode_batch_dev", "sk_tick_run_g72x",
                 "sk_tick_g72x_out_bound_on", "sk_g726_state_init", "sk_g722_state_init", "sk_g711_decoder_create", "sk_g722_decoder_create",
                 "sk_g726_decoder_create", "sk_g72x_decoder_decode_i16", "sk_g72x_decoder_decode_i32", "sk_g72x_decoder_decode_f32",
                 "sk_g726_decoder_flush", "sk_g72x_decoder_last_error"):
        assert name in exported and name in soundkit_amd.declared_symbols(), name
    assert b"telephony" in _lib.lib.sk_strerror(-701)


def test_calls_without_an_engine_are_refused():
    n = C.c_size_t(7)
    assert _lib.lib.sk_g72x_decode(None, 3, 32000, 0, None, 0, None, 0, C.byref(n), None, None, 0) == -1
    h = C.c_void_p()
    assert _lib.lib.sk_g722_decoder_create(None, C.byref(h)) == -1 and not h.value
    assert _lib.lib.sk_g726_decoder_flush(None) == -1
    assert _lib.lib.sk_g72x_decoder_last_error(None) == b""


def test_wrappers_check_their_arguments():
    with pytest.raises(ValueError, match="rate must be one of"):
        telephony.G726Decoder(None, rate=8000)
    with pytest.raises(ValueError, match="packing must be"):
        telephony.G726Decoder(None, rate=32000, packing=2)
    with pytest.raises(ValueError, match="law must be"):
        telephony.G711Decoder(None, telephony.G722)
    with pytest.raises(ValueError, match="codec must be"):
        telephony.new_state(4)
    assert telephony.decoded_samples(telephony.G726, 7, 40000) == 8 and telephony.decoded_samples(telephony.G722, 5) == 10
    assert telephony.decoded_samples(telephony.ULAW, 5) == 5 and telephony.decoded_samples(telephony.G726, 5, 16000) == 20

"""The GSM 06.10 decode stage on the GPU (csrc/gsm_decode.hip through sk_gsm_decode, sk_gsm_decode_batch and GsmDecoder), bit for bit
against tests/gsm_model.py, which tests/test_gsm_cpu.py pins to the reference's recording.  Every comparison is equality.

The recording reaches no saturating add or subtract and no lag outside 40 ... 120 (test_gsm_cpu.py counts them), so random frames and
built frames are what holds those paths; the model counts what they reach and the tests assert it."""
import ctypes as C
import functools
import os
import wave

import numpy as np
import pytest

import gsm_model as M

gpu = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gsm")
NAME = "A_Tusk_is_used_to_make_costly_gifts"


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(GOLDEN, NAME + ".gsm"), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def twin():
    with wave.open(os.path.join(GOLDEN, NAME + ".decoded.wav")) as w:
        return np.frombuffer(w.readframes(w.getnframes()), "<i2")


def model_units(units, variant=M.STANDARD, core=None):
    """-> ([s16le bytes per unit], final state words, the core)"""
    core = core or M.GsmCore()
    out = [M.decode_packets(core, u, variant).astype("<i2").tobytes() for u in units]
    return out, core.words(), core


@functools.lru_cache(maxsize=None)
def fixture_final_words():
    return model_units([fixture()])[1]


def new_state():
    from soundkit_amd import telephony
    return telephony.new_state(telephony.GSM)


def words(state):
    from soundkit_amd import telephony
    return telephony.state_words(state)


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------

@gpu
def test_fixture_equals_its_twin_in_one_call(engine):
    state = new_state()
    got = np.frombuffer(engine.gsm_decode(fixture(), state), "<i2")
    assert got.size == 23680 and np.array_equal(got, twin())
    assert words(state) == fixture_final_words()


@gpu
def test_fixture_in_the_microsoft_framing_equals_its_twin(engine):
    from soundkit_amd import telephony
    state = new_state()
    got = np.frombuffer(engine.gsm_decode(M.standard_to_microsoft(fixture()), state, telephony.GSM_MICROSOFT), "<i2")
    assert np.array_equal(got, twin())
    assert words(state) == fixture_final_words()


@gpu
@pytest.mark.parametrize("frames", [1, 2, 3, 7])
def test_fixture_cut_into_units_with_the_state_carried(engine, frames):
    """as the units of one stream in one batch, and as calls of their own with the state handed on"""
    data = fixture()
    units = [data[at:at + 33 * frames] for at in range(0, len(data), 33 * frames)]
    state = new_state()
    got = engine.gsm_decode_batch([{"n_units": len(units), "state": state}], units)
    assert b"".join(got) == twin().tobytes() and [len(g) for g in got] == [len(u) // 33 * 320 for u in units]
    assert words(state) == fixture_final_words()
    state = new_state()
    assert b"".join(engine.gsm_decode(u, state) for u in units[:12]) == twin()[:12 * frames * 160].tobytes()
    assert words(state) == model_units([data[:12 * frames * 33]])[1]


# ---- random frames: the saturations -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_stream():
    """64 random frames: (bytes, the model's s16le, its final words)"""
    data = M.build_stream(M.random_frames(2026, 64))
    pcm, final, core = model_units([data])
    c = core.count
    # the seed reaches every path the recording does not
    assert c.sat_add >= 1 and c.sat_sub >= 1 and c.nc_out_of_range >= 1 and c.clipped_frames >= 1, vars(c)
    return data, pcm[0], final


def test_the_random_frames_reach_the_saturations_in_the_model():
    data, pcm, _ = random_stream()
    assert len(data) == 64 * 33 and len(pcm) == 64 * 320


@gpu
@pytest.mark.parametrize("variant", [M.STANDARD, M.MICROSOFT], ids=["standard", "microsoft"])
def test_random_frames_equal_the_model(engine, variant):
    data, pcm, final = random_stream()
    state = new_state()
    got = engine.gsm_decode(data if variant == M.STANDARD else M.standard_to_microsoft(data), state, variant)
    assert got == pcm
    assert words(state) == final


# ---- built frames: the edges ------------------------------------------------------------------------------------------------------------

def edge_streams():
    """name -> frames (76 parameters each); every stream starts fresh, so its first subframe meets nrp = 40"""
    loud = dict(xmaxc=(63, 48, 40, 63), bc=(3, 3, 3, 3))
    out = {}
    # the lag: in range at both ends, just outside, far outside; the first subframe of a fresh stream out of range
    for nc in (39, 40, 120, 121, 0, 127):
        out["nc %d first" % nc] = [M.make_params(nc=(nc, 77, nc, 101), **loud), M.make_params(nc=(nc, nc, 120, nc), **loud)]
    out["nc after a valid one"] = [M.make_params(nc=(97, 0, 127, 39), **loud), M.make_params(nc=(121, 120, 40, 39), **loud)]
    # the block maximum: both ends of both branches of the exponent, and the mantissa's normalisation
    for x in (0, 7, 8, 15, 16, 63):
        out["xmaxc %d" % x] = [M.make_params(xmaxc=(x, x, 63 - x, x), nc=(40, 41, 80, 119), bc=(0, 1, 2, 3)), M.make_params(xmaxc=(x,) * 4, bc=(3, 2, 1, 0))]
    # every grid position with every gain
    for mc in range(4):
        out["mc %d" % mc] = [M.make_params(mc=(mc, (mc + 1) % 4, (mc + 2) % 4, (mc + 3) % 4), bc=(b, b, (b + 1) % 4, (b + 2) % 4), xmaxc=(50, 33, 20, 9),
                                           nc=(45, 60, 100, 120)) for b in range(4)]
    # the log-area ratios at both ends, and a swing from one to the other through the interpolation
    lo, hi = (0,) * 8, tuple((1 << b) - 1 for b in M.LAR_BITS)
    out["larc zero"] = [M.make_params(larc=lo, **loud)] * 2
    out["larc ones"] = [M.make_params(larc=hi, **loud)] * 2
    out["larc swing"] = [M.make_params(larc=lo, **loud), M.make_params(larc=hi, **loud), M.make_params(larc=lo, **loud)]
    # all pulses at both ends
    out["xmc ends"] = [M.make_params(xmc=[[0] * 13, [7] * 13, [0, 7] * 6 + [0], [7, 0] * 6 + [7]], **loud)] * 2
    return out


@functools.lru_cache(maxsize=None)
def edge_built():
    built = {}
    reached = M.Counters()
    for name, frames in edge_streams().items():
        data = M.build_stream(frames)
        pcm, final, core = model_units([data])
        built[name] = (data, pcm[0], final)
        reached.nc_out_of_range += core.count.nc_out_of_range
    assert reached.nc_out_of_range >= 10
    return built


def test_the_edge_streams_decode_in_the_model():
    built = edge_built()
    assert len(built) == 21 and len({b[1] for b in built.values()}) > 16  # the edges give different samples


@gpu
def test_edge_frames_equal_the_model(engine):
    """all edge streams in one batch, each a fresh stream"""
    built = edge_built()
    names = sorted(built)
    states = [new_state() for _ in names]
    got = engine.gsm_decode_batch([{"n_units": 1, "state": st} for st in states], [built[n][0] for n in names])
    for n, g, st in zip(names, got, states):
        assert g == built[n][1], n
        assert words(st) == built[n][2], n


@gpu
def test_edge_frames_in_the_microsoft_framing(engine):
    built = edge_built()
    names = [n for n in sorted(built) if len(built[n][0]) % 66 == 0]
    states = [new_state() for _ in names]
    got = engine.gsm_decode_batch([{"n_units": 1, "variant": M.MICROSOFT, "state": st} for st in states], [M.standard_to_microsoft(built[n][0]) for n in names])
    assert len(names) >= 20
    for n, g, st in zip(names, got, states):
        assert g == built[n][1], n
        assert words(st) == built[n][2], n


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------

LENGTHS = (1, 2, 4, 5)  # frames: two exercise the LAR interpolation, four and more wrap the 120-sample history


@functools.lru_cache(maxsize=None)
def shaped_stream(i):
    """stream i of a batch: (bytes, s16le, final words); LENGTHS[i % 4] random frames, an even number in the Microsoft framing"""
    n = LENGTHS[i % 4]
    data = M.build_stream(M.random_frames(9000 + i, n))
    pcm, final, _ = model_units([data])
    return data, pcm[0], final


@gpu
@pytest.mark.parametrize("n_streams", [1, 63, 64, 65, 130])
def test_batches_of_streams_of_different_lengths(engine, n_streams):
    states = [new_state() for _ in range(n_streams)]
    got = engine.gsm_decode_batch([{"n_units": 1, "state": st} for st in states], [shaped_stream(i)[0] for i in range(n_streams)])
    for i in range(n_streams):
        assert got[i] == shaped_stream(i)[1], i
        assert words(states[i]) == shaped_stream(i)[2], i


@gpu
def test_an_empty_unit_between_two_full_ones_and_both_variants_in_one_batch(engine):
    data, pcm, final = random_stream()
    a, b = data[:5 * 33], data[5 * 33:12 * 33]
    ms = M.standard_to_microsoft(data[:12 * 33])
    want_final = model_units([data[:12 * 33]])[1]
    st = [new_state() for _ in range(4)]
    streams = [{"n_units": 3, "state": st[0]}, {"n_units": 2, "variant": M.MICROSOFT, "state": st[1]}, {"n_units": 0, "state": st[2]},
               {"n_units": 3, "variant": M.MICROSOFT, "state": st[3]}]
    got = engine.gsm_decode_batch(streams, [a, b"", b, ms[:65 * 2], ms[65 * 2:], b"", ms, b""])
    assert [len(g) for g in got] == [1600, 0, 2240, 1280, 2560, 0, 3840, 0]
    assert got[0] + got[2] == got[3] + got[4] == got[6] == pcm[:12 * 320]
    assert words(st[0]) == words(st[1]) == words(st[3]) == want_final
    assert words(st[2]) == M.GsmCore().words()  # a stream without units keeps its carry


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------

def raw_batch(engine, streams, units, states, out_cap=None, n_states=None):
    """sk_gsm_decode_batch with the status coming back; streams: (variant, n_units, state index); `states` is the caller's array"""
    from soundkit_amd._lib import G72xUnit, GsmStream, lib
    ts = (GsmStream * max(len(streams), 1))()
    for i, (variant, n, state) in enumerate(streams):
        ts[i].variant, ts[i].n_units, ts[i].state = variant, n, state
    table = (G72xUnit * max(len(units), 1))()
    total = 0
    for k, u in enumerate(units):
        table[k].offset, table[k].size = total, len(u)
        total += (len(u) + 15) & ~15
    blob = np.zeros(max(total, 16), np.uint8)
    for k, u in enumerate(units):
        blob[table[k].offset:table[k].offset + len(u)] = np.frombuffer(bytes(u), np.uint8)
    need = sum((len(u) // 33 * 320 + 15) & ~15 for u in units)
    out = np.full(need + 64, 0xAB, np.uint8)
    used = C.c_size_t(77)
    rc = lib.sk_gsm_decode_batch(engine._h, ts, len(streams), table, len(units), blob.ctypes.data, total, out.ctypes.data, need if out_cap is None else out_cap,
                                 C.byref(used), states, len(states) if n_states is None else n_states)
    return rc, used.value, out


@gpu
def test_refusals_leave_the_states_byte_for_byte_as_they_were(engine):
    from soundkit_amd._lib import GsmState
    data = random_stream()[0]
    units = [data[:66], data[66:165], data[165:198]]
    states = (GsmState * 3)()
    for i in range(3):  # carries that are in use: after a different number of frames each
        st = new_state()
        engine.gsm_decode(data[33:33 * (i + 2)], st)
        states[i] = st
    before = bytes(states)
    rows = [(0, 1, 0), (0, 1, 1), (0, 1, 2)]
    bad_magic = bytearray(units[2])
    bad_magic[0] = 0x50 | (bad_magic[0] & 15)
    last_frame_bad = bytearray(units[1])
    last_frame_bad[66] &= 0x0F
    refusals = [("a partial packet", -1, rows, [units[0], units[1][:-1], units[2]], None, None),
                ("a bad magic in the last frame of the last stream", -701, rows, [units[0], units[1], bytes(bad_magic)], None, None),
                ("a bad magic in the last frame of a longer unit", -701, rows, [units[0], bytes(last_frame_bad), units[2]], None, None),
                ("an out_cap one byte short", -1, rows, units, 640 + 960 + 320 - 1, None),
                ("a state named twice", -1, [(0, 1, 0), (0, 1, 1), (0, 1, 1)], units, None, None),
                ("a state that is not there", -1, rows, units, None, 2),
                ("a variant that is none", -1, [(0, 1, 0), (2, 1, 1), (0, 1, 2)], units, None, None),
                ("units that do not add up", -1, [(0, 1, 0), (0, 1, 1), (0, 2, 2)], units, None, None)]
    for label, status, table, us, cap, n_states in refusals:
        rc, used, out = raw_batch(engine, table, us, states, cap, n_states)
        assert rc == status and used == 0, label
        assert bytes(states) == before, label
        assert out.tobytes() == b"\xAB" * out.size, label  # nothing was written
    # the same call without the fault decodes, from the carries as they were
    want = []
    for i in range(3):
        core = M.GsmCore()
        M.decode_packets(core, data[33:33 * (i + 2)])
        want.append(model_units([units[i]], core=core))
    rc, used, out = raw_batch(engine, rows, units, states)
    assert rc == 0 and used == 640 + 960 + 320
    assert out[:used].tobytes() == b"".join(w[0][0] for w in want)
    for i in range(3):
        assert words(states[i]) == want[i][1]


@gpu
def test_single_call_refusals_and_their_texts(engine):
    from soundkit_amd import telephony
    from soundkit_amd._lib import lib
    data = fixture()
    state = new_state()
    engine.gsm_decode(data[:330], state)
    before = bytes(state)

    def call(variant, payload, out_cap=None):
        src = np.frombuffer(payload, np.uint8)
        out = np.full(max(len(payload) * 10, 16), 0xAB, np.uint8)
        n, text = C.c_size_t(77), C.create_string_buffer(200)
        rc = lib.sk_gsm_decode(engine._h, variant, src.ctypes.data, src.size, out.ctypes.data, out.size if out_cap is None else out_cap, C.byref(n), C.byref(state),
                               text, 200)
        assert bytes(state) == before and n.value == 0 and out.tobytes() == b"\xAB" * out.size
        return rc, text.value.decode()

    assert call(0, data[330:330 + 65]) == (-1, "")  # a partial packet
    assert call(1, data[330:330 + 66]) == (-1, "")
    assert call(2, data[330:330 + 33]) == (-1, "")
    assert call(0, data[330:330 + 66], 639) == (-1, "")  # out_cap one byte short
    bad = bytearray(data[330:330 + 99])
    bad[66] = 0xE0 | (bad[66] & 15)
    assert call(0, bytes(bad)) == (-701, "GSM decoder rejected frame")
    assert call(0, data[:33] * 1639) == (-701, "Output buffer too small for GSM decode: need 262240, have 262144")
    assert call(1, bytes(65 * 820)) == (-701, "Output buffer too small for GSM decode: need 262400, have 262144")
    with pytest.raises(telephony.TelephonyError, match="^GSM decoder rejected frame$"):
        engine.gsm_decode(bytes(bad), state)
    assert bytes(state) == before
    # and the stream goes on from where it was
    assert engine.gsm_decode(data[330:660], state) == twin()[1600:3200].tobytes()


@gpu
def test_1638_frames_pass_in_one_call(engine):
    """the limit itself: 262 080 samples.  The model decodes the recording once; the call's first 148 frames are the recording, and the
    state that comes back continues it."""
    data = fixture()
    payload = (data * 12)[:1638 * 33]
    state = new_state()
    got = np.frombuffer(engine.gsm_decode(payload, state), "<i2")
    assert got.size == 262080 and np.array_equal(got[:23680], twin())
    again = new_state()
    parts = [engine.gsm_decode(payload[at:at + 33 * 234], again) for at in range(0, len(payload), 33 * 234)]
    assert b"".join(parts) == got.tobytes() and words(again) == words(state)


# ---- GsmDecoder ---------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("variant,chunk", [(M.STANDARD, 41), (M.STANDARD, 19), (M.MICROSOFT, 17)], ids=["standard-41", "standard-19", "microsoft-17"])
def test_decoder_holds_the_partial_packet_across_calls(engine, variant, chunk):
    from soundkit_amd import telephony
    data = fixture()[:33 * 40]
    want = twin()[:160 * 40]
    if variant == M.MICROSOFT:
        data = M.standard_to_microsoft(data)
    dec = telephony.GsmDecoder(engine, variant)
    assert (dec.sample_rate, dec.channels) == (8000, 1)
    got = [dec.decode_i16(data[at:at + chunk]) for at in range(0, len(data), chunk)]
    assert any(g.size == 0 for g in got) == (chunk < 33)  # a call that completes no packet gives nothing
    assert np.array_equal(np.concatenate(got), want)
    dec.flush()


@gpu
def test_decoder_i32_and_f32_follow_from_i16(engine):
    from soundkit_amd import telephony
    data = random_stream()[0][:33 * 8]
    want = np.frombuffer(random_stream()[1][:320 * 8], "<i2")
    a, b, c = (telephony.GsmDecoder(engine) for _ in range(3))
    i16, i32, f32 = a.decode_i16(data), b.decode_i32(data), c.decode_f32(data)
    assert np.array_equal(i16, want) and want.any()
    assert i32.dtype == np.int32 and np.array_equal(i32, want.astype(np.int32) << 16)
    assert f32.dtype == np.float32 and np.array_equal(f32, want.astype(np.float32) / np.float32(32768))


@gpu
def test_decoder_flush_reset_and_errors(engine):
    from soundkit_amd import telephony
    from soundkit_amd._lib import lib
    data = fixture()
    dec = telephony.GsmDecoder(engine)
    assert np.array_equal(dec.decode_i16(data[:69]), twin()[:320])
    with pytest.raises(telephony.TelephonyError, match=r"^GSM stream ended with 3 trailing partial-frame byte\(s\)$"):
        dec.flush()
    # a rejected frame consumes nothing: the pending bytes and the carry stay, and the stream goes on
    bad = bytearray(data[69:165])
    bad[30] = 0x10 | (bad[30] & 15)  # byte 99 of the stream: the fourth frame's first
    with pytest.raises(telephony.TelephonyError, match="^GSM decoder rejected frame$"):
        dec.decode_i16(bytes(bad))
    assert np.array_equal(dec.decode_i16(data[69:165]), twin()[320:800])
    dec.flush()
    # SK_ERR_CAPACITY with the reference's text, nothing consumed
    out = np.zeros(319, np.int16)
    n = C.c_size_t(5)
    src = np.frombuffer(data[165:231], np.uint8)
    assert lib.sk_gsm_decoder_decode_i16(dec._h, src.ctypes.data, 66, out.ctypes.data, 319, C.byref(n)) == -7 and n.value == 0
    assert lib.sk_gsm_decoder_last_error(dec._h) == b"Output buffer too small for GSM decode: need 320, have 319"
    assert np.array_equal(dec.decode_i16(data[165:231]), twin()[800:1120])
    # reset: a new stream, nothing pending
    dec.decode_i16(data[231:240])
    dec.reset()
    dec.flush()
    assert np.array_equal(dec.decode_i16(data[:330]), twin()[:1600])

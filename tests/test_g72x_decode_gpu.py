"""The telephony decode stage on the GPU (csrc/g72x_decode.hip through sk_g72x_decode, sk_g72x_decode_batch and the Decoder objects),
bit for bit against tests/g72x_model.py, which tests/test_g72x_cpu.py pins to the reference's recordings."""
import ctypes as C
import functools
import os
import wave

import numpy as np
import pytest

import g72x_model as M

gpu = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = "A_Tusk_is_used_to_make_costly_gifts"
# (id, codec, G.726 rate, input, twin, rate of the twin)
FIXTURES = [("g726-%d" % k, M.G726, k * 1000, "g726/%s_%d.g726" % (NAME, k), "g726/%s_%d.decoded.wav" % (NAME, k), 8000) for k in (16, 24, 32, 40)] + [
    ("g722", M.G722, 0, "g722/%s.g722" % NAME, "g722/%s.decoded.wav" % NAME, 16000),
    ("ulaw", M.ULAW, 0, "g711/%s.ulaw" % NAME, "aiff/g711_ulaw.decoded.wav", 8000),
    ("alaw", M.ALAW, 0, "g711/%s.alaw" % NAME, "aiff/g711_alaw.decoded.wav", 8000)]


def load(path):
    with open(os.path.join(GOLDEN, path), "rb") as f:
        return f.read()


def twin(path):
    with wave.open(os.path.join(GOLDEN, path)) as w:
        return np.frombuffer(w.readframes(w.getnframes()), "<i2")


def make_decoder(engine, codec, rate, packing=M.LEFT):
    from soundkit_amd import telephony
    if codec == M.G726:
        return telephony.G726Decoder(engine, rate, packing)
    return telephony.G722Decoder(engine) if codec == M.G722 else telephony.G711Decoder(engine, codec, 8000, 1)


def model_decode(codec, rate, packing, units, words=None):
    """-> ([samples per unit], the model's final state words or None); G.726 units hold whole groups"""
    if codec == M.G726:
        dec = M.G726Decoder(rate, packing)
        if words is not None:
            dec.core = M.G726Core(words)
        out = [dec.decode(u) for u in units]
        assert not dec.pending
        return out, dec.core.words()
    if codec == M.G722:
        dec = M.G722Decoder(words)
        return [dec.decode(u) for u in units], dec.words()
    return [M.g711_decode(u, codec) for u in units], None


@gpu
@pytest.mark.parametrize("fx", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_fixture_equals_its_twin_in_one_call(engine, fx):
    from soundkit_amd import telephony
    _, codec, rate, src, ref, _ = fx
    state = telephony.new_state(codec)
    got = np.frombuffer(engine.g72x_decode(codec, load(src), state, rate or 32000, M.LEFT), "<i2")
    assert np.array_equal(got, twin(ref))
    if state is not None:  # the carry that comes back is the model's
        assert telephony.state_words(state) == model_decode(codec, rate, M.LEFT, [load(src)])[1]


@gpu
@pytest.mark.parametrize("fx", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_fixture_equals_its_twin_through_the_decoder_in_127_byte_sends(engine, fx):
    """the carried state from send to send, and for G.726-24 / -40 the pending partial group (127 is no multiple of 3 or 5)"""
    _, codec, rate, src, ref, hz = fx
    data = load(src)
    dec = make_decoder(engine, codec, rate)
    assert (dec.sample_rate, dec.channels) == (hz, 1)
    got = np.concatenate([dec.decode_i16(data[k:k + 127]) for k in range(0, len(data), 127)])
    assert np.array_equal(got, twin(ref))
    if codec == M.G726:
        dec.flush()


@gpu
@pytest.mark.parametrize("fx", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_fixture_equals_its_twin_through_the_decoder_in_1_byte_sends(engine, fx):
    """one byte a send over the fixture's first 1500 bytes: at 24 / 40 kbit/s two sends in three (four in five) complete no group"""
    from soundkit_amd import telephony
    _, codec, rate, src, ref, _ = fx
    data = load(src)[:1500]
    dec = make_decoder(engine, codec, rate)
    pieces = [dec.decode_i16(data[k:k + 1]) for k in range(len(data))]
    want = twin(ref)[:telephony.decoded_samples(codec, len(data), rate or 32000)]
    assert np.array_equal(np.concatenate(pieces), want) and want.size >= 1500
    if codec == M.G726 and rate in (24000, 40000):
        assert sum(1 for p in pieces if p.size == 0) == len(data) - len(data) // M.G726_GROUP_BYTES[rate]
        dec.flush()


@gpu
def test_g726_flush_reports_the_partial_group(engine):
    from soundkit_amd import telephony
    dec = telephony.G726Decoder(engine, 40000, telephony.LEFT)
    assert dec.decode_i16(bytes(range(7))).size == 8
    with pytest.raises(telephony.TelephonyError, match=r"^G\.726 stream ended with 2 trailing partial-packet byte\(s\)$"):
        dec.flush()
    dec.reset()
    dec.flush()


@gpu
@pytest.mark.parametrize("fx", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_decode_i32_and_f32_follow_from_i16(engine, fx):
    _, codec, rate, src, ref, _ = fx
    data = load(src)[4000:4000 + 1200]
    i16 = make_decoder(engine, codec, rate).decode_i16(data)
    i32 = make_decoder(engine, codec, rate).decode_i32(data)
    f32 = make_decoder(engine, codec, rate).decode_f32(data)
    assert i16.size and i32.dtype == np.int32 and f32.dtype == np.float32
    assert np.array_equal(i32, i16.astype(np.int32) << 16)
    assert np.array_equal(f32, i16.astype(np.float32) / np.float32(32768.0))


# ---- a batch of mixed streams ---------------------------------------------------------------------------------------------------------

KINDS = [(M.G726, r, p) for r in (16000, 24000, 32000, 40000) for p in (M.LEFT, M.RIGHT)] + [(M.G722, 0, 0), (M.ULAW, 0, 0), (M.ALAW, 0, 0)]
GROUPS = [0, 1, 63, 64, 65, 2, 17, 0, 5]  # groups (G.726) or bytes per unit, dealt round robin; some streams also get a unit of about 3000 bytes


def tone_stream(rate, packing):
    """a tone near 2 kHz, then quiet, then steps: through the model's encoder this pulls a2 to its clamp, sets the tone detector and, at
    the steps, takes the transition reset -- which random bytes rarely reach"""
    t = np.arange(1600)
    pcm = (12000 * np.sin(t * np.pi / 2 * 0.98)).astype(np.int16)
    pcm[800:] //= 8
    pcm[1200:1210] = 30000
    pcm[1400:1600:2] = -30000
    return M.g726_encode(pcm, rate, packing)


@functools.lru_cache(maxsize=None)
def batch():
    """130 streams (two waves and a ragged third): all four rates x both packings, G.722, both laws; several units a stream.  Random
    bytes drive the adaptation into its output and scale clamps; six streams are tone_stream's.  -> [(codec, rate, packing, units)]"""
    rng = np.random.default_rng(726)
    out = []
    for i in range(130):
        codec, rate, packing = KINDS[i % len(KINDS)]
        gb = M.G726_GROUP_BYTES[rate] if codec == M.G726 else 1
        n_units = 1 + i % 4
        lens = [GROUPS[(i + 3 * u) % len(GROUPS)] * gb for u in range(n_units)]
        if i % 13 == 5:
            lens.append(3000 // gb * gb)
        units = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
        if codec == M.G726 and rate != 16000 and 22 <= i < 33:  # one of each rate and packing above 16 kbit/s
            data = tone_stream(rate, packing)
            units = [data[:65 * gb], data[65 * gb:66 * gb], data[66 * gb:]]
        out.append((codec, rate, packing, units))
    return out


@functools.lru_cache(maxsize=None)
def batch_model():
    return [model_decode(c, r, p, units) for c, r, p, units in batch()]


def run_batch(engine, streams, deal=None):
    """streams through Engine.g72x_decode_batch; deal: per stream a list of unit lists to use instead of its own units.
    -> ([samples per stream], [state words or None per stream])"""
    from soundkit_amd import telephony
    entries, units = [], []
    for i, (codec, rate, packing, us) in enumerate(streams):
        us = deal[i] if deal is not None else us
        entries.append({"codec": codec, "rate": rate or 32000, "packing": packing, "n_units": len(us), "state": telephony.new_state(codec)})
        units += us
    got = engine.g72x_decode_batch(entries, units)
    out, at = [], 0
    for e in entries:
        out.append([np.frombuffer(g, "<i2") for g in got[at:at + e["n_units"]]])
        at += e["n_units"]
    return out, [telephony.state_words(e["state"]) if e["state"] is not None else None for e in entries]


def test_the_batch_reaches_the_clamps_and_the_transition_reset():
    """(no GPU) what the batch's streams are for: in the model they saturate the output, hold yu at both ends, clamp a2, set the tone
    detector and take the transition reset"""
    seen = set()
    for codec, rate, packing, units in batch():
        if codec != M.G726:
            continue
        core = M.G726Core()
        data, gb = b"".join(units), M.G726_GROUP_BYTES[rate]
        for g in range(0, len(data), gb):
            for code in M.unpack_code_group(data[g:g + gb], M.G726_BITS[rate], packing):
                td = core.td
                v = core.decode_code(code, rate)
                if td and core.ap == 256 and core.a == [0, 0] and core.b == [0] * 6:
                    seen.add("transition reset at %d" % rate)
                if v in (-32768, 32767):
                    seen.add("output clamp")
                if core.yu in (544, 5120):
                    seen.add("yu at %d" % core.yu)
                if abs(core.a[1]) == 12288:
                    seen.add("a2 clamp")
    assert seen == {"output clamp", "yu at 544", "yu at 5120", "a2 clamp"} | {"transition reset at %d" % r for r in (24000, 32000, 40000)}
    assert len(batch()) == 130 and {k[:3] for k in batch()} == set(KINDS)


@gpu
def test_a_batch_of_130_mixed_streams_equals_the_model(engine):
    streams, want = batch(), batch_model()
    got, states = run_batch(engine, streams)
    for i, (codec, rate, packing, units) in enumerate(streams):
        assert len(got[i]) == len(units)
        for u in range(len(units)):
            assert np.array_equal(got[i][u], want[i][0][u]), (i, codec, rate, packing, u, len(units[u]))
        assert states[i] == want[i][1], (i, codec, rate, packing)
    assert sum(len(s[3]) for s in streams) > 300 and any(len(u) >= 2990 for s in streams for u in s[3])


@gpu
def test_the_same_bytes_dealt_into_units_differently(engine):
    streams, want = batch(), batch_model()
    rng = np.random.default_rng(5)
    deal = []
    for codec, rate, packing, units in streams:
        data = b"".join(units)
        gb = M.G726_GROUP_BYTES[rate] if codec == M.G726 else 1
        cuts = sorted(int(c) * gb for c in rng.integers(0, len(data) // gb + 1, 3))
        deal.append([data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])])
    got, states = run_batch(engine, streams, deal)
    for i in range(len(streams)):
        assert np.array_equal(np.concatenate(got[i]), np.concatenate(want[i][0])), streams[i][:3]
        assert states[i] == want[i][1], streams[i][:3]


# ---- bounds and limits ------------------------------------------------------------------------------------------------------------------

def raw_decode(engine, codec, rate, packing, data, out_cap, state):
    """sk_g72x_decode with a guarded output -> (status, out_len, text, the whole buffer: out_cap bytes then 64 guard bytes)"""
    from soundkit_amd._lib import lib
    src = np.frombuffer(bytes(data), np.uint8)
    out = np.full(out_cap + 64, 0xA5, np.uint8)
    n = C.c_size_t(99)
    text = C.create_string_buffer(256)
    rc = lib.sk_g72x_decode(engine._h, codec, rate, packing, src.ctypes.data, src.size, out.ctypes.data, out_cap, C.byref(n),
                            C.byref(state) if state is not None else None, text, 256)
    return rc, n.value, text.value.decode(), out


@gpu
@pytest.mark.parametrize("kind", [(M.G726, 16000, M.RIGHT, 333), (M.G726, 24000, M.LEFT, 3 * 111), (M.G726, 32000, M.LEFT, 333), (M.G726, 40000, M.RIGHT, 5 * 67),
                                  (M.G722, 0, 0, 333), (M.ULAW, 0, 0, 333)], ids=lambda k: "%d-%d-%d" % k[:3])
def test_an_output_one_byte_short_is_refused_and_nothing_is_written_past_the_end(engine, kind):
    from soundkit_amd import telephony
    codec, rate, packing, n = kind
    data = np.random.default_rng(9).integers(0, 256, n, dtype=np.uint8).tobytes()
    want = model_decode(codec, rate, packing, [data])
    need = want[0][0].size * 2
    assert need % 16 != 0 or rate in (24000, 40000)  # the end of the output is no 16-byte store's natural end (a group of 8 samples is one)
    state = telephony.new_state(codec)
    fresh = telephony.state_words(state) if state is not None else None
    rc, n_out, _, buf = raw_decode(engine, codec, rate or 32000, packing, data, need - 1, state)
    assert rc == -1 and n_out == 0 and (buf == 0xA5).all()
    assert state is None or telephony.state_words(state) == fresh
    rc, n_out, _, buf = raw_decode(engine, codec, rate or 32000, packing, data, need, state)
    assert rc == 0 and n_out == need and (buf[need:] == 0xA5).all()
    assert np.array_equal(np.frombuffer(buf[:need].tobytes(), "<i2"), want[0][0])
    assert state is None or telephony.state_words(state) == want[1]


@gpu
@pytest.mark.parametrize("kind", [(M.ULAW, 0, 262145, 262145, "G.711"), (M.G722, 0, 131073, 262146, "G.722"), (M.G726, 32000, 131073, 262146, "G.726"),
                                  (M.G726, 40000, 5 * 32769, 262152, "G.726")], ids=lambda k: "%s-%d" % (k[4], k[1]))
def test_a_call_beyond_the_scratch_is_refused_with_the_references_text(engine, kind):
    from soundkit_amd import telephony
    codec, rate, n, samples, name = kind
    rng = np.random.default_rng(3)
    state = telephony.new_state(codec)
    if state is not None:  # a state that is not the initial one
        engine.g72x_decode(codec, rng.integers(0, 256, 40, dtype=np.uint8).tobytes(), state, rate or 32000)
        before = telephony.state_words(state)
    rc, n_out, text, buf = raw_decode(engine, codec, rate or 32000, M.LEFT, bytes(n), 2 * samples, state)
    assert rc == telephony.ERR_STREAM and n_out == 0 and (buf == 0xA5).all()
    assert text == "Output buffer too small for %s decode: need %d, have 262144" % (name, samples)
    assert state is None or telephony.state_words(state) == before
    with pytest.raises(telephony.TelephonyError, match="need %d, have 262144" % samples):
        engine.g72x_decode(codec, bytes(n), state, rate or 32000)


@gpu
def test_exactly_the_scratch_is_taken(engine):
    data = np.random.default_rng(4).integers(0, 256, 131072, dtype=np.uint8).tobytes()  # 262 144 samples of G.726-32
    got = np.frombuffer(engine.g72x_decode(M.G726, data, None, 32000, M.RIGHT), "<i2")
    assert got.size == 262144
    head = model_decode(M.G726, 32000, M.RIGHT, [data[:2000]])[0][0]
    assert np.array_equal(got[:4000], head)


@gpu
def test_tables_that_do_not_add_up_are_refused(engine):
    import soundkit_amd
    from soundkit_amd import telephony
    st = telephony.new_state(M.G726)
    for entries, units in [([{"codec": M.G726, "rate": 24000, "n_units": 1, "state": st}], [bytes(4)]),  # no whole group
                           ([{"codec": M.G726, "rate": 12345, "n_units": 1, "state": st}], [bytes(4)]),
                           ([{"codec": 7, "n_units": 1}], [bytes(4)]),
                           ([{"codec": M.G722, "n_units": 2, "state": telephony.new_state(M.G722)}], [bytes(4)])]:
        with pytest.raises(soundkit_amd.SoundkitError) as exc:
            engine.g72x_decode_batch(entries, units)
        assert exc.value.status == -1
    assert telephony.state_words(st) == M.G726Core().words()


@gpu
@pytest.mark.parametrize("kind", [(M.G726, 16000, M.RIGHT, 333), (M.G726, 24000, M.LEFT, 3 * 111), (M.G726, 32000, M.LEFT, 333), (M.G726, 40000, M.RIGHT, 5 * 67),
                                  (M.G722, 0, 0, 333), (M.ULAW, 0, 0, 333), (M.ALAW, 0, 0, 17)], ids=lambda k: "%d-%d-%d" % k[:3])
def test_the_kernels_write_nothing_past_the_end_of_a_device_buffer(engine, kind):
    """sk_g72x_decode_dev: input and output in device memory, guard bytes in front of and behind the output.  What the kernels themselves
    store -- k_g726's pairs, k_g722_qmf's pairs, the G.711 expansion's 16-sample groups and its sample-by-sample rest -- stays inside."""
    import torch
    from soundkit_amd import telephony
    from soundkit_amd._lib import lib
    codec, rate, packing, n = kind
    data = np.random.default_rng(10).integers(0, 256, n, dtype=np.uint8)
    want = model_decode(codec, rate, packing, [data.tobytes()])
    need = want[0][0].size * 2
    src = torch.zeros((n + 15) // 16 * 16 + 16, dtype=torch.uint8, device="cuda")
    src[:n] = torch.from_numpy(data.copy()).cuda()
    buf = torch.full((256 + need + 256,), 0xA5, dtype=torch.uint8, device="cuda")  # the output begins 256 bytes in: 16-byte aligned
    assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    state = telephony.new_state(codec)
    got = C.c_size_t(0)
    torch.cuda.synchronize()
    rc = lib.sk_g72x_decode_dev(engine._h, codec, rate or 32000, packing, src.data_ptr(), n, buf.data_ptr() + 256, need - 1, C.byref(got),
                                C.byref(state) if state is not None else None, None, 0)
    assert rc == -1 and got.value == 0
    rc = lib.sk_g72x_decode_dev(engine._h, codec, rate or 32000, packing, src.data_ptr(), n, buf.data_ptr() + 256, need, C.byref(got),
                                C.byref(state) if state is not None else None, None, 0)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert rc == 0 and got.value == need
    assert (host[:256] == 0xA5).all() and (host[256 + need:] == 0xA5).all()
    assert np.array_equal(np.frombuffer(host[256:256 + need].tobytes(), "<i2"), want[0][0])
    assert state is None or telephony.state_words(state) == want[1]

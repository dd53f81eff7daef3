"""MPEG Layer I / II on the device: Mp3Decoder (sk_mp3_decoder_decode_*, no switch) and the batched stage call
(sk_mpa_decode_frames_*, csrc/mp12_synth.hip) against the float64 model of tests/mp12_model.py -- the reference's MP2 fixture and
streams written by tests/mp12_builder.py -- at the bounds tests/test_mp3_fixtures_gpu.py holds Layer III to: relative RMS below
1e-6, largest difference below 4e-6 of the peak; the integer outputs bit for bit through the reference's f32_to_i16 / f32_to_i32."""
import numpy as np
import pytest

import mp12_builder as B
import mp12_model as M
from oracle import oracle as O
from soundkit_amd import mp3
from test_mp12_cpu import CONFIGS, FIXTURE

pytestmark = pytest.mark.gpu
MAX = mp3.MAX_SAMPLES_PER_FRAME


def decode_chunks(dec, chunks, kind="i16", room=2 * MAX):
    """the reference tests' loop: one decode call per chunk, then empty input until nothing comes"""
    dtype = {"f32": np.float32, "i16": np.int16, "i32": np.int32}[kind]
    fn = getattr(dec, "decode_" + kind)
    out, scratch = [np.zeros(0, dtype)], np.zeros(room, dtype)
    for chunk in chunks:
        n = fn(chunk, scratch)
        out.append(scratch[:n].copy())
    while True:
        n = fn(b"", scratch)
        if n == 0:
            break
        out.append(scratch[:n].copy())
    return np.concatenate(out)


def pieces(data, size):
    return [data[i:i + size] for i in range(0, len(data), size)]


def assert_meets_the_model(got, want):
    assert got.shape == want.shape
    err = np.sqrt(np.mean((got.astype(np.float64) - want) ** 2)) / np.sqrt(np.mean(want ** 2))
    worst = np.abs(got - want).max() / np.abs(want).max()
    print("relative RMS %.3g, largest difference %.3g of the peak" % (err, worst))
    assert err < 1e-6, err
    assert worst < 4e-6, worst


@pytest.fixture(scope="module", autouse=True)
def synthesis_window(engine):
    """the bare stage call needs the engine's window D; a decoder handle would have set it (sk_mp3_decoder_create)"""
    mp3.set_synthesis_window(np.ctypeslib.as_array(mp3.iso_tables().window), engine)


@pytest.fixture(scope="module")
def fixture_bytes():
    return open(FIXTURE, "rb").read()


@pytest.fixture(scope="module")
def fixture_model(fixture_bytes):
    return M.Decoder().stream(fixture_bytes)


def test_the_fixture_through_mp3decoder(engine, fixture_bytes, fixture_model):
    dec = mp3.Mp3Decoder(engine=engine)
    try:
        got = decode_chunks(dec, [fixture_bytes], "f32", room=1 << 17).reshape(-1, 2)
        assert dec.sample_rate() == 48000 and dec.channels() == 2 and dec.frames_decoded() == 42 and dec.buffer_len() == 0
        dec.reset()
        got16 = decode_chunks(dec, [fixture_bytes], "i16", room=1 << 17).reshape(-1, 2)
        dec.reset()
        got32 = decode_chunks(dec, [fixture_bytes], "i32", room=1 << 17).reshape(-1, 2)
    finally:
        dec.close()
    assert got.shape == (42 * 1152, 2)
    assert_meets_the_model(got, fixture_model)
    assert np.array_equal(got16, O.pcm_convert("MP3_F32_TO_I16", got.reshape(-1)).reshape(-1, 2))
    assert np.array_equal(got32, O.pcm_convert("MP3_F32_TO_I32", got.reshape(-1)).reshape(-1, 2))


def test_chunk_invariance(engine, fixture_bytes):
    outs = []
    for chunks in ([fixture_bytes], pieces(fixture_bytes, 113), pieces(fixture_bytes, 4096)):
        dec = mp3.Mp3Decoder(engine=engine)
        try:
            outs.append(decode_chunks(dec, chunks))
            assert dec.frames_decoded() == 42 and dec.sample_rate() == 48000 and dec.channels() == 2
        finally:
            dec.close()
    assert outs[0].size == 42 * 1152 * 2
    assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()


def test_stray_bytes_in_front_do_not_settle_the_layer(engine, fixture_bytes):
    """Garbage in front of the stream that holds a Layer III-looking header (and a lone Layer II-looking one): neither is a confirmed
    frame, so neither settles the stream's layer, at any chunking -- the decode is the clean stream's"""
    dec = mp3.Mp3Decoder(engine=engine)
    try:
        clean = decode_chunks(dec, [fixture_bytes])
    finally:
        dec.close()
    junk = bytes(range(1, 40)) + b"\xff\xfb\x90\x00" + bytes(57) + b"\xff\xfd\xa4\x04" + bytes(range(3, 90))
    for chunks in ([junk + fixture_bytes], pieces(junk + fixture_bytes, 113), pieces(junk + fixture_bytes, 31), [junk[:45], junk[45:] + fixture_bytes]):
        dec = mp3.Mp3Decoder(engine=engine)
        try:
            got = decode_chunks(dec, chunks)
            assert dec.frames_decoded() == 42 and dec.sample_rate() == 48000
        finally:
            dec.close()
        assert got.tobytes() == clean.tobytes()


def builder_stream(name, n_frames=3):
    rng = np.random.default_rng(1000 + sum(name.encode()))
    frames = [B.random_frame(rng, *CONFIGS[name])[0] for _ in range(n_frames)]
    return frames


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_builder_streams(engine, name):
    """three frames, fed in two calls cut inside the second frame: the FIFO is carried across frames and across calls"""
    frames = builder_stream(name)
    data = b"".join(frames)
    want = M.Decoder().stream(data)
    h = M.parse_header(data[:4])
    assert want.shape == (3 * h["samples_per_channel"], h["channels"])
    cut = len(frames[0]) + len(frames[1]) // 2
    dec = mp3.Mp3Decoder(engine=engine)
    try:
        got = decode_chunks(dec, [data[:cut], data[cut:]], "f32").reshape(-1, h["channels"])
        assert dec.frames_decoded() == 3 and dec.sample_rate() == h["sample_rate"] and dec.channels() == h["channels"]
    finally:
        dec.close()
    assert_meets_the_model(got, want)


def records_of(frames):
    out = []
    for f in frames:
        rc, info = mp3.mpa_parse_header(f[:4])
        assert rc == 0
        rc, rec = mp3.mpa_parse_frame(f, info)
        assert rc == 0
        out.append((rec, f))
    return out


def test_mixed_batch(engine, fixture_bytes):
    """one launch over two Layer II streams of different tables, a mono LSF stream and a Layer I stream, their frames interleaved:
    every stream gets what it gets alone"""
    streams = {
        "fixture": (2, [fixture_bytes[576 * i:576 * i + 576] for i in range(3)]),
        "joint": (2, builder_stream("joint bound 4")),
        "lsf mono": (1, builder_stream("LSF mono 24k 64k")),
        "layer one": (2, builder_stream("Layer I stereo 48k 384k")),
    }
    alone = {}
    for name, (ch, frames) in streams.items():
        sid = engine.open_stream(48000, ch)
        try:
            recs, n, buf = mp3.mpa_pack_frames(records_of(frames))
            rc, pcm, st = mp3.mpa_decode_frames(recs, [sid] * n, n, buf, engine)
            assert rc == 0 and not st.any()
            alone[name] = pcm.copy()
        finally:
            engine.close_stream(sid)
    sids = {name: engine.open_stream(48000, ch) for name, (ch, _) in streams.items()}
    try:
        order = [(name, i) for i in range(3) for name in streams]  # frame 0 of every stream, then frame 1, ...
        recs, n, buf = mp3.mpa_pack_frames(records_of([streams[name][1][i] for name, i in order]))
        rc, pcm, st = mp3.mpa_decode_frames(recs, [sids[name] for name, _ in order], n, buf, engine)
        assert rc == 0 and not st.any()
        at, got = 0, {name: [] for name in streams}
        for name, i in order:
            size = alone[name].size // 3
            got[name].append(pcm[at:at + size])
            at += size
        assert at == pcm.size
        for name in streams:
            assert np.concatenate(got[name]).tobytes() == alone[name].tobytes(), name
    finally:
        for sid in sids.values():
            engine.close_stream(sid)


def test_a_record_that_does_not_add_up_never_reaches_the_kernel(engine, fixture_bytes):
    """the stage call checks classes, widths and bounds against byte_len: such a frame is dropped, its neighbours are not"""
    frames = [fixture_bytes[576 * i:576 * i + 576] for i in range(3)]
    sid = engine.open_stream(48000, 2)
    try:
        recs, n, buf = mp3.mpa_pack_frames(records_of(frames))
        rc, clean, st = mp3.mpa_decode_frames(recs, [sid] * n, n, buf, engine, s16=True)
        assert rc == 0 and not st.any() and clean.size == 3 * 2304
        engine.reset_stream(sid)
        recs[1].granule_bits += 1         # the samples would no longer be where the classes say
        rc, pcm, st = mp3.mpa_decode_frames(recs, [sid] * n, n, buf, engine, s16=True)
        assert rc == 0 and st.tolist() == [0, -304, 0] and pcm.size == 2 * 2304
        assert np.array_equal(pcm[:2304], clean[:2304])
        engine.reset_stream(sid)
        recs[1].granule_bits -= 1
        recs[2].byte_len = 400            # the last code would end beyond the frame
        rc, pcm, st = mp3.mpa_decode_frames(recs, [sid] * n, n, buf, engine, s16=True)
        assert rc == 0 and st.tolist() == [0, 0, -304] and np.array_equal(pcm, clean[:2 * 2304])
    finally:
        engine.close_stream(sid)


def test_full_device(engine, fixture_bytes):
    """2048 streams x the fixture's first two frames in ONE launch: every stream's bytes equal stream 0's and the single-stream decode"""
    n_streams = 2048
    frames = records_of([fixture_bytes[:576], fixture_bytes[576:1152]])
    sid = engine.open_stream(48000, 2)
    try:
        recs, n, buf = mp3.mpa_pack_frames(frames)
        rc, single, st = mp3.mpa_decode_frames(recs, [sid] * n, n, buf, engine, s16=True)
        assert rc == 0 and not st.any() and single.size == 2 * 2304 and single.any()
    finally:
        engine.close_stream(sid)
    sids = [engine.open_stream(48000, 2) for _ in range(n_streams)]
    try:
        # the two frames' bytes once; every stream's records point at them
        many = (type(recs[0]) * (2 * n_streams))()
        for s in range(n_streams):
            many[2 * s], many[2 * s + 1] = recs[0], recs[1]
        ids = np.repeat(np.asarray(sids, np.uint32), 2)
        rc, pcm, st = mp3.mpa_decode_frames(many, ids, 2 * n_streams, buf, engine, s16=True)
        assert rc == 0 and not st.any()
        pcm = pcm.reshape(n_streams, 2 * 2304)
        assert np.array_equal(pcm[0], single)
        assert (pcm == pcm[0]).all()
    finally:
        for sid in sids:
            engine.close_stream(sid)

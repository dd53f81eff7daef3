"""The Vorbis decode stage on the GPU (csrc/vorbis_decode.hip through sk_vorbis_entropy_decode, sk_vorbis_decode_packets, VorbisDecoder
and VorbisPacketDecoder) against tests/vorbis_model.py: the entropy stage bit for bit, the f32 PCM within four times the float32
model's own distance from float64, the s16 of the Ogg fixture within one step of the reference's recording.

The measured distances are in profiles/vorbis.md."""
import wave

import numpy as np
import pytest

import vorbis_cases as CASES
import vorbis_model as M

pytestmark = pytest.mark.gpu

OK = 0


def product_setup(case):
    from soundkit_amd import vorbis
    return vorbis.Setup(vorbis.parse_ident(case.headers[0]), case.headers[2])


@pytest.fixture(scope="module")
def setups():
    return {c.name: product_setup(c) for c in CASES.all_cases()}


@pytest.fixture(scope="module")
def staged(engine, setups):
    """every case's packets, well-formed and damaged, through ONE sk_vorbis_entropy_decode: 200 packets of seven setups, so that the
    lanes of a wave belong to different streams -> {name: ([packets], [device dicts])}"""
    groups, names = [], []
    for k, c in enumerate(CASES.all_cases()):
        packets = list(c.packets) + CASES.damaged_packets(c, 7 + k)
        groups.append((setups[c.name], packets))
        names.append((c.name, packets))
    assert sum(len(p) for _, p in names) > 65
    got = engine.vorbis_entropy_decode(groups)
    return {name: (packets, rows) for (name, packets), rows in zip(names, got)}


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", [c.name for c in CASES.all_cases()])
def test_entropy_stage_equals_the_model_bit_for_bit(staged, name):
    case = next(c for c in CASES.all_cases() if c.name == name)
    packets, rows = staged[name]
    statuses = set()
    for i, (p, d) in enumerate(zip(packets, rows)):
        want = M.entropy_decode(case.setup, p, np.float32)
        statuses.add(want.status)
        assert d["status"] == want.status, (name, i, d["status"], want.status)
        if want.status != OK:
            assert d["blocksize"] == 0 and d["residue"].size == 0
            continue
        assert (d["mode"], d["blockflag"], d["prev_flag"], d["next_flag"], d["blocksize"]) == (want.mode, want.blockflag, want.prev, want.next, want.n), (name, i)
        assert d["used"] == want.used, (name, i, d["used"], want.used)
        assert np.array_equal(d["final_y"], want.final_y[:, :65]), (name, i)
        assert np.array_equal(d["step2"], want.step2), (name, i)
        assert d["residue"].shape == want.residue.shape and np.array_equal(bits(d["residue"]), bits(want.residue)), (name, i)
    assert {M.ST_NOT_AUDIO, M.ST_SHORT, OK} <= statuses


def test_built_streams_reach_every_path(staged):
    """what the random packets are for: unused channels, channels that end inside a floor, residues cut by the packet's end"""
    used = [u for name, (packets, rows) in staged.items() if name not in ("ogg", "webm") for d in rows if d["status"] == OK for u in d["used"]]
    assert 0 in used and 1 in used
    assert any(d["status"] == M.ST_SHORT for _, rows in staged.values() for d in rows)


def rel_rms(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)) / np.sqrt(np.mean(b.astype(np.float64) ** 2)))


@pytest.fixture(scope="module")
def pcm_f32(engine, setups):
    """every case's well-formed packets through ONE sk_vorbis_decode_packets, f32 out -> {name: [(status, [frames][ch])]}"""
    from soundkit_amd import vorbis
    cases = CASES.all_cases()
    got = engine.vorbis_decode_packets([(vorbis.StreamState(setups[c.name]), c.packets) for c in cases], as_f32=True)
    return {c.name: rows for c, rows in zip(cases, got)}


@pytest.mark.parametrize("name", [c.name for c in CASES.all_cases()])
def test_f32_pcm_within_four_times_the_float32_models_distance(pcm_f32, name):
    case = next(c for c in CASES.all_cases() if c.name == name)
    m64, m32 = CASES.model_pcm(case, np.float64), CASES.model_pcm(case, np.float32)
    worst_dev = worst_model = 0.0
    for i, ((status, pcm), (s64, want), (_, w32)) in enumerate(zip(pcm_f32[name], m64, m32)):
        assert status == s64 == OK
        assert pcm.shape == want.T.shape, (name, i, pcm.shape, want.T.shape)  # the first packet: no frames; then prev / 4 + this / 4
        if i == 0:
            assert pcm.shape[0] == 0
            continue
        if not np.any(want):
            assert not np.any(pcm)
            continue
        dev, model = rel_rms(pcm.T, want), rel_rms(w32, want)
        worst_dev, worst_model = max(worst_dev, dev), max(worst_model, model)
        assert dev <= 4 * model, (name, i, dev, model)
    print("%s: relative RMS against float64, worst packet: device %.3g, float32 model %.3g" % (name, worst_dev, worst_model))


def test_window_transitions_and_sample_counts(pcm_f32):
    for case in CASES.built_cases():
        bs = (case.ident["blocksize_0"], case.ident["blocksize_1"])
        sizes = [bs[f] for f in CASES.FLAGS]
        got = [pcm.shape[0] for _, pcm in pcm_f32[case.name]]
        assert got == [0] + [sizes[i - 1] // 4 + sizes[i] // 4 for i in range(1, len(sizes))], case.name
    assert {(a, b) for a, b in zip(CASES.FLAGS, CASES.FLAGS[1:])} == {(0, 0), (0, 1), (1, 1), (1, 0)}


def test_packets_dealt_over_calls_give_the_same_samples(engine, setups, pcm_f32):
    """the overlap and the previous block size carried by the caller: one packet per call, and 3 + the rest, equal one call bit for bit"""
    from soundkit_amd import vorbis
    for case in CASES.built_cases()[:3] + CASES.fixture_cases()[1:]:
        whole = np.concatenate([pcm for _, pcm in pcm_f32[case.name]])
        for cut in (1, 3):
            st, pieces = vorbis.StreamState(setups[case.name]), []
            for at in range(0, len(case.packets), cut):
                pieces += [pcm for _, pcm in engine.vorbis_decode_packets([(st, case.packets[at:at + cut])], as_f32=True)[0]]
            assert np.array_equal(bits(np.concatenate(pieces)), bits(whole)), (case.name, cut)


def test_a_damaged_packet_costs_its_own_samples_and_the_overlap_that_follows(engine, setups):
    from soundkit_amd import vorbis
    case = CASES.built_cases()[0]
    bad = bytes([case.packets[3][0] | 1]) + case.packets[3][1:]
    packets = case.packets[:3] + [bad, b""] + case.packets[4:]
    got = engine.vorbis_decode_packets([(vorbis.StreamState(setups[case.name]), packets)], as_f32=True)[0]
    want = CASES.model_pcm(case, np.float32, packets)
    assert [s for s, _ in got] == [s for s, _ in want] == [0, 0, 0, M.ST_NOT_AUDIO, M.ST_SHORT, 0, 0, 0]
    for (_, pcm), (s, w) in zip(got, want):
        assert pcm.shape[0] == (0 if w is None else w.shape[1])
        if w is not None and w.size:
            # against the float32 model: both carry f32 rounding of some 1e-7 (the exact bound is the test above's); overlapping with the
            # wrong packet's half would show as an error of order 1
            assert rel_rms(pcm.T, w.astype(np.float64)) < 1e-5


def test_ogg_fixture_s16_against_the_recording(engine):
    """VorbisDecoder over the file in pieces of 641 bytes and whole: the same bytes, the recording's length, every sample within one step"""
    from soundkit_amd import vorbis
    data = open(CASES.OGG, "rb").read()
    w = wave.open(CASES.RECORDING)
    rec = np.frombuffer(w.readframes(w.getnframes()), "<i2")
    outs = []
    for piece in (641, len(data)):
        dec, got = vorbis.VorbisDecoder(engine=engine), []
        for at in range(0, len(data), piece):
            a = dec.add(data[at:at + piece])
            if a is not None:
                assert (a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 8000)
                got.append(np.frombuffer(a.data.tobytes(), "<i2"))
        a = dec.finish()
        if a is not None:
            got.append(np.frombuffer(a.data.tobytes(), "<i2"))
        outs.append(np.concatenate(got))
    assert np.array_equal(outs[0], outs[1])
    assert outs[0].size == rec.size == 23680
    d = np.abs(outs[0].astype(np.int32) - rec.astype(np.int32))
    print("samples one step from the recording: %d of %d (%.2e)" % ((d > 0).sum(), d.size, (d > 0).mean()))
    assert d.max() <= 1


def test_webm_packets_through_the_packet_decoder(engine):
    from soundkit_amd import vorbis
    case = CASES.fixture_cases()[1]
    dec = vorbis.VorbisPacketDecoder(engine=engine)
    assert [dec.decode_packet(h) for h in case.headers] == [None, None, None]
    assert (dec.sample_rate(), dec.channels()) == (44100, 2)
    want = CASES.model_pcm(case, np.float64)
    for i, (p, (_, w)) in enumerate(zip(case.packets, want)):
        got = dec.decode_packet(p)
        assert got.dtype == np.int16 and got.size == w.size
        if w.size:
            assert np.abs(got.reshape(-1, 2).T.astype(np.int32) - M.to_s16(w).astype(np.int32)).max() <= 1, i


def test_decoder_objects_capacity_and_refusals(engine):
    """sk_vorbis_decoder_*: an output too small loses nothing (the next call delivers), a first packet that is not a Vorbis
    identification header ends the decoder with the parser's text, and so does a damaged page with the Ogg parser's"""
    from soundkit_amd import SoundkitError, vorbis
    data = open(CASES.OGG, "rb").read()
    whole = vorbis.VorbisDecoder(engine=engine)
    want = np.frombuffer(whole.add(data).data.tobytes(), "<i2")
    assert whole.finish() is None and want.size == 23680
    small = vorbis.VorbisDecoder(engine=engine)
    small._out = np.zeros(16, np.int16)
    assert np.array_equal(np.frombuffer(small.add(data).data.tobytes(), "<i2"), want) and small.finish() is None
    other = M.ogg_page(2, 0, 5, 0, [8], b"OpusHead") + M.ogg_page(4, 0, 5, 1, [1], b"\x00")
    dec = vorbis.VorbisDecoder(engine=engine)
    with pytest.raises(SoundkitError) as e:
        dec.add(other)
    assert e.value.status == vorbis.ERR_STREAM and "not a Vorbis identification header" in str(e.value)
    with pytest.raises(SoundkitError):
        dec.add(b"")
    bad = bytearray(data)
    bad[5000] ^= 0x10
    dec = vorbis.VorbisDecoder(engine=engine)
    with pytest.raises(SoundkitError) as e:
        dec.add(bytes(bad))
    assert "Ogg CRC mismatch on page" in str(e.value)
    pd = vorbis.VorbisPacketDecoder(engine=engine)
    assert pd.sample_rate() is None
    with pytest.raises(SoundkitError) as e:
        pd.decode_packet(b"\x05vorbis")
    assert "not a Vorbis identification header" in str(e.value)
    case = CASES.fixture_cases()[0]
    assert [pd.decode_packet(h) for h in case.headers] == [None, None, None] and pd.decode_packet(case.packets[0]).size == 0
    with pytest.raises(SoundkitError) as e:
        pd.decode_packet(b"\x01")
    assert e.value.status == vorbis.NOT_AUDIO
    assert pd.decode_packet(case.packets[1]).size == 256  # the decoder goes on: the overlap is as the first packet left it

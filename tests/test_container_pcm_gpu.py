"""Container PCM and FLAC-in-MP4 on the GPU: SK_AIFF_F64LE in k_aiff_elem against numpy's float64 -> float32 and against SK_AIFF_F64BE on
the swapped bytes; mp4.decode_file on the MOV fixtures against their recorded hashes, against the raw-PCM path on the same payload under
output options, and twin against twin; the edit trim on runs of frames; FLAC-in-MP4 files built from the FLAC fixtures against the native
FLAC decode."""
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import mp4_builder as B
import mp4_pcm_builder as P
from soundkit_amd import SoundkitError, engine as E, flac, mp4, pipeline

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MOV = os.path.join(HERE, "golden", "mov_pcm")
HASHES = json.load(open(os.path.join(MOV, "pcm_hashes.json")))
FLAC = os.path.join(HERE, "golden", "flac")
DOWN = pipeline.DecodeOptions(16, 16000, 1)


def joined(audio):
    return b"".join(a.data.tobytes() for a in audio)


def mov(name):
    return open(os.path.join(MOV, name), "rb").read()


def payload_of(data):
    index = mp4.Mp4Index.from_file(data)
    return b"".join(index.packet_bytes(data))


def little(payload, width):
    return np.frombuffer(payload, np.uint8).reshape(-1, width)[:, ::-1].tobytes()


# ---- SK_AIFF_F64LE ---------------------------------------------------------------------------------------------------------------------

def f64_values(n):
    """ordinary values mixed with +-0, ties at the rounding bit, results that are f32 subnormals, overflow to infinity, and NaN"""
    f32 = lambda b: np.array([b], np.uint32).view(np.float32)[0].astype(np.float64)
    one, ulp = 1.0, 2.0 ** -23
    special = [0.0, -0.0, one + ulp / 2, one + 3 * ulp / 2, one + ulp / 2 + 2.0 ** -50, one + ulp / 2 - 2.0 ** -50, -(one + ulp / 2), 2.0 - 2.0 ** -25,
               2.0 ** -149, 2.0 ** -150, 2.0 ** -150 + 2.0 ** -190, 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149, -(2.0 ** -151), 2.0 ** -126 - 2.0 ** -150,
               3.0 * 2.0 ** -140, 5e-324, -5e-324, f32(0x7f7fffff), f32(0x7f7fffff) + 2.0 ** 102, f32(0x7f7fffff) + 2.0 ** 103, 2.0 ** 128, -1e300,
               float("inf"), float("-inf"), float("nan")]
    rng = np.random.default_rng(64 + n)
    v = rng.uniform(-1.5, 1.5, n)
    at = rng.permutation(n)[:min(n, len(special))]
    order = rng.permutation(len(special))[:len(at)]
    v[at] = np.array(special)[order]
    tail = n % 16  # the lanes that go sample by sample: a tie, a subnormal result, an overflow, a NaN and the rest of TAIL, from the end backwards
    if tail:
        v[n - tail:] = np.array(TAIL)[:tail][::-1]
    return v


_ULP = 2.0 ** -23
TAIL = [float("nan"), 1.0 + _ULP / 2, 2.0 ** -150 + 2.0 ** -190, 2.0 ** 128, -0.0, 1.0 + 3 * _ULP / 2, 1.5 * 2.0 ** -149, -1e300, 2.0 - 2.0 ** -25,
        float("-inf"), 5e-324, -(1.0 + _ULP / 2), 2.0 ** -126 - 2.0 ** -150, 0.0, 2.5 * 2.0 ** -149]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 15, 16, 17, 4099])
def test_f64le_is_numpy_rounding_and_f64be_on_the_swapped_bytes(engine, n):
    v = f64_values(n)
    with np.errstate(over="ignore", invalid="ignore"):
        want = v.astype("<f4").tobytes()
    got = engine.aiff_decode(E.AIFF_F64LE, 1, v.astype("<f8").tobytes())
    assert got == want
    assert got == engine.aiff_decode(E.AIFF_F64BE, 1, v.astype(">f8").tobytes())


def test_f64le_tail_lanes_see_every_special_value(engine):
    """47 = 2 x 16 + 15 samples: all fifteen of TAIL lie in the per-sample tail"""
    v = f64_values(47)
    assert np.isnan(v[-1]) and v[-2] == 1.0 + _ULP / 2 and np.array_equal(v[32:][::-1][1:], np.array(TAIL)[1:])
    with np.errstate(over="ignore", invalid="ignore"):
        want = v.astype("<f4").tobytes()
    assert engine.aiff_decode(E.AIFF_F64LE, 1, v.astype("<f8").tobytes()) == want
    assert engine.aiff_decode(E.AIFF_F64BE, 1, v.astype(">f8").tobytes()) == want


def test_f64le_keeps_channels_interleaved_and_refuses_half_a_sample(engine):
    v = f64_values(2 * 37)
    with np.errstate(over="ignore", invalid="ignore"):
        assert engine.aiff_decode(E.AIFF_F64LE, 2, v.astype("<f8").tobytes()) == v.astype("<f4").tobytes()
    with pytest.raises(SoundkitError):
        engine.aiff_decode(E.AIFF_F64LE, 1, bytes(12))
    with pytest.raises(SoundkitError):
        engine.aiff_decode(E.AIFF_F64LE + 1, 1, bytes(8))


# ---- the MOV fixtures ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sched(engine):
    s = pipeline.BatchScheduler(engine, max_streams=8)
    yield s
    s.close()


def raw_path(sched, payload, fmt, options):
    """the payload through the scheduler's raw-PCM stream of that format, to the end"""
    h = sched.spawn_raw_pcm(pipeline.RawPcmFormat(48000, 2, fmt), options)
    out = []
    try:
        for piece in (payload, b""):
            while True:
                try:
                    h.send(piece)
                    break
                except pipeline.DecodeError as e:
                    assert e.kind == "InputBufferFull"
                    out.append(h.recv())
        while True:
            a = h.recv()
            if a is None:
                break
            out.append(a)
    finally:
        h.cancel()
    assert all(not isinstance(a, Exception) for a in out), out
    return [a for a in out if a is not None]


@pytest.fixture(scope="module")
def decoded(engine, sched):
    """every fixture once: (config, audio with no options, audio at 16 kHz mono 16-bit)"""
    out = {}
    for name in sorted(HASHES["mov_pcm"]):
        config, plain = mp4.decode_file(mov(name), engine=engine)
        _, down = mp4.decode_file(mov(name), DOWN, scheduler=sched, engine=engine)
        out[name] = (config, plain, down)
    return out


@pytest.mark.parametrize("name", sorted(HASHES["mov_pcm"]))
def test_decode_file_without_options_keeps_the_files_bytes(decoded, name):
    want = HASHES["mov_pcm"][name]
    config, audio, _ = decoded[name]
    payload = payload_of(mov(name))
    assert [len(a.data) // (a.channel_count * a.bits_per_sample // 8) for a in audio] == [4096, 704]
    if want["bits"] == 64:  # rounded to f32 little-endian on the GPU
        with np.errstate(over="ignore", invalid="ignore"):
            rounded = np.frombuffer(payload, ">f8" if want["big_endian"] else "<f8").astype("<f4").tobytes()
        assert joined(audio) == rounded
        assert all((a.bits_per_sample, a.audio_format.name, a.endianness.name) == (32, "PCMFloat", "LittleEndian") for a in audio)
        return
    assert joined(audio) == payload
    canonical = little(payload, want["bits"] // 8) if want["big_endian"] else payload
    assert hashlib.sha256(canonical).hexdigest() == want["sha256"]
    for a in audio:
        assert (a.bits_per_sample, a.channel_count, a.sampling_rate) == (want["bits"], 2, 48000)
        assert a.audio_format.name == ("PCMFloat" if want["float"] else "PCMSigned")
        assert a.endianness.name == ("BigEndian" if want["big_endian"] else "LittleEndian")


@pytest.mark.parametrize("name", sorted(HASHES["mov_pcm"]))
def test_output_options_are_the_raw_pcm_path_on_the_same_payload(decoded, sched, name):
    want = HASHES["mov_pcm"][name]
    _, _, down = decoded[name]
    payload = payload_of(mov(name))
    canonical = little(payload, want["bits"] // 8) if want["big_endian"] else payload
    if want["bits"] == 64:
        with np.errstate(over="ignore", invalid="ignore"):
            canonical = np.frombuffer(canonical, "<f8").astype("<f4").tobytes()
    fmt = E.FMT_F32LE if want["float"] else {24: E.FMT_S24LE, 32: E.FMT_S32LE}[want["bits"]]
    ref = raw_path(sched, canonical, fmt, DOWN)
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 16000) for a in down)
    assert joined(down) == joined(ref) and len(joined(down)) >= 2 * 1500


@pytest.mark.parametrize("kind", ["s24", "s32", "f32", "f64"])
def test_byte_order_twins_decode_alike(decoded, kind):
    be, le = decoded["pcm-%sbe.mov" % kind], decoded["pcm-%sle.mov" % kind]
    assert joined(be[2]) == joined(le[2])
    if kind == "f64":
        assert joined(be[1]) == joined(le[1])
    else:
        assert little(joined(be[1]), int(kind[1:]) // 8) == joined(le[1])


def test_other_widths_are_refused(engine):
    data = P.movie(P.sound_entry(b"sowt", 0, 2, 8), [bytes(40)], sample_size=2)
    with pytest.raises(SoundkitError, match="unsupported container PCM sample depth: 8"):
        mp4.decode_file(data, engine=engine)
    data = P.movie(P.sound_entry(b"lpcm", 2, 2, 64, v2=dict(flags=P.SIGNED | P.PACKED)), [bytes(160)], sample_size=16)
    with pytest.raises(SoundkitError, match="unsupported container PCM sample depth: 64"):
        mp4.decode_file(data, engine=engine)


def test_the_edit_keeps_the_frames_the_index_trim_gives(engine):
    frames = np.arange(2 * 6000, dtype="<i2").tobytes()
    data = P.movie(P.sound_entry(b"sowt", 0, 2, 16), [frames[:4 * 5000], frames[4 * 5000:]], sample_size=4, edit=[(60, 1000)], movie_timescale=600)
    index = mp4.Mp4Index.from_file(data)
    kept = [index.trim(i, d, 48000) for i, (_, _, d, _) in enumerate(index.samples)]
    assert kept == [(1000, 3096), (0, 904), (0, 800)]  # runs of 4096, 904 (the chunk's end) and 1000 frames; 4800 frames from frame 1000
    _, audio = mp4.decode_file(data, engine=engine)
    assert [len(a.data) // 4 for a in audio] == [3096, 904, 800]
    assert joined(audio) == frames[4 * 1000:4 * 5800]
    f64 = np.linspace(-1, 1, 2 * 6000)
    data = P.movie(P.sound_entry(b"fl64", 0, 2, 16, children=P.enda(1)), [f64.astype("<f8").tobytes()], sample_size=16, edit=[(60, 1000)], movie_timescale=600)
    _, audio = mp4.decode_file(data, engine=engine)
    assert joined(audio) == f64.astype("<f4").tobytes()[8 * 1000:8 * 5800]


# ---- FLAC in MP4 -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def native(engine):
    """the native FLAC decode of the two fixtures, as the little-endian PCM of their width"""
    out = {}
    for bits in (16, 24):
        data = open(os.path.join(FLAC, "A_Tusk_is_used_to_make_costly_gifts_%dbit.flac" % bits), "rb").read()
        rc, found, used = flac.scan(data, None, final=True)  # the fixtures are frames alone: no marker, no STREAMINFO
        assert rc == 0 and used == len(data) and len(found) == 11
        pcm, status = flac.decode_frames([(f, data[f["offset"]:f["offset"] + f["frame_bytes"]]) for f in found], engine)
        assert not any(status)
        out[bits] = (data, pcm)
    return out


@pytest.mark.parametrize("form", ["dfla", "bare", "stream"])
@pytest.mark.parametrize("bits", [16, 24])
def test_flac_in_mp4_is_the_native_flac_decode(engine, native, bits, form):
    data, want = native[bits]
    file, frames, blocks, first = P.flac_in_mp4(data, form, layout="mdat_first" if form == "bare" else "moov_first")
    config, audio = mp4.decode_file(file, engine=engine)
    assert config.codec == "flac" and len(audio) == len(frames) == 11
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (bits, first["channels"], first["sample_rate"]) for a in audio)
    assert [len(a.data) // (first["channels"] * bits // 8) for a in audio] == blocks
    assert joined(audio) == want and len(want) == 45056 * first["channels"] * bits // 8


def test_flac_in_mp4_under_an_edit_and_options(engine, native, sched):
    data, want = native[16]
    file, _, _, first = P.flac_in_mp4(data, "dfla", edit=[(600, 5000)])
    _, audio = mp4.decode_file(file, engine=engine)  # one second (600 / 600) from frame 5000
    width = 2 * first["channels"]
    assert joined(audio) == want[width * 5000:width * (5000 + first["sample_rate"])]
    _, down = mp4.decode_file(file, pipeline.DecodeOptions(16, 8000, 1), scheduler=sched, engine=engine)
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 8000) for a in down) and len(joined(down)) >= 2 * 7500


def test_a_configuration_that_holds_frames_is_refused(engine, native):
    data, _ = native[16]
    info, frames, blocks, first = P.flac_frames(data)
    entry = P.sound_entry(b"fLaC", 0, first["channels"], 16, first["sample_rate"],
                          B.box(b"dfLa", b"fLaC" + bytes([0x80, 0, 0, 34]) + info + frames[0] + frames[1]))
    file = P.movie(entry, [frames[2]], sizes=[[len(frames[2])]], durations=[[blocks[2]]], timescale=first["sample_rate"])
    with pytest.raises(SoundkitError, match="MP4 FLAC configuration unexpectedly contained audio frames"):
        mp4.decode_file(file, engine=engine)


# ---- CAF -------------------------------------------------------------------------------------------------------------------------------

CAF = os.path.join(HERE, "golden", "caf_pcm")


def caf_file(name):
    return open(os.path.join(CAF, name), "rb").read()


@pytest.mark.parametrize("name", sorted(HASHES["caf_pcm"]))
def test_caf_decode_file_keeps_the_files_bytes_and_takes_the_raw_pcm_path(engine, sched, name):
    from soundkit_amd import caf
    want = HASHES["caf_pcm"][name]
    data = caf_file(name)
    index, audio = caf.decode_file(data, engine=engine)
    payload = b"".join(index.packet_bytes(data))
    canonical = little(payload, want["bits"] // 8) if want["big_endian"] else payload
    assert hashlib.sha256(canonical).hexdigest() == want["sha256"]
    assert [len(a.data) // (a.channel_count * a.bits_per_sample // 8) for a in audio] == [4096, 704]
    if want["bits"] == 64:
        with np.errstate(over="ignore", invalid="ignore"):
            canonical = np.frombuffer(canonical, "<f8").astype("<f4").tobytes()
        assert joined(audio) == canonical
        assert all((a.bits_per_sample, a.audio_format.name, a.endianness.name) == (32, "PCMFloat", "LittleEndian") for a in audio)
    else:
        assert joined(audio) == payload
        assert all((a.bits_per_sample, a.audio_format.name, a.endianness.name) ==
                   (want["bits"], "PCMFloat" if want["float"] else "PCMSigned", "BigEndian" if want["big_endian"] else "LittleEndian") for a in audio)
    _, down = caf.decode_file(data, DOWN, scheduler=sched, engine=engine)
    fmt = E.FMT_F32LE if want["float"] else {16: E.FMT_S16LE, 24: E.FMT_S24LE, 32: E.FMT_S32LE}[want["bits"]]
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 16000) for a in down)
    assert joined(down) == joined(raw_path(sched, canonical, fmt, DOWN))


def test_caf_and_mov_twins_of_one_payload_decode_alike(engine, sched, decoded):
    from soundkit_amd import caf
    for caf_name, mov_name in (("pcm-s24le.caf", "pcm-s24be.mov"), ("pcm-s32be.caf", "pcm-s32le.mov"), ("pcm-f32le.caf", "pcm-f32be.mov"),
                               ("pcm-f64be.caf", "pcm-f64le.mov")):
        _, down = caf.decode_file(caf_file(caf_name), DOWN, scheduler=sched, engine=engine)
        assert joined(down) == joined(decoded[mov_name][2]), caf_name


def test_caf_alac_is_what_decode_caf_gives(engine):
    from soundkit_amd import alac, caf
    data = open(os.path.join(HERE, "golden", "alac", "A_Tusk_is_used_to_make_costly_gifts.caf"), "rb").read()
    _, want = alac.decode_caf(data, engine=engine)
    index, got = caf.decode_file(data, engine=engine)
    assert index.codec == "alac" and [a.data.tobytes() for a in got] == [a.data.tobytes() for a in want] and len(got) > 1


# ---- decode_audio_file -----------------------------------------------------------------------------------------------------------------

def test_decode_audio_file_sends_each_kind_of_input_where_the_reference_does(engine, sched, decoded):
    import soundkit_amd
    from soundkit_amd import caf, ts, webm

    def run(data, options=None):
        return soundkit_amd.decode_audio_file(data, options, scheduler=sched, engine=engine)

    with pytest.raises(SoundkitError, match="media file is empty"):
        run(b"")
    got = run(mov("pcm-s24be.mov"))  # `mdat` first, `moov` last: what spawn() cannot take
    assert (got.container, got.selected_track.codec) == ("mp4", "pcm") and joined(got.frames) == joined(decoded["pcm-s24be.mov"][1])
    prefix, moved = B.box(b"free", bytes(20)) + B.box(b"wide", b""), bytearray(mov("pcm-f64le.mov"))  # behind free / wide boxes, with options
    at = moved.find(b"stco")
    for k in range(struct.unpack_from(">I", moved, at + 8)[0]):  # every chunk lies len(prefix) bytes further on
        struct.pack_into(">I", moved, at + 12 + 4 * k, struct.unpack_from(">I", moved, at + 12 + 4 * k)[0] + len(prefix))
    got = run(prefix + bytes(moved), DOWN)
    assert got.container == "mp4" and joined(got.frames) == joined(decoded["pcm-f64le.mov"][2])
    got = run(caf_file("pcm-s16be.caf"))
    assert (got.container, got.selected_track.codec) == ("caf", "pcm") and joined(got.frames) == joined(caf.decode_file(caf_file("pcm-s16be.caf"), engine=engine)[1])
    for data, text in ((b"RIFF" + bytes(4) + b"AVI LIST" + bytes(64), "AVI is not built"), (b"\0\0\x01\xba" + bytes(64), "MPEG-PS is not built"),
                       (bytes(100) + b"\x06\x0e\x2b\x34" + bytes(64), "MXF is not built")):
        with pytest.raises(SoundkitError, match=text):
            run(data)
    golden = os.path.join(HERE, "golden")
    data = open(os.path.join(golden, "ts", "aac-stereo-48k.ts"), "rb").read()
    got = run(data)
    assert got.container == "mpeg-ts" and joined(got.frames) == joined(ts.decode_file(data, scheduler=sched, engine=engine)[1]) and got.frames
    data = open(os.path.join(golden, "webm", "A_Tusk_is_used_to_make_costly_gifts.webm"), "rb").read()  # an Opus track: what webm.decode_file says
    with pytest.raises(SoundkitError, match="unsupported or disabled WebM codec: A_OPUS"):
        run(data)
    with pytest.raises(SoundkitError, match="unsupported or disabled WebM codec: A_OPUS"):
        webm.decode_file(data, scheduler=sched, engine=engine)
    # anything else: through spawn() to the end of the stream
    wav = open(os.path.join(golden, "wav_stereo_A_Tusk.wav"), "rb").read()
    got = run(wav)
    assert got.container is None and joined(got.frames) == wav[wav.find(b"data") + 8:][:len(joined(got.frames))] and len(joined(got.frames)) == 4 * 47360

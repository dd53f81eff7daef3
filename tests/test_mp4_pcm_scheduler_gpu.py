"""MP4 streams with a `fLaC` or a PCM track through the batch scheduler: at the config event such a stream becomes a FLAC stream (as a
WebM A_FLAC track does) or a raw PCM stream of the entry's format (as transport-stream LPCM does).  Beside an ADTS stream, at two piece
sizes, each concatenates to what `mp4.decode_file` gives without the edit trim; a 64-bit float track, an ALAC track and a `moov`-last
file end alone, with their texts."""
import os

import pytest

import mp4_builder as B
import mp4_cases as CASES
import mp4_pcm_builder as P
from soundkit_amd import mp4, pipeline
from test_mp4_scheduler_gpu import cut, run_on

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MOV = os.path.join(HERE, "golden", "mov_pcm")
FLAC = os.path.join(HERE, "golden", "flac")


def mov(name):
    return open(os.path.join(MOV, name), "rb").read()


def joined(outs):
    assert all(not isinstance(o, pipeline.DecodeError) for o in outs), [str(o) for o in outs if isinstance(o, pipeline.DecodeError)]
    return b"".join(o.data.tobytes() for o in outs)


@pytest.fixture(scope="module")
def files():
    flac16 = open(os.path.join(FLAC, "A_Tusk_is_used_to_make_costly_gifts_16bit.flac"), "rb").read()
    return {"s24be": B.faststart(mov("pcm-s24be.mov")), "s24le": B.faststart(mov("pcm-s24le.mov")), "f32le": B.faststart(mov("pcm-f32le.mov")),
            "flac": P.flac_in_mp4(flac16, "dfla")[0], "f64le": B.faststart(mov("pcm-f64le.mov")), "alac": B.faststart(CASES.fixture("alac_A_Tusk.m4a")),
            "moov_last": mov("pcm-s32le.mov"), "adts": CASES.golden("aac", "mono16k_A_Tusk.aac")}


@pytest.fixture(scope="module")
def whole(engine, files):
    """what decode_file gives; the fixtures' edit keeps every frame, the built FLAC file has none: no trim either way"""
    return {k: mp4.decode_file(files[k], engine=engine)[1] for k in ("s24be", "s24le", "f32le", "flac")}


@pytest.fixture(scope="module")
def sched(engine):
    s = pipeline.BatchScheduler(engine, entropy_threads=4, max_streams=16)
    yield s
    s.close()


@pytest.mark.parametrize("piece", [1 << 20, 1000])
def test_pcm_and_flac_tracks_decode_beside_an_adts_stream(sched, files, whole, piece):
    names = ["adts", "s24be", "s24le", "f32le", "flac", "f64le", "alac", "moov_last", "adts"]
    outs = dict(zip(range(len(names)), run_on(sched, [(None, cut(files[n], piece)) for n in names])))
    for i, n in enumerate(names):
        if n not in whole:
            continue
        want = whole[n]
        got = outs[i]
        assert joined(got) == b"".join(a.data.tobytes() for a in want), n
        assert {(o.bits_per_sample, o.channel_count, o.sampling_rate, o.audio_format, o.endianness) for o in got} == \
            {(a.bits_per_sample, a.channel_count, a.sampling_rate, a.audio_format, a.endianness) for a in want}, n
    # the three that end with a text end alone
    for i, text in ((5, "Decoding failed: MP4 64-bit float PCM is not decoded in a stream; decode the whole file (decode_file)"),
                    (6, "Decoding failed: MP4/M4A audio track is not AAC"),
                    (7, "Decoding failed: MP4 mdat appears before moov; use the seekable MP4 packet API")):
        assert len(outs[i]) == 1 and isinstance(outs[i][0], pipeline.DecodeError) and str(outs[i][0]) == text, (names[i], [str(o) for o in outs[i]])
    # the ADTS streams beside them are untouched: 48 access units each, the same bytes in both
    assert len(outs[0]) == len(outs[8]) == 48 and joined(outs[0]) == joined(outs[8])


def test_fragmented_pcm_and_flac_streams_are_refused_at_the_config_event(sched, files):
    pcm = P.fragmented(P.sound_entry(b"sowt", 0, 2, 16), [bytes(4)] * 10, [1] * 10)
    flac16 = open(os.path.join(FLAC, "A_Tusk_is_used_to_make_costly_gifts_16bit.flac"), "rb").read()
    info, frames, blocks, first = P.flac_frames(flac16)
    entry = P.sound_entry(b"fLaC", 0, first["channels"], 16, first["sample_rate"], B.box(b"dfLa", P.dfla(info, "dfla")))
    flac = P.fragmented(entry, frames, blocks, first["sample_rate"])
    outs = run_on(sched, [(None, cut(files["adts"], 4099)), (None, cut(pcm, 1 << 20)), (None, cut(flac, 4099))])
    for got, text in ((outs[1], "Decoding failed: fragmented MP4 pcm tracks are not built"), (outs[2], "Decoding failed: fragmented MP4 flac tracks are not built")):
        assert len(got) == 1 and isinstance(got[0], pipeline.DecodeError) and str(got[0]) == text, [str(o) for o in got]
    assert len(outs[0]) == 48 and joined(outs[0])


def test_output_options_apply_to_a_routed_stream(sched, files, engine):
    down = pipeline.DecodeOptions(16, 16000, 1)
    outs = run_on(sched, [(down, cut(files["s24be"], 1 << 20)), (down, cut(files["s24le"], 4099)), (down, cut(files["flac"], 4099))])
    assert joined(outs[0]) == joined(outs[1]) and len(joined(outs[0])) >= 2 * 1500
    assert all((o.bits_per_sample, o.channel_count, o.sampling_rate) == (16, 1, 16000) for o in outs[0] + outs[1] + outs[2])
    _, want = mp4.decode_file(files["s24be"], down, scheduler=sched, engine=engine)
    assert joined(outs[0]) == b"".join(a.data.tobytes() for a in want)

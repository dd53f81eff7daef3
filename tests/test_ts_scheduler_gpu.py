"""MPEG transport streams through the batch scheduler: `spawn()` takes one by its three syncs (`spawn_mpeg_ts()` one that is joined in
mid-segment), the stream is demuxed on its entropy thread and from its track's first packet on it is what that track is -- an ADTS
stream, an MPEG audio stream of the first frame's layer, a raw stream of big-endian PCM whose pieces are the PES payloads.  So its
AudioData are, bit for bit and unit for unit, those of the twin that was fed what tests/ts_model.py finds in it: the elementary stream
through `spawn()`, the payloads through `spawn_raw_pcm(S16BE, 48000, 2)`.  The neighbours of the round -- an ADTS, a WAV and a WebM
stream -- give what they give without it.  A stream that is refused ends alone, with the reference's text, behind every unit that was
complete in front of the refusal."""
import pytest

import ts_builder as B
import ts_cases as CASES
import ts_model as M
from soundkit_amd import pipeline
from soundkit_amd.engine import FMT_S16BE
from test_webm_scheduler_gpu import cut, run_round, shape, sniffed

pytestmark = pytest.mark.gpu

ADTS = CASES.adts_frames(CASES.ADTS)
NEIGHBOURS = {"adts": (sniffed(), cut(CASES.ADTS, 3000)), "wav": (sniffed(), cut(CASES.golden("wav_stereo_A_Tusk.wav")[:200000], 50000)),
              "webm": (sniffed(), cut(CASES.golden("vorbis", "yt_itag_171_vorbis.webm"), 4096))}


def twin(data):
    """what the model finds in a transport stream, as the stream the scheduler had before the container: -> (spawn, sends)"""
    events, _ = M.demux(data)
    payloads = [e["data"] for kind, e in events if kind == "packet"]
    if events and events[0][1]["codec"] == "pcm":
        c = events[0][1]
        assert (c["bits"], c["rate"], c["channels"]) == (16, 48000, 2)
        return (lambda sched: sched.spawn_raw_pcm(pipeline.RawPcmFormat(48000, 2, FMT_S16BE))), payloads
    return sniffed(), cut(b"".join(payloads), 4096)


def clean(out):
    assert all(err is None for _, err in out.values()), {n: str(e) for n, (_, e) in out.items() if e is not None}


@pytest.fixture(scope="module")
def alone(engine):
    """the neighbours in a round of their own"""
    out = run_round(engine, NEIGHBOURS)
    clean(out)
    assert len(out["adts"][0]) == 48 and len(out["wav"][0]) > 0 and len(out["webm"][0]) == 55
    return {name: shape(got) for name, (got, _) in out.items()}


@pytest.mark.parametrize("lanes, budget", [(1, 0), (2, 5)], ids=["one lane", "two lanes, 5 frames a stream and tick"])
def test_fixtures_equal_their_twins_beside_streams_that_do_not_change(engine, alone, lanes, budget):
    streams = dict(NEIGHBOURS)
    for name in CASES.FIXTURES:
        data = CASES.fixture(name)
        streams[name + " twin"] = twin(data)
        for piece in (1000, 4096, len(data)):
            streams["%s in %d" % (name, piece)] = (sniffed(), cut(data, piece))
    sched = pipeline.BatchScheduler(engine, entropy_threads=3, max_streams=32, lanes=lanes, max_stream_frames_per_tick=budget)
    try:
        out = run_round(engine, streams, sched=sched)
    finally:
        sched.close()
    clean(out)
    for name in CASES.FIXTURES:
        want = shape(out[name + " twin"][0])
        units = {"aac.ts": 48, "aac.m2ts": 48, "mp2.ts": 84, "lpcm.m2ts": 20}[name]  # a Layer II frame is two AudioData of 576 frames
        assert len(want) == units and all(s[:3] == (16, 2, 48000) for s in want)
        for piece in (1000, 4096, len(CASES.fixture(name))):
            assert shape(out["%s in %d" % (name, piece)][0]) == want, (name, piece)
    for name in NEIGHBOURS:
        assert shape(out[name][0]) == alone[name], name


def test_output_options_equal_the_twins_under_the_same_options(engine):
    options = pipeline.DecodeOptions(16, 16000, 1)
    streams = {}
    for name in CASES.FIXTURES:
        data = CASES.fixture(name)
        spawn, sends = twin(data)
        if name == "lpcm.m2ts":
            spawn = lambda sched: sched.spawn_raw_pcm(pipeline.RawPcmFormat(48000, 2, FMT_S16BE), options)  # noqa: E731
        else:
            spawn = sniffed(options)
        streams[name + " twin"] = (spawn, sends)
        streams[name] = (sniffed(options), cut(data, 4096))
    out = run_round(engine, streams)
    clean(out)
    for name in CASES.FIXTURES:
        want = shape(out[name + " twin"][0])
        assert want and all(s[:3] == (16, 1, 16000) for s in want) and shape(out[name][0]) == want, name


def test_a_join_in_mid_segment_through_spawn_mpeg_ts(engine):
    streams = {}
    for name, off in (("aac.ts", 100), ("lpcm.m2ts", 100), ("aac.ts", 700)):  # 100: inside the first packet, which carries no table
        data = CASES.fixture(name)[off:]
        assert M.demux(data)[1] is None
        streams["%s %d" % (name, off)] = (lambda sched: sched.spawn_mpeg_ts(), cut(data, 1000))
        streams["%s %d twin" % (name, off)] = twin(data)
        streams[name + " whole"] = twin(CASES.fixture(name))
    streams["sniffed"] = (sniffed(), cut(CASES.fixture("mp2.ts"), 1000))  # spawn_mpeg_ts takes a stream that begins at a packet as spawn() does
    streams["known"] = (lambda sched: sched.spawn_mpeg_ts(), cut(CASES.fixture("mp2.ts"), 1000))
    out = run_round(engine, streams)
    clean(out)
    for name, off in (("aac.ts", 100), ("lpcm.m2ts", 100), ("aac.ts", 700)):
        want = shape(out["%s %d twin" % (name, off)][0])
        assert want and shape(out["%s %d" % (name, off)][0]) == want, (name, off)
        if off == 100:
            assert want == shape(out[name + " whole"][0])
    assert len(out["aac.ts 700"][0]) == 40  # the audio in front of the next PAT and PMT is lost
    assert len(out["known"][0]) == 84 and shape(out["known"][0]) == shape(out["sniffed"][0])


def test_built_layer_iii_and_layer_i_streams_decode_like_their_elementary_streams(engine):
    cases = CASES.builder_cases()
    streams = {}
    for name in ("layer3", "layer1", "adts_204", "lpcm_16", "pts_wrap", "duplicate_and_gap"):
        known = lambda sched: sched.spawn_mpeg_ts()  # noqa: E731  (stride 204 is none of the two that spawn() takes by itself)
        streams[name] = (known if name == "adts_204" else sniffed(), cut(cases[name], 1000))
        streams[name + " twin"] = twin(cases[name])
    out = run_round(engine, streams)
    clean(out)
    for name in ("layer3", "layer1", "adts_204", "lpcm_16", "pts_wrap", "duplicate_and_gap"):
        want = shape(out[name + " twin"][0])
        assert len(want) > 4 and shape(out[name][0]) == want, name
    assert len(out["layer1"][0]) == 24 and all(s[:3] == (16, 2, 48000) and len(s[3]) == 384 * 4 for s in shape(out["layer1"][0]))
    assert all(s[:3] == (16, 2, 16000) for s in shape(out["layer3"][0])) and len(out["layer3"][0]) >= 38


def test_refused_streams_end_alone_with_the_references_text(engine, alone):
    cases = CASES.builder_cases()

    def scrambled(m):
        m.pes(0x100, B.pes(b"".join(ADTS[:3]), 1000)).pes(0x100, B.pes(b"".join(ADTS[3:6]), 6760))
        m.raw(B.packet(0x100, m.next_cc(0x100), bytes(184), scrambling=2))
        m.pes(0x100, B.pes(b"".join(ADTS[6:9]), 12520))

    streams = dict(NEIGHBOURS)
    streams.update({name: (sniffed(), cut(cases[name], 1000)) for name in ("dts", "ac3", "latm")})
    streams["scrambled"] = (sniffed(), cut(CASES.with_packets(scrambled), 1000))
    streams["three frames"] = (sniffed(), [b"".join(ADTS[:3])])
    streams["no audio"] = (sniffed(), [CASES.with_packets(lambda m: m.pes(0x100, B.pes(bytes(500), 1, 1, 0xe0)), 0x1b)])
    out = run_round(engine, streams)
    for name, codec in (("dts", "dts"), ("ac3", "ac3"), ("latm", "aac")):
        got, err = out[name]
        assert got == [] and str(err) == "Invalid input format: unsupported MPEG-TS audio codec " + codec, name
    got, err = out["scrambled"]
    assert str(err) == "Invalid input format: scrambled MPEG-TS packets are unsupported"
    assert len(got) == 3 and shape(got) == shape(out["three frames"][0])  # the PES that was complete in front of it
    got, err = out["no audio"]
    assert got == [] and str(err) == "Invalid input format: MPEG-TS has no supported audio track"
    for name in NEIGHBOURS:
        assert out[name][1] is None and shape(out[name][0]) == alone[name], name

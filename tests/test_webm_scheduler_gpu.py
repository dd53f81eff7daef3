"""WebM / Matroska streams through the batch scheduler: `spawn()` sniffs the EBML magic, the stream is demuxed on its entropy thread
and from its first Cluster on it is what its audio track is -- a Vorbis stream whose packets come from the demuxer, an ADTS stream, a
native FLAC stream.  So its AudioData are, bit for bit and unit for unit, those of the twin that was fed the unwrapped bytes: the
`spawn_vorbis_packets` handle, the ADTS stream, the FLAC stream -- whole and in sends of 641 bytes, on one lane and on two, with and
without output options.  A stream that is refused ends alone, with its text, and leaves its slot reusable."""
import pytest

import webm_cases as CASES
import webm_vorbis
from soundkit_amd import pipeline

pytestmark = pytest.mark.gpu

ADTS = CASES.golden("aac", "aac-stereo-48k.adts")
FLAC = CASES.golden("flac", "A_Tusk_is_used_to_make_costly_gifts.flac")
OGG = CASES.golden("vorbis", "A_Tusk_is_used_to_make_costly_gifts.ogg")


def cut(data, n):
    return [data[at:at + n] for at in range(0, len(data), n)]


def drain(h):
    """-> ([AudioData], the error that ended the stream or None)"""
    out = []
    while True:
        a = h.recv(60000)
        if a is None:
            return out, None
        if isinstance(a, Exception):
            return out, a
        out.append(a)


def feed(h, sends):
    """sends with the queue's back-pressure honoured (an output is taken when the input is full); a stream that has ended takes no more"""
    got = []
    for s in list(sends) + [b""]:
        while True:
            try:
                h.send(s)
                break
            except pipeline.DecodeError as e:
                if e.kind == "PipelineClosed":
                    return got
                assert e.kind == "InputBufferFull", e
                a = h.recv(60000)
                if a is None or isinstance(a, Exception):
                    return got + ([a] if a is not None else [])
                got.append(a)
    return got


def shape(outs):
    return [(a.bits_per_sample, a.channel_count, a.sampling_rate, a.data.tobytes()) for a in outs]


def run_round(engine, streams, lanes=1, sched=None):
    """streams: {name: (spawn, [sends])}, all spawned before anything is sent -> {name: ([AudioData], error)}"""
    own = sched is None
    sched = sched or pipeline.BatchScheduler(engine, entropy_threads=2, max_streams=16, lanes=lanes)
    try:
        handles = {name: spawn(sched) for name, (spawn, _) in streams.items()}
        early = {name: feed(handles[name], streams[name][1]) for name in handles}
        out = {}
        for name, h in handles.items():
            rest, err = drain(h)
            items = early[name] + rest + [err]  # (feed may have met the error already)
            out[name] = ([a for a in items if a is not None and not isinstance(a, Exception)], next((a for a in items if isinstance(a, Exception)), None))
            h.cancel()
        return out
    finally:
        if own:
            sched.close()


def sniffed(options=None):
    return lambda sched: sched.spawn(options)


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("sends", ["641", "whole"])
def test_the_vorbis_fixture_beside_its_packets_an_adts_an_ogg_and_a_flac_stream(engine, lanes, sends):
    data = CASES.fixture("vorbis")
    headers, packets = webm_vorbis.vorbis_track(data)
    out = run_round(engine, {
        "webm": (sniffed(), cut(data, 641) if sends == "641" else [data]),
        "packets": (lambda sched: sched.spawn_vorbis_packets(*headers), packets),
        "adts": (sniffed(), cut(ADTS, 3000)), "ogg": (sniffed(), cut(OGG, 641)), "flac": (sniffed(), cut(FLAC, 4096))}, lanes)
    assert all(err is None for _, err in out.values()), {n: str(e) for n, (_, e) in out.items()}
    want = shape(out["packets"][0])
    assert len(want) == 55 and all(s[:3] == (16, 2, 44100) for s in want)  # one per packet that yields frames
    assert shape(out["webm"][0]) == want
    assert len(out["adts"][0]) == 48 and [a.data.size // 2 for a in out["ogg"][0]] == [256] * 92 + [128]
    assert sum(a.data.size for a in out["flac"][0]) > 40000


def test_aac_and_flac_tracks_equal_their_unwrapped_twins_unit_for_unit(engine):
    aac_file, adts = CASES.wrapped_aac()
    flac_file, flac = CASES.wrapped_flac()
    out = run_round(engine, {"aac": (sniffed(), cut(aac_file, 641)), "adts": (sniffed(), cut(adts, 4096)), "aac whole": (sniffed(), [aac_file]),
                             "flac": (sniffed(), cut(flac_file, 641)), "native": (sniffed(), cut(flac, 4096)), "flac whole": (sniffed(), [flac_file])}, 2)
    assert all(err is None for _, err in out.values()), {n: str(e) for n, (_, e) in out.items()}
    want = shape(out["adts"][0])
    assert len(want) == 48 and shape(out["aac"][0]) == want and shape(out["aac whole"][0]) == want
    want = shape(out["native"][0])
    assert len(want) > 4 and shape(out["flac"][0]) == want and shape(out["flac whole"][0]) == want


@pytest.mark.parametrize("options", [pipeline.DecodeOptions(16, 16000, 1), pipeline.DecodeOptions(24)], ids=["16 kHz mono s16", "24 bits"])
def test_output_options_equal_the_twins_under_the_same_options(engine, options):
    data = CASES.fixture("vorbis")
    headers, packets = webm_vorbis.vorbis_track(data)
    aac_file, adts = CASES.wrapped_aac()
    flac_file, flac = CASES.wrapped_flac()
    out = run_round(engine, {
        "webm": (sniffed(options), cut(data, 641)), "packets": (lambda sched: sched.spawn_vorbis_packets(*headers, options), packets),
        "aac": (sniffed(options), cut(aac_file, 1000)), "adts": (sniffed(options), cut(adts, 4096)),
        "flac": (sniffed(options), cut(flac_file, 1000)), "native": (sniffed(options), cut(flac, 4096))})
    assert all(err is None for _, err in out.values()), {n: str(e) for n, (_, e) in out.items()}
    for got, twin in (("webm", "packets"), ("aac", "adts"), ("flac", "native")):
        want = shape(out[twin][0])
        assert want and shape(out[got][0]) == want, got
        assert all(s[0] == options.output_bits_per_sample for s in want)


def test_discard_padding_cuts_the_last_audio_data_to_128_frames(engine):
    data, headers, packets = CASES.wrapped_ogg({93: 16000000})
    front, _, _ = CASES.wrapped_ogg({1: -16000000, 93: 16000000})
    out = run_round(engine, {"webm": (sniffed(), cut(data, 641)), "ogg": (sniffed(), cut(OGG, 641)), "front": (sniffed(), [front])})
    assert all(err is None for _, err in out.values()), {n: str(e) for n, (_, e) in out.items()}
    want = shape(out["ogg"][0])
    assert [len(s[3]) // 2 for s in want] == [256] * 92 + [128]
    assert shape(out["webm"][0]) == want  # the Ogg decoder's cut to the final granule position and the container's padding agree
    got = shape(out["front"][0])
    assert got[0] == want[0][:3] + (want[0][3][256:],) and got[1:] == want[1:]  # 128 frames off the front of the first, nothing else moves


def test_refused_streams_end_alone_and_leave_their_slots_reusable(engine):
    data = CASES.fixture("vorbis")
    headers, packets = webm_vorbis.vorbis_track(data)
    sched = pipeline.BatchScheduler(engine, entropy_threads=2, max_streams=4)
    try:
        where = data.index(packets[20]) + 5  # inside the 21st block
        out = run_round(engine, {"opus": (sniffed(), cut(CASES.fixture("opus"), 641)), "cut": (sniffed(), cut(data[:where], 641)),
                                 "webm": (sniffed(), cut(data, 641)), "adts": (sniffed(), cut(ADTS, 3000))}, sched=sched)
        got, err = out["opus"]
        assert got == [] and str(err) == "Decoding failed: unsupported or disabled WebM codec: A_OPUS"
        whole, err = out["webm"]
        assert err is None and len(whole) == 55 and len(out["adts"][0]) == 48 and out["adts"][1] is None  # the others of the round are complete
        got, err = out["cut"]
        assert shape(got) == shape(whole)[:19]  # 20 whole blocks: every packet but the first yields
        assert str(err).startswith("Decoding failed: truncated WebM element: ") and str(err).endswith(" buffered bytes remain")
        again = run_round(engine, {k: (sniffed(), [data]) for k in "abcd"}, sched=sched)  # every slot once more
        assert all(err is None and shape(got) == shape(whole) for got, err in again.values())
    finally:
        sched.close()

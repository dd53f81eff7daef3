"""MP4 / M4A streams through the batch scheduler: `spawn()` sniffs `ftyp`, the stream is demuxed on its entropy thread and every AAC
sample goes, ADTS-wrapped, where an ADTS stream's frame goes.  So an MP4 stream's AudioData are, bit for bit, those of an ADTS stream fed
the same samples -- whole or in 1000-byte pieces, regular or fragmented, at two frame budgets, with the host and the GPU front end, with
and without output options -- and a stream the demuxer or the config check refuses ends alone, with its text."""
import time

import pytest

import mp4_builder as B
import mp4_cases as CASES
import mp4_model as M
from soundkit_amd import pipeline

pytestmark = pytest.mark.gpu

TO_16K_MONO = pipeline.DecodeOptions(16, 16000, 1)


def cut(data, n):
    return [data[at:at + n] for at in range(0, len(data), n)]


def run_on(sched, streams, deadline_s=120):
    """streams: (DecodeOptions or None, [chunks]) -> per stream its outputs.  Sending and receiving take turns, so that a stream whose
    output queue is full never holds up its own input"""
    handles = [sched.spawn(o) for o, _ in streams]
    pos, outs, live, t0 = [0] * len(handles), [[] for _ in handles], set(range(len(handles))), time.time()
    while live:
        assert time.time() - t0 < deadline_s, "scheduler stalled"
        for i in list(live):
            chunks = streams[i][1]
            try:
                if pos[i] < len(chunks):
                    handles[i].send(chunks[pos[i]])
                    pos[i] += 1
                elif pos[i] == len(chunks):
                    handles[i].finish()
                    pos[i] += 1
            except pipeline.DecodeError as e:
                if e.kind == "PipelineClosed":
                    pos[i] = len(chunks) + 1
                else:
                    assert e.kind == "InputBufferFull", e
            got = handles[i].try_recv()
            while got is not None:
                outs[i].append(got)
                got = handles[i].try_recv()
            if pos[i] > len(chunks) and handles[i].ended() and handles[i].try_recv() is None:
                live.discard(i)
        time.sleep(0.0002)
    for h in handles:
        h.cancel()
    return outs


def run(engine, streams, budget=0, gpu_entropy=0, max_streams=None):
    sched = pipeline.BatchScheduler(engine, entropy_threads=4, max_streams=max_streams or len(streams) + 4, max_stream_frames_per_tick=budget,
                                    gpu_entropy=gpu_entropy)
    try:
        return run_on(sched, streams)
    finally:
        sched.close()


def shape(outs):
    """what an AudioData sequence is compared by"""
    assert all(not isinstance(o, pipeline.DecodeError) for o in outs), [str(o) for o in outs if isinstance(o, pipeline.DecodeError)]
    return [(o.bits_per_sample, o.channel_count, o.sampling_rate, o.data.tobytes()) for o in outs]


@pytest.fixture(scope="module")
def files():
    cfg, units = CASES.mac_aac_units()
    return {
        "faststart": B.faststart(CASES.fixture("mac_aac_A_Tusk.m4a")),
        "fragmented": B.fragmented(cfg, units, per_moof=7, per_trun=3),
        "h264": CASES.fixture("h264-high-aac.mp4"),
        "h264_fragmented": CASES.fixture("h264-aac-fragmented.mp4"),
    }


def test_the_faststart_rewrite_is_the_fixture_with_moov_in_front(files):
    assert M.adts_bytes(files["faststart"]) == CASES.golden("aac", "mono16k_A_Tusk.aac") == M.adts_bytes(files["fragmented"])
    assert [n for n, _, _ in M.boxes(files["faststart"]) if n in (b"moov", b"mdat")] == [b"moov", b"mdat"]
    assert M.adts_bytes(files["h264"]) == M.adts_bytes(files["h264_fragmented"])


@pytest.mark.parametrize("gpu_entropy", [0, 1])
@pytest.mark.parametrize("budget", [0, 3])
def test_mp4_streams_are_their_adts_twins(engine, files, budget, gpu_entropy):
    mono, stereo = CASES.golden("aac", "mono16k_A_Tusk.aac"), M.adts_bytes(files["h264"])
    neighbours = [(None, cut(CASES.golden("aac", "aac-stereo-48k.adts"), 4096)),
                  (None, cut(CASES.golden("flac", "A_Tusk_is_used_to_make_costly_gifts.flac"), 3000))]
    alone = run(engine, neighbours + [(None, cut(mono, 4096)), (None, cut(stereo, 4096))], budget, gpu_entropy)
    names = ["faststart", "fragmented", "h264", "h264_fragmented"]
    streams = [(None, [files[n]]) for n in names] + [(None, cut(files[n], 1000)) for n in names]
    outs = run(engine, neighbours + streams, budget, gpu_entropy)
    twins = [shape(alone[2]), shape(alone[2]), shape(alone[3]), shape(alone[3])] * 2
    assert [len(t) for t in twins[:4]] == [48, 48, 142, 142]
    for name, got, want in zip(names * 2, outs[2:], twins):
        assert shape(got) == want, name
    assert [shape(o) for o in outs[:2]] == [shape(o) for o in alone[:2]]  # the neighbours are what they are without MP4 streams beside them


def test_output_options_equal_the_adts_twin_under_the_same_options(engine, files):
    stereo = M.adts_bytes(files["h264"])
    outs = run(engine, [(TO_16K_MONO, cut(stereo, 4096)), (TO_16K_MONO, [files["h264"]]), (TO_16K_MONO, cut(files["h264_fragmented"], 1000))])
    want = shape(outs[0])
    assert all(s[:3] == (16, 1, 16000) for s in want) and sum(len(s[3]) for s in want) > 2 * 47000  # 145 408 frames at a third of the rate
    assert shape(outs[1]) == want and shape(outs[2]) == want


def test_refused_streams_end_alone_and_leave_their_slots_reusable(engine, files):
    cfg, units = CASES.mac_aac_units()
    track = M.index(files["faststart"])
    cut_at = track["samples"][30][0] + 5  # inside the 31st sample
    sbr = dict(cfg, private=bytes([0x2c, 0x0a, 0x88, 0x00]))  # object type 5 in front: SBR signalled explicitly
    many = dict(cfg, private=bytes([0x14, 0x18]), channels=3)  # channel configuration 3
    cases = [
        ("mdat first", CASES.fixture("mac_aac_A_Tusk.m4a"), 0, "Decoding failed: " + CASES.MDAT_FIRST),
        # this file signals SBR through the backward-compatible sync extension behind an AAC-LC config, which the AAC-LC config check
        # (like the reference's) does not read: the first access unit's SBR fill element ends the stream, before any audio
        ("HE-AAC", CASES.fixture("yt_itag_139_he_aac.mp4"), 0, "Decoding failed: SBR/HE-AAC extension payload"),
        ("explicit SBR", B.regular(sbr, units), 0, "Decoding failed: AAC-LC decoder init: unsupported AAC feature"),
        ("three channels", B.regular(many, units), 0, None),
        ("ALAC", B.faststart(CASES.fixture("alac_A_Tusk.m4a")), 0, "Decoding failed: MP4/M4A audio track is not AAC"),
        ("cut mid-sample", files["faststart"][:cut_at], 30, "Decoding failed: truncated MP4 box mdat"),
        ("cut mid-sample, fragmented", files["fragmented"][:M.index(files["fragmented"])["samples"][30][0] + 5], 30, "Decoding failed: truncated MP4 box mdat"),
    ]
    good = [(None, cut(files["faststart"], 1000)), (None, cut(CASES.golden("aac", "mono16k_A_Tusk.aac"), 4096))]
    streams = good + [(None, cut(data, 1000)) for _, data, _, _ in cases]
    sched = pipeline.BatchScheduler(engine, entropy_threads=4, max_streams=len(streams))
    try:
        outs = run_on(sched, streams)
        want = shape(outs[1])
        assert len(want) == 48 and shape(outs[0]) == want  # the good streams of the round are untouched
        for (name, _, units_before, text), got in zip(cases, outs[2:]):
            assert len(got) == units_before + 1 and isinstance(got[-1], pipeline.DecodeError), (name, len(got))
            assert shape(got[:-1]) == want[:units_before], name  # every complete unit first
            if text is not None:
                assert str(got[-1]) == text, name
            else:
                assert str(got[-1]).startswith("Decoding failed: AAC-LC decoder init: "), (name, str(got[-1]))
        again = run_on(sched, [(None, [files["faststart"]])] * len(streams))  # every slot once more
        assert all(shape(o) == want for o in again)
    finally:
        sched.close()

"""ALAC packet streams through the batch scheduler (sk_pipeline_spawn_alac_packets): the cookie at the spawn, every send exactly one packet,
the empty send the end; budgeted in whole packets, decoded by the ALAC tick in the PCM family's shared path.  The reference's fixture
beside an ADTS and a FLAC stream, at two frame budgets, equals decode_caf and -- with default options -- its decoded twin; a damaged
packet ends only its own stream, with its text; decode_caf with output options equals the raw PCM path on the twin's samples."""
import os

import pytest

import alac_builder as B
import alac_cases as CASES
import alac_model as M
from soundkit_amd import pipeline
from test_flac_scheduler_gpu import cut, feed
from test_pcm_pipeline_gpu import drain, read

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "alac", "A_Tusk_is_used_to_make_costly_gifts.caf")
TWIN = os.path.join(HERE, "golden", "alac", "A_Tusk_is_used_to_make_costly_gifts.decoded.wav")
FLAC = os.path.join(HERE, "golden", "flac", "A_Tusk_is_used_to_make_costly_gifts.flac")


def twin_pcm():
    w = open(TWIN, "rb").read()
    return w[w.index(b"data") + 8:]


def run(engine, alac_streams, others, budget=0):
    """alac_streams: (cookie, DecodeOptions, [packets]); others: chunk lists of detected streams -> per stream its outputs"""
    sched = pipeline.BatchScheduler(engine, entropy_threads=4, max_streams=len(alac_streams) + len(others) + 4, max_stream_frames_per_tick=budget)
    try:
        handles = [sched.spawn_alac_packets(c, o) for c, o, _ in alac_streams] + [sched.spawn() for _ in others]
        feed(handles, [p for _, _, p in alac_streams] + list(others))
        outs = drain(handles)
        for h in handles:
            h.cancel()
    finally:
        sched.close()
    return outs


def audio(outs):
    assert all(not isinstance(o, pipeline.DecodeError) for o in outs), [str(o) for o in outs if isinstance(o, pipeline.DecodeError)]
    return b"".join(o.data.tobytes() for o in outs)


@pytest.fixture(scope="module")
def fixture_parts():
    from soundkit_amd import alac
    data = open(FIXTURE, "rb").read()
    at, size = M.caf_chunks(data)["kuki"]
    return data, data[at:at + size], alac.CafAlacPacketIndex.from_file(data).packet_bytes(data)


@pytest.mark.parametrize("budget", [0, 2])
def test_the_fixture_beside_an_adts_and_a_flac_stream(engine, fixture_parts, budget):
    from soundkit_amd import alac
    data, cookie, packets = fixture_parts
    others = [cut(read("aac/aac-stereo-48k.adts"), 4096), cut(open(FLAC, "rb").read(), 3000)]
    alone = run(engine, [], others, budget)
    to16k = pipeline.DecodeOptions(16, 16000, 1)
    outs = run(engine, [(cookie, None, packets), (cookie, to16k, packets)], others, budget)
    # default options: one AudioData per packet, the twin's bytes
    assert [(o.bits_per_sample, o.channel_count, o.sampling_rate, len(o.data) // 2) for o in outs[0]] == [(16, 1, 8000, 4096)] * 5 + [(16, 1, 8000, 3200)]
    assert audio(outs[0]) == twin_pcm()
    sched = pipeline.BatchScheduler(engine, max_streams=8)
    try:
        _, whole = alac.decode_caf(data, engine=engine)
        # with options: what decode_caf gives (the raw PCM stream's conversion of the same samples)
        _, converted = alac.decode_caf(data, to16k, scheduler=sched, engine=engine)
    finally:
        sched.close()
    assert [a.data.tobytes() for a in whole] == [o.data.tobytes() for o in outs[0]]
    assert all((o.bits_per_sample, o.channel_count, o.sampling_rate) == (16, 1, 16000) for o in outs[1])
    assert audio(outs[1]) == b"".join(a.data.tobytes() for a in converted) and len(audio(outs[1])) > 2 * 46000  # 47 360 frames at twice the rate, less what the filter holds back
    # the neighbours are what they are alone
    assert [audio(o) for o in outs[2:]] == [audio(o) for o in alone]


def test_a_damaged_packet_ends_only_its_own_stream(engine, fixture_parts):
    _, cookie, packets = fixture_parts
    cfg = B.config(4096, 16, 2, 44100)
    good = [CASES.signal("tone", n, 16, n, 2) for n in (300, 4096, 77)]
    built = [B.packet(cfg, ch, order=4, shift=6, mix_weight=1, mix_shift=2) for ch in good]
    device_rejects = [built[0], B.packet(cfg, good[1], ptype=3), built[2]]
    host_rejects = [built[0], bytes([0xE0]), built[2]]
    element = [built[0], B.packet(cfg, good[1], before=lambda w: w.put(2, 3)), built[2]]
    mono = pipeline.DecodeOptions(16, None, 1)
    streams = [(B.cookie(cfg), None, built), (B.cookie(cfg, "qt"), None, device_rejects), (B.cookie(cfg, "mp4"), None, host_rejects),
               (B.cookie(cfg), None, element), (B.cookie(cfg), mono, device_rejects), (cookie, None, packets)]
    outs = run(engine, streams, [])
    assert audio(outs[0]) == b"".join(M.pcm_bytes(ch, 16) for ch in good)
    assert audio(outs[5]) == twin_pcm()
    syntax = "Decoding failed: ALAC packet rejected: the elements break the syntax or miss the packet's end"
    for i, text in ((1, syntax), (2, syntax), (3, "Decoding failed: ALAC packet rejected: a CCE or PCE element is not supported")):
        assert audio(outs[i][:1]) == M.pcm_bytes(good[0], 16)  # the packet in front of the damage has gone out
        assert len(outs[i]) == 2 and isinstance(outs[i][1], pipeline.DecodeError) and str(outs[i][1]) == text
    assert isinstance(outs[4][-1], pipeline.DecodeError) and str(outs[4][-1]) == syntax  # behind a conversion


def test_a_refused_cookie_spawns_nothing(engine):
    from soundkit_amd import SoundkitError
    sched = pipeline.BatchScheduler(engine, max_streams=4)
    try:
        for bad in (b"", B.cookie(dict(B.config(), bit_depth=20)), B.cookie(B.config())[:23]):
            with pytest.raises(SoundkitError) as e:
                sched.spawn_alac_packets(bad)
            assert e.value.status == -602
    finally:
        sched.close()


def test_decode_caf_with_options_equals_the_pcm_path_on_the_twin(engine):
    """DecodeOptions(16, 16000, 1): the twin's samples through a raw PCM stream, packet by packet as decode_caf hands them on"""
    from soundkit_amd import alac
    from soundkit_amd import engine as E
    data = open(FIXTURE, "rb").read()
    opts = pipeline.DecodeOptions(16, 16000, 1)
    sched = pipeline.BatchScheduler(engine, max_streams=8)
    try:
        index, got = alac.decode_caf(data, opts, scheduler=sched, engine=engine)
        twin = twin_pcm()
        h = sched.spawn_raw_pcm(pipeline.RawPcmFormat(8000, 1, E.FMT_S16LE), opts)
        pieces = [twin[at:at + 8192] for at in range(0, len(twin), 8192)]
        feed([h], [pieces])
        want = drain([h])[0]
        h.cancel()
    finally:
        sched.close()
    assert (index.valid_frames, index.frames_per_packet, len(index.packets)) == (23680, 4096, 6)
    assert audio(got) == audio(want) and len(audio(got)) > 2 * 46000
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 16000) for a in got)

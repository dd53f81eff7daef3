"""Vorbis through the batch scheduler: an Ogg Vorbis stream taken by the sniffing `spawn` (the Ogg walk and the header parse on the entropy
threads, the audio packets in the Vorbis tick), in sends of 641 bytes and whole, equal to vorbis.VorbisDecoder bit for bit; the WebM
fixture's demuxed packets through `spawn_vorbis_packets`, equal to vorbis.VorbisPacketDecoder; both beside an ADTS stream and a FLAC
stream in one round, on one lane and on two; an `OggS` stream whose first packet is not Vorbis refused alone while the others finish;
the output options behind the decode; the refusals' texts."""
import os

import numpy as np
import pytest

import vorbis_cases as CASES
import vorbis_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ADTS = os.path.join(GOLDEN, "aac", "aac-stereo-48k.adts")
FLAC = os.path.join(GOLDEN, "flac", "A_Tusk_is_used_to_make_costly_gifts.flac")
FLAC_TWIN = os.path.join(GOLDEN, "linear16_A_Tusk.s16le")


def read(path):
    with open(path, "rb") as f:
        return f.read()


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
    """sends with the queue's back-pressure honoured (an output is taken when the input is full)"""
    from soundkit_amd.pipeline import DecodeError
    got = []
    for s in list(sends) + [b""]:
        while True:
            try:
                h.send(s)
                break
            except DecodeError as e:
                assert e.kind == "InputBufferFull", e
                a = h.recv(60000)
                assert a is not None and not isinstance(a, Exception), a
                got.append(a)
    return got


def s16(audios):
    return np.concatenate([np.frombuffer(a.data.tobytes(), "<i2") for a in audios]) if audios else np.zeros(0, np.int16)


def cut(data, n):
    return [data[at:at + n] for at in range(0, len(data), n)]


@pytest.fixture(scope="module")
def ogg_want(engine):
    """VorbisDecoder over the fixture in pieces of 641 bytes"""
    from soundkit_amd import vorbis
    data = read(CASES.OGG)
    dec, got = vorbis.VorbisDecoder(engine=engine), []
    for piece in cut(data, 641):
        a = dec.add(piece)
        if a is not None:
            got.append(a)
    a = dec.finish()
    if a is not None:
        got.append(a)
    want = s16(got)
    assert want.size == 23680
    return want


@pytest.fixture(scope="module")
def webm_want(engine):
    """VorbisPacketDecoder over the WebM fixture's packets: one array per packet"""
    from soundkit_amd import vorbis
    case = CASES.fixture_cases()[1]
    dec = vorbis.VorbisPacketDecoder(engine=engine)
    for h in case.headers:
        assert dec.decode_packet(h) is None
    return [dec.decode_packet(p) for p in case.packets]


def run_round(engine, lanes, ogg_sends, with_other=True):
    """the Ogg fixture (sniffed), the WebM packets, an ADTS stream, a FLAC stream and, with_other, an Ogg stream that is not Vorbis, all
    spawned before anything is sent -> {name: ([AudioData], error)}"""
    from soundkit_amd import pipeline
    case = CASES.fixture_cases()[1]
    sched = pipeline.BatchScheduler(engine, entropy_threads=2, max_streams=16, lanes=lanes)
    try:
        handles = {"ogg": sched.spawn(), "webm": sched.spawn_vorbis_packets(*case.headers), "adts": sched.spawn(), "flac": sched.spawn()}
        sends = {"ogg": ogg_sends, "webm": case.packets, "adts": cut(read(ADTS), 3000), "flac": cut(read(FLAC), 4096)}
        if with_other:
            handles["other"] = sched.spawn()
            sends["other"] = [M.ogg_page(2, 0, 5, 0, [19], b"OpusHead" + bytes(11)) + M.ogg_page(4, 0, 5, 1, [1], b"\x00")]
        early = {name: feed(handles[name], sends[name]) for name in handles}
        out = {}
        for name, h in handles.items():
            rest, err = drain(h)
            out[name] = (early[name] + rest, err)
            h.cancel()
        return out
    finally:
        sched.close()


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("sends", ["641", "whole"])
def test_both_vorbis_streams_beside_adts_and_flac_in_one_round(engine, ogg_want, webm_want, lanes, sends):
    data = read(CASES.OGG)
    out = run_round(engine, lanes, cut(data, 641) if sends == "641" else [data])
    # the Ogg fixture: one AudioData per packet that yields frames (93 of 94), the last one cut to the final granule position
    ogg, err = out["ogg"]
    assert err is None and len(ogg) == 93
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 8000) for a in ogg)
    assert [a.data.size // 2 for a in ogg] == [256] * 92 + [128]
    assert np.array_equal(s16(ogg), ogg_want)
    # the WebM packets: one AudioData per packet that yields frames, each equal to VorbisPacketDecoder's
    webm, err = out["webm"]
    want = [w for w in webm_want if w.size]
    assert err is None and len(webm) == len(want) == len(webm_want) - 1
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 2, 44100) for a in webm)
    for a, w in zip(webm, want):
        assert np.array_equal(np.frombuffer(a.data.tobytes(), "<i2"), w)
    # the neighbours finish as they do alone
    adts, err = out["adts"]
    assert err is None and len(adts) == 48
    flac, err = out["flac"]
    assert err is None and np.array_equal(s16(flac), np.frombuffer(read(FLAC_TWIN), "<i2"))
    # an Ogg stream that is not Vorbis reaches no decoder: it ends without audio, as it did before Vorbis was taken
    other, err = out["other"]
    assert other == [] and err is None


def test_output_options_behind_the_decode(engine, ogg_want):
    """8 -> 16 kHz through the scheduler equals the PCM scheduler path on VorbisDecoder's samples: the same tick body behind both"""
    from soundkit_amd import pipeline
    from soundkit_amd.engine import FMT_S16LE
    sched = pipeline.BatchScheduler(engine, entropy_threads=2, max_streams=8)
    try:
        opt = pipeline.DecodeOptions(output_sample_rate=16000)
        h = sched.spawn(opt)
        early = feed(h, cut(read(CASES.OGG), 997))
        got, err = drain(h)
        h.cancel()
        assert err is None
        got = early + got
        p = sched.spawn_raw_pcm(pipeline.RawPcmFormat(8000, 1, FMT_S16LE), opt)
        early = feed(p, [ogg_want[at:at + 256].astype("<i2").tobytes() for at in range(0, ogg_want.size, 256)])
        want, err = drain(p)
        p.cancel()
        assert err is None
        want = early + want
        assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 16000) for a in got)
        assert s16(got).size > 2 * 23000 and np.array_equal(s16(got), s16(want))
    finally:
        sched.close()


def test_refusals_end_their_stream_with_the_parsers_texts(engine):
    from soundkit_amd import SoundkitError, pipeline
    data = read(CASES.OGG)
    case = CASES.fixture_cases()[1]
    sched = pipeline.BatchScheduler(engine, entropy_threads=2, max_streams=8)
    try:
        bad = bytearray(data)
        bad[9000] ^= 0x10  # inside the last page: its CRC fails, the packets of the pages in front have gone out
        h = sched.spawn()
        early = feed(h, cut(bytes(bad), 641))
        got, err = drain(h)
        h.cancel()
        assert err is not None and "Decoding failed: Ogg CRC mismatch on page" in str(err) and 0 < len(early + got) < 93
        h = sched.spawn()
        feed(h, [data[:9000]])  # cut inside a page
        got, err = drain(h)
        h.cancel()
        assert err is not None and "Decoding failed: truncated Ogg page" in str(err)
        h = sched.spawn_vorbis_packets(*case.headers)
        feed(h, [case.packets[0], b"\x01" + case.packets[1][1:], case.packets[2]])
        got, err = drain(h)
        h.cancel()
        assert err is not None and "Decoding failed: Vorbis packet rejected: not a Vorbis audio packet" in str(err)
        with pytest.raises(SoundkitError) as e:
            sched.spawn_vorbis_packets(case.headers[0], case.headers[1], case.headers[2][:100])
        assert "too short" in str(e.value)
    finally:
        sched.close()

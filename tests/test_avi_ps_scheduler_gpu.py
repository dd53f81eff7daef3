"""AVI and MPEG program streams through the batch scheduler: `spawn()` takes an AVI by its `RIFF....AVI ` and a program stream by its
`00 00 01 BA`, the stream is demuxed on its entropy thread, and from its config event on it is what its track is -- a raw PCM stream,
a stream of the AIFF tick (AVI's 8-bit samples, DVD LPCM's 24-bit groups) or an MPEG audio stream.  One round holds an AVI PCM stream, an
AVI 8-bit stream, an AVI MP3 stream, DVD LPCM at 16 and 24 bits and an MP2 program stream beside an ADTS and a WAV stream, sent in
4 KiB pieces (a stream with a chunk above 1 MiB in 64 KiB pieces): every stream's concatenated output equals its decode_file output, a refused stream ends alone with its text behind the
units that were complete in front of it, and the ADTS and the WAV stream give what they give in a round without the new streams."""
import pytest

import avi_builder as AB
import ps_builder as PB
from soundkit_amd import avi, pipeline, ps
from test_webm_scheduler_gpu import cut, run_round, shape, sniffed

pytestmark = pytest.mark.gpu

AVI = AB.cases()
PS = PB.cases()
ADTS = AB.golden("aac", "aac-stereo-48k.adts")
NEIGHBOURS = {"adts": (sniffed(), cut(ADTS, 3000)), "wav": (sniffed(), cut(AB.golden("wav_stereo_A_Tusk.wav")[:200000], 4096))}
# "avi 24 big": one chunk above 1 MiB of 3-byte frames -- the PCM pass takes it in slices of 1 MiB, which cut through frames
NEW = {"avi 24 big": AB.big_chunk()[0], "avi pcm": AVI["pcm16_split_frames"][0], "avi 24": AVI["pcm24"][0], "avi f32": AVI["f32"][0], "avi records": AVI["pcm16_records"][0],
       "avi avix": AVI["pcm16_avix"][0], "avi u8": AVI["u8_odd_chunks"][0], "avi mp3": AVI["mp3"][0], "ps lpcm16": PS["lpcm16_2ch"][0],
       "ps lpcm16 mpeg1": PS["lpcm16_48k_mono_mpeg1"][0], "ps lpcm24": PS["lpcm24_2ch"][0], "ps lpcm24 6ch": PS["lpcm24_6ch"][0], "ps mp2": PS["mp2"][0]}


def sends_of(name, data):
    """4 KiB pieces -- but 64 KiB for the stream whose first chunk is above 1 MiB: it has no output to give before that chunk is whole, and
    the helper that feeds a round waits for an output when the input queue (128 sends) is full, so its sends must fit the queue"""
    return cut(data, 65536 if name == "avi 24 big" else 4096)


def joined(audios):
    return b"".join(a.data.tobytes() for a in audios)


def clean(out):
    assert all(err is None for _, err in out.values()), {n: str(e) for n, (_, e) in out.items() if e is not None}


def decode_file(name, data, options, sched, engine):
    return (avi if name.startswith("avi") else ps).decode_file(data, options, scheduler=sched, engine=engine)[1]


@pytest.fixture(scope="module")
def alone(engine):
    """the neighbours in a round of their own"""
    out = run_round(engine, NEIGHBOURS)
    clean(out)
    assert len(out["adts"][0]) == 48 and len(out["wav"][0]) > 0
    return {name: shape(got) for name, (got, _) in out.items()}


@pytest.mark.parametrize("lanes", [1, 2])
def test_every_new_stream_equals_its_decode_file_beside_streams_that_do_not_change(engine, alone, lanes):
    streams = dict(NEIGHBOURS)
    streams.update({name: (sniffed(), sends_of(name, data)) for name, data in NEW.items()})
    sched = pipeline.BatchScheduler(engine, entropy_threads=3, max_streams=32, lanes=lanes)
    try:
        out = run_round(engine, streams, sched=sched)
        clean(out)
        for name, data in NEW.items():
            got = out[name][0]
            want = decode_file(name, data, None, sched, engine)
            assert joined(got) == joined(want) and len(joined(got)) > 4000, name
            assert {(a.bits_per_sample, a.channel_count, a.sampling_rate, a.audio_format, a.endianness) for a in got} == \
                   {(a.bits_per_sample, a.channel_count, a.sampling_rate, a.audio_format, a.endianness) for a in want}, name
    finally:
        sched.close()
    for name in NEIGHBOURS:
        assert shape(out[name][0]) == alone[name], name


def test_under_output_options_every_new_stream_equals_its_decode_file(engine):
    options = pipeline.DecodeOptions(16, 16000, 1)
    new = {name: data for name, data in NEW.items() if name != "ps lpcm24 6ch"}  # (six channels behind a conversion: the test below)
    sched = pipeline.BatchScheduler(engine, entropy_threads=3, max_streams=32)
    try:
        out = run_round(engine, {name: (sniffed(options), sends_of(name, data)) for name, data in new.items()}, sched=sched)
        clean(out)
        for name, data in new.items():
            got = out[name][0]
            assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 16000) for a in got), name
            assert joined(got) == joined(decode_file(name, data, options, sched, engine)) and len(joined(got)) > 1400, name
    finally:
        sched.close()


def test_three_to_eight_channels_need_the_wide_pool_as_any_pcm_stream_does(engine):
    import soundkit_amd
    options = pipeline.DecodeOptions(16, 16000, 1)
    streams = {"6ch": (sniffed(options), cut(PS["lpcm24_6ch"][0], 4096)), "8ch 16": (sniffed(options), cut(PS["lpcm16_8ch"][0], 4096))}
    out = run_round(engine, streams)
    for name in streams:
        assert out[name][0] == [] and str(out[name][1]) == "Decoding failed: conversion of PCM with more than 2 channels is not supported", name
    wide = soundkit_amd.Engine(0, 64)
    try:
        wide.enable_wide_pcm(8)
        sched = pipeline.BatchScheduler(wide, entropy_threads=2, max_streams=8)
        try:
            out = run_round(wide, streams, sched=sched)
            clean(out)
            for name, case in (("6ch", "lpcm24_6ch"), ("8ch 16", "lpcm16_8ch")):
                want = ps.decode_file(PS[case][0], options, scheduler=sched, engine=wide)[1]
                assert joined(out[name][0]) == joined(want) and len(joined(want)) > 1400, name
        finally:
            sched.close()
    finally:
        wide.close()


def test_refused_streams_end_alone_with_their_text_behind_the_units_in_front(engine, alone):
    pcm = AB.waveformat(1, 1, 16000, 16)
    wma = AB.riff(b"AVI ", AB.hdrl(AB.strl(b"auds", AB.waveformat(0x161, 2, 44100, 16))), AB.lst(b"movi", AB.wb(0, bytes(400))))
    ac3 = AB.riff(b"AVI ", AB.hdrl(AB.strl(b"auds", AB.waveformat(0x2000, 2, 48000, 0))), AB.lst(b"movi", AB.wb(0, bytes(400))))
    depth = AB.riff(b"AVI ", AB.hdrl(AB.strl(b"auds", AB.waveformat(1, 2, 48000, 12))), AB.lst(b"movi", AB.wb(0, bytes(400))))
    no_audio = AB.riff(b"AVI ", AB.hdrl(AB.video_strl()), AB.lst(b"movi", AB.dc(0)))
    many = AB.riff(b"AVI ", AB.hdrl(AB.strl(b"auds", AB.waveformat(1, 33, 8000, 8))), AB.lst(b"movi", AB.wb(0, bytes(66))))
    # two whole chunks, then bytes that are no chunk table: the chunks' frames are delivered, then the text
    trailing = AB.riff(b"AVI ", AB.hdrl(AB.strl(b"auds", pcm)), AB.lst(b"movi", AB.wb(0, AB.S16[:2000]), AB.wb(0, AB.S16[2000:4000]), b"\x00\x00\x07"))
    head = PB.pack_header() + PB.system_header()
    good = [PB.pes2(0xBD, PB.lpcm_header(16, 48000, 2, frames=k) + PB.pack16(AB.S16_STEREO[800 * k:800 * (k + 1)]), 90000 + k) for k in range(3)]
    twenty = head + PB.pes2(0xBD, PB.lpcm_header(20, 48000, 2) + bytes(100), 1)
    changes = head + b"".join(good) + PB.pes2(0xBD, PB.lpcm_header(24, 48000, 2) + bytes(120), 5)
    streams = dict(NEIGHBOURS)
    streams.update({name: (sniffed(), cut(data, 4096)) for name, data in
                    dict(wma=wma, ac3=ac3, depth=depth, no_audio=no_audio, many=many, trailing=trailing, twenty=twenty, changes=changes, no_track=head + PB.video()).items()})
    out = run_round(engine, streams)
    for name, text in (("wma", "AVI WMA decoding is not implemented"), ("ac3", "AVI AC-3 audio is not built"), ("depth", "unsupported AVI integer PCM depth 12"),
                       ("no_audio", "AVI has no audio stream"), ("many", "AVI 8-bit PCM with more than 32 channels is not built"), ("twenty", "20-bit DVD LPCM decoding is not implemented"),
                       ("no_track", "MPEG-PS has no supported DVD LPCM track")):
        got, err = out[name]
        assert got == [] and str(err) == "Invalid input format: " + text, (name, str(err))
    got, err = out["trailing"]
    assert str(err) == "Invalid input format: AVI chunk table has trailing data" and joined(got) == AB.S16[:4000]
    got, err = out["changes"]
    assert str(err) == "Invalid input format: DVD LPCM format changes mid-stream" and joined(got) == PB.pack16(AB.S16_STEREO[:2400])
    for name in NEIGHBOURS:
        assert out[name][1] is None and shape(out[name][0]) == alone[name], name

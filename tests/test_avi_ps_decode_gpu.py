"""soundkit_amd.avi.decode_file and soundkit_amd.ps.decode_file on the device, on the files tests/avi_builder.py and tests/ps_builder.py
write.  With no options a PCM track gives back the bytes it was written from (8-bit widened by `(u8 - 128) << 8`, 24-bit DVD LPCM
unpacked, 16-bit DVD LPCM big-endian as it lies in the stream); down to 16 kHz mono s16 it equals the same PCM as a WAV file through
spawn(), the path that was there before the containers; an MP3 track in AVI and an MP2 track in a program stream equal Mp3Decoder on
the elementary stream.  Every comparison is bit for bit."""
import struct

import numpy as np
import pytest

import avi_builder as AB
import ps_builder as PB
from soundkit_amd import SoundkitError, avi, media_file, pipeline, ps
from soundkit_amd.audio_types import Endianness
from test_ts_decode_gpu import mpa_samples

pytestmark = pytest.mark.gpu
OPTIONS = pipeline.DecodeOptions(16, 16000, 1)
AVI = dict(AB.cases(), pcm24_big_chunk=AB.big_chunk())  # (a chunk above 1 MiB: the Python demuxer's packet buffer grows)
PS = PB.cases()
GUID_TAIL = bytes([0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])


def joined(audios):
    return b"".join(a.data.tobytes() for a in audios)


def wav_of(pcm, tag, channels, rate, bits):
    """little-endian PCM as a WAV file: a plain fmt chunk for 16-bit mono / stereo, WAVE_FORMAT_EXTENSIBLE otherwise"""
    align = channels * bits // 8
    if bits == 16 and channels <= 2:
        fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, bits)
    else:
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, channels, rate, rate * align, align, bits, 22, bits, 0) + struct.pack("<H", tag) + GUID_TAIL
    body = b"WAVE" + AB.chunk(b"fmt ", fmt) + AB.chunk(b"data", pcm)
    return b"RIFF" + struct.pack("<I", len(body)) + body


@pytest.fixture(scope="module")
def wide():
    """an engine with wide slots and its scheduler: the 6- and 8-channel tracks behind a conversion need them, as any PCM stream does"""
    import soundkit_amd
    eng = soundkit_amd.Engine(0, 64)
    eng.enable_wide_pcm(8)
    s = pipeline.BatchScheduler(eng, entropy_threads=2, max_streams=4)
    yield eng, s
    s.close()
    eng.close()


def widened(u8):
    return ((np.frombuffer(u8, np.uint8).astype(np.int16) - 128) << 8).astype("<i2").tobytes()


# ---- AVI -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(n for n in AVI if n != "mp3"))
def test_an_avi_pcm_track_is_its_bytes_and_converts_like_a_wav_file(wide, name):
    engine, sched = wide
    data, tag, channels, rate, bits, index, track = AVI[name]
    config, got = avi.decode_file(data, scheduler=sched, engine=engine)
    assert (config.stream_index, config.format_tag, config.channels, config.sample_rate, config.bits_per_sample) == (index, tag, channels, rate, bits)
    pcm, out_bits = (widened(track), 16) if bits == 8 else (track, bits)
    assert joined(got) == pcm
    frame = channels * out_bits // 8
    assert [len(a.data) // frame for a in got] == [4096] * (len(pcm) // frame // 4096) + [len(pcm) // frame % 4096]
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate, a.endianness) == (out_bits, channels, rate, Endianness.LittleEndian) for a in got)
    assert all(a.audio_format.name == ("PCMFloat" if tag == 3 else "PCMSigned") for a in got)
    _, down = avi.decode_file(data, OPTIONS, scheduler=sched, engine=engine)
    twin = media_file.decode_complete_stream(wav_of(pcm, tag, channels, rate, out_bits), OPTIONS, sched)
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 16000) for a in down)
    assert joined(down) == joined(twin) and len(joined(down)) >= 2 * 5900


def test_the_cut_file_decodes_to_the_chunks_in_front_of_the_cut(wide):
    engine, sched = wide
    data, front = AB.cut_inside_a_chunk()
    _, got = avi.decode_file(data, scheduler=sched, engine=engine)
    assert joined(got) == front


def test_an_mp3_track_in_avi_is_mp3decoder_on_the_elementary_stream(wide):
    engine, sched = wide
    want = mpa_samples(engine, AB.MP3)
    config, got = avi.decode_file(AVI["mp3"][0], scheduler=sched, engine=engine)
    assert config.format_tag == 0x55 and all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 16000) for a in got)
    assert joined(got) == want.astype("<i2").tobytes() and want.size > 16000


def test_avi_refusals_on_the_device_path(wide):
    engine, sched = wide
    silent = AB.riff(b"AVI ", AB.hdrl(AB.strl(b"auds", AB.waveformat(0x55, 1, 16000, 0))), AB.lst(b"movi", AB.wb(0, bytes(600))))
    with pytest.raises(SoundkitError, match="Decoding failed: AVI audio track emitted no frames"):  # 600 zero bytes hold no MPEG audio frame
        avi.decode_file(silent, scheduler=sched, engine=engine)


# ---- MPEG program streams ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(n for n in PS if PS[n][1] == "pcm-dvd"))
def test_a_dvd_lpcm_track_is_its_pcm_and_converts_like_a_wav_file(wide, name):
    engine, sched = wide
    data, kind, track, rate, channels, bits, pcm = PS[name]
    config, got = ps.decode_file(data, scheduler=sched, engine=engine)
    assert (config.kind, config.sample_rate, config.channels, config.bits_per_sample) == ("pcm-dvd", rate, channels, bits)
    # 16 bits: big-endian as it lies in the stream; 24 bits: unpacked on the device
    assert joined(got) == (track if bits == 16 else pcm)
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (bits, channels, rate) for a in got)
    assert all(a.endianness == (Endianness.BigEndian if bits == 16 else Endianness.LittleEndian) for a in got)
    frame = channels * bits // 8
    assert [len(a.data) // frame for a in got] == [4096] * (len(pcm) // frame // 4096) + ([len(pcm) // frame % 4096] if len(pcm) // frame % 4096 else [])
    _, down = ps.decode_file(data, OPTIONS, scheduler=sched, engine=engine)
    twin = media_file.decode_complete_stream(wav_of(pcm, 1, channels, rate, bits), OPTIONS, sched)
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 16000) for a in down)
    assert joined(down) == joined(twin) and len(joined(down)) >= 2 * 700


def test_an_mpeg_audio_track_that_decodes_to_nothing_is_refused_as_an_avi_mp3_track_is(wide):
    engine, sched = wide
    silent = PB.pack_header() + PB.pes2(0xC0, bytes(600), 1)  # 600 zero bytes hold no MPEG audio frame
    with pytest.raises(SoundkitError, match="Decoding failed: MPEG-PS MPEG audio track emitted no frames"):
        ps.decode_file(silent, scheduler=sched, engine=engine)


@pytest.mark.parametrize("name", ["mp2", "mp2_mpeg1_c1"])
def test_an_mp2_track_in_a_program_stream_is_mp3decoder_on_the_elementary_stream(wide, name):
    engine, sched = wide
    data, kind, es = PS[name][:3]
    want = mpa_samples(engine, es)
    config, got = ps.decode_file(data, scheduler=sched, engine=engine)
    assert (config.kind, config.stream_id) == ("mpeg-audio", 0xC1 if name.endswith("c1") else 0xC0)
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 2, 48000) for a in got)
    assert joined(got) == want.astype("<i2").tobytes() and want.size >= 12 * 1152 * 2


def test_lpcm_wins_over_mpeg_audio_in_a_file(wide):
    engine, sched = wide
    head = PB.pack_header() + PB.system_header()
    lpcm = PB.pes2(0xBD, PB.lpcm_header(16, 48000, 2) + bytes(range(64)), 1)
    mixed = head + PB.pes2(0xC0, PB.MP2[:576], 2) + lpcm + PB.pes2(0xC0, PB.MP2[576:1152], 3) + lpcm
    config, got = ps.decode_file(mixed, scheduler=sched, engine=engine)
    assert config.kind == "pcm-dvd" and joined(got) == bytes(range(64)) * 2

"""soundkit_amd.webm's WebmDecoder and decode_file on the device: every comparison is bit for bit against a decoder that was there
before the container -- VorbisPacketDecoder on the packets, VorbisDecoder on the Ogg file the packets were taken from, the ADTS
decoder, FlacDecoder -- so the container adds nothing and loses nothing, and DiscardPadding cuts exactly its frames."""
import numpy as np
import pytest

import webm_cases as CASES
import webm_vorbis
from soundkit_amd import SoundkitError, pipeline, webm

pytestmark = pytest.mark.gpu


def decode(engine, data, piece):
    """WebmDecoder over `data` in pieces -> (s16 samples of all calls, the AudioData)"""
    d, got = webm.WebmDecoder(engine), []
    try:
        for at in range(0, len(data), piece):
            a = d.add(data[at:at + piece])
            if a is not None:
                got.append(a)
        a = d.finish()
        if a is not None:
            got.append(a)
    finally:
        d.close()
    assert all(a.bits_per_sample == 16 for a in got)
    return np.concatenate([np.frombuffer(a.data.tobytes(), "<i2") for a in got]) if got else np.zeros(0, np.int16), got


@pytest.fixture(scope="module")
def ogg_want(engine):
    """VorbisDecoder over the Ogg fixture: per audio packet 256 frames, none for the first, 128 for the last"""
    from soundkit_amd import vorbis
    dec = vorbis.VorbisDecoder(engine=engine)
    got = [dec.add(CASES.golden("vorbis", "A_Tusk_is_used_to_make_costly_gifts.ogg")), dec.finish()]
    want = np.concatenate([np.frombuffer(a.data.tobytes(), "<i2") for a in got if a is not None])
    assert want.size == 23680
    return want


def test_vorbis_fixture_equals_the_packet_decoder_however_it_is_cut(engine):
    from soundkit_amd import vorbis
    data = CASES.fixture("vorbis")
    headers, packets = webm_vorbis.vorbis_track(data)
    dec = vorbis.VorbisPacketDecoder(engine=engine)
    for h in headers:
        assert dec.decode_packet(h) is None
    want = np.concatenate([dec.decode_packet(p) for p in packets])
    assert want.size > 2 * 40000
    whole, audios = decode(engine, data, len(data))
    assert len(audios) == 1 and (audios[0].channel_count, audios[0].sampling_rate) == (2, 44100)
    assert np.array_equal(whole, want)
    for piece in (641, 7):
        got, audios = decode(engine, data, piece)
        assert np.array_equal(got, want), piece
        assert len(audios) > 1


def test_discard_padding_at_the_back_is_the_ogg_decoders_cut(engine, ogg_want):
    data, _, packets = CASES.wrapped_ogg({93: 16000000})
    assert len(packets) == 94
    got, audios = decode(engine, data, 1000)
    assert (audios[0].channel_count, audios[0].sampling_rate) == (1, 8000)
    assert got.size == 23680 and np.array_equal(got, ogg_want)
    uncut, _ = decode(engine, CASES.wrapped_ogg()[0], 1000)
    assert uncut.size == 93 * 256 and np.array_equal(uncut[:23680], ogg_want)


def test_discard_padding_at_the_front_takes_that_blocks_front_and_nothing_else(engine, ogg_want):
    data, _, _ = CASES.wrapped_ogg({1: -16000000, 93: 16000000})  # the second audio packet: the first that yields frames
    got, _ = decode(engine, data, 1000)
    assert np.array_equal(got, ogg_want[128:])
    both, _ = decode(engine, CASES.wrapped_ogg({2: -4125000, 93: 16000000})[0], len(data))  # 33 frames off the front of the second 256
    assert np.array_equal(both, np.concatenate([ogg_want[:256], ogg_want[256 + 33:]]))


def test_aac_track_equals_the_adts_decoder(engine):
    from soundkit_amd.aac import AacDecoder, decode_i16_with_drain
    data, adts = CASES.wrapped_aac()
    dec, out = AacDecoder(engine), np.zeros(64 * 1024, np.int16)
    want = np.concatenate([np.concatenate(decode_i16_with_drain(dec, adts[at:at + 4096], out) or [np.zeros(0, np.int16)]) for at in range(0, len(adts), 4096)])
    dec.close()
    assert want.size == 48 * 1024
    for piece in (len(data), 1000):
        got, audios = decode(engine, data, piece)
        assert (audios[0].channel_count, audios[0].sampling_rate) == (1, 16000)
        assert np.array_equal(got, want), piece


def test_flac_track_equals_the_flac_decoder(engine):
    from soundkit_amd.flac import FlacDecoder
    data, flac = CASES.wrapped_flac()
    dec, out, want = FlacDecoder(engine), np.zeros(1 << 18, np.int16), []
    n = dec.decode_i16(flac, out)
    while n:
        want.append(out[:n].copy())
        n = dec.decode_i16(b"", out)
    rate, channels = dec.sample_rate(), dec.channels()
    dec.close()
    want = np.concatenate(want)
    assert want.size > 20000
    for piece in (len(data), 1000):
        got, audios = decode(engine, data, piece)
        assert (audios[0].channel_count, audios[0].sampling_rate) == (channels, rate)
        assert np.array_equal(got, want), piece


def test_opus_is_refused_with_the_references_text(engine):
    with pytest.raises(SoundkitError) as e:
        decode(engine, CASES.fixture("opus"), 4096)
    assert str(e.value).endswith(": unsupported or disabled WebM codec: A_OPUS")


def test_decode_file_applies_the_options_the_unwrapped_stream_gets(engine):
    """to 16 kHz mono s16: the WebM fixture against its packets' samples through the same output stage"""
    from soundkit_amd import alac, vorbis
    data = CASES.fixture("vorbis")
    headers, packets = webm_vorbis.vorbis_track(data)
    dec = vorbis.VorbisPacketDecoder(engine=engine)
    for h in headers:
        dec.decode_packet(h)
    samples = np.concatenate([dec.decode_packet(p) for p in packets])
    options = pipeline.DecodeOptions(16, 16000, 1)
    sched = pipeline.BatchScheduler(engine, entropy_threads=2, max_streams=4)
    try:
        config, got = webm.decode_file(data, options, scheduler=sched, engine=engine)
        want = alac.output_stage([samples.astype("<i2").tobytes()], 44100, 2, 16, options, sched)
        plain_config, plain = webm.decode_file(data, None, scheduler=sched, engine=engine)
    finally:
        sched.close()
    assert config.codec_id == "A_VORBIS" and all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 16000) for a in got)
    assert b"".join(a.data.tobytes() for a in got) == b"".join(a.data.tobytes() for a in want)
    assert sum(a.data.size for a in got) > 2 * 14000
    assert b"".join(a.data.tobytes() for a in plain) == samples.astype("<i2").tobytes()

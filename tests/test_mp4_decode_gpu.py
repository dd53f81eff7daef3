"""mp4.decode_file (decode_seekable_mp4_audio for `aac` and `alac` tracks): the container is walked on the host, the packets go to the
decoders that were there before it, the edit list trims what they give.  The AAC fixture against the ADTS decoder on its ADTS twin, the
ALAC fixture against the CAF fixture's recording and decode_caf, fragmented builds of the same units, and the output options."""
import os
import wave

import numpy as np
import pytest

import mp4_builder as B
import mp4_cases as CASES
from soundkit_amd import SoundkitError, aac, alac, mp4, pipeline

pytestmark = pytest.mark.gpu


def joined(audio):
    return b"".join(a.data.tobytes() for a in audio)


@pytest.fixture(scope="module")
def adts_pcm(engine):
    """the ADTS decoder on mono16k_A_Tusk.aac: 48 frames of 1024"""
    dec, out = aac.AacDecoder(engine), np.zeros(64 * 1024, np.int16)
    got = np.concatenate(aac.decode_i16_with_drain(dec, CASES.golden("aac", "mono16k_A_Tusk.aac"), out))
    dec.close()
    assert got.size == 48 * 1024
    return got


def test_the_aac_fixture_is_the_adts_decode_trimmed_by_its_edit_list(engine, adts_pcm):
    config, audio = mp4.decode_file(CASES.fixture("mac_aac_A_Tusk.m4a"), engine=engine)
    assert (config.codec, config.edit) == ("aac", (0, 1024, 47360))
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 16000) for a in audio)
    assert [len(a.data) // 2 for a in audio] == [1024] * 46 + [256]  # the first packet is all priming
    assert joined(audio) == adts_pcm[1024:48384].astype("<i2").tobytes() and len(joined(audio)) == 2 * 47360


def test_fragmented_and_moov_first_builds_give_the_same_bytes(engine, adts_pcm):
    cfg, units = CASES.mac_aac_units()
    want = adts_pcm[1024:48384].astype("<i2").tobytes()
    edit = [(2960 * 600 // 1000, 1024)]
    for data in (B.regular(cfg, units, edit=edit), B.fragmented(cfg, units, per_moof=7, per_trun=3, edit=edit),
                 B.fragmented(cfg, units, per_moof=48, base="none", video=True, edit=edit)):
        config, audio = mp4.decode_file(data, engine=engine)
        assert joined(audio) == want, config
    # without an edit list every frame stays
    _, audio = mp4.decode_file(B.fragmented(cfg, units, per_moof=16), engine=engine)
    assert joined(audio) == adts_pcm.astype("<i2").tobytes()


def test_the_alac_fixture_is_the_caf_recording(engine):
    rec = wave.open(os.path.join(CASES.GOLDEN, "alac", "A_Tusk_is_used_to_make_costly_gifts.decoded.wav"))
    twin = rec.readframes(rec.getnframes())
    caf = CASES.golden("alac", "A_Tusk_is_used_to_make_costly_gifts.caf")
    _, from_caf = alac.decode_caf(caf, engine=engine)
    config, audio = mp4.decode_file(CASES.fixture("alac_A_Tusk.m4a"), engine=engine)
    assert config.codec == "alac" and all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 8000) for a in audio)
    assert joined(audio) == twin == joined(from_caf) and len(twin) == 2 * 23680
    assert [a.data.tobytes() for a in audio] == [a.data.tobytes() for a in from_caf]
    # a fragmented build of the same packets: the demuxer's walk instead of the index
    cfg, packets, durations = CASES.alac_units()
    _, audio = mp4.decode_file(B.fragmented(cfg, packets, durations=durations, per_moof=2, edit=[(23680 * 600 // 8000, 0)]), engine=engine)
    assert joined(audio) == twin
    _, audio = mp4.decode_file(B.fragmented(cfg, packets, durations=durations, per_moof=4, per_trun=1), engine=engine)
    assert joined(audio) == twin  # no edit list: whole packets, and the last one states its own 3200 frames


def test_output_options_are_what_decode_caf_gives(engine):
    opts = pipeline.DecodeOptions(24, 8000, None)
    sched = pipeline.BatchScheduler(engine, max_streams=8)
    try:
        _, want = alac.decode_caf(CASES.golden("alac", "A_Tusk_is_used_to_make_costly_gifts.caf"), opts, scheduler=sched, engine=engine)
        _, got = mp4.decode_file(CASES.fixture("alac_A_Tusk.m4a"), opts, scheduler=sched, engine=engine)
        down = pipeline.DecodeOptions(16, 16000, None)  # through the resampler and its flush
        _, want_down = alac.decode_caf(CASES.golden("alac", "A_Tusk_is_used_to_make_costly_gifts.caf"), down, scheduler=sched, engine=engine)
        _, got_down = mp4.decode_file(CASES.fixture("alac_A_Tusk.m4a"), down, scheduler=sched, engine=engine)
    finally:
        sched.close()
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (24, 1, 8000) for a in got)
    assert [a.data.tobytes() for a in got] == [a.data.tobytes() for a in want] and len(joined(got)) == 3 * 23680
    assert [a.data.tobytes() for a in got_down] == [a.data.tobytes() for a in want_down] and len(joined(got_down)) > 2 * 46000


def test_refusals(engine):
    cfg, units = CASES.mac_aac_units()
    sbr = dict(cfg, private=bytes([0x2c, 0x0a, 0x88, 0x00]))  # object type 5 in front: SBR signalled explicitly
    with pytest.raises(SoundkitError) as e:
        mp4.decode_file(B.regular(sbr, units), engine=engine)
    assert "AAC-LC decoder init: UnsupportedFeature" in str(e.value)
    with pytest.raises(SoundkitError) as e:  # an edit that keeps nothing of what is there
        mp4.decode_file(B.regular(cfg, units[:3], edit=[(600, 1 << 20)]), engine=engine)
    assert str(e.value).endswith("Decoding failed: MP4 aac track emitted no audio frames")

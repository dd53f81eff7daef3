"""The CPU part of tests/test_family_rounds_gpu.py: the stream table of tests/family_rounds.py is what that file takes it for -- every
stream has at least twelve units, the models' output for the chosen cuts is the reference's recording, the round-sharing condition is far
from its edge, and every damaged stream fails in its model at the unit the GPU test expects."""
import family_rounds as T


def test_every_stream_has_at_least_twelve_units():
    plain, converted, main = T.table()
    assert len(plain) == 14 and len(converted) == 14 and len(main) == 3
    for s in plain + converted + main:
        assert s.units >= 12, (s.name, s.units)
    # the framers hold bytes back: some GSM and G.726 sends complete nothing, others leave a partial packet or group behind
    by_name = {s.name: s for s in plain}
    assert all(len(x) % 33 for x in by_name["GSM standard"].sends) and by_name["GSM Microsoft"].units < len(by_name["GSM Microsoft"].sends)
    for name, group in (("G.726 24k right", 3), ("G.726 40k left", 5)):
        assert any(len(x) % group for x in by_name[name].sends), name
    # every family twice or more, every converted stream with options that change something
    for s in converted:
        bits, rate, channels = s.options
        assert (bits, rate or s.shape[2], channels or s.shape[1]) != s.shape, s.name
    assert {s.options for s in converted} >= {T.TO16K, T.TO8K, (24, None, None), (16, None, 2)}


def test_the_models_output_for_these_cuts_is_the_recording():
    plain, _, _ = T.table()
    twins = 0
    for s in plain:
        units, text = s.model()
        assert text is None and all(units), s.name
        width = s.shape[0] // 8 * s.shape[1]
        assert all(len(u) % width == 0 for u in units) or s.name == "G.711 A-law stereo", s.name
        if s.twin is not None:
            assert b"".join(units) == s.twin, s.name
            twins += 1
    # without a recording, the model alone: the two AIFF-C streams (IMA4 is lossy, the 24-bit form has no twin), the built ALAC stream, stereo A-law
    assert twins == 10


def test_the_round_sharing_condition_is_far_from_its_edge():
    plain, converted, main = T.table()
    for quota in (1, 3):
        rounds, ideal = T.rounds_without_sharing(plain + converted + main, quota)
        print("quota %d: %d rounds without sharing, %d at best" % (quota, rounds, ideal))
        assert rounds >= 4 * ideal, (quota, rounds, ideal)
    for quota in (8, 32):  # the defaults behind a budget of 0 (host and device front end)
        rounds, ideal = T.rounds_without_sharing(plain + converted + main, quota)
        print("quota %d: %d rounds without sharing, %d at best" % (quota, rounds, ideal))


def test_every_damaged_stream_fails_in_its_model_where_the_gpu_test_expects_it():
    streams = T.failing_streams()
    assert len(streams) == 9
    for s in streams:
        units, text = s.model()
        assert text is not None and text == s.end_text(), (s.name, text)
        assert len(units) == s.good_units >= 4, (s.name, len(units))
    by_name = {s.name: s for s in streams}
    assert by_name["AIFF-C truncated inside the sound"].end_text().startswith("Decoding failed: truncated AIFF stream in state Audio {")
    # the two device rejections pass the host's framers: the FLAC frame's CRCs hold, the ALAC packet's frame count reads
    import alac_model
    import flac_model
    bad = by_name["ALAC, a packet the device rejects"]
    assert alac_model.packet_frames(alac_model.parse_cookie(bad.spawn[1]), bad.sends[5]) == 4096
    data = b"".join(by_name["FLAC, a frame the device rejects"].sends)
    info, _, pos = flac_model.split_stream(data)
    for _ in range(5):
        pos += flac_model.decode_frame(data[pos:], info)[0]["frame_bytes"]
    h = flac_model.parse_header(data[pos:], info)
    assert h["block_size"] == 90

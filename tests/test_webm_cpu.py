"""The WebM / Matroska demuxer on the host (csrc/webm_stream.h through soundkit_amd.webm): its events against tests/webm_model.py on the
two fixtures and on the files tests/webm_builder.py writes, whole and in pieces of 7 and of 4096 bytes; every refusal with its text;
the budgets; the discard-padding conversion; and a sanitizer fuzz (tests/fuzz_webm.cpp).  No GPU."""
import os
import struct
import subprocess

import pytest

import webm_builder as B
import webm_cases as CASES
import webm_model as M
import webm_vorbis
from soundkit_amd import SoundkitError, lib, webm

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = dict({name: CASES.fixture(name) for name in CASES.FIXTURES}, **CASES.builder_cases())
AAC = B.track(1, b"A_AAC", private=b"\x14\x08", rate=16000.0, channels=1, default_duration=64000000)
FRAME = [bytes(range(9))]


def demux_in_pieces(data, piece):
    """-> the events through WebmAudioDemuxer; a refusal raises with .events = what came before it"""
    d, events = webm.WebmAudioDemuxer(), []
    try:
        for at in range(0, len(data), piece):
            events += d.add(data[at:at + piece])
        events += d.finish()
    except SoundkitError as e:
        e.events = events + e.events
        raise
    finally:
        d.close()
    return events


def as_model(events):
    """the demuxer's events in the model's form"""
    out = []
    for e in events:
        if isinstance(e, webm.WebmAudioConfig):
            out.append(("config", dict(number=e.track_number, kind="audio", codec_id=e.codec_id, private=e.codec_private, rate=e.sample_rate, channels=e.channels,
                                       default_duration=e.default_duration_ns, codec_delay=e.codec_delay_ns, seek_pre_roll=e.seek_pre_roll_ns,
                                       scale=e.track_timestamp_scale, prefix=e.header_stripping_prefix, timecode_scale_ns=e.timecode_scale_ns)))
        else:
            out.append(("packet", dict(track=e.track_number, codec_id=e.codec_id, data=e.data, timestamp_ns=e.timestamp_ns, duration_ns=e.duration_ns,
                                       discard_padding_ns=e.discard_padding_ns)))
    return out


def refused(fn, text):
    with pytest.raises(SoundkitError) as e:
        fn()
    assert str(e.value).endswith(": " + text), str(e.value)
    return e.value


def refuses(data, text, piece=None):
    """the demuxer and the model refuse `data` with `text`, after the same events"""
    events, error = M.demux(data)
    assert error == text, error
    e = refused(lambda: demux_in_pieces(data, piece or max(len(data), 1)), text)
    assert as_model(e.events) == events


# ---- events against the model ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("piece", [0, 7, 4096])
@pytest.mark.parametrize("name", sorted(FILES))
def test_demuxer_matches_model(name, piece):
    data = FILES[name]
    events, error = M.demux(data)
    assert error is None and sum(kind == "packet" for kind, _ in events) > 0
    assert as_model(demux_in_pieces(data, piece or len(data))) == events


def test_vorbis_fixture_is_what_the_test_walker_finds():
    data = CASES.fixture("vorbis")
    events = demux_in_pieces(data, 641)
    headers, packets = webm_vorbis.vorbis_track(data)
    config = events[0]
    assert (config.codec_id, config.sample_rate, config.channels, config.track_number) == ("A_VORBIS", 44100, 2, 1)
    assert [len(h) for h in webm.vorbis_headers(config.codec_private)] == [30, 93, 4140]
    assert webm.vorbis_headers(config.codec_private) == headers
    assert len(events) == 57 and [e.data for e in events[1:]] == packets
    assert all(e.duration_ns is None and e.discard_padding_ns is None for e in events[1:])


def test_opus_fixture():
    events = demux_in_pieces(CASES.fixture("opus"), 4096)
    config, packets = events[0], events[1:]
    assert (config.codec_id, config.sample_rate, config.channels) == ("A_OPUS", 48000, 1)
    assert config.codec_private == b"OpusHead\x01\x01\x38\x01\x80\xbb\x00\x00\x00\x00\x00"
    assert (config.pre_skip, config.output_gain, config.mapping_family) == (312, 0, 0)
    assert (config.codec_delay_ns, config.seek_pre_roll_ns) == (6500000, 80000000)
    assert len(packets) == 149
    assert [(k, p.discard_padding_ns) for k, p in enumerate(packets) if p.discard_padding_ns is not None] == [(148, 13500000)]
    assert {p.duration_ns for p in packets} == {20000000}  # from each packet's TOC byte: the track declares none
    assert [p.timestamp_ns for p in packets[:3]] == [-6500000, 14500000, 34500000]


def test_built_cases_hold_what_they_are_named_for():
    packets = lambda name: [e for kind, e in M.demux(FILES[name])[0] if kind == "packet"]  # noqa: E731
    assert [len(p["data"]) for p in packets("lacing_xiph")] == [9, 300, 255, 7, 510]  # the empty frame is dropped
    assert [p["timestamp_ns"] for p in packets("lacing_xiph")] == [0, 64000000, 128000000, 192000000, 256000000]  # ... and takes no time
    assert [len(p["data"]) for p in packets("lacing_ebml")] == [9, 100, 90, 400, 8, 70]
    groups = packets("block_groups")
    assert [p["duration_ns"] for p in groups] == [None, None, 3000000, 3000000, 3000000, None, 4000000, 3500000, 3500000, None]
    assert [p["discard_padding_ns"] for p in groups] == [None, None, None, None, None, 16000000, -1, None, -129, None]
    assert all(p["data"][:2] == b"\x21\x1a" for p in packets("header_stripping")) and len(packets("header_stripping")) == 3
    assert [p["timestamp_ns"] for p in packets("scales")] == [
        0 * 833332.5 - 6500000, 10 * 833332.5 - 6500000, 16 * 833332.5 - 6500000,
        16 * 833332.5 - 6500000 + 2499998 // 2]  # ticks x 333 333 ns x 2.5 minus CodecDelay; the laced frame a half of round(3 x 833 332.5) later
    both = M.demux(FILES["two_audio_and_video"])[0]
    assert [e["number"] for kind, e in both if kind == "config"] == [2, 130]
    assert [(e["track"], e["duration_ns"]) for kind, e in both if kind == "packet"] == [(2, 64000000), (130, 20000000), (130, 20000000), (130, 10000000),
                                                                                        (130, 40000000), (2, 64000000)]
    assert [e["codec_id"] for kind, e in M.demux(FILES["duplicate_track_number"])[0] if kind == "config"] == ["A_AAC"]
    assert [(e["rate"], e["channels"]) for kind, e in M.demux(FILES["rate_and_channels_by_default"])[0] if kind == "config"] == [(48000, 2)]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def one_block(tracks, block, **more):
    return B.webm(tracks, [B.cluster(0, [block])], **more)


def test_refusals_from_the_header():
    refuses(b"\x1a\x45\xdf\xa4" + bytes(8), "invalid WebM: expected EBML header, got 0x1A45DFA4")
    refuses(bytes(8), "invalid WebM EBML element ID")
    tail = B.el(B.SEGMENT, b"")
    refuses(B.ebml_header(read_version=2) + tail, "unsupported EBML read version 2")
    refuses(B.ebml_header(max_id=5) + tail, "unsupported EBML element width")
    refuses(B.ebml_header(max_size=9) + tail, "unsupported EBML element width")
    refuses(B.ebml_header(doc_type=b"mkv") + tail, "unsupported EBML DocType mkv")
    refuses(B.ebml_header(doc_type=None) + tail, "WebM EBML header is missing DocType")
    refuses(B.ebml_header(doc_read_version=5) + tail, "unsupported Matroska DocTypeReadVersion 5")
    refuses(B.ebml_header(extra=B.el(0xEC, b"", size=40)) + tail, "truncated WebM track settings")
    refuses(B.ebml_header() + B.el(B.TRACKS, b""), "invalid WebM: expected Segment, got 0x1654AE6B")
    matroska = B.webm([AAC], [B.cluster(0, [B.simple_block(1, 0, FRAME)])], header=B.ebml_header(doc_type=b"matroska", doc_read_version=4))
    assert M.demux(matroska)[1] is None and len(demux_in_pieces(matroska, 7)) == 2


def test_refusals_from_the_tracks():
    block = B.simple_block(1, 0, FRAME)
    refuses(one_block([], block), "WebM source has no supported media track")
    refuses(one_block([B.track(1, b"A_PCM/INT/LIT")], block), "WebM source has no supported media track")
    refuses(one_block([B.track(1, b"V_VP9", kind=1)], block), "WebM source has no supported audio track")
    refuses(B.webm([AAC], []), "WebM source has no supported audio track")  # no Cluster: the configurations were never handed out
    refuses(B.webm([AAC], [], timecode_scale=0), "WebM TimecodeScale must be positive")
    refuses(B.webm([B.track(1, b"A_AAC", scale=0.0)], []), "WebM TrackTimestampScale must be finite and positive")
    refuses(B.webm([B.track(1, b"A_AAC", extra=B.el(0x23314F, struct.pack(">f", float("inf"))))], []), "WebM TrackTimestampScale must be finite and positive")
    refuses(B.webm([B.track(1, b"A_AAC", extra=B.el(0x23314F, bytes(3)))], []), "WebM TrackTimestampScale must be finite and positive")
    refuses(B.webm([B.track(1, b"A_AAC", extra=B.el(0xEC, b"", size=100))], []), "truncated WebM TrackEntry")
    refuses(B.webm([B.track(1, b"A_AAC", extra=B.el(0xE1, B.el(0x9F, b"", size=9)))], []), "truncated WebM track settings")


def test_refusals_from_the_content_encodings():
    case = lambda enc: B.webm([B.track(1, b"A_AAC", encodings=enc)], [])  # noqa: E731
    one = B.el(0x6240, B.el(0x5034, B.uint(0x4254, 3) + B.el(0x4255, b"ab")))
    refuses(case(B.header_stripping(b"ab", algo=0)), "unsupported Matroska ContentCompAlgo 0; only header stripping is supported")
    refuses(case(B.header_stripping(b"ab", algo=1)), "unsupported Matroska ContentCompAlgo 1; only header stripping is supported")
    refuses(case(B.header_stripping(b"ab", enc_type=1)), "encrypted Matroska ContentEncoding is unsupported")
    refuses(case(B.header_stripping(b"ab", scope=2)), "Matroska ContentEncoding does not apply to frame data")
    refuses(case(B.header_stripping(b"ab", settings=False)), "Matroska header stripping has no prefix bytes")
    refuses(case(B.el(0x6D80, B.el(0x6240, B.uint(0x5031, 0)))), "Matroska ContentEncoding has no compression settings")
    refuses(case(B.el(0x6D80, one + one)), "multiple Matroska ContentEncodings are unsupported")
    refuses(case(B.el(0x6D80, B.el(0xEC, bytes(3)))), "empty Matroska ContentEncodings is unsupported")
    refuses(case(B.el(0x6D80, b"\x00\x00\x00")), "invalid WebM ContentEncodings element")
    refuses(case(B.el(0x6D80, b"\x62\x40\x00")), "truncated WebM ContentEncodings size")
    refuses(case(B.el(0x6D80, B.el(0x6240, b"", size=7))), "truncated WebM ContentEncoding")
    refuses(case(B.el(0x6D80, B.el(0x6240, B.el(0x5034, b"", size=3)))), "truncated WebM track settings")


def test_refusals_from_the_blocks():
    bare = B.track(1, b"A_AAC", private=b"\x14\x08")
    raw = lambda body, tracks=(AAC,): one_block(list(tracks), B.el(B.SIMPLE_BLOCK, body))  # noqa: E731
    refuses(raw(b"\x00\x00\x00\x00\x00"), "invalid WebM block track number")
    refuses(raw(b""), "invalid WebM block track number")
    refuses(raw(b"\x81\x00\x00"), "truncated WebM block header")
    refuses(raw(b"\x81\x00\x00\x82"), "Truncated Xiph-laced block")
    refuses(raw(b"\x81\x00\x00\x84"), "Truncated fixed-laced block")
    refuses(raw(b"\x81\x00\x00\x86"), "Truncated EBML-laced block")
    refuses(raw(b"\x81\x00\x00\x82\x01\xff"), "Truncated Xiph lacing size")
    refuses(raw(b"\x81\x00\x00\x82\x01\x09abc"), "Xiph-laced frame sizes exceed block payload")
    refuses(raw(b"\x81\x00\x00\x84\x02abcd"), "Invalid fixed-laced block size")
    refuses(raw(b"\x81\x00\x00\x86\x02"), "Truncated EBML-laced first frame size")
    refuses(raw(b"\x81\x00\x00\x86\x02\x81"), "Truncated EBML-laced frame size delta")
    refuses(raw(b"\x81\x00\x00\x86\x02\x81\x80abc"), "Negative EBML-laced frame size")  # 1, then 1 - 63
    refuses(raw(b"\x81\x00\x00\x86\x01\x89abc"), "EBML-laced frame sizes exceed block payload")
    refuses(raw(b"\x81\x00\x00\x82\x01\x01abc", (bare,)), "laced WebM A_AAC timing cannot be resolved deterministically")
    refuses(one_block([B.track(1, b"A_OPUS")], B.simple_block(1, 0, [b"\x08a", b"\x0b\x3fz"], "xiph")),
            "laced WebM A_OPUS timing cannot be resolved deterministically")  # 63 frames of 20 ms are no Opus packet
    group = lambda body: one_block([AAC], B.el(B.BLOCK_GROUP, body))  # noqa: E731
    refuses(group(B.el(B.BLOCK, b"", size=9)), "truncated WebM BlockGroup")
    refuses(group(B.el(B.DISCARD_PADDING, b"")), "invalid WebM signed integer size")
    refuses(group(B.el(B.DISCARD_PADDING, bytes(9))), "invalid WebM signed integer size")
    far = B.webm([AAC], [B.el(B.CLUSTER, B.uint(B.TIMECODE, 1 << 63, 8))])
    refuses(far, "WebM cluster timecode exceeds i64")
    late = B.webm([AAC], [B.cluster((1 << 63) - 1, [B.simple_block(1, 1, FRAME)])])
    refuses(late, "WebM block timestamp overflow")
    refuses(B.webm([AAC], [B.cluster(1 << 62, [B.simple_block(1, 0, FRAME)])]), "WebM nanosecond timestamp overflow")
    refuses(one_block([B.track(1, b"A_AAC", codec_delay=1 << 63)], B.simple_block(1, 0, FRAME)), "WebM CodecDelay exceeds the signed timeline range")
    refuses(B.webm([B.track(1, b"A_AAC", codec_delay=(1 << 63) - 1)], [B.cluster(0, [B.simple_block(1, -2, FRAME)])], timecode_scale=1),
            "WebM CodecDelay timestamp underflow")
    refuses(one_block([AAC], B.block_group(1, 0, FRAME, duration=(1 << 64) - 1)), "WebM BlockDuration overflow")


def test_blocks_of_unreported_tracks_are_dropped_before_their_lacing_is_read():
    data = B.webm([AAC], [B.cluster(0, [B.el(B.SIMPLE_BLOCK, b"\x85\x00\x00\x86"), B.simple_block(1, 0, FRAME)])])
    events = demux_in_pieces(data, 7)
    assert as_model(events) == M.demux(data)[0] and len(events) == 2


def test_vorbis_codec_private_refusals():
    for private, text in ((b"", "Missing Vorbis CodecPrivate"), (b"\x01\x01ab", "Expected 3 Vorbis headers in CodecPrivate, got 2"),
                          (b"\xff", "Expected 3 Vorbis headers in CodecPrivate, got 256"), (b"\x02\xff", "Truncated Xiph lacing size"),
                          (b"\x02\x01", "Truncated Xiph lacing size"), (b"\x02\x02\x02abc", "Vorbis CodecPrivate header sizes exceed payload")):
        refused(lambda: webm.vorbis_headers(private), text)
    assert webm.vorbis_headers(b"\x02\x01\xff\x01a" + bytes(256) + b"xyz") == [b"a", bytes(256), b"xyz"]
    assert webm.vorbis_headers(b"\x02\x00\x00") == [b"", b"", b""]


# ---- budgets ---------------------------------------------------------------------------------------------------------------------------

def test_budgets_hold_from_the_headers():
    d = webm.WebmAudioDemuxer()
    refused(lambda: d.add(bytes(4 * 1024 * 1024 + 1)), "WebM input chunk exceeds the 4194304 byte streaming budget")
    refused(lambda: d.add(b"\x1a"), "WebM input chunk exceeds the 4194304 byte streaming budget")  # it stays refused
    d.close()
    head = B.ebml_header() + B.el(B.SEGMENT, b"", size=B.UNKNOWN)
    big_tags = head + B.eid(B.TAGS) + B.vint(16 * 1024 * 1024 + 1)
    refuses(big_tags, "WebM element 0x1254C367 exceeds the 16777216 byte budget")
    at_budget = head + B.eid(B.TAGS) + B.vint(16 * 1024 * 1024)
    refuses(at_budget, "truncated WebM element: %d buffered bytes remain" % 8)
    in_cluster = head + B.el(B.TRACKS, AAC) + B.el(B.CLUSTER, b"", size=B.UNKNOWN)
    refuses(in_cluster + B.eid(B.SIMPLE_BLOCK) + B.vint(64 * 1024 * 1024 + 1), "WebM element 0xA3 exceeds the 67108864 byte budget")
    refuses(in_cluster + B.eid(B.BLOCK_GROUP) + B.vint(64 * 1024 * 1024 + 1), "WebM element 0xA0 exceeds the 67108864 byte budget")
    refuses(in_cluster + B.eid(B.CUES) + B.vint(16 * 1024 * 1024 + 1), "WebM element 0x1C53BB6B exceeds the 16777216 byte budget")
    refuses(B.eid(B.EBML) + B.vint(16 * 1024 * 1024 + 1), "WebM element 0x1A45DFA3 exceeds the 16777216 byte budget")
    # an unknown size is a number anywhere but at Segment and Cluster
    refuses(head + B.el(B.TRACKS, B.el(B.TRACK_ENTRY, b"", size=B.UNKNOWN)), "WebM element 0xAE exceeds the 16777216 byte budget")
    refuses(head + B.el(B.INFO, b"", size=B.UNKNOWN), "WebM element 0x1549A966 exceeds the 16777216 byte budget")
    refuses(in_cluster + B.el(B.BLOCK_GROUP, b"", size=B.UNKNOWN), "WebM element 0xA0 exceeds the 67108864 byte budget")


def test_finish_inside_an_element():
    whole = FILES["lacing_xiph"]
    cut = whole[:-5]
    events, error = M.demux(cut)
    assert error.startswith("truncated WebM element: ") and error.endswith(" buffered bytes remain")
    for piece in (len(cut), 7):
        e = refused(lambda: demux_in_pieces(cut, piece), error)
        assert as_model(e.events) == events and len(events) == 2  # the config and the first block
    refuses(whole[:3], "truncated WebM element: 3 buffered bytes remain")
    refuses(whole[:20], "truncated WebM element: 20 buffered bytes remain")  # inside the EBML header: nothing was consumed
    refuses(b"", "WebM source has no supported audio track")


# ---- discard padding -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("padding, rate, decoded, want", [
    (None, 8000, 256, (0, 0)), (0, 8000, 256, (0, 0)), (16000000, 8000, 256, (0, 128)), (16000001, 8000, 256, (0, 129)), (15999999, 8000, 256, (0, 128)),
    (1, 48000, 960, (0, 1)), (13500000, 48000, 960, (0, 648)), (-16000000, 8000, 256, (128, 0)), (-16000001, 8000, 256, (129, 0)), (-1, 44100, 1024, (1, 0)),
    (10 ** 9, 8000, 256, (0, 256)), (-10 ** 9, 8000, 256, (256, 0)), (32000000, 8000, 256, (0, 256)), (32000001, 8000, 256, (0, 256)), (5, 8000, 0, (0, 0)),
    (125000, 8000, 256, (0, 1)), (125001, 8000, 256, (0, 2)), ((1 << 63) - 1, 1, 7, (0, 7)), (-(1 << 63), 1, 7, (7, 0))])
def test_discard_frames(padding, rate, decoded, want):
    assert webm.discard_frames(padding, rate, decoded) == want


def test_discard_frames_overflow():
    refused(lambda: webm.discard_frames((1 << 63) - 1, 48000, 10), "WebM discard-padding conversion overflow")
    refused(lambda: webm.discard_frames(-(1 << 63), 2, 10), "WebM discard-padding conversion overflow")


# ---- the decoder's refusals that need no device ------------------------------------------------------------------------------------------

def test_decoder_refusals():
    block = B.simple_block(1, 0, FRAME)

    def decode(data):
        d = webm.WebmDecoder()
        try:
            d.add(data)
            d.finish()
        finally:
            d.close()

    refused(lambda: decode(CASES.fixture("opus")), "unsupported or disabled WebM codec: A_OPUS")
    refused(lambda: decode(one_block([B.track(1, b"A_ALAC", private=bytes(24))], block)), "unsupported or disabled WebM codec: A_ALAC")
    refused(lambda: decode(FILES["two_audio_and_video"]), "WebM decoder received more than one audio configuration")
    refused(lambda: decode(one_block([B.track(1, b"A_VORBIS")], block)), "Missing Vorbis CodecPrivate")
    refused(lambda: decode(one_block([B.track(1, b"A_AAC")], block)), "WebM A_AAC CodecPrivate holds no AudioSpecificConfig with a rate of the table")
    refused(lambda: decode(one_block([B.track(1, b"A_AAC", private=b"\x17\x88")], block)),
            "WebM A_AAC CodecPrivate holds no AudioSpecificConfig with a rate of the table")  # index 15: a rate written out
    refused(lambda: decode(one_block([B.track(1, b"A_FLAC")], block)), "WebM A_FLAC CodecPrivate holds no fLaC marker and STREAMINFO block")
    refused(lambda: decode(one_block([B.track(1, b"A_FLAC", private=b"fLaC" + bytes(30))], block)),
            "WebM A_FLAC CodecPrivate holds no fLaC marker and STREAMINFO block")
    refused(lambda: decode(one_block([B.track(1, b"A_VORBIS", private=b"\x01ab")], block)), "Expected 3 Vorbis headers in CodecPrivate, got 2")


# ---- fuzz and ABI ----------------------------------------------------------------------------------------------------------------------

def test_mutated_files_under_sanitizers(tmp_path):
    """tests/fuzz_webm.cpp: csrc/webm_stream.h alone with AddressSanitizer + UBSan on the CPU -- seeded mutations of the fixtures and the
    builder's files through the demuxer, whole and in pieces"""
    exe = str(tmp_path / "fuzz_webm")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "fuzz_webm.cpp")], cwd=HERE)
    paths = []
    for name, data in sorted(FILES.items()):
        paths.append(str(tmp_path / (name + ".bin")))
        with open(paths[-1], "wb") as f:
            f.write(data)
    out = subprocess.run([exe, "150"] + paths, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "fuzz_webm ok" in out.stdout


def test_the_abi_exports_the_new_symbols():
    for name in ("sk_webm_demuxer_create", "sk_webm_demuxer_destroy", "sk_webm_demuxer_add", "sk_webm_demuxer_finish", "sk_webm_demuxer_last_error",
                 "sk_webm_demuxer_n_tracks", "sk_webm_demuxer_config", "sk_webm_demuxer_pending", "sk_webm_demuxer_take", "sk_webm_vorbis_headers",
                 "sk_webm_discard_frames"):
        assert hasattr(lib, name), name
    assert lib.sk_strerror(webm.ERR_STREAM).decode() == "WebM stream rejected"


def test_the_rewrapped_fixtures_hold_the_packets_they_were_made_from():
    """what the GPU tests decode: the Ogg Vorbis, ADTS and native FLAC fixtures as WebM files"""
    data, headers, packets = CASES.wrapped_ogg({1: -16000000, 93: 16000000})
    events = demux_in_pieces(data, 641)
    assert as_model(events) == M.demux(data)[0]
    assert webm.vorbis_headers(events[0].codec_private) == headers and [e.data for e in events[1:]] == packets and len(packets) == 94
    assert [(k, e.discard_padding_ns) for k, e in enumerate(events[1:]) if e.discard_padding_ns is not None] == [(1, -16000000), (93, 16000000)]
    data, adts = CASES.wrapped_aac()
    events = demux_in_pieces(data, 641)
    assert events[0].codec_private == b"\x14\x08" and len(events) == 49  # AAC-LC, 16 kHz, mono
    from soundkit_amd import mp4
    assert b"".join(mp4.adts_header(b"\x14\x08", 16000, 1, len(e.data)) + e.data for e in events[1:]) == adts
    data, flac = CASES.wrapped_flac()
    events = demux_in_pieces(data, 641)
    assert events[0].codec_private[:4] == b"fLaC" and len(events) == 43
    assert events[0].codec_private + b"".join(e.data for e in events[1:]) == flac

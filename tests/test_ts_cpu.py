"""The MPEG-TS demuxer on the host (csrc/ts_stream.h through soundkit_amd.ts): its events against tests/ts_model.py on the four fixtures
and on the streams tests/ts_builder.py writes, whole and in pieces of 1, 188, 4096 and 65 536 bytes; the fixtures' elementary streams
against the golden files; every refusal with its text; the budgets; the sniff test at its edges; and a sanitizer fuzz
(tests/fuzz_ts.cpp).  No GPU."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import ts_builder as B
import ts_cases as CASES
import ts_model as M
from soundkit_amd import SoundkitError, lib, ts

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = dict({name: CASES.fixture(name) for name in CASES.FIXTURES}, **CASES.builder_cases())
ADTS = CASES.adts_frames(CASES.ADTS)


def demux_in_pieces(data, piece):
    """-> the events through TsAudioDemuxer; a refusal raises with .events = what came before it"""
    d, events = ts.TsAudioDemuxer(), []
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
        if isinstance(e, ts.TsAudioConfig):
            out.append(("config", dict(codec=e.codec, format=e.packet_format, stream_type=e.stream_type, pid=e.pid, program=e.program_number, stride=e.packet_stride,
                                       prefix=e.packet_prefix, rate=e.sample_rate, channels=e.channels, bits=e.bits_per_sample, bytes_per_frame=e.bytes_per_frame,
                                       frames_per_packet=e.frames_per_packet, header=e.lpcm_header)))
        else:
            out.append(("packet", dict(data=e.data, pts=e.pts, dts=e.dts, duration=e.duration, cc=e.continuity_counter, discontinuity=e.discontinuity)))
    return out


def refused(fn, text):
    with pytest.raises(SoundkitError) as e:
        fn()
    assert str(e.value).endswith(": " + text), str(e.value)
    return e.value


def refuses(data, text, piece=None, packets=None):
    """the demuxer and the model refuse `data` with `text`, after the same events"""
    events, error = M.demux(data)
    assert error == text, error
    e = refused(lambda: demux_in_pieces(data, piece or max(len(data), 1)), text)
    assert as_model(e.events) == events
    if packets is not None:
        assert sum(kind == "packet" for kind, _ in events) == packets
    if piece is None:
        refuses(data, text, 777, packets)


def packets_of(events):
    return [e for kind, e in events if kind == "packet"]


def config_of(events):
    configs = [e for kind, e in events if kind == "config"]
    assert len(configs) == 1 and events[0][0] == "config"
    return configs[0]


# ---- events against the model, however the bytes are cut -------------------------------------------------------------------------------

@pytest.mark.parametrize("piece", [0, 1, 188, 4096, 65536])
@pytest.mark.parametrize("name", sorted(FILES))
def test_demuxer_matches_model_however_it_is_cut(name, piece):
    data = FILES[name]
    events, error = M.demux(data)
    assert error is None and len(packets_of(events)) > 0
    assert as_model(demux_in_pieces(data, piece or len(data))) == events


@pytest.mark.parametrize("name", sorted(CASES.FIXTURES))
def test_fixtures_hold_their_elementary_streams(name):
    events, error = M.demux(CASES.fixture(name))
    config, packets = config_of(events), packets_of(events)
    assert error is None and len(packets) == CASES.PACKETS[name]
    m2ts = name.endswith(".m2ts")
    assert (config["pid"], config["program"], config["stride"], config["prefix"]) == (0x1100 if m2ts else 0x100, 1, 192 if m2ts else 188, 4 if m2ts else 0)
    assert (config["rate"], config["channels"]) == (48000, 2)
    stream = b"".join(p["data"] for p in packets)
    if name.startswith("aac"):
        assert (config["codec"], config["format"], config["stream_type"]) == ("aac", "adts", 0x06 if m2ts else 0x0f)  # FFmpeg's M2TS mode: private PES in an HDMV program
        assert stream == CASES.ADTS and len(stream) == 16568 and {p["duration"] for p in packets} == {1920}
        assert [p["pts"] - packets[0]["pts"] for p in packets[:9]] == [1920 * k for k in range(9)] and all(p["dts"] == p["pts"] for p in packets)
    elif name.startswith("mp2"):
        assert (config["codec"], config["format"], config["stream_type"]) == ("mp2", "raw", 0x03)
        assert stream == CASES.MP2 and len(stream) == 24192 and {p["duration"] for p in packets} == {2160} and len({p["pts"] for p in packets}) == 42
    else:
        assert (config["codec"], config["stream_type"], config["bits"], config["bytes_per_frame"], config["frames_per_packet"]) == ("pcm", 0x80, 16, 4, 240)
        assert config["header"] == bytes([0x03, 0xC0, 0x31, 0x40]) and {len(p["data"]) for p in packets} == {960} and {p["duration"] for p in packets} == {450}
        assert hashlib.sha256(np.frombuffer(stream, ">i2").astype("<i2").tobytes()).hexdigest() == CASES.LPCM_SHA256


def test_built_cases_hold_what_they_are_named_for():
    events = {name: M.demux(FILES[name])[0] for name in FILES}
    for stride, prefix in ((188, 0), (192, 4), (204, 0)):
        config, packets = config_of(events["adts_%d" % stride]), packets_of(events["adts_%d" % stride])
        assert (config["stride"], config["prefix"]) == (stride, prefix) and [p["data"] for p in packets] == ADTS[:18]
        assert [p["pts"] for p in packets[:6]] == [90000, 91920, 93840, 95760, 91920, 93840]  # a PES every 1920 ticks, a frame every 1920
    assert config_of(events["layer3"])["codec"] == "mp3" and config_of(events["layer3"])["rate"] == 16000
    assert b"".join(p["data"] for p in packets_of(events["layer3"])) == b"".join(CASES.layer3_frames()) and len(packets_of(events["layer3"])) == 40
    assert {p["duration"] for p in packets_of(events["layer3"])} == {3240}  # 576 samples at 16 kHz
    assert config_of(events["layer1"])["codec"] == "mp1" and {len(p["data"]) for p in packets_of(events["layer1"])} == {256}
    assert {p["duration"] for p in packets_of(events["layer1"])} == {720} and len(packets_of(events["layer1"])) == 24
    c = config_of(events["lpcm_24_96k"])
    assert (c["rate"], c["bits"], c["bytes_per_frame"], c["frames_per_packet"], c["header"][2:]) == (96000, 24, 6, 160, b"\x34\xc0")
    assert {p["duration"] for p in packets_of(events["lpcm_24_96k"])} == {150}
    assert (config_of(events["hdmv_private_aac"])["codec"], config_of(events["hdmv_private_aac"])["stream_type"]) == ("aac", 6)
    for name in ("ac3", "ac3_by_descriptor", "ac3_by_registration"):
        c = config_of(events[name])
        assert (c["codec"], c["format"], c["rate"], c["channels"]) == ("ac3", "raw", None, None) and packets_of(events[name])[0]["duration"] is None
    assert config_of(events["dts"])["codec"] == "dts" and len(packets_of(events["dts"])) == 4
    assert (config_of(events["latm"])["codec"], config_of(events["latm"])["format"]) == ("aac", "latm")
    assert [len(p["data"]) for p in packets_of(events["latm"])] == [103, 10, 303]
    two = events["two_programs"]
    assert (config_of(two)["program"], config_of(two)["pid"]) == (2, 0x201) and [p["data"] for p in packets_of(two)] == ADTS[:12]
    moved = packets_of(events["version_change"])
    assert [p["data"] for p in moved] == ADTS[:17] and config_of(events["version_change"])["pid"] == 0x100
    assert [p["pts"] for p in moved[7:10]] == [90000 + 7680 + 3 * 1920, 200000, 300000]
    gap = packets_of(events["duplicate_and_gap"])
    assert [p["data"] for p in gap] == ADTS[:6] + ADTS[9:15]  # the duplicate changes nothing, the PES in front of the gap goes
    assert [k for k, p in enumerate(gap) if p["discontinuity"]] == [6]
    assert events["leading_garbage"] == events["adts_188"] and len(packets_of(events["garbage_in_the_middle"])) == 18
    wrap = packets_of(events["pts_wrap"])
    assert [p["pts"] for p in wrap[::2]] == [(1 << 33) - 3 * 3840 + 3840 * k for k in range(6)] and wrap[-1]["pts"] > 1 << 33
    split = packets_of(events["split_sections_dts_and_flags"])
    assert [p["data"] for p in split] == ADTS[:6] and [p["pts"] - p["dts"] for p in split] == [100] * 6
    assert [p["discontinuity"] for p in split] == [False, False, True, False, False, False]
    loose = packets_of(events["no_timestamps_and_partial_tails"])
    assert [p["data"] for p in loose] == ADTS[:4] + [ADTS[5]] and [p["pts"] for p in loose] == [None, None, None, 1234, 99]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def audio(payload, stream_type=0x0f, tail=(), **more):
    """one PES with `payload` on the audio PID, then the PES that makes the demuxer look at it"""
    def make(m):
        m.pes(0x100, B.pes(b"".join(ADTS[:2]), 1000)).pes(0x100, payload if more.get("raw") else B.pes(payload, 2000))
        for p in tail:
            m.raw(p)
    return CASES.with_packets(make, stream_type, **{k: v for k, v in more.items() if k != "raw"})


def test_refusals_from_the_packets():
    one = lambda **kw: CASES.with_packets(lambda m: m.pes(0x100, B.pes(ADTS[0], 1)).raw(B.packet(0x100, 1, bytes(184), **kw)))  # noqa: E731
    refuses(one(error=True), "MPEG-TS packet has the transport-error indicator")
    refuses(one(scrambling=2), "scrambled MPEG-TS packets are unsupported")
    refuses(one(afc=0), "MPEG-TS packet has reserved adaptation-field control")
    long_field = bytes([0x47, 0x01, 0x00, 0x31, 184]) + bytes(183)
    refuses(CASES.with_packets(lambda m: m.raw(long_field)), "MPEG-TS adaptation field exceeds its packet")
    exact = bytes([0x47, 0x01, 0x00, 0x31, 183]) + bytes(183)  # a field that fills the packet: no payload, nothing refused
    assert M.demux(CASES.with_packets(lambda m: m.raw(exact)))[1] is None


def test_refusals_from_the_sections():
    def psi(payload, pid=0, start=True, before=None):
        def make(m):
            if before is not None:
                m.raw(before)
                m.cc[pid] = before[3] & 15
            m.raw(B.packet(pid, m.next_cc(pid), payload + b"\xff" * (184 - len(payload)), start=start))
        return CASES.with_packets(make)

    refuses(psi(bytes([184])), "PSI pointer exceeds payload")
    refuses(psi(b"\x00\x00\xb0\x00"), "PSI section size 3 is out of range")
    refuses(psi(b"\x00\x00\xbf\xff"), "PSI section size 4098 is out of range")
    refuses(psi(b"\x00\x00\xb3\xfe"), "PSI section size 1025 is out of range")
    started = B.packet(0, 1, b"\x00" + B.pat([(1, 0x1000)] * 60)[:183], start=True)
    refuses(psi(b"\x02\x00\x00" + B.pat([(1, 0x1000)]), before=started), "PSI pointer starts a new section before the previous section ends")
    refuses(psi(b"\x00" + B.pat([(1, 0x1000)], version=3, crc=0x12345678)), "MPEG-TS PSI CRC mismatch")
    refuses(psi(b"\x00" + B.pmt(1, [(0x0f, 0x100, b"")], version=2, crc=1), pid=0x1000), "MPEG-TS PSI CRC mismatch")
    over = bytearray(B.pmt(1, [(0x0f, 0x100, b"")], version=2)[:-4])
    over[10:12] = b"\xf0\x09"  # program_info_length beyond the section
    refuses(psi(b"\x00" + bytes(over) + M.crc32_mpeg2(bytes(over)).to_bytes(4, "big"), pid=0x1000), "MPEG-TS PMT program descriptors exceed their section")
    over = bytearray(B.pmt(1, [(0x1b, 0x101, b"")], version=2)[:-4])
    over[15:17] = b"\xf0\x01"  # ES_info_length beyond the section
    refuses(psi(b"\x00" + bytes(over) + M.crc32_mpeg2(bytes(over)).to_bytes(4, "big"), pid=0x1000), "MPEG-TS PMT descriptor exceeds its section")


def test_refusals_from_the_pes():
    raw = lambda data: audio(data, raw=True)  # noqa: E731
    refuses(raw(b"\x00\x00\x02" + bytes(20)), "invalid MPEG-TS PES header", packets=2)
    refuses(raw(b"\x00\x00\x01\xc0\x00"), "invalid MPEG-TS PES header", packets=2)
    refuses(raw(b"\x00\x00\x01\xc0\x00\x00\x80\x00\x09" + bytes(5)), "MPEG-TS PES optional header is truncated", packets=2)
    refuses(raw(b"\x00\x00\x01\xc0\x00\x00\x80\x80\x05" + b"\x20" + bytes(4) + ADTS[0]), "invalid or truncated MPEG-TS PES timestamp", packets=2)
    refuses(raw(b"\x00\x00\x01\xc0\x00\x00\x80\x80\x00\x21"), "invalid or truncated MPEG-TS PES timestamp", packets=2)
    refuses(raw(b"\x00\x00\x01\xc0\x00\x00\x80\xc0\x05" + B.stamp(3, 5) + b"\x11\x00"), "invalid or truncated MPEG-TS PES timestamp", packets=2)
    refuses(raw(b"\x00\x00\x01\xc0\x00\x04\x80\x00\x05" + bytes(30)), "MPEG-TS PES length ends inside its header", packets=2)
    # a gap inside a PES: what is left of it has no header
    def torn(m):
        m.pes(0x100, B.pes(b"".join(ADTS[:4]), 1000))
        del m.packets[-3]
        m.pes(0x100, B.pes(ADTS[4], 2000))
    refuses(CASES.with_packets(torn), "invalid MPEG-TS PES header", packets=0)


def test_refusals_from_the_emitters():
    mp2 = CASES.mpa_frames(CASES.MP2, 3)
    first = lambda payload, stream_type, **pmt: CASES.with_packets(lambda m: m.pes(0x100, B.pes(payload, 1)), stream_type, **pmt)  # noqa: E731
    refuses(first(mp2[0] + mp2[1][:100], 0x03), "MPEG audio frame is truncated at the PES boundary", packets=1)
    refuses(first(mp2[0] + b"\xff\xff\x00", 0x04), "MPEG audio PES ends with an incomplete frame", packets=1)
    assert M.demux(first(mp2[0] + b"\xff\xff\xff", 0x03))[1] is None  # FF to the end is stuffing
    refuses(first(CASES.loas(40) + CASES.loas(50)[:20], 0x11), "LOAS/LATM access unit is truncated at the PES boundary", packets=1)
    refuses(first(CASES.loas(40) + b"\x01", 0x11), "LOAS/LATM PES ends with an incomplete access unit", packets=1)


def test_bluray_lpcm_refusals_are_this_projects_own():
    first = lambda payload: CASES.with_packets(lambda m: m.pes(0x100, B.pes(CASES.lpcm_unit(8), 1)).pes(0x100, B.pes(payload, 2)), 0x80)  # noqa: E731
    refuses(first(b"\x00\x00\x31"), "Blu-ray LPCM access unit of 3 bytes is shorter than its 4-byte header", packets=1)
    refuses(first(CASES.lpcm_unit(8, size=30)), "Blu-ray LPCM size field 30 disagrees with the 32 payload bytes", packets=1)
    refuses(first(CASES.lpcm_unit(8, rate_code=2)), "unsupported Blu-ray LPCM rate code 2", packets=1)
    refuses(first(CASES.lpcm_unit(8)[:3] + b"\x00" + CASES.lpcm_unit(8)[4:]), "unsupported Blu-ray LPCM depth code 0", packets=1)
    refuses(first(CASES.lpcm_unit(8, assignment=1)), "mono Blu-ray LPCM (channel assignment 1, with its pad channel) is not built", packets=1)
    refuses(first(CASES.lpcm_unit(8, assignment=9)), "Blu-ray LPCM channel assignment 9 is not built: stereo alone is", packets=1)
    refuses(first(CASES.lpcm_unit(8, 20)), "20-bit Blu-ray LPCM is not built", packets=1)
    refuses(first(CASES.lpcm_unit(8, 24)[:2] + CASES.lpcm_unit(7, 24)[2:] + b"\x00\x00"), "Blu-ray LPCM size field 48 disagrees with the 44 payload bytes", packets=1)
    odd = bytes([0, 46, 0x31, 0xc0]) + bytes(46)
    refuses(first(odd), "Blu-ray LPCM payload of 46 bytes is no whole number of 6-byte frames", packets=1)


# ---- budgets, sniffing, streams without audio ----------------------------------------------------------------------------------------------

def test_budgets():
    d = ts.TsAudioDemuxer()
    refused(lambda: d.add(bytes(4 * 1024 * 1024 + 1)), "MPEG-TS input chunk exceeds the 4194304 byte streaming budget")
    refused(lambda: d.add(b"\x47"), "MPEG-TS input chunk exceeds the 4194304 byte streaming budget")  # it stays refused
    d.close()
    assert M.demux(bytes(4 * 1024 * 1024 + 1))[1] == "MPEG-TS input chunk exceeds the 4194304 byte streaming budget"
    fits = CASES.with_packets(lambda m: m.pes(0x100, b"\x00\x00\x01\xc0\x00\x00\x80\x00\x00" + bytes(1024 * 1024 - 9)), 0x81)
    events, error = M.demux(fits)
    assert error is None and len(events[1][1]["data"]) == 1024 * 1024 - 9
    assert as_model(demux_in_pieces(fits, 1 << 20)) == events
    over = CASES.with_packets(lambda m: m.pes(0x100, b"\x00\x00\x01\xc0\x00\x00\x80\x00\x00" + bytes(1024 * 1024 - 8)), 0x81)
    refuses(over, "MPEG-TS PES exceeds the 1048576 byte packet budget", piece=1 << 20, packets=0)


def test_streams_without_an_audio_track_hand_out_nothing():
    video_only = CASES.with_packets(lambda m: m.pes(0x100, B.pes(bytes(500), 1, 1, 0xe0)), 0x1b)
    for data in (video_only, b"", bytes(5000), FILES["adts_188"][:4 * 188]):
        assert M.demux(data) == ([], None) and demux_in_pieces(data, 333) == []
    d = ts.TsAudioDemuxer()
    assert d.add(FILES["aac.ts"][:940]) == [] and d.config is None and 0 < d.buffered_bytes() <= 3 * 184  # only the PES's first packets are kept
    d.close()


@pytest.mark.parametrize("n, stride, want", [(376, 188, False), (377, 188, True), (388, 192, False), (389, 192, True)])
def test_sniff_at_its_edges(n, stride, want):
    data = FILES["adts_%d" % stride][:n]
    assert ts.sniff(data) is want and M.sniff(data) is want


def test_sniff_leaves_the_other_formats_alone():
    wav = CASES.golden("wav_stereo_A_Tusk.wav")
    mp3 = CASES.golden("mp3", "stereo16k_A_Tusk_encoded.mp3")
    for data in (wav, CASES.ADTS, mp3, CASES.MP2, b"", b"\x47", b"\x47" * 376):
        assert not ts.sniff(data[:4096]) and not M.sniff(data[:4096])
    assert ts.sniff(b"\x47" * 377)
    for name in CASES.FIXTURES:
        assert ts.sniff(CASES.fixture(name)) and not ts.sniff(CASES.fixture(name)[100:])  # a join in mid-segment is spawn_mpeg_ts's


def test_decode_file_refusals_that_need_no_device():
    for name, codec in (("dts", "dts"), ("ac3", "ac3"), ("latm", "aac")):
        refused(lambda: ts.decode_file(FILES[name]), "Invalid input format: unsupported MPEG-TS audio codec " + codec)
    refused(lambda: ts.decode_file(bytes(3000)), "Invalid input format: MPEG-TS has no supported audio track")
    scrambled = CASES.with_packets(lambda m: m.raw(B.packet(0x100, 0, bytes(184), scrambling=1)))
    refused(lambda: ts.decode_file(scrambled), "Invalid input format: scrambled MPEG-TS packets are unsupported")


# ---- fuzz and ABI ----------------------------------------------------------------------------------------------------------------------

def test_mutated_streams_under_sanitizers(tmp_path):
    """tests/fuzz_ts.cpp: csrc/ts_stream.h alone with AddressSanitizer + UBSan on the CPU -- seeded mutations of the fixtures and the
    builder's streams through the demuxer, whole and in pieces"""
    exe = str(tmp_path / "fuzz_ts")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "fuzz_ts.cpp")], cwd=HERE)
    paths = []
    for name, data in sorted(FILES.items()):
        paths.append(str(tmp_path / (name + ".bin")))
        with open(paths[-1], "wb") as f:
            f.write(data)
    out = subprocess.run([exe, "150"] + paths, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "fuzz_ts ok" in out.stdout


def test_the_abi_exports_the_new_symbols():
    for name in ("sk_ts_demuxer_create", "sk_ts_demuxer_destroy", "sk_ts_demuxer_add", "sk_ts_demuxer_finish", "sk_ts_demuxer_last_error",
                 "sk_ts_demuxer_config", "sk_ts_demuxer_pending", "sk_ts_demuxer_take", "sk_ts_sniff", "sk_pipeline_spawn_mpeg_ts"):
        assert hasattr(lib, name), name
    assert lib.sk_strerror(ts.ERR_STREAM).decode() == "MPEG-TS stream rejected"

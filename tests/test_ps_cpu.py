"""The MPEG program stream demuxer on the host (csrc/ps_stream.h through soundkit_amd.ps): its events against tests/ps_model.py on the
streams tests/ps_builder.py writes, whole and in pieces of 1, 7, 188, 4096 and 65 536 bytes; the model's DVD LPCM unpacking against the
known-answer group and the builder's packer; every refusal with its text, from the smallest stream that provokes it; the track choice
in its three modes; the budgets -- the 512 MiB of payload by feeding the same 63 PES packets again and again while the packets are
taken, which needs no file of that size --; and a sanitizer fuzz (tests/fuzz_ps.cpp).  No GPU."""
import os
import subprocess

import pytest

import ps_builder as B
import ps_model as M
from soundkit_amd import SoundkitError, lib, ps

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = B.cases()


def demux_in_pieces(data, piece, mode=ps.TRACK_FIRST):
    """-> the events through PsAudioDemuxer; a refusal raises with .events = what came before it"""
    d, events = ps.PsAudioDemuxer(mode), []
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
    out = []
    for e in events:
        if isinstance(e, ps.PsAudioConfig):
            out.append(("config", dict(kind=e.kind, stream_id=e.stream_id, substream_id=e.substream_id, rate=e.sample_rate, channels=e.channels,
                                       bits=e.bits_per_sample, block_bytes=e.block_bytes)))
        else:
            out.append(("packet", e.data))
    return out


def refused(fn, text):
    with pytest.raises(SoundkitError) as e:
        fn()
    assert str(e.value).endswith(": " + text), str(e.value)
    return e.value


def refuses(data, text, packets=None, mode=ps.TRACK_FIRST):
    """the demuxer and the model refuse `data` with `text`, after the same events, however the bytes are cut"""
    events, error = M.demux(data, mode)
    assert error == text, error
    for piece in (max(len(data), 1), 777, 5):
        e = refused(lambda: demux_in_pieces(data, piece, mode), text)
        assert as_model(e.events) == events
    if packets is not None:
        assert sum(kind == "packet" for kind, _ in events) == packets


def track_of(events):
    return b"".join(e for kind, e in events if kind == "packet")


# ---- DVD LPCM's packing ------------------------------------------------------------------------------------------------------------------

def test_the_known_answer_group():
    """straight from unpack_dvd_lpcm: 00 01 02 ... 0B -> 08 01 00  09 03 02  0A 05 04  0B 07 06"""
    assert M.unpack_dvd_lpcm(bytes(range(12)), 24, 1) == bytes([8, 1, 0, 9, 3, 2, 10, 5, 4, 11, 7, 6])
    assert M.unpack_dvd_lpcm(bytes(range(12)), 24, 2) == M.unpack_dvd_lpcm(bytes(range(12)), 24, 4) == M.unpack_dvd_lpcm(bytes(range(12)), 24, 1)
    assert M.unpack_dvd_lpcm(bytes([1, 2, 3, 4]), 16, 2) == bytes([2, 1, 4, 3])


@pytest.mark.parametrize("channels", [1, 2, 3, 4, 5, 6, 7, 8])
def test_the_model_undoes_the_builders_packer(channels):
    pcm = B.widen(B.A.S16[:2 * 96], channels, 24)
    assert len(pcm) % M.block_size(24, channels) == 0 and M.block_size(24, channels) == B.block_bytes(24, channels)
    assert M.unpack_dvd_lpcm(B.pack24(pcm), 24, channels) == pcm
    pcm = B.widen(B.A.S16[:2 * 96], channels, 16)
    assert M.unpack_dvd_lpcm(B.pack16(pcm), 16, channels) == pcm


def test_partial_blocks_and_20_bits_in_the_model():
    for channels, size in ((1, 12), (2, 12), (4, 12), (8, 24), (3, 36), (6, 72)):
        assert M.block_size(24, channels) == size
        with pytest.raises(M.Refused, match="DVD LPCM ends with a partial 24-bit sample block"):
            M.unpack_dvd_lpcm(bytes(size + 12 if size > 12 else 13), 24, channels)
    with pytest.raises(M.Refused, match="DVD LPCM ends with a partial sample block"):
        M.unpack_dvd_lpcm(bytes(6), 16, 2)
    with pytest.raises(M.Refused, match="20-bit DVD LPCM decoding is not implemented"):
        M.unpack_dvd_lpcm(bytes(10), 20, 2)


# ---- events against the model, however the bytes are cut -------------------------------------------------------------------------------

@pytest.mark.parametrize("piece", [0, 1, 7, 188, 4096, 65536])
@pytest.mark.parametrize("name", sorted(CASES))
def test_demuxer_matches_model_however_it_is_cut(name, piece):
    data = CASES[name][0]
    events, error = M.demux(data)
    assert error is None and events[0][0] == "config" and sum(kind == "config" for kind, _ in events) == 1
    assert as_model(demux_in_pieces(data, piece or len(data))) == events


@pytest.mark.parametrize("name", sorted(CASES))
def test_built_streams_hold_what_they_are_named_for(name):
    data, kind, track, rate, channels, bits, pcm = CASES[name]
    events, error = M.demux(data)
    config = events[0][1]
    assert error is None and ps.sniff(data) and M.looks_like_mpeg_ps(data)
    assert (config["kind"], config["rate"], config["channels"], config["bits"]) == (kind, rate, channels, bits)
    assert track_of(events) == track and len(events) >= 4
    if kind == "pcm-dvd":
        assert config["block_bytes"] == B.block_bytes(bits, channels) and all(len(e) % config["block_bytes"] == 0 for k, e in events if k == "packet")
        assert M.unpack_dvd_lpcm(track, bits, channels) == pcm
    else:
        assert config["stream_id"] == (0xC1 if name.endswith("c1") else 0xC0)


def test_the_structures_the_streams_are_built_for():
    two, one = CASES["lpcm24_6ch"][0], CASES["lpcm16_48k_mono_mpeg1"][0]
    assert two[:5] == b"\x00\x00\x01\xba\x44" and one[:5] == b"\x00\x00\x01\xba\x21"
    for data in (two, one):
        assert b"\x00\x00\x01\xbb" in data and b"\x00\x00\x01\xbe" in data and b"\x00\x00\x01\xe0\x00\x00" in data and data.endswith(b"\x00\x00\x01\xb9")
    assert b"\x00\x00\x01\xbd" in one and b"\xff\xff\x60\x20\x21" in one  # MPEG-1: stuffing, the STD field, a PTS
    # blocks straddle packets: 2011 and 1999 sample bytes a packet, 72 bytes a block -- the carry puts them together again
    sizes = [len(e) for k, e in M.demux(two)[0] if k == "packet"]
    assert sizes[:2] == [2011 // 72 * 72, (2011 % 72 + 1999) // 72 * 72]


# ---- the track choice --------------------------------------------------------------------------------------------------------------------

def test_which_track_is_taken():
    lpcm = B.pes2(0xBD, B.lpcm_header(16, 48000, 2) + bytes(range(8)), 1)
    other = B.pes2(0xBD, B.lpcm_header(16, 48000, 2, substream=0xA1) + bytes(8), 2)
    ac3 = B.pes2(0xBD, bytes([0x80, 1, 0, 1]) + bytes(40), 3)
    mpa, mpa2 = B.pes2(0xC0, b"\xff\xfd" + bytes(30), 4), B.pes2(0xC3, b"\xff\xfd" + bytes(20), 5)
    head = B.pack_header() + B.system_header()
    mixed = head + ac3 + mpa + lpcm + mpa2 + other + mpa + lpcm
    for mode, want in ((ps.TRACK_FIRST, (b"\xff\xfd" + bytes(30)) * 2), (ps.TRACK_LPCM, bytes(range(8)) * 2), (ps.TRACK_MPEG_AUDIO, (b"\xff\xfd" + bytes(30)) * 2)):
        events, error = M.demux(mixed, mode)
        assert error is None and track_of(events) == want
        for piece in (1, 13, len(mixed)):
            assert as_model(demux_in_pieces(mixed, piece, mode)) == events
    lpcm_first = head + lpcm + mpa + other + lpcm
    events, error = M.demux(lpcm_first)
    assert error is None and events[0][1]["substream_id"] == 0xA0 and track_of(events) == bytes(range(8)) * 2
    assert as_model(demux_in_pieces(lpcm_first, 3)) == events
    refuses(head + ac3 + B.video(), "MPEG-PS has no supported DVD LPCM track")
    refuses(head + mpa, "MPEG-PS has no supported DVD LPCM track", mode=ps.TRACK_LPCM)
    refuses(head + lpcm, "MPEG-PS has no supported DVD LPCM track", mode=ps.TRACK_MPEG_AUDIO)
    refuses(b"", "MPEG-PS has no supported DVD LPCM track")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def test_refusals_from_the_pes_headers():
    head = B.pack_header()
    good = B.pes2(0xBD, B.lpcm_header(16, 48000, 1) + b"\x01\x02", 1)
    refuses(head + good + B.packet(0xBD, b"\x81\x00"), "MPEG-2 PES header is truncated", packets=1)
    refuses(head + good + B.packet(0xBD, b"\xff\x81\x80\x05\x21\x00"), "MPEG-2 PES optional header is truncated", packets=1)
    refuses(head + good + B.packet(0xBD, b"\xff\xff\x60\x20"), "MPEG-1 PES header is truncated", packets=1)
    refuses(head + good + B.packet(0xBD, b"\x21\x00\x01\x00"), "MPEG-1 PES timestamp is truncated", packets=1)
    refuses(head + good + B.packet(0xBD, b"\x60\x20\x31" + bytes(8)), "MPEG-1 PES timestamp is truncated", packets=1)
    refuses(head + good + b"\x00\x00\x01\xbd\x00", "MPEG-PS PES length is truncated", packets=1)
    refuses(head + good + good[:-1], "MPEG-PS PES packet is truncated", packets=1)
    refuses(head + B.pes2(0xC0, bytes(40), 1)[:-1], "MPEG-PS PES packet is truncated", packets=0)
    # ignored, not refused: nothing but stuffing, and an MPEG-1 header that begins with none of the three forms
    for ignored in (B.packet(0xBD, b"\xff" * 9), B.packet(0xBD, b""), B.packet(0xBD, b"\x55" + bytes(20)), B.packet(0xBD, b"\x60\x20\x00" + bytes(20))):
        events, error = M.demux(head + good + ignored + good)
        assert error is None and track_of(events) == b"\x01\x02" * 2
        assert as_model(demux_in_pieces(head + good + ignored + good, 4)) == events
    # a video packet cut off, a pack header cut off: the end of the stream, no refusal
    for tail in (B.video()[:-5], B.pack_header()[:9], b"\x00\x00\x01", b"\x00\x00\x01\xe0\x01"):
        events, error = M.demux(head + good + tail)
        assert error is None and as_model(demux_in_pieces(head + good + tail, 2)) == events


def test_refusals_from_dvd_lpcm():
    head = B.pack_header(False)
    def one(bits, channels, n, rate=48000, k=0):
        return B.pes1(0xBD, B.lpcm_header(bits, rate, channels, frames=k) + bytes(range(n)), 90000 + k)
    refuses(head + one(20, 2, 10), "20-bit DVD LPCM decoding is not implemented", packets=0)
    bad = bytearray(B.lpcm_header(16, 48000, 2))
    bad[5] |= 0xC0
    refuses(head + B.pes2(0xBD, bytes(bad) + bytes(8), 1), "unsupported DVD LPCM sample depth 28", packets=0)
    refuses(head + one(16, 2, 8) + one(24, 2, 12), "DVD LPCM format changes mid-stream", packets=1)
    refuses(head + one(16, 2, 8) + one(16, 1, 8), "DVD LPCM format changes mid-stream", packets=1)
    refuses(head + one(16, 2, 8) + one(16, 2, 8, rate=96000), "DVD LPCM format changes mid-stream", packets=1)
    refuses(head + one(16, 2, 8) + one(20, 2, 10), "DVD LPCM format changes mid-stream", packets=1)
    refuses(head + one(16, 2, 8) + one(16, 2, 7), "DVD LPCM ends with a partial sample block", packets=2)
    refuses(head + one(16, 6, 11), "DVD LPCM ends with a partial sample block", packets=0)
    refuses(head + one(24, 2, 23), "DVD LPCM ends with a partial 24-bit sample block", packets=1)
    refuses(head + one(24, 8, 12), "DVD LPCM ends with a partial 24-bit sample block", packets=0)
    refuses(head + one(24, 6, 71), "DVD LPCM ends with a partial 24-bit sample block", packets=0)
    events, error = M.demux(head + one(24, 8, 12) + one(24, 8, 12))  # two packets make one block
    assert error is None and [len(e) for k, e in events if k == "packet"] == [24]
    short = B.pes2(0xBD, B.lpcm_header(16, 48000, 2)[:6], 1)  # fewer than 7 bytes: not LPCM
    refuses(head + short, "MPEG-PS has no supported DVD LPCM track")


def test_budgets_and_decode_file_refusals_that_need_no_device():
    d = ps.PsAudioDemuxer()
    refused(lambda: d.add(bytes(4 * 1024 * 1024 + 1)), "MPEG-PS input chunk exceeds the 4194304 byte streaming budget")
    refused(lambda: d.add(b"\x00"), "MPEG-PS input chunk exceeds the 4194304 byte streaming budget")  # it stays refused
    d.close()
    with pytest.raises(SoundkitError) as e:  # no such track mode
        ps.PsAudioDemuxer(3)
    assert e.value.status == -1
    head = B.pack_header()
    refused(lambda: ps.decode_file(head + B.video()), "Invalid input format: MPEG-PS has no supported DVD LPCM track")
    twenty = B.pes2(0xBD, B.lpcm_header(20, 48000, 2) + bytes(10), 1)
    refused(lambda: ps.decode_file(head + twenty), "Invalid input format: 20-bit DVD LPCM decoding is not implemented")
    refused(lambda: ps.decode_file(head + B.pes2(0xC0, b"\xff\xfd" + bytes(30), 4) + twenty), "Invalid input format: 20-bit DVD LPCM decoding is not implemented")
    partial = B.pes2(0xBD, B.lpcm_header(16, 48000, 2) + bytes(6), 1)
    refused(lambda: ps.decode_file(head + partial), "Invalid input format: DVD LPCM ends with a partial sample block")


@pytest.mark.parametrize("kind", ["lpcm", "mpeg audio"])
def test_the_payload_budget_is_met_by_a_stream_that_is_fed_and_drained(kind):
    """decode_mpeg_ps_audio's 512 MiB (lib.rs:618-626), which the walker also holds an MPEG audio track to: 8193 PES packets of 65 524
    payload bytes pass, the 8194th is refused -- and a last packet that fills the budget to the byte is not"""
    n = 65524
    if kind == "lpcm":
        one = B.pes2(0xBD, B.lpcm_header(16, 48000, 2) + bytes(n))
        last = lambda k: B.pes2(0xBD, B.lpcm_header(16, 48000, 2) + bytes(k))  # noqa: E731
    else:
        one = B.pes2(0xC0, bytes(n))
        last = lambda k: B.pes2(0xC0, bytes(k))  # noqa: E731
    assert len(one) <= 6 + 65535 and 63 * len(one) <= 4 * 1024 * 1024
    left = 512 * 1024 * 1024 - 8193 * n
    assert 0 < left < n and left % 4 == 0
    for tail, text in ((last(left), None), (last(left + 4), "MPEG-PS audio payload exceeds budget"), (one, "MPEG-PS audio payload exceeds budget")):
        d = ps.PsAudioDemuxer()
        assert d.add(B.pack_header()) == []
        packets = 0
        for _ in range(8193 // 63):
            packets += sum(len(e.data) == n for e in d.add(one * 63) if isinstance(e, ps.PsPacket))
        packets += sum(len(e.data) == n for e in d.add(one * (8193 % 63)) if isinstance(e, ps.PsPacket))
        assert packets == 8193
        if text is None:
            assert [len(e.data) for e in d.add(tail)] == [left] and d.finish() == []
        else:
            e = refused(lambda: d.add(tail), text)
            assert e.events == []
            refused(lambda: d.add(b"\x00"), text)  # it stays refused
        d.close()


def test_a_dvd_lpcm_track_without_a_sample_emits_no_frames():
    """one LPCM PES whose payload is exactly the seven header bytes: a track, a config, and nothing to decode"""
    data = B.pack_header() + B.pes2(0xBD, B.lpcm_header(16, 48000, 2), 1)
    events, error = M.demux(data)
    assert error is None and [kind for kind, _ in events] == ["config"] and as_model(demux_in_pieces(data, 3)) == events
    refused(lambda: ps.decode_file(data), "Decoding failed: MPEG-PS DVD LPCM track emitted no frames")
    data = B.pack_header() + B.pes2(0xBD, B.lpcm_header(24, 48000, 2), 1)
    refused(lambda: ps.decode_file(data), "Decoding failed: MPEG-PS DVD LPCM track emitted no frames")


def test_the_schedulers_sniffing_rule():
    """pipeline.cpp takes 00 00 01 BA in front of the transport-stream and the MPEG sync rules: four bytes decide"""
    data = CASES["mp2"][0]
    assert ps.sniff(data[:4]) and not ps.sniff(data[:3]) and not ps.sniff(b"\x00\x00\x01\xbb") and not ps.sniff(B.MP2[:64])


# ---- fuzz and ABI ----------------------------------------------------------------------------------------------------------------------

def test_mutated_streams_under_sanitizers(tmp_path):
    """tests/fuzz_ps.cpp: csrc/ps_stream.h alone with AddressSanitizer + UBSan on the CPU -- seeded mutations of the builder's streams
    through the demuxer in its three track modes, whole and in pieces"""
    exe = str(tmp_path / "fuzz_ps")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "fuzz_ps.cpp")], cwd=HERE)
    paths = []
    for name, case in sorted(CASES.items()):
        paths.append(str(tmp_path / (name + ".mpg")))
        with open(paths[-1], "wb") as f:
            f.write(case[0])
    out = subprocess.run([exe, "100"] + paths, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "fuzz_ps ok" in out.stdout


def test_the_abi_exports_the_new_symbols():
    for name in ("sk_ps_demuxer_create", "sk_ps_demuxer_destroy", "sk_ps_demuxer_add", "sk_ps_demuxer_finish", "sk_ps_demuxer_next",
                 "sk_ps_demuxer_last_error"):
        assert hasattr(lib, name), name
    assert lib.sk_strerror(ps.ERR_STREAM).decode() == "MPEG-PS stream rejected"

"""The AVI demuxer on the host (csrc/avi_stream.h through soundkit_amd.avi): its events against tests/avi_model.py on the files
tests/avi_builder.py writes, whole and in pieces of 1, 7, 188, 4096 and 65 536 bytes; every refusal with its text, from the smallest
file that provokes it; the budgets -- the 512 MiB of payload by feeding one 4 MiB chunk again and again while the packets are taken, which
needs no file of that size --; the scheduler's sniffing rule as Python states it; and a sanitizer fuzz (tests/fuzz_avi.cpp).  No GPU."""
import os
import struct
import subprocess

import pytest

import avi_builder as B
import avi_model as M
from soundkit_amd import SoundkitError, avi, lib

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = B.cases()
PCM16 = B.waveformat(1, 1, 16000, 16)


def demux_in_pieces(data, piece):
    """-> the events through AviAudioDemuxer; a refusal raises with .events = what came before it"""
    d, events = avi.AviAudioDemuxer(), []
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
        if isinstance(e, avi.AviAudioConfig):
            out.append(("config", dict(index=e.stream_index, tag=e.format_tag, channels=e.channels, rate=e.sample_rate, bits=e.bits_per_sample)))
        else:
            out.append(("packet", e.data))
    return out


def refused(fn, text):
    with pytest.raises(SoundkitError) as e:
        fn()
    assert str(e.value).endswith(": " + text), str(e.value)
    return e.value


def refuses(data, text, packets=None):
    """the demuxer and the model refuse `data` with `text`, after the same events, however the bytes are cut"""
    events, error = M.demux(data)
    assert error == text, error
    for piece in (max(len(data), 1), 777, 5):
        e = refused(lambda: demux_in_pieces(data, piece), text)
        assert as_model(e.events) == events
    if packets is not None:
        assert sum(kind == "packet" for kind, _ in events) == packets


def track_of(events):
    return b"".join(e for kind, e in events if kind == "packet")


# ---- events against the model, however the bytes are cut -------------------------------------------------------------------------------

@pytest.mark.parametrize("piece", [0, 1, 7, 188, 4096, 65536])
@pytest.mark.parametrize("name", sorted(CASES))
def test_demuxer_matches_model_however_it_is_cut(name, piece):
    data = CASES[name][0]
    events, error = M.demux(data)
    assert error is None and events[0][0] == "config" and sum(kind == "config" for kind, _ in events) == 1
    assert as_model(demux_in_pieces(data, piece or len(data))) == events


@pytest.mark.parametrize("name", sorted(CASES))
def test_built_files_hold_what_they_are_named_for(name):
    data, tag, channels, rate, bits, index, track = CASES[name]
    events, error = M.demux(data)
    assert error is None
    assert events[0] == ("config", dict(index=index, tag=tag, channels=channels, rate=rate, bits=bits))
    assert track_of(events) == track and len(events) > 4
    assert avi.sniff(data) and M.looks_like_avi(data)


def test_the_structures_the_files_are_built_for():
    assert CASES["pcm16_records"][0].count(b"rec ") == 6 and CASES["pcm16_avix"][0].count(b"RIFF") == 2
    assert b"AVIX" in CASES["pcm16_avix"][0] and b"ix00" in CASES["pcm16_avix"][0]
    odd = [len(e) for kind, e in M.demux(CASES["u8_odd_chunks"][0])[0] if kind == "packet"]
    assert {999, 1, 1001} <= set(odd)
    assert CASES["pcm16_audio_first"][0].index(b"auds") < CASES["pcm16_audio_first"][0].index(b"vids")
    assert CASES["pcm16_stereo"][0].index(b"vids") < CASES["pcm16_stereo"][0].index(b"auds")


@pytest.mark.parametrize("piece", [0, 1, 7, 188, 4096])
def test_a_file_cut_inside_a_chunk_gives_the_chunks_in_front_of_it(piece):
    data, front = B.cut_inside_a_chunk()
    events, error = M.demux(data)
    assert error is None and track_of(events) == front and len(events) == 5
    assert as_model(demux_in_pieces(data, piece or len(data))) == events


def test_a_file_cut_inside_a_chunk_header_is_trailing_data():
    """for_each_riff_chunk on a prefix: where no 8-byte header fits any more, what is left must be zeros (lib.rs:530-532)"""
    whole = CASES["pcm16_audio_first"][0]
    at = whole.index(b"00wb", whole.index(b"00wb") + 1)  # the second audio chunk's header
    refuses(whole[:at + 5], "AVI chunk table has trailing data", packets=1)


def test_the_stream_index_is_hex():
    """avi_stream_id: `0a` names stream 10"""
    strls = [B.video_strl()] * 10 + [B.strl(b"auds", PCM16)]
    data = B.riff(b"AVI ", B.hdrl(*strls), B.lst(b"movi", B.chunk(b"10wb", b"\x01\x02"), B.chunk(b"0awb", b"\x03\x04"), B.chunk(b"0Awb", b"\x05\x06")))
    events, error = M.demux(data)
    assert error is None and events[0][1]["index"] == 10 and track_of(events) == b"\x03\x04\x05\x06"
    assert as_model(demux_in_pieces(data, 3)) == events


def test_a_chunk_that_runs_past_its_list_ends_the_list():
    """a leaf behind its container's end is dropped, a LIST is entered for what is there, and neither is followed by anything of the parent"""
    inner = B.wb(1, b"\x01\x02") + B.chunk(b"01wb", b"\x03\x04\x05\x06", size=400)
    data = B.riff(b"AVI ", B.hdrl(B.video_strl(), B.strl(b"auds", PCM16)), B.lst(b"movi", B.lst(b"rec ", inner), B.wb(1, b"\x07\x08")), B.chunk(b"idx1", bytes(16)))
    events, error = M.demux(data)
    assert error is None and track_of(events) == b"\x01\x02\x07\x08"
    assert as_model(demux_in_pieces(data, 1)) == events
    over = B.lst(b"rec ", B.wb(0, b"\x01\x02"), B.wb(0, b"\x03\x04"), size=4 + 10 + 10 + 50)  # the LIST itself claims more than `movi` holds
    data = B.riff(b"AVI ", B.hdrl(B.strl(b"auds", PCM16)), B.lst(b"movi", over, size=4 + len(over)))
    events, error = M.demux(data)
    assert error is None and track_of(events) == b"\x01\x02\x03\x04"
    for piece in (1, 9, len(data)):
        assert as_model(demux_in_pieces(data, piece)) == events


def test_a_chunk_above_a_megabyte_is_one_packet():
    """larger than the 64 KiB the Python demuxer takes packets into at first: the buffer grows to what sk_avi_demuxer_next says it needs"""
    data, tag, channels, rate, bits, index, track = B.big_chunk()
    events, error = M.demux(data)
    assert error is None and [len(e) for kind, e in events if kind == "packet"] == [len(track) - 3000, 3000] and track_of(events) == track
    for piece in (4096, 65536, len(data)):
        assert as_model(demux_in_pieces(data, piece)) == events


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def with_strl(*strl_children):
    return B.riff(b"AVI ", B.lst(b"hdrl", B.lst(b"strl", *strl_children)), B.lst(b"movi", B.wb(0, b"\x00\x00")))


def test_refusals_from_the_header():
    strh = B.chunk(b"strh", b"auds" + bytes(52))
    refuses(with_strl(strh), "AVI audio stream has no strf format")
    refuses(with_strl(strh, B.chunk(b"strf", PCM16[:15])), "AVI WAVEFORMAT is truncated")
    refuses(with_strl(strh, B.chunk(b"strf", B.waveformat(1, 0, 16000, 16))), "AVI channel count is invalid")
    refuses(with_strl(strh, B.chunk(b"strf", B.waveformat(1, 256, 16000, 16))), "AVI channel count is invalid")
    refuses(with_strl(strh, B.chunk(b"strf", B.waveformat(1, 2, 0, 16))), "AVI sample rate is zero")
    refuses(B.riff(b"AVI ", B.hdrl(B.video_strl()), B.lst(b"movi", B.dc(0))), "AVI has no audio stream")
    refuses(B.riff(b"AVI ", B.hdrl(B.video_strl())), "AVI has no audio stream")
    refuses(b"", "AVI has no audio stream")
    refuses(b"RIFF\x04\x00\x00", "AVI has no audio stream")  # fewer than the twelve bytes of a form's head
    wide = bytearray(B.waveformat(1, 255, 16000, 16))
    wide[14:16] = struct.pack("<H", 4000)  # wBitsPerSample above 255 is clamped
    clamped = M.demux(with_strl(strh, B.chunk(b"strf", bytes(wide))))
    assert clamped[1] is None and clamped[0][0][1]["bits"] == 255 and clamped[0][0][1]["channels"] == 255
    assert as_model(demux_in_pieces(with_strl(strh, B.chunk(b"strf", bytes(wide))), 6)) == clamped[0]


def test_refusals_from_the_forms_and_chunks():
    good = B.hdrl(B.strl(b"auds", PCM16))
    refuses(b"JUNK" + bytes(20), "AVI contains data outside a RIFF form")
    refuses(B.riff(b"WAVE", good), "invalid AVI RIFF form type")
    refuses(B.riff(b"AVI ", good, B.lst(b"movi", B.wb(0, b"\x01\x02"))) + B.riff(b"AVIZ"), "invalid AVI RIFF form type", packets=1)
    refuses(B.riff(b"AVI ", good, B.chunk(b"LIST", b"mo")), "AVI LIST type is truncated")
    refuses(B.riff(b"AVI ", good, B.lst(b"movi", B.wb(0, b"\x01\x02"), b"\x00\x00\x07")), "AVI chunk table has trailing data", packets=1)
    refuses(B.riff(b"AVI ", B.lst(b"hdrl", B.strl(b"auds", PCM16), b"xyz")), "AVI chunk table has trailing data")
    zeros = B.riff(b"AVI ", good, B.lst(b"movi", B.wb(0, b"\x01\x02"), bytes(7)))  # zeros behind the last chunk are padding
    assert M.demux(zeros)[1] is None and as_model(demux_in_pieces(zeros, 3)) == M.demux(zeros)[0]
    behind = B.riff(b"AVI ", good, B.lst(b"movi", B.wb(0, b"\x01\x02"))) + b"garbage behind the last form, which is not looked at"
    assert M.demux(behind)[1] is None and as_model(demux_in_pieces(behind, 11)) == M.demux(behind)[0]


def test_record_nesting():
    def nested(depth):
        inner = B.wb(0, b"\x01\x02")
        for _ in range(depth):
            inner = B.lst(b"rec ", inner)
        return B.riff(b"AVI ", B.hdrl(B.strl(b"auds", PCM16)), B.lst(b"movi", inner))
    events, error = M.demux(nested(8))
    assert error is None and track_of(events) == b"\x01\x02" and as_model(demux_in_pieces(nested(8), 2)) == events
    refuses(nested(9), "AVI record nesting exceeds budget", packets=0)


def test_budgets():
    d = avi.AviAudioDemuxer()
    refused(lambda: d.add(bytes(4 * 1024 * 1024 + 1)), "AVI input chunk exceeds the 4194304 byte streaming budget")
    refused(lambda: d.add(b"R"), "AVI input chunk exceeds the 4194304 byte streaming budget")  # it stays refused
    d.close()
    # 1 000 001 chunks in one list
    many = B.riff(b"AVI ", B.hdrl(B.strl(b"auds", PCM16)), B.lst(b"movi", B.chunk(b"JUNK", b"") * 1000001))
    assert M.demux(many)[1] == "AVI chunk count exceeds budget"
    refused(lambda: demux_in_pieces(many, 1 << 20), "AVI chunk count exceeds budget")
    fits = B.riff(b"AVI ", B.hdrl(B.strl(b"auds", PCM16)), B.lst(b"movi", B.chunk(b"JUNK", b"") * 1000000))
    assert [type(e) for e in demux_in_pieces(fits, 1 << 20)] == [avi.AviAudioConfig]
    # a header list above this project's bound is refused where its size is read
    big = b"RIFF" + struct.pack("<I", 1 << 30) + b"AVI " + b"LIST" + struct.pack("<I", 16 * 1024 * 1024 + 5) + b"hdrl"
    refused(lambda: demux_in_pieces(big, 24), "AVI hdrl list exceeds the 16777216 byte header budget")


def fed_up_to_the_payload_budget():
    """a demuxer that has handed out 128 chunks of 4 MiB - 8 bytes and one of 1024: exactly 512 MiB of payload -> (demuxer, packets so far)"""
    d = avi.AviAudioDemuxer()
    head = b"RIFF" + struct.pack("<I", 0xFFFFFFF0) + b"AVI " + B.hdrl(B.strl(b"auds", PCM16)) + b"LIST" + struct.pack("<I", 0xFFFFFF00) + b"movi"
    events = d.add(head)
    assert [type(e) for e in events] == [avi.AviAudioConfig]
    piece = B.wb(0, bytes(4 * 1024 * 1024 - 8))  # a chunk and its header: the most one add takes
    packets = 0
    for _ in range(128):
        got = d.add(piece)
        assert len(got) == 1 and len(got[0].data) == 4 * 1024 * 1024 - 8
        packets += 1
    got = d.add(B.wb(0, bytes(1024)))
    assert len(got) == 1 and 128 * (4 * 1024 * 1024 - 8) + 1024 == 512 * 1024 * 1024
    return d, packets + 1


def test_the_payload_budget_is_met_by_a_stream_that_is_fed_and_drained():
    """collect_avi_audio_chunks' 512 MiB (lib.rs:549-553): exactly the budget passes, two bytes more are refused once their chunk is whole,
    and a file that ends inside the chunk that would cross it ends quietly, as the reference's prefix rule has it"""
    d, packets = fed_up_to_the_payload_budget()
    assert packets == 129 and d.add(B.dc(1)) == [] and d.add(B.wb(1, b"\x01\x02")) == []  # other streams' chunks do not count
    over = B.chunk(b"00wb", bytes(3000))
    assert d.add(over[:8]) == [] and d.add(over[8:-1]) == []  # not whole yet: nothing is said
    e = refused(lambda: d.add(over[-1:]), "AVI audio payload exceeds budget")
    assert e.events == []
    refused(lambda: d.add(b"x"), "AVI audio payload exceeds budget")  # it stays refused
    d.close()
    d, _ = fed_up_to_the_payload_budget()
    assert d.add(B.wb(0, b"\x01\x02")[:9]) == [] and d.finish() == []  # the file ends inside the chunk: no packet, no refusal
    d.close()
    d, _ = fed_up_to_the_payload_budget()
    e = refused(lambda: d.add(B.wb(0, b"\x01\x02")), "AVI audio payload exceeds budget")  # the smallest chunk that crosses it
    d.close()


def test_decode_file_refusals_that_need_no_device():
    def tagged(tag, bits=16):
        return B.riff(b"AVI ", B.hdrl(B.strl(b"auds", B.waveformat(tag, 2, 48000, bits))), B.lst(b"movi", B.wb(0, bytes(48))))
    for tag in (0x160, 0x161, 0x162, 0x163):
        refused(lambda: avi.decode_file(tagged(tag)), "Invalid input format: AVI WMA decoding is not implemented")
    refused(lambda: avi.decode_file(tagged(0x2000)), "Invalid input format: AVI AC-3 audio is not built")
    refused(lambda: avi.decode_file(tagged(0x0002)), "Invalid input format: unsupported AVI audio format tag 0x0002")
    refused(lambda: avi.decode_file(tagged(0xFFFE)), "Invalid input format: unsupported AVI audio format tag 0xfffe")
    refused(lambda: avi.decode_file(tagged(1, 12)), "Invalid input format: unsupported AVI integer PCM depth 12")
    refused(lambda: avi.decode_file(tagged(3, 64)), "Invalid input format: unsupported AVI float PCM depth 64")
    many = B.riff(b"AVI ", B.hdrl(B.strl(b"auds", B.waveformat(1, 33, 8000, 8))), B.lst(b"movi", B.wb(0, bytes(66))))
    refused(lambda: avi.decode_file(many), "Invalid input format: AVI 8-bit PCM with more than 32 channels is not built")
    partial = B.riff(b"AVI ", B.hdrl(B.strl(b"auds", B.waveformat(1, 2, 48000, 16))), B.lst(b"movi", B.wb(0, bytes(47))))
    refused(lambda: avi.decode_file(partial), "Invalid input format: AVI PCM ends with a partial sample frame")
    empty = B.riff(b"AVI ", B.hdrl(B.strl(b"auds", PCM16)), B.lst(b"movi", B.dc(1), B.wb(0, b"")))
    refused(lambda: avi.decode_file(empty), "Invalid input format: AVI audio track contains no packets")
    refused(lambda: avi.decode_file(B.riff(b"AVI ", B.hdrl(B.video_strl()))), "Invalid input format: AVI has no audio stream")


def test_the_schedulers_sniffing_rule():
    """pipeline.cpp takes `RIFF....AVI ` where it takes `RIFF....WAVE`: twelve bytes decide"""
    data = CASES["pcm16_stereo"][0]
    assert avi.sniff(data[:12]) and not avi.sniff(data[:11]) and not avi.sniff(B.golden("wav_stereo_A_Tusk.wav")[:12])
    assert not avi.sniff(b"RIFF" + bytes(4) + b"AVIX")


# ---- fuzz and ABI ----------------------------------------------------------------------------------------------------------------------

def test_mutated_files_under_sanitizers(tmp_path):
    """tests/fuzz_avi.cpp: csrc/avi_stream.h alone with AddressSanitizer + UBSan on the CPU -- seeded mutations of the builder's files
    through the demuxer, whole and in pieces"""
    exe = str(tmp_path / "fuzz_avi")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "fuzz_avi.cpp")], cwd=HERE)
    paths = []
    for name, case in sorted(CASES.items()):
        paths.append(str(tmp_path / (name + ".avi")))
        with open(paths[-1], "wb") as f:
            f.write(case[0])
    out = subprocess.run([exe, "150"] + paths, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "fuzz_avi ok" in out.stdout


def test_the_abi_exports_the_new_symbols():
    for name in ("sk_avi_demuxer_create", "sk_avi_demuxer_destroy", "sk_avi_demuxer_add", "sk_avi_demuxer_finish", "sk_avi_demuxer_next",
                 "sk_avi_demuxer_last_error"):
        assert hasattr(lib, name), name
    assert lib.sk_strerror(avi.ERR_STREAM).decode() == "AVI stream rejected"

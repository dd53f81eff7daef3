"""MP4 / MOV `pcm` and `fLaC` sample entries on the host (csrc/mp4_stream.h) through the C ABI: the eight MOV fixtures against the hashes
the reference's tests record for them, built sample entries of every version and name with every refusal text, the runs of frames a PCM
track's samples leave as (from the index and from the demuxer alike), the three `dfLa` forms, and a sanitizer fuzz
(tests/fuzz_container_pcm.cpp).  No GPU."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import mp4_builder as B
import mp4_pcm_builder as P
from soundkit_amd import SoundkitError, mp4
from soundkit_amd._lib import Mp4TrackInfo, lib

HERE = os.path.dirname(os.path.abspath(__file__))
MOV = os.path.join(HERE, "golden", "mov_pcm")
HASHES = json.load(open(os.path.join(MOV, "pcm_hashes.json")))
FLAC = os.path.join(HERE, "golden", "flac")


def demux(data, piece):
    d, events = mp4.Mp4Demuxer(), []
    try:
        for at in range(0, len(data), piece):
            events += d.add(data[at:at + piece])
        events += d.finish()
    finally:
        d.close()
    return events[0], events[1:]


def canonical(payload, bits, big_endian):
    width = (bits + 7) // 8
    return np.frombuffer(payload, np.uint8).reshape(-1, width)[:, ::-1].tobytes() if big_endian else payload


def refusal(data):
    with pytest.raises(SoundkitError) as e:
        mp4.Mp4Index.from_file(data)
    return str(e.value)


def pcm_file(entry, frames=10, width=4, **more):
    return P.movie(entry, [bytes(k & 255 for k in range(frames * width))], sample_size=width, **more)


# ---- the fixtures ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(HASHES["mov_pcm"]))
def test_mov_fixture_is_described_and_its_payload_has_the_recorded_hash(name):
    want = HASHES["mov_pcm"][name]
    data = open(os.path.join(MOV, name), "rb").read()
    index = mp4.Mp4Index.from_file(data)
    c = index.config
    assert (c.codec, c.sample_rate, c.channels, c.bits_per_sample, c.codec_private) == ("pcm", 48000, 2, want["bits"], b"")
    assert c.pcm == {"codec_id": want["codec_id"], "big_endian": want["big_endian"], "is_float": want["float"], "bits_per_sample": want["bits"],
                     "bytes_per_frame": 2 * want["bits"] // 8, "frames_per_packet": 1}
    width = 2 * want["bits"] // 8
    assert [(size, duration, start) for _, size, duration, start in index.samples] == [(4096 * width, 4096, 0), (704 * width, 704, 4096)]
    payload = b"".join(index.packet_bytes(data))
    assert hashlib.sha256(canonical(payload, want["bits"], want["big_endian"])).hexdigest() == want["sha256"]
    # `moov` lies behind `mdat` in these files: the demuxer says so; rearranged, it hands out the index's runs
    with pytest.raises(SoundkitError, match="MP4 mdat appears before moov; use the seekable MP4 packet API"):
        demux(data, 4096)
    fast = B.faststart(data)
    for piece in (1 << 20, 4099):
        config, packets = demux(fast, piece)
        assert config.pcm == c.pcm and [(len(p.data), p.duration, p.start_time) for p in packets] == [(s, d, t) for _, s, d, t in index.samples]
        assert b"".join(p.data for p in packets) == payload


def test_the_new_codec_ids_leave_the_track_record_as_it_was():
    assert C.sizeof(Mp4TrackInfo) == 64  # ten u32, three u64: the layout the AAC / ALAC callers were built against
    assert mp4.CODECS == {1: "aac", 2: "alac", 3: "flac", 4: "pcm"}


# ---- built sample entries ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, big", [(b"sowt", False), (b"twos", True)])
@pytest.mark.parametrize("bits", [16, 24, 32])
def test_sowt_and_twos_take_the_declared_bits(name, big, bits):
    c = mp4.Mp4Index.from_file(pcm_file(P.sound_entry(name, 0, 2, bits), 12, 2 * bits // 8)).config
    assert c.pcm == {"codec_id": name.decode(), "big_endian": big, "is_float": False, "bits_per_sample": bits, "bytes_per_frame": 2 * bits // 8,
                     "frames_per_packet": 1}


def test_version_one_and_two_geometry():
    """the values of the reference's parses_quicktime_version_one_and_two_lpcm_geometry"""
    one = mp4.Mp4Index.from_file(pcm_file(P.sound_entry(b"sowt", 1, 2, 16, v1=(1, 2, 4, 2)))).config
    assert (one.pcm["bytes_per_frame"], one.pcm["frames_per_packet"], one.bits_per_sample) == (4, 1, 16)
    fallback = mp4.Mp4Index.from_file(pcm_file(P.sound_entry(b"sowt", 1, 2, 0, v1=(1, 3, 6, 3)), width=6)).config  # bits from bytes per sample
    assert (fallback.bits_per_sample, fallback.pcm["bytes_per_frame"]) == (24, 6)
    two = mp4.Mp4Index.from_file(pcm_file(P.sound_entry(b"lpcm", 2, 2, 24, v2=dict(flags=P.SIGNED | P.PACKED)), width=6)).config
    assert (two.sample_rate, two.channels, two.bits_per_sample) == (48000, 2, 24)
    assert two.pcm == {"codec_id": "lpcm", "big_endian": False, "is_float": False, "bits_per_sample": 24, "bytes_per_frame": 6, "frames_per_packet": 1}
    big_float = mp4.Mp4Index.from_file(pcm_file(P.sound_entry(b"lpcm", 2, 2, 32, v2=dict(flags=P.FLOAT | P.BIG | P.PACKED)), width=8)).config
    assert (big_float.pcm["big_endian"], big_float.pcm["is_float"]) == (True, True)
    high_rate = mp4.Mp4Index.from_file(pcm_file(P.sound_entry(b"lpcm", 2, 2, 16, rate=192000, v2=dict(rate=191999.6)))).config
    assert high_rate.sample_rate == 192000  # the f64 rate, rounded


@pytest.mark.parametrize("name, bits, is_float", [(b"in24", 24, False), (b"in32", 32, False), (b"fl32", 32, True), (b"fl64", 64, True)])
def test_enda_in_the_entry_and_inside_wave(name, bits, is_float):
    width = 2 * bits // 8
    for children, big in ((b"", True), (P.enda(0), True), (P.enda(1), False), (P.wave(P.enda(1)), False), (P.wave(P.enda(0)), True)):
        for version in (0, 1):
            c = mp4.Mp4Index.from_file(pcm_file(P.sound_entry(name, version, 2, 16, children=children, v1=(1, bits // 8, width, bits // 8)), width=width)).config
            assert (c.bits_per_sample, c.pcm["big_endian"], c.pcm["is_float"], c.pcm["bytes_per_frame"]) == (bits, big, is_float, width)


def test_every_refusal_has_its_text():
    assert "unsupported QuickTime audio sample-entry version 3" in refusal(pcm_file(P.sound_entry(b"sowt", 3)))
    assert "invalid QuickTime enda flag 2" in refusal(pcm_file(P.sound_entry(b"in24", 0, children=P.enda(2)), width=6))
    assert "invalid QuickTime enda flag 258" in refusal(pcm_file(P.sound_entry(b"fl32", 0, children=P.wave(P.enda(258))), width=8))
    assert "QuickTime enda atom is truncated" in refusal(pcm_file(P.sound_entry(b"in24", 0, children=B.box(b"enda", b"\1")), width=6))
    for version in (0, 1):
        assert "QuickTime lpcm requires a version-two sample entry" in refusal(pcm_file(P.sound_entry(b"lpcm", version)))
    assert "non-interleaved QuickTime LPCM is unsupported" in refusal(
        pcm_file(P.sound_entry(b"lpcm", 2, 2, 24, v2=dict(flags=P.SIGNED | P.PACKED | P.NON_INTERLEAVED)), width=6))
    assert "unsigned QuickTime LPCM is unsupported" in refusal(pcm_file(P.sound_entry(b"lpcm", 2, v2=dict(flags=P.PACKED))))
    assert "unpacked QuickTime LPCM is unsupported" in refusal(pcm_file(P.sound_entry(b"lpcm", 2, v2=dict(flags=P.SIGNED))))
    assert "aligned-high QuickTime LPCM is unsupported" in refusal(pcm_file(P.sound_entry(b"lpcm", 2, v2=dict(flags=P.SIGNED | P.PACKED | P.ALIGNED_HIGH))))
    assert "invalid QuickTime version-two sample rate" in refusal(pcm_file(P.sound_entry(b"lpcm", 2, v2=dict(rate=float("nan")))))
    assert "invalid QuickTime version-two sample rate -48000" in refusal(pcm_file(P.sound_entry(b"lpcm", 2, v2=dict(rate=-48000.0))))
    assert "invalid QuickTime version-two sample rate 0" in refusal(pcm_file(P.sound_entry(b"lpcm", 2, v2=dict(rate=0.0))))
    assert "QuickTime version-two channel count exceeds u8" in refusal(pcm_file(P.sound_entry(b"lpcm", 2, v2=dict(channels=256))))
    assert "QuickTime version-two sample depth exceeds u8" in refusal(pcm_file(P.sound_entry(b"lpcm", 2, v2=dict(bits=256))))
    cut = P.sound_entry(b"lpcm", 2)
    assert "QuickTime version-two audio sample entry is truncated" in refusal(pcm_file(B.box(b"lpcm", cut[8:8 + 60])))
    assert "QuickTime audio sample entry has zero sample rate or channels" in refusal(pcm_file(P.sound_entry(b"sowt", 0, 0, 16)))
    # a float entry's integer flags are not looked at
    mp4.Mp4Index.from_file(pcm_file(P.sound_entry(b"lpcm", 2, 2, 32, v2=dict(flags=P.FLOAT)), width=8))
    # an entry nobody reads is stepped over: the track is not chosen
    assert "MP4 source has no supported audio track" in refusal(pcm_file(P.sound_entry(b"ulaw", 0, 2, 8), width=2))


def test_the_first_audio_track_with_a_supported_entry_is_chosen():
    pcm = pcm_file(P.sound_entry(b"twos", 0, 2, 16))
    assert mp4.Mp4Index.from_file(pcm).config.codec == "pcm"
    aac = B.regular({"codec": "aac", "sample_rate": 48000, "channels": 2, "private": bytes([0x11, 0x90])}, [b"\1\2\3"] * 3)
    c = mp4.Mp4Index.from_file(aac).config
    assert (c.codec, c.pcm, c.sample_rate) == ("aac", None, 48000)


def test_fragmented_files_are_described_and_decode_file_refuses_them():
    pcm = P.fragmented(P.sound_entry(b"sowt", 0, 2, 16), [bytes(4)] * 10, [1] * 10)
    c = mp4.Mp4Index.from_file(pcm).config
    assert (c.codec, c.fragmented, c.sample_count, c.pcm["codec_id"]) == ("pcm", True, 0, "sowt")
    config, packets = demux(pcm, 613)
    assert config.fragmented and [p.data for p in packets] == [bytes(4)] * 10  # the fragment walk hands out the samples as they are
    with pytest.raises(SoundkitError, match="fragmented MP4 pcm tracks are not built"):
        mp4.decode_file(pcm)
    info, frames, blocks, first = P.flac_frames(open(os.path.join(FLAC, "A_Tusk_is_used_to_make_costly_gifts_16bit.flac"), "rb").read())
    entry = P.sound_entry(b"fLaC", 0, first["channels"], 16, first["sample_rate"], B.box(b"dfLa", P.dfla(info, "dfla")))
    flac = P.fragmented(entry, frames, blocks, first["sample_rate"])
    assert mp4.Mp4Index.from_file(flac).config.codec == "flac"
    with pytest.raises(SoundkitError, match="fragmented MP4 flac tracks are not built"):
        mp4.decode_file(flac)


# ---- runs of frames ----------------------------------------------------------------------------------------------------------------------

def runs(data):
    return [(offset, size, duration, start) for offset, size, duration, start in mp4.Mp4Index.from_file(data).samples]


def same_runs_from_the_demuxer(data, want):
    for piece in (len(data), 4099, 613):
        _, packets = demux(data, piece)
        assert [(len(p.data), p.duration, p.start_time) for p in packets] == [(s, d, t) for _, s, d, t in want]
        assert [p.data for p in packets] == [data[o:o + s] for o, s, _, _ in want]


ENTRY = P.sound_entry(b"sowt", 0, 2, 16)


def test_constant_stsz_runs_are_cut_at_chunks_and_at_4096_frames():
    chunks = [bytes([k]) * (4 * n) for k, n in enumerate((5000, 4096, 1, 9000))]
    data = P.movie(ENTRY, chunks, sample_size=4)
    got = runs(data)
    assert [(s // 4, d) for _, s, d, _ in got] == [(4096, 4096), (904, 904), (4096, 4096), (1, 1), (4096, 4096), (4096, 4096), (808, 808)]
    assert [t for _, _, _, t in got] == [0, 4096, 5000, 9096, 9097, 13193, 17289]
    assert b"".join(data[o:o + s] for o, s, _, _ in got) == b"".join(chunks)
    same_runs_from_the_demuxer(data, got)


def test_constant_stsz_runs_stay_under_one_mebibyte():
    data = P.movie(P.sound_entry(b"sowt", 0, 2, 16), [bytes(1000 * 2049)], sample_size=1000)  # "frames" of 1000 bytes: 1048 fit in 1 MiB
    assert [(s, d) for _, s, d, _ in runs(data)] == [(1048000, 1048), (1001000, 1001)]


def test_constant_stsz_makes_no_record_per_frame():
    """144 000 000 frames in one chunk index to 35 157 runs at once; the file's mdat does not hold them, which the index says"""
    table = P.movie(ENTRY, [bytes(8)], sample_size=4)
    at = table.find(b"stsz")
    big = table[:at + 12] + struct.pack(">I", 144_000_000) + table[at + 16:]
    at = big.find(b"stts")
    big = big[:at + 12] + struct.pack(">I", 144_000_000) + big[at + 16:]
    at = big.find(b"stsc")
    big = big[:at + 16] + struct.pack(">I", 144_000_000) + big[at + 20:]
    assert "MP4 sample 0 extends past the source" in refusal(big)


def test_listed_sizes_merge_only_contiguous_neighbours():
    frames = [bytes([k]) * 4 for k in range(12)]
    chunks = [b"".join(frames[0:4]), b"".join(frames[4:8]), b"".join(frames[8:12])]
    sizes, ones = [[4] * 4] * 3, [[1] * 4] * 3
    together = P.movie(ENTRY, chunks, sizes=sizes, durations=ones)  # three chunks that touch: one run
    assert [(s, d, t) for _, s, d, t in runs(together)] == [(48, 12, 0)]
    same_runs_from_the_demuxer(together, runs(together))
    byte_gap = P.movie(ENTRY, chunks, sizes=sizes, durations=ones, gaps=[0, 3, 0])
    assert [(s, d, t) for _, s, d, t in runs(byte_gap)] == [(16, 4, 0), (32, 8, 4)]
    same_runs_from_the_demuxer(byte_gap, runs(byte_gap))
    # a gap in time cannot be written into a file -- every start is the sum of the durations before it, so a longer frame is still
    # contiguous -- and is held where the tables can be made by hand: check_coalesce in tests/fuzz_container_pcm.cpp (the fuzz test below)
    longer_frame = P.movie(ENTRY, chunks, sizes=sizes, durations=[[1, 1, 1, 1], [1, 1, 1, 5], [1, 1, 1, 1]])
    assert [(s, d, t) for _, s, d, t in runs(longer_frame)] == [(48, 16, 0)]
    # the frame cap counts a run's duration: 4096 ticks a run
    n = 5000
    long = P.movie(ENTRY, [bytes(4 * n)], sizes=[[4] * n], durations=[[1] * n])
    assert [(s, d, t) for _, s, d, t in runs(long)] == [(16384, 4096, 0), (4 * 904, 904, 4096)]
    same_runs_from_the_demuxer(long, runs(long))
    # and the byte cap: 1 MiB a run
    fat = P.movie(ENTRY, [bytes(3 * 400000)], sizes=[[400000] * 3], durations=[[1] * 3])
    assert [(s, d) for _, s, d, _ in runs(fat)] == [(800000, 2), (400000, 1)]


def test_trim_applies_to_a_run():
    data = P.movie(ENTRY, [bytes(4 * 6000)], sample_size=4, edit=[(60, 1000)], movie_timescale=600)  # 60 / 600 s = 4800 frames from frame 1000
    index = mp4.Mp4Index.from_file(data)
    assert [(d, t) for _, _, d, t in index.samples] == [(4096, 0), (1904, 4096)]
    assert index.trim(0, 4096, 48000) == (1000, 3096) and index.trim(1, 1904, 48000) == (0, 1704)


# ---- dfLa --------------------------------------------------------------------------------------------------------------------------------

def test_dfla_forms_and_refusals():
    info = bytes(range(34))
    stream = b"fLaC" + bytes([0x80, 0, 0, 34]) + info
    assert mp4.flac_config(bytes(4) + bytes([0x80, 0, 0, 34]) + info) == stream
    assert mp4.flac_config(info) == stream
    assert mp4.flac_config(stream + b"tail") == stream + b"tail"
    more = bytes(4) + bytes([0, 0, 0, 34]) + info + bytes([0x84, 0, 0, 2, 9, 9])  # a second block follows: kept
    assert mp4.flac_config(more) == b"fLaC" + more[4:]
    for bad, text in ((b"", "MP4 dfLa decoder configuration is truncated"), (bytes(3), "MP4 dfLa decoder configuration is truncated"),
                      (bytes(7), "MP4 dfLa has no leading FLAC STREAMINFO block"),
                      (bytes(4) + bytes([0x81, 0, 0, 34]) + info, "MP4 dfLa has no leading FLAC STREAMINFO block"),
                      (bytes(4) + bytes([0x80, 0, 0, 33]) + info, "MP4 dfLa has an invalid FLAC STREAMINFO block"),
                      (bytes(4) + bytes([0x80, 0, 1, 34]) + info + bytes(300), "MP4 dfLa has an invalid FLAC STREAMINFO block")):
        with pytest.raises(SoundkitError) as e:
            mp4.flac_config(bad)
        assert text in str(e.value), (bad, str(e.value))


@pytest.mark.parametrize("form", ["dfla", "bare", "stream"])
def test_flac_track_config_and_packets(form):
    data = open(os.path.join(FLAC, "A_Tusk_is_used_to_make_costly_gifts_16bit.flac"), "rb").read()
    file, frames, blocks, first = P.flac_in_mp4(data, form)
    index = mp4.Mp4Index.from_file(file)
    c = index.config
    assert (c.codec, c.sample_rate, c.channels, c.bits_per_sample, c.pcm) == ("flac", first["sample_rate"], first["channels"], first["bits_per_sample"], None)
    assert c.codec_private[:8] == b"fLaC" + bytes([0x80, 0, 0, 34]) and len(c.codec_private) == 42
    assert index.packet_bytes(file) == frames and [d for _, _, d, _ in index.samples] == blocks
    config, packets = demux(file, 4099)
    assert config.codec_private == c.codec_private and [p.data for p in packets] == frames
    broken = file.replace(b"dfLa", b"dfLx")  # no dfLa child: the reference's text for an empty configuration
    assert "MP4 dfLa decoder configuration is truncated" in refusal(broken)


# ---- fuzz --------------------------------------------------------------------------------------------------------------------------------

def test_mutated_moov_under_sanitizers(tmp_path):
    """tests/fuzz_container_pcm.cpp: csrc/mp4_stream.h alone with AddressSanitizer + UBSan on the CPU -- seeded mutations of the `moov` of
    two fixtures (rearranged so that the demuxer reads them too), of a built lpcm and a built fLaC file, through the index and the demuxer in
    ragged pieces, and of the header chunks of a PCM and an ALAC CAF file through csrc/caf_stream.h"""
    exe = str(tmp_path / "fuzz_container_pcm")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "fuzz_container_pcm.cpp")], cwd=HERE)
    files = {"s24be": B.faststart(open(os.path.join(MOV, "pcm-s24be.mov"), "rb").read()),
             "f64le": B.faststart(open(os.path.join(MOV, "pcm-f64le.mov"), "rb").read()),
             "lpcm": pcm_file(P.sound_entry(b"lpcm", 2, 2, 24, children=P.wave(P.enda(1))), 300, 6),
             "caf_s24le": open(os.path.join(HERE, "golden", "caf_pcm", "pcm-s24le.caf"), "rb").read(),
             "caf_alac": open(os.path.join(HERE, "golden", "alac", "A_Tusk_is_used_to_make_costly_gifts.caf"), "rb").read(),
             "flac": P.flac_in_mp4(open(os.path.join(FLAC, "A_Tusk_is_used_to_make_costly_gifts_24bit.flac"), "rb").read())[0]}
    paths = []
    for name, data in sorted(files.items()):
        paths.append(str(tmp_path / (name + ".bin")))
        with open(paths[-1], "wb") as f:
            f.write(data)
    out = subprocess.run([exe, "400"] + paths, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "fuzz_container_pcm ok" in out.stdout

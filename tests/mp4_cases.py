"""The MP4 files the CPU tests, the fuzz program and the GPU tests share: the five fixtures of tests/golden/mp4 and the builder's cases."""
import os

import mp4_builder as B
import mp4_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FIXTURES = ("mac_aac_A_Tusk.m4a", "alac_A_Tusk.m4a", "yt_itag_139_he_aac.mp4", "h264-high-aac.mp4", "h264-aac-fragmented.mp4")
MDAT_FIRST = "MP4 mdat appears before moov; use the seekable MP4 packet API"


def fixture(name):
    with open(os.path.join(GOLDEN, "mp4", name), "rb") as f:
        return f.read()


def golden(*path):
    with open(os.path.join(GOLDEN, *path), "rb") as f:
        return f.read()


def mac_aac_units():
    """(config, the 48 AAC-LC units) of the 16 kHz mono fixture"""
    track, packets = M.demux(fixture("mac_aac_A_Tusk.m4a"))
    return {"codec": "aac", "sample_rate": 16000, "channels": 1, "private": track["private"]}, [p for p, _, _ in packets]


def alac_units():
    track, packets = M.demux(fixture("alac_A_Tusk.m4a"))
    return {"codec": "alac", "sample_rate": 8000, "channels": 1, "bits": 16, "private": track["private"]}, [p for p, _, _ in packets], \
        [d for _, _, d in packets]


def filler_units(n, size=None):
    """bytes that are no audio: for cases only the demuxer sees"""
    return [bytes((7 * k + j) & 255 for j in range(size or 20 + (k * 37) % 90)) for k in range(n)]


def builder_cases():
    """name -> file bytes; every path of the demuxer the issue names"""
    aac, units = mac_aac_units()
    alac, packets, durations = alac_units()
    edit = [(2960 * 600 // 1000, 1024)]
    small = filler_units(23)
    return {
        "moov_first": B.regular(aac, units, edit=edit),
        "mdat_first": B.regular(aac, units, layout="mdat_first", edit=edit),
        "co64": B.regular(aac, small, co64=True),
        "wide_mdat": B.regular(aac, small, wide_mdat=True),
        "constant_stsz": B.regular(aac, filler_units(9, 64), constant=True),
        "per_chunk_5": B.regular(aac, small, per_chunk=5),
        "video_first": B.regular(aac, small, video=True, per_chunk=3),
        "junk": B.regular(aac, small, junk=True),
        "junk_mdat_first": B.regular(aac, small, layout="mdat_first", junk=True),
        "esds_long_lengths": B.regular(aac, small, length_bytes=4),
        "mvhd_v1_edit": B.regular(aac, small, mvhd_version=1, edit=[(100, -1), (600, 2048)]),
        "alac_moov_first": B.regular(alac, packets, durations=durations, edit=[(23680 * 600 // 8000, 0)]),
        "frag_one_per_trun": B.fragmented(aac, units, per_moof=7, per_trun=1),
        "frag_many_per_trun": B.fragmented(aac, units, per_moof=16),
        "frag_no_base_flag": B.fragmented(aac, small, per_moof=6, base="none"),
        "frag_explicit_base": B.fragmented(aac, small, per_moof=6, base="explicit"),
        "frag_video_moof_base": B.fragmented(aac, small, per_moof=5, video=True),
        "frag_video_inherited_base": B.fragmented(aac, small, per_moof=5, video=True, base="none", per_trun=2),
        "frag_defaults": B.fragmented(aac, filler_units(12, 40), per_moof=4, trex_defaults=True, tfdt_version=0, junk=True),
        "frag_alac": B.fragmented(alac, packets, durations=durations, per_moof=2),
    }

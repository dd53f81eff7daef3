"""The streams the Vorbis GPU tests share: the two fixtures and built streams (tests/vorbis_builder.py) at the smallest shapes at which
the kernels can still go wrong -- block sizes 64/128, 64/64, 256/2048 and 64/8192 (the FFT's smallest and largest size, one and several
rounds of its 256 lanes), 1, 2, 3 and 8 channels, residue types 0, 1 and 2, every floor multiplier, all four window transitions, and
beside the well-formed packets random bytes, truncated packets, an empty packet and packets whose audio bit is wrong."""
import os

import numpy as np

import vorbis_builder as B
import vorbis_model as M
import webm_vorbis

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "vorbis")
OGG = os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts.ogg")
RECORDING = os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts.decoded.wav")
WEBM = os.path.join(GOLDEN, "yt_itag_171_vorbis.webm")

# short / long sequence with every transition: S-S, S-L, L-L, L-S
FLAGS = [0, 0, 1, 1, 0, 1, 0]
BUILT = [
    # name, channels, block sizes, residue types (short, long), floor multipliers
    ("mono-64-128", 1, (64, 128), (1, 2), (2, 1)),
    ("stereo-64-64", 2, (64, 64), (0, 1), (3, 4)),
    ("three-256-2048", 3, (256, 2048), (2, 0), (1, 2)),
    ("eight-64-8192", 8, (64, 8192), (1, 2), (4, 3)),
    ("stereo-64-128-type2", 2, (64, 128), (2, 2), (2, 2)),
]


class Case:
    """name, the three headers, the model's setup, the audio packets"""

    def __init__(self, name, headers, packets):
        self.name, self.headers, self.packets = name, headers, packets
        self.ident = M.parse_ident(headers[0])
        self.setup = M.parse_setup(headers[2], self.ident["channels"], self.ident["blocksize_0"], self.ident["blocksize_1"])


_cache = {}


def fixture_cases():
    if "fixtures" not in _cache:
        pk = M.ogg_packets(open(OGG, "rb").read())
        hdr, packets = webm_vorbis.vorbis_track(open(WEBM, "rb").read())
        _cache["fixtures"] = [Case("ogg", [p["data"] for p in pk[:3]], [p["data"] for p in pk[3:]]), Case("webm", hdr, packets)]
    return _cache["fixtures"]


def built_cases():
    """well-formed packets only: FLAGS with matching window flags"""
    if "built" not in _cache:
        out = []
        for k, (name, ch, bs, rtype, mult) in enumerate(BUILT):
            s = B.default_setup(ch, bs[0], bs[1], rtype=rtype, multiplier=mult, seed=10 * k)
            rng = np.random.default_rng(100 + k)
            packets = [B.packet(rng, s, f, FLAGS[i - 1] if i else 0, FLAGS[i + 1] if i + 1 < len(FLAGS) else 0) for i, f in enumerate(FLAGS)]
            out.append(Case(name, [B.ident_header(ch, 16000, bs[0], bs[1]), B.comment_header(), B.setup_header(s)], packets))
        _cache["built"] = out
    return _cache["built"]


def damaged_packets(case, seed):
    """random bytes (the type bit as it falls), truncations of a good packet to 0, 1, 2, 3 and half its bytes, the audio bit wrong"""
    rng = np.random.default_rng(seed)
    good = case.packets[2]
    out = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(1, 120, 6)]
    out += [good[:n] for n in (0, 1, 2, 3, len(good) // 2)]
    out.append(bytes([good[0] | 1]) + good[1:])
    return out


def all_cases():
    return fixture_cases() + built_cases()


def model_pcm(case, dtype, packets=None):
    """-> [(status, [ch][frames] of dtype or None)] per packet, the overlap carried"""
    key = ("pcm", case.name, np.dtype(dtype).name)
    if packets is None and key in _cache:
        return _cache[key]
    st = M.Stream(case.setup, dtype)
    out = [st.decode(p) for p in (case.packets if packets is None else packets)]
    if packets is None:
        _cache[key] = out
    return out

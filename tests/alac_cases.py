"""The built Apple Lossless packets that tests/test_alac_cpu.py (model(builder(x)) == x) and tests/test_alac_decode_gpu.py (device ==
model) share.  Each case: (name, cfg, [(packet bytes, channels x n samples)]).  Built once per process."""
import functools

import numpy as np

import alac_builder as B


def signal(kind, n, depth, seed=0, channels=1):
    """channels lists of n signed samples of `depth` bits"""
    rng = np.random.RandomState(seed)
    top = (1 << (depth - 1)) - 1
    out = []
    for c in range(channels):
        t = np.arange(n, dtype=np.float64)
        if kind == "tone":  # a decaying two-tone with a little noise: what a predictor is for
            v = (0.3 * top * np.sin(t * (0.05 + 0.01 * c)) + 0.1 * top * np.sin(t * 0.31 + c)) * np.exp(-t / (n + 1.0)) + rng.randint(-3, 4, n)
        elif kind == "full":  # full scale, alternating sign: the coefficient walk runs its whole length, the 32-bit sums wrap
            v = np.where((np.arange(n) + c) % 2 == 0, top, -top - 1).astype(np.float64)
        elif kind == "rand":  # every value of the depth: escapes above 0xFFFF from 24 bits on
            v = rng.randint(-top - 1, top + 1, n, dtype=np.int64).astype(np.float64)
        elif kind == "loud":  # residuals just under the escape: the history stays high, k sits at the Rice limit
            v = rng.randint(-0x7FF0, 0x7FF0, n).astype(np.float64)
        elif kind == "silence":
            v = np.zeros(n)
        elif kind == "sparse":  # zeros with lone samples: runs of every length, a run of 1 among them
            v = np.zeros(n)
            at = np.cumsum(rng.randint(1, 40, n))
            at = at[at < n]
            v[at] = rng.randint(-9, 10, at.size)
            if n > 8:
                v[2], v[4] = 3, -2  # a run of exactly 1 between them
        elif kind == "tail":  # sound, then zeros to the very last sample
            v = np.zeros(n)
            v[:n // 3] = rng.randint(-50, 51, n // 3)
        else:
            raise ValueError(kind)
        out.append([int(x) for x in np.clip(np.rint(v), -top - 1, top).astype(np.int64)])
    return out


def _one(name, cfg, kind, n, seed=0, **kw):
    ch = signal(kind, n, cfg["bit_depth"], seed, cfg["channels"])
    return name, cfg, [(B.packet(cfg, ch, **kw), ch)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    m16, m24, m32 = (B.config(4096, d, 1, 44100) for d in (16, 24, 32))
    s16, s24, s32 = (B.config(4096, d, 2, 48000) for d in (16, 24, 32))
    for order in (0, 1, 4, 8, 30, 31):
        out.append(_one(f"order{order}", m16, "tone", 4096 if order == 4 else 700, order, order=order, shift=6))
        # where the predictor's warm-up branches end
        for n in sorted({1, 2, max(order, 1), order + 1, order + 2}):
            out.append(_one(f"order{order}_n{n}", m16, "rand", n, n, order=order, shift=5))
    for shift in range(1, 10):
        out.append(_one(f"shift{shift}", m16, "tone", 300, shift, order=4, shift=shift))
    for order in (0, 4, 31):
        out.append(_one(f"type15_order{order}", m16, "tone", 500, order, order=order, shift=6, ptype=15))
    out.append(_one("full16", m16, "full", 600, order=8, shift=9, coefs=[32767, -32768] * 4))
    out.append(_one("full24", m24, "full", 600, order=8, shift=1, coefs=[32767, -32768] * 4))
    out.append(_one("full24_order30", m24, "full", 400, order=30, shift=2, coefs=[32767] * 30))
    out.append(_one("rand16", m16, "rand", 600, order=4, shift=6))
    out.append(_one("rand24_escapes", m24, "rand", 600, order=0, shift=4))
    out.append(_one("rand32_escapes", m32, "rand", 300, order=2, shift=4))
    out.append(_one("loud24_k_at_kb", m24, "loud", 600, order=0, shift=4))
    out.append(_one("loud24_kb5", B.config(4096, 24, 1, 44100, kb=5), "loud", 300, order=0, shift=4))
    out.append(_one("pb_factor7", m16, "tone", 300, order=4, shift=6, pb_factor=7))
    out.append(_one("pb_factor0", m16, "tone", 300, order=4, shift=6, pb_factor=0))
    for kind in ("silence", "sparse", "tail"):
        out.append(_one(kind, m16, kind, 900, order=0, shift=4))
        out.append(_one(kind + "_order4", m16, kind, 900, order=4, shift=6))
    big = B.config(65536, 16, 1, 44100)
    out.append(_one("run_ffff", big, "silence", 65536, order=0, shift=4))  # one run of 0xFFFF that ends at the last sample
    for name, cfg in (("pair16", s16), ("pair24", s24)):
        for weight, shift in ((0, 0), (1, 2), (3, 2), (255, 8), (2, 40)):
            out.append(_one(f"{name}_mix{weight}_{shift}", cfg, "tone", 400, weight, order=4, shift=6, mix_weight=weight, mix_shift=shift))
        out.append(_one(f"{name}_rand", cfg, "rand", 400, 5, order=2, shift=6, mix_weight=1, mix_shift=2))  # odd sums, full range
    for name, cfg in (("mono24", m24), ("mono32", m32), ("pair24", s24), ("pair32", s32)):
        for extra in (1, 2):
            out.append(_one(f"{name}_extra{extra}", cfg, "rand", 333, extra, order=4, shift=6, extra_bytes=extra, mix_weight=1, mix_shift=2))
    out.append(_one("mono32_extra3", m32, "rand", 333, 3, order=4, shift=6, extra_bytes=3))
    out.append(_one("mono32", m32, "tone", 300, order=4, shift=6))
    for name, cfg in (("raw16", m16), ("raw24_pair", s24), ("raw32", m32)):
        out.append(_one(name, cfg, "rand", 200, raw=True))
    out.append(_one("dse", m16, "tone", 300, order=4, shift=6, dse=b"\x01\x02\x03\x04\x05"))
    out.append(_one("dse_long", m16, "tone", 300, order=4, shift=6, dse=bytes(range(256)) + b"xyz"))
    out.append(_one("fil", s16, "tone", 300, order=4, shift=6, fil=3))
    out.append(_one("fil_long", s16, "tone", 300, order=4, shift=6, fil=40))
    out.append(_one("dse_fil_first", m16, "tone", 300, order=4, shift=6, before=lambda w: (B.write_dse(w, b"ab", align=False), B.write_fil(w, 2))))
    out.append(_one("whole_frame", B.config(256, 16, 1, 8000), "tone", 256, order=4, shift=6))  # no size field
    out.append(_one("whole_frame_sized", B.config(256, 16, 1, 8000), "tone", 256, order=4, shift=6, has_size=True))
    for ch in range(1, 9):
        cfg = B.config(4096, 16 if ch % 2 else 24, ch, 48000)
        els = [B.Element(k, order=4, shift=6, mix_weight=1 if k == "cpe" else 0, mix_shift=2) for k in B.layout(ch, lfe=ch in (3, 5))]
        out.append(_one(f"channels{ch}", cfg, "tone", 301, ch, elements=els))
    out.append(_one("sce_sce", s16, "tone", 300, elements=[B.Element("sce", order=4, shift=6), B.Element("sce", order=8, shift=7)]))
    return out


@functools.lru_cache(maxsize=None)
def many():
    """130 packets of mixed lengths for one call: (cfg, [(packet, chans)])"""
    cfg = B.config(4096, 16, 2, 44100)
    rng = np.random.RandomState(7)
    out = []
    for i in range(130):
        n = int(rng.choice([1, 2, 5, 64, 65, 255, 256, 257, 600, 1024]))
        ch = signal(("tone", "sparse", "rand")[i % 3], n, 16, i, 2)
        out.append((B.packet(cfg, ch, order=(0, 4, 8, 31)[i % 4], shift=6, mix_weight=i % 3, mix_shift=2), ch))
    return cfg, out

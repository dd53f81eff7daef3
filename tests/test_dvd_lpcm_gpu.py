"""SK_AIFF_DVD_S24 on the GPU: DVD LPCM's 24-bit packing through Engine.aiff_decode bit for bit against tests/ps_model.py's
unpack_dvd_lpcm (the reference's, pinned by its known-answer group in tests/test_ps_cpu.py), at the sample counts on both sides of a
lane's 16 and a workgroup's 4096; and through tick_run_aiff on three streams of 1, 2 and 6 channels, as decoded and behind 48 -> 16 kHz
mono s16, where every stream equals the CPU chain on the model's PCM and does not depend on how the blocks are dealt out over ticks.

"Equals" is bit for bit wherever that can be had: the decode itself, the streams as decoded, and every deal against every other.
Behind the resampler it cannot: the CPU chain is the oracle's StreamingResampler, a restatement of rubato that accumulates each output
sample's 256 taps in one order in float, while the device's matrix-core resampler sums the same products tile by tile in another, so
the two f32 results differ in their last bits and a sample that lies on a rounding edge of the final s16 lands one step apart.  That
is the PCM tick's property, not this encoding's -- the decode in front of it is exact -- and the bound is the one the project holds
that same chain to everywhere (tests/test_pcm_pipeline_gpu.py lsb_check, tests/test_rate_pairs_gpu.py): at most one step, on at most
one sample in a hundred.  Measured here: one step on 0.04 to 0.14 % of 2820 samples."""
import numpy as np
import pytest

import pcm_worker_model as W
import ps_builder as B
import ps_model as M
import rate_pairs as R
import wide_pcm_model as WIDE
from soundkit_amd import SoundkitError
from soundkit_amd import engine as E
from test_pcm_pipeline_gpu import lsb_check

pytestmark = pytest.mark.gpu

KNOWN = bytes(range(12))
KNOWN_ANSWER = bytes([8, 1, 0, 9, 3, 2, 10, 5, 4, 11, 7, 6])


def test_the_known_answer_group(engine):
    assert M.unpack_dvd_lpcm(KNOWN, 24, 1) == KNOWN_ANSWER
    assert engine.aiff_decode(E.AIFF_DVD_S24, 1, KNOWN) == KNOWN_ANSWER


@pytest.mark.parametrize("samples", [4, 12, 16, 20, 4092, 4096, 4100, 8196])
def test_random_bytes_unpack_as_the_model_unpacks_them(engine, samples):
    packed = np.random.default_rng(samples).integers(0, 256, 3 * samples, dtype=np.uint8).tobytes()
    want = M.unpack_dvd_lpcm(packed, 24, 1)
    assert len(want) == 3 * samples
    for channels in (1, 2):  # the channel count plays no part in the permutation
        assert engine.aiff_decode(E.AIFF_DVD_S24, channels, packed) == want


def test_the_packer_round_trip(engine):
    pcm = B.widen(B.A.S16[:2 * 1028], 3, 24)
    assert engine.aiff_decode(E.AIFF_DVD_S24, 3, B.pack24(pcm)) == pcm


@pytest.mark.parametrize("n", [1, 11, 13, 24 + 6, 48 + 3])
def test_a_length_that_is_no_multiple_of_12_is_refused(engine, n):
    with pytest.raises(SoundkitError) as e:
        engine.aiff_decode(E.AIFF_DVD_S24, 2, bytes(n))
    assert e.value.status == -1
    with pytest.raises(SoundkitError) as e:
        engine.tick_run_aiff([{"encoding": E.AIFF_DVD_S24, "channels": 2, "out_bits": 24, "out_channels": 2, "n_units": 1}], [bytes(n)])
    assert e.value.status == -1


# ---- through the tick ------------------------------------------------------------------------------------------------------------------

FRAMES = [1000, 4096, 4, 3492]  # per unit: whole blocks at 1, 2 and 6 channels (4, 2 and 4 frames a block); 8592 frames: two chunks and a tail
CHANNELS = [1, 2, 6]


@pytest.fixture(scope="module")
def wide(engine):
    """an engine with wide slots for the 6-channel stream behind a conversion (the session's `engine` first: it stays the default)"""
    import soundkit_amd
    eng = soundkit_amd.Engine(0, 16)
    eng.enable_wide_pcm(4)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def streams():
    """per channel count: (packed units, the model's PCM per unit)"""
    out = []
    for ch in CHANNELS:
        pcm = R.encode(R.signal(48000, ch)[:, :sum(FRAMES)], W.FMT_S24LE)
        units = R.cut(pcm, 3 * ch, FRAMES)
        packed = [B.pack24(u) for u in units]
        unpacked = [M.unpack_dvd_lpcm(p, 24, ch) for p in packed]
        assert unpacked == units and all(len(p) % M.block_size(24, ch) == 0 for p in packed)
        out.append((packed, unpacked))
    return out


def run(engine, streams, convert, deals):
    """the three streams side by side over the ticks of `deals` (units per stream per tick), then a tick that takes what is left and
    flushes the resamplers -> per stream the records (bits, channels, is_float, bytes)"""
    entries, sids = [], []
    for ch in CHANNELS:
        entry = {"encoding": E.AIFF_DVD_S24, "channels": ch, "out_bits": 16 if convert else 24, "out_channels": 1 if convert else ch}
        sid = None
        if convert:
            sid = engine.open_stream(48000, ch)
            engine.resampler_open(sid, 48000, 16000)
            entry.update(stream=sid, resample=1)
        sids.append(sid)
        entries.append(entry)
    out, at = [[] for _ in CHANNELS], [0] * len(CHANNELS)
    try:
        for deal in list(deals) + [None]:
            units = []
            for i, entry in enumerate(entries):
                n = len(FRAMES) - at[i] if deal is None else deal[i]
                entry["n_units"], entry["flush"] = n, 1 if deal is None and convert else 0
                units += streams[i][0][at[i]:at[i] + n]
                at[i] += n
            for idx, status, frames, ch_o, bits_o, data, is_float in engine.tick_run_aiff(entries, units):
                assert status == 0 and len(data) == frames * ch_o * bits_o // 8
                out[idx].append((bits_o, ch_o, is_float, data))
    finally:
        for sid in sids:
            if sid is not None:
                engine.resampler_close(sid)
                engine.close_stream(sid)
    return out


DEALS = {"all at once": [[4, 4, 4]], "one unit a tick": [[1, 1, 1]] * 4, "uneven": [[2, 0, 1], [0, 3, 0], [1, 0, 2]]}


def test_as_decoded_every_unit_is_the_models_pcm(engine, streams):
    for name, deals in DEALS.items():
        got = run(engine, streams, False, deals)
        for k, ch in enumerate(CHANNELS):
            assert [r[:3] for r in got[k]] == [(24, ch, False)] * len(FRAMES), (name, ch)
            assert [r[3] for r in got[k]] == streams[k][1], (name, ch)


def test_behind_48_to_16_khz_mono_s16_every_stream_is_the_cpu_chain(wide, oracle, streams):
    got = {name: run(wide, streams, True, deals) for name, deals in DEALS.items()}
    for k, ch in enumerate(CHANNELS):
        stage = WIDE.WideOutputStage if ch > 2 else W.OutputStage
        want = R.cpu_chain(oracle, W.FMT_S24LE, 48000, ch, streams[k][1], 16, 16000, 1, stage=stage)
        assert R.structure(want) == [(16, 1, False, 2 * n) for n in R.chunk_counts(48000, 16000, sum(FRAMES))]
        mine = got["all at once"][k]
        assert R.structure(mine) == R.structure(want), ch
        a, b = b"".join(m[3] for m in mine), b"".join(w[3] for w in want)
        print("\ndvd_lpcm tick ch=%d worst=%d share=%.5f" % ((ch,) + R.lsb_share(a, b)))
        lsb_check(a, b, "DVD LPCM, %d channel(s), 48 -> 16 kHz mono" % ch)
        for name in DEALS:
            assert b"".join(m[3] for m in got[name][k]) == a, (name, ch)

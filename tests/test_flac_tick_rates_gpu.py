"""FLAC through the tick behind a resampler at every sample rate a frame header can name: one built stream per rate code of
flac_stream.h's table, each rate that sk_resampler_open takes on both sides going down to 16 and 8 kHz (8 -> 16 kHz goes up), 8, 16
and 24 kHz up to 48 kHz and 44.1 -> 48 kHz; depth, channel count and stereo assignment rotate through the streams.  Every stream must
give exactly what sk_tick_run_pcm gives for the same samples handed in as little-endian units, whichever way its frames are dealt out
over ticks.  The two header rates the resampler does not take are refused with their status.

The expected value here is another tick, which shares the resampler with this one.  What holds sk_tick_run_pcm itself to the CPU
chain at these 20 pairs, on streams of the same eight unit sizes -- every record's size exactly, every sample within one step -- is
tests/test_rate_pairs_gpu.py::test_pcm_tick_meets_the_cpu_chain_at_every_pair.

Every built stream is first decoded by the model (tests/flac_model.py) back to its source samples, on the CPU."""
import functools
import random

import pytest

import flac_builder as B
import flac_model as M

gpu = pytest.mark.gpu

KINDS = [{"type": "verbatim"}, {"type": "fixed", "order": 2, "params": "auto"},
         {"type": "lpc", "order": 4, "precision": 12, "shift": 11, "coefs": [2000, -900, 300, -50], "params": "auto"}]
HEADER_RATES = [88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000]  # rate codes 1 ... 11
REFUSED = [176400, 192000]                                                                     # not among the resampler's rates
# 8594 frames: two resampler chunks of 4096 and a tail for the flush; the last block is one sample
SIZES = [1152, 4096, 17, 576, 2304, 192, 256, 1]
# rate -> (channels, bits, stereo assignment, out_bits, out_channels)
SHAPES = {88200: (2, 16, 10, 16, 1), 8000: (1, 16, None, 16, 1), 16000: (2, 24, 10, 16, 2), 22050: (1, 24, None, 16, 1),
          24000: (2, 16, 8, 16, 2), 32000: (1, 16, None, 24, 1), 44100: (2, 24, 10, 16, 1), 48000: (1, 24, None, 16, 1),
          96000: (2, 16, 9, 16, 1), 176400: (1, 16, None, 16, 1), 192000: (2, 24, 10, 16, 1)}
PAIRS = [(r, out) for r in HEADER_RATES if r not in REFUSED for out in (16000, 8000) if r != out] + \
        [(8000, 48000), (16000, 48000), (24000, 48000), (44100, 48000)]
DEALS = {"all at once": lambda i: [8],
         "one frame a tick": lambda i: [1] * 8,
         "uneven": lambda i: [[3, 0, 0, 4, 1], [0, 1, 6, 0, 1], [1, 5, 0, 0, 2]][i % 3]}  # ticks in which a stream has nothing


def checked_frames(data, blocks):
    """the frames of a built stream as the product's reader cuts them, after the model has decoded each back to its source block"""
    from soundkit_amd import flac
    r = flac.FlacReader()
    frames = r.add(data) + r.add(b"")
    r.close()
    assert len(frames) == len(blocks)
    for (d, raw), ch in zip(frames, blocks):
        h, got = M.decode_frame(raw)
        assert got == ch and (h["block_size"], h["channels"], d["block_size"], d["channels"]) == (len(ch[0]), len(ch)) * 2
    return frames


@functools.lru_cache(maxsize=None)
def built(rate):
    """-> ([(frame dict, frame bytes)], [contract bytes per frame]) of the stream at this header rate"""
    nch, bits, assignment = SHAPES[rate][:3]
    rng = random.Random(rate)
    lim = int((1 << (bits - 1)) * 0.7)
    blocks = [[[rng.randrange(-lim, lim) for _ in range(n)] for _ in range(nch)] for n in SIZES]
    data, _ = B.stream(blocks, bits, rate, lambda i, ch: [KINDS[(i + c) % 3 if len(ch[0]) >= 4 else 0] for c in range(len(ch))], assignment=assignment)
    frames = checked_frames(data, blocks)
    assert all(d["sample_rate"] == rate and d["bits_per_sample"] == bits for d, _ in frames)
    return frames, [M.contract_bytes({"bits_per_sample": bits, "block_size": len(ch[0])}, ch) for ch in blocks]


def test_every_built_stream_decodes_in_the_model_to_its_source():
    assert len(HEADER_RATES) == 11 and len(PAIRS) == 20
    for rate in HEADER_RATES:
        frames, pcm = built(rate)
        nch, bits = SHAPES[rate][:2]
        assert [d["block_size"] for d, _ in frames] == SIZES and sum(len(p) for p in pcm) == sum(SIZES) * nch * M.width(bits)


@gpu
def test_rate_changes_at_every_header_rate_meet_the_pcm_tick_however_the_frames_are_dealt_out(engine):
    from test_flac_tick_gpu import pcm_fmt, resampled
    flac_streams, pcm_streams, flac_units, pcm_units = [], [], [], []
    for rate, out_rate in PAIRS:
        nch, bits, _, out_bits, out_ch = SHAPES[rate]
        frames, pcm = built(rate)
        head = {"rate": rate, "out_rate": out_rate, "channels": nch}
        flac_streams.append(dict(head, entry={"channels": nch, "bits_per_sample": bits, "out_bits": out_bits, "out_channels": out_ch}))
        pcm_streams.append(dict(head, entry={"channels": nch, "format": pcm_fmt(bits), "out_bits": out_bits, "out_channels": out_ch}))
        flac_units.append(frames)
        pcm_units.append(pcm)

    def deal(of):
        per = [of(i) for i in range(len(PAIRS))]
        assert all(sum(p) == 8 for p in per)
        ticks = max(len(p) for p in per)
        return [[p[t] if t < len(p) else 0 for p in per] for t in range(ticks)]

    want = resampled(engine, "pcm", pcm_streams, pcm_units, deal(DEALS["all at once"]))
    for k, (rate, out_rate) in enumerate(PAIRS):  # the output is there: about frames * out_rate / rate of it, less the filter's delay
        frame_out = SHAPES[rate][3] // 8 * SHAPES[rate][4]
        assert len(want[k]) % frame_out == 0
        assert 0.9 * sum(SIZES) * out_rate / rate < len(want[k]) // frame_out < 1.1 * sum(SIZES) * out_rate / rate + 300, (rate, out_rate)
        assert any(want[k])
    for name, of in DEALS.items():
        got = resampled(engine, "flac", flac_streams, flac_units, deal(of))
        for k, pair in enumerate(PAIRS):
            assert got[k] == want[k], (name, pair)


@gpu
def test_header_rates_the_resampler_does_not_take_are_refused(engine):
    import soundkit_amd
    for rate in REFUSED:
        frames, pcm = built(rate)
        nch, bits = SHAPES[rate][:2]
        sid = engine.open_stream(rate, nch)
        try:
            for out_rate in (16000, 8000):
                with pytest.raises(soundkit_amd.SoundkitError) as exc:
                    engine.resampler_open(sid, rate, out_rate)
                assert exc.value.status == -6
            # ... and the tick refuses a stream that asks for a resampler it does not have; as decoded, the stream still delivers
            entry = {"channels": nch, "bits_per_sample": bits, "out_bits": 16, "out_channels": 1, "n_units": len(frames)}
            with pytest.raises(soundkit_amd.SoundkitError) as exc:
                engine.tick_run_flac([dict(entry, stream=sid, resample=1)], frames)
            assert exc.value.status == -5
        finally:
            engine.close_stream(sid)
        recs, status = engine.tick_run_flac([dict(entry, out_bits=8 * M.width(bits), out_channels=nch)], frames)
        assert not any(status) and [r[5] for r in recs] == pcm

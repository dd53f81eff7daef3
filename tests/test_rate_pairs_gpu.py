"""The streaming resampler -- rs_process_ready / rs_run_rounds, the 48 -> 16 kHz FIR and the generic sinc kernels with a time-index
set per chunk -- held to the CPU chain (oracle.StreamingResampler, restated rubato) at every one of the 20 rate pairs of
test_flac_tick_rates_gpu.PAIRS, through the entry itself and through every tick that ends in it.  The other tick tests compare a
tick with another tick or with the one-stream path, which share that code; here every expected sample comes from the CPU.

1. sk_resampler_process_f32 / _flush_f32, mono and stereo, every pair: the output count of every call is the CPU chain's, the samples
   within 1e-6 relative RMS and 4e-6 of full scale (the float tolerance test_fir_gpu.py holds this entry to at its five pairs);
   nine streams 0 ... 8 chunks into their walk in one call at the steepest ratio and at the largest up-sampling one.
2. sk_tick_run_pcm, a mono s16 and a stereo s24 -> mono stream per pair, all 40 in the same ticks: the records of
   pcm_worker_model.OutputStage in count, order and size; the samples within one step on at most 1 % (lsb_check); two ways of
   dealing the units out give the same bytes.
3. float, 24-bit and 32-bit outputs behind a rate change at four pairs: the float tolerance, plus one step of the output width for
   the integers' final rounding.
4. sk_tick_run (AAC) at every rate of the AAC table the resampler takes, to 16 kHz mono, 8 kHz and 48 kHz, against oracle synthesis
   -> s16 -> / 32768 -> oracle.StreamingResampler -> downmix -> s16, on the fixture's first twelve access units (all but silent:
   they pin the records) and on twelve loud ones (they pin the samples); the four AAC rates it does not take are refused.
5. 3-, 6- and 8-channel rows (an engine with the pool of wide streams): the records and samples of wide_pcm_model.WideOutputStage;
   a silent channel stays silent.

Checked once against a copy of the reference whose 22.05 -> 16 kHz sub-filters were scaled by 1 + 1e-4: parts 1, 2, 4 (the loud units)
and 5 fail at that pair and nowhere else, while test_flac_tick_rates_gpu.py, whose expected value is another tick, cannot see it.
Measured on MI355X: profiles/rate_pairs.md.  The signal and the expected records: tests/rate_pairs.py; the CPU chain's own distance
from float64 on this signal: tests/test_rate_pairs_cpu.py."""
import functools

import numpy as np
import pytest

import pcm_worker_model as M
import rate_pairs as R
import wide_pcm_model as W
from soundkit_amd import decoder
from soundkit_amd.engine import make_descs
from test_pcm_pipeline_gpu import lsb_check, run_pcm_ticks
from test_tick_gpu import parsed, run_ticks

pytestmark = pytest.mark.gpu

RMS_BOUND, ABS_BOUND = 1e-6, 4e-6  # the project's float tolerance for this entry (test_fir_gpu.py)


def float_check(got, want, what, lsb=0.0):
    """relative RMS and largest difference of full scale 1 within the float tolerance, plus `lsb` for a final rounding to integers"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and want.size, (what, got.shape, want.shape)
    rms_d, rms_w, worst = float(np.sqrt(np.mean((got - want) ** 2))), float(np.sqrt(np.mean(want ** 2))), float(np.abs(got - want).max())
    print("\nrate_pairs %s rel_rms=%.3e max=%.3e" % (what, rms_d / rms_w, worst))
    assert rms_w > 0.05, what  # there is a signal
    assert rms_d < RMS_BOUND * rms_w + lsb and worst < ABS_BOUND + lsb, (what, rms_d / rms_w, worst)


# ---- 1. the streaming entry -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", R.PAIRS, ids=R.label)
def test_streaming_entry_meets_the_cpu_chain(engine, oracle, pair):
    in_hz, out_hz = pair
    for ch in (1, 2):
        x = R.signal(in_hz, ch).astype(np.float32)
        ours = decoder.StreamingResampler(in_hz, out_hz, ch, engine)
        ref = oracle.StreamingResampler(in_hz, out_hz, ch)
        got, want, pos = [], [], 0
        for size in R.BLOCKS + [R.FRAMES - sum(R.BLOCKS)]:
            blk = x[:, pos:pos + size]
            pos += size
            a, b = ours.process(blk), ref.process(blk)
            assert a.shape == b.shape, (ch, size, a.shape, b.shape)
            got.append(a), want.append(b)
        assert pos == R.FRAMES
        a, b = ours.flush(), ref.flush()
        ours.close()
        assert a.shape == b.shape and a.shape[1] > 0, (ch, a.shape, b.shape)
        got.append(a), want.append(b)
        assert [w.shape[1] for w in want if w.shape[1]] == [n for n in R.chunk_counts(in_hz, out_hz)]
        float_check(np.concatenate(got, 1), np.concatenate(want, 1), "part1 %d %d ch=%d" % (in_hz, out_hz, ch))


@pytest.mark.parametrize("pair", [(96000, 8000), (8000, 48000)], ids=R.label)
def test_streams_of_different_ages_at_the_steep_and_the_upsampling_ratio(engine, oracle, pair):
    """test_fir_gpu.py::test_streams_of_different_ages_share_a_launch's shape at the two ratios it has not seen: nine mono streams,
    stream k being k chunks (and a bit) into its walk of the time index, served by one call with one index set per row"""
    in_hz, out_hz = pair
    rng = np.random.default_rng(in_hz + out_hz)
    n = 9
    sids = [engine.open_stream(in_hz, 1) for _ in range(n)]
    refs = [oracle.StreamingResampler(in_hz, out_hz, 1) for _ in range(n)]
    try:
        for sid in sids:
            engine.resampler_open(sid, in_hz, out_hz)
        for k in range(1, n):
            pre = (0.7 * rng.uniform(-1, 1, (1, 4096 * k + 100 * k))).astype(np.float32)
            a, b = engine.resampler_process([sids[k]], pre[None], 1)[0], refs[k].process(pre)
            assert a.shape == b.shape, (k, a.shape, b.shape)
        got, want = [[] for _ in range(n)], [[] for _ in range(n)]
        for frames in (4096, 9000, 1234):
            data = (0.7 * rng.uniform(-1, 1, (n, 1, frames))).astype(np.float32)
            outs = engine.resampler_process(sids, data, 1)
            for k in range(n):
                w = refs[k].process(data[k])
                assert outs[k].shape == w.shape, (k, frames, outs[k].shape, w.shape)
                got[k].append(outs[k]), want[k].append(w)
        outs = engine.resampler_flush(sids, 1)
        for k in range(n):
            w = refs[k].flush()
            assert outs[k].shape == w.shape, (k, outs[k].shape, w.shape)
            got[k].append(outs[k]), want[k].append(w)
        assert len({sum(w.shape[1] for w in want[k]) for k in range(n)}) > 1  # the streams really are at different places
        float_check(np.concatenate([np.concatenate(g, 1) for g in got], 1), np.concatenate([np.concatenate(w, 1) for w in want], 1),
                    "part1-ages %d %d" % pair)
        for k in range(n):
            assert np.abs(np.concatenate(got[k], 1) - np.concatenate(want[k], 1)).max() < ABS_BOUND, k
    finally:
        for sid in sids:
            engine.close_stream(sid)


# ---- 2. the PCM tick, one and two channels ------------------------------------------------------------------------------------------------

def test_pcm_tick_meets_the_cpu_chain_at_every_pair(engine, oracle):
    specs = R.pcm_specs()
    assert len(specs) == 40
    deals = {"all at once": run_pcm_ticks(engine, specs, [len(R.UNITS)] * len(specs)),
             "one unit a tick": run_pcm_ticks(engine, specs, [1] * len(specs))}
    for k, spec in enumerate(specs):
        want = R.cpu_chain(oracle, *spec)
        what = "%d %d ch=%d" % (spec[1], spec[5], spec[2])
        assert len(want) == 3
        for name, got in deals.items():
            assert R.structure(got[k]) == R.structure(want), (name, what, R.structure(got[k]), R.structure(want))
        mine = b"".join(m[3] for m in deals["all at once"][k])
        print("\nrate_pairs part2 %s worst=%d share=%.5f" % ((what,) + R.lsb_share(mine, b"".join(w[3] for w in want))))
        lsb_check(mine, b"".join(w[3] for w in want), "PCM tick " + what)
        assert [m[3] for m in deals["one unit a tick"][k]] == [m[3] for m in deals["all at once"][k]], what


# ---- 3. outputs wider than 16 bits ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", [(48000, 16000), (44100, 16000), (96000, 8000), (8000, 48000)], ids=R.label)
def test_wider_outputs_behind_a_rate_change(engine, oracle, pair):
    """a float source to float (mono), 24-bit stereo to 24 bits (both channels kept), 32-bit stereo to 32-bit mono"""
    rate, out_rate = pair
    kinds = [(M.FMT_F32LE, 1, 32, 1), (M.FMT_S24LE, 2, 24, 2), (M.FMT_S32LE, 2, 32, 1)]
    specs = [(fmt, rate, ch, list(R.source_units(rate, ch, fmt)), bits, out_rate, out_ch) for fmt, ch, bits, out_ch in kinds]
    got = run_pcm_ticks(engine, specs, [3, 8, 1])
    for spec, mine in zip(specs, got):
        fmt, bits, out_ch = spec[0], spec[4], spec[6]
        want = R.cpu_chain(oracle, *spec)
        is_float = fmt == M.FMT_F32LE
        assert len(want) == 3 and all(w[:3] == (bits, out_ch, is_float) for w in want)
        assert R.structure(mine) == R.structure(want), (pair, fmt, R.structure(mine), R.structure(want))
        float_check(np.concatenate([R.as_floats(m) for m in mine]), np.concatenate([R.as_floats(w) for w in want]),
                    "part3 %d %d %s" % (rate, out_rate, "f32" if is_float else "s%d" % bits), lsb=0.0 if is_float else 2.0 ** -(bits - 1))


# ---- 4. the AAC tick ------------------------------------------------------------------------------------------------------------------------

AAC_UNITS = 12  # 12 288 frames: three resampler chunks
AAC_RATES = [96000, 88200, 48000, 44100, 32000, 24000, 22050, 16000, 8000]  # the AAC table's rates that are common rates
AAC_NOT_COMMON = [64000, 12000, 11025, 7350]                                # ... and the four that are not
# The fixture's first twelve access units are all but silent (at most 8 steps of s16), and its loudest reach 1180 steps: at that level
# a resampler whose gain is off by 1e-4 moves no sample by a whole step.  So beside the first twelve units as parsed() gives them,
# which pin the records, units 24 ... 35 run with their spectra scaled by 16 (a power of two: the synthesis is linear, the oracle
# synthesises the same scaled spectra): peaks near 19 000 steps, where such an error moves every fifth sample.
AAC_SPANS = {"first": (0, 1.0), "loud": (24, 16.0)}


@functools.lru_cache(maxsize=None)
def aac_units(span):
    rate, ch, frames = parsed("aac-stereo-48k.adts")
    assert (rate, ch) == (48000, 2)
    first, gain = AAC_SPANS[span]
    return [(c * np.float32(gain), seqs, shapes) for c, seqs, shapes in frames[first:first + AAC_UNITS]]


_synth = {}


def oracle_s16_frames(oracle, span):
    """the units' PCM as the worker hands it to the resampler: oracle synthesis -> float_sample_to_i16 -> / 32768, [unit][2][1024] f32"""
    if span not in _synth:
        chans = [oracle.Channel() for _ in range(2)]
        out = []
        for coeffs, seqs, shapes in aac_units(span):
            pcm, _ = oracle.synthesize_stream(coeffs[None], [seqs], [shapes], chans)
            out.append(oracle.planar_f32_to_s16_interleaved(pcm[0]).reshape(1024, 2).T.astype(np.float32) / np.float32(32768.0))
        peak = max(float(np.abs(q).max()) for q in out)
        assert peak < 0.999 and (span != "loud" or peak > 0.4), (span, peak)  # nothing clips; the loud span is loud
        _synth[span] = out
    return _synth[span]


def aac_cpu_chain(oracle, span, rate, out_rate, out_ch):
    rs = oracle.StreamingResampler(rate, out_rate, 2)
    chunks = [rs.process(q) for q in oracle_s16_frames(oracle, span)] + [rs.flush()]
    want = []
    for w in chunks:
        if w.shape[1]:
            want.append(oracle.planar_f32_to_s16_interleaved(oracle.downmix_mono(w)[None] if out_ch == 1 else w).tobytes())
    return want


@pytest.mark.parametrize("span", list(AAC_SPANS))
@pytest.mark.parametrize("out_rate,out_ch", [(16000, 1), (8000, 2), (48000, 1)])
def test_aac_tick_meets_the_cpu_chain_at_every_rate(engine, oracle, out_rate, out_ch, span):
    """the synthesis does not look at the rate: twelve access units of the 48 kHz fixture on a stream opened at R, 5 units a tick"""
    rates = [r for r in AAC_RATES if r != out_rate] if out_rate != 48000 else [8000, 16000, 24000]
    assert all((r, out_rate) in R.PAIRS for r in rates) and len(rates) == (3 if out_rate == 48000 else 8)
    specs = [(r, 2, aac_units(span), 16, out_rate, out_ch) for r in rates]
    got = run_ticks(engine, specs, [5] * len(specs))
    for r, mine in zip(rates, got):
        want = aac_cpu_chain(oracle, span, r, out_rate, out_ch)
        counts = R.chunk_counts(r, out_rate, AAC_UNITS * 1024)
        assert [len(w) for w in want] == [2 * out_ch * n for n in counts] and len(counts) == 4  # three chunks and the flush
        assert [(b, c, len(d)) for b, c, d in mine] == [(16, out_ch, len(w)) for w in want], (r, out_rate)
        what = "%s %d %d" % (span, r, out_rate)
        print("\nrate_pairs part4 %s worst=%d share=%.5f" % ((what,) + R.lsb_share(b"".join(m[2] for m in mine), b"".join(want))))
        lsb_check(b"".join(m[2] for m in mine), b"".join(want), "AAC tick " + what)


def test_aac_rates_the_resampler_does_not_take_are_refused(engine):
    """test_flac_tick_rates_gpu.py::test_header_rates_the_resampler_does_not_take_are_refused for the AAC tick: sk_resampler_open
    returns SK_ERR_UNSUPPORTED, a tick that asks for the resampler the stream does not have is refused as a whole
    (SK_ERR_BAD_STREAM), and as decoded the stream delivers what it delivers at 48 kHz"""
    import soundkit_amd
    units = aac_units("loud")
    at_48k = run_ticks(engine, [(48000, 2, units, 16, None, None)], [5])[0]
    assert len(at_48k) == AAC_UNITS and all(len(d) == 4096 and any(d) for _, _, d in at_48k)
    for rate in AAC_NOT_COMMON:
        sid = engine.open_stream(rate, 2)
        try:
            for out_rate in (16000, 8000, 48000):
                with pytest.raises(soundkit_amd.SoundkitError) as exc:
                    engine.resampler_open(sid, rate, out_rate)
                assert exc.value.status == -6
            c, seqs, shapes = units[0]
            descs, n = make_descs([(sid, 2, list(seqs), list(shapes))])
            with pytest.raises(soundkit_amd.SoundkitError) as exc:
                engine.tick_run([{"stream": sid, "n_frames": 1, "out_bits": 16, "out_channels": 1, "resample": 1}], descs, n, c.ravel())
            assert exc.value.status == -5
        finally:
            engine.close_stream(sid)
        assert run_ticks(engine, [(rate, 2, units, 16, None, None)], [5])[0] == at_48k, rate


# ---- 5. wide rows ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wide(engine):
    """an engine with 8 wide slots (the session's `engine` first: the decoder mirrors' default stays that one)"""
    import soundkit_amd
    eng = soundkit_amd.Engine(0, 16)
    eng.enable_wide_pcm(8)
    yield eng
    eng.close()


@pytest.mark.parametrize("C,pair", [(6, (16000, 48000)), (6, (22050, 16000)), (6, (96000, 8000)), (3, (8000, 16000)), (8, (8000, 16000))],
                         ids=lambda v: R.label(v) if isinstance(v, tuple) else "%d ch" % v)
def test_wide_rows_meet_the_cpu_chain(wide, oracle, C, pair):
    """every channel its own seed, channel C // 2 silent; all channels kept (the silent one stays silent), and the mono downmix"""
    rate, out_rate = pair
    silent = C // 2
    units = list(R.source_units(rate, C, M.FMT_S16LE, silent))
    specs = [(M.FMT_S16LE, rate, C, units, 16, out_rate, C), (M.FMT_S16LE, rate, C, units, 16, out_rate, 1)]
    got = run_pcm_ticks(wide, specs, [3, 8])
    for spec, mine in zip(specs, got):
        want = R.cpu_chain(oracle, *spec, stage=W.WideOutputStage)
        out_ch = spec[6]
        assert R.structure(want) == [(16, out_ch, False, 2 * out_ch * n) for n in R.chunk_counts(rate, out_rate)]
        assert R.structure(mine) == R.structure(want), (C, pair, out_ch, R.structure(mine), R.structure(want))
        a, b = b"".join(m[3] for m in mine), b"".join(w[3] for w in want)
        print("\nrate_pairs part5 %d %d ch=%d->%d worst=%d share=%.5f" % ((rate, out_rate, C, out_ch) + R.lsb_share(a, b)))
        lsb_check(a, b, "%d ch -> %d, %s" % (C, out_ch, R.label(pair)))
        if out_ch == C:
            rows = np.frombuffer(a, "<i2").reshape(-1, C)
            assert not rows[:, silent].any()
            assert all(rows[:, c].any() for c in range(C) if c != silent)

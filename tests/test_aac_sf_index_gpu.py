"""AAC-LC at all 13 sampling-frequency indices on the GPU, on the units of tests/aac_index_cases.py (the oracle's results are computed
once per process there; test_aac_sf_index_cpu.py holds the same units to the host front end and the tables to their gates).

The device finds the index from the stream's rate by a table of its own (sf_index_of, csrc/engine.cpp) and reads the band offsets
through the per-index slots of sk_ec::host_tables() copied to LDS; the other GPU tests run indices 0, 3, 4, 6, 8 and 11 only.

1. Engine.entropy_decode: all 26 (index, channels) streams in one call that takes the first half of every stream, a second call for the
   rest -- spectra, sequence and shape bit for bit the oracle's; the units with max_sfb one past the table, last in streams of their
   own, give the oracle's error kind and zero spectra.
2. the same through the quantised hand-over, AacLcFrontEnd.parse_q + Engine.expand_q_decode.
3. the tick three ways (host front end, GPU front end, quantised hand-over) per index: byte-identical AudioData, as decoded and to
   16 kHz mono at the eight common rates other than 16 kHz.
4. one scheduler round of thirteen streams, one per index, with gpu_entropy 0, 1 and 2: the records of the host-mode tick; to
   16 kHz mono the four rates the resampler does not take end with the reference's error and disturb nobody.  (They did: the failed
   pass left a row in the tick that asked for a resampler, and the tick refused every stream in it; the last test holds the fix for
   the ADTS, Layer III and Layer I / II framers alike.)
Every comparison is equality."""
import os
import time

import numpy as np
import pytest

import aac_index_cases as A
import rate_pairs as R
from oracle import aac_frontend as OF
from soundkit_amd import aac_lc, pipeline
from soundkit_amd._lib import ERR_NAMES
from test_entropy_gpu import run
from test_scheduler_gpu import as_tuples

pytestmark = pytest.mark.gpu

HALF = A.ACCEPTED // 2
COMMON_TO_16K = [96000, 88200, 48000, 44100, 32000, 24000, 22050, 8000]   # the AAC rates the resampler takes to 16 kHz
NOT_COMMON = [64000, 12000, 11025, 7350]
assert sorted(COMMON_TO_16K + NOT_COMMON + [16000]) == sorted(OF.RATES)
RESAMPLER_ERROR = "Decoding failed: Failed to create resampler: unsupported rate pair"


def all_streams():
    return [s for sf_index in A.INDICES for s in A.cases(sf_index).values()]


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def check_unit(got, want, what):
    status, coeffs, seq, shape = got
    assert status == 0, (what, status, ERR_NAMES.get(status))
    assert (seq, shape) == (want[1], want[2]), what
    assert same_bits(coeffs, want[0]), (what, int((coeffs.view(np.uint32) != want[0].view(np.uint32)).sum()))


# ---- 1. the GPU front end -------------------------------------------------------------------------------------------------------------

def test_gpu_front_end_equals_oracle_at_every_index(engine):
    streams = all_streams()
    assert len(streams) == 26
    sids = [engine.open_stream(OF.RATES[s.sf_index], s.channels) for s in streams]
    try:
        compared = 0
        for first, last in ((0, HALF), (HALF, A.ACCEPTED)):
            got = engine.entropy_decode([(sid, last - first) for sid in sids], [au for s in streams for au in s.units[first:last]])
            assert len(got) == 26 * (last - first)
            pos = 0
            for s in streams:
                for k in range(first, last):
                    check_unit(got[pos], s.want[k], (s.sf_index, s.channels, k, s.label[k]))
                    pos += 1
                    compared += 1
        assert compared == 26 * A.ACCEPTED
    finally:
        for sid in sids:
            engine.close_stream(sid)


def over_streams():
    out = [(s, o) for s in all_streams() for o in s.over]
    assert len(out) == 2 * (6 * 2 + 7 * 1)    # long at every index, short where the table has fewer than 15 bands; mono and stereo
    return out


def test_gpu_front_end_refuses_a_band_past_the_table(engine):
    """every stream is [an accepted unit, the unit with max_sfb one past the table], all in one call"""
    overs = over_streams()
    sids = [engine.open_stream(OF.RATES[s.sf_index], s.channels) for s, _ in overs]
    try:
        got = engine.entropy_decode([(sid, 2) for sid in sids], [au for _, (_, first, _, over, _) in overs for au in (first, over)])
        assert len(got) == 2 * len(overs)
        for n, (s, (name, first, first_want, over, err)) in enumerate(overs):
            what = (s.sf_index, s.channels, name)
            check_unit(got[2 * n], first_want, what)
            status, coeffs, _, _ = got[2 * n + 1]
            assert status != 0 and ERR_NAMES[status] == err.kind == "InvalidConfig", (what, status, ERR_NAMES.get(status))
            assert not coeffs.any(), what
    finally:
        for sid in sids:
            engine.close_stream(sid)


# ---- 2. the quantised hand-over ---------------------------------------------------------------------------------------------------------

def test_quantised_hand_over_equals_oracle_at_every_index(engine):
    streams = all_streams()
    sids = [engine.open_stream(OF.RATES[s.sf_index], s.channels) for s in streams]
    fes = [aac_lc.AacLcFrontEnd(s.asc) for s in streams]
    try:
        compared = 0
        for first, last in ((0, HALF), (HALF, A.ACCEPTED)):
            parsed = [fe.parse_q(au) for s, fe in zip(streams, fes) for au in s.units[first:last]]   # the host half accepts them all
            got = engine.expand_q_decode([(sid, last - first) for sid in sids], parsed)
            assert len(got) == 26 * (last - first)
            pos = 0
            for s in streams:
                for k in range(first, last):
                    check_unit(got[pos], s.want[k], (s.sf_index, s.channels, k, s.label[k]))
                    pos += 1
                    compared += 1
        assert compared == 26 * A.ACCEPTED
    finally:
        for sid in sids:
            engine.close_stream(sid)


def test_quantised_hand_over_refuses_a_band_past_the_table(engine):
    """the two halves together give the oracle's verdict: the host half (parse_q) refuses what fails up to the spectral data, with the
    oracle's kind and text; what it lets through, the device half refuses with the oracle's kind and zero spectra"""
    overs = over_streams()
    table, parsed, owners, host_refused = [], [], [], 0
    sids = [engine.open_stream(OF.RATES[s.sf_index], s.channels) for s, _ in overs]
    try:
        for n, (s, (name, first, first_want, over, err)) in enumerate(overs):
            fe = aac_lc.AacLcFrontEnd(s.asc)
            mine = [fe.parse_q(first)]
            try:
                mine.append(fe.parse_q(over))
            except aac_lc.AacLcError as e:
                assert e.kind == err.kind and str(e) == "%s: %s" % (err.kind, err), (s.sf_index, s.channels, name, str(e))
                host_refused += 1
            table.append((sids[n], len(mine)))
            parsed += mine
            owners += [(n, j) for j in range(len(mine))]
        got = engine.expand_q_decode(table, parsed)
        assert len(got) == len(owners)
        device_refused = 0
        for (n, j), g in zip(owners, got):
            s, (name, first, first_want, over, err) = overs[n]
            if j == 0:
                check_unit(g, first_want, (s.sf_index, s.channels, name))
            else:
                assert g[0] != 0 and ERR_NAMES[g[0]] == err.kind and not g[1].any(), (s.sf_index, s.channels, name, g[0])
                device_refused += 1
        assert host_refused + device_refused == len(overs)
    finally:
        for sid in sids:
            engine.close_stream(sid)


# ---- 3. the tick, three ways ------------------------------------------------------------------------------------------------------------

PER_TICK = [5, 3]
_host_ticks = {}


def specs_of(sf_index, options):
    bits, rate, ch = options
    return [(aac_lc.AacLcFrontEnd(s.asc), s.units, bits, rate, ch) for s in A.cases(sf_index).values()]


def host_tick(engine, sf_index, options):
    """the host-mode tick's records of the index's mono and stereo stream, [(bits, channels, bytes)] each; computed once"""
    key = (sf_index, options)
    if key not in _host_ticks:
        _host_ticks[key] = run(engine, "host", specs_of(sf_index, options), PER_TICK)
    return _host_ticks[key]


def expected_sizes(sf_index, channels, options):
    """the records a stream of 44 units gives: one per unit as decoded, one per 4096-frame chunk and the flush behind a rate change"""
    bits, rate, ch = options
    out_ch = ch or channels
    if rate and rate != OF.RATES[sf_index]:
        return [(bits or 16, out_ch, 2 * out_ch * n) for n in R.chunk_counts(OF.RATES[sf_index], rate, A.ACCEPTED * 1024)]
    return [(bits or 16, out_ch, 2 * out_ch * 1024)] * A.ACCEPTED


def three_ways(engine, sf_index, options):
    want = host_tick(engine, sf_index, options)
    for (channels, s), w in zip(A.cases(sf_index).items(), want):
        assert not [x for x in w if x[0] == "error"], (sf_index, channels, [x for x in w if x[0] == "error"])
        assert [(b, c, len(d)) for b, c, d in w] == expected_sizes(sf_index, channels, options), (sf_index, channels)
        assert any(any(d) for _, _, d in w), (sf_index, channels)   # not silence
    for mode in ("gpu", "quant"):
        got = run(engine, mode, specs_of(sf_index, options), PER_TICK)
        assert len(got) == len(want) == 2
        for channels, w, g in zip((1, 2), want, got):
            assert len(g) == len(w), (mode, sf_index, channels, len(g), len(w), [x for x in g if x[0] == "error"])
            assert g == w, (mode, sf_index, channels, [k for k, (a, b) in enumerate(zip(g, w)) if a != b][:4])


@pytest.mark.parametrize("sf_index", A.INDICES)
def test_tick_three_ways_as_decoded(engine, sf_index):
    three_ways(engine, sf_index, (None, None, None))


@pytest.mark.parametrize("rate", COMMON_TO_16K)
def test_tick_three_ways_to_16k_mono(engine, rate):
    three_ways(engine, OF.RATES.index(rate), (16, 16000, 1))


# ---- 4. one scheduler round ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[0, 1, 2], ids=["host_front_end", "gpu_front_end", "host_huffman_gpu_rest"])
def sched(engine, request):
    s = pipeline.BatchScheduler(engine, entropy_threads=4, max_streams=64, max_frames_per_tick=256, max_stream_frames_per_tick=4,
                                gpu_entropy=request.param)
    yield s
    s.close()


CHUNK_SIZES = [4096, 333, 211, 100000, 777, 64, 5000, 97, 2048, 1500, 150, 40000, 1234]


def feed_and_drain(handles, datas, chunk_sizes, deadline_s=60):
    """every stream's bytes in pieces of its chunk size, then finish, taking the outputs meanwhile; a stream that has ended on an error
    takes no more input (PipelineClosed): it is noted, not fed further -> (outputs per stream, streams that closed while being fed)"""
    n = len(handles)
    pos, fed, closed, outs, live = [0] * n, [False] * n, set(), [[] for _ in range(n)], set(range(n))
    t0 = time.time()
    while live:
        assert time.time() - t0 < deadline_s, ("scheduler stalled", sorted(live))
        for i in sorted(live):
            if not fed[i]:
                piece = datas[i][pos[i]:pos[i] + chunk_sizes[i]]      # empty behind the last byte: finish
                try:
                    handles[i].send(piece)
                    pos[i] += len(piece)
                    fed[i] = not piece
                except pipeline.DecodeError as e:
                    assert e.kind in ("InputBufferFull", "PipelineClosed"), (i, e.kind)
                    if e.kind == "PipelineClosed":
                        fed[i] = True
                        closed.add(i)
            while True:
                got = handles[i].try_recv()
                if got is None:
                    break
                outs[i].append(got)
            if fed[i] and handles[i].ended():
                live.discard(i)
        time.sleep(0.0002)
    return outs, closed


def scheduler_round(sched, options):
    """thirteen streams, one per index, mono at the even indices and stereo at the odd ones
    -> (channel counts, outputs per stream, streams that closed while being fed)"""
    channels = [1 + (sf_index & 1) for sf_index in A.INDICES]
    datas = [A.cases(sf_index)[ch].adts() for sf_index, ch in zip(A.INDICES, channels)]
    handles = [sched.spawn(pipeline.DecodeOptions(*options)) for _ in datas]
    try:
        outs, closed = feed_and_drain(handles, datas, CHUNK_SIZES)
    finally:
        for h in handles:
            h.cancel()
    return channels, outs, closed


def test_scheduler_round_as_decoded(engine, sched):
    channels, outs, closed = scheduler_round(sched, (None, None, None))
    assert not closed
    for sf_index, ch, got in zip(A.INDICES, channels, outs):
        assert all(not isinstance(g, Exception) for g in got), (sf_index, [str(g) for g in got if isinstance(g, Exception)])
        want = host_tick(engine, sf_index, (None, None, None))[ch - 1]
        assert len(want) == A.ACCEPTED
        assert as_tuples(got) == [(b, c, OF.RATES[sf_index], d) for b, c, d in want], (sf_index, ch, len(got))


def test_scheduler_round_to_16k_mono(engine, sched):
    options = (16, 16000, 1)
    channels, outs, closed = scheduler_round(sched, options)
    refused = 0
    for sf_index, ch, got in zip(A.INDICES, channels, outs):
        if OF.RATES[sf_index] in NOT_COMMON:
            assert len(got) == 1 and isinstance(got[0], pipeline.DecodeError), (sf_index, len(got))
            assert str(got[0]) == RESAMPLER_ERROR, (sf_index, str(got[0]))
            refused += 1
            continue
        assert all(not isinstance(g, Exception) for g in got), (sf_index, [str(g) for g in got if isinstance(g, Exception)])
        want = host_tick(engine, sf_index, options)[ch - 1]     # at 16 kHz: the 16-bit mono records, no rate change
        assert len(want) == len(expected_sizes(sf_index, ch, options))
        assert as_tuples(got) == [(b, c, 16000, d) for b, c, d in want], (sf_index, ch, len(got))
    assert refused == 4
    assert closed <= {i for i in A.INDICES if OF.RATES[i] in NOT_COMMON}, closed   # only a refused stream stops taking input


REFUSED = {"adts": "aac/aac-stereo-48k.adts", "layer_3": "mp3/stereo16k_A_Tusk_encoded.mp3", "layer_2": "mp2/stereo48k_A_Tusk_1s.mp2"}


@pytest.mark.parametrize("kind", list(REFUSED))
def test_a_refused_output_rate_ends_only_its_stream(engine, sched, kind):
    """What the round above found at the four AAC rates, for each of the scheduler's three framers that open a resampler on a stream's
    first header: 12 kHz is no rate the resampler gives, so a stream asked for it ends with the reference's error -- and the pass that
    failed must not leave a row in the tick that asks for the resampler the stream does not have, which made the tick refuse every
    stream in it ("engine tick: stream is not open").  Four neighbours as decoded deliver what one of them delivers alone."""
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    neighbour = open(os.path.join(gold, "aac", "aac-stereo-48k.adts"), "rb").read()
    refused = open(os.path.join(gold, REFUSED[kind]), "rb").read()

    def round_of(datas, options):
        handles = [sched.spawn(pipeline.DecodeOptions(*o)) for o in options]
        try:
            return feed_and_drain(handles, datas, [100000] * len(datas))
        finally:
            for h in handles:
                h.cancel()
    alone, closed = round_of([neighbour], [(None, None, None)])
    assert not closed and len(alone[0]) == 48 and not any(isinstance(a, Exception) for a in alone[0])
    outs, closed = round_of([neighbour, refused, neighbour, refused, neighbour, neighbour],
                            [(None, None, None), (16, 12000, 1), (None, None, None), (16, 12000, 1), (None, None, None), (None, None, None)])
    assert closed <= {1, 3}
    for k, got in enumerate(outs):
        if k in (1, 3):
            assert len(got) == 1 and isinstance(got[0], pipeline.DecodeError) and str(got[0]) == RESAMPLER_ERROR, (k, [str(g) for g in got][:2])
        else:
            assert not any(isinstance(a, Exception) for a in got), (k, [str(a) for a in got if isinstance(a, Exception)])
            assert as_tuples(got) == as_tuples(alone[0]), (k, len(got))

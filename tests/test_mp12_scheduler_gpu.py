"""MPEG Layer I and II behind the batch scheduler (csrc/pipeline.cpp, sk_tick_run_mixed_mpa): a stream whose first confirmed frame is
Layer I or II is parsed on the entropy threads (allocation, scale factors), its frames ride in the tick beside the AAC units and the
Layer III granules, and every Layer II frame becomes two AudioData of 576 frames, every Layer I frame one of 384, that take the same
apply_output_options path.

The reference's MP2 fixture (Layer II, MPEG-1, 48 kHz, stereo):
* no options: alone and beside one ADTS and one Layer III stream -- every stream equals its single decoder;
* 16 kHz mono 16 bit (48 -> 16 k through the FIR): against the oracle's CPU chain on Mp3Decoder's s16;
* a frame whose allocation overruns is dropped, exactly that frame; the clean stream beside it is untouched.

Streams written by tests/mp12_builder.py, one per configuration of tests/test_mp12_cpu.py's CONFIGS -- both layers, MPEG-1 and LSF,
every Layer II table, mono / stereo / dual / joint stereo with each bound, CRC and padding, six source rates -- with scale-factor
indices from 9 up, so that no expected sample leaves +-1 (asserted on the float64 model of tests/mp12_model.py, with a peak above 0.1,
before the GPU's output is looked at):
* no options: all nineteen in one scheduler at two frame budgets, two front ends and on two lanes -- each equals its single
  decoder bit for bit, in units of 384 / 576 frames, and lies within one s16 step of f32_to_i16 of the model;
* rate, channel and width changes (every source rate to 16 kHz mono and to 8 kHz, 16 -> 16 kHz, 16 and 24 -> 48 kHz, 24 bit)
  against the CPU chain on Mp3Decoder's s16;
* the tick itself through Engine.tick_run_mpa, where the test decides which frames share a tick: the output does not depend on
  how the frames are dealt out over ticks, with and without a resampler; a tick it refuses changes no stream state; an empty tick
  with flush yields the flush tail;
* a damaged Layer I frame loses exactly its 384 frames."""
import threading
import types

import numpy as np
import pytest

import mp12_builder as B
import mp12_model as M
from soundkit_amd import mp3, pipeline
from soundkit_amd._lib import SoundkitError
from test_mp12_cpu import CONFIGS
from test_scheduler_gpu import drain, feed_all
from test_scheduler_mp3_gpu import read, single_decoder

pytestmark = pytest.mark.gpu
MP2 = "mp2/stereo48k_A_Tusk_1s.mp2"
ADTS = "aac/aac-stereo-48k.adts"
MP3 = "mp3/stereo16k_A_Tusk_encoded.mp3"


def run(engine, datas, chunks, options=None, **config):
    """options: None, one DecodeOptions for every stream, or a list with one (or None) per stream"""
    config.setdefault("max_streams", 8)
    sched = pipeline.BatchScheduler(engine, entropy_threads=3, **config)
    try:
        options = options if isinstance(options, list) else [options] * len(datas)
        handles = [sched.spawn(o) if o is not None else sched.spawn() for o in options]
        feeder = threading.Thread(target=feed_all, args=(handles, datas, chunks))
        feeder.start()
        outs = drain(handles, 60)
        feeder.join()
        for h in handles:
            h.cancel()
    finally:
        sched.close()
    for got in outs:
        assert got and not any(isinstance(a, Exception) for a in got), [a for a in got if isinstance(a, Exception)][:1]
    return outs


def samples_of(outs):
    return np.concatenate([np.frombuffer(a.data.tobytes(), "<i2") for a in outs])


@pytest.fixture(scope="module")
def mp2_alone(engine):
    rate, channels, samples = single_decoder(engine, "mp2", read(MP2))
    assert (rate, channels, samples.size) == (48000, 2, 42 * 1152 * 2) and np.abs(samples.astype(np.int32)).max() > 500
    return samples


@pytest.mark.parametrize("front_end", [0, 3], ids=["host_front_end", "gpu_front_end_with_mp3_huffman_in_the_tick"])
def test_the_fixture_alone_and_beside_an_adts_and_a_layer_three_stream(engine, mp2_alone, front_end):
    names = [MP2, ADTS, MP3, MP2]
    datas = [read(n) for n in names]
    want = [mp2_alone, single_decoder(engine, ADTS, datas[1])[2], single_decoder(engine, MP3, datas[2])[2], mp2_alone]
    alone = run(engine, [datas[0]], [100000], gpu_entropy=front_end)[0]
    assert np.array_equal(samples_of(alone), mp2_alone)
    # small per-stream and per-tick budgets: many ticks, every one with frames of all three kinds; odd chunk sizes
    outs = run(engine, datas, [113, 1500, 777, 4096], max_frames_per_tick=24, max_stream_frames_per_tick=5, gpu_entropy=front_end)
    for name, got, samples in zip(names, outs, want):
        if name == MP2:
            assert len(got) == 84  # two AudioData per Layer II frame
            assert all((a.sampling_rate, a.channel_count, a.bits_per_sample, a.data.size) == (48000, 2, 16, 576 * 2 * 2) for a in got)
        assert np.array_equal(samples_of(got), samples), name


def test_sixteen_kilohertz_mono_meets_the_cpu_chain(engine, oracle, mp2_alone):
    q = mp2_alone.reshape(-1, 2)  # Mp3Decoder's i16 AudioData
    rs = oracle.StreamingResampler(48000, 16000, 2)
    outs = []
    for g in range(0, q.shape[0], 576):  # the worker resamples AudioData by AudioData
        res = rs.process(np.ascontiguousarray(q[g:g + 576].T.astype(np.float32) / np.float32(32768.0)))
        if res.shape[1]:
            outs.append(oracle.planar_f32_to_s16_interleaved(oracle.downmix_mono(res)[None]))
    tail = rs.flush()
    if tail.shape[1]:
        outs.append(oracle.planar_f32_to_s16_interleaved(oracle.downmix_mono(tail)[None]))
    want = np.concatenate([o.reshape(-1) for o in outs]).astype(np.int32)
    assert np.abs(want).max() > 300

    data = read(MP2)
    got = run(engine, [data] * 3, [777, 4096, 100000], pipeline.DecodeOptions(16, 16000, 1))
    for outs in got:
        assert all(a.sampling_rate == 16000 and a.channel_count == 1 and a.bits_per_sample == 16 for a in outs)
        mine = samples_of(outs).astype(np.int32)
        assert mine.size == want.size, (mine.size, want.size)
        d = np.abs(mine - want)
        print("largest difference %d, %.4f %% of the samples differ" % (int(d.max()), 100 * float((d > 0).mean())))
        assert d.max() <= 1 and (d > 0).mean() < 0.01, (int(d.max()), float((d > 0).mean()))


def test_a_damaged_frame_loses_exactly_its_samples(engine, mp2_alone):
    good = read(MP2)
    bad = bytearray(good)
    k = 17
    bad[576 * k + 4:576 * k + 24] = b"\xff" * 20  # every allocation of frame 17 at its widest class: the samples would overrun the frame
    bad = bytes(bad)
    want_bad = single_decoder(engine, "mp2", bad)[2]
    assert want_bad.size == 41 * 2304
    outs = run(engine, [good, bad, good], [1500, 1500, 333], max_stream_frames_per_tick=4)
    assert np.array_equal(samples_of(outs[0]), mp2_alone) and np.array_equal(samples_of(outs[2]), mp2_alone)
    mine = samples_of(outs[1])
    assert len(outs[1]) == 82 and mine.size == 41 * 2304
    assert np.array_equal(mine, want_bad)
    assert np.array_equal(mine[:k * 2304], mp2_alone[:k * 2304])  # untouched up to the damage; behind it the FIFO has missed a frame


# ---- streams written by the builder: every configuration of CONFIGS ---------------------------------------------------------------
SCF_FLOOR = 9                  # scale-factor indices 9 ... 63: no stream leaves +-1, the quietest peaks near 0.25 (mp12_builder.random_frame)
L1_FRAMES, L2_FRAMES = 24, 10  # 9216 and 11 520 PCM frames: more than two 4096-frame resampler chunks
CHUNKS = [61, 113, 777, 4096, 1 << 20]
INVALID_ARG = -1
L1_STEREO_48K, L1_MONO_44K, L1_JOINT_32K, L1_DUAL_16K = ("Layer I stereo 48k 384k", "Layer I mono 44.1k 192k pad crc", "Layer I joint bound 8 32k",
                                                          "Layer I LSF dual 16k 128k")
L2_STEREO_48K, L2_MONO_32K = "B.2a stereo 48k 192k", "B.2b mono 32k 128k"


def build_stream(name, scf_floor=SCF_FLOOR):
    """one stream of a configuration and what the float64 model makes of it; the two model-side conditions every test below rests on
    are asserted here, before any GPU output exists"""
    cfg = CONFIGS[name]
    rng = np.random.default_rng(1000 + sum(name.encode()))
    frames = [B.random_frame(rng, *cfg, scf_floor=scf_floor)[0] for _ in range(L1_FRAMES if cfg[0] == 1 else L2_FRAMES)]
    data = b"".join(frames)
    h = M.parse_header(data[:4])
    model = M.Decoder().stream(data)
    unit = 384 if h["layer"] == 1 else 576
    assert model.shape == (len(frames) * h["samples_per_channel"], h["channels"]) and h["samples_per_channel"] % unit == 0
    peak = float(np.abs(model).max())
    assert peak <= 1.0, (name, peak)  # an expected sample outside +-1: raise this stream's scf_floor
    assert peak > 0.1, (name, peak)
    return types.SimpleNamespace(name=name, layer=h["layer"], rate=h["sample_rate"], channels=h["channels"], unit=unit, frames=frames, data=data,
                                 model=model, units=len(frames) * h["samples_per_channel"] // unit)


@pytest.fixture(scope="module")
def built():
    return {name: build_stream(name) for name in sorted(CONFIGS)}


@pytest.fixture(scope="module")
def alone(engine, built):
    """every stream through its single decoder (Mp3Decoder, s16): held to the float64 model by tests/test_mp12_decoder_gpu.py"""
    out = {}
    for name, b in built.items():
        rate, channels, samples = single_decoder(engine, "mp2", b.data)
        assert (rate, channels, samples.size) == (b.rate, b.channels, b.model.size), name
        out[name] = samples
    return out


@pytest.fixture(scope="module")
def others(engine):
    return [(read(n), single_decoder(engine, n, read(n))[2]) for n in (ADTS, MP3)]


def check_every_configuration(engine, oracle, built, alone, others, **config):
    names = sorted(CONFIGS)
    datas = [built[n].data for n in names] + [d for d, _ in others]
    outs = run(engine, datas, [CHUNKS[i % len(CHUNKS)] for i in range(len(datas))], max_streams=32, max_frames_per_tick=24, **config)
    for name, got in zip(names, outs):
        b = built[name]
        assert all((a.sampling_rate, a.channel_count, a.bits_per_sample) == (b.rate, b.channels, 16) for a in got), name
        assert [a.data.size for a in got] == [b.unit * b.channels * 2] * b.units, (name, len(got), b.units)  # one per Layer I frame, two per Layer II frame
        mine = samples_of(got)
        assert np.array_equal(mine, alone[name]), name
        want = oracle.pcm_convert("MP3_F32_TO_I16", b.model.astype(np.float32).reshape(-1)).astype(np.int32)
        assert np.abs(mine.astype(np.int32) - want).max() <= 1, name
    for (_, samples), got in zip(others, outs[len(names):]):
        assert np.array_equal(samples_of(got), samples)


@pytest.mark.parametrize("front_end", [0, 3], ids=["host_front_end", "gpu_front_end_with_mp3_huffman_in_the_tick"])
@pytest.mark.parametrize("stream_budget", [1, 5])
def test_every_configuration_equals_its_single_decoder(engine, oracle, built, alone, others, stream_budget, front_end):
    """All nineteen streams beside an ADTS and a Layer III stream, 24 units per tick; a Layer I stream hands a pass `stream_budget`
    frames, a Layer II stream half of it and never less than one (parse_some_mpa)"""
    check_every_configuration(engine, oracle, built, alone, others, max_stream_frames_per_tick=stream_budget, gpu_entropy=front_end)


def test_every_configuration_on_two_lanes(engine, oracle, built, alone, others):
    check_every_configuration(engine, oracle, built, alone, others, max_stream_frames_per_tick=5, gpu_entropy=1, lanes=2)


# ---- rate, channel and width changes against the CPU chain -------------------------------------------------------------------------
def cpu_chain(oracle, samples, channels, unit, in_hz, out_hz, mono):
    """apply_output_options on Mp3Decoder's s16, AudioData by AudioData: / 32768, StreamingResampler, downmix, s16 -> one int16 array per
    AudioData the worker would send (with a resampler: one per completed chunk, then the flushed tail)"""
    q = samples.reshape(-1, channels)

    def planar(block):
        return np.ascontiguousarray(block.T.astype(np.float32) / np.float32(32768.0))

    def finish(p):
        return oracle.planar_f32_to_s16_interleaved(oracle.downmix_mono(p)[None] if mono and channels > 1 else p)
    if in_hz == out_hz:
        return [finish(planar(q[g:g + unit])) for g in range(0, q.shape[0], unit)]
    rs = oracle.StreamingResampler(in_hz, out_hz, channels)
    res = [rs.process(planar(q[g:g + unit])) for g in range(0, q.shape[0], unit)] + [rs.flush()]
    return [finish(r) for r in res if r.shape[1]]


def assert_meets_the_chain(label, mine, want):
    """the project's bounds wherever a resampler runs: equal counts, at most one step, fewer than 1 % of the samples differing"""
    mine, want = mine.astype(np.int32), want.astype(np.int32)
    assert mine.size == want.size, (label, mine.size, want.size)
    d = np.abs(mine - want)
    print("%s: largest difference %d, %.4f %% of %d samples differ" % (label, int(d.max()), 100 * float((d > 0).mean()), d.size))
    assert np.abs(want).max() > 1000, label
    assert d.max() <= 1 and (d > 0).mean() < 0.01, (label, int(d.max()), float((d > 0).mean()))


# every source rate CONFIGS holds; per rate a Layer I and a Layer II stream where there is one, mono and stereo sources
EVERY_RATE = [L1_STEREO_48K, "B.2c mono 48k 48k", L1_MONO_44K, "B.2b stereo 44.1k 256k crc", L1_JOINT_32K, L2_MONO_32K, "LSF mono 24k 64k",
              "LSF stereo 22.05k 128k pad", L1_DUAL_16K, "joint bound 16 LSF"]
CHANGES = {
    "to_16k_mono": (EVERY_RATE, pipeline.DecodeOptions(16, 16000, 1)),   # the two 16 kHz streams: no resampler, bit for bit
    "to_8k": (EVERY_RATE, pipeline.DecodeOptions(16, 8000, None)),
    "up_to_48k": ([L1_DUAL_16K, "joint bound 16 LSF", "LSF mono 24k 64k"], pipeline.DecodeOptions(16, 48000, None)),  # the largest output per chunk
    "to_24_bit": (["B.2d mono 32k 32k"], pipeline.DecodeOptions(24, None, 1)),  # a width change only
}


@pytest.mark.parametrize("change", sorted(CHANGES))
def test_rate_channel_and_width_changes_meet_the_cpu_chain(engine, oracle, built, alone, change):
    names, opts = CHANGES[change]
    assert change not in ("to_16k_mono", "to_8k") or {built[n].rate for n in names} == {built[n].rate for n in built}
    outs = run(engine, [built[n].data for n in names], [CHUNKS[(i + 1) % len(CHUNKS)] for i in range(len(names))], opts, max_streams=16,
               max_stream_frames_per_tick=6)
    for name, got in zip(names, outs):
        b = built[name]
        rate, channels, bits = opts.output_sample_rate or b.rate, opts.output_channels or b.channels, opts.output_bits_per_sample
        assert all((a.sampling_rate, a.channel_count, a.bits_per_sample) == (rate, channels, bits) for a in got), name
        if bits == 24:  # i16 -> / 32768 -> f32_to_s24 (f32_channels_to_bytes), one AudioData per unit
            s24 = oracle.pcm_convert("F32LE_TO_S24", oracle.pcm_convert("VEC_I16_TO_F32", alone[name]))
            want = s24.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
            assert [a.data.size for a in got] == [b.unit * channels * 3] * b.units
            assert b"".join(a.data.tobytes() for a in got) == want, name
            continue
        want = cpu_chain(oracle, alone[name], b.channels, b.unit, b.rate, rate, channels < b.channels)
        mine = samples_of(got)
        if rate == b.rate:  # nothing to resample: the single decoder's samples, downmixed
            assert [a.data.size for a in got] == [w.size * 2 for w in want], name
            assert np.array_equal(mine, np.concatenate(want)), name
            print("%s -> %s: no resampler, bit for bit" % (name, change))
        else:
            assert_meets_the_chain("%s -> %s" % (name, change), mine, np.concatenate(want))


# ---- the tick itself: Engine.tick_run_mpa, where the test decides which frames share a tick -----------------------------------------
@pytest.fixture(scope="module")
def synthesis_window(engine):
    """the engine's window D (a decoder handle or the scheduler would have set it)"""
    mp3.set_synthesis_window(np.ctypeslib.as_array(mp3.iso_tables().window), engine)


def records_of(frames):
    out = []
    for f in frames:
        rc, info = mp3.mpa_parse_header(f[:4])
        assert rc == 0
        rc, rec = mp3.mpa_parse_frame(f, info)
        assert rc == 0
        out.append((rec, f))
    return out


def run_ticks(engine, jobs, flush=None):
    """jobs: [(stream of `built`, its (record, bytes) pairs, frames per tick, output rate or None, output channels)] on fresh engine
    streams that share every tick; flush "last": in the last tick with frames, "alone": in an empty tick behind it.
    -> per job the tick's output records (stream_index, status, frames, channels, bits, bytes)"""
    sids = [engine.open_stream(b.rate, b.channels) for b, _, _, _, _ in jobs]
    try:
        for sid, (b, _, _, out_rate, _) in zip(sids, jobs):
            if out_rate:
                engine.resampler_open(sid, b.rate, out_rate)
        outs, at = [[] for _ in jobs], [0] * len(jobs)
        n_ticks = max(len(parts) for _, _, parts, _, _ in jobs)
        for t in range(n_ticks + (flush == "alone")):
            table = []
            for j, (b, recs, parts, out_rate, out_channels) in enumerate(jobs):
                take = parts[t] if t < len(parts) else 0
                end = (flush == "last" and t == n_ticks - 1) or t == n_ticks
                table.append(dict(stream=sids[j], channels=b.channels, out_bits=16, out_channels=out_channels, resample=bool(out_rate),
                                  flush=bool(out_rate) and end, frames=recs[at[j]:at[j] + take]))
                at[j] += take
            for r in engine.tick_run_mpa(table):
                assert r[1] == 0 and (r[3], r[4], len(r[5])) == (jobs[r[0]][4], 16, r[2] * jobs[r[0]][4] * 2), r[:5]
                outs[r[0]].append(r)
        assert all(at[j] == len(jobs[j][1]) for j in range(len(jobs)))
        return outs
    finally:
        for sid in sids:
            engine.close_stream(sid)


def bytes_of(records):
    return b"".join(r[5] for r in records)


# one tick (4224 PCM frames of Layer I: the chunk boundary falls inside the eleventh unit), one frame per tick, uneven ticks
PARTITIONS = [([11], [10], "last"), ([1] * 11, [1] * 10, "alone"), ([3, 1, 5, 2], [3, 1, 5, 1], "alone")]


def test_the_output_does_not_depend_on_how_frames_are_dealt_out_over_ticks(engine, oracle, built, alone, synthesis_window):
    one, two = built[L1_STEREO_48K], built[L2_MONO_32K]
    recs = [records_of(one.frames[:11]), records_of(two.frames[:10])]
    got = []
    for p1, p2, flush in PARTITIONS:
        outs = run_ticks(engine, [(one, recs[0], p1, 16000, 1), (two, recs[1], p2, 16000, 1)], flush)
        got.append([bytes_of(o) for o in outs])
    assert got[0] == got[1] == got[2]
    for b, n, mine in ((one, 11, got[0][0]), (two, 10, got[0][1])):
        size = n * (1152 if b.layer == 2 else 384) * b.channels
        want = cpu_chain(oracle, alone[b.name][:size], b.channels, b.unit, b.rate, 16000, b.channels > 1)
        assert_meets_the_chain("%s, %d frames -> 16 kHz mono in ticks" % (b.name, n), np.frombuffer(mine, "<i2"), np.concatenate(want))


def test_without_a_resampler_every_partition_gives_the_single_decoders_bytes(engine, built, alone, synthesis_window):
    one, two = built[L1_STEREO_48K], built[L2_MONO_32K]
    recs = [records_of(one.frames[:11]), records_of(two.frames[:10])]
    for p1, p2, _ in PARTITIONS:
        outs = run_ticks(engine, [(one, recs[0], p1, None, 2), (two, recs[1], p2, None, 1)])
        assert [r[2] for r in outs[0]] == [384] * 11 and [r[2] for r in outs[1]] == [576] * 20
        assert bytes_of(outs[0]) == alone[one.name][:11 * 384 * 2].tobytes()
        assert bytes_of(outs[1]) == alone[two.name][:10 * 1152].tobytes()


def test_a_refused_tick_leaves_the_stream_as_it_was(engine, built, synthesis_window):
    """Four ticks the entry point must refuse (SK_ERR_INVALID_ARG), each between the same two clean ticks of one resampling stream:
    the clean ticks' bytes are those of a stream that never saw a refusal -- the polyphase FIFO and the resampler's fill are untouched"""
    one = built[L1_STEREO_48K]
    recs, foreign = records_of(one.frames[:11]), records_of(built[L2_STEREO_48K].frames[:1])
    assert foreign[0][0].channels == recs[0][0].channels == 2 and foreign[0][0].sample_rate == recs[0][0].sample_rate

    def entry(sid, **more):
        return dict(stream=sid, channels=2, out_bits=16, out_channels=1, resample=True, **more)

    def mixed_layers(sid):
        engine.tick_run_mpa([entry(sid, frames=[recs[4], foreign[0], recs[5]])])

    def granule_bits_off_by_one(sid):
        packed = mp3.mpa_pack_frames(recs[4:7])
        packed[0][1].granule_bits += 1
        engine.tick_run_mpa([entry(sid, n_frames=3)], packed)

    def odd_byte_offset(sid):
        packed = mp3.mpa_pack_frames(recs[4:7])
        packed[0][1].byte_offset += 2
        engine.tick_run_mpa([entry(sid, n_frames=3)], packed)

    def count_disagrees(sid):
        engine.tick_run_mpa([entry(sid, n_frames=2)], mp3.mpa_pack_frames(recs[4:7]))

    def session(refusals):
        sid = engine.open_stream(one.rate, one.channels)
        try:
            engine.resampler_open(sid, one.rate, 16000)
            out = engine.tick_run_mpa([entry(sid, frames=recs[:4])])
            for refused in refusals:
                with pytest.raises(SoundkitError) as exc:
                    refused(sid)
                assert exc.value.status == INVALID_ARG, (refused.__name__, str(exc.value))
            out += engine.tick_run_mpa([entry(sid, frames=recs[4:], flush=True)])
            assert all(r[1] == 0 for r in out)
            return [(r[2], r[5]) for r in out]
        finally:
            engine.close_stream(sid)
    clean = session([])
    assert len(clean) == 2  # one 4096-frame chunk, then the flushed tail
    for refused in (mixed_layers, granule_bits_off_by_one, odd_byte_offset, count_disagrees):
        assert session([refused]) == clean, refused.__name__
    assert session([mixed_layers, granule_bits_off_by_one, odd_byte_offset, count_disagrees]) == clean


def test_an_empty_tick_with_flush_yields_the_flush_tail(engine, oracle, built, alone, synthesis_window):
    one = built[L1_STEREO_48K]
    want = cpu_chain(oracle, alone[one.name][:11 * 384 * 2], 2, 384, 48000, 16000, True)
    assert len(want) == 2  # 4224 frames in: one chunk, and a tail that holds the other 128 frames and the delay line
    sid = engine.open_stream(one.rate, one.channels)
    try:
        engine.resampler_open(sid, one.rate, 16000)
        entry = dict(stream=sid, channels=2, out_bits=16, out_channels=1, resample=True)
        first = engine.tick_run_mpa([dict(entry, frames=records_of(one.frames[:11]))])
        tail = engine.tick_run_mpa([dict(entry, frames=[], flush=True)])
    finally:
        engine.close_stream(sid)
    assert [(r[1], r[2], r[3], r[4]) for r in first] == [(0, want[0].size, 1, 16)]
    assert [(r[1], r[2], r[3], r[4]) for r in tail] == [(0, want[1].size, 1, 16)]
    assert_meets_the_chain("the chunk", np.frombuffer(first[0][5], "<i2"), want[0])
    assert_meets_the_chain("the flush tail of an empty tick", np.frombuffer(tail[0][5], "<i2"), want[1])


# ---- damage -----------------------------------------------------------------------------------------------------------------------
def test_a_damaged_layer_one_frame_loses_exactly_its_384_frames(engine, built, alone):
    one, two = built[L1_STEREO_48K], built[L2_STEREO_48K]
    k, size = 7, len(one.frames[0])
    assert size == 384 and all(len(f) == size for f in one.frames)
    bad = bytearray(one.data)
    bad[size * k + 4:size * k + 36] = b"\xff" * 32  # every allocation of frame 7 (4 bits x 32 subbands x 2 channels) is the forbidden index 15
    bad = bytes(bad)
    rc, info = mp3.mpa_parse_header(bad[size * k:size * k + 4])
    assert rc == 0 and mp3.mpa_parse_frame(bad[size * k:size * (k + 1)], info)[0] == -304
    want_bad = single_decoder(engine, "mp2", bad)[2]
    assert want_bad.size == (L1_FRAMES - 1) * 768
    outs = run(engine, [one.data, bad, two.data, one.data], [1500, 1500, 777, 333], max_stream_frames_per_tick=4)
    assert np.array_equal(samples_of(outs[0]), alone[one.name]) and np.array_equal(samples_of(outs[3]), alone[one.name])
    assert np.array_equal(samples_of(outs[2]), alone[two.name])
    mine = samples_of(outs[1])
    assert len(outs[1]) == L1_FRAMES - 1 and all(a.data.size == 384 * 2 * 2 for a in outs[1])
    assert np.array_equal(mine, want_bad)
    assert np.array_equal(mine[:k * 768], alone[one.name][:k * 768])  # untouched up to the damage; behind it the FIFO has missed a frame
    assert not np.array_equal(mine[k * 768:(k + 1) * 768], alone[one.name][(k + 1) * 768:(k + 2) * 768])

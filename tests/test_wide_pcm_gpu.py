"""PCM sources of 3 ... 8 channels on the GPU (csrc/pcm_wide.hip; sk_engine_enable_wide_pcm, sk_pcm_downmix, sk_tick_run_pcm and the
resampler on wide streams) against wide_pcm_model, which restates downmix_channels (soundkit-decoder/src/lib.rs:3492-3561):

* sk_pcm_downmix bit for bit: every channel count and target, frame counts around the kernel's 512-frame slice, the peak of the
  stereo branch in every awkward place, zeros, NaN and infinities;
* the tick without a rate change: every format x channel count x depth x target side by side in the same ticks, bit for bit against
  the model and the one-stream path, with quiet and loud units of one stream next to each other;
* the resampler on 6 and 8 rows: every row the bits of the same samples as a mono stream;
* the tick with a rate change: the one-stream path's bytes whatever the cut; the model's downmix applied to the GPU's own resampled
  rows bit for bit (the peak pass behind the resampler, without a tolerance); the CPU chain within lsb_check's bound;
* 1024 six-channel streams in one tick.

Every test runs on its own engine with the pool of wide streams; the session's engine stays without it."""
import numpy as np
import pytest

import pcm_worker_model as M
import wide_pcm_model as W
from soundkit_amd import decoder
from soundkit_amd.audio_types import AudioData, EncodingFlag, Endianness
from test_pcm_pipeline_gpu import fmt_fields, lsb_check, run_pcm_ticks

pytestmark = pytest.mark.gpu

SLICE = 512  # kWideSliceFrames
FORMATS = list(range(M.FMT_S16LE, M.FMT_F32BE + 1))


@pytest.fixture(scope="module")
def wide(engine):
    """the module's engine with 32 wide slots (the session's `engine` first: the decoder mirrors' default stays that one)"""
    import soundkit_amd
    eng = soundkit_amd.Engine(0, 64)
    eng.enable_wide_pcm(32)
    assert eng.wide_pcm_streams == 32
    yield eng
    eng.close()


def same(a, b):
    """bit for bit, any NaN equal to any NaN (the sign and payload of a generated NaN are the platform's)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ---- the pool and what a wide stream may do -----------------------------------------------------------------------------------------

def test_pool_rules(wide, engine):
    import soundkit_amd
    from soundkit_amd._lib import SoundkitError
    assert engine.wide_pcm_streams == 0
    with pytest.raises(SoundkitError) as exc:  # without the pool: as before
        engine.open_stream(48000, 6)
    assert exc.value.status == -1
    with pytest.raises(SoundkitError) as exc:
        engine.tick_run_pcm([{"n_units": 1, "format": M.FMT_S16LE, "channels": 6, "out_bits": 16, "out_channels": 1}], [bytes(12 * 40)])
    assert exc.value.status == -6
    with pytest.raises(SoundkitError) as exc:  # once per engine
        wide.enable_wide_pcm(4)
    assert exc.value.status == -1
    with pytest.raises(SoundkitError) as exc:  # nine channels: beyond SK_MAX_PCM_CHANNELS
        wide.tick_run_pcm([{"n_units": 1, "format": M.FMT_S16LE, "channels": 9, "out_bits": 16, "out_channels": 1}], [bytes(18 * 40)])
    assert exc.value.status == -6
    with pytest.raises(SoundkitError) as exc:
        wide.open_stream(48000, 9)
    assert exc.value.status == -1
    small = soundkit_amd.Engine(0, 8)
    try:
        with pytest.raises(SoundkitError) as exc:
            small.enable_wide_pcm(9)  # more than max_streams
        assert exc.value.status == -1
        with pytest.raises(SoundkitError) as exc:
            small.enable_wide_pcm(0)  # a pool of nothing is no pool
        assert exc.value.status == -1 and small.wide_pcm_streams == 0
        small.enable_wide_pcm(2)
        a, b = small.open_stream(48000, 3), small.open_stream(44100, 8)
        with pytest.raises(SoundkitError) as exc:
            small.open_stream(48000, 5)
        assert exc.value.status == -7  # SK_ERR_CAPACITY: no wide slot left; narrow streams still open
        n = small.open_stream(48000, 2)
        small.close_stream(a)
        c = small.open_stream(48000, 6)  # the slot came back
        # a wide stream has no synthesis state and decodes nothing
        with pytest.raises(SoundkitError) as exc:
            small.get_state(c, 2)
        assert exc.value.status == -1
        for sid in (b, c, n):
            small.close_stream(sid)
        late = soundkit_amd.Engine(0, 8)
        try:
            s = late.open_stream(48000, 2)
            late.resampler_open(s, 48000, 16000)
            with pytest.raises(SoundkitError) as exc:  # the rows are allocated: too late
                late.enable_wide_pcm(2)
            assert exc.value.status == -1
        finally:
            late.close()
    finally:
        small.close()


# ---- sk_pcm_downmix ---------------------------------------------------------------------------------------------------------------

FRAME_COUNTS = [1, 63, 64, 65, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE - 1, 2 * SLICE, 2 * SLICE + 1]


def test_downmix_every_shape(wide):
    rng = np.random.default_rng(1)
    n_scaled = n_plain = 0
    for C in range(3, 9):
        for frames in FRAME_COUNTS:
            x = rng.uniform(-0.55, 0.55, (C, frames)).astype(np.float32)  # |L|, |R| reach 0.55 * 2.414 = 1.33: both sides of 1 occur
            for T in (1, 2, 3, C):
                got = wide.downmix(x, T)
                assert same(got, W.downmix_channels(x, T)), (C, T, frames)
            m = W.peak(*W.surround_pair(x))
            n_scaled += m > 1
            n_plain += m <= 1
    assert n_scaled >= 10 and n_plain >= 10
    for C, T in ((1, 1), (1, 2), (2, 1), (2, 2), (2, 5), (8, 9)):  # narrow inputs and targets beyond the channel count
        x = rng.uniform(-1, 1, (C, 700)).astype(np.float32)
        assert same(wide.downmix(x, T), W.downmix_channels(x, T)), (C, T)
    assert wide.downmix(np.zeros((6, 0), np.float32), 2).shape == (2, 0)


@pytest.mark.parametrize("C", [3, 6, 8])
def test_downmix_peak_placement(wide, C):
    frames = 2 * SLICE + 1
    rng = np.random.default_rng(C)
    quiet = rng.uniform(-0.3, 0.3, (C, frames)).astype(np.float32)
    assert W.peak(*W.surround_pair(quiet)) < 1
    above = np.nextafter(np.float32(1), np.float32(2))
    cases = {
        "in the last frame": (0, frames - 1, 3.0),
        "in R only": (1, 5, 2.5),
        "from a negative sample": (0, 300, -1.75),
        "in the second workgroup, the rest in the first": (1, SLICE + 7, 4.0),
        "in the third workgroup through the centre channel": (2, 2 * SLICE, -3.0),
        "exactly 1.0": (0, 100, None),
        "the next float above 1.0": (0, 100, above),
    }
    for name, (c, f, v) in cases.items():
        x = quiet.copy()
        if v is None:
            x[:, f] = 0
            x[0, f] = 1.0
        elif abs(v) < 1.5:
            x[:, f] = 0
            x[c, f] = v
        else:
            x[c, f] = v
        want = W.downmix_channels(x, 2)
        m = W.peak(*W.surround_pair(x))
        assert (m == 1.0) if v is None else (m > 1.0), name
        assert same(wide.downmix(x, 2), want), name
        if v is None:
            assert np.array_equal(want, np.stack(W.surround_pair(x)))  # unscaled
    assert same(wide.downmix(np.zeros((C, frames), np.float32), 2), np.zeros((2, frames), np.float32))
    neg = -np.abs(quiet)
    neg[:, :3] = -0.0
    assert same(wide.downmix(neg, 2), W.downmix_channels(neg, 2))  # signed zeros stay what they are


@pytest.mark.parametrize("C", [3, 5, 8])
def test_downmix_nan_and_infinity(wide, C):
    frames = SLICE + 9
    rng = np.random.default_rng(40 + C)
    base = rng.uniform(-0.9, 0.9, (C, frames)).astype(np.float32)
    for name, plant in {"a NaN": [(0, 3, np.nan)], "NaNs in both and beyond the slice": [(0, 3, np.nan), (1, SLICE + 2, np.nan), (2, 9, np.nan)],
                        "+inf": [(1, 17, np.inf)], "-inf in the second workgroup": [(0, SLICE + 1, -np.inf)],
                        "inf and NaN": [(0, 1, np.inf), (1, 2, np.nan)], "inf - inf": [(0, 4, np.inf), (2, 4, -np.inf)]}.items():
        x = base.copy()
        for c, f, v in plant:
            x[c, f] = v
        for T in (1, 2, 3):
            assert same(wide.downmix(x, T), W.downmix_channels(x, T)), (name, T)
    assert np.isnan(wide.downmix(np.full((C, 5), np.nan, np.float32), 2)).all()


# ---- sources ----------------------------------------------------------------------------------------------------------------------

def encode(values, fmt):
    """[frames][C] float64 in about +-1 -> the bytes of a source in `fmt` (floats: as they are; integers: scaled to the full range)"""
    bits, is_float, be = fmt_fields(fmt)
    if is_float:
        return np.ascontiguousarray(values.astype(">f4" if be else "<f4")).tobytes()
    q = np.clip(np.round(values * (2.0 ** (bits - 1) - 1)), -(2.0 ** (bits - 1)), 2.0 ** (bits - 1) - 1).astype(np.int64)
    if bits == 24:
        b = np.ascontiguousarray((q & 0xffffff).astype("<u4")).view(np.uint8).reshape(-1, 4)[:, :3]
        return np.ascontiguousarray(b[:, ::-1] if be else b).tobytes()
    return np.ascontiguousarray(q.astype((">i" if be else "<i") + str(bits // 8))).tobytes()


def cut(data, frame_bytes, unit_frames):
    out, pos = [], 0
    for f in unit_frames:
        out.append(data[pos:pos + f * frame_bytes])
        pos += f * frame_bytes
    assert pos == len(data)
    return out


def one_at_a_time(eng, fmt, rate, ch, units, bits, out_rate, out_ch):
    """the one-stream path on `eng`: decoder.apply_output_options unit by unit, then the resampler's flush"""
    src_bits, is_float, be = fmt_fields(fmt)
    rs, out = None, []
    for u in units:
        audio = AudioData(src_bits, ch, rate, u, EncodingFlag.PCMFloat if is_float else EncodingFlag.PCMSigned,
                          Endianness.BigEndian if be else Endianness.LittleEndian)
        got, rs = decoder.apply_output_options(audio, bits, out_rate, out_ch, rs, engine=eng)
        out += [(a.bits_per_sample, a.channel_count, a.audio_format == EncodingFlag.PCMFloat, a.data.tobytes()) for a in got]
    if rs is not None:
        fl = EncodingFlag.PCMFloat if (bits == 32 and is_float) else EncodingFlag.PCMSigned
        out += [(a.bits_per_sample, a.channel_count, a.audio_format == EncodingFlag.PCMFloat, a.data.tobytes())
                for a in decoder.flush_resampler_frames(rs, bits, out_ch, fl)]
        rs.close()
    return out


def model(oracle, fmt, rate, ch, units, bits, out_rate, out_ch):
    """-> (records in the tick's form, the stage)"""
    src_bits, is_float, be = fmt_fields(fmt)
    stage = W.WideOutputStage(oracle, rate, ch, src_bits, is_float, be, bits, out_rate, out_ch)
    outs = [o for u in units for o in stage.piece(u)] + stage.flush()
    assert not any(o[4] for o in outs)
    return [(o[0], o[1], o[3], o[5]) for o in outs], stage


def records(outs):
    return [(o[0], o[1], o[2], len(o[3])) for o in outs]


# ---- the tick without a rate change -----------------------------------------------------------------------------------------------

# frames per unit: the short ones lie between long ones, so a store past a record's end hits a neighbour; even positions are loud,
# odd ones quiet (a quarter of the amplitude): the stereo branch's peak is on both sides of 1.0 in adjacent units of one stream
DIRECT_UNITS = [SLICE - 1, 1, SLICE, 2, SLICE + 1, 15, 2 * SLICE + 1, 16, SLICE - 1, 17, SLICE + 1, SLICE, 1, SLICE + 1]


def direct_source(fmt, C):
    rng = np.random.default_rng([3, fmt & ~1, C])
    frames = sum(DIRECT_UNITS)
    v = rng.uniform(-1.0, 1.0, (frames, C))
    pos = 0
    for k, f in enumerate(DIRECT_UNITS):
        if k % 2:
            v[pos:pos + f] *= 0.25
        pos += f
    if fmt >= M.FMT_F32LE:  # beyond the clamp, and what audio_data_to_f32_channels turns into zero
        v[7, 0], v[8, 1], v[SLICE + 30, C - 1] = 1.5, -1.25, 1.125
        v[40, 1], v[41, 2], v[SLICE + 3, 0] = np.inf, np.nan, -np.inf
    for a in range(C):
        for b in range(a):
            assert (v[:, a] != v[:, b]).all()  # channels pairwise different: a swapped or dropped one shows
    width = fmt_fields(fmt)[0] // 8
    return cut(encode(v, fmt), width * C, DIRECT_UNITS)


def targets(C):
    return [1, 2] + ([3] if C > 3 else []) + [C]


@pytest.fixture(scope="module")
def direct(wide):
    specs = []
    for fmt in FORMATS:
        for C in range(3, 9):
            units = direct_source(fmt, C)
            for bits in (16, 24, 32):
                for T in targets(C):
                    if not (T == C and bits == fmt_fields(fmt)[0]):  # the fast path needs no device
                        specs.append((fmt, 16000, C, units, bits, None, T))
    got = run_pcm_ticks(wide, specs, [1 + (3 * i) % 5 for i in range(len(specs))])
    return specs, got


def test_direct_against_the_model(direct, oracle):
    specs, got = direct
    assert len(specs) == 8 * (3 * 3 + 5 * 3 * 4) - 8 * 6
    both_sides = 0
    for spec, mine in zip(specs, got):
        want, stage = model(oracle, *spec)
        assert records(mine) == records(want), spec[:3] + spec[4:]
        for k, (m, w) in enumerate(zip(mine, want)):
            assert m[3] == w[3], (spec[:3] + spec[4:], "unit %d of %d frames" % (k, DIRECT_UNITS[k]))
        if spec[6] == 2:
            p = stage.peaks
            assert len(p) == len(DIRECT_UNITS)
            both_sides += any(p[k] > 1.0 and p[k + 1] < 1.0 for k in range(len(p) - 1)) and any(p[k] < 1.0 and p[k + 1] > 1.0 for k in range(len(p) - 1))
    assert both_sides == 8 * 6 * 3  # every stereo stream has a loud unit next to a quiet one, both ways round


def test_direct_against_the_one_stream_path(direct, wide):
    specs, got = direct
    for spec, mine in zip(specs, got):
        want = one_at_a_time(wide, *spec)
        assert records(mine) == records(want), spec[:3] + spec[4:]
        assert all(m[3] == w[3] for m, w in zip(mine, want)), spec[:3] + spec[4:]


# ---- the resampler on wide streams ------------------------------------------------------------------------------------------------

def rel_rms(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)) / np.sqrt(np.mean(b.astype(np.float64) ** 2)))


@pytest.mark.parametrize("in_hz", [48000, 44100])
@pytest.mark.parametrize("C", [6, 8])
def test_wide_resampler_rows_are_independent(wide, oracle, C, in_hz):
    rng = np.random.default_rng(C + in_hz)
    x = rng.uniform(-1, 1, (C, 40000)).astype(np.float32)
    x[3] = 0  # a silent row
    sizes = [997, 4096, 1, 9000, 4095, 20481 - 4096 * 2, 30000]
    ours = decoder.StreamingResampler(in_hz, 16000, C, wide)
    ref = oracle.StreamingResampler(in_hz, 16000, C)
    monos = [decoder.StreamingResampler(in_hz, 16000, 1, wide) for _ in range(C)]
    got, want, rows, pos = [], [], [[] for _ in range(C)], 0
    for size in sizes:
        blk = x[:, pos:pos + size]
        pos += blk.shape[1]
        a, b = ours.process(blk), ref.process(blk)
        assert a.shape == b.shape, (size, a.shape, b.shape)
        got.append(a), want.append(b)
        for c in range(C):
            rows[c].append(monos[c].process(blk[c:c + 1]))
    a, b = ours.flush(), ref.flush()
    assert a.shape == b.shape and a.shape[1] > 0
    got.append(a), want.append(b)
    for c in range(C):
        rows[c].append(monos[c].flush())
        monos[c].close()
    wide.reset_stream(ours.stream)  # and a reset wide stream starts over with the same bits
    again = np.concatenate([ours.process(x[:, :8192]), ours.flush()], 1)
    ours.close()
    got, want = np.concatenate(got, 1), np.concatenate(want, 1)
    assert got.shape[1] > 9000 and rel_rms(got, want) < 1e-6 and np.abs(got - want).max() < 2e-6
    for c in range(C):
        assert np.array_equal(got[c], np.concatenate(rows[c], 1)[0]), c
    assert not got[3].any()
    fresh = decoder.StreamingResampler(in_hz, 16000, C, wide)
    first = np.concatenate([fresh.process(x[:, :8192]), fresh.flush()], 1)
    fresh.close()
    assert np.array_equal(again, first)


# ---- the tick with a rate change --------------------------------------------------------------------------------------------------

INGEST_FRAMES = 4096 * 3 + 1500
INGEST_HEAD = [1, 3, 16, 17, SLICE - 1, SLICE + 1, 4097]


def ingest_unit_frames(total=INGEST_FRAMES, head=INGEST_HEAD):
    rng = np.random.default_rng(5)
    out, left = list(head), total - sum(head)
    while left > 0:
        n = min(left, int(rng.integers(1, 3001)))
        out.append(n)
        left -= n
    return out


def ingest_source(kind, fmt, C, rate, unit_frames):
    """kind: "random" (full range), "quiet" (|L|, |R| stay below 0.95 behind the resampler) or "loud" (a 440 Hz tone in phase in
    every channel: every chunk's peak is well above 1.05)"""
    frames = sum(unit_frames)
    rng = np.random.default_rng([9, C, rate, {"random": 0, "quiet": 1, "loud": 2}[kind]])
    v = rng.uniform(-1.0, 1.0, (frames, C))
    if kind == "quiet":
        v *= 0.2
    elif kind == "loud":
        tone = 0.9 * np.sin(2 * np.pi * 440.0 * np.arange(frames) / rate)
        v = 0.05 * v + tone[:, None] * (1.0 - 0.01 * np.arange(C))[None, :]
    return cut(encode(v, fmt), fmt_fields(fmt)[0] // 8 * C, unit_frames)


@pytest.mark.parametrize("in_rate", [48000, 44100])
@pytest.mark.parametrize("C", [3, 6, 8])
def test_ingest_and_pack(wide, oracle, C, in_rate):
    S16, S24BE, F32 = M.FMT_S16LE, M.FMT_S24BE, M.FMT_F32LE
    uf = ingest_unit_frames()
    T3 = 3 if C > 3 else 2
    f32_units = ingest_source("random", F32, C, in_rate, uf)
    loud_f32 = ingest_source("loud", F32, C, in_rate, uf)
    specs = [  # (format, rate, channels, units, out_bits, out_rate, out_channels)
        (F32, in_rate, C, f32_units, 32, 16000, C),   # 0: the GPU's own resampled rows, as floats
        (F32, in_rate, C, f32_units, 32, 16000, 2),   # 1 ... 3: the exact composition
        (F32, in_rate, C, f32_units, 16, 16000, 2),
        (F32, in_rate, C, f32_units, 24, 16000, 1),
        (F32, in_rate, C, loud_f32, 32, 16000, C),    # 4, 5: the same with every chunk scaled
        (F32, in_rate, C, loud_f32, 16, 16000, 2),
        (S16, in_rate, C, ingest_source("random", S16, C, in_rate, uf), 16, 16000, 1),      # 6 ... 8: the CPU chain
        (S24BE, in_rate, C, ingest_source("random", S24BE, C, in_rate, uf), 16, 16000, T3),
        (S16, in_rate, C, ingest_source("quiet", S16, C, in_rate, uf), 16, 16000, 2),
        (S24BE, in_rate, C, ingest_source("loud", S24BE, C, in_rate, uf), 16, 16000, 2),    # 9: loud
    ]
    if C == 6:  # a unit larger than a resampler row holds: cut at a multiple of kPcmCutFrames and continued in the next round
        big = [5, 20480 + 16 * 3 + 5, 700]
        specs.append((S16, in_rate, C, ingest_source("random", S16, C, in_rate, big), 16, 16000, 1))
    per_tick = [4 + i % 3 for i in range(len(specs))]
    got = run_pcm_ticks(wide, specs, per_tick)
    # (a) the one-stream path, whatever the cut
    for k, (spec, mine) in enumerate(zip(specs, got)):
        want = one_at_a_time(wide, *spec)
        assert mine and records(mine) == records(want), (k, records(mine), records(want))
        assert all(m[3] == w[3] for m, w in zip(mine, want)), k
    # (b) the model's downmix + bytes applied to the GPU's own rows, chunk by chunk, bit for bit
    for rows_at, others in ((0, (1, 2, 3)), (4, (5,))):
        rows = got[rows_at]
        assert all(r[:3] == (32, C, True) for r in rows) and len(rows) == 4
        planar = [np.frombuffer(r[3], "<f4").reshape(-1, C).T for r in rows]
        for k in others:
            bits, T = specs[k][4], specs[k][6]
            fmt = M.FMT_F32LE if bits == 32 else {16: M.FMT_S16LE, 24: M.FMT_S24LE}[bits]
            assert len(got[k]) == len(rows)
            for n, (p, mine) in enumerate(zip(planar, got[k])):
                want = oracle.f32_planar_to_bytes(fmt, W.downmix_channels(p, T)).tobytes()
                assert mine[:3] == (bits, T, bits == 32) and mine[3] == want, (k, "chunk %d" % n)
        peaks = [float(W.peak(*W.surround_pair(np.ascontiguousarray(p)))) for p in planar]
        print("\n%d channels, %d Hz, %s source: chunk peaks %s" % (C, in_rate, "loud" if rows_at else "random", ["%.3f" % p for p in peaks]))
        assert all(p > 1.05 for p in peaks) if rows_at else True
    # (c), (d) the CPU chain: records equal, samples within one LSB on at most 1 %
    for k in (6, 7, 8, 9) + ((10,) if C == 6 else ()):
        want, stage = model(oracle, *specs[k])
        label = "%d ch, %d -> 16000 Hz, stream %d -> %d ch" % (C, in_rate, k, specs[k][6])
        assert records(got[k]) == records(want), label
        if k == 8:
            assert stage.peaks and max(stage.peaks) <= 0.95, stage.peaks  # quiet: no scale is applied
        if k == 9:
            assert stage.peaks and min(stage.peaks) >= 1.05, stage.peaks  # loud: a last-bit difference cannot flip the decision
        lsb_check(b"".join(m[3] for m in got[k]), b"".join(w[3] for w in want), label)


# ---- the full device once ---------------------------------------------------------------------------------------------------------

def test_1024_wide_streams_in_one_tick(oracle):
    import soundkit_amd
    n, C, frames = 1024, 6, 4096
    rng = np.random.default_rng(6)
    unit = encode(rng.uniform(-1.0, 1.0, (frames, C)), M.FMT_S16LE)
    eng = soundkit_amd.Engine(0, n)
    try:
        eng.enable_wide_pcm(n)
        table = [{"n_units": 1, "format": M.FMT_S16LE, "channels": C, "out_bits": 16, "out_channels": 2} for _ in range(n)]
        outs = eng.tick_run_pcm(table, [unit] * n)
        want, _ = model(oracle, M.FMT_S16LE, 48000, C, [unit], 16, None, 2)
        assert len(outs) == n and [o[0] for o in outs] == list(range(n))
        assert all(o[1] == 0 and o[2:5] == (frames, 2, 16) and o[5] == outs[0][5] for o in outs)
        assert outs[0][5] == want[0][3]
        sids = [eng.open_stream(48000, C) for _ in range(n)]
        for s in sids:
            eng.resampler_open(s, 48000, 16000)
        table = [{"stream": s, "n_units": 1, "format": M.FMT_S16LE, "channels": C, "out_bits": 16, "out_channels": 1, "resample": 1, "flush": 1} for s in sids]
        outs = eng.tick_run_pcm(table, [unit] * n)
        want, _ = model(oracle, M.FMT_S16LE, 48000, C, [unit], 16, 16000, 1)
        per = len(want)
        assert per >= 1 and len(outs) == n * per
        first = outs[:per]
        assert [(16, o[3], False, len(o[5])) for o in first] == records(want)
        for i in range(n):
            mine = outs[i * per:(i + 1) * per]
            assert all(o[0] == i and o[1] == 0 for o in mine) and [o[5] for o in mine] == [o[5] for o in first], i
        lsb_check(b"".join(o[5] for o in first), b"".join(w[3] for w in want), "1024 x 6 ch -> 16 kHz mono")
    finally:
        eng.close()

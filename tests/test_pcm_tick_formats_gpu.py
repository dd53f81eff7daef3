"""The PCM tick (sk_tick_run_pcm: k_pcm_direct, k_pcm_ingest) on every input format, mono and stereo, on extreme values and on the unit
lengths its kernels branch on.  test_pcm_pipeline_gpu.py runs one speech recording in five shapes; here every input is synthetic:

* sources(): SK_FMT_S16LE ... SK_FMT_F32BE x {1, 2} channels, full-range random values per channel (left never equals right, so a
  swapped, doubled or dropped channel changes the output) with each format's extreme values planted in both channels -- once inside
  whole 16-sample groups, once in units' last incomplete groups, once on each side of a 4096-sample slice boundary;
* k_pcm_direct: every source to 16 / 24 / 32 bits, same channels and mono, all streams side by side in the same ticks, units of
  1 ... 12289 samples with the short ones between long ones: every record equal to the CPU chain's (pcm_worker_model.OutputStage on
  the C oracle) and to the one-stream path's (decoder.apply_output_options: pcm.hip's kernels);
* k_pcm_ingest: every source as 48 -> 16 kHz (the fixed FIR) and 44.1 -> 16 kHz (the generic resampler) over several ticks: equal to
  the one-stream path whatever the cut; to 16 bits within one LSB on at most 1 % of the samples of the CPU chain (lsb_check, the bound
  this resampler is held to everywhere); a silent channel stays silent on its own side;
* stereo 24- / 32-bit / float WAV files (one WAVE_FORMAT_EXTENSIBLE) and raw PCM streams through the scheduler against the model."""
import struct

import numpy as np
import pytest

import pcm_worker_model as M
import twin_fit
from pcm_worker_model import OutputStage, ragged, raw_worker, wav_worker
from test_pcm_pipeline_gpu import as_model, fmt_fields, lsb_check, one_at_a_time, run_pcm_ticks, through_scheduler, wav_file

pytestmark = pytest.mark.gpu

FORMATS = list(range(M.FMT_S16LE, M.FMT_F32BE + 1))
OUT_OPTIONS = [(bits, out_ch) for bits in (16, 24, 32) for out_ch in (None, 1)]

# ---- synthetic sources ------------------------------------------------------------------------------------------------------------

S16_SET = [0x8000, 0x7fff, 0x0000, 0x0001, 0xffff, 0x00ff, 0xff00]  # -32768, 32767, 0, 1, -1, 255, -256
# the last five tell an arithmetic shift from a logical one and a truncation from a rounding in exact_sample_to_i16
S24_SET = [0x800000, 0x7fffff, 0x000000, 0xffffff, 0x0000ff, 0xffff00, 0xfffeff, 0x007fff, 0x008000]
S32_SET = [0x80000000, 0x7fffffff, 0xffffffff, 0x0000ffff, 0xffff0000, 0xfffeffff, 0x00008000, 0x7fff8000]


def f32_set(wild):
    """bit patterns: signed zeros, +-1 and its neighbour, beyond the clamp, infinities, a quiet and a signalling NaN, subnormals, and
    the rounding ties of float_sample_to_i16 and of the 24-bit scaling; `wild` adds +-1e30 (finite, so it would go through the filter)"""
    above = np.nextafter(np.float32(1), np.float32(2))
    vals = [0.0, -0.0, 1.0, -1.0, above, -above, 1.5, -1.5, np.inf, -np.inf] + ([1e30, -1e30] if wild else [])
    for k in (0, 1, 12345, 32766):
        vals += [(k + 0.5) / 32767, -(k + 0.5) / 32768]
    for k in (0, 4194303):
        vals += [(k + 0.5) / 8388607, -(k + 0.5) / 8388608]
    bits = [int(b) for b in np.array(vals, np.float64).astype(np.float32).view(np.uint32)]
    return bits + [0x7fc00001, 0x7f800001, 0x00000001, 0x807fffff]  # quiet NaN, signalling NaN, smallest subnormal, largest (negative)


def planted_set(fmt, wild):
    if fmt >= M.FMT_F32LE:
        return f32_set(wild)
    return {16: S16_SET, 24: S24_SET, 32: S32_SET}[fmt_fields(fmt)[0]]


def make_source(fmt, ch, unit_frames, wild, seed=0):
    """-> (bytes, coverage) of a source of sum(unit_frames) frames that will be cut into units of unit_frames.
    coverage[where] = the (channel, value) pairs planted: where = "group" (whole 16-sample groups of the longest unit), "before" /
    "after" (the last samples before and the first after that unit's 4096-sample slice boundary), "tail" (units' last incomplete groups)"""
    width = fmt_fields(fmt)[0] // 8
    is_float = fmt >= M.FMT_F32LE
    rng = np.random.default_rng([seed, fmt & ~1, ch])  # (a big-endian source is its little-endian twin byte-swapped)
    frames = int(sum(unit_frames))
    if is_float:
        w = rng.uniform(-1.25, 1.25, (frames, ch)) if wild else rng.uniform(-1.0, 1.0, (frames, ch))
        w = np.ascontiguousarray(w.astype(np.float32)).view(np.uint32).copy()
    else:
        w = rng.integers(0, 1 << (8 * width), (frames, ch), dtype=np.uint64).astype(np.uint32)
    P = planted_set(fmt, wild)
    n = len(P)
    assert len(set(P)) == n
    cover = {"group": set(), "before": set(), "after": set(), "tail": set()}

    def plant(where, frame, count, phase):  # left runs through P from `phase`, right one step ahead: both see every value, never the same one
        for k in range(count):
            for c in range(ch):
                v = P[(phase + k + c) % n]
                w[frame + k, c] = v
                cover[where].add((c, v))
        return phase + count

    starts = np.concatenate([[0], np.cumsum(unit_frames)]).astype(np.int64)
    big = int(np.argmax(unit_frames))
    assert unit_frames[big] * ch >= 4096 + n * ch and 32 + n * ch <= 4096 - n * ch
    plant("group", starts[big] + 32 // ch, n, 0)
    plant("before", starts[big] + 4096 // ch - n, n, 0)
    plant("after", starts[big] + 4096 // ch, n, 0)
    phase = 0
    for u, f in enumerate(unit_frames):
        tail = (f * ch % 16) // ch
        phase = plant("tail", starts[u] + f - tail, tail, phase)
    assert all(len(c) == n * ch for c in cover.values()), {k: len(c) for k, c in cover.items()}
    if ch == 2:
        same = w[:, 0] == w[:, 1]
        w[same, 1] ^= 1
        assert not (w[:, 0] == w[:, 1]).any()
    data = np.ascontiguousarray(w.astype("<u4").reshape(-1, 1).view(np.uint8)[:, :width]).ravel()
    if fmt & 1:
        data = twin_fit.swap_bytes(data, width)
    return data.tobytes(), cover


def cut(data, frame_bytes, unit_frames):
    out, pos = [], 0
    for f in unit_frames:
        out.append(data[pos:pos + f * frame_bytes])
        pos += f * frame_bytes
    assert pos == len(data)
    return out


def records(outs):
    return [(o[0], o[1], o[2], len(o[3])) for o in outs]


def model_records(outs):
    """OutputStage's (bits, channels, rate, is_float, big_endian, bytes) in the tick's form"""
    assert not any(o[4] for o in outs)
    return [(o[0], o[1], o[3], o[5]) for o in outs]


# ---- k_pcm_direct: no rate change -----------------------------------------------------------------------------------------------

# samples per unit (frames x channels): around the 16-sample group, the 4096-sample slice and its multiples; every short unit but the
# first and the last lies directly between two long ones, so a whole-group store or a tail running past its record hits a neighbour
SHORT = {1: [33, 1, 2, 7, 8, 15, 16, 17, 31, 32], 2: [17, 1, 2, 3, 4, 7, 8, 9, 15, 16]}  # frames
LONG = {1: [4080, 4095, 4096, 4097, 4112, 8191, 8192, 8193, 12289], 2: [2040, 2047, 2048, 2049, 2056, 4095, 4096, 4097, 6145]}


def direct_unit_frames(ch):
    out = []
    for k, s in enumerate(SHORT[ch]):
        out.append(s)
        if k < len(LONG[ch]):
            out.append(LONG[ch][k])
    return out


def is_fast_path(fmt, ch, bits, out_ch):
    return bits == fmt_fields(fmt)[0] and (out_ch or ch) == ch


@pytest.fixture(scope="module")
def direct(engine):
    """all 16 sources x every (out_bits, out_channels) that is not the fast path, side by side in the same ticks.
    -> [(fmt, ch, units, bits, out_ch, the tick's outputs)]"""
    specs = []
    for fmt in FORMATS:
        for ch in (1, 2):
            frames = direct_unit_frames(ch)
            data, _ = make_source(fmt, ch, frames, wild=True)
            units = cut(data, fmt_fields(fmt)[0] // 8 * ch, frames)
            for bits, out_ch in OUT_OPTIONS:
                if not is_fast_path(fmt, ch, bits, out_ch):
                    specs.append((fmt, 16000, ch, units, bits, None, out_ch))
    got = run_pcm_ticks(engine, specs, [1 + (3 * i) % 4 for i in range(len(specs))])
    return [(s[0], s[2], s[3], s[4], s[6], g) for s, g in zip(specs, got)]


def test_sources_cover_what_they_claim():
    """the generator itself: every planted value in every channel at each of the four places, for the direct and the resampling
    layouts (make_source asserts it); short units between long ones; left never equals right"""
    for ch in (1, 2):
        frames = direct_unit_frames(ch)
        samples = [f * ch for f in frames]
        asked = [1, 2, 7, 8, 15, 16, 17, 31, 32, 33, 4080, 4095, 4096, 4097, 4112, 8191, 8192, 8193, 12289]
        assert all(n in samples or (ch == 2 and n % 2 and (n - 1 in samples or n + 1 in samples)) for n in asked)  # (stereo: an even neighbour)
        assert sum(1 for k in range(1, len(samples) - 1) if samples[k] <= 18 and min(samples[k - 1], samples[k + 1]) >= 4080) >= 7
        for fmt in FORMATS:
            _, cover = make_source(fmt, ch, frames, wild=True)
            assert all(len(c) == ch * len(planted_set(fmt, True)) for c in cover.values())
            make_source(fmt, ch, ingest_unit_frames(ch), wild=False)


def test_fast_path_is_refused(engine):
    """nothing to convert: the scheduler delivers such pieces as they are, and the tick refuses the stream"""
    from soundkit_amd._lib import SoundkitError
    for fmt in FORMATS:
        for ch in (1, 2):
            bits = fmt_fields(fmt)[0]
            with pytest.raises(SoundkitError) as exc:
                engine.tick_run_pcm([{"n_units": 1, "format": fmt, "channels": ch, "out_bits": bits, "out_channels": ch}], [bytes(bits // 8 * ch * 40)])
            assert exc.value.status == -1


def test_direct_against_the_cpu_chain(direct, oracle):
    for fmt, ch, units, bits, out_ch, mine in direct:
        src_bits, is_float, be = fmt_fields(fmt)
        stage = OutputStage(oracle, 16000, ch, src_bits, is_float, be, bits, None, out_ch)
        want = model_records([o for u in units for o in stage.piece(u)])
        assert records(mine) == records(want), (fmt, ch, bits, out_ch)
        for k, (m, w) in enumerate(zip(mine, want)):
            assert m[3] == w[3], (fmt, ch, bits, out_ch, "unit %d of %d frames" % (k, len(units[k]) // (src_bits // 8 * ch)))


def test_direct_against_the_one_stream_path(direct):
    for fmt, ch, units, bits, out_ch, mine in direct:
        want = one_at_a_time(fmt, 16000, ch, units, bits, None, out_ch)
        assert records(mine) == records(want), (fmt, ch, bits, out_ch)
        for k, (m, w) in enumerate(zip(mine, want)):
            assert m[3] == w[3], (fmt, ch, bits, out_ch, k)


def test_direct_covers_every_path(direct):
    """what the streams of `direct` contain by construction, and the record shape each path must give"""
    seen = {}
    for fmt, ch, units, bits, out_ch, mine in direct:
        assert len(mine) == len(units) == 19
        seen[(fmt, ch, bits, out_ch or ch)] = mine
    S16, S24, S32, F32 = M.FMT_S16LE, M.FMT_S24LE, M.FMT_S32LE, M.FMT_F32LE
    count = 0
    for base in (S24, S32, F32):  # stereo -> mono at every depth, both byte orders
        for fmt in (base, base + 1):
            for bits in (16, 24, 32):
                float_out = base == F32 and bits == 32
                assert all(m[:3] == (bits, 1, float_out) for m in seen[(fmt, 2, bits, 1)])
                count += 1
    for fmt in (S24, S24 + 1, S32, S32 + 1):  # the exact path: stereo in, 16 bits, both channels kept
        assert all(m[:3] == (16, 2, False) for m in seen[(fmt, 2, 16, 2)])
        count += 1
    for fmt in (S16, S16 + 1):
        assert all(m[:3] == (24, 1, False) for m in seen[(fmt, 2, 24, 1)])  # the downmix with 24 bytes per lane
        count += 1
        for bits in (24, 32):
            assert all(m[:3] == (bits, 1, False) for m in seen[(fmt, 1, bits, 1)])
            count += 1
    for fmt in (F32, F32 + 1):  # mono float with the wild values down to integers
        for bits in (16, 24):
            assert all(m[:3] == (bits, 1, False) for m in seen[(fmt, 1, bits, 1)])
            count += 1
    print("\ndirect: %d streams in the same ticks, %d distinct (format, channels, out_bits, out_channels), %d required combinations present"
          % (len(direct), len(seen), count))
    assert len(direct) == 72 and len(seen) == 56 and count == 32


# ---- k_pcm_ingest: rate change ------------------------------------------------------------------------------------------------------

INGEST_FRAMES = 60000
# 1, 3, 17: the stream's fill, where the next unit's rows start, goes through every 4-byte alignment; 2047 / 2049 and 4095 / 4097: around
# the 4096-sample slice for two channels and for one; 20 480 + 16 * 3 + 5: more than a row's five chunks hold, so it is cut at a
# multiple of kPcmCutFrames and continued in the next round
INGEST_HEAD = [1, 3, 16, 17, 2047, 2049, 20480 + 16 * 3 + 5, 4095, 4097]
SHORT_HEAD = [1, 3, 16, 17, 2047, 2049, 4097]  # for the shorter sources


def ingest_unit_frames(ch, total=INGEST_FRAMES, head=INGEST_HEAD):
    rng = np.random.default_rng([5, ch])
    out, left = list(head), total - sum(head)
    while left > 0:
        n = min(left, int(rng.integers(1, 4001)))
        out.append(n)
        left -= n
    return out


def ingest_specs(in_rate, bits, out_ch):
    specs = []
    for fmt in FORMATS:
        for ch in (1, 2):
            frames = ingest_unit_frames(ch)
            data, _ = make_source(fmt, ch, frames, wild=False)
            specs.append((fmt, in_rate, ch, cut(data, fmt_fields(fmt)[0] // 8 * ch, frames), bits, 16000, out_ch))
    return specs


@pytest.mark.parametrize("bits,out_ch", OUT_OPTIONS)
@pytest.mark.parametrize("in_rate", [48000, 44100])
def test_ingest_every_format(engine, oracle, in_rate, bits, out_ch):
    """all 16 sources side by side through the resampler, over at least three ticks with the flush in the last: the one-stream path's
    records and bytes; to 16 bits the CPU chain's records, and its samples within lsb_check's bound"""
    specs = ingest_specs(in_rate, bits, out_ch)
    per_tick = [5 + i % 3 for i in range(len(specs))]
    assert all(len(s[3]) > 2 * p for s, p in zip(specs, per_tick))  # rs_fill is carried over at least twice
    got = run_pcm_ticks(engine, specs, per_tick)
    for spec, mine in zip(specs, got):
        fmt, _, ch, units = spec[:4]
        src_bits, is_float, be = fmt_fields(fmt)
        label = "format %d, %d ch, %d -> 16000 Hz, %d bits, %d ch" % (fmt, ch, in_rate, bits, out_ch or ch)
        assert mine and all(m[:3] == (bits, out_ch or ch, is_float and bits == 32) for m in mine), label
        want = one_at_a_time(*spec)
        assert records(mine) == records(want), label
        for k, (m, w) in enumerate(zip(mine, want)):
            assert m[3] == w[3], (label, k)
        if bits == 16:
            stage = OutputStage(oracle, in_rate, ch, src_bits, is_float, be, 16, 16000, out_ch)
            cpu = model_records([o for u in units for o in stage.piece(u)] + stage.flush())
            assert records(mine) == records(cpu), label
            lsb_check(b"".join(m[3] for m in mine), b"".join(c[3] for c in cpu), label)


def test_ingest_keeps_the_channels_apart(engine):
    """a stereo source with one channel silent, and its mirror: the 16-bit stereo output is zero exactly on the silent side, whatever
    the references say"""
    frames = ingest_unit_frames(2)
    specs, silent = [], []
    for in_rate in (48000, 44100):
        for fmt in (M.FMT_S16BE, M.FMT_S24LE, M.FMT_S24BE, M.FMT_S32BE, M.FMT_F32LE):
            width = fmt_fields(fmt)[0] // 8
            data, _ = make_source(fmt, 2, frames, wild=False, seed=1)
            for side in (0, 1):
                a = np.frombuffer(data, np.uint8).reshape(-1, 2, width).copy()
                a[:, side, :] = 0
                specs.append((fmt, in_rate, 2, cut(a.tobytes(), 2 * width, frames), 16, 16000, None))
                silent.append(side)
    got = run_pcm_ticks(engine, specs, [5 + i % 3 for i in range(len(specs))])
    for spec, side, mine in zip(specs, silent, got):
        y = np.frombuffer(b"".join(m[3] for m in mine), "<i2").reshape(-1, 2)
        assert all(m[:3] == (16, 2, False) for m in mine) and y.shape[0] > 15000, spec[:2]
        assert not y[:, side].any(), (spec[:2], side)
        assert (y[:, 1 - side] != 0).mean() > 0.99, (spec[:2], side)


# ---- through the scheduler ----------------------------------------------------------------------------------------------------------

def wav_extensible(channels, rate, bits, pcm):
    """WAVE_FORMAT_EXTENSIBLE: the 40-byte `fmt ` chunk with the PCM sub-format GUID"""
    guid = struct.pack("<IHH", 1, 0, 0x0010) + bytes([0x80, 0x00, 0x00, 0xaa, 0x00, 0x38, 0x9b, 0x71])
    fmt = struct.pack("<HHIIHHHHI", 0xfffe, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits, 22, bits, 3) + guid
    assert len(fmt) == 40
    return b"RIFF" + struct.pack("<I", 60 + len(pcm)) + b"WAVEfmt " + struct.pack("<I", 40) + fmt + b"data" + struct.pack("<I", len(pcm)) + pcm


def test_stereo_formats_through_the_scheduler(engine, oracle):
    """14 streams in ragged chunks: stereo 24-bit, 32-bit, float and WAVE_FORMAT_EXTENSIBLE 24-bit WAV files and raw S24BE / F32BE / S32LE
    stereo, each under two of the five options: the model's records, info and bytes (the resampled ones within lsb_check's bound)"""
    from soundkit_amd import pipeline
    rng = np.random.default_rng(77)
    rate = 48000
    frames = ingest_unit_frames(2, 20000, SHORT_HEAD)

    def pcm(fmt):
        return make_source(fmt, 2, frames, wild=False, seed=2)[0]
    sources = [("wav", wav_file(2, rate, 24, pcm(M.FMT_S24LE))), ("wav", wav_file(2, rate, 32, pcm(M.FMT_S32LE))),
               ("wav", wav_file(2, rate, 32, pcm(M.FMT_F32LE), tag=3)), ("wav", wav_extensible(2, rate, 24, pcm(M.FMT_S24LE))),
               (M.FMT_S24BE, pcm(M.FMT_S24BE)), (M.FMT_F32BE, pcm(M.FMT_F32BE)), (M.FMT_S32LE, pcm(M.FMT_S32LE))]
    options = [(16, None, 1), (24, None, 1), (32, None, 1), (16, None, None), (16, 16000, 1)]
    streams, want, opts = [], [], []
    for k in range(14):
        kind, data = sources[k % 7]
        bits, out_rate, out_ch = options[k % 5]
        chunks = ragged(data, rng, 1, 40000)
        opt = pipeline.DecodeOptions(bits, out_rate, out_ch)
        if kind == "wav":
            streams.append((None, opt, chunks))
            want.append(wav_worker(oracle, chunks, bits, out_rate, out_ch))
        else:
            streams.append((pipeline.RawPcmFormat(rate, 2, kind), opt, chunks))
            want.append(raw_worker(oracle, chunks, rate, 2, kind, bits, out_rate, out_ch))
        opts.append(options[k % 5])
    assert {(k % 7, k % 5) for k in range(14)} >= {(s, 4) for s in (4, 2)}  # a WAV and a raw stream are resampled
    outs = through_scheduler(engine, streams)
    for k, (exp, exp_err) in enumerate(want):
        got, err = as_model(outs[k])
        assert err == exp_err is None, (k, err, exp_err)
        assert exp and [g[:5] + (len(g[5]),) for g in got] == [w[:5] + (len(w[5]),) for w in exp], k
        if opts[k][1]:
            lsb_check(b"".join(g[5] for g in got), b"".join(w[5] for w in exp), "stream %d" % k)
        else:
            assert all(g[5] == w[5] for g, w in zip(got, exp)), k

"""Plain float64 references of the GPU kernels' operations, vectorised over streams and rows (numpy / scipy on the CPU).

TEST INFRASTRUCTURE ONLY, imported by the tests the way kernel_model.py is.  Every constant is the oracle's, taken as f64:
the windows (oracle.sine_window, oracle.kbd_window: long alpha 4, short alpha 6), the 48 -> 16 kHz taps and the generic-ratio
sub-filters (oracle.resampler_taps / resampler_sincs).  Only the arithmetic differs from the oracle: every sum is in float64,
so these functions measure how far a kernel (or the f32 oracle) is from the exact operation.  tests/test_f64_ref.py pins each
one against the C oracle.

Large batches go through in chunks (CHUNK_ROWS rows at a time) so that host memory stays within a few GB; the FFTs use at most
WORKERS threads.
"""
import os

import numpy as np
import scipy.fft as sfft

from oracle import oracle as O

WORKERS = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS") or 16), len(os.sched_getaffinity(0))))
CHUNK_ROWS = 512
FIR_DELAY = 125  # y[m] = sum_p taps[p] x[3m - 125 + p]: rubato's 128-frame delay after downsample_audio's trim, at ratio 1/3


def rel_rms(got, want):
    want = np.asarray(want, np.float64)
    return float(np.sqrt(np.mean((np.asarray(got, np.float64) - want) ** 2) / np.mean(want ** 2)))


# ---- IMDCT -------------------------------------------------------------------------------------------------------------

def imdct(x, workers=None):
    """[..., N] -> [..., 2N] float64: y[s] = (1/32768/N) sum_k x[k] cos(pi/(4N) (2s+1+N)(2k+1)) (dsp.rs:453-474, in f64).
    One complex inverse FFT of length 2N per transform; the twiddle phases are reduced exactly in integers first."""
    x = np.asarray(x)
    n = x.shape[-1]
    k = np.arange(n)
    # (2s+1+N)(2k+1) pi/(4N) = pi (2s+1+N)/(4N) + 2 pi s k/(2N) + pi (N+1) k/(2N)
    pre = np.exp(2j * np.pi * (((n + 1) * k) % (4 * n)) / (4 * n))
    s = np.arange(2 * n)
    post = np.exp(2j * np.pi * (2 * s + 1 + n) / (8 * n)) * (2 * n) / 32768.0 / n
    y = sfft.ifft(x.astype(np.float64) * pre, n=2 * n, axis=-1, workers=workers or WORKERS)
    return (y * post).real


# ---- AAC synthesis -----------------------------------------------------------------------------------------------------

_WIN = {}


def windows():
    """(first[seq][prev_shape][1024], second[seq][shape][1024], short[shape][256]) in f64: dsp.rs:353-387's window halves of
    the long-transform sequences (row 2, EightShort, unused) and the two short windows"""
    if not _WIN:
        long_w = np.stack([O.sine_window(2048), O.kbd_window(2048, 4.0)]).astype(np.float64)
        short_w = np.stack([O.sine_window(256), O.kbd_window(256, 6.0)]).astype(np.float64)
        first = np.zeros((4, 2, 1024))
        second = np.zeros((4, 2, 1024))
        for sh in (0, 1):
            first[O.ONLY_LONG, sh] = first[O.LONG_START, sh] = long_w[sh, :1024]
            first[O.LONG_STOP, sh, 448:576] = short_w[sh, :128]
            first[O.LONG_STOP, sh, 576:] = 1.0
            second[O.ONLY_LONG, sh] = second[O.LONG_STOP, sh] = long_w[sh, 1024:]
            second[O.LONG_START, sh, :448] = 1.0
            second[O.LONG_START, sh, 448:576] = short_w[sh, 128:]
        _WIN.update(first=first, second=second, short=short_w)
    return _WIN["first"], _WIN["second"], _WIN["short"]


def synthesize(coeffs, seqs, shapes, delay=None, prev_shape=None, win=None, workers=None):
    """AAC-LC synthesis of independent channels (dsp.rs:230-338 as the oracle restates it), float64.

    coeffs [C][F][1024] (f32 values), seqs / shapes [C][F] -> (pcm [C][F][1024] f64, delay [C][1024], prev_shape [C]).
    delay / prev_shape: the carried state before frame 0 (default: a fresh channel, zeros and Sine).
    win: (first, second, short) in place of windows() -- the negative controls change one coefficient.
    workers: FFT threads (default WORKERS; 1 when the caller runs chunks on a thread pool of its own)."""
    coeffs = np.asarray(coeffs)
    c, f, _ = coeffs.shape
    seqs = np.asarray(seqs).reshape(c, f)
    shapes = np.asarray(shapes).reshape(c, f).astype(np.intp)
    first, second, short = win if win is not None else windows()
    delay = np.zeros((c, 1024)) if delay is None else np.array(delay, np.float64)
    prev = np.zeros(c, np.intp) if prev_shape is None else np.asarray(prev_shape, np.intp).copy()
    out = np.empty((c, f, 1024))
    for fr in range(f):
        sq, sh = seqs[:, fr].astype(np.intp), shapes[:, fr]
        lng = np.nonzero(sq != O.EIGHT_SHORT)[0]
        if lng.size:
            y = imdct(coeffs[lng, fr], workers)
            out[lng, fr] = y[:, :1024] * first[sq[lng], prev[lng]] + delay[lng]
            delay[lng] = y[:, 1024:] * second[sq[lng], sh[lng]]
        srt = np.nonzero(sq == O.EIGHT_SHORT)[0]
        if srt.size:
            y = imdct(coeffs[srt, fr].reshape(-1, 8, 128), workers)  # [c][window][256]
            cur = short[sh[srt]]
            y[:, 0, :128] *= short[prev[srt], :128]
            y[:, 0, 128:] *= cur[:, 128:]
            y[:, 1:] *= cur[:, None, :]
            buf = np.zeros((srt.size, 2048))
            for w in range(8):
                buf[:, 448 + 128 * w:704 + 128 * w] += y[:, w]
            out[srt, fr] = buf[:, :1024] + delay[srt]
            delay[srt] = buf[:, 1024:]
        prev = sh.copy()
    return out, delay, prev


# ---- s16 narrowing -----------------------------------------------------------------------------------------------------

def float_sample_to_i16(x):
    """soundkit-decoder lib.rs:1815-1827 vectorised: clamp to [-1, 1] in f32 (non-finite -> 0), scale by 32768 below zero and
    32767 above in f64, round half away from zero, saturate.  The f64 product of an f32 and a 15-bit integer is exact, so
    floor(|v| + 0.5) is C's round() on it."""
    x = np.asarray(x, np.float32)
    finite = np.where(np.isfinite(x), np.clip(x, np.float32(-1.0), np.float32(1.0)), np.float32(0.0)).astype(np.float64)
    scaled = np.where(finite < 0.0, finite * 32768.0, finite * 32767.0)
    r = np.copysign(np.floor(np.abs(scaled) + 0.5), scaled)
    return np.clip(r, -32768, 32767).astype(np.int16)


def float_sample_to_i16_torch(x):
    """the same rounding on a torch tensor (f32 in, int16 out), in f64 where it scales: checks a whole device batch in place"""
    import torch
    f = torch.where(torch.isfinite(x), x.clamp(-1.0, 1.0), torch.zeros_like(x)).double()
    s = torch.where(f < 0, f * 32768.0, f * 32767.0)
    return (torch.sign(s) * torch.floor(s.abs() + 0.5)).clamp(-32768, 32767).to(torch.int16)


# ---- 48 -> 16 kHz FIR --------------------------------------------------------------------------------------------------

def fir_48k_16k(x, n_out, taps=None, delay=FIR_DELAY, workers=None):
    """downsample_audio 48 -> 16 kHz in f64: y[m] = sum_p taps[p] x[3m - delay + p], zero outside the row.
    x [R][T] -> [R][n_out].  Polyphase: three decimated correlations of 86 taps, summed in the frequency domain."""
    x = np.asarray(x)
    workers = workers or WORKERS
    taps = (O.resampler_taps(16000 / 48000) if taps is None else np.asarray(taps)).astype(np.float64)
    r, t = x.shape
    h = np.zeros(258)
    h[:taps.size] = taps
    hp = h.reshape(86, 3)[::-1]  # [85 - q][phase]
    u_len = n_out + 86
    length = sfft.next_fast_len(u_len, real=True)
    hf = sfft.rfft(hp, n=length, axis=0, workers=workers).T  # [phase][freq]
    out = np.empty((r, n_out))
    for a in range(0, r, CHUNK_ROWS):
        b = min(r, a + CHUNK_ROWS)
        xp = np.zeros((b - a, 3 * u_len))
        lo, hi = max(0, -delay), min(t, 3 * u_len - delay)
        xp[:, delay + lo:delay + hi] = x[a:b, lo:hi]
        u = xp.reshape(b - a, u_len, 3)
        acc = None
        for p in range(3):
            term = sfft.rfft(u[:, :, p], n=length, axis=1, workers=workers) * hf[p]
            acc = term if acc is None else acc + term
        out[a:b] = sfft.irfft(acc, n=length, axis=1, workers=workers)[:, 85:85 + n_out]
    return out


def s16_chain(pcm16_planar, n_out, workers=None):
    """the worker's resample step on s16 rows: s / 32768 -> the f64 FIR.  pcm16 [R][T] int16 -> [R][n_out] f64"""
    return fir_48k_16k(np.asarray(pcm16_planar).astype(np.float64) / 32768.0, n_out, workers=workers)


def fir_48k_16k_at(x, cols, taps=None, block=256):
    """the same filter at the output columns `cols` only (direct f64 dot products): x [R][T] -> [R][len(cols)].
    Rows go through `block` at a time; each is widened to f64 with the FIR_DELAY zeros in front and 256 behind."""
    x = np.asarray(x)
    taps = (O.resampler_taps(16000 / 48000) if taps is None else np.asarray(taps)).astype(np.float64)
    cols = np.asarray(cols, np.int64)
    idx = 3 * cols[:, None] + np.arange(256)[None, :]
    out = np.empty((x.shape[0], cols.size))
    for a in range(0, x.shape[0], block):
        xb = x[a:a + block]
        xp = np.zeros((xb.shape[0], FIR_DELAY + xb.shape[1] + 256))
        xp[:, FIR_DELAY:FIR_DELAY + xb.shape[1]] = xb
        out[a:a + block] = xp[:, idx] @ taps
    return out


# ---- generic-ratio resampler (rubato SincFixedIn, Linear) ---------------------------------------------------------------

def sinc_resample(x, in_hz, out_hz, sincs=None, out_block=1024):
    """oracle/sk_oracle.c's sko_downsample_planar (one chunk of the whole row, fresh state) with the same sub-filter table,
    the same f64 time index accumulated step by step, the same sub-filter pair and f32 interpolation fraction; only the two
    256-tap dot products and the interpolation are evaluated in float64.  x [R][T] -> [R][n]."""
    x = np.asarray(x, np.float32)
    r, t = x.shape
    ratio = out_hz / in_hz
    sincs = (O.resampler_sincs(ratio) if sincs is None else np.asarray(sincs)).astype(np.float64)
    t_ratio = 1.0 / ratio
    end_idx = t - 257 - int(np.ceil(t_ratio))
    n_max = int((end_idx + 128) * ratio) + 4
    idx = np.add.accumulate(np.concatenate([[-128.0], np.full(n_max + 1, t_ratio)]))  # sequential, as `idx += t_ratio`
    n = int(np.searchsorted(idx, end_idx, side="left"))  # outputs while the index before the step is below end_idx
    idx = idx[1:n + 1]
    fl = np.floor(idx)
    index0 = fl.astype(np.int64)
    sub0 = np.floor((idx - fl) * 256.0).astype(np.int64)
    sub1 = sub0 + 1
    index1 = index0 + (sub1 >= 256)
    sub1 = np.where(sub1 >= 256, sub1 - 256, sub1)
    scaled = idx * 256.0
    frac = (scaled - np.floor(scaled)).astype(np.float32).astype(np.float64)
    xp = np.concatenate([np.zeros((r, 512)), x.astype(np.float64), np.zeros((r, 512))], axis=1)  # buf[i + 512] = x[i]
    out = np.empty((r, n))
    j = np.arange(256)
    for a in range(0, n, out_block):
        b = min(n, a + out_block)
        w0 = xp[:, (index0[a:b, None] + 512 + j)]  # [R][outputs][256]
        w1 = xp[:, (index1[a:b, None] + 512 + j)]
        p0 = np.einsum("rnj,nj->rn", w0, sincs[sub0[a:b]])
        p1 = np.einsum("rnj,nj->rn", w1, sincs[sub1[a:b]])
        out[:, a:b] = p0 + frac[a:b] * (p1 - p0)
    return out



# ---- MP3: requantisation and the hybrid synthesis filterbank ---------------------------------------------------------------

def _requant_chunk(args):
    from oracle import mp3_bitstream
    granules, quant, long_o, short_o, pretab = args
    out, at = [], 0
    for g in granules:
        out.append(mp3_bitstream.requantize_granule(g, quant[at:at + g["channels"]], long_o, short_o, pretab))
        at += g["channels"]
    return np.concatenate(out)


def mp3_requant(granules, quant, long_o, short_o, pretab, processes=None):
    """ISO/IEC 11172-3 2.4.3.4.7-9 in f64 as oracle/mp3_bitstream.py requantize_granule states it (requantisation, mid/side,
    intensity stereo, short-block reorder), over many granules: chunks on at most WORKERS fresh processes (the oracle is
    per-line Python; the processes never touch a GPU).  quant: the granules' channels one after another -> xr f64 alike."""
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    starts = np.concatenate([[0], np.cumsum([g["channels"] for g in granules])])
    step = max(1, len(granules) // (4 * (processes or WORKERS)))
    jobs = [(granules[a:a + step], quant[starts[a]:starts[min(a + step, len(granules))]], long_o, short_o, pretab)
            for a in range(0, len(granules), step)]
    with ProcessPoolExecutor(processes or WORKERS, mp_context=multiprocessing.get_context("spawn")) as ex:
        return np.concatenate(list(ex.map(_requant_chunk, jobs)))


_MP3 = {}


def _mp3_tables():
    if not _MP3:
        from oracle import mp3_hybrid as M
        i36, k18 = np.arange(36)[:, None], np.arange(18)[None, :]
        i12, k6 = np.arange(12)[:, None], np.arange(6)[None, :]
        u_idx = np.concatenate([np.r_[128 * i:128 * i + 32, 128 * i + 96:128 * i + 128] for i in range(8)])
        boundaries = np.array([(18 * sb - 1 - i, 18 * sb + i, i, sb) for sb in range(1, 32) for i in range(8)])
        _MP3.update(m36=np.cos(np.pi / 72 * (2 * i36 + 1 + 18) * (2 * k18 + 1)), m12=np.cos(np.pi / 24 * (2 * i12 + 1 + 6) * (2 * k6 + 1)),
                    win=np.stack([M.block_window(b) for b in (0, 1, 3)]), win12=M.block_window(2), cs=M.CS, ca=M.CA,
                    matrix=M.MATRIX, u_idx=u_idx, boundaries=boundaries)
    return _MP3


def mp3_hybrid(xr, block_types, mixed, d512, overlap=None, v=None):
    """oracle/mp3_hybrid.py Channel.granule vectorised over channels (alias reduction, IMDCT 36 / 3 x 12, block windows,
    overlap-add, frequency inversion, polyphase synthesis with window d512), float64.
    xr [C][G][576] in the hybrid's line order, block_types / mixed [C][G] -> (pcm [C][G][576], overlap [C][32][18], v [C][1024])."""
    t = _mp3_tables()
    xr = np.asarray(xr, np.float64)
    c, n_gran, _ = xr.shape
    bts, mix = np.asarray(block_types).reshape(c, n_gran), np.asarray(mixed).reshape(c, n_gran).astype(bool)
    overlap = np.zeros((c, 32, 18)) if overlap is None else np.array(overlap, np.float64)
    v = np.zeros((c, 1024)) if v is None else np.array(v, np.float64)
    d512 = np.asarray(d512, np.float64)
    lo_i, hi_i, bi, sbi = t["boundaries"].T
    pcm = np.empty((c, n_gran, 576))
    for g in range(n_gran):
        bt, mx = bts[:, g], mix[:, g]
        x = xr[:, g].copy()
        # 2.4.3.4.10.1: long blocks every boundary, mixed short blocks the first, short blocks none
        use = (bt != 2)[:, None] | ((bt == 2) & mx)[:, None] & (sbi == 1)[None, :]  # [C][boundary butterflies]
        lo, hi = x[:, lo_i], x[:, hi_i]
        x[:, lo_i] = np.where(use, lo * t["cs"][bi] - hi * t["ca"][bi], lo)
        x[:, hi_i] = np.where(use, hi * t["cs"][bi] + lo * t["ca"][bi], hi)
        x = x.reshape(c, 32, 18)
        eff = np.where((bt == 2)[:, None] & mx[:, None] & (np.arange(32) < 2)[None, :], 0, bt[:, None])  # [C][32]
        longw = t["win"][np.clip(np.where(eff == 3, 2, eff), 0, 2)]  # windows of block types 0, 1, 3
        raw = (x @ t["m36"].T) * longw
        short = np.zeros((c, 32, 36))
        xs = x.reshape(c, 32, 6, 3)  # X_w[m] = x18[3 m + w]
        for w in range(3):
            short[:, :, 6 * w + 6:6 * w + 18] += (xs[:, :, :, w] @ t["m12"].T) * t["win12"]
        raw = np.where((eff == 2)[:, :, None], short, raw)
        out = raw[:, :, :18] + overlap
        overlap = raw[:, :, 18:].copy()
        out[:, 1::2, 1::2] *= -1.0
        for ss in range(18):
            v[:, 64:] = v[:, :-64].copy()
            v[:, :64] = out[:, :, ss] @ t["matrix"].T
            pcm[:, g, 32 * ss:32 * ss + 32] = (v[:, t["u_idx"]] * d512).reshape(c, 16, 32).sum(axis=1)
    return pcm, overlap, v

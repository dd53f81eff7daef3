// pcm_wide.hip -- PCM sources of 3 ... 8 channels for gfx950: what pcm_tick.hip's kernels do for mono and stereo, without their
// assumption that a lane's 16 samples are whole frames, and all three branches of downmix_channels (soundkit-decoder/src/lib.rs:
// 3492-3561) instead of the mono one alone:
//
//   k_pcm_wide         one job = one AudioData (or a cut of one): interleaved bytes or planar f32 rows in, downmix, interleaved bytes
//                      or planar f32 rows out.  The tick's direct conversion (bytes -> bytes), its pack behind the resampler rounds
//                      (rows -> bytes) and sk_pcm_downmix_dev (rows -> rows) are this one body.
//   k_pcm_wide_ingest  k_pcm_ingest for C rows.
//
// A workgroup takes kWideSliceFrames whole frames.  Interleaved input is fetched as in pcm_tick.hip -- 16 samples per lane with 16-byte
// loads -- into a padded LDS tile, the lanes then walk FRAMES of that tile; interleaved output is collected as one word per sample
// in a second tile and leaves as consecutive dwords on consecutive lanes.
//
// The stereo branch of a source with more than two channels scales by 1 / max(|L|, |R|) taken over the WHOLE AudioData when that
// exceeds 1, so it takes two launches over the same jobs: PEAK = true reduces every workgroup's maximum (NaN left out, as
// f32::max leaves it out) and folds it into the job's word with one atomic maximum on the bit pattern -- non-negative floats order
// like unsigned integers, and a maximum does not depend on the order of arrival, so results repeat bit for bit -- and PEAK = false
// recomputes L / R and applies the scale.
#include "pcm_group.h"

namespace sk {

namespace {

constexpr uint32_t kWideMaxCh = 8;
constexpr uint32_t kWideTileIn = kWideSliceFrames * kWideMaxCh;         // samples of the largest slice
constexpr uint32_t kWideTileOut = kWideTileIn;  // one word per output sample; all channels when a resampled stream keeps them

// downmix_channels for one frame: x = its C channels, y = its min(T, C) outputs BEFORE the stereo branch's normalisation.
// f32, the reference's operations in the reference's order (the build has -ffp-contract=off).
__device__ __forceinline__ void downmix_frame(const float (&x)[kWideMaxCh], uint32_t C, uint32_t T, float (&y)[kWideMaxCh]) {
    if (T == 1) {  // lib.rs:3500-3508: mono[i] += sample * scale, channels in order
        const float scale = 1.0f / (float)C;
        float acc = 0.0f;
#pragma unroll
        for (uint32_t c = 0; c < kWideMaxCh; ++c)
            if (c < C) acc += x[c] * scale;
        y[0] = acc;
    } else if (T == 2 && C > 2) {  // lib.rs:3512-3538: L + 0.707 C + 0.707 Ls, R + 0.707 C + 0.707 Rs; channels 3, 6, 7 unused
        const float k = 0.707f;
        float l = x[0], r = x[1];
        l += k * x[2];
        r += k * x[2];
        if (C > 4) l += k * x[4];
        if (C > 5) r += k * x[5];
        y[0] = l;
        y[1] = r;
    } else {  // lib.rs:3560: the first T channels
#pragma unroll
        for (uint32_t c = 0; c < kWideMaxCh; ++c) y[c] = x[c];
    }
}

// fold(0.0, f32::max) over |v| on the bit pattern: a NaN never raises it, +inf does
__device__ __forceinline__ uint32_t peak_fold(uint32_t m, float v) {
    const float a = fabsf(v);
    const uint32_t b = __float_as_uint(a);
    return (a == a && b > m) ? b : m;
}

// BYTES_IN: the jobs' sources are interleaved bytes (all jobs of a launch agree); a launch over planar rows reserves no input tile
template <bool PEAK, bool BYTES_IN>
__device__ __forceinline__ void wide_body(const WideJob &job, uint32_t *peaks) {
    __shared__ float tin[BYTES_IN ? kWideTileIn + kWideTileIn / 32 : 1];
    __shared__ uint32_t tout[PEAK ? 1 : kWideTileOut + kWideTileOut / 32];
    __shared__ uint32_t wave_max[4];
    const uint32_t C = job.ch_in, T = job.ch_out;
    const bool normalise = T == 2 && C > 2 && job.peak != kWideNoPeak;
    if (PEAK && !normalise) return;
    const uint32_t f0 = blockIdx.x * kWideSliceFrames;
    if (f0 >= job.frames) return;  // the whole workgroup leaves
    const uint32_t nf = min(kWideSliceFrames, job.frames - f0);
    const bool bytes_in = BYTES_IN, bytes_out = job.fmt_out != kWidePlanar;

    if (bytes_in) {  // the slice's samples -> f32 in LDS, as k_pcm_ingest stages them
        const int fmt = job.fmt_in, ib = fmt_bytes(fmt);
        const uint8_t *src = static_cast<const uint8_t *>(job.src);
        const size_t base = (size_t)f0 * C;
        const uint32_t n = nf * C, s0 = threadIdx.x * 16;
        if (s0 + 16 <= n) {
            uint32_t raw[16];
            load_group_any(ib, src, base + s0, raw);
#pragma unroll
            for (int s = 0; s < 16; ++s) tin[tile_at(s0 + s)] = sample_to_f32(0, fmt, raw[s]);
        } else {
            for (uint32_t s = s0; s < n; ++s) tin[tile_at(s)] = sample_to_f32(0, fmt, load_raw_scalar(src + (base + s) * ib, ib));
        }
        __syncthreads();
    }

    float scale = 1.0f;
    bool scaled = false;
    if (!PEAK && normalise) {  // lib.rs:3541-3554
        const float m = __uint_as_float(peaks[job.peak]);
        if (m > 1.0f) scaled = true, scale = 1.0f / m;
    }
    uint32_t m_bits = 0;
    const float *rows = static_cast<const float *>(job.src);
    for (uint32_t f = threadIdx.x; f < nf; f += 256) {
        float x[kWideMaxCh], y[kWideMaxCh];
#pragma unroll
        for (uint32_t c = 0; c < kWideMaxCh; ++c) {
            x[c] = 0.0f;
            if (c < C) x[c] = bytes_in ? tin[tile_at(f * C + c)] : rows[(size_t)c * job.src_stride + f0 + f];
        }
        downmix_frame(x, C, T, y);
        if (PEAK) {
            m_bits = peak_fold(peak_fold(m_bits, y[0]), y[1]);
            continue;
        }
        if (scaled) y[0] *= scale, y[1] *= scale;
        if (bytes_out) {
#pragma unroll
            for (uint32_t c = 0; c < kWideMaxCh; ++c)
                if (c < T) tout[tile_at(f * T + c)] = f32_to_sample(job.fmt_out, y[c]);
        } else {
            float *out = static_cast<float *>(job.dst);
#pragma unroll
            for (uint32_t c = 0; c < kWideMaxCh; ++c)
                if (c < T) out[(size_t)c * job.dst_stride + f0 + f] = y[c];
        }
    }

    if (PEAK) {  // wave, workgroup, then one atomic per workgroup
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m_bits = max(m_bits, (uint32_t)__shfl_xor((int)m_bits, o));
        if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m_bits;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t m = max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3]));
            if (m) atomicMax(&peaks[job.peak], m);
        }
        return;
    }
    if (!bytes_out) return;
    __syncthreads();
    // the slice's output bytes as dwords, consecutive lanes on consecutive dwords; what is left of the last dword byte by byte
    const uint32_t ob = (uint32_t)fmt_bytes(job.fmt_out), nb = nf * T * ob, nd = nb >> 2;
    uint8_t *out = static_cast<uint8_t *>(job.dst) + (size_t)f0 * T * ob;  // 16-byte aligned: kWideSliceFrames is a multiple of 16
    for (uint32_t d = threadIdx.x; d < nd; d += 256) {
        uint32_t w;
        if (ob == 4) {
            w = tout[tile_at(d)];
        } else if (ob == 2) {
            w = tout[tile_at(2 * d)] | (tout[tile_at(2 * d + 1)] << 16);
        } else {  // four 3-byte samples = three dwords
            const uint32_t g = d / 3, r = d - 3 * g;
            w = (tout[tile_at(4 * g + r)] >> (8 * r)) | (tout[tile_at(4 * g + r + 1)] << (24 - 8 * r));
        }
        reinterpret_cast<uint32_t *>(out)[d] = w;
    }
    if (threadIdx.x == 0) {
        for (uint32_t b = nd * 4; b < nb; ++b) {
            const uint32_t s = b / ob;
            out[b] = (uint8_t)(tout[tile_at(s)] >> (8 * (b - s * ob)));
        }
    }
}

template <bool PEAK, bool BYTES_IN>
__global__ __launch_bounds__(256) void k_pcm_wide(const WideJob *jobs, uint32_t n_jobs, uint32_t *peaks) {
    const uint32_t j = blockIdx.y;
    if (j >= n_jobs) return;
    const WideJob job = jobs[j];
    wide_body<PEAK, BYTES_IN>(job, peaks);
}

template <bool PEAK>
__global__ __launch_bounds__(256) void k_pcm_wide_one(const WideJob job, uint32_t *peaks) {  // planar rows in
    wide_body<PEAK, false>(job, peaks);
}

// one workgroup = kWideSliceFrames frames of one job: converted 16 samples per lane into LDS, then written row by row with consecutive
// lanes on consecutive frames (coalesced dwords: a row starts at the stream's fill, so nothing wider is available)
__global__ __launch_bounds__(256) void k_pcm_wide_ingest(const PcmWideIngestJob *jobs, uint32_t n_jobs) {
    __shared__ float tile[kWideTileIn + kWideTileIn / 32];
    const uint32_t j = blockIdx.y;
    if (j >= n_jobs) return;
    const PcmWideIngestJob job = jobs[j];
    const uint32_t f0 = blockIdx.x * kWideSliceFrames;
    if (f0 >= job.frames) return;  // the whole workgroup leaves
    const uint32_t C = job.ch, nf = min(kWideSliceFrames, job.frames - f0), n = nf * C;
    const int fmt = job.fmt, ib = fmt_bytes(fmt);
    const size_t base = (size_t)f0 * C;
    const uint32_t s0 = threadIdx.x * 16;
    if (s0 + 16 <= n) {
        uint32_t raw[16];
        load_group_any(ib, job.src, base + s0, raw);
#pragma unroll
        for (int s = 0; s < 16; ++s) tile[tile_at(s0 + s)] = sample_to_f32(0, fmt, raw[s]);
    } else {
        for (uint32_t s = s0; s < n; ++s) tile[tile_at(s)] = sample_to_f32(0, fmt, load_raw_scalar(job.src + (base + s) * ib, ib));
    }
    __syncthreads();
    for (uint32_t c = 0; c < C; ++c) {
        float *row = job.dst + (size_t)c * job.row_stride + f0;
        for (uint32_t f = threadIdx.x; f < nf; f += 256) row[f] = tile[tile_at(f * C + c)];
    }
}

uint32_t wide_slices(uint32_t frames) { return (frames + kWideSliceFrames - 1) / kWideSliceFrames; }

}  // namespace

hipError_t launch_pcm_wide(const WideJob *jobs, uint32_t n_jobs, uint32_t n_peak_jobs, uint32_t max_frames, bool bytes_in, uint32_t *peaks, hipStream_t s) {
    if (n_jobs == 0 || max_frames == 0) return hipSuccess;
    const dim3 block(256);
    for (int pass = n_peak_jobs ? 0 : 1; pass < 2; ++pass) {
        for (uint32_t j0 = 0; j0 < n_jobs; j0 += 65535) {
            const uint32_t n = n_jobs - j0 < 65535 ? n_jobs - j0 : 65535;
            const dim3 grid(wide_slices(max_frames), n);
            if (pass == 0 && bytes_in) hipLaunchKernelGGL((k_pcm_wide<true, true>), grid, block, 0, s, jobs + j0, n, peaks);
            else if (pass == 0) hipLaunchKernelGGL((k_pcm_wide<true, false>), grid, block, 0, s, jobs + j0, n, peaks);
            else if (bytes_in) hipLaunchKernelGGL((k_pcm_wide<false, true>), grid, block, 0, s, jobs + j0, n, peaks);
            else hipLaunchKernelGGL((k_pcm_wide<false, false>), grid, block, 0, s, jobs + j0, n, peaks);
        }
    }
    return hipGetLastError();
}

hipError_t launch_pcm_wide_one(const WideJob &job, uint32_t *peaks, hipStream_t s) {
    if (job.frames == 0) return hipSuccess;
    if (job.peak != kWideNoPeak) hipLaunchKernelGGL(k_pcm_wide_one<true>, dim3(wide_slices(job.frames)), dim3(256), 0, s, job, peaks);
    hipLaunchKernelGGL(k_pcm_wide_one<false>, dim3(wide_slices(job.frames)), dim3(256), 0, s, job, peaks);
    return hipGetLastError();
}

hipError_t launch_pcm_wide_ingest(const PcmWideIngestJob *jobs, uint32_t n_jobs, uint32_t max_frames, hipStream_t s) {
    if (n_jobs == 0 || max_frames == 0) return hipSuccess;
    for (uint32_t j0 = 0; j0 < n_jobs; j0 += 65535) {
        const uint32_t n = n_jobs - j0 < 65535 ? n_jobs - j0 : 65535;
        hipLaunchKernelGGL(k_pcm_wide_ingest, dim3(wide_slices(max_frames), n), dim3(256), 0, s, jobs + j0, n);
    }
    return hipGetLastError();
}

}  // namespace sk

// pcm_tick.hip -- the PCM streams' tick for gfx950 (sk_tick_run_pcm, engine.cpp): what the reference's worker does to a WAV or
// raw PCM stream's AudioData in apply_output_options (soundkit-decoder/src/lib.rs:3324-3456), for every unit of every stream
// of a tick in ONE launch per kind:
//
//   k_pcm_direct  no rate change: exact_signed_pcm_to_i16 (lib.rs:3458-3489), or audio_data_to_f32_channels (:3563-3617) ->
//                 mono downmix (:3492-3510) -> f32_channels_to_bytes (:3619-3683) in registers: the f32 never goes to HBM.
//   k_pcm_ingest  rate change: audio_data_to_f32_channels straight into the stream's resampler staging rows (what k_row_copies
//                 does for decoded units); the resampler rounds, the downmix and the byte conversion are the tick's own
//                 (rs_process_ready, k_pack_jobs).
//
// Both: a job table in the tick arena, grid = (slices of kPcmSliceSamples samples, jobs).  The host packs every unit at a 16-byte
// aligned offset, so a lane fetches its 16 samples with 2 / 3 / 4 16-byte loads (s16 / s24 / s32 and f32; big-endian forms are
// the same loads plus a byte swap); only a unit's last, incomplete group of 16 goes sample by sample.  The sample arithmetic is
// pcm_sample.h's, shared with pcm.hip.
#include "pcm_group.h"

namespace sk {

namespace {

// N samples (16, or 8 after a downmix) of OB bytes each, masked to their width, as N * OB / 8 8-byte stores (dst is 8-byte aligned:
// a job's output starts 16-byte aligned and a group is 16 ... 64 bytes)
template <int OB, int N>
__device__ __forceinline__ void store_group(uint8_t *dst, const uint32_t (&v)[16]) {
    constexpr int D = N * OB / 4;
    uint32_t o[D];
    if (OB == 4) {
#pragma unroll
        for (int i = 0; i < D; ++i) o[i] = v[i];
    } else if (OB == 2) {
#pragma unroll
        for (int i = 0; i < D; ++i) o[i] = v[2 * i] | (v[2 * i + 1] << 16);
    } else {
#pragma unroll
        for (int g = 0; g < N / 4; ++g) {  // four 3-byte samples = three dwords
            o[3 * g] = v[4 * g] | (v[4 * g + 1] << 24);
            o[3 * g + 1] = (v[4 * g + 1] >> 8) | (v[4 * g + 2] << 16);
            o[3 * g + 2] = (v[4 * g + 2] >> 16) | (v[4 * g + 3] << 8);
        }
    }
    uint2 *out = reinterpret_cast<uint2 *>(dst);
#pragma unroll
    for (int i = 0; i < D / 2; ++i) out[i] = make_uint2(o[2 * i], o[2 * i + 1]);
}

template <int N>
__device__ __forceinline__ void store_group_any(int ob, uint8_t *dst, const uint32_t (&v)[16]) {
    if (ob == 2) store_group<2, N>(dst, v);
    else if (ob == 3) store_group<3, N>(dst, v);
    else store_group<4, N>(dst, v);
}

// one workgroup = kPcmSliceSamples samples of one job, a lane = 16 of them; the lane's 16 ... 64 bytes of output leave as 8-byte
// stores (lane-strided: the measured weak spot of this kernel)
__global__ __launch_bounds__(256) void k_pcm_direct(const PcmDirectJob *jobs, uint32_t n_jobs) {
    const uint32_t j = blockIdx.y;
    if (j >= n_jobs) return;
    const PcmDirectJob job = jobs[j];
    const uint32_t total = job.frames * job.ch_in;  // samples
    const uint32_t s0 = blockIdx.x * kPcmSliceSamples + threadIdx.x * 16;
    if (s0 >= total) return;
    const int fi = job.fmt_in, fo = job.fmt_out;
    const int ib = fmt_bytes(fi), ob = fmt_bytes(fo);
    const bool down = job.ch_out < job.ch_in;  // two channels to one
    if (s0 + 16 <= total) {
        uint32_t raw[16], v[16];
        load_group_any(ib, job.src, s0, raw);
        if (job.exact) {
#pragma unroll
            for (int s = 0; s < 16; ++s) v[s] = exact_sample_to_i16(fi, raw[s]);
        } else if (down) {
#pragma unroll
            for (int f = 0; f < 8; ++f) {
                v[f] = f32_to_sample(fo, downmix2(sample_to_f32(0, fi, raw[2 * f]), sample_to_f32(0, fi, raw[2 * f + 1])));
                v[8 + f] = 0;
            }
        } else {
#pragma unroll
            for (int s = 0; s < 16; ++s) v[s] = f32_to_sample(fo, sample_to_f32(0, fi, raw[s]));
        }
        if (down) store_group_any<8>(ob, job.dst + (size_t)(s0 / 2) * ob, v);
        else store_group_any<16>(ob, job.dst + (size_t)s0 * ob, v);
        return;
    }
    // the unit's last, incomplete group: sample by sample (frame by frame when downmixing)
    if (down) {
        for (uint32_t s = s0; s + 1 < total; s += 2) {
            const float l = sample_to_f32(0, fi, load_raw_scalar(job.src + (size_t)s * ib, ib));
            const float r = sample_to_f32(0, fi, load_raw_scalar(job.src + (size_t)(s + 1) * ib, ib));
            store_raw_scalar(job.dst + (size_t)(s / 2) * ob, f32_to_sample(fo, downmix2(l, r)), ob);
        }
    } else {
        for (uint32_t s = s0; s < total; ++s) {
            const uint32_t raw = load_raw_scalar(job.src + (size_t)s * ib, ib);
            store_raw_scalar(job.dst + (size_t)s * ob, job.exact ? exact_sample_to_i16(fi, raw) : f32_to_sample(fo, sample_to_f32(0, fi, raw)), ob);
        }
    }
}

// one workgroup = kPcmSliceSamples samples of one job: converted 16 per lane into LDS, then written to the channel rows with
// consecutive lanes on consecutive frames (coalesced dwords: a row starts at the stream's fill, so nothing wider is available)
__global__ __launch_bounds__(256) void k_pcm_ingest(const PcmIngestJob *jobs, uint32_t n_jobs) {
    __shared__ float tile[kPcmSliceSamples + kPcmSliceSamples / 32];
    const uint32_t j = blockIdx.y;
    if (j >= n_jobs) return;
    const PcmIngestJob job = jobs[j];
    const uint32_t total = job.frames * job.ch;  // samples
    const uint32_t base = blockIdx.x * kPcmSliceSamples;
    if (base >= total) return;  // the whole workgroup leaves
    const uint32_t n = min(kPcmSliceSamples, total - base);
    const int fmt = job.fmt, ib = fmt_bytes(fmt);
    const uint32_t s0 = threadIdx.x * 16;
    if (s0 + 16 <= n) {
        uint32_t raw[16];
        load_group_any(ib, job.src, (size_t)base + s0, raw);
#pragma unroll
        for (int s = 0; s < 16; ++s) tile[tile_at(s0 + s)] = sample_to_f32(0, fmt, raw[s]);
    } else {
        for (uint32_t s = s0; s < n; ++s) tile[tile_at(s)] = sample_to_f32(0, fmt, load_raw_scalar(job.src + (size_t)(base + s) * ib, ib));
    }
    __syncthreads();
    if (job.ch == 2) {
        for (uint32_t i = threadIdx.x; (i & ~63u) < n; i += 256) {  // lanes 0 .. 31 of a wave: 32 consecutive frames of the first row, 32 .. 63: of the second
            const uint32_t wave0 = i & ~63u, lane = i & 63u;
            const uint32_t c = lane >> 5, k = wave0 + 2 * (lane & 31u) + c;  // sample k of the slice: frame (base + k) / 2, channel c
            if (k < n) (c ? job.dst1 : job.dst0)[(base + k) >> 1] = tile[tile_at(k)];
        }
    } else {
        for (uint32_t i = threadIdx.x; i < n; i += 256) job.dst0[base + i] = tile[tile_at(i)];
    }
}

template <typename Job>
hipError_t launch_jobs(void (*kernel)(const Job *, uint32_t), const Job *jobs, uint32_t n_jobs, uint32_t max_samples, hipStream_t s) {
    if (n_jobs == 0 || max_samples == 0) return hipSuccess;
    const uint32_t slices = (max_samples + kPcmSliceSamples - 1) / kPcmSliceSamples;
    for (uint32_t j0 = 0; j0 < n_jobs; j0 += 65535) {
        const uint32_t n = n_jobs - j0 < 65535 ? n_jobs - j0 : 65535;
        hipLaunchKernelGGL(kernel, dim3(slices, n), dim3(256), 0, s, jobs + j0, n);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_pcm_direct(const PcmDirectJob *jobs, uint32_t n_jobs, uint32_t max_samples, hipStream_t s) {
    return launch_jobs(k_pcm_direct, jobs, n_jobs, max_samples, s);
}

hipError_t launch_pcm_ingest(const PcmIngestJob *jobs, uint32_t n_jobs, uint32_t max_samples, hipStream_t s) {
    return launch_jobs(k_pcm_ingest, jobs, n_jobs, max_samples, s);
}

}  // namespace sk

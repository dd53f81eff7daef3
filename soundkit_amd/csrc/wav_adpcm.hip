// wav_adpcm.hip -- WAV's two ADPCM format tags decoded for gfx950 (sk_wav_adpcm_decode; engine.cpp).  Whole blocks of nBlockAlign
// bytes in, interleaved little-endian s16 out, frames_per_block x channels samples a block.  Integers only.
//
//   k_wav_ima   tag 0x11, IMA / DVI ADPCM.  A block: per channel a 4-byte header {predictor s16le, step index u8, reserved}, the
//               predictor being the channel's first sample; then groups of 4 x channels bytes, 4 bytes (8 samples, low nibble first)
//               for channel 0, then 4 for channel 1.  The per-nibble arithmetic is IMA4's (ima_adpcm.h).  A header index above 88
//               rules the block out.
//   k_wav_ms    tag 2, Microsoft ADPCM.  A block: bPredictor u8 for every channel, then iDelta s16le for every channel, then iSamp1,
//               then iSamp2; output iSamp2, iSamp1, then one sample a nibble, high nibble first (stereo: high = left, low = right).
//               pred = (samp1 * c1 + samp2 * c2) / 256 with C's truncating division on the 32-bit (wrapping) sum, new =
//               clamp16(pred + sn * delta), delta = clamp(AdaptationTable[n] * delta / 256, 16, INT_MAX / 768).  The coefficient
//               pairs are the file's.  A bPredictor at or past n_coef rules the block out.
//
// Mapping: neither form carries anything from block to block, so lane (block x channels + channel) decodes one channel of one block
// from its header, serially, and consecutive blocks sit on consecutive lanes.  The lanes read their own bytes directly -- dwords for
// IMA, whose groups are 4-byte aligned, bytes for MS, whose blocks may have any size: a wave's loads are block_align apart, but they
// walk one contiguous span of 64 x block_align bytes (up to 4 MiB at the largest block), every cache line of it is read again by
// the same lane for its next 32 groups, and no LDS staging of 64 blocks of up to 65 535 bytes would fit.  A block that is ruled out
// is written as zeros by its own lanes (each lane reads every channel's header, so both agree), status by the channel-0 lane.
// A job is a run of whole blocks of one stream; grid = (slices of 256 lanes, jobs), as k_aiff_elem's.  Of a job only the first
// keep_frames frames are stored: a stream whose `fact` chunk cuts its last block decodes into a buffer that ends there.
#include "ima_adpcm.h"
#include "sk_device.h"

namespace sk {

namespace {

__device__ const int16_t kMsAdapt[16] = {230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230};
constexpr int kMsDeltaMax = 0x7fffffff / 768;  // keeps AdaptationTable[n] * delta inside 32 bits whatever the nibbles are

__device__ __forceinline__ int le16s(const uint8_t *p) { return (int)(int16_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8)); }

__device__ __forceinline__ void zero_channel(int16_t *out, uint32_t frames, uint32_t ch) {
    for (uint32_t f = 0; f < frames; ++f) out[(size_t)f * ch] = 0;
}
// how many of block `blk`'s frames the job keeps: all but in the block the `fact` cut falls into, none behind it
__device__ __forceinline__ uint32_t frames_kept(const WavAdpcmJob &job, uint32_t blk) {
    const uint64_t first = (uint64_t)blk * job.frames_per_block;
    return first >= job.keep_frames ? 0 : (uint32_t)min((uint64_t)job.frames_per_block, job.keep_frames - first);
}

__global__ __launch_bounds__(256) void k_wav_ima(const WavAdpcmJob *jobs, uint32_t n_jobs) {
    __shared__ int s_step[89];
    for (uint32_t i = threadIdx.x; i < 89; i += 256) s_step[i] = kImaStep[i];
    __syncthreads();
    if (blockIdx.y >= n_jobs) return;
    const WavAdpcmJob &job = jobs[blockIdx.y];
    const uint32_t ch = job.channels;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)job.n_blocks * ch) return;
    const uint32_t blk = (uint32_t)(t / ch), c = (uint32_t)(t % ch);
    const uint8_t *src = job.src + (size_t)blk * job.block_align;
    int16_t *out = reinterpret_cast<int16_t *>(job.dst) + (size_t)blk * job.frames_per_block * ch + c;
    bool bad = false;
    for (uint32_t k = 0; k < ch; ++k) bad |= src[4 * k + 2] > 88;
    if (c == 0) job.status[blk] = bad ? kWavAdpcmBadBlock : 0;
    const uint32_t keep = frames_kept(job, blk);
    if (keep == 0) return;
    if (bad) {
        zero_channel(out, keep, ch);
        return;
    }
    int p = le16s(src + 4 * c), idx = src[4 * c + 2];
    out[0] = (int16_t)p;
    const uint32_t groups = (keep - 1 + 7) / 8;  // the groups that hold a kept frame; of the last one maybe not all eight
    const uint32_t *words = reinterpret_cast<const uint32_t *>(src + 4 * ch) + c;
    out += ch;
    for (uint32_t g = 0; g < groups; ++g) {
        const uint32_t w = words[(size_t)g * ch];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t nib = (w >> (4 * k)) & 15;
            p = clamp_s16(p + ima_delta(s_step[idx], nib));
            idx = ima_next_index(idx, nib);
            if (1 + 8 * g + k < keep) out[(size_t)k * ch] = (int16_t)p;
        }
        out += 8 * ch;
    }
}

__global__ __launch_bounds__(256) void k_wav_ms(const WavAdpcmJob *jobs, uint32_t n_jobs) {
    if (blockIdx.y >= n_jobs) return;
    const WavAdpcmJob &job = jobs[blockIdx.y];
    const uint32_t ch = job.channels;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)job.n_blocks * ch) return;
    const uint32_t blk = (uint32_t)(t / ch), c = (uint32_t)(t % ch);
    const uint8_t *src = job.src + (size_t)blk * job.block_align;
    int16_t *out = reinterpret_cast<int16_t *>(job.dst) + (size_t)blk * job.frames_per_block * ch + c;
    bool bad = false;
    for (uint32_t k = 0; k < ch; ++k) bad |= src[k] >= job.n_coef;
    if (c == 0) job.status[blk] = bad ? kWavAdpcmBadBlock : 0;
    const uint32_t keep = frames_kept(job, blk);
    if (keep == 0) return;
    if (bad) {
        zero_channel(out, keep, ch);
        return;
    }
    const int c1 = job.coef[src[c]][0], c2 = job.coef[src[c]][1];
    int delta = le16s(src + ch + 2 * c), s1 = le16s(src + 3 * ch + 2 * c), s2 = le16s(src + 5 * ch + 2 * c);
    out[0] = (int16_t)s2;
    if (keep < 2) return;
    out[ch] = (int16_t)s1;
    out += 2 * (size_t)ch;
    const uint32_t rest = keep - 2;  // frames the nibbles give
    auto step = [&](uint32_t n) {
        const int sum = (int)((uint32_t)(s1 * c1) + (uint32_t)(s2 * c2));  // each product fits 31 bits; the sum wraps
        const int v = clamp_s16(sum / 256 + ((int)(n ^ 8) - 8) * delta);
        s2 = s1, s1 = v;
        delta = kMsAdapt[n] * delta / 256;
        delta = delta < 16 ? 16 : (delta > kMsDeltaMax ? kMsDeltaMax : delta);
        return (int16_t)v;
    };
    const uint8_t *body = src + 7 * ch;
    if (ch == 1) {
        for (uint32_t i = 0; 2 * i < rest; ++i) {
            const uint32_t b = body[i];
            out[2 * (size_t)i] = step(b >> 4);
            if (2 * i + 1 < rest) out[2 * (size_t)i + 1] = step(b & 15);
        }
    } else {
        for (uint32_t i = 0; i < rest; ++i) {
            const uint32_t b = body[i];
            out[2 * (size_t)i] = step(c == 0 ? b >> 4 : b & 15);
        }
    }
}

}  // namespace

hipError_t launch_wav_adpcm(const WavAdpcmJob *jobs, uint32_t n_jobs, bool ima, uint32_t max_lanes, hipStream_t s) {
    if (n_jobs == 0 || max_lanes == 0) return hipSuccess;
    const uint32_t slices = (max_lanes + 255) / 256;
    for (uint32_t j0 = 0; j0 < n_jobs; j0 += 65535) {
        const uint32_t n = n_jobs - j0 < 65535 ? n_jobs - j0 : 65535;
        if (ima) hipLaunchKernelGGL(k_wav_ima, dim3(slices, n), dim3(256), 0, s, jobs + j0, n);
        else hipLaunchKernelGGL(k_wav_ms, dim3(slices, n), dim3(256), 0, s, jobs + j0, n);
    }
    return hipGetLastError();
}

}  // namespace sk

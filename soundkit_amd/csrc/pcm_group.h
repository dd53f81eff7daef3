// pcm_group.h -- how the PCM ticks' kernels (pcm_tick.hip, pcm_wide.hip) fetch a unit's samples: 16 at a time with 16-byte loads,
// and the padded LDS index of the slice they stage.  Device code only.
#pragma once
#include "pcm_sample.h"

namespace sk {

namespace {

// 16 samples of IB bytes each = IB 16-byte loads; raw[s] = the sample's bytes, little-endian packed in the low bits
template <int IB>
__device__ __forceinline__ void load_group(const uint8_t *src, uint32_t (&raw)[16]) {
    uint32_t w[4 * IB];
    const uint4 *p = reinterpret_cast<const uint4 *>(src);
#pragma unroll
    for (int k = 0; k < IB; ++k) {
        const uint4 v = p[k];
        w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        if (IB == 4) {
            raw[s] = w[s];
        } else if (IB == 2) {
            raw[s] = (w[s >> 1] >> (16 * (s & 1))) & 0xffff;
        } else {  // bytes 3s .. 3s + 2 of 48
            const int bit = 24 * s, d = bit >> 5, sh = bit & 31;
            const uint64_t pair = (uint64_t)w[d] | ((uint64_t)(d + 1 < 4 * IB ? w[d + 1] : 0u) << 32);
            raw[s] = (uint32_t)(pair >> sh) & 0xffffff;
        }
    }
}

template <int IB>
__device__ __forceinline__ void load_group_fmt(const uint8_t *src, size_t first_sample, uint32_t (&raw)[16]) {
    load_group<IB>(src + first_sample * IB, raw);
}

__device__ __forceinline__ void load_group_any(int ib, const uint8_t *src, size_t first_sample, uint32_t (&raw)[16]) {
    if (ib == 2) load_group_fmt<2>(src, first_sample, raw);
    else if (ib == 3) load_group_fmt<3>(src, first_sample, raw);
    else load_group_fmt<4>(src, first_sample, raw);
}

__device__ __forceinline__ int fmt_bytes(int fmt) { return fmt <= SK_FMT_S16BE ? 2 : (fmt <= SK_FMT_S24BE ? 3 : 4); }

// LDS index of sample i of the slice: one pad float per 32, so that the lanes' 16-sample runs do not all start in one bank
__device__ __forceinline__ uint32_t tile_at(uint32_t i) { return i + (i >> 5); }

}  // namespace

}  // namespace sk

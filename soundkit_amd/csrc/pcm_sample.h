// pcm_sample.h -- the per-sample arithmetic of the PCM conversions, shared by pcm.hip (the one-call ops) and pcm_tick.hip
// (the batched tick): one definition, so the pinned ops and the tick cannot drift apart.  Device code only.
#pragma once
#include "sk_device.h"

#include "../../include/soundkit_amd.h"

namespace sk {

// ---- Rust cast semantics ---------------------------------------------------------------
__device__ __forceinline__ int f32_as_i32(float x) {
    if (x != x) return 0;
    if (x <= -2147483648.0f) return INT32_MIN;
    if (x >= 2147483648.0f) return INT32_MAX;
    return (int)x;
}
__device__ __forceinline__ int f32_as_i16(float x) {
    if (x != x) return 0;
    if (x <= -32768.0f) return -32768;
    if (x >= 32767.0f) return 32767;
    return (int)x;
}
__device__ __forceinline__ float clamp1(float x) {  // f32::clamp(-1, 1): NaN stays NaN
    if (x < -1.0f) x = -1.0f;
    if (x > 1.0f) x = 1.0f;
    return x;
}
__device__ __forceinline__ uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }
__device__ __forceinline__ uint32_t bswap16(uint32_t v) { return ((v & 0xff) << 8) | ((v >> 8) & 0xff); }
__device__ __forceinline__ int sext24(uint32_t v) { return (int)(((v & 0xffffffu) ^ 0x800000u) - 0x800000u); }
__device__ __forceinline__ int sext16(uint32_t v) { return (int)(short)(unsigned short)v; }
__device__ __forceinline__ uint32_t be24(uint32_t v) { return ((v & 0xff) << 16) | (v & 0xff00) | ((v >> 16) & 0xff); }

// soundkit-decoder lib.rs:1815-1827; the f64-free exact form of sk_device.h (exhaustively equal, tools/check_f32_rounding.c)
__device__ __forceinline__ int float_sample_to_i16(float s) { return dev_float_sample_to_i16_f32(s); }
__device__ __forceinline__ int f32_to_i32_pcm(float x) {  // audio_bytes.rs:194-199 (both scales are 2^31 in f32)
    return f32_as_i32(clamp1(x) * 2147483648.0f);
}
__device__ __forceinline__ int f32_to_s24_pcm(float x) {  // audio_bytes.rs:210-216
    const float c = clamp1(x);
    return c >= 0.0f ? f32_as_i32(c * 8388607.0f) : f32_as_i32(c * 8388608.0f);
}

// Scalar element access.  2- and 4-byte elements are naturally aligned (API contract), so they move
// as one typed access; only 3-byte samples go byte by byte.  (Splitting a sign-extended value into
// byte stores is also what hipcc 7.2 folds into a zero-extending v_perm_b32 -- avoid that shape.)
__device__ __forceinline__ uint32_t load_raw_scalar(const uint8_t *p, int ib) {
    if (ib == 4) return *reinterpret_cast<const uint32_t *>(p);
    if (ib == 2) return *reinterpret_cast<const uint16_t *>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}
__device__ __forceinline__ void store_raw_scalar(uint8_t *p, uint32_t v, int ob) {
    if (ob == 4) {
        *reinterpret_cast<uint32_t *>(p) = v;
    } else if (ob == 2) {
        *reinterpret_cast<uint16_t *>(p) = (uint16_t)v;
    } else {
        p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16);
    }
}

// raw = the sample's bytes as they lie in memory, little-endian packed in the low bits
__device__ __forceinline__ float sample_to_f32(int variant, int fmt, uint32_t raw) {
    float s;
    switch (fmt) {
    case SK_FMT_F32LE: s = __uint_as_float(raw); break;
    case SK_FMT_F32BE: s = __uint_as_float(bswap32(raw)); break;
    case SK_FMT_S16LE: s = (float)sext16(raw) / 32768.0f; break;
    case SK_FMT_S16BE: s = (float)sext16(bswap16(raw)) / 32768.0f; break;
    case SK_FMT_S24LE: s = (float)sext24(raw) / (variant == 0 ? 8388608.0f : 2147483648.0f); break;
    case SK_FMT_S24BE: s = (float)sext24(be24(raw)) / 8388608.0f; break;
    case SK_FMT_S32LE: s = (float)(int)raw / 2147483648.0f; break;
    default: s = (float)(int)bswap32(raw) / 2147483648.0f; break;
    }
    if (variant == 0 && !isfinite(s)) s = 0.0f;  // soundkit-decoder lib.rs:3614
    return s;
}

__device__ __forceinline__ uint32_t f32_to_sample(int fmt, float x) {
    switch (fmt) {
    case SK_FMT_F32LE: return __float_as_uint(x);
    case SK_FMT_S16LE: return (uint32_t)float_sample_to_i16(x) & 0xffff;
    case SK_FMT_S24LE: {  // soundkit-decoder lib.rs:3649-3661
        const float c = clamp1(x);
        return (uint32_t)(c >= 0.0f ? f32_as_i32(c * 8388607.0f) : f32_as_i32(c * 8388608.0f)) & 0xffffff;
    }
    default: return (uint32_t)f32_to_i32_pcm(x);  // S32LE, lib.rs:3664-3677
    }
}

// exact_signed_pcm_to_i16 (soundkit-decoder lib.rs:3458-3489): the top 16 bits of a 24- / 32-bit signed sample
__device__ __forceinline__ uint32_t exact_sample_to_i16(int fmt, uint32_t raw) {
    int s;
    switch (fmt) {
    case SK_FMT_S24LE: s = sext24(raw) >> 8; break;
    case SK_FMT_S24BE: s = sext24(be24(raw)) >> 8; break;
    case SK_FMT_S32LE: s = (int)raw >> 16; break;
    default: s = (int)bswap32(raw) >> 16; break;
    }
    return (uint32_t)s & 0xffff;
}

// downmix_channels(.., 1) for two channels (lib.rs:3492-3510): mono += sample * (1 / channels), channels in order
__device__ __forceinline__ float downmix2(float l, float r) {
    const float scale = 1.0f / 2.0f;
    float acc = 0.0f;
    acc += l * scale;
    acc += r * scale;
    return acc;
}

}  // namespace sk

// aiff_decode.hip -- the AIFF / AIFF-C streams' decode stage for gfx950 (sk_aiff_decode, sk_tick_run_aiff; engine.cpp): what the
// reference's AiffDecoder does to the sound bytes in decode_stream_bytes (soundkit-aiff/src/lib.rs:477-560), for every unit of
// every stream of a tick.  Source-encoded sample groups in, little-endian PCM of the output contract (lib.rs:41-54) out:
//
//   k_aiff_elem   every encoding but IMA4 (DVD LPCM's 24-bit groups are permuted byte for byte: SK_AIFF_DVD_S24): u8 / s8 widened to s16, 2- / 3- / 4-byte big-endian samples reversed (f32be as an integer
//                 swap: NaN payloads and subnormals survive), the little-endian forms copied, f64be and f64le rounded to f32 in integer
//                 arithmetic (nearest even, subnormal results kept, overflow to infinity), mu-law and A-law expanded to s16.
//                 pcm_tick.hip's conventions: a job table, grid = (slices of kPcmSliceSamples samples, jobs), units at 16-byte
//                 aligned offsets so a lane moves its 16 samples with 16-byte loads and stores; a unit's last incomplete 16 go
//                 sample by sample.
//   k_aiff_ima4   IMA4 ADPCM: a 34-byte packet per channel gives 64 samples.  One wave per stream walks the stream's units in order,
//                 64 packets a round.  The step-index chain of a packet depends on the packet alone, so every lane first summarises
//                 its packet (sum, minimum and maximum of the running sum of its 64 deltas, last step index); a wave-uniform walk
//                 then gives every packet its starting predictor -- end = start + sum wherever start + min / max stays inside s16, a
//                 clamped serial decode of the packet where it does not -- and every lane decodes its packet from its true start.
//                 The state (predictor, step index per channel) enters with the stream's record and leaves through states_out.
//
// The carry rule between packets is QuickTime's: a packet whose header agrees with the carried state -- the same
// step index and a predictor within 0x7f -- continues from the carried full-precision predictor; any other packet restarts from its
// header.  The step index is the header's either way.
#include "ima_adpcm.h"
#include "pcm_group.h"

namespace sk {

namespace {

enum : uint32_t {  // enum sk_aiff_encoding
    kU8, kS8, kS16BE, kS16LE, kS24BE, kS32BE, kS32LE, kF32BE, kF64BE, kUlaw, kAlaw, kIma4, kUnassigned12, kF64LE,  // kF64LE = 13: appended, the range tests below rest on the order
    kDvdS24  // = 14: DVD LPCM's 24-bit packing, appended for the same reason
};

__device__ __forceinline__ int enc_in_bytes(uint32_t enc) {
    return enc <= kS8 || enc == kUlaw || enc == kAlaw ? 1 : (enc <= kS16LE ? 2 : (enc == kS24BE || enc == kDvdS24 ? 3 : (enc == kF64BE || enc == kF64LE ? 8 : 4)));
}
__device__ __forceinline__ int enc_out_bytes(uint32_t enc) {
    return enc == kS24BE || enc == kDvdS24 ? 3 : ((enc >= kS32BE && enc <= kF64BE) || enc == kF64LE ? 4 : 2);
}

// ITU-T G.711 expansion to 16-bit linear
__device__ __forceinline__ uint32_t ulaw_to_s16(uint32_t code) {
    const uint32_t u = ~code & 0xff;
    const int t = (int)((((u & 0x0f) << 3) + 0x84) << ((u >> 4) & 7));
    return (uint32_t)((u & 0x80) ? 0x84 - t : t - 0x84) & 0xffff;
}
__device__ __forceinline__ uint32_t alaw_to_s16(uint32_t code) {
    const uint32_t a = (code ^ 0x55) & 0xff;
    const uint32_t seg = (a >> 4) & 7;
    int t = (int)((a & 0x0f) << 4);
    t = seg == 0 ? t + 8 : ((t + 0x108) << (seg - 1));
    return (uint32_t)((a & 0x80) ? t : -t) & 0xffff;
}

// `f64 as f32` on the bits: round to nearest even, subnormal results kept, overflow to infinity, NaN to a quiet NaN
__device__ __forceinline__ uint32_t f64_bits_to_f32_bits(uint32_t hi, uint32_t lo) {
    const uint32_t sign = hi & 0x80000000u;
    const int exp = (int)((hi >> 20) & 0x7ff);
    const uint64_t man = ((uint64_t)(hi & 0xfffffu) << 32) | lo;
    if (exp == 0x7ff) return man ? (sign | 0x7fc00000u | (uint32_t)(man >> 29)) : (sign | 0x7f800000u);
    const int e = exp - 1023 + 127;
    if (e >= 255) return sign | 0x7f800000u;
    if (e <= 0) {  // a subnormal f32 or zero: the 53-bit significand shifted below the 2^-149 grid
        const int shift = 29 + 1 - e;
        if (exp == 0 || shift > 54) return sign;
        const uint64_t m = man | (1ull << 52);
        uint32_t q = (uint32_t)(m >> shift);
        const uint64_t rem = m & ((1ull << shift) - 1), half = 1ull << (shift - 1);
        if (rem > half || (rem == half && (q & 1))) q += 1;
        return sign | q;
    }
    uint32_t bits = ((uint32_t)e << 23) | (uint32_t)(man >> 29);
    const uint32_t rem = lo & 0x1fffffffu;
    if (rem > 0x10000000u || (rem == 0x10000000u && (bits & 1))) bits += 1;  // a carry runs into the exponent, up to infinity
    return sign | bits;
}

// raw = the sample's bytes as they lie in memory, little-endian packed (not for f64be)
__device__ __forceinline__ uint32_t elem_decode(uint32_t enc, uint32_t raw) {
    switch (enc) {
    case kU8: return ((raw - 128u) << 8) & 0xffff;
    case kS8: return (raw << 8) & 0xffff;
    case kS16BE: return bswap16(raw);
    case kS24BE: return be24(raw);
    case kS32BE: case kF32BE: return bswap32(raw);
    case kUlaw: return ulaw_to_s16(raw);
    case kAlaw: return alaw_to_s16(raw);
    default: return raw;  // sowt, 23ni
    }
}

// One 12-byte group of 24-bit DVD LPCM (four big-endian 16-bit high parts g[0..7], then the four low bytes g[8..11]) as the three dwords
// that hold it -> the three dwords of its four little-endian samples [g[8+i], g[2i+1], g[2i]].  Every output byte is one input byte:
// v_perm_b32 selects (0 ... 3: the second operand's bytes, 4 ... 7: the first's), one for the outer dwords, two for the middle one,
// whose bytes come from all three inputs.
__device__ __forceinline__ void dvd_s24_group(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t &o0, uint32_t &o1, uint32_t &o2) {
    o0 = __builtin_amdgcn_perm(w2, w0, 0x05000104u);                                          // g8 g1 g0 g9
    o1 = __builtin_amdgcn_perm(w1, __builtin_amdgcn_perm(w2, w0, 0x06060203u), 0x05020100u);  // g3 g2 g10 g5
    o2 = __builtin_amdgcn_perm(w2, w1, 0x02030700u);                                          // g4 g11 g7 g6
}

// 16 samples of OB = 2 or 3 bytes each as OB 16-byte stores
template <int OB>
__device__ __forceinline__ void store16(uint8_t *dst, const uint32_t (&v)[16]) {
    uint32_t o[4 * OB];
    if (OB == 2) {
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (v[2 * i] & 0xffff) | (v[2 * i + 1] << 16);
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {  // four 3-byte samples = three dwords
            o[3 * g] = (v[4 * g] & 0xffffff) | (v[4 * g + 1] << 24);
            o[3 * g + 1] = ((v[4 * g + 1] >> 8) & 0xffff) | (v[4 * g + 2] << 16);
            o[3 * g + 2] = ((v[4 * g + 2] >> 16) & 0xff) | (v[4 * g + 3] << 8);
        }
    }
    uint4 *out = reinterpret_cast<uint4 *>(dst);
#pragma unroll
    for (int i = 0; i < OB; ++i) out[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
}

__global__ __launch_bounds__(256) void k_aiff_elem(const AiffElemJob *jobs, uint32_t n_jobs) {
    const uint32_t j = blockIdx.y;
    if (j >= n_jobs) return;
    const AiffElemJob job = jobs[j];
    const uint32_t total = job.samples;
    const uint32_t s0 = blockIdx.x * kPcmSliceSamples + threadIdx.x * 16;
    if (s0 >= total) return;
    const uint32_t enc = job.enc;
    const int ib = enc_in_bytes(enc), ob = enc_out_bytes(enc);
    if (enc == kDvdS24) {  // DVD LPCM at 24 bits: a byte permutation inside every 12-byte group; total is a multiple of 4 (the host checks it)
        const uint8_t *src = job.src + (size_t)s0 * 3;
        uint8_t *dst = job.dst + (size_t)s0 * 3;
        if (s0 + 16 <= total) {  // four groups: three 16-byte loads, three 16-byte stores (a lane's offset is a multiple of 48)
            const uint4 *p = reinterpret_cast<const uint4 *>(src);
            const uint4 a = p[0], b = p[1], c = p[2];
            uint4 x, y, z;
            dvd_s24_group(a.x, a.y, a.z, x.x, x.y, x.z);
            dvd_s24_group(a.w, b.x, b.y, x.w, y.x, y.y);
            dvd_s24_group(b.z, b.w, c.x, y.z, y.w, z.x);
            dvd_s24_group(c.y, c.z, c.w, z.y, z.z, z.w);
            uint4 *d = reinterpret_cast<uint4 *>(dst);
            d[0] = x, d[1] = y, d[2] = z;
            return;
        }
        // the unit's last 4, 8 or 12 samples: group by group, dword loads and stores (a group's offset is a multiple of 4)
        for (uint32_t s = s0; s + 4 <= total; s += 4, src += 12, dst += 12) {
            const uint32_t *p = reinterpret_cast<const uint32_t *>(src);
            uint32_t *d = reinterpret_cast<uint32_t *>(dst);
            uint32_t o0, o1, o2;
            dvd_s24_group(p[0], p[1], p[2], o0, o1, o2);
            d[0] = o0, d[1] = o1, d[2] = o2;
        }
        return;
    }
    if (s0 + 16 <= total && ib == 4) {  // 4-byte samples move dword for dword: four 16-byte loads, four 16-byte stores
        const uint4 *p = reinterpret_cast<const uint4 *>(job.src + (size_t)s0 * 4);
        uint4 *d = reinterpret_cast<uint4 *>(job.dst + (size_t)s0 * 4);
        const bool swap = enc != kS32LE;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint4 q = p[k];
            if (swap) q = make_uint4(bswap32(q.x), bswap32(q.y), bswap32(q.z), bswap32(q.w));
            d[k] = q;
        }
        return;
    }
    if (s0 + 16 <= total && enc == kF64LE) {  // f64le: as f64be below, the dwords as they lie (the low one first)
        const uint4 *p = reinterpret_cast<const uint4 *>(job.src + (size_t)s0 * 8);
        uint4 *d = reinterpret_cast<uint4 *>(job.dst + (size_t)s0 * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 q0 = p[2 * k], q1 = p[2 * k + 1];
            d[k] = make_uint4(f64_bits_to_f32_bits(q0.y, q0.x), f64_bits_to_f32_bits(q0.w, q0.z), f64_bits_to_f32_bits(q1.y, q1.x),
                              f64_bits_to_f32_bits(q1.w, q1.z));
        }
        return;
    }
    if (s0 + 16 <= total && ib == 8) {  // f64be: eight 16-byte loads, four 16-byte stores
        const uint4 *p = reinterpret_cast<const uint4 *>(job.src + (size_t)s0 * 8);
        uint4 *d = reinterpret_cast<uint4 *>(job.dst + (size_t)s0 * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 q0 = p[2 * k], q1 = p[2 * k + 1];
            d[k] = make_uint4(f64_bits_to_f32_bits(bswap32(q0.x), bswap32(q0.y)), f64_bits_to_f32_bits(bswap32(q0.z), bswap32(q0.w)),
                              f64_bits_to_f32_bits(bswap32(q1.x), bswap32(q1.y)), f64_bits_to_f32_bits(bswap32(q1.z), bswap32(q1.w)));
        }
        return;
    }
    // Every width has its own loads, its own stores and its own return.  With the three store forms behind one shared conversion
    // hipcc 7.2 merged their tails and stored samples 9 ... 15 of the 4-byte form from registers no path had written.
    if (s0 + 16 <= total) {  // 1-, 2- and 3-byte samples
        uint32_t raw[16], v[16];
        if (ib == 1) {
            const uint4 q = *reinterpret_cast<const uint4 *>(job.src + s0);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int s = 0; s < 16; ++s) raw[s] = (w[s >> 2] >> (8 * (s & 3))) & 0xff;
        } else if (ib == 2) {
            load_group_fmt<2>(job.src, s0, raw);
        } else {
            load_group_fmt<3>(job.src, s0, raw);
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) v[s] = elem_decode(enc, raw[s]);
        uint8_t *dst = job.dst + (size_t)s0 * ob;
        if (ob == 2) store16<2>(dst, v);
        else store16<3>(dst, v);
        return;
    }
    // the unit's last, incomplete group: sample by sample
    for (uint32_t s = s0; s < total; ++s) {
        const uint8_t *p = job.src + (size_t)s * ib;
        uint32_t v;
        if (enc == kF64LE) {
            const uint32_t lo = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
            const uint32_t hi = (uint32_t)p[4] | ((uint32_t)p[5] << 8) | ((uint32_t)p[6] << 16) | ((uint32_t)p[7] << 24);
            v = f64_bits_to_f32_bits(hi, lo);
        } else if (ib == 8) {
            const uint32_t hi = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
            const uint32_t lo = ((uint32_t)p[4] << 24) | ((uint32_t)p[5] << 16) | ((uint32_t)p[6] << 8) | p[7];
            v = f64_bits_to_f32_bits(hi, lo);
        } else {
            v = elem_decode(enc, ib == 1 ? (uint32_t)p[0] : load_raw_scalar(p, ib));
        }
        store_raw_scalar(job.dst + (size_t)s * ob, v, ob);
    }
}

// ---- IMA4 ----------------------------------------------------------------------------------------------------------------------

// (the step table and the per-nibble arithmetic: ima_adpcm.h, shared with wav_adpcm.hip)
constexpr int kImaPacket = 34;

// where packet `pk` (in LDS) ends when it starts at `start`: the reference's arithmetic, nibble by nibble
__device__ int ima_serial_end(const uint8_t *pk, const int *step, int start, int idx) {
    int p = start;
    for (int b = 0; b < 32; ++b) {
        const uint32_t byte = pk[2 + b];
        p = clamp_s16(p + ima_delta(step[idx], byte & 15));
        idx = ima_next_index(idx, byte & 15);
        p = clamp_s16(p + ima_delta(step[idx], byte >> 4));
        idx = ima_next_index(idx, byte >> 4);
    }
    return p;
}

__global__ __launch_bounds__(64) void k_aiff_ima4(const AiffImaStream *streams, uint32_t n_streams, const AiffImaUnit *units, uint32_t *states_out) {
    __shared__ __attribute__((aligned(16))) uint8_t pk[64 * kImaPacket];
    __shared__ int s_step[89];
    __shared__ int s_sum[64], s_min[64], s_max[64], s_hdr[64];  // s_hdr: header predictor << 16 | header index << 8 | end index
    const uint32_t stream = blockIdx.x, lane = threadIdx.x;
    if (stream >= n_streams) return;
    for (uint32_t i = lane; i < 89; i += 64) s_step[i] = kImaStep[i];
    const AiffImaStream st = streams[stream];
    const uint32_t ch = st.channels;
    int p0 = st.predictor[0], p1 = st.predictor[1];
    int i0 = st.step_index[0] > 88 ? 88 : st.step_index[0], i1 = st.step_index[1] > 88 ? 88 : st.step_index[1];
    __syncthreads();
    for (uint32_t u = 0; u < st.n_units; ++u) {
        const AiffImaUnit unit = units[st.first_unit + u];
        const uint32_t total = unit.groups * ch;  // packets
        for (uint32_t first = 0; first < total; first += 64) {
            const uint32_t n = min(64u, total - first), nbytes = n * kImaPacket;
            const uint8_t *src = unit.src + (size_t)first * kImaPacket;  // 64 packets are 2176 bytes: 16-byte aligned again
            for (uint32_t i = lane; i * 16 < nbytes; i += 64) {
                if (i * 16 + 16 <= nbytes) {
                    reinterpret_cast<uint4 *>(pk)[i] = reinterpret_cast<const uint4 *>(src)[i];
                } else {
                    for (uint32_t k = i * 16; k < nbytes; k += 2) *reinterpret_cast<uint16_t *>(pk + k) = *reinterpret_cast<const uint16_t *>(src + k);
                }
            }
            __syncthreads();
            // ---- every lane: its packet into registers, and the packet's summary ----
            uint32_t w[8];
            int hdr_pred = 0, hdr_idx = 0;
            if (lane < n) {
                const uint16_t *h = reinterpret_cast<const uint16_t *>(pk + lane * kImaPacket);
                const uint32_t h0 = h[0];
                const uint32_t word = ((h0 & 0xff) << 8) | (h0 >> 8);
                hdr_pred = (int)(int16_t)(word & 0xff80);
                hdr_idx = (int)(word & 0x7f);
                if (hdr_idx > 88) hdr_idx = 88;
#pragma unroll
                for (int i = 0; i < 8; ++i) w[i] = (uint32_t)h[1 + 2 * i] | ((uint32_t)h[2 + 2 * i] << 16);
                int idx = hdr_idx, acc = 0, lo = 0, hi = 0;
#pragma unroll
                for (int t = 0; t < 64; ++t) {
                    const uint32_t nib = (w[t >> 3] >> (4 * (t & 7))) & 15;
                    acc += ima_delta(s_step[idx], nib);
                    idx = ima_next_index(idx, nib);
                    lo = min(lo, acc);
                    hi = max(hi, acc);
                }
                s_sum[lane] = acc, s_min[lane] = lo, s_max[lane] = hi;
                s_hdr[lane] = (int)(((uint32_t)hdr_pred << 16) | ((uint32_t)hdr_idx << 8) | (uint32_t)idx);
            }
            __syncthreads();
            // ---- the walk: every lane the same steps (LDS broadcasts), each keeps its own packet's start ----
            int my_start = 0;
            for (uint32_t k = 0; k < n; ++k) {
                const bool second = ch == 2 && (k & 1);
                const int hd = s_hdr[k];
                const int hp = hd >> 16, hx = (hd >> 8) & 0xff, ex = hd & 0xff;
                const int carried = second ? p1 : p0, carried_idx = second ? i1 : i0;
                const int diff = hp - carried;
                const int start = (carried_idx == hx && diff >= -0x7f && diff <= 0x7f) ? carried : hp;
                if (k == lane) my_start = start;
                int end;
                if (start + s_min[k] >= -32768 && start + s_max[k] <= 32767) end = start + s_sum[k];
                else end = ima_serial_end(pk + k * kImaPacket, s_step, start, hx);
                if (second) p1 = end, i1 = ex;
                else p0 = end, i0 = ex;
            }
            // ---- every lane: its packet from its true start, as 32 dwords of two samples ----
            uint32_t out[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) out[i] = 0;
            if (lane < n) {
                int idx = hdr_idx, p = my_start;
#pragma unroll
                for (int t = 0; t < 64; ++t) {
                    const uint32_t nib = (w[t >> 3] >> (4 * (t & 7))) & 15;
                    p = clamp_s16(p + ima_delta(s_step[idx], nib));
                    idx = ima_next_index(idx, nib);
                    if (t & 1) out[t >> 1] |= (uint32_t)p << 16;
                    else out[t >> 1] = (uint32_t)p & 0xffff;
                }
            }
            if (ch == 2) {
                // lanes 2g and 2g + 1 hold the two channels of group g: the even lane writes frames 0 .. 31, the odd one 32 .. 63
                const bool odd = lane & 1;
                uint32_t mix[32];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const uint32_t got = (uint32_t)__shfl_xor((int)(odd ? out[i] : out[16 + i]), 1);
                    const uint32_t keep = odd ? out[16 + i] : out[i];
                    const uint32_t l = odd ? got : keep, r = odd ? keep : got;
                    mix[2 * i] = (l & 0xffff) | (r << 16);
                    mix[2 * i + 1] = (l >> 16) | (r & 0xffff0000u);
                }
#pragma unroll
                for (int i = 0; i < 32; ++i) out[i] = mix[i];
            }
            if (lane < n) {
                uint4 *dst = reinterpret_cast<uint4 *>(unit.dst + ((size_t)first + lane) * 128);
#pragma unroll
                for (int i = 0; i < 8; ++i) dst[i] = make_uint4(out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]);
            }
            __syncthreads();  // the packets in LDS are replaced in the next round
        }
    }
    if (lane == 0) {
        states_out[2 * stream] = ((uint32_t)p0 & 0xffff) | ((uint32_t)i0 << 16);
        states_out[2 * stream + 1] = ((uint32_t)p1 & 0xffff) | ((uint32_t)i1 << 16);
    }
}

}  // namespace

hipError_t launch_aiff_elem(const AiffElemJob *jobs, uint32_t n_jobs, uint32_t max_samples, hipStream_t s) {
    if (n_jobs == 0 || max_samples == 0) return hipSuccess;
    const uint32_t slices = (max_samples + kPcmSliceSamples - 1) / kPcmSliceSamples;
    for (uint32_t j0 = 0; j0 < n_jobs; j0 += 65535) {
        const uint32_t n = n_jobs - j0 < 65535 ? n_jobs - j0 : 65535;
        hipLaunchKernelGGL(k_aiff_elem, dim3(slices, n), dim3(256), 0, s, jobs + j0, n);
    }
    return hipGetLastError();
}

hipError_t launch_aiff_ima4(const AiffImaStream *streams, uint32_t n_streams, const AiffImaUnit *units, uint32_t *states_out, hipStream_t s) {
    if (n_streams == 0) return hipSuccess;
    hipLaunchKernelGGL(k_aiff_ima4, dim3(n_streams), dim3(64), 0, s, streams, n_streams, units, states_out);
    return hipGetLastError();
}

}  // namespace sk

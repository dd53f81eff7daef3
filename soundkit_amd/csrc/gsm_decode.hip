// gsm_decode.hip -- the GSM 06.10 full-rate decode stage for gfx950 (sk_gsm_decode, sk_gsm_decode_batch, sk_tick_run_gsm; engine.cpp):
// 33-byte frames (or the Microsoft framing's 65-byte pairs) to s16le, bit for bit what libgsm's gsm_decode gives behind the reference's
// GsmDecoder.  Integers only, all arithmetic in 32-bit registers: every operand is a 16-bit value, so a product fits 31 bits and
// MULT_R needs no truncation (the one product that would, -32768 x -32768, cannot occur: QLB, FAC, INVA and 28180 are positive and a
// reflection coefficient's magnitude stays below 32768).
//
// The frame's 260 parameter bits are read where they lie -- MSB first from bit `base_bit + frame x stride_bits` of the unit, which
// covers both framings -- out of aligned dwords that hold bytes of the unit.
//
//   k_gsm_excite  one stream per wave, lanes 0 ... 39 one sample of the subframe each: RPE decoding (a lane's sample is one of the 13
//                 pulses or zero) and long-term synthesis.  The lag Nr is at least 40, so drp[k - Nr] always lies in earlier
//                 subframes and the 40 samples are independent; only the walk over subframes is serial.  The 120-sample history is a
//                 ring in LDS.  The reconstructed short-term residual leaves as s16 in the workspace; dp and nrp are carried.
//   k_gsm_synth   one stream per lane: per frame the LAR decoding, the four interpolation segments and the 8-stage lattice over 160
//                 samples with rrp[8] and v[8] in registers, then the de-emphasis; eight s16 leave as one 16-byte store.  v, msr and
//                 LARpp are carried.
//
// The split keeps the serial lane's walk to what is serial in the sample -- the lattice and the de-emphasis -- and takes the
// dynamically indexed history out of it.
#include "sk_device.h"

namespace sk {

namespace {

__device__ __forceinline__ int gsm_sat(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
__device__ __forceinline__ int gsm_mult_r(int a, int b) { return (__mul24(a, b) + 16384) >> 15; }

// n <= 25 bits, MSB first, from bit index `bit` of the unit.  The second dword is read only when the field reaches into it, so
// nothing beyond the dword that holds the field's last byte is touched.
__device__ __forceinline__ uint32_t gsm_bits(const uint32_t *w, uint32_t bit, uint32_t n) {
    const uint32_t i = bit >> 5, sh = bit & 31;
    uint32_t v = __builtin_bswap32(w[i]) << sh;
    if (sh + n > 32) v |= __builtin_bswap32(w[i + 1]) >> (32 - sh);
    return v >> (32 - n);
}

constexpr uint32_t kDp = 0, kV = 120, kMsr = 128, kNrp = 129, kLarpp = 130;  // sk_gsm_state's words

__global__ __launch_bounds__(64) void k_gsm_excite(const GsmStream *streams, uint32_t n_streams, const GsmUnit *units, const int32_t *states_in,
                                                   int32_t *states_out, int16_t *ws) {
    __shared__ int ring[120];  // the history: the sample at position q of the stream's walk lies in slot q % 120
    const uint32_t idx = blockIdx.x, lane = threadIdx.x;
    if (idx >= n_streams) return;
    const GsmStream st = streams[idx];
    const int32_t *in = states_in + (size_t)st.state * kGsmStateWords;
    int32_t *out = states_out + (size_t)st.state * kGsmStateWords;
    ring[lane] = in[kDp + lane];
    if (lane < 56) ring[64 + lane] = in[kDp + 64 + lane];
    int nrp = in[kNrp];
    __syncthreads();
    uint32_t pos = 0;  // slot of the next subframe's first sample: 0, 40 or 80
    int16_t *wt = ws + st.ws_offset;
    for (uint32_t u = 0; u < st.n_units; ++u) {
        const GsmUnit unit = units[st.first_unit + u];
        const uint32_t *w = reinterpret_cast<const uint32_t *>(unit.src);
        for (uint32_t f = 0; f < unit.frames; ++f) {
            const uint32_t bit = st.base_bit + f * st.stride_bits + 36;
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t at = bit + 56 * j;
                const uint32_t head = gsm_bits(w, at, 17);  // Nc 7 | bc 2 | Mc 2 | xmaxc 6
                const int nc = head >> 10, bc = (head >> 8) & 3, mc = (head >> 6) & 3, xmaxc = head & 63;
                // the block maximum's exponent and mantissa
                int exp = xmaxc > 15 ? (xmaxc >> 3) - 1 : 0;
                int mant = xmaxc - (exp << 3);
                if (mant == 0) {
                    exp = -4, mant = 7;
                } else {
                    while (mant <= 7) mant = mant << 1 | 1, --exp;
                    mant -= 8;
                }
                const int t1 = 18431 + 2048 * mant;  // FAC[mant]
                const int t2 = 6 - exp, t3 = t2 ? 1 << (t2 - 1) : 0;
                const int nr = (nc < 40 || nc > 120) ? nrp : nc;
                nrp = nr;
                const int brp = bc == 0 ? 3277 : (bc == 1 ? 11469 : (bc == 2 ? 21299 : 32767));  // QLB[bc]
                int drp = 0;
                if (lane < 40) {
                    // this lane's sample is pulse i when lane = Mc + 3 i
                    const int d = (int)lane - mc, i = d / 3;
                    int erp = 0;
                    if (d >= 0 && d == 3 * i && i < 13) {
                        const int xmc = (int)gsm_bits(w, at + 17 + 3 * i, 3);
                        erp = gsm_sat(gsm_mult_r(t1, ((xmc << 1) - 7) << 12) + t3) >> t2;
                    }
                    uint32_t slot = pos + lane + 120 - (uint32_t)nr;  // position - Nr, mod 120: below 240
                    slot = slot >= 120 ? slot - 120 : slot;
                    drp = gsm_sat(erp + gsm_mult_r(brp, ring[slot]));
                }
                __syncthreads();  // a lag above 80 reads slots that this subframe writes
                if (lane < 40) {
                    ring[pos + lane] = drp;
                    wt[lane] = (int16_t)drp;
                }
                __syncthreads();
                pos = pos == 80 ? 0 : pos + 40;
                wt += 40;
            }
        }
    }
    // oldest first again
    for (uint32_t k = lane; k < 120; k += 64) out[kDp + k] = ring[pos + k >= 120 ? pos + k - 120 : pos + k];
    if (lane == 0) out[kNrp] = nrp;
}

// LARp of one coefficient in segment seg (samples 0-12, 13-26, 27-39, 40-159) -> the reflection coefficient
__device__ __forceinline__ int gsm_rrp(int p, int c, int seg) {
    int larp;
    if (seg == 0) larp = gsm_sat(gsm_sat((p >> 2) + (c >> 2)) + (p >> 1));
    else if (seg == 1) larp = gsm_sat((p >> 1) + (c >> 1));
    else if (seg == 2) larp = gsm_sat(gsm_sat((p >> 2) + (c >> 2)) + (c >> 1));
    else larp = c;
    int t = larp < 0 ? (larp == -32768 ? 32767 : -larp) : larp;
    t = t < 11059 ? t << 1 : (t < 20070 ? t + 11059 : gsm_sat((t >> 2) + 26112));
    return larp < 0 ? -t : t;
}

__device__ __forceinline__ int gsm_lar(int larc, int mic, int b, int inva) {
    int t = gsm_sat(larc + mic) << 10;
    t = gsm_sat(t - (b << 1));
    t = gsm_mult_r(inva, t);
    return gsm_sat(t + t);
}

__global__ __launch_bounds__(64) void k_gsm_synth(const GsmStream *streams, uint32_t n_streams, const GsmUnit *units, const int32_t *states_in,
                                                  int32_t *states_out, const int16_t *ws) {
    const uint32_t idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= n_streams) return;
    const GsmStream st = streams[idx];
    const int32_t *in = states_in + (size_t)st.state * kGsmStateWords;
    int32_t *out = states_out + (size_t)st.state * kGsmStateWords;
    int v[8], p[8], c[8], rrp[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = in[kV + i], p[i] = in[kLarpp + i], c[i] = 0, rrp[i] = 0;
    int msr = in[kMsr];
    const uint4 *wt = reinterpret_cast<const uint4 *>(ws + st.ws_offset);  // frames of 320 bytes from a 16-byte aligned base
    for (uint32_t u = 0; u < st.n_units; ++u) {
        const GsmUnit unit = units[st.first_unit + u];
        const uint32_t *w = reinterpret_cast<const uint32_t *>(unit.src);
        uint4 *dst = reinterpret_cast<uint4 *>(unit.dst);
        for (uint32_t f = 0; f < unit.frames; ++f) {
            const uint32_t bit = st.base_bit + f * st.stride_bits;
            const uint32_t a = gsm_bits(w, bit, 22), b = gsm_bits(w, bit + 22, 14);  // LARc 6 6 5 5 | 4 4 3 3
            c[0] = gsm_lar(a >> 16, -32, 0, 13107);
            c[1] = gsm_lar((a >> 10) & 63, -32, 0, 13107);
            c[2] = gsm_lar((a >> 5) & 31, -16, 2048, 13107);
            c[3] = gsm_lar(a & 31, -16, -2560, 13107);
            c[4] = gsm_lar(b >> 10, -8, 94, 19223);
            c[5] = gsm_lar((b >> 6) & 15, -8, -1792, 17476);
            c[6] = gsm_lar((b >> 3) & 7, -4, -341, 31454);
            c[7] = gsm_lar(b & 7, -4, -1144, 29708);
            for (uint32_t g = 0; g < 20; ++g) {  // eight samples a step: one 16-byte load, one 16-byte store
                const uint4 x = wt[g];
                const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
                uint32_t ys[4];
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    // the segments begin at samples 0, 13, 27 and 40: (g, t) = (0, 0), (1, 5), (3, 3), (5, 0)
                    if (t == 0 || t == 3 || t == 5) {
                        const int seg = t == 0 ? (g == 0 ? 0 : (g == 5 ? 3 : -1)) : (t == 5 ? (g == 1 ? 1 : -1) : (g == 3 ? 2 : -1));
                        if (seg >= 0) {
#pragma unroll
                            for (int i = 0; i < 8; ++i) rrp[i] = gsm_rrp(p[i], c[i], seg);
                        }
                    }
                    int sri = (int)(int16_t)(xs[t >> 1] >> (16 * (t & 1)));
#pragma unroll
                    for (int i = 7; i >= 0; --i) {
                        sri = gsm_sat(sri - gsm_mult_r(rrp[i], v[i]));
                        if (i < 7) v[i + 1] = gsm_sat(v[i] + gsm_mult_r(rrp[i], sri));  // v[8] is never read
                    }
                    v[0] = sri;
                    msr = gsm_sat(sri + gsm_mult_r(msr, 28180));
                    const uint32_t y = (uint32_t)gsm_sat(msr + msr) & 0xFFF8u;
                    ys[t >> 1] = (t & 1) ? ys[t >> 1] | (y << 16) : y;
                }
                dst[g] = make_uint4(ys[0], ys[1], ys[2], ys[3]);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) p[i] = c[i];
            wt += 20, dst += 20;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) out[kV + i] = v[i], out[kLarpp + i] = p[i];
    out[kMsr] = msr;
}

}  // namespace

hipError_t launch_gsm(const GsmStream *streams, uint32_t n_streams, const GsmUnit *units, const int32_t *states_in, int32_t *states_out, int16_t *ws,
                      hipStream_t s) {
    if (n_streams == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gsm_excite, dim3(n_streams), dim3(64), 0, s, streams, n_streams, units, states_in, states_out, ws);
    hipLaunchKernelGGL(k_gsm_synth, dim3((n_streams + 63) / 64), dim3(64), 0, s, streams, n_streams, units, states_in, states_out, ws);
    return hipGetLastError();
}

}  // namespace sk

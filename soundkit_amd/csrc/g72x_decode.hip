// g72x_decode.hip -- the telephony streams' decode stage for gfx950 (sk_g72x_decode, sk_g72x_decode_batch, sk_tick_run_g72x;
// engine.cpp): headerless G.726 (16 / 24 / 32 / 40 kbit/s, both packings) and G.722 (64 kbit/s) bytes to s16le, bit for bit what the
// reference's G726Decoder and G722Decoder give.  Integers only.  G.711 has no kernel here: its two expansions are k_aiff_elem's
// (aiff_decode.hip), reached through launch_aiff_elem.
//
//   k_g726        one stream per lane.  The recurrence is serial in the sample (every sample rewrites both predictors and the
//                 quantiser scale), so the parallelism is across streams.  A lane walks its stream's units in order, two samples a
//                 step: each code comes out of two aligned dwords of the unit, the two s16 leave as one 4-byte store (a wider
//                 store needs a second loop for the rest, see the kernel).  Rate and packing are the lane's
//                 own, so a launch mixes them; the per-rate tables are read from constant memory.  The state (sk_g726_state, 24
//                 words) enters from states_in and leaves through states_out.
//   k_g722_adpcm  one stream per lane: both ADPCM bands of every byte, (rlow, rhigh) packed into one word of the workspace per byte,
//                 the two bands' state carried as above.  The first 22 - 2n words of the QMF carry of a stream of n < 11 bytes are
//                 moved up here, where one lane has the stream to itself.
//   k_g722_qmf    one output pair per lane: the 24-tap receive filter over the workspace and, for a stream's first 11 pairs, over
//                 the 22-entry carry; the last 11 pairs of a call become the new carry.
//
// Splitting G.722 keeps the serial walk to the part that is serial: the filter is 24 multiplies a pair that no lane has to wait for.
#include "sk_device.h"

namespace sk {

namespace {

// ---- G.726 -----------------------------------------------------------------------------------------------------------------------

// the rates' tables one behind the other: 2-bit codes at 0, 3-bit at 4, 4-bit at 12, 5-bit at 28 (= (1 << bits) - 4)
__constant__ int16_t kDqln[60] = {
    116, 365, 365, 116,
    -2048, 135, 273, 373, 373, 273, 135, -2048,
    -2048, 4, 135, 213, 273, 323, 373, 425, 425, 373, 323, 273, 213, 135, 4, -2048,
    -2048, -66, 28, 104, 169, 224, 274, 318, 358, 395, 429, 459, 488, 514, 539, 566,
    566, 539, 514, 488, 459, 429, 395, 358, 318, 274, 224, 169, 104, 28, -66, -2048};
__constant__ int16_t kWi[60] = {
    -22, 439, 439, -22,
    -4, 30, 137, 582, 582, 137, 30, -4,
    -12, 18, 41, 64, 112, 198, 355, 1122, 1122, 355, 198, 112, 64, 41, 18, -12,
    14, 14, 24, 39, 40, 41, 58, 100, 141, 179, 219, 280, 358, 440, 529, 696,
    696, 529, 440, 358, 280, 219, 179, 141, 100, 58, 41, 40, 39, 24, 14, 14};
__constant__ int16_t kFi[60] = {
    0, 0xE00, 0xE00, 0,
    0, 0x200, 0x400, 0xE00, 0xE00, 0x400, 0x200, 0,
    0, 0, 0, 0x200, 0x200, 0x200, 0x600, 0xE00, 0xE00, 0x600, 0x200, 0x200, 0x200, 0, 0, 0,
    0, 0, 0, 0, 0, 0x200, 0x200, 0x200, 0x200, 0x200, 0x400, 0x600, 0x800, 0xA00, 0xC00, 0xC00,
    0xC00, 0xC00, 0xA00, 0x800, 0x600, 0x400, 0x200, 0x200, 0x200, 0x200, 0x200, 0, 0, 0, 0, 0};

struct G726Regs {  // sk_g726_state in registers
    int yl, yu, dms, dml, ap;
    int a[2], b[6], pk[2], dq[6], sr[2], td;
};

// the reference's quan over 1, 2, 4 ... 16384: the bit length, at most 15
__device__ __forceinline__ int bit_length15(int v) {
    const int n = 32 - __clz(v);
    return v <= 0 ? 0 : (n > 15 ? 15 : n);
}

__device__ __forceinline__ int fmult(int an, int srn) {
    const int anmag = an > 0 ? an : ((-an) & 0x1FFF);
    const int anexp = bit_length15(anmag) - 6;
    const int anmant = anmag == 0 ? 32 : (anexp >= 0 ? anmag >> anexp : anmag << -anexp);
    const int wanexp = anexp + ((srn >> 6) & 0xF) - 13;
    const int wanmant = (anmant * (srn & 0x3F) + 0x30) >> 4;
    const int ret = wanexp >= 0 ? ((wanmant << wanexp) & 0x7FFF) : (wanmant >> -wanexp);
    return (an ^ srn) < 0 ? -ret : ret;
}

// magnitude to the 4-bit exponent, 6-bit mantissa form the predictors multiply in
__device__ __forceinline__ int float_form(int mag) {
    const int exp = bit_length15(mag);
    return (exp << 6) + ((mag << 6) >> exp);
}

__device__ __forceinline__ int clamp_i(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one code through G726Core::decode_code; bits = 2 ... 5
__device__ int g726_decode_code(G726Regs &s, uint32_t code, int bits) {
    const int base = (1 << bits) - 4;
    const bool wide = bits == 5;
    int sezi = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) sezi += fmult(s.b[k] >> 2, s.dq[k]);
    const int sez = sezi >> 1;
    const int se = (sezi + fmult(s.a[1] >> 2, s.sr[1]) + fmult(s.a[0] >> 2, s.sr[0])) >> 1;
    // step size
    int y;
    if (s.ap >= 256) {
        y = s.yu;
    } else {
        y = s.yl >> 6;
        const int dif = s.yu - y, al = s.ap >> 2;
        if (dif > 0) y += (dif * al) >> 6;
        else if (dif < 0) y += (dif * al + 0x3F) >> 6;
    }
    // reconstruct
    const bool sign = (code >> (bits - 1)) & 1;
    const int dql = (int)kDqln[base + code] + (y >> 2);
    int dq;
    if (dql < 0) {
        dq = sign ? -0x8000 : 0;
    } else {
        const int dex = (dql >> 7) & 15, dqt = 128 + (dql & 127);
        dq = (dqt << 7) >> (14 - dex);
        if (sign) dq -= 0x8000;
    }
    const int sr = dq < 0 ? se - (dq & (wide ? 0x7FFF : 0x3FFF)) : se + dq;
    const int dqsez = sr - se + sez;
    const int wi = (int)kWi[base + code] * 32, fi = kFi[base + code];

    // ---- update ----
    const int pk0 = dqsez < 0 ? 1 : 0;
    const int mag = dq & 0x7FFF;
    const int ylint = s.yl >> 15, ylfrac = (s.yl >> 10) & 0x1F;
    const int thr1 = (32 + ylfrac) << ylint;
    const int thr2 = ylint > 9 ? (31 << 10) : thr1;
    const int dqthr = (thr2 + (thr2 >> 1)) >> 1;
    const bool tr = s.td != 0 && mag > dqthr;

    s.yu = clamp_i(y + ((wi - y) >> 5), 544, 5120);
    s.yl += s.yu + ((-s.yl) >> 6);

    int a2p = 0;
    if (tr) {
        s.a[0] = s.a[1] = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s.b[k] = 0;
    } else {
        const int pks1 = pk0 ^ s.pk[0];
        a2p = s.a[1] - (s.a[1] >> 7);
        if (dqsez != 0) {
            const int fa1 = pks1 ? s.a[0] : -s.a[0];
            if (fa1 < -8191) a2p -= 0x100;
            else if (fa1 > 8191) a2p += 0xFF;
            else a2p += fa1 >> 5;
            if (pk0 ^ s.pk[1]) {
                if (a2p <= -12160) a2p = -12288;
                else if (a2p >= 12416) a2p = 12288;
                else a2p -= 0x80;
            } else if (a2p <= -12416) {
                a2p = -12288;
            } else if (a2p >= 12160) {
                a2p = 12288;
            } else {
                a2p += 0x80;
            }
        }
        s.a[1] = a2p;
        s.a[0] -= s.a[0] >> 8;
        if (dqsez != 0) s.a[0] += pks1 == 0 ? 192 : -192;
        const int a1ul = 15360 - a2p;
        s.a[0] = clamp_i(s.a[0], -a1ul, a1ul);
        const int decay = wide ? 9 : 8;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            s.b[k] -= s.b[k] >> decay;
            if (mag != 0) s.b[k] += (dq ^ s.dq[k]) >= 0 ? 128 : -128;
        }
    }
#pragma unroll
    for (int k = 5; k > 0; --k) s.dq[k] = s.dq[k - 1];
    if (mag == 0) s.dq[0] = dq >= 0 ? 0x20 : -0x3E0;
    else s.dq[0] = dq >= 0 ? float_form(mag) : float_form(mag) - 0x400;

    s.sr[1] = s.sr[0];
    if (sr == 0) s.sr[0] = 0x20;
    else if (sr > 0) s.sr[0] = float_form(sr);
    else if (sr > -32768) s.sr[0] = float_form(-sr) - 0x400;
    else s.sr[0] = -0x3E0;

    s.pk[1] = s.pk[0];
    s.pk[0] = pk0;
    s.td = tr ? 0 : (a2p < -11776 ? 1 : 0);
    s.dms += (fi - s.dms) >> 5;
    s.dml += ((fi << 2) - s.dml) >> 7;
    if (tr) {
        s.ap = 256;
    } else {
        const int d = (s.dms << 2) - s.dml;
        if (y < 1536 || s.td != 0 || (d < 0 ? -d : d) >= (s.dml >> 3)) s.ap += (0x200 - s.ap) >> 4;
        else s.ap += (-s.ap) >> 4;
    }
    return clamp_i(sr * 4, -32768, 32767);
}

// the code that begins at bit q of the unit: two bytes hold it (at most 7 + 5 bits).  They come out of two aligned dwords that lie
// inside the unit's (len + 3) / 4 dwords -- nothing beyond the dword that holds the unit's last byte is touched; what the second
// byte holds beyond the unit is shifted or masked away, since the unit ends with a whole code.
__device__ __forceinline__ uint32_t take_code(const uint8_t *src, uint32_t q, uint32_t len, int bits, bool right) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(src);
    const uint32_t pos = q >> 3, off = q & 7, last = (len - 1) >> 2, i = pos >> 2;
    const uint32_t two = __builtin_amdgcn_alignbyte(w[i + 1 > last ? last : i + 1], w[i], pos & 3) & 0xffff;  // byte pos | byte pos + 1 << 8
    const uint32_t mask = (1u << bits) - 1;
    if (right) return (two >> off) & mask;                        // LSB first
    const uint32_t be = ((two & 0xff) << 8) | (two >> 8);         // MSB first: the two bytes as one big-endian number
    return (be >> (16 - off - bits)) & mask;
}

__global__ __launch_bounds__(64) void k_g726(const G72xStream *streams, uint32_t n_streams, const G72xUnit *units, const int32_t *states_in,
                                             int32_t *states_out) {
    const uint32_t idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= n_streams) return;
    const G72xStream st = streams[idx];
    const int32_t *in = states_in + (size_t)st.state * kG726StateWords;
    G726Regs s;
    s.yl = in[0], s.yu = in[1], s.dms = in[2], s.dml = in[3], s.ap = in[4];
    s.a[0] = in[5], s.a[1] = in[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) s.b[k] = in[7 + k], s.dq[k] = in[15 + k];
    s.pk[0] = in[13], s.pk[1] = in[14], s.sr[0] = in[21], s.sr[1] = in[22], s.td = in[23];
    const int bits = st.bits;
    const bool right = st.packing != 0;
    for (uint32_t u = 0; u < st.n_units; ++u) {
        const G72xUnit *up = units + st.first_unit + u;
        const uint32_t len = up->bytes;
        if (len == 0) continue;
        const uint8_t *const src = up->src;
        uint8_t *const dst_base = up->dst;
        // two samples a step (every group holds an even number): one decode body twice, one 4-byte store.  Eight samples a step with
        // a 16-byte store and a second loop for the rest made the compiler copy the state's registers in pairs with packed moves,
        // which the default build keeps clear of (tests/test_build_flavour.py); the walk is bound by its arithmetic, not by its stores.
        const uint32_t pairs = len * 4 / (uint32_t)bits;  // len * 8 / bits codes
        uint32_t *dst = reinterpret_cast<uint32_t *>(dst_base);
        for (uint32_t i = 0; i < pairs; ++i) {
            const uint32_t q = i * 2 * bits;
            const int a = g726_decode_code(s, take_code(src, q, len, bits, right), bits);
            const int b = g726_decode_code(s, take_code(src, q + bits, len, bits, right), bits);
            dst[i] = ((uint32_t)a & 0xffff) | ((uint32_t)b << 16);
        }
    }
    int32_t *out = states_out + (size_t)st.state * kG726StateWords;
    out[0] = s.yl, out[1] = s.yu, out[2] = s.dms, out[3] = s.dml, out[4] = s.ap;
    out[5] = s.a[0], out[6] = s.a[1];
#pragma unroll
    for (int k = 0; k < 6; ++k) out[7 + k] = s.b[k], out[15 + k] = s.dq[k];
    out[13] = s.pk[0], out[14] = s.pk[1], out[21] = s.sr[0], out[22] = s.sr[1], out[23] = s.td;
}

// ---- G.722 -----------------------------------------------------------------------------------------------------------------------

__constant__ int16_t kQm2[4] = {-7408, -1616, 7408, 1616};
__constant__ int16_t kQm4[16] = {0, -20456, -12896, -8968, -6288, -4240, -2584, -1200, 20456, 12896, 8968, 6288, 4240, 2584, 1200, 0};
__constant__ int16_t kQm6[64] = {
    -136, -136, -136, -136, -24808, -21904, -19008, -16704, -14984, -13512, -12280, -11192, -10232, -9360, -8576, -7856,
    -7192, -6576, -6000, -5456, -4944, -4464, -4008, -3576, -3168, -2776, -2400, -2032, -1688, -1360, -1040, -728,
    24808, 21904, 19008, 16704, 14984, 13512, 12280, 11192, 10232, 9360, 8576, 7856, 7192, 6576, 6000, 5456,
    4944, 4464, 4008, 3576, 3168, 2776, 2400, 2032, 1688, 1360, 1040, 728, 432, 136, -432, -136};
__constant__ int16_t kWl[8] = {-60, -30, 58, 172, 334, 538, 1198, 3042};
__constant__ uint8_t kRl42[16] = {0, 7, 6, 5, 4, 3, 2, 1, 7, 6, 5, 4, 3, 2, 1, 0};
__constant__ int16_t kIlb[32] = {2048, 2093, 2139, 2186, 2233, 2282, 2332, 2383, 2435, 2489, 2543, 2599, 2656, 2714, 2774, 2834,
                                 2896, 2960, 3025, 3091, 3158, 3228, 3298, 3371, 3444, 3520, 3597, 3676, 3756, 3838, 3922, 4008};
__constant__ int16_t kWh[3] = {0, -214, 798};
__constant__ uint8_t kRh2[4] = {2, 1, 2, 1};
__constant__ int16_t kQmf[12] = {3, -11, 12, 32, -210, 951, 3876, -805, 362, -156, 53, -11};

struct G722Band {  // one band of sk_g722_state: 22 words
    int s, sz, r[2], p[2], a[2], b[6], d[6], nb, det;
};

__device__ __forceinline__ int sat16(int v) { return clamp_i(v, -32768, 32767); }

__device__ __forceinline__ void band_load(G722Band &b, const int32_t *w) {
    b.s = w[0], b.sz = w[1], b.r[0] = w[2], b.r[1] = w[3], b.p[0] = w[4], b.p[1] = w[5], b.a[0] = w[6], b.a[1] = w[7];
#pragma unroll
    for (int k = 0; k < 6; ++k) b.b[k] = w[8 + k], b.d[k] = w[14 + k];
    b.nb = w[20], b.det = w[21];
}
__device__ __forceinline__ void band_store(const G722Band &b, int32_t *w) {
    w[0] = b.s, w[1] = b.sz, w[2] = b.r[0], w[3] = b.r[1], w[4] = b.p[0], w[5] = b.p[1], w[6] = b.a[0], w[7] = b.a[1];
#pragma unroll
    for (int k = 0; k < 6; ++k) w[8 + k] = b.b[k], w[14 + k] = b.d[k];
    w[20] = b.nb, w[21] = b.det;
}

__device__ __forceinline__ int g722_scale(int nb, int k) {
    const int w = k - (nb >> 11), v = kIlb[(nb >> 6) & 31];
    return w < 0 ? v << -w : v >> w;
}

// the standard's block 4: RECONS, PARREC, UPPOL2, UPPOL1, UPZERO, DELAYA, FILTEP, FILTEZ, PREDIC
__device__ void g722_block4(G722Band &b, int d) {
    const int r0 = sat16(b.s + d), p0 = sat16(b.sz + d);
    const bool same0 = (p0 < 0) == (b.p[0] < 0), same1 = (p0 < 0) == (b.p[1] < 0);
    int wd1 = sat16(b.a[0] * 4);
    int wd2 = same0 ? -wd1 : wd1;
    if (wd2 > 32767) wd2 = 32767;
    const int a2 = clamp_i((same1 ? 128 : -128) + (wd2 >> 7) + ((b.a[1] * 32512) >> 15), -12288, 12288);
    int a1 = sat16((same0 ? 192 : -192) + ((b.a[0] * 32640) >> 15));
    const int lim = sat16(15360 - a2);
    a1 = clamp_i(a1, -lim, lim);
    const int step = d == 0 ? 0 : 128;
#pragma unroll
    for (int k = 0; k < 6; ++k) b.b[k] = sat16((((b.d[k] < 0) == (d < 0)) ? step : -step) + ((b.b[k] * 32640) >> 15));
#pragma unroll
    for (int k = 5; k > 0; --k) b.d[k] = b.d[k - 1];
    b.d[0] = d;
    b.r[1] = b.r[0], b.r[0] = r0;
    b.p[1] = b.p[0], b.p[0] = p0;
    b.a[0] = a1, b.a[1] = a2;
    const int sp = sat16(((a1 * sat16(2 * b.r[0])) >> 15) + ((a2 * sat16(2 * b.r[1])) >> 15));
    int sz = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) sz += (b.b[k] * sat16(2 * b.d[k])) >> 15;
    b.sz = sat16(sz);
    b.s = sat16(sp + b.sz);
}

// one byte through both bands: (uint16_t)rlow | rhigh << 16
__device__ __forceinline__ uint32_t g722_bands(G722Band &lo, G722Band &hi, uint32_t code) {
    const uint32_t ilow = code & 63, ihigh = (code >> 6) & 3;
    const int rlow = clamp_i(lo.s + ((lo.det * kQm6[ilow]) >> 15), -16384, 16383);
    const int dlowt = (lo.det * kQm4[ilow >> 2]) >> 15;
    lo.nb = clamp_i(((lo.nb * 127) >> 7) + kWl[kRl42[ilow >> 2]], 0, 18432);
    lo.det = g722_scale(lo.nb, 8) << 2;
    g722_block4(lo, dlowt);
    const int dhigh = (hi.det * kQm2[ihigh]) >> 15;
    const int rhigh = clamp_i(dhigh + hi.s, -16384, 16383);
    hi.nb = clamp_i(((hi.nb * 127) >> 7) + kWh[kRh2[ihigh]], 0, 22528);
    hi.det = g722_scale(hi.nb, 10) << 2;
    g722_block4(hi, dhigh);
    return ((uint32_t)rlow & 0xffff) | ((uint32_t)rhigh << 16);
}

__global__ __launch_bounds__(64) void k_g722_adpcm(const G72xStream *streams, uint32_t n_streams, const G72xUnit *units, const int32_t *states_in,
                                                   int32_t *states_out, uint32_t *ws) {
    const uint32_t idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= n_streams) return;
    const G72xStream st = streams[idx];
    const int32_t *in = states_in + (size_t)st.state * kG722StateWords;
    int32_t *out = states_out + (size_t)st.state * kG722StateWords;
    G722Band lo, hi;
    band_load(lo, in);
    band_load(hi, in + 22);
    uint32_t *w = ws + st.ws_offset;
    uint32_t n = 0;
    for (uint32_t u = 0; u < st.n_units; ++u) {
        const G72xUnit unit = units[st.first_unit + u];
        const uint32_t len = unit.bytes;
        const uint32_t *src = reinterpret_cast<const uint32_t *>(unit.src);
        uint32_t next = len ? src[0] : 0;
        for (uint32_t p = 0; p < len; p += 4) {  // the dword that holds the unit's last byte is the last one read
            const uint32_t word = next;
            if (p + 4 < len) next = src[(p >> 2) + 1];
            const uint32_t m = len - p < 4 ? len - p : 4;
            for (uint32_t k = 0; k < m; ++k) w[n + p + k] = g722_bands(lo, hi, (word >> (8 * k)) & 0xff);
        }
        n += len;
    }
    band_store(lo, out);
    band_store(hi, out + 22);
    // a call of fewer than 11 bytes keeps the younger part of the old carry; k_g722_qmf writes the pairs behind it
    for (uint32_t k = 0; 2 * n + k < 22; ++k) out[44 + k] = in[44 + 2 * n + k];
}

// pair j of a stream as (rlow + rhigh, rlow - rhigh): from the workspace, or for j < 0 from the carry
__device__ __forceinline__ void qmf_pair(const uint32_t *w, const int32_t *carry, int j, int &sum, int &diff) {
    if (j < 0) {
        sum = carry[22 + 2 * j], diff = carry[23 + 2 * j];
    } else {
        const uint32_t v = w[j];
        const int rlow = (int16_t)(v & 0xffff), rhigh = (int16_t)(v >> 16);
        sum = rlow + rhigh, diff = rlow - rhigh;
    }
}

__global__ __launch_bounds__(256) void k_g722_qmf(const G72xStream *streams, uint32_t n_streams, const G72xUnit *units, const int32_t *states_in,
                                                  int32_t *states_out, const uint32_t *ws) {
    const uint32_t idx = blockIdx.y;
    if (idx >= n_streams) return;
    const G72xStream st = streams[idx];
    const uint32_t n = st.total_bytes;
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int32_t *carry = states_in + (size_t)st.state * kG722StateWords + 44;
    const uint32_t *w = ws + st.ws_offset;
    int x1 = 0, x2 = 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        int sum, diff;
        qmf_pair(w, carry, (int)j - 11 + i, sum, diff);
        x2 += sum * kQmf[i];
        x1 += diff * kQmf[11 - i];
    }
    // which unit pair j lies in
    uint32_t u = 0, at = j;
    G72xUnit unit = units[st.first_unit];
    while (at >= unit.bytes) at -= unit.bytes, unit = units[st.first_unit + ++u];
    reinterpret_cast<uint32_t *>(unit.dst)[at] = ((uint32_t)sat16(x1 >> 11) & 0xffff) | ((uint32_t)sat16(x2 >> 11) << 16);
    if (j + 11 >= n) {  // one of the call's last 11 pairs: slot 11 - (n - j) of the new carry
        int sum, diff;
        qmf_pair(w, carry, (int)j, sum, diff);
        int32_t *out = states_out + (size_t)st.state * kG722StateWords + 44 + 2 * (11 - (n - j));
        out[0] = sum, out[1] = diff;
    }
}

}  // namespace

hipError_t launch_g726(const G72xStream *streams, uint32_t n_streams, const G72xUnit *units, const int32_t *states_in, int32_t *states_out, hipStream_t s) {
    if (n_streams == 0) return hipSuccess;
    hipLaunchKernelGGL(k_g726, dim3((n_streams + 63) / 64), dim3(64), 0, s, streams, n_streams, units, states_in, states_out);
    return hipGetLastError();
}

hipError_t launch_g722(const G72xStream *streams, uint32_t n_streams, const G72xUnit *units, const int32_t *states_in, int32_t *states_out, uint32_t *ws,
                       uint32_t max_bytes, hipStream_t s) {
    if (n_streams == 0) return hipSuccess;
    hipLaunchKernelGGL(k_g722_adpcm, dim3((n_streams + 63) / 64), dim3(64), 0, s, streams, n_streams, units, states_in, states_out, ws);
    if (max_bytes == 0) return hipGetLastError();
    for (uint32_t s0 = 0; s0 < n_streams; s0 += 65535) {
        const uint32_t n = n_streams - s0 < 65535 ? n_streams - s0 : 65535;
        hipLaunchKernelGGL(k_g722_qmf, dim3((max_bytes + 255) / 256, n), dim3(256), 0, s, streams + s0, n, units, states_in, states_out, ws);
    }
    return hipGetLastError();
}

}  // namespace sk

// alac_decode.hip -- the Apple Lossless decode stage for gfx950 (sk_alac_decode_packets, sk_alac_packet_decoder_*; engine.cpp): packets as
// a container cut them in, interleaved little-endian PCM out.  Integer arithmetic only, all of it 32-bit two's-complement wrapping (done
// in uint32_t, so nothing is undefined).  flac_decode.hip's structure: three launches over every packet of a call.
//
//   k_alac_entropy  one packet per lane, the packets handed out longest first.  The lane walks the elements (SCE / CPE / LFE decoded,
//                   DSE / FIL stepped over by their length fields, CCE / PCE rejected, END), reads each element's header and per channel
//                   prediction type, quantiser shift, pb_factor, order and coefficients into a record, steps over the extra-bit fields
//                   (their bit position goes into the record) and reads the adaptive-Golomb residuals -- history, zero runs, sign
//                   modifier, escapes -- into the packet's planar i32 workspace.  An uncompressed element's samples go there directly.
//                   Bits past the packet's last byte read as zero and mark the packet invalid; every loop is bounded by the bits the
//                   packet has left or by the frame count the host read (alac_stream.h), which every element must repeat.
//   k_alac_predict  one channel of one packet per lane (the host lists them: packet << 3 | channel): prediction type 15's first-order sum, out[0] = e[0], the first-order warm-up,
//                   then val = (sum (out[i-order+j] - d) * c[j] + half) >> shift, out[i] = sx(val + d + e[i]) and the sign walk that
//                   adapts c[] -- in place.  Window and coefficients live in registers, in four sizes (4, 8, 16, 32) chosen by order.
//                   The coefficients adapt as 32-bit values: a 16-bit one that adaptation carries past 32767 does not wrap.
//   k_alac_output   one block per packet, a lane per sample frame: pair unmix (a -= (b * weight) >> shift; b += a; out = b, a), the
//                   extra fields read in parallel from the recorded bit position, interleave in bitstream channel order, and the
//                   cookie's width (2, 3 or 4 bytes).
//
// A packet whose status is not SK_OK writes nothing: the later stages step over it.
#include <hip/hip_runtime.h>

#include "sk_device.h"

namespace sk {

namespace {

constexpr int32_t kInvalid = -601;      // SK_ALAC_INVALID
constexpr int32_t kElement = -603;      // SK_ALAC_UNSUPPORTED
constexpr int32_t kUnsupported = -6;    // SK_ERR_UNSUPPORTED

struct Bits {
    const uint8_t *base;  // 4-byte aligned
    uint32_t len;         // of the whole buffer
    uint32_t start;       // byte offset of the packet
    uint32_t pos, end;    // bits from the packet's start
    bool over;

    __device__ __forceinline__ uint32_t word(uint32_t w) const {  // big-endian word at byte w (a multiple of 4), zeros past the buffer
        if (w + 4 <= len) return __builtin_bswap32(*reinterpret_cast<const uint32_t *>(base + w));
        uint32_t v = 0;
        for (uint32_t i = 0; i < 4; ++i) v = (v << 8) | (w + i < len ? base[w + i] : 0u);
        return v;
    }
    __device__ __forceinline__ uint32_t peek32() const {  // the next 32 bits, zeros from the packet's end on
        if (pos >= end) return 0u;
        const uint32_t a = start + (pos >> 3), w = a & ~3u, off = ((a & 3u) << 3) | (pos & 7u);
        const uint64_t both = ((uint64_t)word(w) << 32) | word(w + 4);
        uint32_t v = (uint32_t)(both >> (32 - off));
        const uint32_t avail = end - pos;
        if (avail < 32) v &= ~(0xffffffffu >> avail);
        return v;
    }
    __device__ __forceinline__ void skip(uint32_t n) {
        pos += n;
        over |= pos > end;
    }
    __device__ __forceinline__ uint32_t read(uint32_t n) {  // 0 ... 32 bits
        const uint32_t v = n ? peek32() >> (32 - n) : 0u;
        skip(n);
        return v;
    }
    __device__ __forceinline__ int32_t read_signed(uint32_t n) {  // 1 ... 32 bits
        const int32_t v = (int32_t)peek32() >> (32 - n);
        skip(n);
        return v;
    }
    // up to nine one bits; nine of them: `escape` raw bits.  Otherwise count * (2^k - 1) plus what the next k bits add (k = 1: the count)
    __device__ __forceinline__ uint32_t scalar(uint32_t k, uint32_t escape) {
        const uint32_t v = peek32();
        const uint32_t ones = v == 0xffffffffu ? 32u : (uint32_t)__builtin_clz(~v);
        if (ones >= 9) {
            skip(9);
            return read(escape);
        }
        skip(ones + 1);
        if (k == 1) return ones;
        uint32_t x = ones * ((1u << k) - 1u);
        const uint32_t e = peek32() >> (32 - k);
        if (e > 1) x += e - 1, skip(k);
        else skip(k - 1);
        return x;
    }
};

__device__ __forceinline__ uint32_t floor_log2(uint32_t v) { return v ? 31u - (uint32_t)__builtin_clz(v) : 0u; }

__device__ __forceinline__ int32_t sx(uint32_t v, uint32_t bps) {
    const uint32_t sh = 32u - bps;
    return (int32_t)(v << sh) >> sh;
}

// the residuals of one channel; false: the packet is invalid
__device__ bool read_residuals(Bits &b, const AlacParams &p, int32_t *__restrict__ dst, uint32_t n, uint32_t bps, uint32_t pb_factor) {
    const uint32_t m = pb_factor * p.pb / 4u, kb = p.kb;
    uint32_t history = p.mb, modifier = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t k = min(floor_log2((history >> 9) + 3u), kb);
        const uint32_t x = b.scalar(k, bps) + modifier;
        modifier = 0;
        dst[i] = (int32_t)((x >> 1) ^ (0u - (x & 1u)));
        history = x > 0xffffu ? 0xffffu : history + x * m - ((history * m) >> 9);
        if (history < 128u && i + 1 < n) {
            k = min(7u - floor_log2(history) + ((history + 16u) >> 6), kb);
            const uint32_t run = b.scalar(k, 16);
            if (run >= n - i) return false;  // the run reaches the element's end
            for (uint32_t r = 0; r < run; ++r) dst[i + 1 + r] = 0;
            i += run;
            if (run <= 0xffffu) modifier = 1;
            history = 0;
        }
        if (b.over) return false;
    }
    return true;
}

__global__ void __launch_bounds__(64) k_alac_entropy(const AlacParams *__restrict__ cfgs, const AlacPacket *__restrict__ packets, const uint32_t *__restrict__ by_length,
                                                    uint32_t n_packets, const uint8_t *__restrict__ bytes, uint32_t bytes_len, int32_t *__restrict__ ws,
                                                    AlacChannel *__restrict__ recs, int32_t *__restrict__ status) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_packets) return;
    const uint32_t pi = by_length[t];
    const AlacPacket pk = packets[pi];
    const AlacParams p = cfgs[pk.cfg];
    Bits b{bytes, bytes_len, pk.byte_offset, 0u, pk.byte_len * 8u, false};
    const uint32_t depth = p.bit_depth, want = p.channels, frames = pk.frames;
    int32_t st = p.kb == 0 ? kInvalid : 0;
    uint32_t done = 0;  // channels so far
    while (st == 0) {
        const uint32_t tag = b.read(3);
        if (b.over) {  // no END
            st = kInvalid;
            break;
        }
        if (tag == 7) break;
        if (tag == 2 || tag == 5) {
            st = kElement;
            break;
        }
        if (tag == 4) {  // DSE: instance tag, align flag, count (255: one more byte of it), the bytes
            b.skip(4);
            const uint32_t align = b.read(1);
            uint32_t count = b.read(8);
            if (count == 255) count += b.read(8);
            if (align) b.skip((8u - (b.pos & 7u)) & 7u);
            b.skip(8u * count);
            continue;
        }
        if (tag == 6) {  // FIL
            uint32_t count = b.read(4);
            if (count == 15) count += b.read(8) - 1u;
            b.skip(8u * count);
            continue;
        }
        const uint32_t el_ch = tag == 1 ? 2u : 1u;
        if (done + el_ch > want) {
            st = kInvalid;
            break;
        }
        b.skip(16);  // instance tag, 12 unused bits
        const uint32_t has_size = b.read(1), extra = 8u * b.read(2), raw = b.read(1);
        const uint32_t n = has_size ? b.read(32) : p.frame_length;
        if (b.over || n != frames) {  // frames is 1 ... frame_length: the host refused everything else
            st = kInvalid;
            break;
        }
        if (depth + el_ch - 1u > 32u + extra) {
            st = kUnsupported;
            break;
        }
        if (depth + el_ch - 1u <= extra) {
            st = kInvalid;
            break;
        }
        const uint32_t bps = depth - extra + el_ch - 1u;
        AlacChannel *rec = recs + pk.rec0 + done;
        int32_t *dst = ws + pk.ws_offset + (size_t)done * frames;
        if (raw) {
            for (uint32_t c = 0; c < el_ch; ++c) {
                AlacChannel &r = rec[c];
                r.extra_pos = 0, r.bps = (uint8_t)depth, r.order = 0, r.shift = 0, r.ptype = 0, r.mix_shift = 0, r.mix_weight = 0, r.extra_bits = 0;
                r.role = (uint8_t)(el_ch == 2 ? c + 1 : 0), r.raw = 1;
            }
            for (uint32_t i = 0; i < n && !b.over; ++i)
                for (uint32_t c = 0; c < el_ch; ++c) dst[(size_t)c * frames + i] = b.read_signed(depth);
            if (b.over) st = kInvalid;
            done += el_ch;
            continue;
        }
        const uint32_t mix_shift = b.read(8), mix_weight = b.read(8);
        uint32_t pb_factor[2] = {0, 0};
        for (uint32_t c = 0; c < el_ch; ++c) {
            AlacChannel &r = rec[c];
            const uint32_t ptype = b.read(4), shift = b.read(4);
            pb_factor[c] = b.read(3);
            const uint32_t order = b.read(5);
            for (uint32_t j = order; j-- > 0;) r.coef[j] = (int16_t)b.read_signed(16);  // the last one read is coef[0]
            if (ptype != 0 && ptype != 15) st = kInvalid;
            r.bps = (uint8_t)bps, r.order = (uint8_t)order, r.shift = (uint8_t)shift, r.ptype = (uint8_t)ptype;
            r.mix_shift = (uint8_t)mix_shift, r.mix_weight = (uint8_t)mix_weight, r.extra_bits = (uint8_t)extra;
            r.role = (uint8_t)(el_ch == 2 ? c + 1 : 0), r.raw = 0;
        }
        const uint32_t extra_pos = b.pos;
        rec[0].extra_pos = extra_pos;
        if (el_ch == 2) rec[1].extra_pos = extra_pos;
        b.skip(n * el_ch * extra);  // at most 65536 * 2 * 24 bits
        if (b.over) st = kInvalid;
        for (uint32_t c = 0; c < el_ch && st == 0; ++c)
            if (!read_residuals(b, p, dst + (size_t)c * frames, n, bps, pb_factor[c])) st = kInvalid;
        done += el_ch;
    }
    if (st == 0 && (b.over || b.end - b.pos >= 8u || done != want)) st = kInvalid;  // fewer than 8 padding bits may follow END
    status[pi] = st;
}

template <int MAXO>
__device__ __forceinline__ void predict_regs(int32_t *__restrict__ s, const int16_t *__restrict__ coef, uint32_t n, uint32_t order, uint32_t shift,
                                             uint32_t bps) {
    // p[j] = out[i - order + j], d = out[i - order - 1]; the slots from `order` on stay zero and take no part
    uint32_t p[MAXO], c[MAXO];
#pragma unroll
    for (int j = 0; j < MAXO; ++j) {
        const bool in = (uint32_t)j < order;
        p[j] = in ? (uint32_t)s[1 + j] : 0u;
        c[j] = in ? (uint32_t)(int32_t)coef[j] : 0u;
    }
    uint32_t d = (uint32_t)s[0];
    const uint32_t half = shift ? 1u << (shift - 1) : 0u;
    for (uint32_t i = order + 1; i < n; ++i) {
        uint32_t sum = 0;
#pragma unroll
        for (int j = 0; j < MAXO; ++j) sum += (p[j] - d) * c[j];  // c[j] = 0 from `order` on
        const int32_t val = (int32_t)(sum + half) >> shift;
        const int32_t e = s[i];
        const int32_t v = sx((uint32_t)val + d + (uint32_t)e, bps);
        s[i] = v;
        if (e != 0) {
            const int32_t sign_e = e > 0 ? 1 : -1;
            uint32_t err = (uint32_t)e;
#pragma unroll
            for (int j = 0; j < MAXO; ++j) {
                // the walk ends at the first j whose remaining error has lost e's sign; err no longer changes then, so the test stays false
                if ((uint32_t)j < order && (int32_t)(err * (uint32_t)sign_e) > 0) {
                    const int32_t diff = (int32_t)(d - p[j]);
                    const int32_t sg = (diff > 0 ? 1 : diff < 0 ? -1 : 0) * sign_e;
                    c[j] -= (uint32_t)sg;
                    err -= (uint32_t)((int32_t)((uint32_t)diff * (uint32_t)sg) >> shift) * (uint32_t)(j + 1);
                }
            }
        }
        d = p[0];
#pragma unroll
        for (int j = 0; j < MAXO; ++j) {  // ascending: p[j + 1] is still the old one
            const uint32_t next = j + 1 < MAXO ? p[j + 1 < MAXO ? j + 1 : j] : 0u;
            p[j] = (uint32_t)(j + 1) < order ? next : ((uint32_t)(j + 1) == order ? (uint32_t)v : 0u);
        }
    }
}

__device__ __forceinline__ void first_order_sum(int32_t *__restrict__ s, uint32_t n, uint32_t bps) {
    uint32_t prev = (uint32_t)s[0];
    for (uint32_t i = 1; i < n; ++i) {
        prev = (uint32_t)sx(prev + (uint32_t)s[i], bps);
        s[i] = (int32_t)prev;
    }
}

__global__ void __launch_bounds__(64) k_alac_predict(const AlacPacket *__restrict__ packets, const uint32_t *__restrict__ lanes, uint32_t n_lanes,
                                                    const AlacChannel *__restrict__ recs, int32_t *__restrict__ ws, const int32_t *__restrict__ status) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_lanes) return;
    const uint32_t pi = lanes[t] >> 3, ch = lanes[t] & 7u;
    if (status[pi] != 0) return;  // a record is complete only when its packet was accepted
    const AlacPacket pk = packets[pi];
    const AlacChannel *rec = recs + pk.rec0 + ch;
    if (rec->raw) return;
    const uint32_t n = pk.frames, order = rec->order, shift = rec->shift, bps = rec->bps;
    int32_t *s = ws + pk.ws_offset + (size_t)ch * n;
    if (rec->ptype == 15) first_order_sum(s, n, bps);
    if (order == 0 || n <= 1) return;
    if (order == 31) {
        first_order_sum(s, n, bps);
        return;
    }
    {  // the warm-up: samples 1 ... order are first-order sums
        uint32_t prev = (uint32_t)s[0];
        const uint32_t stop = min(order, n - 1);
        for (uint32_t i = 1; i <= stop; ++i) {
            prev = (uint32_t)sx(prev + (uint32_t)s[i], bps);
            s[i] = (int32_t)prev;
        }
    }
    if (n <= order + 1) return;
    if (order <= 4) predict_regs<4>(s, rec->coef, n, order, shift, bps);
    else if (order <= 8) predict_regs<8>(s, rec->coef, n, order, shift, bps);
    else if (order <= 16) predict_regs<16>(s, rec->coef, n, order, shift, bps);
    else predict_regs<32>(s, rec->coef, n, order, shift, bps);
}

__device__ __forceinline__ void put_sample(uint8_t *p, int32_t v, uint32_t width, bool aligned) {
    if (width == 2 && aligned) *reinterpret_cast<uint16_t *>(p) = (uint16_t)v;
    else if (width == 4 && aligned) *reinterpret_cast<uint32_t *>(p) = (uint32_t)v;
    else
        for (uint32_t k = 0; k < width; ++k) p[k] = (uint8_t)((uint32_t)v >> (8 * k));
}

// `bits` (8, 16 or 24) bits at bit position q of the packet; zeros past its end
__device__ __forceinline__ uint32_t extra_field(const uint8_t *__restrict__ packet, uint32_t byte_len, uint32_t q, uint32_t bits) {
    const uint32_t at = q >> 3;
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; ++k) v = (v << 8) | (at + k < byte_len ? packet[at + k] : 0u);
    return (v >> (32 - (q & 7u) - bits)) & ((1u << bits) - 1u);
}

__global__ void __launch_bounds__(256) k_alac_output(const AlacParams *__restrict__ cfgs, const AlacPacket *__restrict__ packets, const AlacChannel *__restrict__ recs,
                                                    const int32_t *__restrict__ ws, const int32_t *__restrict__ status,
                                                    const uint8_t *__restrict__ bytes, uint8_t *__restrict__ out) {
    const uint32_t pi = blockIdx.x;
    if (status[pi] != 0) return;
    const AlacPacket pk = packets[pi];
    const AlacParams p = cfgs[pk.cfg];
    const uint32_t ch_n = p.channels, n = pk.frames, width = p.bit_depth / 8u;
    uint8_t *dst = out + pk.out_offset;
    const bool aligned = (((uintptr_t)dst) & (width - 1)) == 0;  // width 3 never takes the typed stores
    const uint8_t *packet = bytes + pk.byte_offset;
    const AlacChannel *rec = recs + pk.rec0;
    for (uint32_t c = 0; c < ch_n;) {
        const AlacChannel r = rec[c];
        const uint32_t el_ch = r.role == 1 ? 2u : 1u, extra = r.extra_bits;
        const int32_t *s0 = ws + pk.ws_offset + (size_t)c * n, *s1 = s0 + n;
        const uint32_t mix_shift = min((uint32_t)r.mix_shift, 31u), weight = r.mix_weight;
        for (uint32_t i = threadIdx.x; i < n; i += 256) {
            uint32_t v0 = (uint32_t)s0[i], v1 = 0;
            if (el_ch == 2) {
                v1 = (uint32_t)s1[i];
                if (weight) {
                    const uint32_t a = v0 - (uint32_t)((int32_t)(v1 * weight) >> mix_shift), b = v1 + a;
                    v0 = b, v1 = a;
                }
            }
            if (extra) {
                const uint32_t q = r.extra_pos + i * el_ch * extra;
                v0 = (v0 << extra) | extra_field(packet, pk.byte_len, q, extra);
                if (el_ch == 2) v1 = (v1 << extra) | extra_field(packet, pk.byte_len, q + extra, extra);
            }
            uint8_t *at = dst + ((size_t)i * ch_n + c) * width;
            put_sample(at, (int32_t)v0, width, aligned);
            if (el_ch == 2) put_sample(at + width, (int32_t)v1, width, aligned);
        }
        c += el_ch;
    }
}

}  // namespace

hipError_t launch_alac_entropy(const AlacParams *cfgs, const AlacPacket *packets, const uint32_t *by_length, uint32_t n_packets, const uint8_t *bytes,
                               uint32_t bytes_len, int32_t *ws, AlacChannel *recs, int32_t *status, hipStream_t s) {
    if (n_packets == 0) return hipSuccess;
    hipLaunchKernelGGL(k_alac_entropy, dim3((n_packets + 63) / 64), dim3(64), 0, s, cfgs, packets, by_length, n_packets, bytes, bytes_len, ws, recs,
                       status);
    return hipGetLastError();
}

hipError_t launch_alac_predict(const AlacPacket *packets, const uint32_t *lanes, uint32_t n_lanes, const AlacChannel *recs, int32_t *ws,
                               const int32_t *status, hipStream_t s) {
    if (n_lanes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_alac_predict, dim3((n_lanes + 63) / 64), dim3(64), 0, s, packets, lanes, n_lanes, recs, ws, status);
    return hipGetLastError();
}

hipError_t launch_alac_output(const AlacParams *cfgs, const AlacPacket *packets, uint32_t n_packets, const AlacChannel *recs, const int32_t *ws,
                              const int32_t *status, const uint8_t *bytes, uint8_t *out, hipStream_t s) {
    if (n_packets == 0) return hipSuccess;
    hipLaunchKernelGGL(k_alac_output, dim3(n_packets), dim3(256), 0, s, cfgs, packets, recs, ws, status, bytes, out);
    return hipGetLastError();
}

}  // namespace sk

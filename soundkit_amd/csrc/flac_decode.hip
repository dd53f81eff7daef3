// flac_decode.hip -- the FLAC streams' decode stage for gfx950 (sk_flac_decode_frames, sk_flac_decoder_*; engine.cpp): whole frames as
// the framer cut them (flac_stream.h) in, interleaved little-endian PCM out.  Integer arithmetic only.  Three launches over every
// frame of a call:
//
//   k_flac_residual  one frame per lane, the frames handed out longest first.  The subframes of a frame are serial in position, so the
//                    lane walks them channel after channel: zero bit, type, wasted bits, warm-up samples, LPC precision / shift /
//                    coefficients, then the Rice partitions (4- or 5-bit parameters, escape partitions with their raw width) --
//                    un-zigzagged into the frame's planar i32 workspace, warm-up samples in front of the residuals they predict.
//                    Bits past the frame's last byte before the CRC-16 read as zero and EVERY loop is bounded by the bits the frame
//                    has left: a damaged unary run ends the frame with a status.  One record per subframe tells the later stages
//                    what to do (a FIXED predictor becomes its coefficients, so the restore has one form).
//   k_flac_restore   one subframe per lane: s[i] = r[i] + (sum coef[j] * s[i-1-j] >> shift) in place, the sum in 64 bits (depth +
//                    precision + log2(order) exceeds 32 bits from 16-bit material on; there is no 32-bit path).  Orders 1 ... 12 keep
//                    history and coefficients in registers; 13 ... 32 keep the coefficients there and read the history back.
//   k_flac_output    one block per frame, a lane per sample frame: wasted-bits shift, left/side, side/right, mid/side (the low bit of
//                    mid comes back from side), interleave, and the contract's width -- <= 8 bits: one byte, sample + 128; <= 16: two;
//                    <= 24: three; else four -- or, for the FlacDecoder, i32 or i16 clamped.
//
// A frame whose status is not SK_OK writes nothing: the later stages step over it.
#include <hip/hip_runtime.h>

#include "sk_device.h"

namespace sk {

namespace {

constexpr int32_t kInvalid = -506;      // SK_FLAC_INVALID
constexpr int32_t kUnsupported = -6;    // SK_ERR_UNSUPPORTED

struct Bits {
    const uint8_t *base;  // 4-byte aligned
    uint32_t len;         // of the whole buffer
    uint32_t start;       // byte offset of the frame
    uint32_t pos, end;    // bits from the frame's start; end = where the CRC-16 begins
    bool over;

    __device__ __forceinline__ uint32_t word(uint32_t w) const {  // big-endian word at byte w (a multiple of 4), zeros past the buffer
        if (w + 4 <= len) return __builtin_bswap32(*reinterpret_cast<const uint32_t *>(base + w));
        uint32_t v = 0;
        for (uint32_t i = 0; i < 4; ++i) v = (v << 8) | (w + i < len ? base[w + i] : 0u);
        return v;
    }
    __device__ __forceinline__ uint32_t peek32() const {
        const uint32_t a = start + (pos >> 3), w = a & ~3u, off = ((a & 3u) << 3) | (pos & 7u);
        const uint64_t both = ((uint64_t)word(w) << 32) | word(w + 4);
        uint32_t v = (uint32_t)(both >> (32 - off));
        const uint32_t avail = end > pos ? end - pos : 0;
        if (avail < 32) v = avail ? v & ~(0xffffffffu >> avail) : 0u;
        return v;
    }
    __device__ __forceinline__ uint32_t read(uint32_t n) {  // 0 ... 32 bits
        const uint32_t v = n ? peek32() >> (32 - n) : 0u;
        pos += n;
        over |= pos > end;
        return v;
    }
    __device__ __forceinline__ int32_t read_signed(uint32_t n) {
        if (n == 0) return 0;
        const int32_t v = (int32_t)peek32() >> (32 - n);
        pos += n;
        over |= pos > end;
        return v;
    }
    __device__ __forceinline__ uint32_t unary() {  // zeros in front of the next one bit
        uint32_t count = 0;
        for (;;) {
            const uint32_t v = peek32();
            if (v) {
                const uint32_t z = (uint32_t)__builtin_clz(v);
                pos += z + 1;
                return count + z;
            }
            count += 32, pos += 32;
            if (pos >= end) {  // the run leaves the frame
                over = true;
                return count;
            }
        }
    }
};

__global__ void __launch_bounds__(64) k_flac_residual(const FlacFrame *__restrict__ frames, const uint32_t *__restrict__ by_length, uint32_t n_frames,
                                                     const uint8_t *__restrict__ bytes, uint32_t bytes_len, int32_t *__restrict__ ws,
                                                     FlacSubframe *__restrict__ subs, int32_t *__restrict__ status) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_frames) return;
    const uint32_t fi = by_length[t];
    const FlacFrame f = frames[fi];
    int32_t st = 0;
    if (f.assignment >= 8 && f.channels != 2) st = kInvalid;
    else if (f.assignment > 10) st = kInvalid;
    else if (f.assignment >= 8 && f.bits >= 32) st = kUnsupported;
    Bits b{bytes, bytes_len, f.byte_offset, (uint32_t)f.header_bytes * 8u, (f.byte_len - 2u) * 8u, false};
    const uint32_t block = f.block_size;
    for (uint32_t ch = 0; ch < f.channels && st == 0; ++ch) {
        int32_t *dst = ws + f.ws_offset + (size_t)ch * block;
        FlacSubframe *rec = subs + f.sub0 + ch;
        const uint32_t head = b.read(8);
        if (head & 0x80u) {  // the padding bit
            st = kInvalid;
            break;
        }
        const uint32_t type = (head >> 1) & 0x3fu;
        uint32_t wasted = 0;
        if (head & 1u) wasted = b.unary() + 1;
        const bool side = (f.assignment == 8 && ch == 1) || (f.assignment == 9 && ch == 0) || (f.assignment == 10 && ch == 1);
        uint32_t bps = (uint32_t)f.bits + (side ? 1u : 0u);
        if (b.over || wasted >= bps) {
            st = kInvalid;
            break;
        }
        bps -= wasted;
        uint32_t order = 0, kind = kFlacPredict, shift = 0;
        bool lpc = false;
        if (type == 0) kind = kFlacConstant;
        else if (type == 1) kind = kFlacVerbatim;
        else if (type >= 8 && type <= 12) order = type - 8;
        else if (type >= 32) order = type - 31, lpc = true;
        else {  // reserved
            st = kInvalid;
            break;
        }
        if (order > block) {
            st = kInvalid;
            break;
        }
        if (kind == kFlacConstant) {
            dst[0] = b.read_signed(bps);
        } else if (kind == kFlacVerbatim) {
            for (uint32_t i = 0; i < block && !b.over; ++i) dst[i] = b.read_signed(bps);
        } else {
            for (uint32_t i = 0; i < order; ++i) dst[i] = b.read_signed(bps);
            if (lpc) {
                const uint32_t pcode = b.read(4);
                const int32_t sh = b.read_signed(5);
                if (pcode == 15 || sh < 0) {
                    st = kInvalid;
                    break;
                }
                shift = (uint32_t)sh;
                for (uint32_t j = 0; j < order; ++j) rec->coef[j] = (int16_t)b.read_signed(pcode + 1);
            } else {
                const int16_t c1[4] = {1, 2, 3, 4}, c2[4] = {0, -1, -3, -6}, c3[4] = {0, 0, 1, 4};
                if (order >= 1) rec->coef[0] = c1[order - 1];
                if (order >= 2) rec->coef[1] = c2[order - 1];
                if (order >= 3) rec->coef[2] = c3[order - 1];
                if (order >= 4) rec->coef[3] = -1;
            }
            const uint32_t method = b.read(2), porder = b.read(4);
            const uint32_t per = block >> porder;
            if (method > 1 || b.over || (block & ((1u << porder) - 1u)) || per < order) {
                st = kInvalid;
                break;
            }
            const uint32_t pbits = method ? 5u : 4u, escape = method ? 31u : 15u;
            uint32_t i = order;
            for (uint32_t p = 0; p < (1u << porder) && !b.over; ++p) {
                const uint32_t k = b.read(pbits), stop = (p + 1) * per;
                if (k == escape) {
                    const uint32_t width = b.read(5);
                    for (; i < stop && !b.over; ++i) dst[i] = b.read_signed(width);
                } else {
                    for (; i < stop && !b.over; ++i) {
                        const uint32_t q = b.unary();
                        const uint32_t u = (q << k) | b.read(k);
                        dst[i] = (int32_t)((u >> 1) ^ (0u - (u & 1u)));
                    }
                }
            }
        }
        if (b.over) {
            st = kInvalid;
            break;
        }
        rec->kind = (uint8_t)kind, rec->order = (uint8_t)order, rec->shift = (uint8_t)shift, rec->wasted = (uint8_t)wasted;
        rec->ws_offset = f.ws_offset + ch * block, rec->block_size = block, rec->frame = fi;
    }
    if (st == 0) {  // the samples end in the byte in front of the CRC-16, the padding bits are zero
        if (b.over || b.pos > b.end || b.end - b.pos > 7) st = kInvalid;
        else if (b.end > b.pos && b.read(b.end - b.pos) != 0) st = kInvalid;
    }
    status[fi] = st;
}

template <int ORDER>
__device__ __forceinline__ void restore_regs(int32_t *__restrict__ s, const int16_t *__restrict__ coef, uint32_t block, uint32_t shift) {
    int32_t h[ORDER], c[ORDER];
#pragma unroll
    for (int j = 0; j < ORDER; ++j) h[j] = s[ORDER - 1 - j], c[j] = coef[j];
    for (uint32_t i = ORDER; i < block; ++i) {
        int64_t acc = 0;
#pragma unroll
        for (int j = 0; j < ORDER; ++j) acc += (int64_t)c[j] * h[j];
        const int32_t v = (int32_t)((uint32_t)s[i] + (uint32_t)(acc >> shift));
        s[i] = v;
#pragma unroll
        for (int j = ORDER - 1; j > 0; --j) h[j] = h[j - 1];
        h[0] = v;
    }
}

__global__ void __launch_bounds__(64) k_flac_restore(const FlacSubframe *__restrict__ subs, uint32_t n_subs, int32_t *__restrict__ ws,
                                                    const int32_t *__restrict__ status) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_subs) return;
    const FlacSubframe *rec = subs + t;
    // a record is complete only when its frame was accepted; the frame index of a rejected frame's record may be stale, so the
    // record's own fields are not trusted before the status says so
    const uint32_t frame = rec->frame;
    if (frame == 0xffffffffu || status[frame] != 0) return;
    if (rec->kind != kFlacPredict || rec->order == 0) return;
    int32_t *s = ws + rec->ws_offset;
    const uint32_t block = rec->block_size, shift = rec->shift;
    switch (rec->order) {
    case 1: restore_regs<1>(s, rec->coef, block, shift); break;
    case 2: restore_regs<2>(s, rec->coef, block, shift); break;
    case 3: restore_regs<3>(s, rec->coef, block, shift); break;
    case 4: restore_regs<4>(s, rec->coef, block, shift); break;
    case 5: restore_regs<5>(s, rec->coef, block, shift); break;
    case 6: restore_regs<6>(s, rec->coef, block, shift); break;
    case 7: restore_regs<7>(s, rec->coef, block, shift); break;
    case 8: restore_regs<8>(s, rec->coef, block, shift); break;
    case 9: restore_regs<9>(s, rec->coef, block, shift); break;
    case 10: restore_regs<10>(s, rec->coef, block, shift); break;
    case 11: restore_regs<11>(s, rec->coef, block, shift); break;
    case 12: restore_regs<12>(s, rec->coef, block, shift); break;
    default: {
        const int order = rec->order;  // 13 ... 32: the coefficients in registers (the loops unroll), the history read back
        int32_t c[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) c[j] = j < order ? rec->coef[j] : 0;
        for (uint32_t i = (uint32_t)order; i < block; ++i) {
            int64_t acc = 0;
#pragma unroll
            for (int j = 0; j < 32; ++j)
                if (j < order) acc += (int64_t)c[j] * s[i - 1 - j];
            s[i] = (int32_t)((uint32_t)s[i] + (uint32_t)(acc >> shift));
        }
    }
    }
}

__device__ __forceinline__ void put_sample(uint8_t *p, int32_t v, uint32_t width, bool aligned) {
    if (width == 1) p[0] = (uint8_t)v;
    else if (width == 2 && aligned) *reinterpret_cast<uint16_t *>(p) = (uint16_t)v;
    else if (width == 4 && aligned) *reinterpret_cast<uint32_t *>(p) = (uint32_t)v;
    else
        for (uint32_t k = 0; k < width; ++k) p[k] = (uint8_t)((uint32_t)v >> (8 * k));
}

__global__ void __launch_bounds__(256) k_flac_output(const FlacFrame *__restrict__ frames, const FlacSubframe *__restrict__ subs,
                                                    const int32_t *__restrict__ ws, const int32_t *__restrict__ status, uint8_t *__restrict__ out,
                                                    uint32_t mode) {
    const uint32_t fi = blockIdx.x;
    if (status[fi] != 0) return;
    const FlacFrame f = frames[fi];
    const uint32_t ch_n = f.channels, block = f.block_size;
    const uint32_t width = mode == kFlacOutI32 ? 4u : mode == kFlacOutI16Clamp ? 2u : (f.bits <= 8 ? 1u : f.bits <= 16 ? 2u : f.bits <= 24 ? 3u : 4u);
    const int32_t bias = (mode == kFlacOutContract && f.bits <= 8) ? 128 : 0;
    uint8_t *dst = out + f.out_offset;
    const bool aligned = (((uintptr_t)dst) & (width - 1)) == 0;  // width 3 never takes the typed stores
    const FlacSubframe *rec = subs + f.sub0;
    if (f.assignment >= 8) {
        const uint32_t k0 = rec[0].kind, k1 = rec[1].kind, w0 = rec[0].wasted, w1 = rec[1].wasted;
        const int32_t *s0 = ws + f.ws_offset, *s1 = s0 + block;
        for (uint32_t i = threadIdx.x; i < block; i += 256) {
            const int32_t a = (int32_t)((uint32_t)s0[k0 == kFlacConstant ? 0 : i] << w0);
            const int32_t b = (int32_t)((uint32_t)s1[k1 == kFlacConstant ? 0 : i] << w1);
            int32_t l, r;
            if (f.assignment == 8) l = a, r = a - b;         // left, side
            else if (f.assignment == 9) l = a + b, r = b;    // side, right
            else {                                           // mid, side
                const int32_t mid = (int32_t)(((uint32_t)a << 1) | ((uint32_t)b & 1u));
                l = (mid + b) >> 1, r = (mid - b) >> 1;
            }
            l += bias, r += bias;
            if (mode == kFlacOutI16Clamp) l = max(-32768, min(32767, l)), r = max(-32768, min(32767, r));
            uint8_t *p = dst + (size_t)i * 2 * width;
            put_sample(p, l, width, aligned);
            put_sample(p + width, r, width, aligned);
        }
        return;
    }
    for (uint32_t c = 0; c < ch_n; ++c) {
        const uint32_t kind = rec[c].kind, wasted = rec[c].wasted;
        const int32_t *s = ws + f.ws_offset + (size_t)c * block;
        for (uint32_t i = threadIdx.x; i < block; i += 256) {
            int32_t v = (int32_t)((uint32_t)s[kind == kFlacConstant ? 0 : i] << wasted) + bias;
            if (mode == kFlacOutI16Clamp) v = max(-32768, min(32767, v));
            put_sample(dst + ((size_t)i * ch_n + c) * width, v, width, aligned);
        }
    }
}

}  // namespace

hipError_t launch_flac_residual(const FlacFrame *frames, const uint32_t *by_length, uint32_t n_frames, const uint8_t *bytes, uint32_t bytes_len,
                                int32_t *ws, FlacSubframe *subs, int32_t *status, hipStream_t s) {
    if (n_frames == 0) return hipSuccess;
    hipLaunchKernelGGL(k_flac_residual, dim3((n_frames + 63) / 64), dim3(64), 0, s, frames, by_length, n_frames, bytes, bytes_len, ws, subs, status);
    return hipGetLastError();
}

hipError_t launch_flac_restore(const FlacSubframe *subs, uint32_t n_subs, int32_t *ws, const int32_t *status, hipStream_t s) {
    if (n_subs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_flac_restore, dim3((n_subs + 63) / 64), dim3(64), 0, s, subs, n_subs, ws, status);
    return hipGetLastError();
}

hipError_t launch_flac_output(const FlacFrame *frames, uint32_t n_frames, const FlacSubframe *subs, const int32_t *ws, const int32_t *status,
                              uint8_t *out, uint32_t mode, hipStream_t s) {
    if (n_frames == 0) return hipSuccess;
    hipLaunchKernelGGL(k_flac_output, dim3(n_frames), dim3(256), 0, s, frames, subs, ws, status, out, mode);
    return hipGetLastError();
}

}  // namespace sk

// vorbis_decode.hip -- the Vorbis I decode stage for gfx950 (sk_vorbis_decode_packets, sk_vorbis_entropy_decode; engine.cpp): audio
// packets as Ogg or a WebM demuxer cut them, PCM out.  f32 and integers only; five launches over the packets and streams of a call.  The tables a
// lane walks are its stream's blob (vorbis_blob.h), every index of which the host has checked (vorbis_stream.h).
//
//   k_vorbis_entropy   one packet per lane, the packets handed out longest first; lanes of one wave may belong to different streams.
//                      The bit reader is LSB first; a read that does not fit sets "end of packet", returns nothing and never touches a
//                      byte behind the packet's last word.  The lane reads the type bit, the mode number and a long block's two window
//                      flags.  The HOST has read the same bits (vorbis_stream.h packet_head) and decides: a packet it refuses gets no
//                      lane, and the statuses the callers see for such packets are the host's; the lane's own checks of these bits are
//                      a guard, and a disagreement is SK_ERR_INTERNAL for the call.  Then per channel floor 1: the nonzero flag,
//                      per partition the class's master book and subclass books, the Y values, and their unwrapping into final Y values
//                      and "used" flags, integers only (a final Y outside [0, range) is clamped into it).  End of packet inside a floor
//                      marks the channel unused.  Then per submap the residue: classification words through the class book, up to eight
//                      passes of VQ adds (type 0 strided, type 1 contiguous, type 2 interleaved over the submap's channels), each add
//                      an f32 addition in stream order into the packet's [channel][n / 2] workspace.  End of packet inside a residue
//                      stops the residue and keeps what has been added.  Every loop is bounded by the setup's counts or consumes bits.
//   k_vorbis_spectrum  one block per packet: inverse coupling of the residue vectors, last step first (one addition or subtraction per
//                      value), then per used channel the floor curve -- the line renderer between the used posts in closed form,
//                      y = y0 + base k + sign floor(k ady / adx), k = x - x0 -- through the inverse-dB table, times the residue.  An
//                      unused channel is zeroed.
//   k_vorbis_imdct     one block per packet-channel: t[j] = (X[2j] + i X[n/2 - 1 - 2j]) w[j]; an n/4-point radix-2 decimation-in-time
//                      FFT in LDS (16 KB at n = 8192); v[k] = T[k] w[k]; u[2k] = Re v, u[n/2 - 1 - 2k] = -Im v; y from u by the three
//                      symmetries; y[m] x window[m], the slopes chosen by the packet's flags; both halves to the workspace.
//   k_vorbis_ola       one block per packet: the right half of the stream's previous accepted packet (from the workspace, or for a
//                      stream's first packet of the call from the carried half) + the left half of this one, prev_n / 4 + n / 4 frames,
//                      interleaved; f32, or s16 as x * 32768, saturated, truncated toward zero.
//   k_vorbis_carry     one block per stream: the right half of the stream's last accepted packet into the carry buffer.
//
// Float operations, in order: VQ add: acc = acc + value.  Coupling: one of m + a, m - a.  Product: table[y] * residue.  Pre- and
// post-twiddle and butterflies: complex products as (ar br - ai bi, ar bi + ai br), then a + t, a - t.  Window: y * w.  Overlap:
// right + left.  The build has -ffp-contract=off, so none of them fuses.
#include <hip/hip_runtime.h>

#include "sk_device.h"
#include "vorbis_blob.h"

namespace sk {

namespace {

using namespace sk_vb;

constexpr int32_t kNotAudio = -801, kBadMode = -802, kShort = -803;  // SK_VORBIS_*

struct VBits {
    const uint32_t *w;  // the packet's first word
    uint32_t pos, end;  // bits
    bool eop;

    __device__ __forceinline__ uint32_t peek() const {  // pos < end; reads the word that holds pos and the one behind it
        const uint32_t i = pos >> 5, sh = pos & 31u;
        const uint32_t lo = w[i], hi = w[i + 1];
        return sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
    }
    __device__ __forceinline__ uint32_t read(uint32_t n) {  // 0 ... 32 bits
        if (n == 0) return 0u;
        if (eop || pos + n > end) {
            eop = true;
            return 0u;
        }
        const uint32_t v = peek();
        pos += n;
        return n >= 32 ? v : v & ((1u << n) - 1u);
    }
};

__device__ __forceinline__ uint32_t ilog(uint32_t x) { return x ? 32u - (uint32_t)__builtin_clz(x) : 0u; }

// one code word of book `rec` (a record's word offset) -> its entry, or -1 at the end of the packet.  At most 32 steps.
__device__ int32_t huff(const uint32_t *blob, uint32_t rec, VBits &b) {
    if (b.eop) return -1;
    if (b.pos >= b.end) {
        b.eop = true;
        return -1;
    }
    const uint32_t single = blob[rec + B_SINGLE];
    if (single) {
        b.pos += 1;
        return (int32_t)single - 1;
    }
    const uint32_t v = b.peek(), avail = b.end - b.pos, lut_bits = blob[rec + B_LUTBITS];
    uint32_t e = blob[blob[rec + B_LUT] + (v & ((1u << lut_bits) - 1u))], used;
    if (e & kLeaf) {
        used = ((e >> 24) & 31u) + 1u;
    } else {
        const uint32_t tree = blob[rec + B_TREE];
        uint32_t node = e;
        used = lut_bits;
        e = 0;
        while (used < 32u) {
            const uint32_t c = blob[tree + 2u * node + ((v >> used) & 1u)];
            ++used;
            if (c & kLeaf) {
                e = c;
                break;
            }
            node = c;
        }
        if (!(e & kLeaf)) {
            b.eop = true;
            return -1;
        }
    }
    if (used > avail) {  // the code word runs past the packet: what lay behind it was not the packet's
        b.eop = true;
        return -1;
    }
    b.pos += used;
    return (int32_t)(e & 0xffffffu);
}

__device__ __forceinline__ int32_t render_point(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t x) {
    const int32_t dy = y1 - y0, adx = x1 - x0, ady = dy < 0 ? -dy : dy;
    const int32_t off = ady * (x - x0) / adx;
    return dy < 0 ? y0 - off : y0 + off;
}

// floor 1 of one channel: the Y values go to fy[] as they are read and are unwrapped in place.  false: unused.
__device__ bool floor1(const uint32_t *blob, const uint32_t *f, VBits &b, int16_t *fy, uint8_t *st) {
    const uint32_t books = blob[H_BOOKS];
    if (!b.read(1)) return false;
    const uint32_t mult = f[F_MULT];
    const int32_t range = mult == 1 ? 256 : mult == 2 ? 128 : mult == 3 ? 86 : 64;
    const uint32_t ybits = ilog((uint32_t)range - 1u);
    fy[0] = (int16_t)b.read(ybits);
    fy[1] = (int16_t)b.read(ybits);
    uint32_t at = 2;
    const uint32_t parts = f[F_PARTS], values = f[F_VALUES];
    for (uint32_t p = 0; p < parts; ++p) {
        const uint32_t cl = f[F_PCLASS + p], cdim = f[F_CDIM + cl], cbits = f[F_CSUB + cl];
        uint32_t cval = 0;
        if (cbits) {
            const int32_t v = huff(blob, books + f[F_CMASTER + cl] * B_SIZE, b);
            if (v < 0) return false;
            cval = (uint32_t)v;
        }
        for (uint32_t j = 0; j < cdim && at < values; ++j, ++at) {
            const uint32_t book = f[F_SUBBOOKS + 8u * cl + (cval & ((1u << cbits) - 1u))];
            cval >>= cbits;
            int32_t y = 0;
            if (book != 0xffffffffu) {
                y = huff(blob, books + book * B_SIZE, b);
                if (y < 0) return false;
            }
            fy[at] = (int16_t)(y > 32767 ? 32767 : y);
        }
    }
    if (b.eop) return false;
    // amplitude unwrapping (the specification's 7.2.4, step 1)
    fy[0] = fy[0] < range ? fy[0] : (int16_t)(range - 1);
    fy[1] = fy[1] < range ? fy[1] : (int16_t)(range - 1);
    st[0] = st[1] = 1;
    for (uint32_t i = 2; i < values; ++i) st[i] = 0;
    for (uint32_t i = 2; i < values; ++i) {
        const uint32_t lo = f[F_LOW + i], hi = f[F_HIGH + i];
        const int32_t pred = render_point((int32_t)f[F_X + lo], fy[lo], (int32_t)f[F_X + hi], fy[hi], (int32_t)f[F_X + i]);
        const int32_t val = fy[i], highroom = range - pred, lowroom = pred;
        const int32_t room = (highroom < lowroom ? highroom : lowroom) * 2;
        int32_t v = pred;
        if (val) {
            st[lo] = st[hi] = st[i] = 1;
            if (val >= room) v = highroom > lowroom ? val - lowroom + pred : pred - val + highroom - 1;
            else v = (val & 1) ? pred - ((val + 1) >> 1) : pred + (val >> 1);
        }
        fy[i] = (int16_t)(v < 0 ? 0 : v > range - 1 ? range - 1 : v);
    }
    return true;
}

// the specification's 8.6.2 for one submap: n_vec vectors of vec_len; type 2 comes here as one vector over nch channels
__device__ void residue(const uint32_t *blob, const uint32_t *r, VBits &b, uint32_t n_vec, uint32_t vec_len, uint32_t dnd_mask, const uint8_t *chans,
                        uint32_t nch, uint32_t n2, float *res, uint8_t *cls) {
    const uint32_t books = blob[H_BOOKS], type = r[R_TYPE];
    const uint32_t lb = r[R_BEGIN] < vec_len ? r[R_BEGIN] : vec_len, le = r[R_END] < vec_len ? r[R_END] : vec_len;
    const uint32_t ps = r[R_PSIZE], parts = (le - lb) / ps, nclass = r[R_NCLASS];
    const uint32_t cbook = books + r[R_CLASSBOOK] * B_SIZE, cw = blob[cbook + B_DIMS];
    if (parts == 0) return;
    for (uint32_t pass = 0; pass < 8; ++pass) {
        uint32_t pc = 0;
        while (pc < parts) {
            if (pass == 0) {
                for (uint32_t j = 0; j < n_vec; ++j) {
                    if (dnd_mask >> j & 1u) continue;
                    const int32_t t0 = huff(blob, cbook, b);
                    if (t0 < 0) return;
                    uint32_t t = (uint32_t)t0;
                    for (uint32_t i = cw; i-- > 0;) {
                        if (i + pc < parts) cls[j * parts + i + pc] = (uint8_t)(t % nclass);
                        t /= nclass;
                    }
                }
            }
            for (uint32_t i = 0; i < cw && pc < parts; ++i, ++pc) {
                for (uint32_t j = 0; j < n_vec; ++j) {
                    if (dnd_mask >> j & 1u) continue;
                    const uint32_t book = r[R_BOOKS + 8u * cls[j * parts + pc] + pass];
                    if (book == 0xffffffffu) continue;
                    const uint32_t rec = books + book * B_SIZE, dims = blob[rec + B_DIMS];
                    const float *vq = reinterpret_cast<const float *>(blob + blob[rec + B_VQ]);
                    const uint32_t off = lb + pc * ps, step = ps / dims;
                    for (uint32_t k = 0; k < step; ++k) {
                        const int32_t e = huff(blob, rec, b);
                        if (e < 0) return;
                        for (uint32_t d = 0; d < dims; ++d) {
                            const uint32_t idx = type == 0 ? off + k + d * step : off + k * dims + d;
                            float *dst = type == 2 ? res + chans[idx % nch] * n2 + idx / nch : res + chans[j] * n2 + idx;
                            *dst = *dst + vq[(uint32_t)e * dims + d];
                        }
                    }
                }
            }
        }
    }
}

__global__ void __launch_bounds__(64) k_vorbis_entropy(const VorbisPacket *packets, const uint32_t *by_length, uint32_t n_lanes, const uint32_t *blobs,
                                                       const uint8_t *bytes, float *res_base, uint8_t *cls_base, VorbisInfo *info) {
    const uint32_t lane = blockIdx.x * 64u + threadIdx.x;
    if (lane >= n_lanes) return;
    const uint32_t pi = by_length[lane];
    const VorbisPacket pk = packets[pi];
    const uint32_t *blob = blobs + pk.blob;
    VorbisInfo &o = info[pi];
    VBits b{reinterpret_cast<const uint32_t *>(bytes + pk.byte_offset), 0u, pk.byte_len * 8u, false};  // byte_len <= 16 MiB: the host refuses more
    const uint32_t type = b.read(1);
    if (b.eop || type) {
        o.status = b.eop ? kShort : kNotAudio;
        return;
    }
    const uint32_t mode = b.read(blob[H_MODEBITS]);
    if (b.eop || mode >= blob[H_NMODES]) {
        o.status = b.eop ? kShort : kBadMode;
        return;
    }
    const uint32_t flag = blob[blob[H_MODES] + mode * MODE_SIZE + MODE_FLAG];
    uint32_t prev = 0, next = 0;
    if (flag) {
        prev = b.read(1), next = b.read(1);
        if (b.eop) {
            o.status = kShort;
            return;
        }
    }
    const uint32_t n = blob[flag ? H_BS1 : H_BS0], n2 = n >> 1, ch = blob[H_CHANNELS];
    o.mode = (uint8_t)mode, o.blockflag = (uint8_t)flag, o.prev_flag = (uint8_t)prev, o.next_flag = (uint8_t)next, o.n = n;
    if (n != pk.n) {  // the host read the same bits: cannot differ; nothing is written where the host did not reserve room
        o.status = kBadMode;
        return;
    }
    const uint32_t *map = blob + blob[H_MAPPINGS] + blob[blob[H_MODES] + mode * MODE_SIZE + MODE_MAPPING] * M_SIZE;
    uint32_t no_res = 0;
    for (uint32_t c = 0; c < ch; ++c) {
        const uint32_t *f = blob + blob[H_FLOORS] + map[M_FLOOR + map[M_MUX + c]] * F_SIZE;
        const bool used = !b.eop && floor1(blob, f, b, o.final_y[c], o.step2[c]);
        o.used[c] = used;
        if (!used) {
            no_res |= 1u << c;
            for (uint32_t i = 0; i < kMaxPosts; ++i) o.final_y[c][i] = 0, o.step2[c][i] = 0;
        }
    }
    const uint32_t *steps = blob + map[M_COUPLING];
    for (uint32_t i = 0; i < map[M_NCOUPLING]; ++i) {
        const uint32_t mag = steps[i] & 0xffu, ang = steps[i] >> 8;
        if (!((no_res >> mag & 1u) && (no_res >> ang & 1u))) no_res &= ~(1u << mag | 1u << ang);
    }
    float *res = res_base + pk.res_offset;
    uint8_t *cls = cls_base + pk.cls_offset;
    for (uint32_t sm = 0; sm < map[M_SUBMAPS]; ++sm) {
        uint8_t chans[kMaxChannels];
        uint32_t nch = 0, dnd = 0;
        for (uint32_t c = 0; c < ch; ++c)
            if (map[M_MUX + c] == sm) {
                if (no_res >> c & 1u) dnd |= 1u << nch;
                chans[nch++] = (uint8_t)c;
            }
        if (nch == 0 || dnd == (1u << nch) - 1u) continue;
        const uint32_t *r = blob + blob[H_RESIDUES] + map[M_RESIDUE + sm] * R_SIZE;
        if (r[R_TYPE] == 2) residue(blob, r, b, 1, n2 * nch, 0, chans, nch, n2, res, cls);
        else residue(blob, r, b, nch, n2, dnd, chans, nch, n2, res, cls);
    }
    o.status = 0;
}

__global__ void __launch_bounds__(256) k_vorbis_spectrum(const VorbisPacket *packets, const uint32_t *blobs, const VorbisInfo *info, float *res_base,
                                                         VorbisTables t) {
    __shared__ int32_t px[kMaxPosts], py[kMaxPosts];
    __shared__ uint32_t posts;
    const VorbisPacket pk = packets[blockIdx.x];
    const VorbisInfo &o = info[blockIdx.x];
    if (pk.n == 0 || o.status != 0) return;
    const uint32_t *blob = blobs + pk.blob;
    const uint32_t n2 = pk.n >> 1, ch = pk.channels;
    const uint32_t *map = blob + blob[H_MAPPINGS] + blob[blob[H_MODES] + o.mode * MODE_SIZE + MODE_MAPPING] * M_SIZE;
    float *res = res_base + pk.res_offset;
    const uint32_t *steps = blob + map[M_COUPLING];
    const uint32_t n_steps = map[M_NCOUPLING];
    for (uint32_t x = threadIdx.x; x < n2 && n_steps; x += 256u) {
        for (uint32_t i = n_steps; i-- > 0;) {
            float *pm = res + (steps[i] & 0xffu) * n2 + x, *pa = res + (steps[i] >> 8) * n2 + x;
            const float m = *pm, a = *pa;
            float nm, na;
            if (m > 0.0f) {
                if (a > 0.0f) nm = m, na = m - a;
                else na = m, nm = m + a;
            } else {
                if (a > 0.0f) nm = m, na = m + a;
                else na = m, nm = m - a;
            }
            *pm = nm, *pa = na;
        }
    }
    for (uint32_t c = 0; c < ch; ++c) {
        float *v = res + c * n2;
        if (!o.used[c]) {
            for (uint32_t x = threadIdx.x; x < n2; x += 256u) v[x] = 0.0f;
            continue;
        }
        const uint32_t *f = blob + blob[H_FLOORS] + map[M_FLOOR + map[M_MUX + c]] * F_SIZE;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t k = 0;
            const int32_t mult = (int32_t)f[F_MULT];
            for (uint32_t i = 0; i < f[F_VALUES]; ++i) {
                const uint32_t j = f[F_SORTED + i];
                if (i == 0 || o.step2[c][j]) px[k] = (int32_t)f[F_X + j], py[k] = o.final_y[c][j] * mult, ++k;
            }
            posts = k;
        }
        __syncthreads();
        const uint32_t np = posts;
        for (uint32_t x = threadIdx.x; x < n2; x += 256u) {
            uint32_t s = 0;
            while (s + 1 < np && px[s + 1] <= (int32_t)x) ++s;
            int32_t y = py[s];
            if (s + 1 < np) {
                const int32_t dy = py[s + 1] - py[s], adx = px[s + 1] - px[s], k = (int32_t)x - px[s];
                const int32_t base = dy / adx, ady = (dy < 0 ? -dy : dy) - (base < 0 ? -base : base) * adx;
                const int32_t steps_up = k * ady / adx;
                y = py[s] + base * k + (dy < 0 ? -steps_up : steps_up);
            }
            y = y < 0 ? 0 : y > 255 ? 255 : y;
            v[x] = t.inverse_db[y] * v[x];
        }
    }
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

__global__ void __launch_bounds__(256) k_vorbis_imdct(const VorbisPacket *packets, const uint32_t *blobs, const VorbisInfo *info, const float *res_base,
                                                      float *pcm_base, VorbisTables t) {
    __shared__ float2 a[2048];
    const VorbisPacket pk = packets[blockIdx.x];
    const VorbisInfo &o = info[blockIdx.x];
    const uint32_t c = blockIdx.y;
    if (pk.n == 0 || o.status != 0 || c >= pk.channels) return;
    const uint32_t *blob = blobs + pk.blob;
    const uint32_t n = pk.n, m = n >> 1, n4 = n >> 2, bits = 31u - (uint32_t)__builtin_clz(n4), e = bits + 2u - 6u;
    const float *X = res_base + pk.res_offset + c * m;
    const float2 *tw = t.twiddle[e], *root = t.root[e];
    for (uint32_t j = threadIdx.x; j < n4; j += 256u)
        a[__brev(j) >> (32u - bits)] = cmul(make_float2(X[2u * j], X[m - 1u - 2u * j]), tw[j]);
    __syncthreads();
    for (uint32_t half = 1, stride = n4 >> 1; half < n4; half <<= 1, stride >>= 1) {
        for (uint32_t q = threadIdx.x; q < (n4 >> 1); q += 256u) {
            const uint32_t k = q & (half - 1u), i0 = ((q - k) << 1) + k, i1 = i0 + half;
            const float2 tt = cmul(a[i1], root[k * stride]), lo = a[i0];
            a[i0] = make_float2(lo.x + tt.x, lo.y + tt.y);
            a[i1] = make_float2(lo.x - tt.x, lo.y - tt.y);
        }
        __syncthreads();
    }
    // u[2k] = Re v[k] lies where a[k].x lay and u[m - 1 - 2k] = -Im v[k] where a[n4 - 1 - k].y lay: a lane takes k and n4 - 1 - k
    // together, so that nobody else reads what it overwrites
    for (uint32_t k = threadIdx.x; k < (n4 >> 1); k += 256u) {
        const uint32_t k2 = n4 - 1u - k;
        const float2 v = cmul(a[k], tw[k]), v2 = cmul(a[k2], tw[k2]);
        a[k] = make_float2(v.x, -v2.y);
        a[k2] = make_float2(v2.x, -v.y);
    }
    __syncthreads();
    const float *u = reinterpret_cast<const float *>(a);  // [m]
    // the window: slopes of bs0 / 2 or bs1 / 2 as the flags of a long block say, short slopes on a short block
    const uint32_t bs0 = blob[H_BS0], bs1 = blob[H_BS1];
    const uint32_t ln = ((o.blockflag && o.prev_flag) ? bs1 : bs0) >> 1, rn = ((o.blockflag && o.next_flag) ? bs1 : bs0) >> 1;
    const uint32_t ls = n4 - (ln >> 1), rs = 3u * n4 - (rn >> 1);
    const float *lslope = t.slope[31u - (uint32_t)__builtin_clz(ln) + 1u - 6u], *rslope = t.slope[31u - (uint32_t)__builtin_clz(rn) + 1u - 6u];
    float *out = pcm_base + pk.pcm_offset + c * n;
    for (uint32_t i = threadIdx.x; i < n; i += 256u) {
        const float y = i < n4 ? u[n4 + i] : i < 3u * n4 ? -u[3u * n4 - 1u - i] : -u[i - 3u * n4];
        float w;
        if (i < ls) w = 0.0f;
        else if (i < ls + ln) w = lslope[i - ls];
        else if (i < rs) w = 1.0f;
        else if (i < rs + rn) w = rslope[rn - 1u - (i - rs)];
        else w = 0.0f;
        out[i] = y * w;
    }
}

__global__ void __launch_bounds__(256) k_vorbis_ola(const VorbisPacket *packets, const VorbisInfo *info, const float *pcm_base, const float *carry,
                                                    void *out, int as_f32) {
    const VorbisPacket pk = packets[blockIdx.x];
    if (pk.n == 0 || info[blockIdx.x].status != 0 || pk.out_frames == 0) return;
    const uint32_t n = pk.n, pn = pk.prev_n, ch = pk.channels, frames = pk.out_frames;
    const float *right = (pk.prev_in_carry ? carry : pcm_base) + pk.prev_pcm;
    const uint32_t rstride = pk.prev_in_carry ? pn >> 1 : pn;
    const float *left = pcm_base + pk.pcm_offset;
    for (uint32_t q = threadIdx.x; q < frames * ch; q += 256u) {
        const uint32_t f = q / ch, c = q - f * ch, i = f + pk.out_skip;
        const float *R = right + c * rstride, *L = left + c * n;
        float v;
        if (pn == n) {
            v = R[i] + L[i];
        } else if (pn > n) {
            const uint32_t a = (pn >> 2) - (n >> 2);
            v = i < a ? R[i] : R[i] + L[i - a];
        } else {
            const uint32_t a = (n >> 2) - (pn >> 2);
            v = i < (pn >> 1) ? R[i] + L[a + i] : L[a + i];
        }
        if (as_f32) {
            reinterpret_cast<float *>(out)[pk.out_offset + q] = v;
        } else {
            const float s = v * 32768.0f;  // exact
            const int32_t k = s != s ? 0 : s >= 32767.0f ? 32767 : s <= -32768.0f ? -32768 : (int32_t)s;
            reinterpret_cast<int16_t *>(out)[pk.out_offset + q] = (int16_t)k;
        }
    }
}

// what a stream leaves with: the right half of its last accepted packet, [channels][n / 2], into the carry buffer (after k_vorbis_ola
// has read what the stream entered with)
__global__ void __launch_bounds__(256) k_vorbis_carry(const VorbisPacket *packets, const VorbisCarry *carries, const float *pcm_base, float *carry) {
    const VorbisCarry cr = carries[blockIdx.x];
    if (cr.packet == 0xffffffffu) return;
    const VorbisPacket pk = packets[cr.packet];
    const uint32_t n = pk.n, half = n >> 1;
    for (uint32_t q = threadIdx.x; q < half * pk.channels; q += 256u) {
        const uint32_t c = q / half, i = q - c * half;
        carry[cr.offset + q] = pcm_base[pk.pcm_offset + c * n + half + i];
    }
}

}  // namespace

hipError_t launch_vorbis_carry(const VorbisPacket *packets, const VorbisCarry *carries, uint32_t n_streams, const float *pcm, float *carry, hipStream_t s) {
    if (n_streams == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vorbis_carry, dim3(n_streams), dim3(256), 0, s, packets, carries, pcm, carry);
    return hipGetLastError();
}

hipError_t launch_vorbis_entropy(const VorbisPacket *packets, const uint32_t *by_length, uint32_t n_lanes, const uint32_t *blobs, const uint8_t *bytes,
                                 float *res, uint8_t *cls, VorbisInfo *info, hipStream_t s) {
    if (n_lanes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vorbis_entropy, dim3((n_lanes + 63u) / 64u), dim3(64), 0, s, packets, by_length, n_lanes, blobs, bytes, res, cls, info);
    return hipGetLastError();
}

hipError_t launch_vorbis_spectrum(const VorbisPacket *packets, uint32_t n_packets, const uint32_t *blobs, const VorbisInfo *info, float *res,
                                  const VorbisTables &t, hipStream_t s) {
    if (n_packets == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vorbis_spectrum, dim3(n_packets), dim3(256), 0, s, packets, blobs, info, res, t);
    return hipGetLastError();
}

hipError_t launch_vorbis_imdct(const VorbisPacket *packets, uint32_t n_packets, const uint32_t *blobs, const VorbisInfo *info, const float *res, float *pcm,
                               uint32_t max_channels, const VorbisTables &t, hipStream_t s) {
    if (n_packets == 0 || max_channels == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vorbis_imdct, dim3(n_packets, max_channels < kMaxChannels ? max_channels : kMaxChannels), dim3(256), 0, s, packets, blobs, info, res,
                       pcm, t);
    return hipGetLastError();
}

hipError_t launch_vorbis_ola(const VorbisPacket *packets, uint32_t n_packets, const VorbisInfo *info, const float *pcm, const float *carry, void *out,
                             int as_f32, hipStream_t s) {
    if (n_packets == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vorbis_ola, dim3(n_packets), dim3(256), 0, s, packets, info, pcm, carry, out, as_f32);
    return hipGetLastError();
}

}  // namespace sk

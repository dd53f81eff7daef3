// mp3_entropy.hip -- parts 2 and 3 of the Layer III main data on gfx950: scale factors (11172-3 2.4.2.7, 13818-3 2.4.3.2), big-values
// pairs and count1 quadruples (2.4.3.4.6).  The device counterpart of sk_mp3_decode_main_data (mp3_decoder.cpp), which is its
// specification: every field of sk_mp3_granule_data comes out bit for bit, the damaged cases included.
//
// One granule-channel per lane.  Where an item starts in its frame's main data is a prefix sum of part2_3_length, known from the
// side information, so the up to four items of a frame are independent -- except scfsi: granule 1 takes scale-factor groups
// from granule 0 of its channel, and gets them by reading those fields of granule 0 again (their bit positions are closed forms).
// The host hands the items out sorted by part2_3_length: a wave runs until its slowest lane is done.
//
// Code tables: any prefix code set with codes of up to 32 bits (sk_mp3_codebook_flatten).  A first-level look-up on the next
// 8 bits per distinct table, all of them in LDS together with the header (19 KiB for the standard's tables); an entry either
// is the code or names a further table, indexed by the next <= 8 bits, in global memory (L2).  Integer work only.
//
// Output: a lane gathers its integers 32 at a time in LDS (16 words per lane, its own column) and writes each full group
// as four 16-byte stores -- half a cache line -- instead of one 4-byte store per pair, 1152 bytes from its neighbour's.
#include "sk_device.h"

namespace sk {

namespace {

struct Bits {  // bits past the end of the item read as zero, and the position keeps counting
    const uint32_t *words;
    uint32_t len_bytes;
    uint32_t pos;
    uint32_t at, w0, w1;  // the two words the position lies in

    __device__ __forceinline__ uint32_t word(uint32_t i) const {
        const uint32_t byte = i * 4u;  // (i < 2^27: positions are sums of a few 16-bit lengths)
        if (byte >= len_bytes) return 0u;
        uint32_t v = __builtin_bswap32(words[i]);  // inside the buffer: the item has >= 8 bytes of room behind it
        const uint32_t left = len_bytes - byte;
        if (left < 4u) v &= ~0u << (8u * (4u - left));
        return v;
    }
    __device__ __forceinline__ uint32_t peek32() {
        const uint32_t i = pos >> 5;
        if (i != at) {
            if (i == at + 1u) w0 = w1;
            else w0 = word(i);
            w1 = word(i + 1u);
            at = i;
        }
        const uint32_t s = pos & 31u;
        return s ? (w0 << s) | (w1 >> (32u - s)) : w0;
    }
    __device__ __forceinline__ uint32_t get(uint32_t n) {  // n <= 32
        if (n == 0) return 0u;
        const uint32_t v = peek32() >> (32u - n);
        pos += n;
        return v;
    }
    // n <= 25 bits at any position, past the reader
    __device__ __forceinline__ uint32_t at_bit(uint32_t bit, uint32_t n) const {
        if (n == 0) return 0u;
        const uint32_t i = bit >> 5, s = bit & 31u;
        const uint32_t a = word(i), b = word(i + 1u);
        return (s ? (a << s) | (b >> (32u - s)) : a) >> (32u - n);
    }
};

// the code the next bits start with: its entry (0: none), position advanced
__device__ __forceinline__ uint32_t read_code(Bits &b, const uint32_t *lds, const uint32_t *blob, uint32_t first) {
    uint32_t v = b.peek32();
    uint32_t e = lds[first + (v >> (32u - kMp3L1Bits))];
    uint32_t width = kMp3L1Bits, used = 0;
    while ((e & 0x80000000u) && used < 32u) {
        used += width;
        v <<= width;
        width = (e >> 26) & 31u;
        e = blob[(e & 0x03ffffffu) + (v >> (32u - width))];
    }
    if (e & 0x80000000u) return 0u;
    b.pos += used + ((e >> 16) & 63u);
    return e;
}

constexpr int kGroupLines = 32;  // lines a lane gathers before it writes them out: 64 bytes

struct Row {  // the 576 integers of one item on their way out
    uint32_t *stage;  // the lane's column of the wave's staging area: word k at stage[k * 64]
    uint4 *out;
    int line;
    __device__ __forceinline__ void flush(int group) {
        uint4 *dst = out + group * (kGroupLines * 2 / 16);
#pragma unroll
        for (int q = 0; q < kGroupLines / 8; ++q) dst[q] = make_uint4(stage[(4 * q) * 64], stage[(4 * q + 1) * 64], stage[(4 * q + 2) * 64], stage[(4 * q + 3) * 64]);
    }
    __device__ __forceinline__ void pair(int x, int y) {  // line is even and < 576
        stage[((line >> 1) & (kGroupLines / 2 - 1)) * 64] = ((uint32_t)x & 0xffffu) | ((uint32_t)y << 16);
        line += 2;
        if ((line & (kGroupLines - 1)) == 0) flush(line / kGroupLines - 1);
    }
    // zeros from `from` (even) to line 576
    __device__ __forceinline__ void zero_rest(int from) {
        line = from;
        while (line & (kGroupLines - 1)) pair(0, 0);
        for (int g = line / kGroupLines; g < 576 / kGroupLines; ++g) {
            uint4 *dst = out + g * (kGroupLines * 2 / 16);
#pragma unroll
            for (int q = 0; q < kGroupLines / 8; ++q) dst[q] = make_uint4(0u, 0u, 0u, 0u);
        }
        line = 576;
    }
};

__device__ __forceinline__ int rate_row(uint32_t hz) {
    const uint32_t rates[kMp3Rates] = {44100, 48000, 32000, 22050, 24000, 16000, 11025, 12000, 8000};
    int row = -1;
#pragma unroll
    for (int i = 0; i < (int)kMp3Rates; ++i) row = rates[i] == hz ? i : row;
    return row;
}

struct ScaleOut {  // where an item's scale factors go: its requantisation record or its cell
    uint8_t *l, *s;
};

// 11172-3 2.4.2.7 (scale_factors_v1)
__device__ void scale_factors_v1(const Mp3CodebookHeader &h, const sk_mp3_side_info &side, int gr, int ch, uint32_t start0, Bits &b, const ScaleOut &o) {
    const sk_mp3_granule_side &s = side.gr[gr][ch];
    const uint32_t slen1 = h.slen[s.scalefac_compress & 15][0], slen2 = h.slen[s.scalefac_compress & 15][1];
    if (s.window_switching && s.block_type == 2) {
        int first_short = 0;
        if (s.mixed_block_flag) {
            for (int band = 0; band < 8; ++band) o.l[band] = (uint8_t)b.get(slen1);
            first_short = 3;
        }
        for (int band = first_short; band < 12; ++band)
            for (int w = 0; w < 3; ++w) o.s[band * 3 + w] = (uint8_t)b.get(band < 6 ? slen1 : slen2);
        return;
    }
    // what granule 0 of this channel holds in its long bands, read again where scfsi says "as before": nothing if its
    // part2_3_length reaches past the main data (it was not decoded), its first 8 bands if it is a mixed block, none if short
    const sk_mp3_granule_side &s0 = side.gr[0][ch];
    const uint32_t z1 = h.slen[s0.scalefac_compress & 15][0], z2 = h.slen[s0.scalefac_compress & 15][1];
    const bool g0_read = start0 + s0.part2_3_length <= b.len_bytes * 8u;
    const bool g0_short = s0.window_switching && s0.block_type == 2;
    for (int band = 0; band < 21; ++band) {
        const int group = band < 6 ? 0 : (band < 11 ? 1 : (band < 16 ? 2 : 3));
        uint32_t v;
        if (gr == 1 && side.scfsi[ch][group]) {
            v = 0;
            if (g0_read) {
                if (!g0_short) v = band < 11 ? b.at_bit(start0 + (uint32_t)band * z1, z1) : b.at_bit(start0 + 11u * z1 + (uint32_t)(band - 11) * z2, z2);
                else if (s0.mixed_block_flag && band < 8) v = b.at_bit(start0 + (uint32_t)band * z1, z1);
            }
        } else {
            v = b.get(group < 2 ? slen1 : slen2);
        }
        o.l[band] = (uint8_t)v;
    }
}

// 13818-3 2.4.3.2 (scale_factors_lsf); returns preflag
__device__ int scale_factors_lsf(const Mp3CodebookHeader &h, const sk_mp3_frame_info &f, const sk_mp3_granule_side &s, int ch, Bits &b, const ScaleOut &o,
                                 uint8_t *intensity_scale) {
    uint32_t slen[4] = {0, 0, 0, 0};
    int row, preflag = 0;
    uint32_t sfc = s.scalefac_compress;
    const bool intensity_channel = f.mode == 1 && (f.mode_ext & 1) && ch == 1;
    if (!intensity_channel) {
        if (sfc < 400) {
            slen[0] = (sfc >> 4) / 5, slen[1] = (sfc >> 4) % 5, slen[2] = (sfc & 15) >> 2, slen[3] = sfc & 3;
            row = 0;
        } else if (sfc < 500) {
            sfc -= 400;
            slen[0] = (sfc >> 2) / 5, slen[1] = (sfc >> 2) % 5, slen[2] = sfc & 3;
            row = 1;
        } else {
            sfc -= 500;
            slen[0] = sfc / 3, slen[1] = sfc % 3;
            preflag = 1;
            row = 2;
        }
    } else {
        *intensity_scale = (uint8_t)(sfc & 1);
        sfc >>= 1;
        if (sfc < 180) {
            slen[0] = sfc / 36, slen[1] = (sfc % 36) / 6, slen[2] = (sfc % 36) % 6;
            row = 3;
        } else if (sfc < 244) {
            sfc -= 180;
            slen[0] = (sfc & 63) >> 4, slen[1] = (sfc & 15) >> 2, slen[2] = sfc & 3;
            row = 4;
        } else {
            sfc -= 244;
            slen[0] = sfc / 3, slen[1] = sfc % 3;
            row = 5;
        }
    }
    const int column = (s.window_switching && s.block_type == 2) ? (s.mixed_block_flag ? 2 : 1) : 0;
    const uint8_t *parts = h.lsf_partitions[row][column];
    int index = 0;
    const int long_bands = column == 0 ? 22 : (column == 2 ? 6 : 0);
    for (int part = 0; part < 4; ++part) {
        const uint32_t n = slen[part];
        for (int k = 0; k < parts[part]; ++k, ++index) {
            uint32_t v = b.get(n) & 0xffu;
            if (intensity_channel && n > 0 && v == ((1u << n) - 1u)) v |= 0x80u;  // "not intensity coded"
            if (index < long_bands) {
                if (index < 22) o.l[index] = (uint8_t)v;
            } else {
                const int rel = index - long_bands + (column == 2 ? 9 : 0);
                if (rel < 39) o.s[rel] = (uint8_t)v;
            }
        }
    }
    return preflag;
}

// 2.4.3.4.6 (huffman): SK_OK or the status; on SK_OK the row is complete
__device__ int huffman(const Mp3CodebookHeader &h, const uint32_t *lds, const uint32_t *blob, const sk_mp3_frame_info &f, const sk_mp3_granule_side &s, Bits &b,
                       uint32_t end_bit, Row &r, Mp3EntropyCell &cell) {
    const uint32_t start_bit = b.pos;
    const int rate = rate_row(f.sample_rate);
    if (rate < 0 || !h.rates_present[rate]) return SK_MP3_UNSUPPORTED;
    const int cut = (s.window_switching && s.block_type == 2) ? (s.mixed_block_flag ? 2 : 1) : 0;
    const uint16_t *region = h.region[rate][cut];
    const int big_end = 2 * (int)s.big_values;
    if (big_end > 576) return SK_MP3_INVALID;
    int region1 = region[min((int)s.region0_count + 1, (int)kMp3RegionCounts - 1)];
    int region2 = region[min((int)s.region0_count + 1 + (int)s.region1_count + 1, (int)kMp3RegionCounts - 1)];
    if (s.window_switching) region2 = 576;  // two regions only
    region1 = min(region1, big_end), region2 = min(region2, big_end);
    const int bounds[4] = {0, region1, region2, big_end};
    for (int k = 0; k < 3; ++k) {
        const uint32_t select = s.table_select[k] & 31u;
        const uint32_t t = h.big[select];
        const uint32_t xlen = t & 0xffu, linbits = (t >> 8) & 0xffu, first = t >> 16;
        if (r.line >= bounds[k + 1]) continue;
        if (!xlen) {
            if (select != 0) return SK_MP3_INVALID;  // a region that holds lines names a table without codes (4, 14)
            while (r.line < bounds[k + 1]) r.pair(0, 0);
            continue;
        }
        while (r.line < bounds[k + 1]) {
            const uint32_t e = read_code(b, lds, blob, first);
            if (!e) return SK_MP3_INVALID;
            int x = (int)((e >> 4) & 15u), y = (int)(e & 15u);
            // x escape, x sign, y escape, y sign: at most 13 + 1 + 13 + 1 bits
            uint32_t v = b.peek32(), used = 0;
            if (linbits && x == (int)xlen - 1) x += (int)(v >> (32u - linbits)), v <<= linbits, used += linbits;
            if (x) {
                if (v >> 31) x = -x;
                v <<= 1, used += 1;
            }
            if (linbits && y == (int)xlen - 1) y += (int)(v >> (32u - linbits)), v <<= linbits, used += linbits;
            if (y) {
                if (v >> 31) y = -y;
                used += 1;
            }
            b.pos += used;
            r.pair(x, y);
        }
    }
    if (b.pos > end_bit) return SK_MP3_INVALID;  // the big values alone overran part2_3_length
    uint32_t accepted = b.pos;
    const uint32_t first = h.count1[s.count1table_select & 1];
    while (b.pos < end_bit && r.line + 4 <= 576) {
        const uint32_t e = read_code(b, lds, blob, first);
        if (!e) return SK_MP3_INVALID;
        uint32_t v = b.peek32(), used = 0;
        int q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            q[k] = (int)((e >> (3 - k)) & 1u);
            if (q[k]) {
                if (v >> 31) q[k] = -1;
                v <<= 1, used += 1;
            }
        }
        b.pos += used;
        if (b.pos > end_bit) break;  // a quadruple that reaches past the end is stuffing, not data
        r.pair(q[0], q[1]);
        r.pair(q[2], q[3]);
        accepted = b.pos;
    }
    cell.part3_bits = (uint16_t)(accepted - start_bit);
    cell.nonzero_lines = (uint16_t)r.line;
    r.zero_rest(r.line);
    return SK_OK;
}

}  // namespace

__global__ __launch_bounds__(64) void k_mp3_entropy(Mp3EntropyArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // header | first-level tables
    __shared__ uint32_t stage[kGroupLines / 2][64];
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(a.blob);
        uint4 *dst = reinterpret_cast<uint4 *>(lds);
        for (uint32_t i = threadIdx.x; i < a.lds_words / 4; i += 64) dst[i] = src[i];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x, per_wave = 64u >> a.lane_shift;
    const uint32_t slot = blockIdx.x * per_wave + lane;
    if (lane >= per_wave || slot >= a.n_items) return;
    const Mp3CodebookHeader &h = *reinterpret_cast<const Mp3CodebookHeader *>(lds);
    const Mp3EntropyItem it = a.items[slot];
    const sk_mp3_frame_item &fr = a.frames[it.frame];
    const sk_mp3_side_info &side = fr.side;
    const int gr = it.gr, ch = it.ch;
    const sk_mp3_granule_side &s = side.gr[gr][ch];

    uint32_t start = 0, start0 = 0;  // of this item, and of granule 0 of its channel
    for (int g = 0; g <= gr; ++g)
        for (int c = 0; c < (int)side.channels; ++c) {
            if (g == 0 && c < ch) start0 += side.gr[0][c].part2_3_length;
            if (g < gr || c < ch) start += side.gr[g][c].part2_3_length;
        }
    const uint32_t end = start + s.part2_3_length;

    const uint32_t cell_at = it.frame * 4u + (uint32_t)gr * 2u + (uint32_t)ch;
    Mp3EntropyCell cell = {};  // the scale factors go straight to memory (zeroed by the host); the rest is stored at the end
    Mp3EntropyCell *cell_out = a.cells + cell_at;
    ScaleOut so;
    uint8_t *preflag_out;
    if (it.record != 0xffffffffu) {
        sk_mp3_requant_channel &rc = a.records[it.record].ch[ch];
        so.l = rc.scalefac_l, so.s = &rc.scalefac_s[0][0], preflag_out = &rc.preflag;
    } else {
        so.l = cell_out->scalefac_l, so.s = &cell_out->scalefac_s[0][0], preflag_out = &cell_out->preflag;
    }

    Bits b;
    b.words = reinterpret_cast<const uint32_t *>(a.bytes + fr.byte_offset);
    b.len_bytes = fr.byte_len;
    b.pos = start;
    b.at = 0xfffffff0u, b.w0 = 0, b.w1 = 0;
    Row r;
    r.stage = &stage[0][lane];
    r.out = reinterpret_cast<uint4 *>(a.is + (size_t)it.row * 576);
    r.line = 0;

    int rc = SK_OK;
    if (end > b.len_bytes * 8u) rc = SK_MP3_NEED_MORE;
    if (rc == SK_OK) {
        int preflag;
        if (fr.header.version == 1) {
            preflag = s.preflag;
            scale_factors_v1(h, side, gr, ch, start0, b, so);
        } else {
            preflag = scale_factors_lsf(h, fr.header, s, ch, b, so, &cell.intensity_scale);
        }
        cell.preflag = (uint8_t)preflag;
        *preflag_out = (uint8_t)preflag;
        cell.part2_bits = (uint16_t)(b.pos - start);
        if (b.pos > end) rc = SK_MP3_INVALID;  // the scale factors alone overran part2_3_length
    }
    if (rc == SK_OK) rc = huffman(h, lds, a.blob, fr.header, s, b, end, r, cell);
    if (rc != SK_OK) {
        cell.part3_bits = 0, cell.nonzero_lines = 0;
        r.zero_rest(0);  // a failed granule-channel has all 576 integers zero
    }
    cell.status = rc;
    cell_out->preflag = cell.preflag;
    cell_out->intensity_scale = cell.intensity_scale;
    cell_out->part2_bits = cell.part2_bits;
    cell_out->nonzero_lines = cell.nonzero_lines;
    cell_out->part3_bits = cell.part3_bits;
    cell_out->status = rc;
    a.status[cell_at] = rc;
}

hipError_t launch_mp3_entropy(const Mp3EntropyArgs &a, hipStream_t s) {
    if (a.n_items == 0) return hipSuccess;
    const uint32_t per_wave = 64u >> a.lane_shift;
    k_mp3_entropy<<<(a.n_items + per_wave - 1) / per_wave, 64, a.lds_words * sizeof(uint32_t), s>>>(a);
    return hipGetLastError();
}

}  // namespace sk

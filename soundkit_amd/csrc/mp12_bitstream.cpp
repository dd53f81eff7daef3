// mp12_bitstream.cpp -- the host side of MPEG Layer I and II (ISO/IEC 11172-3 2.4.1.5-6 / 2.4.2.5-6, 13818-3 2.4.1-2): a header
// parse and a frame scan that know all three layers, and the serial front of a Layer I / II frame -- bit allocation, scale-factor
// selection, scale factors -- read into the record the kernel works from (csrc/mp12_synth.hip).  Behind that front every sample
// code stands at a position that follows from the allocation alone, so the samples stay in the frame's bytes and are unpacked on
// the device.  A frame whose samples would end beyond its bytes is rejected HERE: what reaches the kernel never reads past a frame.
// Tables: mp12_tables.h.  Checked against a float64 model and a frame writer with tables of their own (tests/mp12_model.py,
// tests/mp12_builder.py) and on the reference's MP2 fixture (tests/golden/mp2).
#include "mp12_internal.h"
#include "mp12_tables.h"

#include <cstring>

namespace sk_mp12 {

namespace {

const uint32_t kSampleRate[2][3] = {{44100, 48000, 32000}, {22050, 24000, 16000}};  // MPEG-1, MPEG-2
const uint16_t kBitrateV1L3[16] = {0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 0};

struct Bits {
    const uint8_t *p;
    size_t len;      // bytes
    size_t pos = 0;  // bits; reads beyond len give zeros (the caller compares pos with the frame's end)
    uint32_t get(int n) {
        uint32_t v = 0;
        for (int i = 0; i < n; ++i, ++pos) {
            const size_t byte = pos >> 3;
            v = (v << 1) | (byte < len ? (p[byte] >> (7 - (pos & 7))) & 1u : 0u);
        }
        return v;
    }
};

uint8_t class_of_steps(uint32_t steps) {
    if (steps == 3 || steps == 5 || steps == 9) return (uint8_t)(0x80u | steps);
    uint8_t bits = 0;
    while ((1u << bits) - 1u < steps) ++bits;
    return bits;  // steps = 2^bits - 1
}

bool same_stream(const sk_mpa_frame_info &a, const sk_mpa_frame_info &b) {
    return a.version == b.version && a.layer == b.layer && a.sample_rate == b.sample_rate;
}

}  // namespace

int class_bits(int layer, uint8_t cls) {
    if (cls == 0) return 0;
    if (layer == 1) return cls >= 2 && cls <= 15 ? cls : -1;
    if (cls == (0x80 | 3)) return 5;
    if (cls == (0x80 | 5)) return 7;
    if (cls == (0x80 | 9)) return 10;
    return cls >= 3 && cls <= 16 ? 3 * cls : -1;
}

int parse_header(const uint8_t *d, size_t len, sk_mpa_frame_info *out) {
    if (!d || !out) return SK_ERR_INVALID_ARG;
    if (len < 4) return SK_MP3_NEED_MORE;
    if (d[0] != 0xff || (d[1] & 0xe0) != 0xe0) return SK_MP3_NO_SYNC;
    const unsigned version_bits = (d[1] >> 3) & 3;  // 00 MPEG-2.5, 01 reserved, 10 MPEG-2, 11 MPEG-1
    const unsigned layer_bits = (d[1] >> 1) & 3;    // 11 Layer I, 10 Layer II, 01 Layer III
    if (version_bits == 1 || layer_bits == 0) return SK_MP3_NO_SYNC;
    const unsigned bitrate_index = d[2] >> 4, sr_index = (d[2] >> 2) & 3;
    if (bitrate_index == 15 || sr_index == 3) return SK_MP3_NO_SYNC;
    const int layer = 4 - (int)layer_bits;
    if (bitrate_index == 0) return SK_MP3_UNSUPPORTED;                // free format: the length is not in the header
    if (version_bits == 0 && layer != 3) return SK_MP3_UNSUPPORTED;  // MPEG-2.5 is a Layer III extension
    const bool lsf = version_bits != 3;
    std::memset(out, 0, sizeof *out);
    out->version = version_bits == 3 ? 1 : (version_bits == 2 ? 2 : 25);
    out->layer = (uint8_t)layer;
    out->has_crc = (d[1] & 1) ? 0 : 1;
    out->sample_rate = kSampleRate[lsf ? 1 : 0][sr_index] >> (version_bits == 0 ? 1 : 0);
    out->padding = (d[2] >> 1) & 1;
    out->mode = d[3] >> 6;  // 0 stereo, 1 joint stereo, 2 dual channel, 3 single channel
    out->mode_ext = (d[3] >> 4) & 3;
    out->channels = out->mode == 3 ? 1 : 2;
    const uint32_t fs = out->sample_rate;
    if (layer == 1) {
        out->bitrate_kbps = lsf ? kBitrateV2L1[bitrate_index] : kBitrateV1L1[bitrate_index];
        out->samples_per_channel = 384;
        out->frame_bytes = (12u * out->bitrate_kbps * 1000u / fs + out->padding) * 4u;
    } else if (layer == 2) {
        out->bitrate_kbps = lsf ? kBitrateV2L2[bitrate_index] : kBitrateV1L2[bitrate_index];
        out->samples_per_channel = 1152;
        out->frame_bytes = 144u * out->bitrate_kbps * 1000u / fs + out->padding;
    } else {
        out->bitrate_kbps = lsf ? kBitrateV2L2[bitrate_index] : kBitrateV1L3[bitrate_index];
        out->samples_per_channel = lsf ? 576 : 1152;
        out->frame_bytes = (lsf ? 72u : 144u) * out->bitrate_kbps * 1000u / fs + out->padding;
    }
    if (out->frame_bytes < 4u + (out->has_crc ? 2u : 0u) + 1u) return SK_MP3_NO_SYNC;
    return SK_OK;
}

int scan(const uint8_t *d, size_t len, uint32_t *layer, sk_mpa_frame_info *frames, uint32_t cap, uint32_t *n_frames, size_t *consumed) {
    if (!d || !layer || !n_frames || (cap && !frames) || *layer > 3) return SK_ERR_INVALID_ARG;
    *n_frames = 0;
    uint32_t want = *layer;
    size_t pos = 0;
    if (len >= 10 && d[0] == 'I' && d[1] == 'D' && d[2] == '3' && !((d[6] | d[7] | d[8] | d[9]) & 0x80)) {
        const size_t tag = 10u + (((size_t)d[6] << 21) | ((size_t)d[7] << 14) | ((size_t)d[8] << 7) | d[9]) + ((d[5] & 0x10) ? 10u : 0u);
        if (tag <= len) pos = tag;
    }
    while (pos + 4 <= len) {
        sk_mpa_frame_info h;
        if (parse_header(d + pos, len - pos, &h) != SK_OK || (want && h.layer != want)) {
            ++pos;
            continue;
        }
        const size_t next = pos + h.frame_bytes;
        if (next > len) break;                    // an incomplete frame at the end: needs more input
        if (!want && next + 4 > len) break;       // the stream's first frame must be confirmed by the header behind it
        if (next + 4 <= len) {
            sk_mpa_frame_info follow;
            if (parse_header(d + next, len - next, &follow) != SK_OK || !same_stream(h, follow)) {
                ++pos;
                continue;
            }
        }
        want = h.layer;
        h.offset = (uint32_t)pos;
        if (*n_frames < cap) frames[*n_frames] = h;
        *n_frames += 1;
        pos = next;
    }
    if (consumed) *consumed = pos;
    *layer = want;
    return SK_OK;
}

int find_layer(const uint8_t *d, size_t len) {
    uint32_t layer = 0, n = 0;
    size_t consumed = 0;
    if (!d || scan(d, len, &layer, nullptr, 0, &n, &consumed) != SK_OK) return 0;
    if (layer) return (int)layer;
    sk_mpa_frame_info h;  // the scan stops at a candidate whose frame, or the header behind it, is not in the buffer yet
    if (consumed + 4 <= len && parse_header(d + consumed, len - consumed, &h) == SK_OK) return h.layer == 3 ? -3 : -1;
    return 0;
}

int parse_frame(const uint8_t *frame, size_t len, const sk_mpa_frame_info *h, sk_mpa_frame_record *out) {
    if (!frame || !h || !out) return SK_ERR_INVALID_ARG;
    if (h->layer == 3) return SK_MP3_UNSUPPORTED;
    if (h->layer != 1 && h->layer != 2) return SK_ERR_INVALID_ARG;
    if (h->channels < 1 || h->channels > 2 || h->frame_bytes < 5 || h->frame_bytes > 0xffffu) return SK_ERR_INVALID_ARG;
    if (len < h->frame_bytes) return SK_MP3_NEED_MORE;
    std::memset(out, 0, sizeof *out);
    const int ch = h->channels;
    const AllocTable *table = nullptr;
    int sblimit = 32;
    if (h->layer == 2) {
        table = &kTables[layer2_table(h->version != 1, h->bitrate_kbps, ch, h->sample_rate)];
        sblimit = table->sblimit;
    }
    int bound = h->mode == 1 ? 4 * (h->mode_ext + 1) : sblimit;
    if (bound > sblimit) bound = sblimit;
    if (ch == 1) bound = sblimit;
    out->byte_len = h->frame_bytes;
    out->sample_rate = h->sample_rate;
    out->layer = h->layer;
    out->channels = (uint8_t)ch;
    out->sblimit = (uint8_t)sblimit;
    out->bound = (uint8_t)bound;
    out->granules = 12;

    Bits b{frame, h->frame_bytes};
    b.pos = 32 + (h->has_crc ? 16 : 0);  // the CRC word is stepped over, not verified
    // ---- bit allocation: per channel below the bound, one shared field above it ----
    for (int sb = 0; sb < sblimit; ++sb)
        for (int c = 0; c < (sb < bound ? ch : 1); ++c) {
            uint8_t cls = 0;
            if (h->layer == 1) {
                const uint32_t a = b.get(4);
                if (a == 15) return SK_MP3_INVALID;  // forbidden
                cls = a ? (uint8_t)(a + 1) : 0;
            } else {
                const AllocRow &row = kRows[table->row[sb]];
                const uint32_t a = b.get(row.bits);
                cls = a ? class_of_steps(row.steps[a - 1]) : 0;
            }
            out->cls[c][sb] = cls;
            if (sb >= bound && ch == 2) out->cls[1][sb] = cls;
        }
    // ---- scale factors: each channel its own, above the bound too ----
    if (h->layer == 1) {
        for (int sb = 0; sb < sblimit; ++sb)
            for (int c = 0; c < ch; ++c)
                if (out->cls[c][sb]) {
                    const uint8_t f = (uint8_t)b.get(6);
                    out->scf[c][sb][0] = out->scf[c][sb][1] = out->scf[c][sb][2] = f;
                }
    } else {
        uint8_t scfsi[2][32] = {};
        for (int sb = 0; sb < sblimit; ++sb)
            for (int c = 0; c < ch; ++c)
                if (out->cls[c][sb]) scfsi[c][sb] = (uint8_t)b.get(2);
        for (int sb = 0; sb < sblimit; ++sb)
            for (int c = 0; c < ch; ++c) {
                if (!out->cls[c][sb]) continue;
                uint8_t *f = out->scf[c][sb];
                switch (scfsi[c][sb]) {
                case 0: f[0] = (uint8_t)b.get(6), f[1] = (uint8_t)b.get(6), f[2] = (uint8_t)b.get(6); break;
                case 1: f[0] = f[1] = (uint8_t)b.get(6), f[2] = (uint8_t)b.get(6); break;
                case 2: f[0] = f[1] = f[2] = (uint8_t)b.get(6); break;
                default: f[0] = (uint8_t)b.get(6), f[1] = f[2] = (uint8_t)b.get(6); break;
                }
            }
    }
    // ---- the samples: where they start and how wide a granule (slot) is ----
    uint32_t width = 0;
    for (int sb = 0; sb < sblimit; ++sb)
        for (int c = 0; c < (sb < bound ? ch : 1); ++c) width += (uint32_t)class_bits(h->layer, out->cls[c][sb]);
    out->sample_bit = (uint32_t)b.pos;
    out->granule_bits = (uint16_t)width;
    if (b.pos + (size_t)12 * width > (size_t)h->frame_bytes * 8) return SK_MP3_INVALID;  // the samples would end beyond the frame
    return SK_OK;
}

bool record_adds_up(const sk_mpa_frame_record &r) {
    if (r.layer != 1 && r.layer != 2) return false;
    if (r.channels < 1 || r.channels > 2 || r.sblimit > 32 || r.bound > r.sblimit || r.granules != 12) return false;
    if (r.channels == 1 && r.bound != r.sblimit) return false;
    uint32_t width = 0;
    for (int c = 0; c < 2; ++c)
        for (int sb = 0; sb < 32; ++sb) {
            const uint8_t cls = r.cls[c][sb];
            if ((c >= r.channels || sb >= r.sblimit) && cls) return false;
            const int bits = class_bits(r.layer, cls);
            if (bits < 0) return false;
            if (c == 1 && sb >= r.bound) {
                if (cls != r.cls[0][sb]) return false;  // the shared code has one class
            } else {
                width += (uint32_t)bits;
            }
            for (int k = 0; k < 3; ++k)
                if (r.scf[c][sb][k] > 63) return false;
        }
    if (width != r.granule_bits) return false;
    return (uint64_t)r.sample_bit + 12ull * width <= (uint64_t)r.byte_len * 8;
}

}  // namespace sk_mp12

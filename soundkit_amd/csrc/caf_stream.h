// caf_stream.h -- Core Audio Format on the host, for the formats built here: the chunk walk of a whole file and the packet index of its
// `data` chunk for `lpcm` and `alac` descriptions (CafAudioIndex, soundkit-audio-demux/src/caf.rs: from_file 138-197, from_metadata
// 201-328, parse_description 403-433, parse_packet_table 435-497, resolve_packet_sizes 499-556, resolve_format 560-614; their texts).
// Serial byte parsing, no per-sample work, no HIP; header-only.  The input is untrusted: every read is bounds-checked and every count is
// checked against the bytes that hold it before anything is reserved.  alac_stream.h keeps the ALAC-only index that came before this one.
//
// Two things are this project's own.  An `lpcm` frame padded beyond channels x ceil(bits / 8) bytes is refused (the reference marks it
// unpacked and then reads it as packed).  And an `lpcm` file's packets -- one frame each in what FFmpeg writes -- leave as runs of whole
// packets of at most kMaxRunFrames frames and kMaxRunBytes bytes, so no record per frame is made and the packet budget counts runs.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace sk_caf {

constexpr uint64_t kMaxDescriptionBytes = 32, kMaxCookieBytes = 1024 * 1024, kMaxPacketTableBytes = 64ull * 1024 * 1024, kMaxLayoutBytes = 1024 * 1024;
constexpr uint64_t kMaxPackets = 8000000;            // MAX_CAF_MATERIALIZED_PACKETS
constexpr uint32_t kMaxPacketBytes = 128u * 1024 * 1024;  // MAX_CAF_PACKET_BYTES
constexpr uint32_t kMaxRunFrames = 4096, kMaxRunBytes = 1024 * 1024;
constexpr uint8_t kCodecAlac = 1, kCodecPcm = 2;

inline uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
inline uint64_t be64(const uint8_t *p) { return (uint64_t)be32(p) << 32 | be32(p + 4); }

struct Packet {
    uint64_t offset = 0, start = 0;  // absolute byte offset; the first frame's place on the file's timeline
    uint32_t size = 0, frames = 0;
};

struct Index {
    uint8_t codec = 0;  // kCodecAlac / kCodecPcm
    char format_id[4] = {0, 0, 0, 0};
    uint32_t sample_rate = 0, channels = 0, bits = 0, format_flags = 0;
    uint32_t bytes_per_packet = 0, frames_per_packet = 0;  // the description's
    bool big_endian = false, is_float = false;             // lpcm
    uint32_t bytes_per_frame = 0;                          // lpcm
    uint64_t valid_frames = 0;
    uint32_t priming_frames = 0, remainder_frames = 0;
    std::vector<uint8_t> cookie;
    std::vector<Packet> packets;  // alac: the file's packets; lpcm: runs of them
};

struct PacketTable {
    uint64_t count = 0, valid_frames = 0;
    uint32_t priming_frames = 0, remainder_frames = 0;
    std::vector<uint32_t> sizes;
};

inline std::string name_of(const uint8_t *p) {
    std::string s;
    for (int i = 0; i < 4; ++i) s += (p[i] >= 0x20 && p[i] < 0x7f) ? (char)p[i] : '?';
    return s;
}

// parse_packet_table
inline bool parse_packet_table(const uint8_t *d, size_t len, PacketTable *t, std::string *error) {
    if (len < 24) return *error = "CAF packet table is shorter than 24 bytes", false;
    const int64_t count = (int64_t)be64(d), valid = (int64_t)be64(d + 8);
    const int32_t priming = (int32_t)be32(d + 16), remainder = (int32_t)be32(d + 20);
    if (count < 0 || valid < 0 || priming < 0 || remainder < 0) return *error = "CAF packet table contains a negative count", false;
    if ((uint64_t)count > kMaxPackets) return *error = "CAF packet count exceeds the " + std::to_string(kMaxPackets) + " packet index budget", false;
    if ((uint64_t)count > len - 24) return *error = "CAF packet count exceeds its variable-length table", false;
    t->sizes.clear();
    t->sizes.reserve((size_t)count);
    size_t at = 24;
    while (at < len) {
        if (t->sizes.size() == (size_t)count) return *error = "CAF packet table has trailing bytes", false;
        uint64_t v = 0;
        bool complete = false;
        for (int i = 0; i < 10; ++i) {
            if (at >= len) return *error = "CAF packet size VLQ is truncated", false;
            const uint8_t byte = d[at++];
            if (v >> 57) return *error = "CAF packet size VLQ overflows u64", false;
            v = v << 7 | (byte & 0x7fu);
            if (!(byte & 0x80u)) {
                complete = true;
                break;
            }
        }
        if (!complete) return *error = "CAF packet size VLQ exceeds 10 bytes", false;
        if (v == 0 || v > kMaxPacketBytes) return *error = "CAF packet size " + std::to_string(v) + " exceeds its budget", false;
        t->sizes.push_back((uint32_t)v);
    }
    t->count = (uint64_t)count, t->valid_frames = (uint64_t)valid, t->priming_frames = (uint32_t)priming, t->remainder_frames = (uint32_t)remainder;
    return true;
}

// CafAudioIndex::from_metadata.  pakt == nullptr: the file holds no packet table
inline bool index_from_metadata(const uint8_t *desc, size_t desc_len, const uint8_t *cookie, size_t cookie_len, const uint8_t *pakt, size_t pakt_len,
                                uint64_t data_offset, uint64_t data_size, Index *ix, std::string *error) {
    if (data_size < 4) return *error = "CAF data chunk is shorter than its edit count", false;
    if (cookie_len > kMaxCookieBytes || (pakt && pakt_len > kMaxPacketTableBytes)) return *error = "CAF metadata exceeds its bounded read budget", false;
    // parse_description
    if (desc_len != 32) return *error = "CAF desc must contain 32 bytes, got " + std::to_string(desc_len), false;
    const uint64_t rate_bits = be64(desc);
    double rate;
    std::memcpy(&rate, &rate_bits, 8);
    if (!std::isfinite(rate) || rate <= 0.0 || rate > 4294967295.0 || rate != std::floor(rate)) {
        char text[64];
        std::snprintf(text, sizeof text, "invalid CAF sample rate: %g", rate);
        return *error = text, false;
    }
    const uint32_t channels = be32(desc + 24), bits = be32(desc + 28);
    if (channels < 1 || channels > 255) return *error = "CAF channel count is outside 1...255", false;
    if (bits > 255) return *error = "CAF bits per channel exceeds 255", false;
    *ix = Index{};
    ix->sample_rate = (uint32_t)rate, ix->channels = channels, ix->bits = bits;
    std::memcpy(ix->format_id, desc + 8, 4);
    ix->format_flags = be32(desc + 12), ix->bytes_per_packet = be32(desc + 16), ix->frames_per_packet = be32(desc + 20);
    if (data_offset > UINT64_MAX - 4) return *error = "CAF packet offset overflows u64", false;
    const uint64_t packet_start = data_offset + 4, packet_bytes = data_size - 4;
    if (packet_start > UINT64_MAX - packet_bytes) return *error = "CAF chunk range overflows u64", false;
    PacketTable table;
    if (pakt && !parse_packet_table(pakt, pakt_len, &table, error)) return false;
    // resolve_packet_sizes
    const uint32_t bpp = ix->bytes_per_packet, fpp = ix->frames_per_packet;
    if (fpp == 0) return *error = "CAF frames per packet is zero", false;
    uint64_t count;
    if (bpp == 0) {
        if (!pakt) return *error = "variable-packet CAF source is missing its pakt chunk", false;
        if (table.sizes.size() != table.count) return *error = "CAF variable packet table omits packet sizes", false;
        uint64_t described = 0;
        for (const uint32_t s : table.sizes) described += s;  // at most 8 000 000 x 128 MiB
        if (described != packet_bytes)
            return *error = "CAF packet table describes " + std::to_string(described) + " bytes, data contains " + std::to_string(packet_bytes), false;
        count = table.count;
    } else {
        if (bpp > kMaxPacketBytes) return *error = "CAF packet size " + std::to_string(bpp) + " exceeds its budget", false;
        if (packet_bytes % bpp != 0) return *error = "CAF constant packet size does not divide the data chunk", false;
        count = packet_bytes / bpp;
        if (pakt) {
            if (table.count != count) return *error = "CAF packet table count disagrees with constant packet data", false;
            if (!table.sizes.empty()) return *error = "CAF constant packet table unexpectedly contains packet sizes", false;
        }
    }
    if (count > UINT64_MAX / fpp) return *error = "CAF packet frame count overflows u64", false;
    const uint64_t total_frames = count * fpp;
    if (pakt) {
        const uint64_t accounted = table.valid_frames + table.priming_frames + table.remainder_frames;
        if (accounted < table.valid_frames) return *error = "CAF packet-table frame counts overflow u64", false;
        if (accounted > total_frames) return *error = "CAF packet-table frame counts exceed packet capacity", false;
        ix->valid_frames = table.valid_frames, ix->priming_frames = table.priming_frames, ix->remainder_frames = table.remainder_frames;
    } else {
        ix->valid_frames = total_frames;
    }
    // resolve_format
    if (std::memcmp(ix->format_id, "lpcm", 4) == 0) {
        if (bits == 0) return *error = "CAF LPCM bits per channel is zero", false;
        ix->is_float = (ix->format_flags & 1u) != 0, ix->big_endian = (ix->format_flags & 2u) == 0;
        if (ix->is_float && bits != 32 && bits != 64) return *error = "CAF float PCM must use 32-bit or 64-bit samples", false;
        if (bpp == 0) return *error = "CAF LPCM requires a constant packet size", false;
        ix->bytes_per_frame = bpp / fpp;
        if (ix->bytes_per_frame == 0 || bpp % fpp != 0) return *error = "CAF LPCM packet geometry is not frame-aligned", false;
        const uint32_t minimum = (bits + 7) / 8 * channels;
        if (ix->bytes_per_frame < minimum) return *error = "CAF LPCM bytes per frame cannot hold its channels", false;
        if (ix->bytes_per_frame > minimum) return *error = "CAF LPCM frames padded beyond their channels are unsupported", false;
        ix->codec = kCodecPcm;
    } else if (std::memcmp(ix->format_id, "alac", 4) == 0) {
        ix->codec = kCodecAlac;
    } else {
        return *error = "unsupported CAF audio format " + name_of(desc + 8), false;
    }
    ix->cookie.assign(cookie, cookie + cookie_len);
    // the packets: as the file cuts them, or for lpcm in runs of whole packets
    uint64_t offset = packet_start, start = 0;
    if (ix->codec == kCodecPcm) {
        const uint64_t per_run = std::max<uint64_t>(1, std::min<uint64_t>(kMaxRunFrames / fpp, kMaxRunBytes / bpp));
        const uint64_t runs = (count + per_run - 1) / per_run;
        if (runs > kMaxPackets) return *error = "CAF packet count exceeds the " + std::to_string(kMaxPackets) + " packet index budget", false;
        ix->packets.reserve((size_t)runs);
        for (uint64_t left = count; left > 0;) {
            const uint64_t n = std::min(left, per_run);  // n x bpp <= max(1 MiB, 128 MiB), n x fpp <= max(4096, 2^32 - 1)
            Packet p;
            p.offset = offset, p.start = start, p.size = (uint32_t)(n * bpp), p.frames = (uint32_t)(n * fpp);
            ix->packets.push_back(p);
            offset += n * bpp, start += n * fpp, left -= n;
        }
    } else {
        if (count > kMaxPackets) return *error = "CAF packet count exceeds the " + std::to_string(kMaxPackets) + " packet index budget", false;
        ix->packets.reserve((size_t)count);
        for (uint64_t k = 0; k < count; ++k) {
            Packet p;
            p.offset = offset, p.start = start, p.size = bpp ? bpp : table.sizes[(size_t)k], p.frames = fpp;
            ix->packets.push_back(p);
            offset += p.size, start += fpp;
        }
    }
    if (offset != packet_start + packet_bytes) return *error = "CAF packet ranges do not cover the data chunk", false;
    return true;
}

// CafAudioIndex::from_file: `caff`, version 1, flags 0, then chunks of a 4-byte type and a signed 64-bit size (-1 on the data chunk alone)
inline bool index_from_file(const uint8_t *d, size_t len, Index *ix, std::string *error) {
    if (len < 8) return *error = "CAF source ends before its 8-byte file header", false;
    if (std::memcmp(d, "caff", 4) != 0) return *error = "CAF source does not start with caff", false;
    const uint32_t version = (uint32_t)d[4] << 8 | d[5], flags = (uint32_t)d[6] << 8 | d[7];
    if (version != 1 || flags != 0) return *error = "unsupported CAF header version=" + std::to_string(version) + " flags=" + std::to_string(flags), false;
    struct Found {
        const uint8_t *p = nullptr;
        uint64_t at = 0, size = 0;
        bool have = false;
    } desc, kuki, pakt, chan, data;
    size_t at = 8;
    while (at < len) {
        if (len - at < 12) return *error = "CAF source ends before a chunk header", false;
        const uint8_t *h = d + at;
        const int64_t stated = (int64_t)be64(h + 4);
        const bool is_data = std::memcmp(h, "data", 4) == 0;
        at += 12;
        uint64_t size;
        if (stated == -1 && is_data) size = len - at;
        else if (stated == -1) return *error = "CAF chunk " + name_of(h) + " cannot have an unknown size", false;
        else if (stated < 0) return *error = "CAF chunk has invalid negative size " + std::to_string(stated), false;
        else size = (uint64_t)stated;
        if (size > len - at) return *error = "CAF chunk " + name_of(h) + " exceeds the source length", false;
        Found *f = std::memcmp(h, "desc", 4) == 0 ? &desc : std::memcmp(h, "kuki", 4) == 0 ? &kuki : std::memcmp(h, "pakt", 4) == 0 ? &pakt :
                   std::memcmp(h, "chan", 4) == 0 ? &chan : is_data ? &data : nullptr;
        const uint64_t budget = f == &desc ? kMaxDescriptionBytes : f == &kuki ? kMaxCookieBytes : f == &pakt ? kMaxPacketTableBytes : f == &chan ? kMaxLayoutBytes : 0;
        if (budget && size > budget) return *error = "CAF chunk " + name_of(h) + " exceeds the " + std::to_string(budget) + " byte metadata budget", false;
        if (f) {
            if (f->have) return *error = "CAF source contains multiple " + name_of(h) + " chunks", false;
            f->p = d + at, f->at = at, f->size = size, f->have = true;
        }
        at += (size_t)size;
    }
    if (!desc.have) return *error = "CAF source is missing its desc chunk", false;
    if (!data.have) return *error = "CAF source is missing its data chunk", false;
    static const uint8_t none[1] = {0};
    return index_from_metadata(desc.p, (size_t)desc.size, kuki.have ? kuki.p : none, kuki.have ? (size_t)kuki.size : 0, pakt.have ? pakt.p : nullptr,
                               pakt.have ? (size_t)pakt.size : 0, data.at, data.size, ix, error);
}

}  // namespace sk_caf

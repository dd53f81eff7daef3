// alac_stream.h -- Apple Lossless on the host: the magic cookie in its three wrappings, the frame count of a packet, and the packet
// index of an ALAC CAF file (CafAlacPacketIndex, soundkit-alac/src/lib.rs:38-215, check for check).  No per-sample work, no HIP;
// header-only.
//
// A packet is a sequence of elements, each with a 3-bit tag: 0 SCE (one channel), 1 CPE (two), 3 LFE (one), 4 DSE and 6 FIL (stepped
// over by their own length fields), 2 CCE and 5 PCE (the packet is rejected), 7 END.  Channels leave in bitstream order: whether the
// reference's codec reorders the elements of a stream with more than two channels into a speaker layout could not be read from its
// source, so no reordering is done here or on the device.  The host reads only the first audio element's header (packet_frames), so
// that a packet's place in the output is known before the device decodes it; the device rejects a packet whose elements disagree.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/soundkit_amd.h"

namespace sk_alac {

constexpr uint32_t kMaxFramesPerPacket = 65536;
constexpr uint32_t kMaxPacketBytes = 16u * 1024 * 1024;
constexpr uint32_t kMaxChannels = 8;

inline uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
inline uint64_t be64(const uint8_t *p) { return (uint64_t)be32(p) << 32 | be32(p + 4); }

// validate_stream_info (lib.rs:302-324)
inline bool validate(const sk_alac_config &c, std::string *error) {
    if (c.sample_rate == 0) return *error = "ALAC stream reports a zero sample rate", false;
    if (c.channels < 1 || c.channels > kMaxChannels)
        return *error = "ALAC channel count " + std::to_string(c.channels) + " exceeds the supported range 1-8", false;
    if (c.bit_depth != 16 && c.bit_depth != 24 && c.bit_depth != 32) return *error = "Unsupported ALAC bit depth: " + std::to_string(c.bit_depth), false;
    if (c.frame_length == 0 || c.frame_length > kMaxFramesPerPacket)
        return *error = "ALAC frame length " + std::to_string(c.frame_length) + " exceeds the 1-65536 frame budget", false;
    return true;
}

// bare config | four zero bytes + config (the MP4 `alac` FullBox payload) | `frma` atom + `alac` atom (QuickTime, what a CAF kuki holds)
inline bool parse_cookie(const uint8_t *d, size_t len, sk_alac_config *out, std::string *error) {
    if (len >= 48 && std::memcmp(d + 4, "frma", 4) == 0 && std::memcmp(d + 16, "alac", 4) == 0) d += 24, len -= 24;
    else if (len >= 28 && be32(d) == 0) d += 4, len -= 4;
    if (len < 24) return *error = "ALAC magic cookie is shorter than 24 bytes", false;
    sk_alac_config c{};
    c.frame_length = be32(d);
    c.compatible_version = d[4], c.bit_depth = d[5], c.pb = d[6], c.mb = d[7], c.kb = d[8], c.channels = d[9];
    c.max_run = (uint16_t)(d[10] << 8 | d[11]);
    c.max_frame_bytes = be32(d + 12), c.avg_bit_rate = be32(d + 16), c.sample_rate = be32(d + 20);
    if (!validate(c, error)) return false;
    *out = c;
    return true;
}

// bits of a packet, most significant first; reads past the end give zeros and set `over`
struct Bits {
    const uint8_t *d;
    uint64_t pos, end;
    bool over;
    Bits(const uint8_t *data, size_t len) : d(data), pos(0), end((uint64_t)len * 8), over(false) {}
    uint32_t read(uint32_t n) {  // 0 ... 32
        uint32_t v = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t p = pos + i;
            v = v << 1 | (p < end ? (d[p >> 3] >> (7 - (p & 7)) & 1u) : 0u);
        }
        skip(n);
        return v;
    }
    void skip(uint64_t n) {
        pos += n;
        over |= pos > end;
    }
};

inline void skip_dse(Bits &b) {
    b.skip(4);
    const uint32_t align = b.read(1);
    uint32_t count = b.read(8);
    if (count == 255) count += b.read(8);
    if (align) b.skip((8 - (b.pos & 7)) & 7);
    b.skip(8ull * count);
}

inline void skip_fil(Bits &b) {
    uint32_t count = b.read(4);
    if (count == 15) count += b.read(8) - 1;
    b.skip(8ull * count);
}

inline int packet_frames(const sk_alac_config &c, const uint8_t *packet, size_t len, uint32_t *frames) {
    Bits b(packet, len);
    while (!b.over) {
        const uint32_t tag = b.read(3);
        if (tag == 0 || tag == 1 || tag == 3) {
            b.skip(16);
            const uint32_t has_size = b.read(1);
            b.skip(3);
            const uint32_t n = has_size ? b.read(32) : c.frame_length;
            if (b.over || n == 0 || n > c.frame_length) return SK_ALAC_INVALID;
            *frames = n;
            return SK_OK;
        }
        if (tag == 4) skip_dse(b);
        else if (tag == 6) skip_fil(b);
        else if (tag == 2 || tag == 5) return b.over ? SK_ALAC_INVALID : SK_ALAC_UNSUPPORTED;
        else break;
    }
    return SK_ALAC_INVALID;
}

struct PacketRange {
    uint64_t offset;
    uint32_t size;
};

struct CafIndex {
    sk_alac_config config{};
    uint64_t valid_frames = 0;
    uint32_t priming_frames = 0, remainder_frames = 0, frames_per_packet = 0;
    std::vector<PacketRange> packets;
};

inline bool parse_packet_table(const uint8_t *d, size_t len, CafIndex *ix, std::vector<uint32_t> *sizes, std::string *error) {
    if (len < 24) return *error = "CAF packet table is shorter than 24 bytes", false;
    const int64_t count = (int64_t)be64(d), valid = (int64_t)be64(d + 8);
    const int32_t priming = (int32_t)be32(d + 16), remainder = (int32_t)be32(d + 20);
    if (count < 0 || valid < 0 || priming < 0 || remainder < 0) return *error = "CAF packet table contains a negative count", false;
    if ((uint64_t)count > len - 24) return *error = "CAF packet count exceeds its variable-length table", false;
    size_t at = 24;
    sizes->reserve((size_t)count);
    for (int64_t k = 0; k < count; ++k) {
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
        if (v > 0xffffffffull) return *error = "CAF packet size exceeds the u32 range", false;
        sizes->push_back((uint32_t)v);
    }
    if (at != len) return *error = "CAF packet table has trailing bytes", false;
    ix->valid_frames = (uint64_t)valid, ix->priming_frames = (uint32_t)priming, ix->remainder_frames = (uint32_t)remainder;
    return true;
}

// CafAlacPacketIndex::new
inline bool caf_index(const uint8_t *desc, size_t desc_len, const uint8_t *cookie, size_t cookie_len, const uint8_t *pakt, size_t pakt_len,
                      uint64_t data_offset, uint64_t data_size, CafIndex *ix, std::string *error) {
    if (desc_len != 32) return *error = "CAF desc must contain 32 bytes, got " + std::to_string(desc_len), false;
    uint64_t rate_bits = be64(desc);
    double rate_value;
    std::memcpy(&rate_value, &rate_bits, 8);
    if (std::memcmp(desc + 8, "alac", 4) != 0) return *error = "CAF audio description is not ALAC", false;
    const uint32_t bytes_per_packet = be32(desc + 16), frames_per_packet = be32(desc + 20), channels = be32(desc + 24), bits = be32(desc + 28);
    if (!std::isfinite(rate_value) || rate_value <= 0.0 || rate_value > 4294967295.0) {
        char text[64];
        std::snprintf(text, sizeof text, "invalid CAF sample rate: %g", rate_value);
        return *error = text, false;
    }
    const uint32_t rate = (uint32_t)std::llround(rate_value);
    if (channels < 1 || channels > kMaxChannels) return *error = "CAF ALAC channel count exceeds the supported range", false;
    if (data_size < 4) return *error = "CAF data chunk is shorter than its edit count", false;
    const uint64_t packet_bytes = data_size - 4;
    if (data_offset > UINT64_MAX - 4) return *error = "CAF packet offset overflow", false;
    const uint64_t packet_start = data_offset + 4;
    if (!parse_cookie(cookie, cookie_len, &ix->config, error)) return false;
    const sk_alac_config &c = ix->config;
    if (c.sample_rate != rate || c.channels != channels || (bits != 0 && c.bit_depth != bits))
        return *error = "CAF desc and ALAC magic cookie disagree", false;
    if (frames_per_packet == 0 || frames_per_packet > kMaxFramesPerPacket)
        return *error = "CAF ALAC frames-per-packet " + std::to_string(frames_per_packet) + " exceeds the decoder budget", false;
    ix->frames_per_packet = frames_per_packet;
    std::vector<uint32_t> sizes;
    if (bytes_per_packet == 0) {
        if (!parse_packet_table(pakt, pakt_len, ix, &sizes, error)) return false;
    } else {
        if (packet_bytes % bytes_per_packet != 0) return *error = "CAF constant packet size does not divide the data chunk", false;
        const uint64_t count = packet_bytes / bytes_per_packet;
        if (count > UINT64_MAX / frames_per_packet) return *error = "CAF valid frame count overflow", false;
        if (count > (1ull << 28)) return *error = "CAF packet count exceeds this platform", false;
        ix->valid_frames = count * frames_per_packet;
        ix->priming_frames = ix->remainder_frames = 0;
        if (bytes_per_packet > kMaxPacketBytes) return *error = "CAF ALAC packet size " + std::to_string(bytes_per_packet) + " exceeds its budget", false;
        sizes.assign((size_t)count, bytes_per_packet);
    }
    uint64_t offset = packet_start;
    ix->packets.clear();
    ix->packets.reserve(sizes.size());
    for (const uint32_t size : sizes) {
        if (size == 0 || size > kMaxPacketBytes) return *error = "CAF ALAC packet size " + std::to_string(size) + " exceeds its budget", false;
        ix->packets.push_back({offset, size});
        if (offset > UINT64_MAX - size) return *error = "CAF packet range overflow", false;
        offset += size;
    }
    if (packet_start > UINT64_MAX - packet_bytes) return *error = "CAF data range overflow", false;
    if (offset != packet_start + packet_bytes)
        return *error = "CAF packet table describes " + std::to_string(offset - packet_start) + " bytes, data contains " + std::to_string(packet_bytes), false;
    return true;
}

// a whole CAF file: `caff`, version 1, then chunks of a 4-byte type and a signed 64-bit size (-1 on the data chunk: to the end)
inline bool caf_index_from_file(const uint8_t *d, size_t len, CafIndex *ix, std::string *error) {
    if (len < 8 || std::memcmp(d, "caff", 4) != 0) return *error = "not a CAF file", false;
    if ((d[4] << 8 | d[5]) != 1) return *error = "unsupported CAF version", false;
    struct Found {
        const uint8_t *p = nullptr;
        uint64_t at = 0, size = 0;
        bool have = false;
    } desc, kuki, pakt, data;
    size_t at = 8;
    while (at < len) {
        if (len - at < 12) return *error = "CAF chunk header is truncated", false;
        const uint8_t *h = d + at;
        const int64_t stated = (int64_t)be64(h + 4);
        at += 12;
        uint64_t size;
        if (stated < 0) {
            if (stated != -1 || std::memcmp(h, "data", 4) != 0) return *error = "CAF chunk has a negative size", false;
            size = len - at;
        } else {
            size = (uint64_t)stated;
        }
        if (size > len - at) return *error = "CAF chunk extends past the source", false;
        Found *f = std::memcmp(h, "desc", 4) == 0 ? &desc : std::memcmp(h, "kuki", 4) == 0 ? &kuki : std::memcmp(h, "pakt", 4) == 0 ? &pakt :
                   std::memcmp(h, "data", 4) == 0 ? &data : nullptr;
        if (f) {
            if (f->have) return *error = "CAF source contains multiple " + std::string((const char *)h, 4) + " chunks", false;
            f->p = d + at, f->at = at, f->size = size, f->have = true;
        }
        at += (size_t)size;
    }
    if (!desc.have) return *error = "CAF source has no desc chunk", false;
    if (!kuki.have) return *error = "CAF source has no kuki chunk", false;
    if (!data.have) return *error = "CAF source has no data chunk", false;
    static const uint8_t none[1] = {0};
    return caf_index(desc.p, (size_t)desc.size, kuki.p, (size_t)kuki.size, pakt.have ? pakt.p : none, pakt.have ? (size_t)pakt.size : 0, data.at, data.size,
                     ix, error);
}

}  // namespace sk_alac

// ogg_stream.h -- the incremental Ogg page and packet parser (host only): OggPacketParser of soundkit/src/ogg.rs with its budgets, its
// checks and its error texts.  One logical stream; pages are CRC-checked, packets may continue across pages.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <deque>
#include <string>
#include <vector>

namespace sk_ogg {

constexpr size_t kMaxInputChunkBytes = 4u * 1024 * 1024;
constexpr size_t kMaxPacketBytes = 16u * 1024 * 1024;
constexpr size_t kMaxBufferBytes = kMaxPacketBytes + 64 * 1024;

struct Packet {
    std::vector<uint8_t> data;
    uint32_t serial = 0;
    bool first_in_stream = false, last_in_page = false, last_in_stream = false, has_granule = false;
    uint64_t granule_position = 0;
};

struct CrcTable {
    uint32_t v[256];
    constexpr CrcTable() : v{} {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i << 24;
            for (int k = 0; k < 8; ++k) c = (c & 0x80000000u) ? (c << 1) ^ 0x04C11DB7u : c << 1;
            v[i] = c;
        }
    }
};
inline constexpr CrcTable kCrcTable{};  // made at compile time: the parser runs on several threads

// ogg_page_crc: polynomial 0x04C11DB7, no reflection, zero start; the checksum field (bytes 22..25) counts as zero
inline uint32_t page_crc(const uint8_t *page, size_t len) {
    const uint32_t *t = kCrcTable.v;
    uint32_t crc = 0;
    for (size_t i = 0; i < len; ++i) {
        const uint8_t b = (i >= 22 && i < 26) ? 0 : page[i];
        crc = (crc << 8) ^ t[(crc >> 24) ^ b];
    }
    return crc;
}

class Parser {
  public:
    std::deque<Packet> pending;

    // false: refused, *error says why (the parser is then of no further use, as the reference's after an Err)
    bool add(const uint8_t *data, size_t len, std::string *error) {
        if (len > kMaxInputChunkBytes) return fail(error, "Ogg input chunk exceeds the " + std::to_string(kMaxInputChunkBytes) + " byte streaming budget");
        if (buffer_.size() + len > kMaxBufferBytes) return fail(error, "Ogg input buffer exceeds the " + std::to_string(kMaxBufferBytes) + " byte budget");
        buffer_.insert(buffer_.end(), data, data + len);
        return parse_available(error);
    }

    bool finish(std::string *error) {
        if (!parse_available(error)) return false;
        if (!packet_.empty()) return fail(error, "truncated Ogg packet at end of input");
        if (buffer_.size() != cursor_) return fail(error, "truncated Ogg page: " + std::to_string(buffer_.size() - cursor_) + " bytes remain");
        if (have_serial_ && !seen_eos_) return fail(error, "Ogg logical stream is missing EOS");
        return true;
    }

  private:
    std::vector<uint8_t> buffer_, packet_;
    size_t cursor_ = 0;
    bool have_serial_ = false, have_sequence_ = false, seen_eos_ = false, have_granule_ = false;
    uint32_t serial_ = 0, next_sequence_ = 0;
    uint64_t last_granule_ = 0;

    static bool fail(std::string *error, const std::string &text) {
        if (error) *error = text;
        return false;
    }

    bool parse_available(std::string *error) {
        for (;;) {
            const size_t remaining = buffer_.size() - cursor_;
            if (remaining < 27) break;
            const uint8_t *p = buffer_.data() + cursor_;
            if (memcmp(p, "OggS", 4) != 0) return fail(error, "invalid Ogg capture pattern at byte " + std::to_string(cursor_));
            const uint8_t version = p[4], header_type = p[5];
            uint64_t granule = 0;
            for (int i = 7; i >= 0; --i) granule = granule << 8 | p[6 + i];
            const uint32_t serial = rd32(p + 14), sequence = rd32(p + 18), checksum = rd32(p + 22);
            const size_t segments = p[26], header_size = 27 + segments;
            if (remaining < header_size) break;
            size_t body_size = 0;
            for (size_t i = 0; i < segments; ++i) body_size += p[27 + i];
            const size_t total = header_size + body_size;
            if (remaining < total) break;
            const bool continued = header_type & 1, bos = header_type & 2, eos = header_type & 4;
            // validate_page
            if (version != 0) return fail(error, "unsupported Ogg page version " + std::to_string(version));
            if (page_crc(p, total) != checksum) return fail(error, "Ogg CRC mismatch on page " + std::to_string(sequence));
            if (!have_serial_) {
                if (!bos || sequence != 0) return fail(error, "Ogg logical stream does not begin with BOS page zero");
                have_serial_ = true, serial_ = serial;
            } else if (serial_ != serial) {
                return fail(error, "chained or multiplexed Ogg streams are unsupported");
            } else if (bos) {
                return fail(error, "Ogg BOS flag appears after the first page");
            }
            if (seen_eos_) return fail(error, "Ogg page appears after EOS");
            if (have_sequence_ && sequence != next_sequence_)
                return fail(error, "Ogg page sequence discontinuity: expected " + std::to_string(next_sequence_) + ", got " + std::to_string(sequence));
            have_sequence_ = true, next_sequence_ = sequence + 1;
            if (granule != UINT64_MAX) {
                if (have_granule_ && granule < last_granule_) return fail(error, "Ogg granule position moved backwards");
                have_granule_ = true, last_granule_ = granule;
            }
            if (continued == packet_.empty())
                return fail(error, continued ? "Ogg continued-packet flag has no preceding packet" : "Ogg packet continuation is missing its continued flag");
            // lacing
            size_t at = header_size, completed = 0;
            for (size_t i = 0; i < segments; ++i) {
                const size_t size = p[27 + i];
                if (packet_.size() + size > kMaxPacketBytes) return fail(error, "Ogg packet exceeds the " + std::to_string(kMaxPacketBytes) + " byte packet budget");
                packet_.insert(packet_.end(), p + at, p + at + size);
                at += size;
                if (size < 255) {
                    Packet k;
                    k.data.swap(packet_);
                    k.serial = serial, k.first_in_stream = bos;
                    pending.push_back(std::move(k));
                    ++completed;
                }
            }
            if (completed) {
                Packet &last = pending.back();
                last.last_in_page = true, last.last_in_stream = eos;
                last.has_granule = granule != UINT64_MAX, last.granule_position = last.has_granule ? granule : 0;
            }
            if (eos) {
                if (!packet_.empty() || !completed) return fail(error, "Ogg EOS page does not end with a complete packet");
                if (granule == UINT64_MAX) return fail(error, "Ogg EOS page has no final granule position");
                seen_eos_ = true;
            }
            cursor_ += total;
        }
        if (cursor_ > 64 * 1024 || cursor_ == buffer_.size()) {
            buffer_.erase(buffer_.begin(), buffer_.begin() + (ptrdiff_t)cursor_);
            cursor_ = 0;
        }
        return true;
    }

    static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
};

}  // namespace sk_ogg

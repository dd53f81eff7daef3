// flac_stream.h -- FLAC (RFC 9639) on the host: frame-header parser, framer and incremental stream reader.  No per-sample work, no
// HIP; header-only.
//
// A FLAC frame carries no length.  It ends where the next valid header begins AND the CRC-16 over the span holds: the 14-bit sync code
// turns up inside payloads, now and then with a fitting CRC-8, so a header alone is no boundary (scan()).  The search for the end is
// bounded -- a frame is never longer than
//     STREAMINFO.max_framesize                                                          when STREAMINFO gives one, else
//     19 + ceil((block_size * channels * (bits + 1) + channels * 40) / 8) bytes
// i.e. the longest header (16), the CRC-16 (2) and a byte of padding, around subframes that are all VERBATIM at a side channel's
// width (bits + 1), each with its header byte (8 bits) and the longest wasted-bits count (32 bits).  An encoder has no reason to write
// a subframe longer than its VERBATIM form.  When no span within the bound satisfies the CRC-16 the stream is in error: FLAC is
// lossless, a lost frame is not skipped silently.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/soundkit_amd.h"

namespace sk_flac {

uint8_t crc8(const uint8_t *d, size_t n);                  // x^8 + x^2 + x + 1, initial 0
uint16_t crc16(const uint8_t *d, size_t n, uint16_t crc);  // x^16 + x^15 + x^2 + 1, initial 0, table-driven
int parse_header(const uint8_t *d, size_t len, const sk_flac_streaminfo *info, sk_flac_frame_info *out);
size_t frame_bound(const sk_flac_frame_info &h, const sk_flac_streaminfo *info);
int scan(const uint8_t *d, size_t len, const sk_flac_streaminfo *info, bool final, sk_flac_frame_info *frames, uint32_t cap, uint32_t *n_frames,
         size_t *consumed);
void parse_streaminfo(const uint8_t *b /*[34]*/, sk_flac_streaminfo *out);

class Reader {
public:
    // false: the stream is rejected, `error` has the text (and keeps it).  len == 0 finalises.
    bool add(const uint8_t *bytes, size_t len, sk_flac_frame_info *frames, uint32_t cap, uint32_t *n_frames, const uint8_t **data) {
        return feed(bytes, len, len == 0, frames, cap, n_frames, data);
    }
    // the same with the end of the stream said, not implied: len == 0 without `final` only hands out frames that an earlier call
    // left behind because its table was full (*n_frames == cap means there may be more)
    bool feed(const uint8_t *bytes, size_t len, bool final, sk_flac_frame_info *frames, uint32_t cap, uint32_t *n_frames, const uint8_t **data);
    bool finalised() const { return final_; }
    bool have_info() const { return have_info_; }
    const sk_flac_streaminfo &info() const { return info_; }
    size_t buffered_bytes() const { return buf_.size() - drop_; }
    uint64_t frames() const { return frames_; }
    const std::string &error() const { return error_; }

private:
    enum State { kMarker, kBlockHeader, kStreamInfo, kSkip, kFrames, kFailed };
    bool fail(const std::string &text);
    State state_ = kMarker;
    std::vector<uint8_t> buf_;  // what is held back; in kFrames the frames handed out last lie in front (drop_)
    size_t drop_ = 0;
    uint64_t skip_ = 0;
    bool last_block_ = false, have_info_ = false, final_ = false;
    sk_flac_streaminfo info_{};
    uint64_t frames_ = 0;
    std::string error_;
};

// ---- the definitions: inline, so that every source that needs them -- engine.cpp, pipeline.cpp, and the harnesses that compile single
// product sources -- has them from the header alone, as with pcm_stream.h ----
namespace detail {

struct Crc16Table {
    uint16_t t[256];
    Crc16Table() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i << 8;
            for (int k = 0; k < 8; ++k) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) : (c << 1);
            t[i] = (uint16_t)c;
        }
    }
};
inline const Crc16Table &crc16_table() {
    static const Crc16Table t;
    return t;
}

struct Crc8Table {
    uint8_t t[256];
    Crc8Table() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) : (c << 1);
            t[i] = (uint8_t)c;
        }
    }
};
inline const Crc8Table &crc8_table() {
    static const Crc8Table t;
    return t;
}

inline uint16_t crc16_step(uint16_t crc, uint8_t b) { return (uint16_t)((crc << 8) ^ crc16_table().t[(crc >> 8) ^ b]); }

}  // namespace detail

inline uint8_t crc8(const uint8_t *d, size_t n) {
    uint8_t c = 0;
    for (size_t i = 0; i < n; ++i) c = detail::crc8_table().t[c ^ d[i]];
    return c;
}

inline uint16_t crc16(const uint8_t *d, size_t n, uint16_t crc) {
    for (size_t i = 0; i < n; ++i) crc = detail::crc16_step(crc, d[i]);
    return crc;
}

inline int parse_header(const uint8_t *d, size_t len, const sk_flac_streaminfo *info, sk_flac_frame_info *out) {
    if (len >= 1 && d[0] != 0xFF) return SK_FLAC_NO_SYNC;
    if (len >= 2 && (d[1] & 0xFC) != 0xF8) return SK_FLAC_NO_SYNC;
    if (len < 4) return SK_FLAC_NEED_MORE;
    if (d[1] & 0x02) return SK_FLAC_RESERVED;
    const uint32_t bs_code = d[2] >> 4, rate_code = d[2] & 15, assignment = d[3] >> 4, depth_code = (d[3] >> 1) & 7;
    if (bs_code == 0 || rate_code == 15 || depth_code == 3 || assignment > 10 || (d[3] & 1)) return SK_FLAC_RESERVED;
    const bool variable = (d[1] & 1) != 0;
    // the coded number: 0xxxxxxx, or 110xxxxx ... 11111110 followed by 1 ... 6 bytes 10xxxxxx
    if (len < 5) return SK_FLAC_NEED_MORE;
    size_t p = 4;
    uint32_t extra = 0;
    uint64_t number = 0;
    {
        const uint8_t b = d[p++];
        if (b < 0x80) number = b;
        else if (b < 0xC0 || b == 0xFF) return SK_FLAC_RESERVED;
        else {
            extra = 1;
            while (extra < 6 && (b & (0x40u >> extra))) ++extra;
            number = b & (0x3Fu >> extra);  // 0xFE: six more bytes, no bits of its own
            if (extra == 6 && !variable) return SK_FLAC_RESERVED;  // a frame number has 31 bits at most
        }
    }
    const size_t tail = extra + (bs_code == 6 ? 1 : bs_code == 7 ? 2 : 0) + (rate_code == 12 ? 1 : rate_code >= 13 ? 2 : 0) + 1;
    if (len < p + tail) {
        for (size_t i = 0; i < extra && p + i < len; ++i)
            if ((d[p + i] & 0xC0) != 0x80) return SK_FLAC_RESERVED;
        return SK_FLAC_NEED_MORE;
    }
    for (uint32_t i = 0; i < extra; ++i) {
        const uint8_t b = d[p++];
        if ((b & 0xC0) != 0x80) return SK_FLAC_RESERVED;
        number = (number << 6) | (b & 0x3F);
    }
    uint32_t block = 0;
    switch (bs_code) {
    case 1: block = 192; break;
    case 2: case 3: case 4: case 5: block = 576u << (bs_code - 2); break;
    case 6: block = (uint32_t)d[p] + 1, p += 1; break;
    case 7: block = (((uint32_t)d[p] << 8) | d[p + 1]) + 1, p += 2; break;
    default: block = 256u << (bs_code - 8); break;
    }
    static const uint32_t kRates[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
    uint32_t rate = 0;
    if (rate_code < 12) rate = kRates[rate_code];
    else if (rate_code == 12) rate = (uint32_t)d[p] * 1000u, p += 1;
    else {
        rate = ((uint32_t)d[p] << 8) | d[p + 1], p += 2;
        if (rate_code == 14) rate *= 10;
    }
    if (crc8(d, p) != d[p]) return SK_FLAC_BAD_CRC;
    ++p;
    static const uint8_t kDepths[8] = {0, 8, 12, 0, 16, 20, 24, 32};
    uint32_t bits = kDepths[depth_code];
    if (rate_code == 0 || depth_code == 0) {
        if (!info) return SK_FLAC_NEED_STREAMINFO;
        if (rate_code == 0) rate = info->sample_rate;
        if (depth_code == 0) bits = info->bits_per_sample;
        if (bits < 4 || bits > 32) return SK_FLAC_RESERVED;
    }
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->number = number;
        out->sample_rate = rate;
        out->block_size = block;
        out->header_bytes = (uint8_t)p;
        out->channels = (uint8_t)(assignment < 8 ? assignment + 1 : 2);
        out->assignment = (uint8_t)assignment;
        out->bits_per_sample = (uint8_t)bits;
        out->variable_blocksize = variable ? 1 : 0;
    }
    return SK_OK;
}

inline size_t frame_bound(const sk_flac_frame_info &h, const sk_flac_streaminfo *info) {
    if (info && info->max_framesize) return info->max_framesize;
    const uint64_t bits = (uint64_t)h.block_size * h.channels * (h.bits_per_sample + 1u) + (uint64_t)h.channels * 40u;
    return (size_t)(19 + (bits + 7) / 8);
}

inline int scan(const uint8_t *d, size_t len, const sk_flac_streaminfo *info, bool final, sk_flac_frame_info *frames, uint32_t cap, uint32_t *n_frames,
         size_t *consumed) {
    size_t pos = 0;
    uint32_t n = 0;
    int rc = SK_OK;
    while (n < cap && pos < len) {
        sk_flac_frame_info h;
        rc = parse_header(d + pos, len - pos, info, &h);
        if (rc == SK_FLAC_NEED_MORE) {
            rc = SK_OK;
            break;
        }
        if (rc != SK_OK) break;
        const size_t bound = frame_bound(h, info), least = (size_t)h.header_bytes + 3;  // a subframe byte and the CRC-16
        size_t e = pos + h.header_bytes;
        uint16_t crc = crc16(d + pos, h.header_bytes, 0);  // over [pos, e)
        bool found = false, wait = false;
        for (;;) {
            if (crc == 0 && e - pos >= least) {
                if (e == len) {
                    found = final;
                    wait = !final;
                    break;
                }
                const int next = parse_header(d + e, len - e, info, nullptr);
                if (next == SK_OK) {
                    found = true;
                    break;
                }
                if (next == SK_FLAC_NEED_MORE && !final) {  // might be the next header: the bytes that decide it are still to come
                    wait = true;
                    break;
                }
            }
            if (e == len) {
                wait = true;  // final: what is left forms no frame -- the caller reports it
                break;
            }
            if (e - pos >= bound) break;
            crc = detail::crc16_step(crc, d[e]);
            ++e;
        }
        if (wait) break;
        if (!found) {
            rc = SK_FLAC_BAD_CRC;
            break;
        }
        h.offset = (uint32_t)pos;
        h.frame_bytes = (uint32_t)(e - pos);
        frames[n++] = h;
        pos = e;
    }
    *n_frames = n;
    *consumed = pos;
    return rc;
}

inline void parse_streaminfo(const uint8_t *b, sk_flac_streaminfo *out) {
    std::memset(out, 0, sizeof *out);
    out->min_blocksize = ((uint32_t)b[0] << 8) | b[1];
    out->max_blocksize = ((uint32_t)b[2] << 8) | b[3];
    out->min_framesize = ((uint32_t)b[4] << 16) | ((uint32_t)b[5] << 8) | b[6];
    out->max_framesize = ((uint32_t)b[7] << 16) | ((uint32_t)b[8] << 8) | b[9];
    out->sample_rate = ((uint32_t)b[10] << 12) | ((uint32_t)b[11] << 4) | (b[12] >> 4);
    out->channels = (uint8_t)(((b[12] >> 1) & 7) + 1);
    out->bits_per_sample = (uint8_t)((((b[12] & 1) << 4) | (b[13] >> 4)) + 1);
    out->total_samples = ((uint64_t)(b[13] & 15) << 32) | ((uint64_t)b[14] << 24) | ((uint64_t)b[15] << 16) | ((uint64_t)b[16] << 8) | b[17];
    std::memcpy(out->md5, b + 18, 16);
}

inline bool Reader::fail(const std::string &text) {
    state_ = kFailed;
    error_ = text;
    return false;
}

inline bool Reader::feed(const uint8_t *bytes, size_t len, bool final, sk_flac_frame_info *frames, uint32_t cap, uint32_t *n_frames, const uint8_t **data) {
    *n_frames = 0;
    if (data) *data = nullptr;
    if (state_ == kFailed) return false;
    if (drop_) {
        buf_.erase(buf_.begin(), buf_.begin() + (ptrdiff_t)drop_);
        drop_ = 0;
    }
    if (len && final_) return fail("FLAC stream: bytes after the finalising add");
    if (final) final_ = true;
    const auto take = [&](size_t want) {  // fills buf_ up to `want` bytes; true when it has them
        const size_t n = want - buf_.size() < len ? want - buf_.size() : len;
        buf_.insert(buf_.end(), bytes, bytes + n);
        bytes += n, len -= n;
        return buf_.size() == want;
    };
    const auto after_block = [&] {
        buf_.clear();
        state_ = last_block_ ? kFrames : kBlockHeader;
    };
    while (len && state_ != kFrames) {
        if (state_ == kMarker) {
            if (!take(4)) break;
            if (std::memcmp(buf_.data(), "fLaC", 4) != 0) return fail("not a FLAC stream: the fLaC marker is missing");
            buf_.clear();
            state_ = kBlockHeader;
        } else if (state_ == kBlockHeader) {
            if (!take(4)) break;
            const uint32_t type = buf_[0] & 0x7F, length = ((uint32_t)buf_[1] << 16) | ((uint32_t)buf_[2] << 8) | buf_[3];
            last_block_ = (buf_[0] & 0x80) != 0;
            if (type == 127) return fail("FLAC metadata: block type 127 is forbidden");
            if (!have_info_) {
                if (type != 0) return fail("FLAC metadata: the first block is not STREAMINFO");
                if (length != 34) return fail("FLAC metadata: STREAMINFO is " + std::to_string(length) + " bytes long, not 34");
                buf_.clear();
                state_ = kStreamInfo;
            } else {
                if (type == 0) return fail("FLAC metadata: a second STREAMINFO block");
                skip_ = length;  // PADDING ... PICTURE and the reserved types: stepped over by count
                if (skip_) buf_.clear(), state_ = kSkip;
                else after_block();
            }
        } else if (state_ == kStreamInfo) {
            if (!take(34)) break;
            parse_streaminfo(buf_.data(), &info_);
            if (info_.sample_rate == 0) return fail("FLAC STREAMINFO: sample rate 0");
            if (info_.bits_per_sample < 4) return fail("FLAC STREAMINFO: " + std::to_string(info_.bits_per_sample) + " bits per sample");
            if (info_.max_framesize && info_.max_framesize < 9) return fail("FLAC STREAMINFO: max_framesize is shorter than any frame");
            have_info_ = true;
            after_block();
        } else {  // kSkip
            const size_t n = skip_ < len ? (size_t)skip_ : len;
            bytes += n, len -= n, skip_ -= n;
            if (skip_ == 0) after_block();
        }
    }
    if (state_ != kFrames) {
        if (final_) return fail("truncated FLAC stream: it ends inside the metadata");
        return true;
    }
    if (len) buf_.insert(buf_.end(), bytes, bytes + len);
    size_t consumed = 0;
    uint32_t n = 0;
    const int rc = scan(buf_.data(), buf_.size(), &info_, final_, frames, cap, &n, &consumed);
    for (uint32_t i = 0; i < n; ++i) {
        const sk_flac_frame_info &f = frames[i];
        if (f.channels != info_.channels || f.bits_per_sample != info_.bits_per_sample || f.sample_rate != info_.sample_rate)
            return fail("FLAC frame " + std::to_string(frames_ + i) + ": " + std::to_string(f.channels) + " channels, " +
                        std::to_string(f.bits_per_sample) + " bits, " + std::to_string(f.sample_rate) + " Hz disagree with STREAMINFO");
    }
    if (rc != SK_OK) {
        const std::string at = "FLAC frame " + std::to_string(frames_ + n) + ": ";
        if (rc == SK_FLAC_BAD_CRC) return fail(at + "no frame end with a valid CRC (header CRC-8 or frame CRC-16 fails)");
        if (rc == SK_FLAC_NO_SYNC) return fail(at + "no sync code where the frame must begin");
        if (rc == SK_FLAC_RESERVED) return fail(at + "a reserved value in the frame header");
        return fail(at + "invalid frame header");
    }
    if (final_ && n < cap && consumed < buf_.size())
        return fail("truncated FLAC stream: the last " + std::to_string(buf_.size() - consumed) + " bytes form no frame");
    if (data) *data = buf_.data();
    drop_ = consumed;
    frames_ += n;
    *n_frames = n;
    return true;
}

}  // namespace sk_flac

struct sk_flac_reader {
    sk_flac::Reader reader;
};

// WebM / Matroska, audio only, on the host: the streaming EBML walk of soundkit-webm's WebmMediaDemuxer with the audio view of its
// WebmAudioDemuxer on top (soundkit-webm/src/lib.rs:489-1100, 2097-2196), the CodecPrivate split of A_VORBIS (parse_vorbis_codec_private,
// 333-354) and the discard-padding conversion (discard_padding_frames, 3087-3109).  Serial byte parsing per stream, no per-sample work,
// no HIP; header-only.  The input is untrusted: every size is checked against the bytes that hold it before it is used as an offset, and
// nothing recurses on the input's depth (Tracks and Cluster are entered by stepping over their headers, the masters below a TrackEntry
// have a fixed depth).
//
// As the reference does, an element is parsed once all of it is buffered, so the budgets bound the buffer: 4 MiB a call, 16 MiB a
// metadata element, 64 MiB a block element, both refused from the element's header.  Only Segment and Cluster may have an unknown
// size; anywhere else the all-ones size is a number and meets the budget.  Video tracks of the reference's four codec ids are kept in
// the track list (a repeated TrackNumber loses to the first entry of either kind) and their blocks are walked and dropped.
// Not read: Cues / seeking, chained segments, EBML CRC-32, ContentCompression other than header stripping, encryption, the old
// A_AAC/MPEG4/... ids, the AVC / HEVC / AV1 configuration records.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <string>
#include <utility>
#include <vector>

namespace sk_webm {

constexpr size_t kMaxInputChunkBytes = 4u * 1024 * 1024;        // MAX_WEBM_INPUT_CHUNK_BYTES
constexpr uint64_t kMaxMetadataBytes = 16ull * 1024 * 1024;     // MAX_WEBM_METADATA_ELEMENT_BYTES
constexpr uint64_t kMaxPacketBytes = 64ull * 1024 * 1024;       // MAX_WEBM_PACKET_ELEMENT_BYTES
constexpr size_t kMaxBufferBytes = (size_t)kMaxPacketBytes + 64 * 1024;  // MAX_WEBM_BUFFER_BYTES
enum : uint8_t { kCodecNone = 0, kCodecVorbis = 1, kCodecAac = 2, kCodecFlac = 3, kCodecAlac = 4, kCodecOpus = 5 };
enum : uint8_t { kAudio = 1, kVideo = 2 };

constexpr uint32_t kIdEbml = 0x1A45DFA3, kIdSegment = 0x18538067, kIdTracks = 0x1654AE6B, kIdTrackEntry = 0xAE, kIdCluster = 0x1F43B675,
                   kIdInfo = 0x1549A966, kIdTimecodeScale = 0x2AD7B1, kIdClusterTimecode = 0xE7, kIdSimpleBlock = 0xA3, kIdBlock = 0xA1,
                   kIdBlockGroup = 0xA0, kIdBlockDuration = 0x9B, kIdReferenceBlock = 0xFB, kIdDiscardPadding = 0x75A2;

inline const char *codec_name(uint8_t codec) {
    static const char *const names[] = {"", "A_VORBIS", "A_AAC", "A_FLAC", "A_ALAC", "A_OPUS"};
    return codec <= kCodecOpus ? names[codec] : "";
}

// read_vint: the value without its length marker and the bytes it took; 0 bytes: not there (no data, a zero first byte, or cut short)
inline size_t read_vint(const uint8_t *d, size_t n, uint64_t *value) {
    if (n == 0 || d[0] == 0) return 0;
    const size_t len = (size_t)__builtin_clz((uint32_t)d[0]) - 24 + 1;
    if (n < len) return 0;
    uint64_t v = len < 8 ? (uint64_t)(d[0] & (0xffu >> len)) : 0;
    for (size_t i = 1; i < len; ++i) v = v << 8 | d[i];
    *value = v;
    return len;
}

// read_element_id: the id with its marker, one to four bytes
inline size_t read_id(const uint8_t *d, size_t n, uint32_t *id) {
    if (n == 0 || d[0] == 0) return 0;
    const size_t len = (size_t)__builtin_clz((uint32_t)d[0]) - 24 + 1;
    if (len > 4 || n < len) return 0;
    uint32_t v = 0;
    for (size_t i = 0; i < len; ++i) v = v << 8 | d[i];
    *id = v;
    return len;
}

inline uint64_t read_uint(const uint8_t *d, size_t n) {  // read_uint: the first eight bytes at most
    uint64_t v = 0;
    for (size_t i = 0; i < std::min<size_t>(n, 8); ++i) v = v << 8 | d[i];
    return v;
}

inline double read_float(const uint8_t *d, size_t n) {  // read_float: four or eight bytes, anything else is 0
    if (n == 4) {
        const uint32_t b = (uint32_t)read_uint(d, 4);
        float f;
        std::memcpy(&f, &b, 4);
        return (double)f;
    }
    if (n == 8) {
        const uint64_t b = read_uint(d, 8);
        double f;
        std::memcpy(&f, &b, 8);
        return f;
    }
    return 0.0;
}

inline bool is_unknown_size(uint64_t size, size_t len) { return len >= 1 && len <= 8 && size == (1ull << (len * 7)) - 1; }

inline std::string hex(uint64_t v) {
    char text[24];
    std::snprintf(text, sizeof text, "%llX", (unsigned long long)v);
    return text;
}

// bounded_webm_element_size
inline bool bounded_size(uint32_t id, uint64_t size, std::string *error) {
    const uint64_t budget = (id == kIdSimpleBlock || id == kIdBlock || id == kIdBlockGroup) ? kMaxPacketBytes : kMaxMetadataBytes;
    if (size <= budget) return true;
    *error = "WebM element 0x" + hex(id) + " exceeds the " + std::to_string(budget) + " byte budget";
    return false;
}

// One child of a master whose bytes are all there (parse_media_settings and the loops shaped like it).  1: a child, its payload at
// [*start, *start + *size); 0: the walk ends (fewer than two bytes left, or an id / size that cannot be read); -1: the child runs past
// the master's end
inline int next_child(const uint8_t *d, size_t n, size_t *pos, uint32_t *id, size_t *start, size_t *size) {
    if (*pos + 2 > n) return 0;
    const size_t id_len = read_id(d + *pos, n - *pos, id);
    if (!id_len) return 0;
    uint64_t declared;
    const size_t size_len = read_vint(d + *pos + id_len, n - *pos - id_len, &declared);
    if (!size_len) return 0;
    *start = *pos + id_len + size_len;
    if (declared > n - *start) return -1;
    *size = (size_t)declared;
    *pos = *start + *size;
    return 1;
}

struct Track {
    uint64_t number = 0;
    uint8_t kind = 0, codec = kCodecNone;
    std::string codec_id;
    std::vector<uint8_t> codec_private, prefix;  // prefix: what header stripping took off every frame
    bool has_rate = false, has_channels = false, has_default_duration = false;
    uint32_t sample_rate = 0;
    uint8_t channels = 0;
    uint64_t default_duration_ns = 0, codec_delay_ns = 0, seek_pre_roll_ns = 0;
    double timestamp_scale = 1.0;
};

struct Packet {
    uint64_t track = 0;
    uint8_t codec = kCodecNone;
    std::vector<uint8_t> data;
    int64_t timestamp_ns = 0;
    bool has_duration = false, has_discard = false;
    uint64_t duration_ns = 0;
    int64_t discard_ns = 0;
};

// parse_content_encoding: one ContentEncoding -> the header-stripping prefix
inline bool parse_content_encoding(const uint8_t *d, size_t n, std::vector<uint8_t> *prefix, std::string *error) {
    uint64_t scope = 1, type = 0, algorithm = 0;
    const uint8_t *comp = nullptr, *settings = nullptr;
    size_t comp_len = 0, settings_len = 0, pos = 0, start, size;
    uint32_t id;
    int rc;
    while ((rc = next_child(d, n, &pos, &id, &start, &size)) == 1) {
        if (id == 0x5032) scope = read_uint(d + start, size);
        else if (id == 0x5033) type = read_uint(d + start, size);
        else if (id == 0x5034) comp = d + start, comp_len = size;
    }
    if (rc < 0) return *error = "truncated WebM track settings", false;
    if (type != 0) return *error = "encrypted Matroska ContentEncoding is unsupported", false;
    if ((scope & 1) == 0) return *error = "Matroska ContentEncoding does not apply to frame data", false;
    if (!comp) return *error = "Matroska ContentEncoding has no compression settings", false;
    pos = 0;
    while ((rc = next_child(comp, comp_len, &pos, &id, &start, &size)) == 1) {
        if (id == 0x4254) algorithm = read_uint(comp + start, size);
        else if (id == 0x4255) settings = comp + start, settings_len = size;
    }
    if (rc < 0) return *error = "truncated WebM track settings", false;
    if (algorithm != 3) return *error = "unsupported Matroska ContentCompAlgo " + std::to_string(algorithm) + "; only header stripping is supported", false;
    if (!settings) return *error = "Matroska header stripping has no prefix bytes", false;
    prefix->assign(settings, settings + settings_len);
    return true;
}

// parse_content_encodings
inline bool parse_content_encodings(const uint8_t *d, size_t n, std::vector<uint8_t> *prefix, std::string *error) {
    bool have = false;
    size_t pos = 0;
    while (pos + 2 <= n) {
        uint32_t id;
        const size_t id_len = read_id(d + pos, n - pos, &id);
        if (!id_len) return *error = "invalid WebM ContentEncodings element", false;
        uint64_t declared;
        const size_t size_len = read_vint(d + pos + id_len, n - pos - id_len, &declared);
        if (!size_len) return *error = "truncated WebM ContentEncodings size", false;
        const size_t start = pos + id_len + size_len;
        if (declared > n - start) return *error = "truncated WebM ContentEncoding", false;
        pos = start + (size_t)declared;
        if (id != 0x6240) continue;
        if (have) return *error = "multiple Matroska ContentEncodings are unsupported", false;
        if (!parse_content_encoding(d + start, (size_t)declared, prefix, error)) return false;
        have = true;
    }
    if (!have) return *error = "empty Matroska ContentEncodings is unsupported", false;
    return true;
}

// parse_media_track_entry.  *keep: the entry names a track the reference's lists hold
inline bool parse_track_entry(const uint8_t *d, size_t n, Track *t, bool *keep, std::string *error) {
    *keep = false;
    bool have_number = false;
    size_t pos = 0, start, size;
    uint32_t id;
    int rc;
    while ((rc = next_child(d, n, &pos, &id, &start, &size)) == 1) {
        const uint8_t *v = d + start;
        switch (id) {
        case 0xD7: t->number = read_uint(v, size), have_number = true; break;
        case 0x83: {
            const uint64_t type = read_uint(v, size);
            t->kind = type == 2 ? kAudio : type == 1 ? kVideo : 0;
            break;
        }
        case 0x86: t->codec_id.assign((const char *)v, size); break;
        case 0x63A2: t->codec_private.assign(v, v + size); break;
        case 0x23E383: t->default_duration_ns = read_uint(v, size), t->has_default_duration = t->default_duration_ns > 0; break;
        case 0x56AA: t->codec_delay_ns = read_uint(v, size); break;
        case 0x56BB: t->seek_pre_roll_ns = read_uint(v, size); break;
        case 0x23314F:
            t->timestamp_scale = read_float(v, size);
            if (!std::isfinite(t->timestamp_scale) || t->timestamp_scale <= 0.0) return *error = "WebM TrackTimestampScale must be finite and positive", false;
            break;
        case 0x6D80:
            t->prefix.clear();
            if (!parse_content_encodings(v, size, &t->prefix, error)) return false;
            break;
        case 0xE1: {  // Audio
            size_t p2 = 0, s2, n2;
            uint32_t id2;
            int rc2;
            while ((rc2 = next_child(v, size, &p2, &id2, &s2, &n2)) == 1) {
                if (id2 == 0xB5) {
                    const double rate = read_float(v + s2, n2);
                    if (std::isfinite(rate) && rate > 0.0 && rate <= 4294967295.0) t->sample_rate = (uint32_t)std::round(rate), t->has_rate = true;
                } else if (id2 == 0x9F) {
                    const uint64_t count = read_uint(v + s2, n2);
                    if (count > 0 && count <= 255) t->channels = (uint8_t)count, t->has_channels = true;
                }
            }
            if (rc2 < 0) return *error = "truncated WebM track settings", false;
            break;
        }
        case 0xE0: {  // Video: walked for its bounds alone
            size_t p2 = 0, s2, n2;
            uint32_t id2;
            int rc2;
            while ((rc2 = next_child(v, size, &p2, &id2, &s2, &n2)) == 1) {
            }
            if (rc2 < 0) return *error = "truncated WebM track settings", false;
            break;
        }
        default: break;
        }
    }
    if (rc < 0) return *error = "truncated WebM TrackEntry", false;
    if (!have_number || !t->kind) return true;
    if (t->kind == kAudio) {
        for (uint8_t c = kCodecVorbis; c <= kCodecOpus; ++c)
            if (t->codec_id == codec_name(c)) t->codec = c;
        *keep = t->codec != kCodecNone;
    } else {
        *keep = t->codec_id == "V_VP9" || t->codec_id == "V_AV1" || t->codec_id == "V_MPEG4/ISO/AVC" || t->codec_id == "V_MPEGH/ISO/HEVC";
    }
    return true;
}

// validate_ebml_header
inline bool validate_ebml_header(const uint8_t *d, size_t n, std::string *error) {
    uint64_t read_version = 1, max_id = 4, max_size = 8, doc_read_version = 1;
    bool have_doc = false;
    std::string doc;
    size_t pos = 0, start, size;
    uint32_t id;
    int rc;
    while ((rc = next_child(d, n, &pos, &id, &start, &size)) == 1) {
        if (id == 0x42F7) read_version = read_uint(d + start, size);
        else if (id == 0x42F2) max_id = read_uint(d + start, size);
        else if (id == 0x42F3) max_size = read_uint(d + start, size);
        else if (id == 0x4282) doc.assign((const char *)d + start, size), have_doc = true;
        else if (id == 0x4285) doc_read_version = read_uint(d + start, size);
    }
    if (rc < 0) return *error = "truncated WebM track settings", false;
    if (read_version > 1) return *error = "unsupported EBML read version " + std::to_string(read_version), false;
    if (max_id > 4 || max_size > 8) return *error = "unsupported EBML element width", false;
    if (!have_doc) return *error = "WebM EBML header is missing DocType", false;
    if (doc != "webm" && doc != "matroska") return *error = "unsupported EBML DocType " + doc, false;
    if (doc_read_version > 4) return *error = "unsupported Matroska DocTypeReadVersion " + std::to_string(doc_read_version), false;
    return true;
}

// opus_packet_duration_ns: the TOC byte's frame size times its frame count, at most 120 ms
inline bool opus_packet_duration_ns(const uint8_t *d, size_t n, uint64_t *ns) {
    if (n == 0) return false;
    const uint32_t toc = d[0], config = toc >> 3;
    static const uint32_t silk[4] = {10000, 20000, 40000, 60000}, hybrid[2] = {10000, 20000}, celt[4] = {2500, 5000, 10000, 20000};
    const uint64_t frame_us = config < 12 ? silk[config & 3] : config < 16 ? hybrid[config & 1] : celt[config & 3];
    uint64_t count = 1;
    if ((toc & 3) == 1 || (toc & 3) == 2) count = 2;
    if ((toc & 3) == 3) {
        if (n < 2) return false;
        count = d[1] & 0x3f;
    }
    const uint64_t us = frame_us * count;
    if (count == 0 || us > 120000) return false;
    *ns = us * 1000;
    return true;
}

// the frames of a block's payload as (offset, size) pairs: parse_block_frames with its four lacings
inline bool block_frames(uint8_t flags, const uint8_t *d, size_t n, std::vector<std::pair<size_t, size_t>> *frames, std::string *error) {
    frames->clear();
    const uint8_t lacing = flags & 0x06;
    if (lacing == 0) {
        frames->emplace_back(0, n);
        return true;
    }
    const char *const name = lacing == 0x02 ? "Xiph" : lacing == 0x04 ? "fixed" : "EBML";
    if (n == 0) return *error = std::string("Truncated ") + name + "-laced block", false;
    const size_t count = (size_t)d[0] + 1;
    size_t pos = 1;
    std::vector<uint64_t> sizes;
    sizes.reserve(count);
    uint64_t known = 0;
    if (lacing == 0x02) {
        for (size_t k = 0; k + 1 < count; ++k) {
            uint64_t size = 0;
            for (;;) {
                if (pos >= n) return *error = "Truncated Xiph lacing size", false;
                const uint8_t b = d[pos++];
                size += b;
                if (b != 255) break;
            }
            known += size;
            sizes.push_back(size);
        }
        if (known > n - pos) return *error = "Xiph-laced frame sizes exceed block payload", false;
        sizes.push_back(n - pos - known);
    } else if (lacing == 0x04) {
        if ((n - 1) % count != 0) return *error = "Invalid fixed-laced block size", false;
        sizes.assign(count, (n - 1) / count);
    } else {
        uint64_t first;
        const size_t first_len = read_vint(d + pos, n - pos, &first);
        if (!first_len) return *error = "Truncated EBML-laced first frame size", false;
        pos += first_len;
        int64_t previous = (int64_t)first;
        sizes.push_back(first);
        for (size_t k = 1; k + 1 < count; ++k) {
            uint64_t raw;
            const size_t len = read_vint(d + pos, n - pos, &raw);
            if (!len) return *error = "Truncated EBML-laced frame size delta", false;
            pos += len;
            const int64_t delta = (int64_t)raw - (((int64_t)1 << (7 * len - 1)) - 1);
            if (__builtin_add_overflow(previous, delta, &previous)) return *error = "EBML-laced frame size overflow", false;
            if (previous < 0) return *error = "Negative EBML-laced frame size", false;
            sizes.push_back((uint64_t)previous);
        }
        for (uint64_t s : sizes) {
            known += s;
            if (known > n) break;  // more than the payload holds: no need to add further
        }
        if (known > n - pos) return *error = "EBML-laced frame sizes exceed block payload", false;
        // one frame: the first size is the only one listed and a last, unlisted frame follows it all the same (the reference's reading)
        sizes.push_back(n - pos - known);
    }
    size_t at = pos;
    for (uint64_t s : sizes) {  // split_laced_frames
        if (s > n - at) return *error = "Laced frame extends past block payload", false;
        frames->emplace_back(at, (size_t)s);
        at += (size_t)s;
    }
    if (at != n) return *error = "Laced frame sizes do not consume block payload", false;
    return true;
}

// scale_webm_timestamp / scale_webm_duration: f64 products, rounded half away from zero, saturating at the type's end as `as` does
inline bool scale_timestamp(int64_t ticks, uint64_t scale_ns, double track_scale, int64_t *ns, std::string *error) {
    const double v = (double)ticks * (double)scale_ns * track_scale;
    if (!std::isfinite(v) || v < -9223372036854775808.0 || v > 9223372036854775808.0) return *error = "WebM nanosecond timestamp overflow", false;
    const double r = std::round(v);
    *ns = r >= 9223372036854775808.0 ? INT64_MAX : (int64_t)r;
    return true;
}
inline bool scale_duration(uint64_t ticks, uint64_t scale_ns, double track_scale, uint64_t *ns, std::string *error) {
    const double v = (double)ticks * (double)scale_ns * track_scale;
    if (!std::isfinite(v) || v < 0.0 || v > 18446744073709551616.0) return *error = "WebM BlockDuration overflow", false;
    const double r = std::round(v);
    *ns = r >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)r;
    return true;
}

// parse_vorbis_codec_private: the three headers as (offset, size) into the CodecPrivate
inline bool vorbis_headers(const uint8_t *d, size_t n, size_t offsets[3], size_t sizes[3], std::string *error) {
    if (n == 0) return *error = "Missing Vorbis CodecPrivate", false;
    if (d[0] != 2) return *error = "Expected 3 Vorbis headers in CodecPrivate, got " + std::to_string((unsigned)d[0] + 1), false;
    size_t pos = 1;
    for (int k = 0; k < 2; ++k) {
        size_t size = 0;
        for (;;) {
            if (pos >= n) return *error = "Truncated Xiph lacing size", false;
            const uint8_t b = d[pos++];
            size += b;
            if (b != 255) break;
        }
        sizes[k] = size;
    }
    if (sizes[0] + sizes[1] > n - pos) return *error = "Vorbis CodecPrivate header sizes exceed payload", false;
    sizes[2] = n - pos - sizes[0] - sizes[1];
    offsets[0] = pos, offsets[1] = pos + sizes[0], offsets[2] = pos + sizes[0] + sizes[1];
    return true;
}

// discard_padding_frames: ceil(|ns| * rate / 1e9) capped at the decoded frames; a negative padding trims the front, a positive the back
inline bool discard_frames(int64_t padding_ns, uint32_t rate, uint32_t decoded_frames, uint32_t *front, uint32_t *back, std::string *error) {
    const uint64_t magnitude = padding_ns < 0 ? 0 - (uint64_t)padding_ns : (uint64_t)padding_ns;
    uint64_t product;
    if (__builtin_mul_overflow(magnitude, (uint64_t)rate, &product) || __builtin_add_overflow(product, (uint64_t)999999999, &product))
        return *error = "WebM discard-padding conversion overflow", false;
    const uint32_t frames = (uint32_t)std::min<uint64_t>(product / 1000000000ull, decoded_frames);
    *front = padding_ns < 0 ? frames : 0;
    *back = padding_ns < 0 ? 0 : frames;
    return true;
}

// WebmAudioDemuxer over WebmMediaDemuxer.  add / finish: false is a refusal (error; the demuxer stays refused).  Events: the audio
// tracks (configured, once the first Cluster header has arrived), then `packets` in file order.
struct Demuxer {
    std::vector<Track> tracks;   // every kept entry, audio and video, first TrackNumber wins
    std::vector<Track> audio;    // the reported ones, in file order; valid once `configured`
    std::deque<Packet> packets;
    bool configured = false, failed = false;
    uint64_t timecode_scale_ns = 1000000;
    std::string error;

    size_t buffered() const { return buf_.size() - at_; }
    size_t queued_bytes() const { return queued_; }
    void pop_packet() {
        queued_ -= packets.front().data.size();
        packets.pop_front();
    }
    Packet take_packet() {
        Packet p = std::move(packets.front());
        packets.pop_front();
        queued_ -= p.data.size();
        return p;
    }

    bool add(const uint8_t *data, size_t len) {
        if (failed) return false;
        if (len > kMaxInputChunkBytes) return fail("WebM input chunk exceeds the " + std::to_string(kMaxInputChunkBytes) + " byte streaming budget");
        if (buffered() + len > kMaxBufferBytes) return fail("WebM parser buffer exceeds the " + std::to_string(kMaxBufferBytes) + " byte budget");
        if (at_ > 0) {
            buf_.erase(buf_.begin(), buf_.begin() + (ptrdiff_t)at_);
            at_ = 0;
        }
        if (len) buf_.insert(buf_.end(), data, data + len);
        for (;;) {
            const int before = state_;
            size_t consumed = 0;
            const bool ok = state_ == 0 ? parse_header(&consumed) : state_ == 1 ? parse_tracks(&consumed) : parse_clusters(&consumed);
            if (!ok) return fail(error);
            at_ += consumed;
            if (consumed == 0 && state_ == before) break;
        }
        return true;
    }

    bool finish() {
        if (!add(nullptr, 0)) return false;
        if (buffered()) return fail("truncated WebM element: " + std::to_string(buffered()) + " buffered bytes remain");
        if (audio.empty()) return fail("WebM source has no supported audio track");
        return true;
    }

  private:
    std::vector<uint8_t> buf_;
    size_t at_ = 0, queued_ = 0;
    int state_ = 0;  // 0 header, 1 tracks, 2 clusters
    int64_t cluster_timecode_ = 0;
    std::vector<std::pair<size_t, size_t>> frames_;

    bool fail(const std::string &text) {
        error = text;
        failed = true;
        return false;
    }

    bool parse_header(size_t *consumed) {
        const uint8_t *d = buf_.data() + at_;
        const size_t n = buffered();
        if (n < 4) return true;
        uint32_t id;
        const size_t id_len = read_id(d, n, &id);
        if (!id_len) return error = "invalid WebM EBML element ID", false;
        if (id != kIdEbml) return error = "invalid WebM: expected EBML header, got 0x" + hex(id), false;
        uint64_t size;
        const size_t size_len = read_vint(d + id_len, n - id_len, &size);
        if (!size_len) return true;
        if (!bounded_size(id, size, &error)) return false;
        const size_t total = id_len + size_len + (size_t)size;
        if (n < total) return true;
        if (!validate_ebml_header(d + id_len + size_len, (size_t)size, &error)) return false;
        uint32_t segment;
        const size_t segment_len = read_id(d + total, n - total, &segment);
        if (!segment_len) return true;
        if (segment != kIdSegment) return error = "invalid WebM: expected Segment, got 0x" + hex(segment), false;
        uint64_t ignored;
        const size_t segment_size_len = read_vint(d + total + segment_len, n - total - segment_len, &ignored);
        if (!segment_size_len) return true;
        state_ = 1;
        *consumed = total + segment_len + segment_size_len;
        return true;
    }

    bool parse_tracks(size_t *consumed) {
        const uint8_t *d = buf_.data() + at_;
        const size_t n = buffered();
        size_t pos = 0;
        while (pos + 2 <= n) {
            uint32_t id;
            const size_t id_len = read_id(d + pos, n - pos, &id);
            if (!id_len) break;
            uint64_t size;
            const size_t size_len = read_vint(d + pos + id_len, n - pos - id_len, &size);
            if (!size_len) break;
            const size_t header = id_len + size_len;
            if (id == kIdCluster) {
                if (!configured) {
                    if (tracks.empty()) return error = "WebM source has no supported media track", false;
                    for (const Track &t : tracks)
                        if (t.kind == kAudio) audio.push_back(t);
                    configured = true;
                }
                state_ = 2;
                break;
            }
            if (id == kIdTracks || (id == kIdSegment && is_unknown_size(size, size_len))) {
                pos += header;
                continue;
            }
            if (!bounded_size(id, size, &error)) return false;
            if (size > n - pos - header) break;
            const uint8_t *v = d + pos + header;
            if (id == kIdTrackEntry) {
                Track t;
                bool keep;
                if (!parse_track_entry(v, (size_t)size, &t, &keep, &error)) return false;
                if (keep && std::none_of(tracks.begin(), tracks.end(), [&](const Track &o) { return o.number == t.number; })) tracks.push_back(std::move(t));
            } else if (id == kIdInfo) {
                size_t p2 = 0, s2, n2;
                uint32_t id2;
                int rc;
                while ((rc = next_child(v, (size_t)size, &p2, &id2, &s2, &n2)) == 1)
                    if (id2 == kIdTimecodeScale) timecode_scale_ns = read_uint(v + s2, n2);
                if (rc < 0) return error = "truncated WebM track settings", false;
                if (timecode_scale_ns == 0) return error = "WebM TimecodeScale must be positive", false;
            }
            pos += header + (size_t)size;
        }
        *consumed = pos;
        return true;
    }

    bool parse_clusters(size_t *consumed) {
        size_t pos = 0;
        for (;;) {
            const uint8_t *d = buf_.data() + at_;
            const size_t n = buffered();
            if (pos + 2 > n) break;
            uint32_t id;
            const size_t id_len = read_id(d + pos, n - pos, &id);
            if (!id_len) break;
            uint64_t size;
            const size_t size_len = read_vint(d + pos + id_len, n - pos - id_len, &size);
            if (!size_len) break;
            const size_t header = id_len + size_len;
            if (id == kIdCluster) {
                cluster_timecode_ = 0;
                pos += header;
                continue;
            }
            if (!bounded_size(id, size, &error)) return false;
            if (size > n - pos - header) break;
            const uint8_t *v = d + pos + header;
            if (id == kIdClusterTimecode) {
                const uint64_t t = read_uint(v, (size_t)size);
                if (t > (uint64_t)INT64_MAX) return error = "WebM cluster timecode exceeds i64", false;
                cluster_timecode_ = (int64_t)t;
            } else if (id == kIdSimpleBlock || id == kIdBlock) {
                if (!emit_block(v, (size_t)size, false, 0, false, 0)) return false;
            } else if (id == kIdBlockGroup) {
                if (!parse_block_group(v, (size_t)size)) return false;
            }
            pos += header + (size_t)size;
        }
        *consumed = pos;
        return true;
    }

    bool parse_block_group(const uint8_t *d, size_t n) {
        const uint8_t *block = nullptr;
        size_t block_len = 0, pos = 0, start, size;
        bool has_duration = false, has_discard = false;
        uint64_t duration = 0;
        int64_t discard = 0;
        uint32_t id;
        int rc;
        while ((rc = next_child(d, n, &pos, &id, &start, &size)) == 1) {
            if (id == kIdBlock) {
                block = d + start, block_len = size;
            } else if (id == kIdBlockDuration) {
                duration = read_uint(d + start, size), has_duration = true;
            } else if (id == kIdDiscardPadding) {  // read_int
                if (size < 1 || size > 8) return error = "invalid WebM signed integer size", false;
                uint64_t raw = (d[start] & 0x80) ? ~0ull : 0;
                for (size_t i = 0; i < size; ++i) raw = raw << 8 | d[start + i];
                discard = (int64_t)raw, has_discard = true;
            }
        }
        if (rc < 0) return error = "truncated WebM BlockGroup", false;
        return block ? emit_block(block, block_len, has_duration, duration, has_discard, discard) : true;
    }

    // emit_media_block
    bool emit_block(const uint8_t *d, size_t n, bool has_duration, uint64_t duration_ticks, bool has_discard, int64_t discard_ns) {
        uint64_t number;
        const size_t track_len = read_vint(d, n, &number);
        if (!track_len) return error = "invalid WebM block track number", false;
        if (n < track_len + 3) return error = "truncated WebM block header", false;
        const Track *track = nullptr;
        for (const Track &t : tracks)
            if (t.number == number) {
                track = &t;
                break;
            }
        if (!track) return true;
        const int64_t relative = (int16_t)(uint16_t)((uint32_t)d[track_len] << 8 | d[track_len + 1]);
        const uint8_t flags = d[track_len + 2];
        int64_t ticks, timestamp;
        if (__builtin_add_overflow(cluster_timecode_, relative, &ticks)) return error = "WebM block timestamp overflow", false;
        if (!scale_timestamp(ticks, timecode_scale_ns, track->timestamp_scale, &timestamp, &error)) return false;
        if (track->codec_delay_ns > (uint64_t)INT64_MAX) return error = "WebM CodecDelay exceeds the signed timeline range", false;
        if (__builtin_sub_overflow(timestamp, (int64_t)track->codec_delay_ns, &timestamp)) return error = "WebM CodecDelay timestamp underflow", false;
        const uint8_t *payload = d + track_len + 3;
        if (!block_frames(flags, payload, n - track_len - 3, &frames_, &error)) return false;
        const size_t count = frames_.size();
        bool declared = false;
        uint64_t declared_ns = 0;
        if (has_duration) {
            if (!scale_duration(duration_ticks, timecode_scale_ns, track->timestamp_scale, &declared_ns, &error)) return false;
            declared_ns /= count, declared = true;
        } else if (track->has_default_duration) {
            declared_ns = track->default_duration_ns, declared = true;
        }
        std::vector<std::pair<bool, uint64_t>> durations(count, {declared, declared_ns});
        for (size_t k = 0; k < count && !declared; ++k)
            if (track->codec == kCodecOpus) durations[k].first = opus_packet_duration_ns(payload + frames_[k].first, frames_[k].second, &durations[k].second);
        if (count > 1)
            for (size_t k = 0; k < count; ++k)
                if (!durations[k].first) return error = "laced WebM " + track->codec_id + " timing cannot be resolved deterministically", false;
        uint64_t offset_ns = 0;
        for (size_t k = 0; k < count; ++k) {
            if (frames_[k].second == 0) continue;
            int64_t at;
            if (offset_ns > (uint64_t)INT64_MAX || __builtin_add_overflow(timestamp, (int64_t)offset_ns, &at)) return error = "WebM laced frame timestamp overflow", false;
            if (track->kind == kAudio) {
                Packet p;
                p.track = number, p.codec = track->codec, p.timestamp_ns = at;
                p.data.reserve(track->prefix.size() + frames_[k].second);
                p.data.assign(track->prefix.begin(), track->prefix.end());
                p.data.insert(p.data.end(), payload + frames_[k].first, payload + frames_[k].first + frames_[k].second);
                p.has_duration = durations[k].first, p.duration_ns = durations[k].first ? durations[k].second : 0;
                p.has_discard = has_discard && k + 1 == count, p.discard_ns = p.has_discard ? discard_ns : 0;
                queued_ += p.data.size();
                packets.push_back(std::move(p));
            }
            if (durations[k].first && __builtin_add_overflow(offset_ns, durations[k].second, &offset_ns)) return error = "WebM laced duration overflow", false;
        }
        return true;
    }
};

}  // namespace sk_webm

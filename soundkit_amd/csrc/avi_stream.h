// AVI (.avi, OpenDML `AVIX` forms), audio only, on the host: what soundkit-decoder's decode_avi_audio reads (soundkit-decoder/src/lib.rs:
// 257-570: for_each_avi_riff, for_each_riff_chunk, parse_avi_audio_format, parse_avi_stream_list, collect_avi_audio_chunks, avi_stream_id)
// as one incremental walk with its checks, budgets and texts.  `RIFF....AVI ` and any number of `RIFF....AVIX` forms; `LIST hdrl` ->
// `LIST strl` -> `strh` / `strf`: the first strl whose strh begins `auds` is the track, its stream index its position among all strl
// lists; `LIST movi` chunk by chunk, nested LISTs (`rec `) entered to a depth of 8; `##wb` chunks whose two hex digits are the track's
// index are payload, everything else is stepped over by its size with the odd-size pad byte.  Serial byte parsing per stream, no
// per-sample work, no HIP; header-only.  The input is untrusted: every size is checked against the bytes that hold it before it is used.
//
// The reference has the whole file and walks it twice; this walker sees it once, in pieces, so a container's end is the smallest declared
// end of the containers around it, and the file's own end is only known at finish().  A chunk that runs past its container is what the
// reference calls truncated: a LIST is entered for the bytes that are there and ends its parents with it, a leaf is dropped and ends its
// parents.  A file cut inside a chunk gives the complete chunks in front of it and never the partial one.
// Kept: the unparsed tail (less than 12 bytes once a call returns), the `hdrl` list while it arrives and the one `##wb` chunk that is
// arriving.  `movi` is never buffered whole.
// Beyond the reference: `hdrl` may buffer at most 16 MiB (a text of this project's own); a refusal keeps the packets that were complete
// in front of it and is sticky; a `movi` list in front of any `hdrl` that names an audio stream is `AVI has no audio stream` (the
// reference would find a header behind it).  What the format tag means is the caller's business (avi.py, pipeline.cpp: avi_open).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <deque>
#include <functional>
#include <string>
#include <utility>
#include <vector>

namespace sk_avi {

constexpr size_t kMaxInputChunkBytes = 4u * 1024 * 1024;
constexpr uint64_t kMaxChunks = 1000000;                   // per container, as for_each_riff_chunk counts them
constexpr uint64_t kMaxPayloadBytes = 512ull * 1024 * 1024;
constexpr uint64_t kMaxHeaderBytes = 16ull * 1024 * 1024;  // this project's bound
constexpr int kMaxDepth = 8;

inline uint32_t le32(const uint8_t *d) { return (uint32_t)d[0] | ((uint32_t)d[1] << 8) | ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 24); }
inline uint16_t le16(const uint8_t *d) { return (uint16_t)(d[0] | (d[1] << 8)); }

// looks_like_avi
inline bool sniff(const uint8_t *d, size_t n) { return n >= 12 && std::memcmp(d, "RIFF", 4) == 0 && std::memcmp(d + 8, "AVI ", 4) == 0; }

// avi_stream_id: two hex digits, -1 where a byte is none
inline int stream_id(const uint8_t *d) {
    int value = 0;
    for (int i = 0; i < 2; ++i) {
        const uint8_t b = d[i];
        int digit;
        if (b >= '0' && b <= '9') digit = b - '0';
        else if (b >= 'A' && b <= 'F') digit = b - 'A' + 10;
        else if (b >= 'a' && b <= 'f') digit = b - 'a' + 10;
        else return -1;
        value = value * 16 + digit;
    }
    return value;
}

// for_each_riff_chunk over bytes that are all there (the `hdrl` list): "" or the reference's text
using Visit = std::function<std::string(const uint8_t *id, const uint8_t *payload, size_t len)>;
inline std::string for_each_chunk(const uint8_t *d, size_t n, const Visit &visit) {
    size_t offset = 0;
    uint64_t chunks = 0;
    while (offset + 8 <= n) {
        if (++chunks > kMaxChunks) return "AVI chunk count exceeds budget";
        const uint8_t *id = d + offset;
        const size_t length = le32(d + offset + 4), start = offset + 8;
        if (length > n - start) {  // truncated: a LIST shows what is there, a leaf is dropped
            if (std::memcmp(id, "LIST", 4) == 0 && n - start >= 4) return visit(id, d + start, n - start);
            return "";
        }
        const std::string text = visit(id, d + start, length);
        if (!text.empty()) return text;
        offset = start + length + (length & 1);
    }
    for (size_t i = offset; i < n; ++i)
        if (d[i] != 0) return "AVI chunk table has trailing data";
    return "";
}

struct Config {
    uint32_t stream_index = 0, sample_rate = 0;
    uint16_t format_tag = 0;
    uint8_t channels = 0, bits = 0;
};

struct Packet {
    std::vector<uint8_t> data;
};

struct Demuxer {
    struct Level {
        uint64_t end = 0;      // absolute offset where the container's bytes end: the smallest declared end around it
        uint64_t chunks = 0;
        uint8_t pad = 0;       // the pad byte behind it (its declared length was odd)
        bool clipped = false;  // its declared end lies behind its parent's: the parent ends with it
        bool movi = false;     // `movi` or a LIST inside it: `##wb` chunks are collected here
        int depth = 0;
    };
    std::vector<uint8_t> buffer;
    size_t cursor = 0;
    uint64_t pos = 0;  // absolute offset of buffer[cursor]
    std::vector<Level> stack;
    uint64_t forms = 0, skip_left = 0, collect_left = 0, payload_total = 0;
    bool return_after_skip = false, collecting_hdrl = false, collected_clipped = false, ended = false;
    uint8_t collected_pad = 0;
    std::string fail_after_skip;
    std::vector<uint8_t> current;
    uint32_t strl_seen = 0;

    bool configured = false, failed = false;
    Config config;
    std::deque<Packet> packets;
    size_t queued = 0;
    std::string error;

    bool fail(const std::string &text) {
        if (!failed) error = text;
        failed = true;
        return false;
    }
    size_t buffered() const { return buffer.size() - cursor + current.size(); }
    Packet take_packet() {
        Packet p = std::move(packets.front());
        packets.pop_front();
        queued -= p.data.size();
        return p;
    }

    bool add(const uint8_t *d, size_t n) {
        if (failed) return false;
        if (n > kMaxInputChunkBytes) return fail("AVI input chunk exceeds the " + std::to_string(kMaxInputChunkBytes) + " byte streaming budget");
        if (ended) return true;
        if (n) buffer.insert(buffer.end(), d, d + n);
        return parse_available();
    }

    // the file ends here: what is incomplete is dropped, as the reference drops it from a prefix
    bool finish() {
        if (failed) return false;
        if (!parse_available()) return false;
        if (!ended) {
            const size_t avail = buffer.size() - cursor;
            if (collect_left && collecting_hdrl) {  // a truncated `hdrl` LIST shows what is there
                collect_left = 0;
                if (!parse_hdrl()) return false;
            } else if (!skip_left && !collect_left && !stack.empty()) {
                // a container's walk ends where no further 8-byte header fits: what is left must be zeros.  (12 bytes of a LIST's head
                // that never came whole: a truncated LIST with no type, which is not entered)
                const uint64_t left = stack.back().end - pos;
                if (avail < 8 || left < 8)
                    for (size_t i = 0; i < avail; ++i)
                        if (buffer[cursor + i] != 0) return fail("AVI chunk table has trailing data");
            }
            ended = true;
            buffer.clear();
            cursor = 0;
            current.clear();
        }
        if (!configured) return fail("AVI has no audio stream");
        return true;
    }

    void advance(size_t n) { cursor += n, pos += n; }

    // the innermost container's walk is over: it goes, with every parent that ends with it; behind the last one its pad byte is skipped
    void leave_level() {
        while (!stack.empty()) {
            const Level x = stack.back();
            stack.pop_back();
            if (!x.clipped) {
                skip_left = stack.empty() ? x.pad : std::min<uint64_t>(x.pad, stack.back().end - pos);
                return;
            }
        }
    }

    bool parse_available() {
        while (!failed && !ended) {
            const size_t avail = buffer.size() - cursor;
            if (skip_left) {
                const size_t take = (size_t)std::min<uint64_t>(skip_left, avail);
                advance(take);
                skip_left -= take;
                if (skip_left) break;
                if (!fail_after_skip.empty()) return fail(fail_after_skip);
                if (return_after_skip) {
                    return_after_skip = false;
                    leave_level();
                }
                continue;
            }
            if (collect_left) {
                const size_t take = (size_t)std::min<uint64_t>(collect_left, avail);
                current.insert(current.end(), buffer.begin() + (ptrdiff_t)cursor, buffer.begin() + (ptrdiff_t)(cursor + take));
                advance(take);
                collect_left -= take;
                if (collect_left) break;
                if (collecting_hdrl) {
                    if (!parse_hdrl()) return false;
                } else {
                    Packet p;
                    p.data.swap(current);
                    payload_total += p.data.size();
                    queued += p.data.size();
                    packets.push_back(std::move(p));
                }
                current.clear();
                if (collected_clipped) leave_level();
                else skip_left = std::min<uint64_t>(collected_pad, stack.back().end - pos);
                continue;
            }
            const uint8_t *d = buffer.data() + cursor;
            if (stack.empty()) {  // for_each_avi_riff: the next form
                if (avail < 12) break;
                if (std::memcmp(d, "RIFF", 4) != 0) {
                    if (forms == 0) return fail("AVI contains data outside a RIFF form");
                    ended = true;  // what follows the forms is not looked at
                    break;
                }
                forms += 1;
                const uint32_t length = le32(d + 4);
                if (std::memcmp(d + 8, "AVI ", 4) != 0 && std::memcmp(d + 8, "AVIX", 4) != 0) return fail("invalid AVI RIFF form type");
                Level form;
                form.end = std::max<uint64_t>(pos + 8 + length, pos + 12), form.pad = (uint8_t)(length & 1);
                stack.push_back(form);
                advance(12);
                continue;
            }
            Level &level = stack.back();
            const uint64_t left = level.end - pos;
            if (left < 8) {  // no further header fits: zeros, or the reference's text
                if (avail < left) break;
                for (size_t i = 0; i < left; ++i)
                    if (d[i] != 0) return fail("AVI chunk table has trailing data");
                advance((size_t)left);
                leave_level();
                continue;
            }
            if (avail < 8) break;
            const bool list = std::memcmp(d, "LIST", 4) == 0;
            const uint64_t length = le32(d + 4), start = pos + 8;
            const bool clipped = start + length > level.end;
            const uint64_t size = clipped ? level.end - start : length;  // the payload bytes that belong to it
            if (list && size >= 4 && avail < 12) break;                   // its type
            if (++level.chunks > kMaxChunks) return fail("AVI chunk count exceeds budget");
            const uint8_t pad = (uint8_t)(length & 1);
            auto step_over = [&] {  // a chunk nothing is taken from
                advance(8);
                skip_left = clipped ? size : std::min<uint64_t>(size + pad, level.end - start);
                return_after_skip = clipped;
                if (skip_left == 0 && clipped) return_after_skip = false, leave_level();
            };
            if (!level.movi) {  // a form's own chunks: its lists are looked at
                if (!list || (clipped && size < 4)) {
                    step_over();
                    continue;
                }
                if (size < 4) return fail("AVI LIST type is truncated");
                const uint8_t *kind = d + 8;
                if (std::memcmp(kind, "hdrl", 4) == 0 && !configured) {
                    if (size - 4 > kMaxHeaderBytes) return fail("AVI hdrl list exceeds the " + std::to_string(kMaxHeaderBytes) + " byte header budget");
                    advance(12);
                    current.clear();
                    collecting_hdrl = true, collected_clipped = clipped, collected_pad = pad;
                    collect_left = size - 4;
                    if (collect_left == 0) {  // an empty list names no stream
                        collecting_hdrl = false;
                        if (clipped) leave_level();
                        else skip_left = std::min<uint64_t>(pad, stack.back().end - pos);
                    }
                    continue;
                }
                if (std::memcmp(kind, "movi", 4) == 0) {
                    if (!configured) return fail("AVI has no audio stream");
                    Level movi;
                    movi.end = start + size, movi.pad = pad, movi.clipped = clipped, movi.movi = true, movi.depth = 0;
                    advance(12);
                    stack.push_back(movi);
                    continue;
                }
                step_over();
                continue;
            }
            // collect_avi_audio_chunks
            if (list && size >= 4) {
                if (level.depth + 1 > kMaxDepth) return fail("AVI record nesting exceeds budget");
                Level rec;
                rec.end = start + size, rec.pad = pad, rec.clipped = clipped, rec.movi = true, rec.depth = level.depth + 1;
                advance(12);
                stack.push_back(rec);
                continue;
            }
            if (!clipped && d[2] == 'w' && d[3] == 'b' && stream_id(d) >= 0 && (uint32_t)stream_id(d) == config.stream_index) {
                if (payload_total + length > kMaxPayloadBytes) {  // refused once it has come whole; a file that ends inside it ends quietly
                    step_over();
                    skip_left = length;
                    fail_after_skip = "AVI audio payload exceeds budget";
                    continue;
                }
                advance(8);
                current.clear();
                collecting_hdrl = false, collected_clipped = false, collected_pad = pad;
                collect_left = length;  // (an empty chunk adds nothing and gives no packet)
                continue;
            }
            step_over();
        }
        if (failed || ended) {
            buffer.clear();
            cursor = 0;
        } else if (cursor > 64 * 1024 || cursor == buffer.size()) {
            buffer.erase(buffer.begin(), buffer.begin() + (ptrdiff_t)cursor);
            cursor = 0;
        }
        return !failed;
    }

    // parse_avi_audio_format's visit of one `hdrl` list, with parse_avi_stream_list
    bool parse_hdrl() {
        collecting_hdrl = false;
        std::vector<uint8_t> list;
        list.swap(current);
        const std::string text = for_each_chunk(list.data(), list.size(), [&](const uint8_t *id, const uint8_t *payload, size_t len) -> std::string {
            if (std::memcmp(id, "LIST", 4) != 0 || len < 4 || std::memcmp(payload, "strl", 4) != 0) return "";
            const uint32_t this_stream = strl_seen++;
            if (configured) return "";
            bool audio = false, have_wave = false;
            std::vector<uint8_t> wave;
            const std::string inner = for_each_chunk(payload + 4, len - 4, [&](const uint8_t *cid, const uint8_t *p, size_t n) -> std::string {
                if (std::memcmp(cid, "strh", 4) == 0) audio = n >= 4 && std::memcmp(p, "auds", 4) == 0;
                else if (std::memcmp(cid, "strf", 4) == 0) wave.assign(p, p + n), have_wave = true;
                return "";
            });
            if (!inner.empty()) return inner;
            if (!audio) return "";
            if (!have_wave) return "AVI audio stream has no strf format";
            if (wave.size() < 16) return "AVI WAVEFORMAT is truncated";
            const uint16_t channels = le16(wave.data() + 2);
            if (channels == 0 || channels > 255) return "AVI channel count is invalid";
            const uint32_t rate = le32(wave.data() + 4);
            if (rate == 0) return "AVI sample rate is zero";
            config.stream_index = this_stream, config.format_tag = le16(wave.data()), config.channels = (uint8_t)channels;
            config.sample_rate = rate, config.bits = (uint8_t)std::min<uint16_t>(le16(wave.data() + 14), 255);
            configured = true;
            return "";
        });
        if (!text.empty()) return fail(text);
        return true;
    }
};

}  // namespace sk_avi

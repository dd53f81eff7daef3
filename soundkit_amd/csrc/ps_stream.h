// MPEG program stream (.vob, .mpg), audio only, on the host: what soundkit-decoder's decode_mpeg_ps_audio reads (soundkit-decoder/src/
// lib.rs:572-804: find_start_code, parse_mpeg_pes_payload, parse_dvd_lpcm_header, and the block sizes of unpack_dvd_lpcm) as one
// incremental walk with its checks, budget and texts.  Start codes 00 00 01 xx; the pack header BA is skipped by its own layout (MPEG-2:
// 14 bytes and its stuffing count, MPEG-1: 12 bytes), B9 is four bytes, every id from BB on has a 16-bit length and is stepped over by
// it; a video id with length 0 falls back to the scan for the next start code.  PES headers in the MPEG-2 and the MPEG-1 form.
// private_stream_1 (BD) whose payload begins A0 ... AF is DVD LPCM: four bytes, the 3-byte header, then sample bytes, which leave in
// whole blocks -- the remainder is carried from packet to packet.  Serial byte parsing per stream, no per-sample work, no HIP;
// header-only.  The input is untrusted: every size is checked against the bytes that hold it before it is used as an offset.
//
// Three decisions beyond the reference:
//   1. packets are walked by their length field; the reference rescans every payload for 00 00 01.  The same on any stream whose
//      payloads do not emulate a BD start code.
//   2. the substream id of the first LPCM packet is the track; the reference concatenates every A0 ... AF substream.
//   3. MPEG audio PES (C0 ... DF) is taken as a track: the stream id of the first such packet, its payloads the elementary stream.
// Which kind is the track: kTrackFirst -- the first audio packet of either kind decides (a stream cannot look ahead); kTrackLpcm --
// DVD LPCM alone, MPEG audio is stepped over like video (the reference's view of a file); kTrackMpegAudio -- the reverse.
// 20-bit DVD LPCM is refused with the reference's text at its first packet.  AC-3 / DTS substreams (80 ... 8F) are stepped over.
// A refusal keeps the packets that were complete in front of it and is sticky.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <deque>
#include <string>
#include <utility>
#include <vector>

namespace sk_ps {

constexpr size_t kMaxInputChunkBytes = 4u * 1024 * 1024;
constexpr uint64_t kMaxPayloadBytes = 512ull * 1024 * 1024;
enum : uint8_t { kTrackFirst = 0, kTrackLpcm = 1, kTrackMpegAudio = 2 };
enum : uint8_t { kKindNone = 0, kKindLpcm = 1, kKindMpegAudio = 2 };

// looks_like_mpeg_ps
inline bool sniff(const uint8_t *d, size_t n) { return n >= 4 && d[0] == 0 && d[1] == 0 && d[2] == 1 && d[3] == 0xBA; }

// parse_mpeg_pes_payload: 1 = *start is where the payload begins, 0 = the packet is ignored, -1 = *text
inline int pes_payload(const uint8_t *d, size_t n, size_t *start, std::string *text) {
    size_t cursor = 0;
    while (cursor < n && d[cursor] == 0xff) cursor += 1;
    if (cursor >= n) return 0;
    uint8_t first = d[cursor];
    if ((first & 0xc0) == 0x80) {
        if (n - cursor < 3) return *text = "MPEG-2 PES header is truncated", -1;
        cursor += 3 + (size_t)d[cursor + 2];
        if (cursor > n) return *text = "MPEG-2 PES optional header is truncated", -1;
    } else {
        if ((first & 0xc0) == 0x40) cursor += 2;
        if (cursor >= n) return *text = "MPEG-1 PES header is truncated", -1;
        first = d[cursor];
        if ((first & 0xf0) == 0x20) cursor += 5;
        else if ((first & 0xf0) == 0x30) cursor += 10;
        else if (first == 0x0f) cursor += 1;
        else return 0;
        if (cursor > n) return *text = "MPEG-1 PES timestamp is truncated", -1;
    }
    *start = cursor;
    return 1;
}

// the bytes of one block of sample bytes (unpack_dvd_lpcm)
inline uint32_t lpcm_block_bytes(uint32_t bits, uint32_t channels) {
    if (bits == 16) return 2 * channels;
    return channels == 1 || channels == 2 || channels == 4 ? 12 : (channels == 8 ? 24 : 12 * channels);
}

struct Config {
    uint8_t kind = kKindNone, stream_id = 0, substream_id = 0, channels = 0, bits = 0;
    uint32_t sample_rate = 0, block_bytes = 0;
};

struct Packet {
    std::vector<uint8_t> data;
};

struct Demuxer {
    explicit Demuxer(uint8_t track_mode = kTrackFirst) : mode(track_mode) {}
    uint8_t mode;
    std::vector<uint8_t> buffer;
    size_t cursor = 0;
    uint64_t skip_left = 0, payload_total = 0;
    std::vector<uint8_t> carry;  // sample bytes short of a block
    bool ended = false;

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
    size_t buffered() const { return buffer.size() - cursor + carry.size(); }
    Packet take_packet() {
        Packet p = std::move(packets.front());
        packets.pop_front();
        queued -= p.data.size();
        return p;
    }
    // an id whose packets are read, not stepped over
    bool wanted(uint8_t id) const {
        if (id == 0xBD) return mode != kTrackMpegAudio && config.kind != kKindMpegAudio;
        if (id >= 0xC0 && id <= 0xDF) return mode != kTrackLpcm && config.kind != kKindLpcm && (config.kind == kKindNone || id == config.stream_id);
        return false;
    }

    bool add(const uint8_t *d, size_t n) {
        if (failed) return false;
        if (n > kMaxInputChunkBytes) return fail("MPEG-PS input chunk exceeds the " + std::to_string(kMaxInputChunkBytes) + " byte streaming budget");
        if (ended) return true;
        if (n) buffer.insert(buffer.end(), d, d + n);
        return parse_available(false);
    }
    bool finish() {
        if (failed) return false;
        if (!ended) {
            if (!parse_available(true)) return false;
            ended = true;
            buffer.clear();
            cursor = 0;
            if (!carry.empty())
                return fail(config.bits == 16 ? "DVD LPCM ends with a partial sample block" : "DVD LPCM ends with a partial 24-bit sample block");
        }
        if (!configured) return fail("MPEG-PS has no supported DVD LPCM track");
        return true;
    }

    void emit(const uint8_t *d, size_t n) {
        if (!n) return;
        Packet p;
        p.data.assign(d, d + n);
        queued += n;
        packets.push_back(std::move(p));
    }

    bool parse_available(bool end) {
        while (!failed) {
            size_t avail = buffer.size() - cursor;
            if (skip_left) {
                const size_t take = (size_t)std::min<uint64_t>(skip_left, avail);
                cursor += take;
                skip_left -= take;
                if (skip_left) break;
                continue;
            }
            const uint8_t *d = buffer.data() + cursor;
            if (avail < 4) break;  // (a start code needs its id: find_start_code)
            if (d[0] != 0 || d[1] != 0 || d[2] != 1) {  // the scan; the last bytes may begin a start code
                size_t i = 1;
                while (i + 3 <= avail && !(d[i] == 0 && d[i + 1] == 0 && d[i + 2] == 1)) i += 1;
                cursor += i;
                continue;
            }
            const uint8_t id = d[3];
            if (id == 0xBA) {  // the pack header, by its own layout
                if (avail < 5) break;
                if ((d[4] & 0xc0) == 0x40) {
                    if (avail < 14) break;
                    skip_left = 14 + (size_t)(d[13] & 7);
                } else if ((d[4] & 0xf0) == 0x20) {
                    skip_left = 12;
                } else {
                    skip_left = 4;  // neither layout: the scan goes on behind the code
                }
                continue;
            }
            if (id < 0xBB) {  // B9, and the codes of a video elementary stream
                skip_left = 4;
                continue;
            }
            const bool want = wanted(id);
            if (avail < 6) {
                if (end && want) return fail("MPEG-PS PES length is truncated");
                break;
            }
            const size_t length = ((size_t)d[4] << 8) | d[5];
            if (!want) {
                skip_left = (id >= 0xE0 && id <= 0xEF && length == 0) ? 4 : 6 + (uint64_t)length;
                continue;
            }
            if (avail < 6 + length) {
                if (end) return fail("MPEG-PS PES packet is truncated");
                break;
            }
            if (!parse_pes(id, d + 6, length)) return false;
            cursor += 6 + length;
        }
        if (failed) {
            buffer.clear();
            cursor = 0;
        } else if (cursor > 64 * 1024 || cursor == buffer.size()) {
            buffer.erase(buffer.begin(), buffer.begin() + (ptrdiff_t)cursor);
            cursor = 0;
        }
        return !failed;
    }

    bool parse_pes(uint8_t id, const uint8_t *d, size_t n) {
        size_t start = 0;
        std::string text;
        const int rc = pes_payload(d, n, &start, &text);
        if (rc < 0) return fail(text);
        if (rc == 0) return true;
        const uint8_t *payload = d + start;
        const size_t len = n - start;
        if (id != 0xBD) {  // MPEG audio: the payloads one after the other are the elementary stream
            if (len == 0) return true;
            if (!configured) {
                config.kind = kKindMpegAudio, config.stream_id = id;
                configured = true;
            }
            if (payload_total + len > kMaxPayloadBytes) return fail("MPEG-PS audio payload exceeds budget");
            payload_total += len;
            emit(payload, len);
            return true;
        }
        if (len < 7 || payload[0] < 0xA0 || payload[0] > 0xAF) return true;  // AC-3, DTS, subpictures
        if (configured && payload[0] != config.substream_id) return true;
        // parse_dvd_lpcm_header on the three bytes behind the substream's four
        const uint8_t *h = payload + 4;
        const uint32_t bits = 16 + ((h[1] >> 6) & 3) * 4;
        if (bits != 16 && bits != 20 && bits != 24) return fail("unsupported DVD LPCM sample depth " + std::to_string(bits));
        static const uint32_t rates[4] = {48000, 96000, 44100, 32000};
        const uint32_t rate = rates[(h[1] >> 4) & 3], channels = (h[1] & 7) + 1u;
        if (configured) {
            if (bits != config.bits || rate != config.sample_rate || channels != config.channels) return fail("DVD LPCM format changes mid-stream");
        } else {
            if (bits == 20) return fail("20-bit DVD LPCM decoding is not implemented");
            config.kind = kKindLpcm, config.stream_id = id, config.substream_id = payload[0];
            config.bits = (uint8_t)bits, config.sample_rate = rate, config.channels = (uint8_t)channels;
            config.block_bytes = lpcm_block_bytes(bits, channels);
            configured = true;
        }
        const uint8_t *samples = payload + 7;
        const size_t n_samples = len - 7;
        if (payload_total + n_samples > kMaxPayloadBytes) return fail("MPEG-PS audio payload exceeds budget");
        payload_total += n_samples;
        // whole blocks leave, the remainder waits for the next packet
        carry.insert(carry.end(), samples, samples + n_samples);
        const size_t whole = carry.size() / config.block_bytes * config.block_bytes;
        if (whole) {
            emit(carry.data(), whole);
            carry.erase(carry.begin(), carry.begin() + (ptrdiff_t)whole);
        }
        return true;
    }
};

}  // namespace sk_ps

// MPEG transport stream (.ts, HLS segments, Blu-ray .m2ts), audio only, on the host: the incremental walk of soundkit-audio-demux's
// MpegTsAudioDemuxer (soundkit-audio-demux/src/lib.rs:4196-5330) with its checks, budgets and texts -- packet layout detection (five
// syncs at stride 188, at 192 behind a 4-byte prefix, or at 204), resynchronisation byte by byte, the transport-error / scrambling /
// adaptation-field refusals, the continuity counter per PID (a duplicate is dropped, a gap clears the current PES and the PSI
// assembler), PSI section assembly with CRC-32/MPEG-2, PAT (lowest non-zero program, version tracking), PMT (the first stream
// ts_stream_codec knows), PES headers with 33-bit timestamps unwrapped, and the emitters: one packet per ADTS frame, per MPEG audio
// frame, per LOAS frame, per Blu-ray LPCM PES.  Serial byte parsing per stream, no per-sample work, no HIP; header-only.  The input is
// untrusted: every size is checked against the bytes that hold it before it is used as an offset.
//
// Kept: the unparsed tail of the input (less than five packets once a call returns), the current PES (1 MiB at most) and the PSI
// sections being assembled (1 KiB each).  Packets of every other PID are stepped over one by one.
// Beyond the reference: a refusal keeps the packets that were complete in front of it (there the events of the refused call are
// lost, which would make the output depend on how the bytes are cut); it is sticky.  DTS (stream type 0x82) is reported and every PES
// payload handed out whole -- the core-frame parser is not built, and no decoder here takes DTS.  The 4-byte Blu-ray LPCM header is read
// here (bytes 0-1: big-endian size of what follows; byte 2: channel assignment, rate code; byte 3, top two bits: depth code); stereo at
// 16 or 24 bits is built, everything else is refused with a text of this project's own.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <deque>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace sk_ts {

constexpr size_t kMaxInputChunkBytes = 4u * 1024 * 1024;  // MAX_CONTAINER_INPUT_CHUNK_BYTES
constexpr size_t kMaxPesBytes = 1u * 1024 * 1024;         // MAX_MPEG_TS_PES_BYTES
enum : uint8_t { kCodecNone = 0, kCodecAac = 1, kCodecPcm = 2, kCodecAc3 = 3, kCodecDts = 4, kCodecMp3 = 5, kCodecMp1 = 6, kCodecMp2 = 7, kCodecMpegAudio = 8 };
enum : uint8_t { kFormatRaw = 0, kFormatAdts = 1, kFormatLatm = 2 };

inline const char *codec_name(uint8_t codec) {  // AudioCodec::as_str
    static const char *const names[] = {"unknown", "aac", "pcm", "ac3", "dts", "mp3", "mp1", "mp2", "mpeg-audio"};
    return codec <= kCodecMpegAudio ? names[codec] : "unknown";
}

// looks_like_mpeg_ts of the decoder crate (soundkit-decoder/src/lib.rs:849): three syncs at stride 188, or at 192 behind 4 bytes
inline bool sniff(const uint8_t *d, size_t n) {
    auto at = [&](size_t stride, size_t prefix) {
        for (size_t k = 0; k < 3; ++k)
            if (prefix + k * stride >= n || d[prefix + k * stride] != 0x47) return false;
        return true;
    };
    return at(188, 0) || at(192, 4);
}

struct Layout {
    uint16_t stride = 0, prefix = 0;
};

// detect_ts_layout: five syncs
inline bool detect_layout(const uint8_t *d, size_t n, Layout *out) {
    static const Layout kinds[3] = {{188, 0}, {192, 4}, {204, 0}};
    for (const Layout &l : kinds) {
        if (n < (size_t)l.stride * 5) continue;
        bool all = true;
        for (size_t k = 0; k < 5 && all; ++k) all = d[l.prefix + k * l.stride] == 0x47;
        if (all) {
            *out = l;
            return true;
        }
    }
    return false;
}

inline uint32_t crc32_mpeg2(const uint8_t *d, size_t n) {
    uint32_t crc = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) {
        crc ^= (uint32_t)d[i] << 24;
        for (int b = 0; b < 8; ++b) crc = (crc & 0x80000000u) ? (crc << 1) ^ 0x04C11DB7u : crc << 1;
    }
    return crc;
}

inline bool descriptors_have_tag(const uint8_t *d, size_t n, uint8_t target) {
    while (n >= 2) {
        const size_t len = d[1];
        if (n < 2 + len) return false;
        if (d[0] == target) return true;
        d += 2 + len, n -= 2 + len;
    }
    return false;
}

inline bool descriptors_have_registration(const uint8_t *d, size_t n, const char *target) {
    while (n >= 2) {
        const size_t len = d[1];
        if (n < 2 + len) return false;
        if (d[0] == 0x05 && len >= 4 && std::memcmp(d + 2, target, 4) == 0) return true;
        d += 2 + len, n -= 2 + len;
    }
    return false;
}

// ts_stream_codec
inline bool stream_codec(uint8_t stream_type, const uint8_t *program, size_t program_len, const uint8_t *es, size_t es_len, uint8_t *codec, uint8_t *format) {
    *format = kFormatRaw;
    switch (stream_type) {
    case 0x0f: *codec = kCodecAac, *format = kFormatAdts; return true;
    case 0x11: *codec = kCodecAac, *format = kFormatLatm; return true;
    case 0x03:
    case 0x04: *codec = kCodecMpegAudio; return true;
    case 0x81:
    case 0x87: *codec = kCodecAc3; return true;
    case 0x80: *codec = kCodecPcm; return true;
    case 0x82: *codec = kCodecDts; return true;
    case 0x06:
        if (descriptors_have_tag(es, es_len, 0x6A) || descriptors_have_registration(es, es_len, "AC-3")) {
            *codec = kCodecAc3;
            return true;
        }
        if (descriptors_have_registration(program, program_len, "HDMV")) {  // FFmpeg's M2TS mode: AAC as private PES
            *codec = kCodecAac, *format = kFormatAdts;
            return true;
        }
        return false;
    default: return false;
    }
}

struct MpegAudioHeader {
    size_t frame_length;
    uint32_t sample_rate, samples_per_frame;
    uint8_t channels, layer;
};

// parse_mpeg_audio_header
inline bool parse_mpeg_audio_header(const uint8_t *d, size_t n, MpegAudioHeader *h) {
    if (n < 4 || d[0] != 0xff || (d[1] & 0xe0) != 0xe0) return false;
    const unsigned version_bits = (d[1] >> 3) & 3, layer_bits = (d[1] >> 1) & 3;
    if (version_bits == 1 || layer_bits == 0) return false;
    const unsigned layer = 4 - layer_bits, bitrate_index = d[2] >> 4, rate_index = (d[2] >> 2) & 3;
    if (bitrate_index == 0 || bitrate_index == 15 || rate_index == 3) return false;
    static const uint16_t kbps[5][14] = {{32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384, 416, 448},
                                         {32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384},
                                         {32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320},
                                         {32, 48, 56, 64, 80, 96, 112, 128, 144, 160, 176, 192, 224, 256},
                                         {8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160}};
    const bool mpeg1 = version_bits == 3;
    const unsigned row = mpeg1 ? layer - 1 : (layer == 1 ? 3 : 4);
    static const uint32_t base[3] = {44100, 48000, 32000};
    const uint32_t rate = version_bits == 3 ? base[rate_index] : (version_bits == 2 ? base[rate_index] / 2 : base[rate_index] / 4);
    const uint32_t bitrate = (uint32_t)kbps[row][bitrate_index - 1] * 1000, padding = (d[2] >> 1) & 1;
    if (layer == 1) h->frame_length = (12 * bitrate / rate + padding) * 4, h->samples_per_frame = 384;
    else if (layer == 2 || mpeg1) h->frame_length = 144 * bitrate / rate + padding, h->samples_per_frame = 1152;
    else h->frame_length = 72 * bitrate / rate + padding, h->samples_per_frame = 576;
    h->sample_rate = rate, h->channels = (d[3] >> 6) == 3 ? 1 : 2, h->layer = (uint8_t)layer;
    return true;
}

struct AdtsHeader {
    size_t frame_length;
    uint32_t sample_rate, samples_per_frame;
    uint8_t channels;
};

// parse_adts_header
inline bool parse_adts_header(const uint8_t *d, size_t n, AdtsHeader *h) {
    static const uint32_t rates[13] = {96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 7350};
    if (n < 7 || d[0] != 0xff || (d[1] & 0xf0) != 0xf0 || (d[1] & 0x06) != 0) return false;
    const unsigned index = (d[2] & 0x3c) >> 2;
    if (index >= 13) return false;
    h->sample_rate = rates[index];
    h->channels = (uint8_t)(((d[2] & 1) << 2) | ((d[3] & 0xc0) >> 6));
    h->frame_length = ((size_t)(d[3] & 3) << 11) | ((size_t)d[4] << 3) | (d[5] >> 5);
    if (h->frame_length < 7) return false;
    h->samples_per_frame = 1024 * ((uint32_t)(d[6] & 3) + 1);
    return true;
}

// parse_pes_timestamp; false: `invalid or truncated MPEG-TS PES timestamp`
inline bool parse_pes_timestamp(const uint8_t *d, size_t n, uint64_t *out) {
    if (n < 5 || !(d[0] & 1) || !(d[2] & 1) || !(d[4] & 1)) return false;
    *out = ((uint64_t)((d[0] >> 1) & 7) << 30) | ((uint64_t)d[1] << 22) | ((uint64_t)(d[2] >> 1) << 15) | ((uint64_t)d[3] << 7) | (uint64_t)(d[4] >> 1);
    return true;
}

// PsiSectionAssembler
struct PsiAssembler {
    std::vector<uint8_t> bytes;
    size_t expected = 0;  // 0: the three header bytes are not all there yet
    void reset() {
        bytes.clear();
        expected = 0;
    }
    bool append(const uint8_t *d, size_t n, std::vector<std::vector<uint8_t>> *done, std::string *error) {
        while (n) {
            if (bytes.empty() && d[0] == 0xff) return true;  // stuffing up to the packet's end
            if (!expected) {
                const size_t take = std::min<size_t>(3 - bytes.size(), n);
                bytes.insert(bytes.end(), d, d + take);
                d += take, n -= take;
                if (bytes.size() < 3) return true;
                const size_t want = 3 + ((((size_t)bytes[1] & 0x0f) << 8) | bytes[2]);
                if (want < 4 || want > 1024) {
                    reset();
                    *error = "PSI section size " + std::to_string(want) + " is out of range";
                    return false;
                }
                expected = want;
            }
            const size_t take = std::min(expected - bytes.size(), n);
            bytes.insert(bytes.end(), d, d + take);
            d += take, n -= take;
            if (bytes.size() == expected) {
                done->push_back(std::move(bytes));
                bytes.clear();
                expected = 0;
            }
        }
        return true;
    }
    bool push(const uint8_t *d, size_t n, bool unit_start, std::vector<std::vector<uint8_t>> *done, std::string *error) {
        if (unit_start) {
            if (n == 0) {
                *error = "truncated PSI pointer field";
                return false;
            }
            const size_t pointer = d[0];
            d += 1, n -= 1;
            if (pointer > n) {
                *error = "PSI pointer exceeds payload";
                return false;
            }
            if (!bytes.empty()) {
                if (!append(d, pointer, done, error)) return false;
                if (!bytes.empty()) {
                    *error = "PSI pointer starts a new section before the previous section ends";
                    return false;
                }
            }
            d += pointer, n -= pointer;
        }
        return append(d, n, done, error);
    }
};

struct Config {
    uint8_t codec = kCodecNone, format = kFormatRaw, stream_type = 0, channels = 0;
    bool has_rate = false, has_channels = false, lpcm = false;
    uint16_t pid = 0, program = 0, stride = 0, prefix = 0;
    uint32_t sample_rate = 0;
    uint32_t bits = 0, bytes_per_frame = 0, frames_per_packet = 0;  // Blu-ray LPCM alone
    uint8_t lpcm_header[4] = {0, 0, 0, 0};
};

struct Packet {
    std::vector<uint8_t> data;
    uint64_t pts = 0, dts = 0;
    uint32_t duration = 0;
    bool has_pts = false, has_dts = false, has_duration = false, discontinuity = false;
    uint8_t continuity = 0, codec = kCodecNone;
};

struct Demuxer {
    std::vector<uint8_t> buffer;
    size_t cursor = 0;
    bool have_layout = false;
    Layout layout;
    int32_t pmt_pid = -1, audio_pid = -1, selected_program = -1, pat_version = -1, pmt_version = -1;
    uint8_t audio_codec = kCodecNone, packet_format = kFormatRaw, stream_type = 0;
    bool have_codec = false;
    std::vector<uint8_t> current_pes;
    uint8_t pes_continuity = 0;
    bool pes_discontinuity = false;
    int8_t continuity[8192];
    uint64_t pts_epoch = 0, last_raw_pts = 0;
    bool have_last_pts = false;
    std::map<uint16_t, PsiAssembler> psi;
    bool has_rate = false, has_channels = false;
    uint32_t sample_rate = 0;
    uint8_t channels = 0;

    bool configured = false, failed = false;
    Config config;
    std::deque<Packet> packets;
    size_t queued = 0;
    std::string error;

    Demuxer() { std::memset(continuity, -1, sizeof continuity); }

    bool fail(const std::string &text) {
        if (!failed) error = text;
        failed = true;
        return false;
    }
    size_t buffered() const { return buffer.size() - cursor + current_pes.size(); }
    size_t queued_bytes() const { return queued; }
    Packet take_packet() {
        Packet p = std::move(packets.front());
        packets.pop_front();
        queued -= p.data.size();
        return p;
    }

    bool add(const uint8_t *d, size_t n) {
        if (failed) return false;
        if (n > kMaxInputChunkBytes) return fail("MPEG-TS input chunk exceeds the " + std::to_string(kMaxInputChunkBytes) + " byte streaming budget");
        if (n) buffer.insert(buffer.end(), d, d + n);
        return parse_available();
    }
    bool finish() {
        if (failed) return false;
        return parse_available() && flush_pes();
    }

    // parse_available_packets
    bool parse_available() {
        for (;;) {
            const size_t remaining = buffer.size() - cursor;
            if (!have_layout) {
                if (detect_layout(buffer.data() + cursor, remaining, &layout)) {
                    have_layout = true;
                } else if (remaining >= 204 * 5) {
                    cursor += 1;
                    continue;
                } else {
                    break;
                }
            }
            if (remaining < layout.stride) break;
            const size_t sync = cursor + layout.prefix;
            if (buffer[sync] != 0x47 || sync + 188 > buffer.size()) {
                have_layout = false;
                cursor += 1;
                continue;
            }
            uint8_t packet[188];
            std::memcpy(packet, buffer.data() + sync, 188);
            cursor += layout.stride;
            if (!parse_packet(packet)) break;
        }
        if (cursor > 64 * 1024 || cursor == buffer.size()) {
            buffer.erase(buffer.begin(), buffer.begin() + (ptrdiff_t)cursor);
            cursor = 0;
        }
        return !failed;
    }

    bool parse_packet(const uint8_t *packet) {
        if (packet[1] & 0x80) return fail("MPEG-TS packet has the transport-error indicator");
        if (packet[3] & 0xC0) return fail("scrambled MPEG-TS packets are unsupported");
        const bool unit_start = (packet[1] & 0x40) != 0;
        const uint16_t pid = (uint16_t)(((packet[1] & 0x1f) << 8) | packet[2]);
        const unsigned afc = (packet[3] & 0x30) >> 4;
        const uint8_t cc = packet[3] & 0x0f;
        if (afc == 0) return fail("MPEG-TS packet has reserved adaptation-field control");
        if (afc == 2) return true;
        size_t start = 4;
        bool discontinuity = false;
        if (afc == 3) {
            const size_t len = packet[4], end = 5 + len;
            if (end > 188) return fail("MPEG-TS adaptation field exceeds its packet");
            if (len > 0) discontinuity = (packet[5] & 0x80) != 0;
            start = end;
        }
        if (start >= 188) return true;
        const int previous = continuity[pid];
        continuity[pid] = (int8_t)cc;
        if (previous >= 0) {
            if (cc == previous) return true;  // a duplicate
            if (cc != ((previous + 1) & 0x0f) && !discontinuity) {
                discontinuity = true;
                if ((int32_t)pid == audio_pid) current_pes.clear();
            }
        }
        if (discontinuity) {
            auto it = psi.find(pid);
            if (it != psi.end()) it->second.reset();
        }
        const uint8_t *payload = packet + start;
        const size_t n = 188 - start;
        if (pid == 0 || (int32_t)pid == pmt_pid) {
            const bool pat = pid == 0;
            std::vector<std::vector<uint8_t>> done;
            std::string text;
            if (!psi[pid].push(payload, n, unit_start, &done, &text)) return fail(text);
            for (const std::vector<uint8_t> &section : done)
                if (!(pat ? parse_pat(section) : parse_pmt(section))) return false;
        } else if ((int32_t)pid == audio_pid) {
            if (unit_start) {
                if (!flush_pes()) return false;
                current_pes.clear();
                pes_discontinuity = discontinuity;
                pes_continuity = cc;
            }
            pes_discontinuity |= discontinuity;
            if (current_pes.size() + n > kMaxPesBytes) return fail("MPEG-TS PES exceeds the " + std::to_string(kMaxPesBytes) + " byte packet budget");
            current_pes.insert(current_pes.end(), payload, payload + n);
        }
        return true;
    }

    bool parse_pat(const std::vector<uint8_t> &s) {
        if (s.size() < 12 || s[0] != 0x00) return true;
        const size_t end = 3 + ((((size_t)s[1] & 0x0f) << 8) | s[2]);
        if (end > s.size() || end < 12) return true;
        if (crc32_mpeg2(s.data(), end) != 0) return fail("MPEG-TS PSI CRC mismatch");
        if (!(s[5] & 1)) return true;
        const int version = (s[5] >> 1) & 0x1f;
        if (pat_version == version) return true;
        int32_t program = -1, pid = -1;
        for (size_t pos = 8; pos + 4 <= end - 4; pos += 4) {
            const int32_t number = (s[pos] << 8) | s[pos + 1];
            if (number != 0 && (program < 0 || number < program)) program = number, pid = ((s[pos + 2] & 0x1f) << 8) | s[pos + 3];
        }
        if (program >= 0) {
            if (pmt_pid != pid) {
                audio_pid = -1, pmt_version = -1;
                have_codec = false;
                audio_codec = kCodecNone, packet_format = kFormatRaw, stream_type = 0;
            }
            selected_program = program, pmt_pid = pid, pat_version = version;
        }
        return true;
    }

    bool parse_pmt(const std::vector<uint8_t> &s) {
        if (s.size() < 16 || s[0] != 0x02) return true;
        const size_t end = 3 + ((((size_t)s[1] & 0x0f) << 8) | s[2]);
        if (end > s.size() || end < 16) return true;
        if (crc32_mpeg2(s.data(), end) != 0) return fail("MPEG-TS PSI CRC mismatch");
        if (!(s[5] & 1)) return true;
        const int version = (s[5] >> 1) & 0x1f;
        if (pmt_version == version) return true;
        if (selected_program >= 0 && selected_program != ((s[3] << 8) | s[4])) return true;
        const size_t info_len = (((size_t)s[10] & 0x0f) << 8) | s[11], entries_end = end - 4, program_end = 12 + info_len;
        if (program_end > entries_end) return fail("MPEG-TS PMT program descriptors exceed their section");
        for (size_t pos = program_end; pos + 5 <= entries_end;) {
            const uint8_t type = s[pos];
            const int32_t pid = ((s[pos + 1] & 0x1f) << 8) | s[pos + 2];
            const size_t es_end = pos + 5 + ((((size_t)s[pos + 3] & 0x0f) << 8) | s[pos + 4]);
            if (es_end > entries_end) return fail("MPEG-TS PMT descriptor exceeds its section");
            uint8_t codec, format;
            if (stream_codec(type, s.data() + 12, info_len, s.data() + pos + 5, es_end - pos - 5, &codec, &format)) {
                if (audio_pid < 0) audio_pid = pid, audio_codec = codec, packet_format = format, stream_type = type, have_codec = true;
                pmt_version = version;
                break;
            }
            pos = es_end;
        }
        return true;
    }

    // ensure_config
    void ensure_config(bool rate_known, uint32_t rate, bool channels_known, uint8_t ch) {
        if (configured) return;
        if (rate_known) has_rate = true, sample_rate = rate;
        if (channels_known) has_channels = true, channels = ch;
        config.codec = audio_codec, config.format = packet_format, config.stream_type = stream_type;
        config.pid = (uint16_t)audio_pid, config.program = (uint16_t)(selected_program < 0 ? 0 : selected_program);
        config.stride = layout.stride, config.prefix = layout.prefix;
        config.has_rate = has_rate, config.sample_rate = sample_rate, config.has_channels = has_channels, config.channels = channels;
        configured = true;
    }

    void push(const uint8_t *d, size_t n, bool has_pts, uint64_t pts, bool has_dts, uint64_t dts, bool has_duration, uint32_t duration, bool discontinuity,
              uint8_t codec) {
        Packet p;
        p.data.assign(d, d + n);
        p.has_pts = has_pts, p.pts = pts, p.has_dts = has_dts, p.dts = dts, p.has_duration = has_duration, p.duration = duration;
        p.discontinuity = discontinuity, p.continuity = pes_continuity, p.codec = codec;
        queued += n;
        packets.push_back(std::move(p));
    }

    // flush_current_pes with parse_pes
    bool flush_pes() {
        if (current_pes.empty()) return true;
        std::vector<uint8_t> pes;
        pes.swap(current_pes);
        if (pes.size() < 9 || pes[0] != 0 || pes[1] != 0 || pes[2] != 1) return fail("invalid MPEG-TS PES header");
        const size_t start = 9 + (size_t)pes[8];
        if (start > pes.size()) return fail("MPEG-TS PES optional header is truncated");
        const unsigned flags = (pes[7] >> 6) & 3;
        bool has_pts = false, has_dts = false;
        uint64_t pts = 0, dts = 0;
        if (flags & 2) {
            if (!parse_pes_timestamp(pes.data() + 9, pes.size() - 9, &pts)) return fail("invalid or truncated MPEG-TS PES timestamp");
            has_pts = true;
        }
        if (flags == 3) {
            if (pes.size() < 14 || !parse_pes_timestamp(pes.data() + 14, pes.size() - 14, &dts)) return fail("invalid or truncated MPEG-TS PES timestamp");
            has_dts = true;
        } else {
            has_dts = has_pts, dts = pts;
        }
        const size_t declared = ((size_t)pes[4] << 8) | pes[5];
        const size_t end = declared == 0 ? pes.size() : std::min(6 + declared, pes.size());
        if (end < start) return fail("MPEG-TS PES length ends inside its header");
        if (has_pts) {  // expand_pts
            if (have_last_pts && last_raw_pts > pts && last_raw_pts - pts > (1ull << 32)) pts_epoch += 1ull << 33;
            last_raw_pts = pts, have_last_pts = true;
            pts += pts_epoch;
        }
        if (has_dts) dts = flags == 3 ? pts_epoch + dts : pts;
        if (!have_codec) return true;
        const uint8_t *payload = pes.data() + start;
        const size_t n = end - start;
        if (stream_type == 0x80) return emit_lpcm(payload, n, has_pts, pts, has_dts, dts);
        if (packet_format == kFormatAdts) return emit_adts(payload, n, has_pts, pts, has_dts, dts);
        if (packet_format == kFormatLatm) return emit_loas(payload, n, has_pts, pts, has_dts, dts);
        if (stream_type == 0x03 || stream_type == 0x04) return emit_mpeg_audio(payload, n, has_pts, pts, has_dts, dts);
        ensure_config(false, 0, false, 0);  // AC-3, and DTS whole
        if (n) push(payload, n, has_pts, pts, has_dts, dts, false, 0, pes_discontinuity, audio_codec);
        return true;
    }

    bool emit_lpcm(const uint8_t *d, size_t n, bool has_pts, uint64_t pts, bool has_dts, uint64_t dts) {
        if (n < 4) return fail("Blu-ray LPCM access unit of " + std::to_string(n) + " bytes is shorter than its 4-byte header");
        const size_t size = ((size_t)d[0] << 8) | d[1];
        if (size != n - 4) return fail("Blu-ray LPCM size field " + std::to_string(size) + " disagrees with the " + std::to_string(n - 4) + " payload bytes");
        const unsigned assignment = d[2] >> 4, rate_code = d[2] & 0x0f, depth_code = d[3] >> 6;
        const uint32_t rate = rate_code == 1 ? 48000 : (rate_code == 4 ? 96000 : (rate_code == 5 ? 192000 : 0));
        if (!rate) return fail("unsupported Blu-ray LPCM rate code " + std::to_string(rate_code));
        if (depth_code == 0) return fail("unsupported Blu-ray LPCM depth code 0");
        if (assignment == 1) return fail("mono Blu-ray LPCM (channel assignment 1, with its pad channel) is not built");
        if (assignment != 3) return fail("Blu-ray LPCM channel assignment " + std::to_string(assignment) + " is not built: stereo alone is");
        if (depth_code == 2) return fail("20-bit Blu-ray LPCM is not built");
        const uint32_t bits = depth_code == 1 ? 16 : 24, frame_bytes = bits / 8 * 2;
        if (size % frame_bytes) return fail("Blu-ray LPCM payload of " + std::to_string(size) + " bytes is no whole number of " + std::to_string(frame_bytes) + "-byte frames");
        const uint32_t frames = (uint32_t)(size / frame_bytes);
        audio_codec = kCodecPcm;
        has_rate = has_channels = true, sample_rate = rate, channels = 2;
        if (!configured) {
            ensure_config(true, rate, true, 2);
            config.lpcm = true, config.bits = bits, config.bytes_per_frame = frame_bytes, config.frames_per_packet = frames;
            std::memcpy(config.lpcm_header, d, 4);
        }
        push(d + 4, size, has_pts, pts, has_dts, dts, true, (uint32_t)((uint64_t)frames * 90000 / rate), pes_discontinuity, kCodecPcm);
        return true;
    }

    bool emit_adts(const uint8_t *d, size_t n, bool has_pts, uint64_t pts, bool has_dts, uint64_t dts) {
        size_t pos = 0;
        uint64_t index = 0;
        while (pos + 7 <= n) {
            if (d[pos] != 0xff || (d[pos + 1] & 0xf0) != 0xf0) {
                pos += 1;
                continue;
            }
            AdtsHeader h;
            if (!parse_adts_header(d + pos, n - pos, &h) || pos + h.frame_length > n) break;  // a partial tail is dropped
            ensure_config(true, h.sample_rate, true, h.channels);
            const uint32_t duration = (uint32_t)(90000ull * h.samples_per_frame / h.sample_rate);
            const uint64_t offset = (uint64_t)duration * index;
            push(d + pos, h.frame_length, has_pts, pts + offset, has_dts, dts + offset, true, duration, pes_discontinuity && index == 0, kCodecAac);
            index += 1;
            pos += h.frame_length;
        }
        return true;
    }

    bool emit_mpeg_audio(const uint8_t *d, size_t n, bool has_pts, uint64_t pts, bool has_dts, uint64_t dts) {
        size_t pos = 0;
        uint64_t offset = 0;
        while (pos + 4 <= n) {
            MpegAudioHeader h;
            if (!parse_mpeg_audio_header(d + pos, n - pos, &h)) {
                pos += 1;
                continue;
            }
            if (pos + h.frame_length > n) return fail("MPEG audio frame is truncated at the PES boundary");
            const uint8_t codec = h.layer == 3 ? kCodecMp3 : (h.layer == 1 ? kCodecMp1 : kCodecMp2);
            if (!configured) audio_codec = codec;
            ensure_config(true, h.sample_rate, true, h.channels);
            const uint32_t duration = (uint32_t)((uint64_t)h.samples_per_frame * 90000 / h.sample_rate);
            push(d + pos, h.frame_length, has_pts, pts + offset, has_dts, dts + offset, true, duration, pes_discontinuity && offset == 0, codec);
            offset += duration;
            pos += h.frame_length;
        }
        for (size_t i = pos; i < n; ++i)
            if (d[i] != 0xff) return fail("MPEG audio PES ends with an incomplete frame");
        return true;
    }

    bool emit_loas(const uint8_t *d, size_t n, bool has_pts, uint64_t pts, bool has_dts, uint64_t dts) {
        size_t pos = 0;
        bool first = true;
        while (pos + 3 <= n) {
            if (d[pos] != 0x56 || (d[pos + 1] & 0xe0) != 0xe0) {
                pos += 1;
                continue;
            }
            const size_t length = 3 + ((((size_t)d[pos + 1] & 0x1f) << 8) | d[pos + 2]);
            if (pos + length > n) return fail("LOAS/LATM access unit is truncated at the PES boundary");
            ensure_config(false, 0, false, 0);
            push(d + pos, length, has_pts, pts, has_dts, dts, false, 0, pes_discontinuity && first, kCodecAac);
            first = false;
            pos += length;
        }
        for (size_t i = pos; i < n; ++i)
            if (d[i] != 0xff) return fail("LOAS/LATM PES ends with an incomplete access unit");
        return true;
    }
};

}  // namespace sk_ts

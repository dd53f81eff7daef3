// mp4_stream.h -- ISO base media (MP4 / M4A / fragmented MP4) on the host, audio only: the box header, the `moov` parser for the first
// audio track whose codec is built here (`mp4a` -> AAC, `alac`, `fLaC`, the PCM entries), the streaming demuxer in its two layouts (soundkit-audio-demux/src/lib.rs:
// RegularMp4AudioDemuxer 1400-1678, the fragment walk of Mp4MediaDemuxer 1846-2299), the whole-file sample index (Mp4MediaIndex,
// 925-1080), the edit-list trim of a decoded packet (resolve_pcm_packet_trim, 117-174) and the 7-byte ADTS header an AAC sample is
// wrapped in (create_adts_header, 4102-4120).  Serial byte parsing per stream, no per-sample work, no HIP; header-only.  The input is
// untrusted: every read is bounds-checked, every count is checked against the bytes that hold it before anything is reserved.
//
// One demuxer serves both layouts.  The reference collects 8 KiB, classifies the layout (classify_mp4_layout, 702 ff.: a `moof` first or
// a `moov` that holds `mvex` is fragmented, any other `moov` regular) and then builds one of two demuxers; here the same rule is applied
// at the first `moov` or `moof` the top-level walk meets, so nothing is collected for detection and an `mdat` in front of `moov` is
// refused from its 8-byte header.  Not read: `ctts` and `stss` (audio samples present in decode order and are all sync samples), every
// edit but the first media edit, the `ulaw` / `alaw` / `ima4` / `raw ` QuickTime entries, `chan` layouts, video.  `fLaC` and the PCM entries
// (`sowt twos in24 in32 fl32 fl64 lpcm`, sound descriptions of version 0, 1 and 2) are decoded out of regular files only: a fragmented file with
// such a track is described, and decode_file refuses it.  A PCM track's samples leave as runs of frames (build_constant_pcm_runs,
// coalesce_pcm_runs), the same runs from the index and from the demuxer.  A QuickTime `wave` atom is looked into for `esds` / `alac` /
// `enda` / `dfLa` as the reference does.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

namespace sk_mp4 {

constexpr uint64_t kMaxMetadataBytes = 64ull * 1024 * 1024;  // MAX_MP4_METADATA_BYTES
constexpr uint32_t kMaxPacketBytes = 128u * 1024 * 1024;     // MAX_MEDIA_PACKET_BYTES
constexpr size_t kMaxUnits = 8000000;                        // MAX_MP4_MATERIALIZED_ACCESS_UNITS
constexpr size_t kMaxInputChunkBytes = 4u * 1024 * 1024;     // MAX_CONTAINER_INPUT_CHUNK_BYTES
constexpr uint8_t kCodecAac = 1, kCodecAlac = 2, kCodecFlac = 3, kCodecPcm = 4;
constexpr uint32_t kMaxPcmRunFrames = 4096, kMaxPcmRunBytes = 1024 * 1024;  // MAX_PCM_PACKET_FRAMES, MAX_PCM_PACKET_BYTES

inline uint32_t be16(const uint8_t *p) { return (uint32_t)p[0] << 8 | p[1]; }
inline uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
inline uint64_t be64(const uint8_t *p) { return (uint64_t)be32(p) << 32 | be32(p + 4); }

struct BoxHeader {
    char name[5] = {0, 0, 0, 0, 0};
    uint64_t size = 0;
    uint32_t header = 0;
    bool is(const char *n) const { return std::memcmp(name, n, 4) == 0; }
};

// Mp4BoxHeader::read: false when the header is not complete yet -- or can never be: size 0, a size below the header
inline bool read_box(const uint8_t *d, size_t n, BoxHeader *h) {
    if (n < 8) return false;
    const uint64_t small = be32(d);
    std::memcpy(h->name, d + 4, 4);
    if (small == 1) {
        if (n < 16) return false;
        h->size = be64(d + 8), h->header = 16;
    } else if (small == 0) {
        return false;
    } else {
        h->size = small, h->header = 8;
    }
    return h->size >= h->header;
}

// a byte range inside a parsed box
struct Span {
    const uint8_t *d = nullptr;
    size_t n = 0;
    bool u8(size_t at, uint32_t *v) const { return at < n ? (*v = d[at], true) : false; }
    bool u16(size_t at, uint32_t *v) const { return n >= 2 && at <= n - 2 ? (*v = be16(d + at), true) : false; }
    bool u32(size_t at, uint32_t *v) const { return n >= 4 && at <= n - 4 ? (*v = be32(d + at), true) : false; }
    bool u64(size_t at, uint64_t *v) const { return n >= 8 && at <= n - 8 ? (*v = be64(d + at), true) : false; }
};

// for_each_child_box: stops silently at the first child that is cut or invalid, as the reference does
template <class F>
inline bool each_child(Span s, F f) {
    size_t pos = 0;
    while (s.n - pos >= 8) {
        BoxHeader h;
        if (!read_box(s.d + pos, s.n - pos, &h) || h.size > s.n - pos) break;
        if (!f(h, Span{s.d + pos + h.header, (size_t)h.size - h.header})) return false;
        pos += (size_t)h.size;
    }
    return true;
}

struct Sample {
    uint64_t offset = 0, start = 0;  // absolute byte offset; decode time in the track's timescale
    uint32_t size = 0, duration = 0;
};

// a PCM sample entry (`sowt twos in24 in32 fl32 fl64 lpcm`): signed (or float), packed, interleaved samples of Track::bits bits
struct PcmEntry {
    char name[4] = {0, 0, 0, 0};  // the entry's name
    bool big_endian = false, is_float = false;
    uint32_t bytes_per_frame = 0, frames_per_packet = 0;  // 0: not stated
};

struct Track {
    uint8_t codec = 0;  // kCodecAac / kCodecAlac / kCodecFlac / kCodecPcm
    PcmEntry pcm;       // kCodecPcm
    uint32_t id = 0, timescale = 0, sample_rate = 0, channels = 0, bits = 0;
    std::vector<uint8_t> codec_private;  // AAC: the AudioSpecificConfig; ALAC: the `alac` child's payload (the cookie in its MP4 wrapping);
                                         // FLAC: `fLaC` and the metadata blocks of `dfLa` (normalize_flac_config); PCM: none
    bool has_edit = false;               // the first media edit, in the track's timescale
    uint64_t edit_presentation_start = 0, edit_media_start = 0, edit_duration = 0;
    bool fragmented = false;  // `moov` holds `mvex`, or the sample tables are empty: the samples come in `moof`s
    std::vector<Sample> samples;
};

struct TrexDefaults {
    uint32_t track = 0, description = 0, duration = 0, size = 0;  // 0: none
};

// ---- sample entry ------------------------------------------------------------------------------------------------------------------

// read_descriptor_len: 1 to 4 bytes, 7 bits each
inline bool descriptor_len(Span s, size_t at, size_t *len, size_t *used) {
    size_t v = 0;
    for (size_t i = 0; i < 4 && at + i < s.n; ++i) {
        v = v << 7 | (s.d[at + i] & 0x7fu);
        if (!(s.d[at + i] & 0x80u)) return *len = v, *used = i + 1, true;
    }
    return false;
}

// find_mpeg4_descriptor: ES_Descriptor (3) -> DecoderConfigDescriptor (4) -> DecoderSpecificInfo (5)
// *bad: a length that does not end within four bytes, or one that runs out of what holds it
inline bool find_descriptor(Span s, uint8_t tag, Span *out, bool *bad, int depth = 0) {
    size_t pos = 0;
    while (s.n - pos >= 2) {
        const uint8_t t = s.d[pos++];
        size_t len, used;
        if (!descriptor_len(s, pos, &len, &used)) return *bad = true, false;
        pos += used;
        if (len > s.n - pos) return *bad = true, false;
        const Span body{s.d + pos, len};
        if (t == tag) return *out = body, true;
        const size_t nested = t == 3 && len >= 3 ? 3 : t == 4 && len >= 13 ? 13 : 0;
        if (nested && depth < 4 && find_descriptor(Span{body.d + nested, len - nested}, tag, out, bad, depth + 1)) return true;
        if (*bad) return false;
        pos += len;
    }
    return false;
}

inline uint32_t rate_of_index(uint32_t i) {
    static const uint32_t rates[13] = {96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 7350};
    return i < 13 ? rates[i] : 0;
}

// parse_asc_audio_config: rate and channel configuration where the two-byte form states them
inline bool asc_rate_channels(const uint8_t *asc, size_t n, uint32_t *rate, uint32_t *channels) {
    if (n < 2) return false;
    const uint32_t r = rate_of_index(((asc[0] & 7u) << 1) | (asc[1] >> 7));
    if (!r) return false;
    return *rate = r, *channels = (asc[1] >> 3) & 15u, true;
}

// find_sample_entry_box: a child of the sample entry, also inside `wave` / `sinf` / `schi`
inline bool find_entry_child(Span s, const char *target, Span *out, int depth = 0) {
    size_t pos = 0;
    while (s.n - pos >= 8) {
        BoxHeader h;
        if (!read_box(s.d + pos, s.n - pos, &h) || h.size > s.n - pos) return false;
        const Span body{s.d + pos + h.header, (size_t)h.size - h.header};
        if (h.is(target)) return *out = body, true;
        if ((h.is("wave") || h.is("sinf") || h.is("schi")) && depth < 4 && find_entry_child(body, target, out, depth + 1)) return true;
        pos += (size_t)h.size;
    }
    return false;
}

// normalize_mp4_flac_decoder_configuration: what the FLAC decoder is fed before the packets -- `fLaC`, then the metadata blocks.  Taken:
// data that already begins with `fLaC`, a bare 34-byte STREAMINFO, a `dfLa` payload (version and flags, then the metadata blocks)
inline bool normalize_flac_config(const uint8_t *d, size_t n, std::vector<uint8_t> *out, std::string *error) {
    static const uint8_t magic[4] = {'f', 'L', 'a', 'C'}, head[4] = {0x80, 0, 0, 34};
    out->clear();
    if (n >= 4 && std::memcmp(d, magic, 4) == 0) return out->assign(d, d + n), true;
    out->assign(magic, magic + 4);
    if (n == 34) {
        out->insert(out->end(), head, head + 4);
        out->insert(out->end(), d, d + n);
        return true;
    }
    if (n < 4) return *error = "MP4 dfLa decoder configuration is truncated", false;
    const uint8_t *m = d + 4;
    const size_t mn = n - 4;
    if (mn < 38 || (m[0] & 0x7f) != 0) return *error = "MP4 dfLa has no leading FLAC STREAMINFO block", false;
    const size_t info = (size_t)m[1] << 16 | (size_t)m[2] << 8 | m[3];
    if (info != 34 || mn < 4 + info) return *error = "MP4 dfLa has an invalid FLAC STREAMINFO block", false;
    out->insert(out->end(), m, m + mn);
    return true;
}

// parse_stsd_audio, for the entries built here.  found = false: no such entry (the track is stepped over)
inline bool parse_stsd(Span s, Track *t, bool *found, std::string *error) {
    *found = false;
    uint32_t count;
    if (s.n < 16 || !s.u32(4, &count)) return *error = "MP4 stsd audio table is truncated", false;
    size_t pos = 8;
    for (uint32_t k = 0; k < count; ++k) {
        BoxHeader h;
        if (pos > s.n || !read_box(s.d + pos, s.n - pos, &h)) return *error = "MP4 stsd audio entry header is truncated", false;
        if (h.size > s.n - pos) return *error = "MP4 stsd audio entry is truncated", false;
        const Span e{s.d + pos + h.header, (size_t)h.size - h.header};
        pos += (size_t)h.size;
        const bool aac = h.is("mp4a"), alac = h.is("alac"), flac = h.is("fLaC");
        const bool sowt = h.is("sowt"), twos = h.is("twos"), lpcm = h.is("lpcm");
        const uint32_t fixed_bits = h.is("in24") ? 24 : h.is("in32") || h.is("fl32") ? 32 : h.is("fl64") ? 64 : 0;
        if ((!aac && !alac && !flac && !sowt && !twos && !lpcm && !fixed_bits) || e.n < 28) continue;
        uint32_t version = 0, channels = 0, bits = 0, rate = 0;
        (void)e.u16(8, &version), (void)e.u16(16, &channels), (void)e.u16(18, &bits), (void)e.u32(24, &rate);
        rate >>= 16;
        if (channels > 255) return *error = "QuickTime audio channel count exceeds u8", false;
        if (bits > 255) bits = 0;  // 0: not stated
        size_t children = 28;
        uint32_t bytes_per_frame = 0, frames_per_packet = 1, flags = 0;  // 0: not stated
        if (version == 1) {
            if (e.n < 44) return *error = "QuickTime version-one audio sample entry is truncated", false;
            children = 44;
            uint32_t bytes_per_sample = 0;
            (void)e.u32(28, &frames_per_packet), (void)e.u32(36, &bytes_per_frame), (void)e.u32(40, &bytes_per_sample);
            if (bits == 0 && bytes_per_sample < 32) bits = bytes_per_sample * 8;
        } else if (version == 2) {
            if (e.n < 64) return *error = "QuickTime version-two audio sample entry is truncated", false;
            children = 64;
            uint64_t rate_bits = 0;
            uint32_t bytes_per_packet = 0;
            (void)e.u64(32, &rate_bits), (void)e.u32(40, &channels), (void)e.u32(48, &bits), (void)e.u32(52, &flags);
            (void)e.u32(56, &bytes_per_packet), (void)e.u32(60, &frames_per_packet);
            double r;
            std::memcpy(&r, &rate_bits, 8);
            if (!(r > 0.0) || !(r <= 4294967295.0)) {  // (a NaN fails both)
                char text[80];
                std::snprintf(text, sizeof text, "invalid QuickTime version-two sample rate %g", r);
                return *error = text, false;
            }
            rate = (uint32_t)(r + 0.5);
            if (channels > 255) return *error = "QuickTime version-two channel count exceeds u8", false;
            if (bits > 255) return *error = "QuickTime version-two sample depth exceeds u8", false;
            bytes_per_frame = bytes_per_packet && frames_per_packet && bytes_per_packet % frames_per_packet == 0 ? bytes_per_packet / frames_per_packet : 0;
        } else if (version != 0) {
            return *error = "unsupported QuickTime audio sample-entry version " + std::to_string(version), false;
        }
        const Span rest{e.d + children, e.n - children};
        Span body;
        t->codec_private.clear();
        t->pcm = PcmEntry{};
        if (aac) {
            Span asc;
            bool bad = false;
            if (find_entry_child(rest, "esds", &body) && body.n >= 4 && find_descriptor(Span{body.d + 4, body.n - 4}, 5, &asc, &bad))
                t->codec_private.assign(asc.d, asc.d + asc.n);
            if (bad) return *error = "MP4 esds descriptor length runs past its box", false;
            (void)asc_rate_channels(t->codec_private.data(), t->codec_private.size(), &rate, &channels);
        }
        if (rate == 0 || channels == 0) return *error = "QuickTime audio sample entry has zero sample rate or channels", false;
        if (alac && find_entry_child(rest, "alac", &body)) t->codec_private.assign(body.d, body.d + body.n);
        if (flac) {
            body = Span{};
            (void)find_entry_child(rest, "dfLa", &body);
            if (!normalize_flac_config(body.d, body.n, &t->codec_private, error)) return false;
        }
        if (!aac && !alac && !flac) {
            bool have_enda = false, big = true;
            if (find_entry_child(rest, "enda", &body)) {
                uint32_t flag;
                if (!body.u16(0, &flag)) return *error = "QuickTime enda atom is truncated", false;
                if (flag > 1) return *error = "invalid QuickTime enda flag " + std::to_string(flag), false;
                have_enda = true, big = flag == 0;
            }
            PcmEntry &p = t->pcm;
            std::memcpy(p.name, h.name, 4);
            if (sowt || twos) {
                p.big_endian = twos;
            } else if (lpcm) {
                if (version != 2) return *error = "QuickTime lpcm requires a version-two sample entry", false;
                if (flags & 32u) return *error = "non-interleaved QuickTime LPCM is unsupported", false;
                p.big_endian = (flags & 2u) != 0, p.is_float = (flags & 1u) != 0;
                // the reference carries the three flags below and then reads every entry as signed, packed and low-aligned
                if (!p.is_float && !(flags & 4u)) return *error = "unsigned QuickTime LPCM is unsupported", false;
                if (!p.is_float && !(flags & 8u)) return *error = "unpacked QuickTime LPCM is unsupported", false;
                if (!p.is_float && (flags & 16u)) return *error = "aligned-high QuickTime LPCM is unsupported", false;
            } else {
                bits = fixed_bits;
                p.big_endian = have_enda ? big : true, p.is_float = h.is("fl32") || h.is("fl64");
            }
            if (bytes_per_frame == 0) bytes_per_frame = (bits + 7) / 8 * channels;
            p.bytes_per_frame = bytes_per_frame, p.frames_per_packet = frames_per_packet;
        }
        t->codec = aac ? kCodecAac : alac ? kCodecAlac : flac ? kCodecFlac : kCodecPcm;
        t->sample_rate = rate, t->channels = channels, t->bits = aac ? 0 : bits;
        *found = true;
        return true;
    }
    return true;
}

// ---- sample tables -----------------------------------------------------------------------------------------------------------------

struct Tables {
    bool have_id = false, have_timescale = false, audio = false, have_entry = false;
    std::vector<uint32_t> stts, stsc, sizes;  // stts: (count, duration) pairs; stsc: (first chunk, samples per chunk, description) triples
    uint32_t constant_size = 0, n_sizes = 0;
    std::vector<uint64_t> chunks;
    bool have_elst = false;
    uint64_t elst_duration = 0;  // of the first media edit, movie timescale; elst_empty: the empty edits in front of it
    uint64_t elst_empty = 0, elst_media = 0;
};

// validate_mp4_table_payload
inline bool table_fits(Span s, size_t header, uint32_t count, size_t entry, const char *name, std::string *error) {
    const uint64_t need = (uint64_t)header + (uint64_t)count * entry;
    if (s.n < need)
        return *error = std::string("MP4 ") + name + " declares " + std::to_string(count) + " entries requiring " + std::to_string(need) +
                        " bytes, but the box has " + std::to_string(s.n),
               false;
    return true;
}

inline bool parse_u32_table(Span s, size_t words, const char *name, std::vector<uint32_t> *out, std::string *error) {
    uint32_t count;
    if (!s.u32(4, &count)) return *error = std::string("MP4 ") + name + " header is truncated", false;
    if (!table_fits(s, 8, count, 4 * words, name, error)) return false;
    out->resize((size_t)count * words);
    for (size_t i = 0; i < out->size(); ++i) (*out)[i] = be32(s.d + 8 + 4 * i);
    return true;
}

inline bool parse_stts(Span s, Tables *t, std::string *error) {
    if (!parse_u32_table(s, 2, "stts", &t->stts, error)) return false;
    for (size_t i = 0; i < t->stts.size(); i += 2)
        if (t->stts[i] == 0) return *error = "MP4 stts contains a zero sample count", false;
    return true;
}

inline bool parse_stsc(Span s, Tables *t, std::string *error) {
    if (!parse_u32_table(s, 3, "stsc", &t->stsc, error)) return false;
    uint32_t previous = 0;
    for (size_t i = 0; i < t->stsc.size(); i += 3) {
        if (t->stsc[i] == 0 || t->stsc[i] <= previous) return *error = "MP4 stsc first_chunk values must increase from one", false;
        if (t->stsc[i + 1] == 0 || t->stsc[i + 2] == 0) return *error = "MP4 stsc contains a zero samples-per-chunk or description index", false;
        previous = t->stsc[i];
    }
    if (!t->stsc.empty() && t->stsc[0] != 1) return *error = "MP4 stsc must begin with chunk one", false;
    return true;
}

inline bool parse_stsz(Span s, Tables *t, std::string *error) {
    uint32_t size, count;
    if (!s.u32(4, &size) || !s.u32(8, &count)) return *error = "MP4 stsz header is truncated", false;
    t->sizes.clear();
    t->constant_size = size, t->n_sizes = count;
    if (size > 0) return true;
    if (!table_fits(s, 12, count, 4, "stsz", error)) return false;
    if (count > kMaxUnits)
        return *error = "MP4 stsz has " + std::to_string(count) + " variable-size samples; the materialized access-unit limit is " + std::to_string(kMaxUnits),
               false;
    t->sizes.resize(count);
    for (uint32_t i = 0; i < count; ++i) t->sizes[i] = be32(s.d + 12 + 4 * (size_t)i);
    return true;
}

inline bool parse_chunks(Span s, bool wide, Tables *t, std::string *error) {
    const char *name = wide ? "co64" : "stco";
    uint32_t count;
    if (!s.u32(4, &count)) return *error = std::string("MP4 ") + name + " header is truncated", false;
    if (!table_fits(s, 8, count, wide ? 8 : 4, name, error)) return false;
    t->chunks.resize(count);
    for (uint32_t i = 0; i < count; ++i) t->chunks[i] = wide ? be64(s.d + 8 + 8 * (size_t)i) : be32(s.d + 8 + 4 * (size_t)i);
    return true;
}

// parse_elst + resolve_media_timeline, kept to the first media edit: empty edits (media time -1) in front of it move its place on the
// presentation timeline; a rate other than 1 or another negative media time is refused
inline bool parse_elst(Span s, Tables *t, std::string *error) {
    uint32_t version, count;
    if (!s.u8(0, &version)) return *error = "MP4 elst box is truncated", false;
    if (!s.u32(4, &count)) return *error = "MP4 elst entry count is truncated", false;
    if (version > 1) return *error = "unsupported MP4 elst version " + std::to_string(version), false;
    const size_t entry = version == 1 ? 20 : 12;
    const uint64_t need = 8 + (uint64_t)count * entry;
    if (s.n < need) return *error = "MP4 elst expected " + std::to_string(need) + " bytes, got " + std::to_string(s.n), false;
    t->have_elst = false, t->elst_empty = 0;
    for (uint32_t k = 0; k < count; ++k) {
        const uint8_t *p = s.d + 8 + (size_t)k * entry;
        const uint64_t duration = version == 1 ? be64(p) : be32(p);
        const int64_t media = version == 1 ? (int64_t)be64(p + 8) : (int64_t)(int32_t)be32(p + 4);
        const uint8_t *r = p + (version == 1 ? 16 : 8);
        const int rate_int = (int16_t)be16(r), rate_frac = (int16_t)be16(r + 2);
        if (rate_int != 1 || rate_frac != 0)
            return *error = "unsupported MP4 edit rate " + std::to_string(rate_int) + "+" + std::to_string(rate_frac) + "/65536", false;
        if (media == -1) {
            if (t->elst_empty > UINT64_MAX - duration) return *error = "MP4 edit presentation time overflow", false;
            t->elst_empty += duration;
            continue;
        }
        if (media < 0) return *error = "unsupported MP4 edit media time " + std::to_string(media), false;
        t->have_elst = true, t->elst_duration = duration, t->elst_media = (uint64_t)media;
        return true;
    }
    if (count) return *error = "MP4 edit list contains no media edit", false;
    return true;
}

// scale_mp4_time: rounded to nearest
inline bool scale_time(uint64_t v, uint32_t from, uint32_t to, uint64_t *out, std::string *error) {
    const unsigned __int128 r = ((unsigned __int128)v * to + from / 2) / from;
    if (r > UINT64_MAX) return *error = "MP4 edit duration exceeds u64", false;
    return *out = (uint64_t)r, true;
}

// build_constant_pcm_samples: a PCM track whose `stsz` states one size and whose `stts` one duration.  A "sample" of such a track is a
// single frame; what is handed out is runs of them, cut at every chunk's end, after kMaxPcmRunFrames frames and before kMaxPcmRunBytes
// bytes.  No record per frame is ever made.  (build_samples has checked that `stsc` maps exactly n_sizes frames.)
inline bool build_constant_pcm_runs(const Tables &t, std::vector<Sample> *out, std::string *error) {
    const uint32_t size = t.constant_size, duration = t.stts[1];
    const uint32_t by_bytes = std::max(kMaxPcmRunBytes / size, 1u), by_duration = duration ? std::max(UINT32_MAX / duration, 1u) : kMaxPcmRunFrames;
    const uint32_t most = std::min(kMaxPcmRunFrames, std::min(by_bytes, by_duration));
    const uint64_t estimate = ((uint64_t)t.n_sizes + most - 1) / most + t.chunks.size();
    if (estimate > kMaxUnits) return *error = "PCM track requires more than " + std::to_string(kMaxUnits) + " indexed packet runs", false;
    out->clear();
    out->reserve((size_t)std::min<uint64_t>(estimate, t.n_sizes));
    size_t stsc_at = 0;
    uint64_t time = 0, frames = 0;
    for (size_t c = 0; c < t.chunks.size(); ++c) {
        while (stsc_at + 3 < t.stsc.size() && t.stsc[stsc_at + 3] <= c + 1) stsc_at += 3;
        uint32_t left = t.stsc[stsc_at + 1];
        uint64_t at = t.chunks[c];
        while (left > 0) {
            const uint32_t n = std::min(left, most);
            const uint64_t bytes = (uint64_t)size * n, ticks = (uint64_t)duration * n;
            if (bytes > UINT32_MAX) return *error = "PCM packet size overflow", false;
            if (ticks > UINT32_MAX) return *error = "PCM packet duration overflow", false;
            Sample s;
            s.offset = at, s.size = (uint32_t)bytes, s.duration = (uint32_t)ticks, s.start = time;
            out->push_back(s);
            if (at > UINT64_MAX - bytes) return *error = "PCM sample offset overflow", false;
            at += bytes;
            if (time > UINT64_MAX - ticks) return *error = "PCM sample timestamp overflow", false;
            time += ticks;
            frames += n, left -= n;
        }
    }
    if (frames != t.n_sizes)
        return *error = "MP4 stsc maps " + std::to_string(frames) + " PCM frames, but stsz describes " + std::to_string(t.n_sizes), false;
    return true;
}

// coalesce_regular_pcm_samples: neighbours that are contiguous in bytes and in time merge, up to kMaxPcmRunFrames ticks and
// kMaxPcmRunBytes bytes a run (the reference counts a run's frames by its duration; so does this)
inline void coalesce_pcm_runs(std::vector<Sample> *samples) {
    size_t n = 0;
    for (const Sample &s : *samples) {
        Sample *cur = n ? &(*samples)[n - 1] : nullptr;
        if (cur && cur->offset + cur->size == s.offset && cur->start + cur->duration == s.start &&
            (uint64_t)cur->duration + s.duration <= kMaxPcmRunFrames && (uint64_t)cur->size + s.size <= kMaxPcmRunBytes) {
            cur->size += s.size, cur->duration += s.duration;
        } else {
            (*samples)[n++] = s;
        }
    }
    samples->resize(n);
    samples->shrink_to_fit();
}

// build_regular_samples; pcm: the samples of a PCM track leave as runs of frames
inline bool build_samples(const Tables &t, bool pcm, std::vector<Sample> *out, std::string *error) {
    if (t.n_sizes == 0) return *error = "MP4 audio track is missing stsz sample sizes", false;
    if (t.chunks.empty()) return *error = "MP4 audio track is missing stco/co64 chunk offsets", false;
    if (t.stsc.empty()) return *error = "MP4 audio track is missing stsc sample-to-chunk table", false;
    const uint64_t n = t.n_sizes;
    uint64_t timed = 0;
    for (size_t i = 0; i < t.stts.size(); i += 2) timed += t.stts[i];
    if (timed != n) return *error = "MP4 stts describes " + std::to_string(timed) + " samples, but stsz describes " + std::to_string(n), false;
    for (size_t i = 0; i < t.stsc.size(); i += 3)
        if (t.stsc[i + 2] != 1) return *error = "MP4 stsc references a sample description other than the parsed first entry", false;
    const uint64_t n_chunks = t.chunks.size();
    unsigned __int128 mapped = 0;
    for (size_t i = 0; i < t.stsc.size(); i += 3) {
        const uint64_t first = t.stsc[i];
        if (first > n_chunks) return *error = "MP4 stsc references a chunk beyond stco/co64", false;
        const uint64_t end = i + 3 < t.stsc.size() ? t.stsc[i + 3] : n_chunks + 1;
        mapped += (unsigned __int128)(end - first) * t.stsc[i + 1];
    }
    if (mapped != n) {
        const std::string m = mapped > UINT64_MAX ? std::string("more than 2^64") : std::to_string((uint64_t)mapped);
        return *error = "MP4 stsc maps " + m + " samples, but stsz describes " + std::to_string(n), false;
    }
    if (pcm && t.constant_size && t.stts.size() == 2) return build_constant_pcm_runs(t, out, error);
    if (n > kMaxUnits) return *error = "MP4 track has " + std::to_string(n) + " access units; the materialized limit is " + std::to_string(kMaxUnits), false;
    out->clear();
    out->reserve((size_t)n);
    size_t stsc_at = 0, stts_at = 0;
    uint32_t stts_left = t.stts.empty() ? 0 : t.stts[0];
    uint64_t time = 0;
    for (uint64_t c = 0; c < n_chunks && out->size() < n; ++c) {
        while (stsc_at + 3 < t.stsc.size() && t.stsc[stsc_at + 3] <= c + 1) stsc_at += 3;
        uint64_t at = t.chunks[(size_t)c];
        for (uint32_t k = 0; k < t.stsc[stsc_at + 1] && out->size() < n; ++k) {
            const uint32_t size = t.constant_size ? t.constant_size : t.sizes[out->size()];
            if (size > kMaxPacketBytes) return *error = "MP4 sample exceeds the " + std::to_string(kMaxPacketBytes) + " byte packet budget", false;
            while (stts_left == 0) {  // timed == n: an entry is left
                stts_at += 2;
                stts_left = t.stts[stts_at];
            }
            const uint32_t duration = t.stts[stts_at + 1];
            stts_left -= 1;
            Sample s;
            s.offset = at, s.size = size, s.duration = duration, s.start = time;
            out->push_back(s);
            if (at > UINT64_MAX - size) return *error = "MP4 sample offset overflow", false;
            at += size;
            if (time > UINT64_MAX - duration) return *error = "MP4 sample timestamp overflow", false;
            time += duration;
        }
    }
    if (out->size() != n)
        return *error = "MP4 sample tables described " + std::to_string(n) + " samples but only " + std::to_string(out->size()) + " were mapped to chunks", false;
    if (pcm) coalesce_pcm_runs(out);
    return true;
}

// one `trak`: tables from tkhd, edts/elst, mdia/mdhd, hdlr and stbl.  chosen = false: not an audio track, or no sample entry built here
inline bool parse_trak(Span trak, bool have_movie_timescale, uint32_t movie_timescale, Track *track, bool *chosen, std::string *error) {
    *chosen = false;
    Tables t;
    Track tr;
    struct Walk {
        Tables &t;
        Track &tr;
        std::string *error;
        bool run(Span s, int depth) {
            return each_child(s, [&](const BoxHeader &h, Span p) -> bool {
                uint32_t version = 0;
                if (h.is("tkhd")) {
                    if (p.u8(0, &version)) t.have_id = p.u32(version == 1 ? 20 : 12, &tr.id);
                } else if (h.is("mdhd")) {
                    if (p.u8(0, &version)) t.have_timescale = p.u32(version == 1 ? 20 : 12, &tr.timescale);
                } else if (h.is("hdlr")) {
                    t.audio |= p.n >= 12 && std::memcmp(p.d + 8, "soun", 4) == 0;
                } else if (h.is("elst")) {
                    return parse_elst(p, &t, error);
                } else if (h.is("stsd")) {
                    return parse_stsd(p, &tr, &t.have_entry, error);
                } else if (h.is("stts")) {
                    return parse_stts(p, &t, error);
                } else if (h.is("stsc")) {
                    return parse_stsc(p, &t, error);
                } else if (h.is("stsz")) {
                    return parse_stsz(p, &t, error);
                } else if (h.is("stco") || h.is("co64")) {
                    return parse_chunks(p, h.is("co64"), &t, error);
                } else if ((h.is("edts") || h.is("mdia") || h.is("minf") || h.is("stbl")) && depth < 8) {
                    return run(p, depth + 1);
                }
                return true;
            });
        }
    } walk{t, tr, error};
    if (!walk.run(trak, 0)) return false;
    if (!t.audio || !t.have_entry) return true;
    if (!t.have_id) return *error = "MP4 audio track is missing tkhd track id", false;
    if (!t.have_timescale) return *error = "MP4 audio track has no timescale", false;
    if (tr.timescale == 0) return *error = "MP4 track " + std::to_string(tr.id) + " has zero timescale", false;
    if (t.have_elst) {
        if (!have_movie_timescale || movie_timescale == 0) return *error = "MP4 edit list requires a non-zero movie timescale", false;
        tr.has_edit = true, tr.edit_media_start = t.elst_media;
        if (!scale_time(t.elst_duration, movie_timescale, tr.timescale, &tr.edit_duration, error)) return false;
        if (!scale_time(t.elst_empty, movie_timescale, tr.timescale, &tr.edit_presentation_start, error)) return false;
    }
    tr.fragmented = t.n_sizes == 0 && t.chunks.empty() && t.stsc.empty();
    if (!tr.fragmented && !build_samples(t, tr.codec == kCodecPcm, &tr.samples, error)) return false;
    *track = std::move(tr);
    *chosen = true;
    return true;
}

// `moov`: the movie timescale, `mvex` and its `trex` defaults, and the first audio track with a codec built here
inline bool parse_moov(Span moov, Track *track, std::vector<TrexDefaults> *trex, std::string *error) {
    bool have_movie = false, mvex = false;
    uint32_t movie_timescale = 0;
    trex->clear();
    if (!each_child(moov, [&](const BoxHeader &h, Span p) -> bool {
            uint32_t version = 0;
            if (h.is("mvhd")) {
                if (p.u8(0, &version)) have_movie = p.u32(version == 1 ? 20 : 12, &movie_timescale);
            } else if (h.is("mvex")) {
                mvex = true;
                return each_child(p, [&](const BoxHeader &c, Span q) -> bool {
                    if (!c.is("trex")) return true;
                    if (q.n < 24) return *error = "fragmented MP4 trex box is truncated", false;
                    if (trex->size() >= 65536) return *error = "fragmented MP4 has more than 65536 trex boxes", false;
                    trex->push_back(TrexDefaults{be32(q.d + 4), be32(q.d + 8), be32(q.d + 12), be32(q.d + 16)});
                    return true;
                });
            }
            return true;
        }))
        return false;
    bool chosen = false;
    if (!each_child(moov, [&](const BoxHeader &h, Span p) -> bool {
            if (chosen || !h.is("trak")) return true;
            return parse_trak(p, have_movie, movie_timescale, track, &chosen, error);
        }))
        return false;
    if (!chosen) return *error = "MP4 source has no supported audio track", false;
    if (mvex) track->fragmented = true;
    return true;
}

// ---- fragments ---------------------------------------------------------------------------------------------------------------------

// one `traf` (parse_traf): its samples when it belongs to `track`, and where its data ends (the next traf's inherited base offset)
inline bool parse_traf(Span traf, const Track &track, const std::vector<TrexDefaults> &trex, uint64_t moof_start, bool have_inherited, uint64_t inherited,
                       std::vector<Sample> *out, uint64_t *data_end, std::string *error) {
    bool have_tfhd = false;
    uint32_t flags = 0, id = 0, description = 0, def_duration = 0, def_size = 0;
    bool have_base = false, have_description = false, have_duration = false, have_size = false;
    uint64_t base = 0, decode_time = 0;
    std::vector<Span> truns;
    if (!each_child(traf, [&](const BoxHeader &h, Span p) -> bool {
            if (h.is("tfhd")) {
                if (p.n < 8) return *error = "fragmented MP4 tfhd box is truncated", false;
                flags = be32(p.d) & 0xffffffu, id = be32(p.d + 4);
                size_t pos = 8;
                have_base = have_description = have_duration = have_size = false;
                if (flags & 1) {
                    if (!p.u64(pos, &base)) return *error = "fragmented MP4 tfhd base data offset is truncated", false;
                    have_base = true, pos += 8;
                }
                if (flags & 2) {
                    if (!p.u32(pos, &description)) return *error = "fragmented MP4 tfhd sample description index is truncated", false;
                    have_description = true, pos += 4;
                }
                if (flags & 8) {
                    if (!p.u32(pos, &def_duration)) return *error = "fragmented MP4 tfhd sample duration is truncated", false;
                    have_duration = true, pos += 4;
                }
                if (flags & 0x10) {
                    if (!p.u32(pos, &def_size)) return *error = "fragmented MP4 tfhd sample size is truncated", false;
                    have_size = true;
                }
                have_tfhd = true;
            } else if (h.is("tfdt")) {
                uint32_t v32 = 0;
                decode_time = 0;
                if (p.n >= 8 && p.d[0] == 1) (void)p.u64(4, &decode_time);
                else if (p.n >= 8 && p.d[0] == 0 && p.u32(4, &v32)) decode_time = v32;
            } else if (h.is("trun")) {
                if (truns.size() >= 65536) return *error = "fragmented MP4 traf has more than 65536 trun boxes", false;
                truns.push_back(p);
            }
            return true;
        }))
        return false;
    if (!have_tfhd) return *error = "fragmented MP4 traf is missing tfhd", false;
    const bool mine = id == track.id;
    for (const TrexDefaults &d : trex) {
        if (d.track != id) continue;
        if (!have_description) description = d.description ? d.description : 1, have_description = true;
        if (!have_duration && d.duration) def_duration = d.duration, have_duration = true;
        if (!have_size && d.size) def_size = d.size, have_size = true;
        break;
    }
    if (!have_description) description = 1;
    if (mine && description != 1)
        return *error = "fragmented MP4 track " + std::to_string(id) + " references unsupported sample description " + std::to_string(description), false;
    const uint64_t base_offset = have_base ? base : (flags & 0x020000u) ? moof_start : have_inherited ? inherited : moof_start;
    uint64_t fallback = base_offset, time = decode_time, total = 0;
    for (const Span &p : truns) {
        if (p.n < 8) return *error = "fragmented MP4 trun box is truncated", false;
        if (p.d[0] > 1) return *error = "unsupported fragmented MP4 trun version " + std::to_string(p.d[0]), false;
        const uint32_t f = be32(p.d) & 0xffffffu, count = be32(p.d + 4);
        total += count;
        if (count > kMaxUnits || total > kMaxUnits)
            return *error = "fragmented MP4 traf has " + std::to_string(total) + " access units; the materialized limit is " + std::to_string(kMaxUnits), false;
        size_t pos = 8;
        uint64_t at = fallback;
        if (f & 1) {
            uint32_t raw;
            if (!p.u32(pos, &raw)) return *error = "fragmented MP4 trun data offset is truncated", false;
            pos += 4;
            const int64_t off = (int32_t)raw;
            if (off >= 0) {
                if (base_offset > UINT64_MAX - (uint64_t)off) return *error = "fMP4 data offset overflow", false;
                at = base_offset + (uint64_t)off;
            } else {
                if (base_offset < (uint64_t)-off) return *error = "fMP4 negative data offset underflow", false;
                at = base_offset - (uint64_t)-off;
            }
        }
        if (f & 4) {
            if (p.n < pos + 4) return *error = "fragmented MP4 trun first sample flags are truncated", false;
            pos += 4;
        }
        const size_t fields = ((f >> 8) & 1) + ((f >> 9) & 1) + ((f >> 10) & 1) + ((f >> 11) & 1);
        if (!table_fits(p, pos, count, fields * 4, "trun", error)) return false;
        if (mine) out->reserve(out->size() + count);
        for (uint32_t k = 0; k < count; ++k) {
            uint32_t duration = def_duration, size = def_size;
            bool d_ok = have_duration, s_ok = have_size;
            if (f & 0x100) duration = be32(p.d + pos), d_ok = true, pos += 4;
            if (f & 0x200) size = be32(p.d + pos), s_ok = true, pos += 4;
            if (f & 0x400) pos += 4;
            if (f & 0x800) pos += 4;
            if (!s_ok) return *error = "fragmented MP4 trun sample has no size", false;
            if (size > kMaxPacketBytes) return *error = "fragmented MP4 sample exceeds the " + std::to_string(kMaxPacketBytes) + " byte packet budget", false;
            if (mine) {
                if (!d_ok) return *error = "fragmented MP4 trun sample has no duration", false;
                Sample s;
                s.offset = at, s.size = size, s.duration = duration, s.start = time;
                out->push_back(s);
                if (time > UINT64_MAX - duration) return *error = "fragmented MP4 decode time overflow", false;
                time += duration;
            }
            if (at > UINT64_MAX - size) return *error = "fragmented MP4 sample offset overflow", false;
            at += size;
        }
        fallback = at;
    }
    *data_end = fallback;
    return true;
}

// parse_moof: every traf in turn; a later one inherits the end of the one before it as its base offset
inline bool parse_moof(Span moof, const Track &track, const std::vector<TrexDefaults> &trex, uint64_t moof_start, std::vector<Sample> *out, std::string *error) {
    bool have_inherited = false;
    uint64_t inherited = 0;
    return each_child(moof, [&](const BoxHeader &h, Span p) -> bool {
        if (!h.is("traf")) return true;
        uint64_t end = 0;
        if (!parse_traf(p, track, trex, moof_start, have_inherited, inherited, out, &end, error)) return false;
        have_inherited = true, inherited = end;
        return true;
    });
}

// ---- the streaming demuxer -----------------------------------------------------------------------------------------------------------

struct Packet {
    std::vector<uint8_t> data;  // the sample as it lies in the file
    uint64_t start = 0;         // decode time, track timescale
    uint32_t duration = 0;
};

class Demuxer {
  public:
    bool have_track = false;
    Track track;                 // the config event: set once `moov` has been parsed (track.samples: the regular layout's table)
    std::deque<Packet> packets;  // the packet events, in the order their bytes arrived
    bool failed = false;
    std::string error;

    size_t buffered() const { return buf_.size() - cursor_; }

    bool add(const uint8_t *d, size_t n) {
        if (failed) return false;
        if (finished_) return fail("demuxer is already finished");
        if (n > kMaxInputChunkBytes) return fail("MP4 input chunk exceeds the " + std::to_string(kMaxInputChunkBytes) + " byte streaming budget");
        if (n) buf_.insert(buf_.end(), d, d + n);
        return parse(false);
    }

    bool finish() {
        if (failed) return false;
        if (finished_) return true;
        finished_ = true;
        return parse(true);
    }

  private:
    std::vector<uint8_t> buf_;
    size_t cursor_ = 0;
    uint64_t abs_ = 0, skip_ = 0;  // the file offset of buf_[cursor_]; bytes of a stepped-over box still to come
    bool in_mdat_ = false, finished_ = false, saw_moof_ = false;
    uint64_t mdat_start_ = 0, mdat_end_ = 0;
    size_t next_ = 0;               // regular layout: the next sample of track.samples
    std::vector<TrexDefaults> trex_;
    std::deque<Sample> pending_;    // fragmented layout: the samples of the fragments read, by offset

    bool fail(const std::string &text) {
        failed = true;
        error = text;
        return false;
    }

    void drain(size_t n) {
        cursor_ += n;
        abs_ += n;
        if (cursor_ > 64 * 1024 || cursor_ == buf_.size()) {
            buf_.erase(buf_.begin(), buf_.begin() + (ptrdiff_t)cursor_);
            cursor_ = 0;
        }
    }

    void emit(const Sample &s) {
        Packet p;
        p.data.assign(buf_.begin() + (ptrdiff_t)cursor_ + (ptrdiff_t)(s.offset - abs_), buf_.begin() + (ptrdiff_t)cursor_ + (ptrdiff_t)(s.offset - abs_ + s.size));
        p.start = s.start, p.duration = s.duration;
        packets.push_back(std::move(p));
    }

    // emit_active_mdat_samples: the samples of the table that lie in this mdat, in table order, as their bytes become complete; the
    // buffer is drained up to the next sample's offset
    bool regular_mdat() {
        const uint64_t avail_end = std::min(abs_ + buffered(), mdat_end_);
        const std::vector<Sample> &samples = track.samples;
        const Sample *next = nullptr;
        while (next_ < samples.size()) {
            const Sample &s = samples[next_];
            const uint64_t end = s.offset + s.size;  // build_samples: no overflow
            if (end <= mdat_start_) {
                next_ += 1;
                continue;
            }
            if (s.offset >= mdat_end_) break;
            if (end > mdat_end_) return fail("MP4 sample extends past its mdat payload");
            next = &s;
            if (end > avail_end) break;
            if (s.offset < abs_) return fail("MP4 sample offset was already discarded");
            emit(s);
            next = nullptr;
            next_ += 1;
        }
        const uint64_t until = next ? std::max(std::min(next->offset, avail_end), abs_) : avail_end;
        if (next && next->offset < abs_) return fail("MP4 sample offset was already discarded");
        drain((size_t)(until - abs_));
        if (abs_ >= mdat_end_) in_mdat_ = false;
        return true;
    }

    // emit_active_fragmented_mdat_samples, for the one track
    bool fragmented_mdat() {
        for (;;) {
            const uint64_t avail_end = std::min(abs_ + buffered(), mdat_end_);
            if (pending_.empty() || pending_.front().offset >= mdat_end_ || pending_.front().offset + pending_.front().size > mdat_end_) {
                drain((size_t)(avail_end - abs_));
                if (abs_ == mdat_end_) in_mdat_ = false;
                return true;
            }
            const Sample s = pending_.front();
            if (s.offset < mdat_start_) return fail("fragmented MP4 sample precedes its mdat payload");
            if (s.offset < abs_) return fail("fragmented MP4 samples overlap or arrive out of order");
            if (s.offset > avail_end || s.offset + s.size > avail_end) {  // not all here yet: let go of what lies in front of it
                drain((size_t)(std::min(s.offset, avail_end) - abs_));
                return true;
            }
            emit(s);
            drain((size_t)(s.offset - abs_) + s.size);
            pending_.pop_front();
            if (abs_ == mdat_end_) {
                in_mdat_ = false;
                return true;
            }
        }
    }

    bool parse(bool finalizing) {
        for (;;) {
            if (skip_ > 0) {
                const size_t take = (size_t)std::min<uint64_t>(buffered(), skip_);
                drain(take);
                skip_ -= take;
                if (skip_ > 0) break;
                continue;
            }
            if (in_mdat_) {
                const uint64_t before = abs_;
                if (!(track.fragmented ? fragmented_mdat() : regular_mdat())) return false;
                if (in_mdat_ && abs_ == before) break;
                continue;
            }
            BoxHeader h;
            if (!read_box(buf_.data() + cursor_, buffered(), &h)) break;
            if (h.is("mdat")) {
                if (!have_track) {
                    if (saw_moof_) return fail("fragmented MP4 references unknown track");
                    return fail("MP4 mdat appears before moov; use the seekable MP4 packet API");
                }
                mdat_start_ = abs_ + h.header;
                mdat_end_ = abs_ + h.size < abs_ ? UINT64_MAX : abs_ + h.size;
                drain(h.header);
                in_mdat_ = true;
                continue;
            }
            const bool moov = h.is("moov"), moof = h.is("moof");
            if (!moov && !moof) {  // ftyp, free, skip, sidx, styp, ...: stepped over by size, never buffered
                drain(h.header);
                skip_ = h.size - h.header;
                continue;
            }
            if (h.size - h.header > kMaxMetadataBytes)
                return fail(std::string("MP4 ") + h.name + " metadata exceeds the " + std::to_string(kMaxMetadataBytes) + " byte budget");
            if (buffered() < h.size) {
                if (finalizing) return fail(std::string("truncated MP4 box ") + h.name);
                break;
            }
            const Span payload{buf_.data() + cursor_ + h.header, (size_t)h.size - h.header};
            if (moov) {
                if (have_track) return fail("MP4 source contains multiple moov boxes");
                if (!parse_moov(payload, &track, &trex_, &error)) return failed = true, false;
                if (saw_moof_) track.fragmented = true;
                have_track = true;
            } else {
                saw_moof_ = true;
                if (!have_track) return fail("fragmented MP4 references unknown track");
                if (!track.fragmented) return fail("MP4 moof appears in a file whose moov holds no mvex");
                std::vector<Sample> found;
                if (!parse_moof(payload, track, trex_, abs_, &found, &error)) return failed = true, false;
                if (pending_.size() + found.size() > kMaxUnits)
                    return fail("fragmented MP4 has more than " + std::to_string(kMaxUnits) + " access units waiting for their mdat");
                pending_.insert(pending_.end(), found.begin(), found.end());
                std::stable_sort(pending_.begin(), pending_.end(), [](const Sample &a, const Sample &b) { return a.offset < b.offset; });
            }
            drain((size_t)h.size);
        }
        if (!finalizing) return true;
        if (skip_ > 0) return fail("truncated MP4 top-level box");
        if (in_mdat_) return fail("truncated MP4 box mdat");
        if (buffered() != 0) return fail("truncated MP4 box header");
        if (!pending_.empty()) return fail("fragmented MP4 ended before all indexed samples arrived");
        return true;
    }
};

// ---- the whole file ------------------------------------------------------------------------------------------------------------------

// Mp4MediaIndex::from_file for the chosen audio track: `moov` wherever it lies; every sample's range is checked against the file.  A
// fragmented file gives the track and no samples: its packets come from the Demuxer
inline bool index_from_file(const uint8_t *d, size_t len, Track *track, std::string *error) {
    size_t pos = 0;
    while (len - pos >= 8) {
        BoxHeader h;
        if (!read_box(d + pos, len - pos, &h)) return *error = "invalid MP4 box header at byte " + std::to_string(pos), false;
        if (h.size > len - pos) return *error = std::string("truncated MP4 box ") + h.name + " at byte " + std::to_string(pos), false;
        if (h.is("moov")) {
            if (h.size - h.header > kMaxMetadataBytes) return *error = "MOV/MP4 moov metadata exceeds the " + std::to_string(kMaxMetadataBytes) + " byte budget", false;
            std::vector<TrexDefaults> trex;
            if (!parse_moov(Span{d + pos + h.header, (size_t)h.size - h.header}, track, &trex, error)) return false;
            for (size_t i = 0; i < track->samples.size(); ++i) {
                const Sample &s = track->samples[i];
                if (s.offset > len || s.size > len - s.offset) return *error = "MP4 sample " + std::to_string(i) + " extends past the source", false;
            }
            return true;
        }
        pos += (size_t)h.size;
    }
    return *error = "MP4 source has no moov box", false;
}

// resolve_pcm_packet_trim through Mp4MediaIndex::pcm_packet_trim_at_sample_rate: the frames of a decoded packet that lie inside the
// track's first edit.  The packet's place on the presentation timeline is start - media time + the edit's own start; the cut's start
// rounds up, its end down, both are clamped to the frames decoded.  Nothing left: (decoded_frames, 0).  No edit list: all of it.
inline bool trim(const Track &t, const Sample &s, uint32_t decoded_frames, uint32_t decoded_rate, uint32_t *first, uint32_t *count, std::string *error) {
    if (!t.has_edit) return *first = 0, *count = decoded_frames, true;
    if (s.duration == 0) return *error = "PCM trim packet duration is zero", false;
    if (t.timescale == 0 || decoded_rate == 0) return *error = "PCM trim requires non-zero track and sample rates", false;
    *first = decoded_frames, *count = 0;
    if (decoded_frames == 0 || t.edit_duration == 0) return true;
    const __int128 packet_start = (__int128)s.start - (__int128)t.edit_media_start + (__int128)t.edit_presentation_start;
    const __int128 packet_end = packet_start + s.duration;
    const __int128 line_start = t.edit_presentation_start, line_end = line_start + (__int128)t.edit_duration;
    const __int128 lo = std::max(packet_start, line_start), hi = std::min(packet_end, line_end);
    if (hi <= lo) return true;
    const unsigned __int128 scale = t.timescale, rate = decoded_rate;
    unsigned __int128 a = ((unsigned __int128)(lo - packet_start) * rate + scale - 1) / scale;
    unsigned __int128 b = (unsigned __int128)(hi - packet_start) * rate / scale;
    a = std::min<unsigned __int128>(a, decoded_frames), b = std::min<unsigned __int128>(b, decoded_frames);
    if (b <= a) return true;
    return *first = (uint32_t)a, *count = (uint32_t)(b - a), true;
}

// create_adts_header, byte for byte: profile from the config's object type (no config: 1), the rate's index (15 for a rate off the
// table), the channel count capped at 7, no CRC, buffer fullness all ones
inline void adts_header(const uint8_t *asc, size_t asc_len, uint32_t rate, uint32_t channels, size_t raw_len, uint8_t out[7]) {
    uint32_t profile = 1;
    if (asc_len) {
        const uint32_t aot = asc[0] >> 3;
        profile = std::min<uint32_t>(aot ? aot - 1 : 0, 3);
    }
    uint32_t index = 15;
    for (uint32_t i = 0; i < 13; ++i)
        if (rate_of_index(i) == rate) index = i;
    const uint32_t ch = std::min<uint32_t>(channels & 255u, 7);
    const size_t length = raw_len + 7;
    out[0] = 0xff;
    out[1] = 0xf1;
    out[2] = (uint8_t)(profile << 6 | index << 2 | ch >> 2);
    out[3] = (uint8_t)((ch & 3) << 6 | ((length >> 11) & 3));
    out[4] = (uint8_t)((length >> 3) & 0xff);
    out[5] = (uint8_t)(((length & 7) << 5) | 0x1f);
    out[6] = 0xfc;
}

}  // namespace sk_mp4

// vorbis_stream.h -- Vorbis I on the host: the three header parsers, the validation of everything the setup header says, and the
// device blob of a stream (vorbis_blob.h).  The setup header is untrusted input that later steers table walks on the device: nothing
// leaves this file for the device unless every book number, class book, coupling channel and X list has been checked, and every code
// book is a complete prefix code (or the one-entry case), so that a bounded tree walk always ends in a leaf.
//
// VQ values are expanded to f32 here, in this order: value = ((multiplicand * delta) + minimum) + last, each operation rounded to f32.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "vorbis_blob.h"

namespace sk_vorbis {

constexpr size_t kMaxPacketBytes = 16u * 1024 * 1024;  // the Ogg parser's packet budget; the device counts a packet's bits in 32
constexpr int kOk = 0, kUnsupported = -6 /* SK_ERR_UNSUPPORTED */, kNotAudio = -801, kBadMode = -802, kShort = -803, kErrStream = -804;

struct Ident {
    uint32_t sample_rate = 0, bitrate_maximum = 0, bitrate_nominal = 0, bitrate_minimum = 0;
    uint16_t blocksize_0 = 0, blocksize_1 = 0;
    uint8_t channels = 0;
};

// LSB first; a read that does not fit sets eop and returns 0
struct Bits {
    const uint8_t *p;
    uint64_t n, pos = 0;
    bool eop = false;
    Bits(const uint8_t *data, size_t len) : p(data), n((uint64_t)len * 8) {}
    uint32_t read(uint32_t bits) {
        if (eop || pos + bits > n) {
            eop = true;
            return 0;
        }
        uint64_t v = 0;
        const uint64_t byte = pos >> 3;
        const uint32_t have = (uint32_t)std::min<uint64_t>(8, (n >> 3) - byte);
        for (uint32_t i = 0; i < have; ++i) v |= (uint64_t)p[byte + i] << (8 * i);
        v >>= (pos & 7);
        pos += bits;
        return bits >= 32 ? (uint32_t)v : (uint32_t)(v & ((1ull << bits) - 1));
    }
};

inline uint32_t ilog(uint32_t x) {
    uint32_t r = 0;
    while (x) ++r, x >>= 1;
    return r;
}

inline int fail(std::string *error, const std::string &text, int rc = kErrStream) {
    if (error) *error = text;
    return rc;
}

inline bool is_header(const uint8_t *p, size_t len, uint8_t type) { return len >= 7 && p[0] == type && memcmp(p + 1, "vorbis", 6) == 0; }

inline int parse_ident(const uint8_t *p, size_t len, Ident *out, std::string *error) {
    if (!is_header(p, len, 1)) return fail(error, "not a Vorbis identification header");
    Bits b(p, len);
    b.pos = 56;
    const uint32_t version = b.read(32);
    Ident id;
    id.channels = (uint8_t)b.read(8);
    id.sample_rate = b.read(32);
    id.bitrate_maximum = b.read(32), id.bitrate_nominal = b.read(32), id.bitrate_minimum = b.read(32);
    const uint32_t e0 = b.read(4), e1 = b.read(4), framing = b.read(1);
    if (b.eop) return fail(error, "Vorbis identification header is too short");
    if (version != 0) return fail(error, "unsupported Vorbis version " + std::to_string(version));
    if (id.channels == 0) return fail(error, "Vorbis identification header states no channels");
    if (id.sample_rate == 0) return fail(error, "Vorbis identification header states no sample rate");
    if (e0 < 6 || e1 > 13 || e0 > e1) return fail(error, "Vorbis block sizes outside 64 ... 8192 or out of order");
    if (!framing) return fail(error, "Vorbis identification header lacks its framing bit");
    id.blocksize_0 = (uint16_t)(1u << e0), id.blocksize_1 = (uint16_t)(1u << e1);
    *out = id;
    return kOk;
}

// walked and bounds-checked only
inline int parse_comment(const uint8_t *p, size_t len, std::string *error) {
    if (!is_header(p, len, 3)) return fail(error, "not a Vorbis comment header");
    size_t at = 7;
    auto u32 = [&](uint32_t *v) {
        if (len - at < 4) return false;
        *v = (uint32_t)p[at] | (uint32_t)p[at + 1] << 8 | (uint32_t)p[at + 2] << 16 | (uint32_t)p[at + 3] << 24;
        at += 4;
        return true;
    };
    uint32_t n = 0, count = 0;
    if (!u32(&n) || len - at < n) return fail(error, "Vorbis comment header is too short");
    at += n;
    if (!u32(&count)) return fail(error, "Vorbis comment header is too short");
    for (uint32_t i = 0; i < count; ++i) {
        if (!u32(&n) || len - at < n) return fail(error, "Vorbis comment header is too short");
        at += n;
    }
    if (at >= len || !(p[at] & 1)) return fail(error, "Vorbis comment header lacks its framing bit");
    return kOk;
}

struct Codebook {
    uint32_t dims = 0, entries = 0, lookup_type = 0, value_bits = 0, sequence_p = 0;
    float minimum = 0, delta = 0;
    std::vector<uint8_t> lengths;  // 0: unused
    std::vector<uint32_t> multiplicands;
    int32_t single = -1;
};
struct Floor1 {
    std::vector<uint32_t> partition_class, class_dim, class_sub, class_master, x, low, high, sorted;
    std::vector<std::vector<int32_t>> sub_books;
    uint32_t multiplier = 1, rangebits = 0;
};
struct Residue {
    uint32_t type = 0, begin = 0, end = 0, partition_size = 1, classifications = 1, classbook = 0;
    std::vector<std::vector<int32_t>> books;  // [class][pass], -1: none
};
struct Mapping {
    uint32_t submaps = 1;
    std::vector<std::pair<uint32_t, uint32_t>> coupling;  // magnitude, angle
    std::vector<uint32_t> mux, floor, residue;
};
struct Mode {
    uint32_t blockflag = 0, mapping = 0;
};
struct Setup {
    uint32_t channels = 0, bs[2] = {0, 0};
    std::vector<Codebook> books;
    std::vector<Floor1> floors;
    std::vector<Residue> residues;
    std::vector<Mapping> mappings;
    std::vector<Mode> modes;
    std::vector<uint32_t> blob;
};

inline float float32_unpack(uint32_t x) {
    int32_t mant = (int32_t)(x & 0x1fffff);
    if (x & 0x80000000u) mant = -mant;
    return ldexpf((float)mant, (int)((x & 0x7fe00000u) >> 21) - 788);
}

inline uint32_t lookup1_values(uint32_t entries, uint32_t dims) {
    // the largest r with r^dims <= entries
    uint32_t r = 0;
    for (uint32_t bit = 1u << 24; bit; bit >>= 1) {
        const uint32_t t = r | bit;
        uint64_t acc = 1;
        bool fits = true;
        for (uint32_t i = 0; i < dims && fits; ++i) {
            acc *= t;
            if (acc > entries) fits = false;
        }
        if (fits) r = t;
    }
    return r;
}

// the specification's code word assignment as a binary tree: nodes of two children (kLeaf | entry, or a node index).  false: the lengths
// over- or under-specify the tree.
inline bool build_tree(const Codebook &c, std::vector<uint32_t> *nodes, std::string *why) {
    uint32_t avail[33] = {0};
    bool first = true;
    nodes->assign(2, 0xffffffffu);
    for (uint32_t i = 0; i < c.entries; ++i) {
        const uint32_t l = c.lengths[i];
        if (!l) continue;
        uint32_t code = 0;
        if (first) {
            first = false;
            for (uint32_t k = 1; k <= l; ++k) avail[k] = 1u << (32 - k);
        } else {
            uint32_t z = l;
            while (z > 0 && !avail[z]) --z;
            if (z == 0) {
                *why = "over-specified";
                return false;
            }
            const uint32_t res = avail[z];
            avail[z] = 0;
            code = res >> (32 - l);
            for (uint32_t y = z + 1; y <= l; ++y) avail[y] = res + (1u << (32 - y));
        }
        uint32_t node = 0;
        for (uint32_t k = l; k-- > 0;) {
            const uint32_t bit = (code >> k) & 1, at = 2 * node + bit;
            if (k == 0) {
                if ((*nodes)[at] != 0xffffffffu) return *why = "over-specified", false;
                (*nodes)[at] = sk_vb::kLeaf | i;
            } else {
                if ((*nodes)[at] == 0xffffffffu) {
                    (*nodes)[at] = (uint32_t)(nodes->size() / 2);
                    nodes->push_back(0xffffffffu);
                    nodes->push_back(0xffffffffu);
                } else if ((*nodes)[at] & sk_vb::kLeaf) {
                    return *why = "over-specified", false;
                }
                node = (*nodes)[at];
            }
        }
    }
    for (uint32_t k = 1; k <= 32; ++k)
        if (avail[k]) return *why = "under-specified", false;
    for (uint32_t v : *nodes)
        if (v == 0xffffffffu) return *why = "under-specified", false;
    return true;
}

inline int build_blob(Setup &s, std::string *error);

inline int parse_setup(const uint8_t *p, size_t len, const Ident &id, Setup *out, std::string *error) {
    if (!is_header(p, len, 5)) return fail(error, "not a Vorbis setup header");
    Bits b(p, len);
    b.pos = 56;
    Setup s;
    s.channels = id.channels, s.bs[0] = id.blocksize_0, s.bs[1] = id.blocksize_1;
    const std::string eof = "Vorbis setup header is too short";
    uint64_t blob_words = 0;  // a running lower bound, so that a hostile header is refused before its tables are made
    const uint32_t n_books = b.read(8) + 1;
    for (uint32_t k = 0; k < n_books; ++k) {
        const std::string at = "Vorbis code book " + std::to_string(k);
        if (b.read(24) != 0x564342 || b.eop) return fail(error, b.eop ? eof : at + ": sync pattern missing");
        Codebook c;
        c.dims = b.read(16), c.entries = b.read(24);
        if (b.eop) return fail(error, eof);
        if (c.dims == 0 || c.entries == 0) return fail(error, at + ": no dimensions or no entries");
        c.lengths.assign(c.entries, 0);
        if (b.read(1)) {
            uint32_t cur = 0, ln = b.read(5) + 1;
            while (cur < c.entries) {
                const uint32_t num = b.read(ilog(c.entries - cur));
                if (b.eop) return fail(error, eof);
                if (num > c.entries - cur || ln > 32) return fail(error, at + ": ordered lengths run past the entries");
                for (uint32_t i = 0; i < num; ++i) c.lengths[cur + i] = (uint8_t)ln;
                cur += num, ++ln;
            }
        } else {
            const uint32_t sparse = b.read(1);
            if (c.entries > b.n - b.pos) return fail(error, eof);  // every entry of such a list costs at least a bit
            for (uint32_t i = 0; i < c.entries; ++i) {
                if (sparse && !b.read(1)) continue;
                c.lengths[i] = (uint8_t)(b.read(5) + 1);
            }
        }
        c.lookup_type = b.read(4);
        if (b.eop) return fail(error, eof);
        if (c.lookup_type > 2) return fail(error, at + ": lookup type " + std::to_string(c.lookup_type));
        if (c.lookup_type) {
            c.minimum = float32_unpack(b.read(32)), c.delta = float32_unpack(b.read(32));
            c.value_bits = b.read(4) + 1, c.sequence_p = b.read(1);
            const uint64_t n = c.lookup_type == 1 ? lookup1_values(c.entries, c.dims) : (uint64_t)c.entries * c.dims;
            if (b.eop || n * c.value_bits > b.n - b.pos) return fail(error, eof);
            c.multiplicands.resize((size_t)n);
            for (auto &m : c.multiplicands) m = b.read(c.value_bits);
            blob_words += (uint64_t)c.entries * c.dims;
        }
        blob_words += c.entries;
        if (blob_words * 4 > sk_vb::kMaxBlobBytes)
            return fail(error, "Vorbis setup exceeds the " + std::to_string(sk_vb::kMaxBlobBytes) + " byte table budget", kUnsupported);
        uint32_t used = 0, one = 0;
        for (uint32_t i = 0; i < c.entries; ++i)
            if (c.lengths[i]) ++used, one = i;
        if (used == 0) return fail(error, at + ": no used entry");
        if (used == 1) {
            if (c.lengths[one] != 1) return fail(error, at + ": a single entry must have length 1");
            c.single = (int32_t)one;
        } else {
            std::vector<uint32_t> nodes;
            std::string why;
            if (!build_tree(c, &nodes, &why)) return fail(error, at + ": " + why + " code lengths");
        }
        s.books.push_back(std::move(c));
    }
    const uint32_t nb = (uint32_t)s.books.size();
    for (uint32_t n = b.read(6) + 1, i = 0; i < n; ++i)
        if (b.read(16) != 0) return fail(error, b.eop ? eof : "Vorbis time domain placeholder is not zero");
    for (uint32_t n = b.read(6) + 1, k = 0; k < n; ++k) {
        const std::string at = "Vorbis floor " + std::to_string(k);
        const uint32_t type = b.read(16);
        if (b.eop) return fail(error, eof);
        if (type == 0) return fail(error, at + ": floor type 0 is not built", kUnsupported);
        if (type != 1) return fail(error, at + ": type " + std::to_string(type));
        Floor1 f;
        f.partition_class.resize(b.read(5));
        uint32_t classes = 0;
        for (auto &c : f.partition_class) c = b.read(4), classes = std::max(classes, c + 1);
        for (uint32_t c = 0; c < classes; ++c) {
            f.class_dim.push_back(b.read(3) + 1);
            f.class_sub.push_back(b.read(2));
            f.class_master.push_back(f.class_sub[c] ? b.read(8) : 0);
            if (f.class_sub[c] && f.class_master[c] >= nb) return fail(error, at + ": class master book " + std::to_string(f.class_master[c]) + " does not exist");
            f.sub_books.emplace_back();
            for (uint32_t j = 0; j < (1u << f.class_sub[c]); ++j) {
                const int32_t book = (int32_t)b.read(8) - 1;
                if (book >= (int32_t)nb) return fail(error, at + ": subclass book " + std::to_string(book) + " does not exist");
                f.sub_books[c].push_back(book);
            }
        }
        f.multiplier = b.read(2) + 1, f.rangebits = b.read(4);
        f.x = {0, 1u << f.rangebits};
        for (uint32_t c : f.partition_class)
            for (uint32_t j = 0; j < f.class_dim[c]; ++j) f.x.push_back(b.read(f.rangebits));
        if (b.eop) return fail(error, eof);
        if (f.x.size() > sk_vb::kMaxPosts) return fail(error, at + ": more than 65 posts");
        const uint32_t nv = (uint32_t)f.x.size();
        f.sorted.resize(nv);
        for (uint32_t i = 0; i < nv; ++i) f.sorted[i] = i;
        std::sort(f.sorted.begin(), f.sorted.end(), [&](uint32_t a, uint32_t c) { return f.x[a] < f.x[c]; });
        for (uint32_t i = 1; i < nv; ++i)
            if (f.x[f.sorted[i]] == f.x[f.sorted[i - 1]]) return fail(error, at + ": the X list repeats a value");
        f.low.assign(nv, 0), f.high.assign(nv, 1);
        for (uint32_t i = 2; i < nv; ++i) {
            uint32_t lo = 0, hi = 1;
            for (uint32_t j = 0; j < i; ++j) {
                if (f.x[j] < f.x[i] && f.x[j] > f.x[lo]) lo = j;
                if (f.x[j] > f.x[i] && f.x[j] < f.x[hi]) hi = j;
            }
            f.low[i] = lo, f.high[i] = hi;
        }
        s.floors.push_back(std::move(f));
    }
    for (uint32_t n = b.read(6) + 1, k = 0; k < n; ++k) {
        const std::string at = "Vorbis residue " + std::to_string(k);
        Residue r;
        r.type = b.read(16);
        if (b.eop) return fail(error, eof);
        if (r.type > 2) return fail(error, at + ": type " + std::to_string(r.type));
        r.begin = b.read(24), r.end = b.read(24), r.partition_size = b.read(24) + 1, r.classifications = b.read(6) + 1, r.classbook = b.read(8);
        std::vector<uint32_t> cascade(r.classifications);
        for (auto &c : cascade) {
            const uint32_t low = b.read(3);
            c = (b.read(1) ? b.read(5) : 0) * 8 + low;
        }
        for (uint32_t c : cascade) {
            r.books.emplace_back(8, -1);
            for (uint32_t j = 0; j < 8; ++j)
                if (c >> j & 1) r.books.back()[j] = (int32_t)b.read(8);
        }
        if (b.eop) return fail(error, eof);
        if (r.classbook >= nb) return fail(error, at + ": class book " + std::to_string(r.classbook) + " does not exist");
        if (r.end < r.begin) return fail(error, at + ": end before begin");
        // against the block sizes: the longest vector a residue of this stream can meet is blocksize_1 / 2, times the channels for type 2
        if (r.end > (uint64_t)(s.bs[1] / 2) * (r.type == 2 ? s.channels : 1))
            return fail(error, at + ": end " + std::to_string(r.end) + " lies beyond the longest vector of this stream");
        // within that bound begin / end may still lie beyond the vector of a short block or of a submap with fewer channels: the
        // kernel clamps both to the vector it works on, as the specification has the decode do
        uint64_t words = 1;  // classifications ^ class words must fit the class book's entries, or the digits read off it mean nothing
        for (uint32_t i = 0; i < s.books[r.classbook].dims && words <= (1u << 24); ++i) words *= r.classifications;
        if (words > s.books[r.classbook].entries) return fail(error, at + ": class book has too few entries for its class words");
        for (auto &row : r.books)
            for (int32_t x : row) {
                if (x < 0) continue;
                if (x >= (int32_t)nb) return fail(error, at + ": book " + std::to_string(x) + " does not exist");
                if (s.books[x].lookup_type == 0) return fail(error, at + ": book " + std::to_string(x) + " has no values");
                if (r.partition_size % s.books[x].dims) return fail(error, at + ": partition size is no multiple of the dimensions of book " + std::to_string(x));
            }
        s.residues.push_back(std::move(r));
    }
    for (uint32_t n = b.read(6) + 1, k = 0; k < n; ++k) {
        const std::string at = "Vorbis mapping " + std::to_string(k);
        if (b.read(16) != 0) return fail(error, b.eop ? eof : at + ": type is not 0");
        Mapping m;
        m.submaps = b.read(1) ? b.read(4) + 1 : 1;
        if (b.read(1)) {
            const uint32_t steps = b.read(8) + 1, bits = ilog(s.channels - 1);
            for (uint32_t i = 0; i < steps; ++i) {
                const uint32_t mag = b.read(bits), ang = b.read(bits);
                if (b.eop) return fail(error, eof);
                if (mag == ang || mag >= s.channels || ang >= s.channels) return fail(error, at + ": coupling channels " + std::to_string(mag) + " / " + std::to_string(ang));
                m.coupling.emplace_back(mag, ang);
            }
        }
        if (b.read(2) != 0) return fail(error, b.eop ? eof : at + ": reserved bits set");
        m.mux.assign(s.channels, 0);
        if (m.submaps > 1)
            for (auto &x : m.mux) {
                x = b.read(4);
                if (x >= m.submaps) return fail(error, at + ": channel assigned to submap " + std::to_string(x));
            }
        for (uint32_t i = 0; i < m.submaps; ++i) {
            b.read(8);
            m.floor.push_back(b.read(8)), m.residue.push_back(b.read(8));
            if (b.eop) return fail(error, eof);
            if (m.floor[i] >= s.floors.size()) return fail(error, at + ": floor " + std::to_string(m.floor[i]) + " does not exist");
            if (m.residue[i] >= s.residues.size()) return fail(error, at + ": residue " + std::to_string(m.residue[i]) + " does not exist");
        }
        s.mappings.push_back(std::move(m));
    }
    for (uint32_t n = b.read(6) + 1, k = 0; k < n; ++k) {
        Mode m;
        m.blockflag = b.read(1);
        const uint32_t wt = b.read(16), tt = b.read(16);
        m.mapping = b.read(8);
        if (b.eop) return fail(error, eof);
        if (wt || tt) return fail(error, "Vorbis mode " + std::to_string(k) + ": window or transform type is not 0");
        if (m.mapping >= s.mappings.size()) return fail(error, "Vorbis mode " + std::to_string(k) + ": mapping " + std::to_string(m.mapping) + " does not exist");
        s.modes.push_back(m);
    }
    if (!b.read(1) || b.eop) return fail(error, b.eop ? eof : "Vorbis setup header lacks its framing bit");
    if (s.channels > sk_vb::kMaxChannels) return fail(error, "Vorbis streams of more than 8 channels are not built", kUnsupported);
    if (const int rc = build_blob(s, error)) return rc;
    *out = std::move(s);
    return kOk;
}

inline int build_blob(Setup &s, std::string *error) {
    using namespace sk_vb;
    std::vector<uint32_t> &w = s.blob;
    w.assign(H_SIZE, 0);
    w[H_CHANNELS] = s.channels, w[H_BS0] = s.bs[0], w[H_BS1] = s.bs[1];
    w[H_NMODES] = (uint32_t)s.modes.size(), w[H_MODEBITS] = ilog((uint32_t)s.modes.size() - 1);
    w[H_MODES] = (uint32_t)w.size();
    for (const Mode &m : s.modes) w.push_back(m.blockflag), w.push_back(m.mapping);
    w[H_MAPPINGS] = (uint32_t)w.size();
    w.resize(w.size() + s.mappings.size() * M_SIZE, 0);
    for (size_t k = 0; k < s.mappings.size(); ++k) {
        const Mapping &m = s.mappings[k];
        const size_t at = w[H_MAPPINGS] + k * M_SIZE;
        w[at + M_SUBMAPS] = m.submaps, w[at + M_NCOUPLING] = (uint32_t)m.coupling.size(), w[at + M_COUPLING] = (uint32_t)w.size();
        for (uint32_t c = 0; c < s.channels; ++c) w[at + M_MUX + c] = m.mux[c];
        for (uint32_t i = 0; i < m.submaps; ++i) w[at + M_FLOOR + i] = m.floor[i], w[at + M_RESIDUE + i] = m.residue[i];
        for (auto &step : m.coupling) w.push_back(step.first | step.second << 8);
    }
    w[H_FLOORS] = (uint32_t)w.size();
    w.resize(w.size() + s.floors.size() * F_SIZE, 0);
    for (size_t k = 0; k < s.floors.size(); ++k) {
        const Floor1 &f = s.floors[k];
        uint32_t *r = w.data() + w[H_FLOORS] + k * F_SIZE;
        r[F_VALUES] = (uint32_t)f.x.size(), r[F_MULT] = f.multiplier, r[F_PARTS] = (uint32_t)f.partition_class.size();
        for (size_t i = 0; i < f.partition_class.size(); ++i) r[F_PCLASS + i] = f.partition_class[i];
        for (size_t c = 0; c < f.class_dim.size(); ++c) {
            r[F_CDIM + c] = f.class_dim[c], r[F_CSUB + c] = f.class_sub[c], r[F_CMASTER + c] = f.class_master[c];
            for (size_t j = 0; j < 8; ++j) r[F_SUBBOOKS + 8 * c + j] = j < f.sub_books[c].size() ? (uint32_t)f.sub_books[c][j] : 0xffffffffu;
        }
        for (size_t i = 0; i < f.x.size(); ++i) r[F_X + i] = f.x[i], r[F_LOW + i] = f.low[i], r[F_HIGH + i] = f.high[i], r[F_SORTED + i] = f.sorted[i];
    }
    w[H_RESIDUES] = (uint32_t)w.size();
    w.resize(w.size() + s.residues.size() * R_SIZE, 0xffffffffu);
    for (size_t k = 0; k < s.residues.size(); ++k) {
        const Residue &x = s.residues[k];
        uint32_t *r = w.data() + w[H_RESIDUES] + k * R_SIZE;
        r[R_TYPE] = x.type, r[R_BEGIN] = x.begin, r[R_END] = x.end, r[R_PSIZE] = x.partition_size, r[R_NCLASS] = x.classifications, r[R_CLASSBOOK] = x.classbook;
        for (size_t c = 0; c < x.books.size(); ++c)
            for (size_t j = 0; j < 8; ++j) r[R_BOOKS + 8 * c + j] = (uint32_t)x.books[c][j];
    }
    w[H_BOOKS] = (uint32_t)w.size(), w[H_NBOOKS] = (uint32_t)s.books.size();
    w.resize(w.size() + s.books.size() * B_SIZE, 0);
    for (size_t k = 0; k < s.books.size(); ++k) {
        const Codebook &c = s.books[k];
        const size_t rec = w[H_BOOKS] + k * B_SIZE;
        w[rec + B_DIMS] = c.dims, w[rec + B_ENTRIES] = c.entries, w[rec + B_SINGLE] = (uint32_t)(c.single + 1);
        if (c.single < 0) {
            std::vector<uint32_t> nodes;
            std::string why;
            if (!build_tree(c, &nodes, &why)) return fail(error, "Vorbis code book " + std::to_string(k) + ": " + why + " code lengths");
            uint32_t longest = 0;
            for (uint8_t l : c.lengths) longest = std::max<uint32_t>(longest, l);
            const uint32_t bits = std::min(longest, kLutBits);
            w[rec + B_LUTBITS] = bits, w[rec + B_LUT] = (uint32_t)w.size();
            for (uint32_t v = 0; v < (1u << bits); ++v) {
                uint32_t node = 0, e = 0;
                for (uint32_t d = 0; d < bits; ++d) {
                    const uint32_t child = nodes[2 * node + ((v >> d) & 1)];
                    if (child & kLeaf) {
                        e = child | d << 24;  // length - 1 = d
                        break;
                    }
                    node = e = child;
                }
                w.push_back(e);
            }
            w[rec + B_TREE] = (uint32_t)w.size();
            w.insert(w.end(), nodes.begin(), nodes.end());
        }
        if (c.lookup_type) {
            w[rec + B_VQ] = (uint32_t)w.size();
            const uint32_t lv = (uint32_t)c.multiplicands.size();
            for (uint32_t e = 0; e < c.entries; ++e) {
                float last = 0.0f;
                uint32_t div = 1;
                for (uint32_t i = 0; i < c.dims; ++i) {
                    uint32_t off;
                    if (c.lookup_type == 1) {
                        off = (e / div) % lv;
                        div = (uint64_t)div * lv > 0xffffffffu ? 0xffffffffu : div * lv;
                    } else {
                        off = e * c.dims + i;
                    }
                    volatile float prod = (float)c.multiplicands[off] * c.delta;  // each step rounded to f32, whatever the host's contraction rules
                    volatile float sum = prod + c.minimum;
                    const float v = sum + last;
                    if (c.sequence_p) last = v;
                    uint32_t bitsv;
                    memcpy(&bitsv, &v, 4);
                    w.push_back(bitsv);
                }
            }
        }
        if (w.size() * 4 > kMaxBlobBytes) return fail(error, "Vorbis setup exceeds the " + std::to_string(kMaxBlobBytes) + " byte table budget", kUnsupported);
    }
    w[H_WORDS] = (uint32_t)w.size();
    return kOk;
}

// the first bits of an audio packet, as the device reads them again: type, mode, and for a long block the two window flags
struct PacketHead {
    uint32_t mode = 0, blockflag = 0, prev = 0, next = 0, n = 0;
};
inline int packet_head(const Setup &s, const uint8_t *p, size_t len, PacketHead *h) {
    Bits b(p, len);
    const uint32_t type = b.read(1);
    if (b.eop) return kShort;
    if (type) return kNotAudio;
    h->mode = b.read(ilog((uint32_t)s.modes.size() - 1));
    if (b.eop) return kShort;
    if (h->mode >= s.modes.size()) return kBadMode;
    h->blockflag = s.modes[h->mode].blockflag;
    if (h->blockflag) {
        h->prev = b.read(1), h->next = b.read(1);
        if (b.eop) return kShort;
    }
    h->n = s.bs[h->blockflag];
    return kOk;
}

}  // namespace sk_vorbis

// the C ABI's opaque sk_vorbis_setup (include/soundkit_amd.h): the engine and the scheduler both make and read it
struct sk_vorbis_setup {
    sk_vorbis::Setup setup;
};

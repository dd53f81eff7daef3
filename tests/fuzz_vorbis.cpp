// Mutation fuzz of the host side of the Ogg Vorbis path -- the Ogg page parser, the three header parsers, the blob builder and the
// packet's first bits -- built with AddressSanitizer + UBSan on the CPU (tests/test_vorbis_cpu.py::test_mutated_files_under_sanitizers).
// The bytes come from the network: whatever arrives, every call must come back with a result or a text, with no out-of-bounds access
// and no undefined behaviour.  A setup that is accepted is then walked the way the kernel walks it: every offset and index its blob
// holds must lie inside the blob, and every code book's tree must end in leaves within 32 steps.  Every buffer handed in is a heap
// block of exactly the length named, so that a read past it is seen.
//   usage: fuzz_vorbis ITERATIONS file.ogg
#include "../soundkit_amd/csrc/ogg_stream.h"
#include "../soundkit_amd/csrc/vorbis_stream.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#define check(cond) ((cond) ? (void)0 : (std::fprintf(stderr, "fuzz_vorbis: check failed at line %d\n", __LINE__), std::abort()))

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    g_seed ^= g_seed << 13, g_seed ^= g_seed >> 7, g_seed ^= g_seed << 17;
    return (uint32_t)(g_seed >> 16);
}

static size_t g_oggs = 0, g_ogg_errors = 0, g_idents = 0, g_ident_errors = 0, g_comments = 0, g_comment_errors = 0, g_setups = 0, g_setup_errors = 0;

static std::unique_ptr<uint8_t[]> heap(const uint8_t *d, size_t len) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[len ? len : 1]);
    if (len) std::memcpy(p.get(), d, len);
    return p;
}

static void mutate(uint8_t *d, size_t len, uint32_t most) {
    if (!len) return;
    for (uint32_t k = rnd() % (most + 1); k > 0; --k) {
        if (rnd() & 1) d[rnd() % len] = (uint8_t)rnd();
        else d[rnd() % len] ^= (uint8_t)(1u << (rnd() & 7));
    }
}

// the blob as the kernel reads it
static void check_blob(const sk_vorbis::Setup &s) {
    using namespace sk_vb;
    const std::vector<uint32_t> &w = s.blob;
    const size_t n = w.size();
    check(n >= H_SIZE && w[H_WORDS] == n && n * 4 <= kMaxBlobBytes);
    check(w[H_CHANNELS] >= 1 && w[H_CHANNELS] <= kMaxChannels && w[H_NMODES] >= 1 && w[H_NMODES] <= 64);
    const uint32_t nb = w[H_NBOOKS], books = w[H_BOOKS];
    check(books + (size_t)nb * B_SIZE <= n);
    for (uint32_t k = 0; k < nb; ++k) {
        const uint32_t *b = &w[books + k * B_SIZE];
        if (b[B_VQ]) check(b[B_VQ] + (uint64_t)b[B_ENTRIES] * b[B_DIMS] <= n);
        if (b[B_SINGLE]) {
            check(b[B_SINGLE] <= b[B_ENTRIES]);
            continue;
        }
        check(b[B_LUTBITS] >= 1 && b[B_LUTBITS] <= kLutBits && b[B_LUT] + (1u << b[B_LUTBITS]) <= n);
        // every path from the root ends in a leaf of an existing entry within 32 steps: walk the whole tree
        std::vector<std::pair<uint32_t, uint32_t>> todo{{0u, 0u}};
        size_t leaves = 0;
        while (!todo.empty()) {
            const auto [node, depth] = todo.back();
            todo.pop_back();
            check(depth < 32 && b[B_TREE] + 2ull * node + 1 < n);
            for (uint32_t bit = 0; bit < 2; ++bit) {
                const uint32_t c = w[b[B_TREE] + 2 * node + bit];
                if (c & kLeaf) check((c & 0xffffffu) < b[B_ENTRIES]), ++leaves;
                else todo.emplace_back(c, depth + 1);
            }
            check(leaves <= b[B_ENTRIES]);
        }
        for (uint32_t v = 0; v < (1u << b[B_LUTBITS]); ++v) {
            const uint32_t e = w[b[B_LUT] + v];
            if (e & kLeaf) check((e & 0xffffffu) < b[B_ENTRIES] && ((e >> 24) & 31u) < b[B_LUTBITS]);
            else check(b[B_TREE] + 2ull * e + 1 < n);
        }
    }
    const uint32_t nf = (uint32_t)s.floors.size(), nr = (uint32_t)s.residues.size(), nm = (uint32_t)s.mappings.size();
    check(w[H_FLOORS] + (size_t)nf * F_SIZE <= n && w[H_RESIDUES] + (size_t)nr * R_SIZE <= n && w[H_MAPPINGS] + (size_t)nm * M_SIZE <= n);
    for (uint32_t k = 0; k < nf; ++k) {
        const uint32_t *f = &w[w[H_FLOORS] + k * F_SIZE];
        check(f[F_VALUES] >= 2 && f[F_VALUES] <= kMaxPosts && f[F_PARTS] <= 31 && f[F_MULT] >= 1 && f[F_MULT] <= 4);
        uint32_t values = 2;
        for (uint32_t p = 0; p < f[F_PARTS]; ++p) {
            const uint32_t cl = f[F_PCLASS + p];
            check(cl < 16 && f[F_CDIM + cl] >= 1 && f[F_CDIM + cl] <= 8 && f[F_CSUB + cl] <= 3);
            if (f[F_CSUB + cl]) check(f[F_CMASTER + cl] < nb);
            for (uint32_t j = 0; j < (1u << f[F_CSUB + cl]); ++j) check(f[F_SUBBOOKS + 8 * cl + j] == 0xffffffffu || f[F_SUBBOOKS + 8 * cl + j] < nb);
            values += f[F_CDIM + cl];
        }
        check(values == f[F_VALUES]);
        for (uint32_t i = 0; i < values; ++i) {
            check(f[F_SORTED + i] < values && f[F_LOW + i] < values && f[F_HIGH + i] < values);
            if (i) check(f[F_X + f[F_SORTED + i]] > f[F_X + f[F_SORTED + i - 1]]);
            if (i >= 2) check(f[F_LOW + i] < i && f[F_HIGH + i] < i && f[F_X + f[F_LOW + i]] < f[F_X + i] && f[F_X + f[F_HIGH + i]] > f[F_X + i]);
        }
    }
    for (uint32_t k = 0; k < nr; ++k) {
        const uint32_t *r = &w[w[H_RESIDUES] + k * R_SIZE];
        check(r[R_TYPE] <= 2 && r[R_BEGIN] <= r[R_END] && r[R_PSIZE] >= 1 && r[R_NCLASS] >= 1 && r[R_NCLASS] <= 64 && r[R_CLASSBOOK] < nb);
        for (uint32_t c = 0; c < r[R_NCLASS]; ++c)
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t b = r[R_BOOKS + 8 * c + j];
                if (b == 0xffffffffu) continue;
                check(b < nb && w[books + b * B_SIZE + B_VQ] != 0 && r[R_PSIZE] % w[books + b * B_SIZE + B_DIMS] == 0);
            }
    }
    for (uint32_t k = 0; k < nm; ++k) {
        const uint32_t *m = &w[w[H_MAPPINGS] + k * M_SIZE];
        check(m[M_SUBMAPS] >= 1 && m[M_SUBMAPS] <= 16 && m[M_NCOUPLING] <= 256 && m[M_COUPLING] + (size_t)m[M_NCOUPLING] <= n);
        for (uint32_t i = 0; i < m[M_NCOUPLING]; ++i) {
            const uint32_t st = w[m[M_COUPLING] + i];
            check((st & 0xff) < w[H_CHANNELS] && (st >> 8) < w[H_CHANNELS] && (st & 0xff) != (st >> 8));
        }
        for (uint32_t c = 0; c < w[H_CHANNELS]; ++c) check(m[M_MUX + c] < m[M_SUBMAPS]);
        for (uint32_t i = 0; i < m[M_SUBMAPS]; ++i) check(m[M_FLOOR + i] < nf && m[M_RESIDUE + i] < nr);
    }
    check(w[H_MODES] + (size_t)w[H_NMODES] * MODE_SIZE <= n);
    for (uint32_t k = 0; k < w[H_NMODES]; ++k) check(w[w[H_MODES] + k * MODE_SIZE + MODE_FLAG] <= 1 && w[w[H_MODES] + k * MODE_SIZE + MODE_MAPPING] < nm);
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const long iterations = std::atol(argv[1]);
    std::vector<uint8_t> file;
    {
        FILE *fp = std::fopen(argv[2], "rb");
        if (!fp) return 2;
        uint8_t buf[4096];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, fp)) > 0) file.insert(file.end(), buf, buf + n);
        std::fclose(fp);
    }
    // the file as it is
    std::vector<sk_ogg::Packet> packets;
    {
        sk_ogg::Parser parser;
        std::string text;
        check(parser.add(file.data(), file.size(), &text) && parser.finish(&text));
        for (auto &p : parser.pending) packets.push_back(p);
    }
    check(packets.size() > 4);
    sk_vorbis::Ident ident;
    sk_vorbis::Setup whole;
    std::string text;
    check(sk_vorbis::parse_ident(packets[0].data.data(), packets[0].data.size(), &ident, &text) == 0);
    check(sk_vorbis::parse_comment(packets[1].data.data(), packets[1].data.size(), &text) == 0);
    check(sk_vorbis::parse_setup(packets[2].data.data(), packets[2].data.size(), ident, &whole, &text) == 0);
    check_blob(whole);
    for (long it = 0; it < iterations; ++it) {
        // ---- the Ogg bytes, damaged (with and without the page CRCs mended), cut, in pieces ----
        if (it % 4 == 0) {
            std::vector<uint8_t> s(file);
            const uint32_t how = rnd() % 4;
            if (how == 0) mutate(s.data(), s.size(), 2);
            else if (how == 1) s.resize(rnd() % s.size());
            else if (how == 2) mutate(s.data(), 400, 3);
            if (how != 3 && rnd() % 2) {  // mend the CRCs, so that the damage reaches the checks behind them
                for (size_t at = 0; at + 27 <= s.size();) {
                    if (std::memcmp(&s[at], "OggS", 4)) break;
                    size_t total = 27 + s[at + 26];
                    if (at + total > s.size()) break;
                    for (size_t i = 0; i < s[at + 26]; ++i) total += s[at + 27 + i];
                    if (at + total > s.size()) break;
                    const uint32_t crc = sk_ogg::page_crc(&s[at], total);
                    s[at + 22] = (uint8_t)crc, s[at + 23] = (uint8_t)(crc >> 8), s[at + 24] = (uint8_t)(crc >> 16), s[at + 25] = (uint8_t)(crc >> 24);
                    at += total;
                }
            }
            auto p = heap(s.data(), s.size());
            sk_ogg::Parser parser;
            std::string why;
            bool ok = true;
            const size_t piece = 1 + rnd() % 2000;
            size_t bytes = 0;
            for (size_t at = 0; ok && at < s.size(); at += piece) ok = parser.add(p.get() + at, std::min(piece, s.size() - at), &why);
            ok = ok && parser.finish(&why);
            for (auto &k : parser.pending) bytes += k.data.size(), check(k.data.size() <= sk_ogg::kMaxPacketBytes);
            check(bytes <= s.size());
            if (ok) ++g_oggs;
            else ++g_ogg_errors, check(!why.empty());
        }
        // ---- the identification and comment headers ----
        {
            std::vector<uint8_t> c(packets[0].data);
            if (rnd() % 4 == 0) c.resize(rnd() % (c.size() + 1));
            mutate(c.data(), c.size(), 2);
            auto p = heap(c.data(), c.size());
            sk_vorbis::Ident id;
            std::string why;
            if (sk_vorbis::parse_ident(p.get(), c.size(), &id, &why) == 0)
                ++g_idents, check(id.channels >= 1 && id.blocksize_0 >= 64 && id.blocksize_1 <= 8192 && id.blocksize_0 <= id.blocksize_1 && id.sample_rate);
            else ++g_ident_errors, check(!why.empty());
            std::vector<uint8_t> m(packets[1].data);
            if (rnd() % 4 == 0) m.resize(rnd() % (m.size() + 1));
            mutate(m.data(), m.size(), 2);
            auto q = heap(m.data(), m.size());
            if (sk_vorbis::parse_comment(q.get(), m.size(), &why) == 0) ++g_comments;
            else ++g_comment_errors, check(!why.empty());
        }
        // ---- the setup header, damaged or cut, under an identification header that may differ; then packets' first bits ----
        {
            std::vector<uint8_t> c(packets[2].data);
            if (rnd() % 8 == 0) c.resize(rnd() % (c.size() + 1));
            mutate(c.data(), c.size(), 1 + rnd() % 3);
            auto p = heap(c.data(), c.size());
            sk_vorbis::Ident id = ident;
            if (rnd() % 4 == 0) id.channels = (uint8_t)(1 + rnd() % 10);
            if (rnd() % 4 == 0) id.blocksize_0 = (uint16_t)(64u << (rnd() % 4)), id.blocksize_1 = (uint16_t)(id.blocksize_0 << (rnd() % 5));
            sk_vorbis::Setup s;
            std::string why;
            const int rc = sk_vorbis::parse_setup(p.get(), c.size(), id, &s, &why);
            if (rc == 0) {
                ++g_setups;
                check_blob(s);
                const sk_ogg::Packet &k = packets[3 + rnd() % (packets.size() - 3)];
                size_t len = rnd() % 4 ? k.data.size() : rnd() % 3;
                auto a = heap(k.data.data(), len);
                mutate(a.get(), len, 2);
                sk_vorbis::PacketHead h;
                const int st = sk_vorbis::packet_head(s, a.get(), len, &h);
                if (st == 0) check(h.mode < s.modes.size() && (h.n == s.bs[0] || h.n == s.bs[1]));
                else check(st == sk_vorbis::kNotAudio || st == sk_vorbis::kBadMode || st == sk_vorbis::kShort);
            } else {
                ++g_setup_errors;
                check(!why.empty() && (rc == sk_vorbis::kErrStream || rc == sk_vorbis::kUnsupported));
            }
        }
    }
    std::printf("fuzz_vorbis ok: %ld iterations, Ogg streams %zu / %zu rejected, identification headers %zu / %zu rejected, comment headers %zu / %zu "
                "rejected, setup headers %zu / %zu rejected\n",
                iterations, g_oggs, g_ogg_errors, g_idents, g_ident_errors, g_comments, g_comment_errors, g_setups, g_setup_errors);
    return g_oggs && g_ogg_errors && g_idents && g_ident_errors && g_comments && g_comment_errors && g_setups && g_setup_errors ? 0 : 1;
}

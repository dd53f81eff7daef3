// Mutation fuzz of the host side of the ALAC path -- cookie parse, the packet's frame count, the CAF packet index from its parts and
// from a whole file -- built with AddressSanitizer + UBSan on the CPU (tests/test_alac_cpu.py::test_mutated_files_under_sanitizers).
// The bytes come from the network: whatever arrives, every call must come back with a result or a text, with no out-of-bounds access
// and no undefined behaviour; every packet an index hands out lies inside the data chunk it was told of, is not empty and is not above
// 16 MiB.  Every buffer handed in is a heap block of exactly the length named, so that a read past it is seen.
//   usage: fuzz_alac ITERATIONS file.caf
#include "../soundkit_amd/csrc/alac_stream.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#define check(cond) ((cond) ? (void)0 : (std::fprintf(stderr, "fuzz_alac: check failed at line %d\n", __LINE__), std::abort()))

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    g_seed ^= g_seed << 13, g_seed ^= g_seed >> 7, g_seed ^= g_seed << 17;
    return (uint32_t)(g_seed >> 16);
}

static size_t g_cookies = 0, g_cookie_errors = 0, g_counts = 0, g_count_errors = 0, g_indexes = 0, g_index_errors = 0, g_files = 0, g_file_errors = 0;

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

static void check_config(const sk_alac_config &c) {
    check(c.sample_rate > 0 && c.channels >= 1 && c.channels <= 8 && (c.bit_depth == 16 || c.bit_depth == 24 || c.bit_depth == 32));
    check(c.frame_length >= 1 && c.frame_length <= 65536);
}

static void check_index(const sk_alac::CafIndex &ix, uint64_t data_offset, uint64_t data_size) {
    check_config(ix.config);
    check(ix.frames_per_packet >= 1 && ix.frames_per_packet <= 65536);
    uint64_t at = data_offset + 4;
    for (const sk_alac::PacketRange &p : ix.packets) {
        check(p.offset == at && p.size >= 1 && p.size <= sk_alac::kMaxPacketBytes);
        at += p.size;
    }
    check(at == data_offset + data_size);
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
    // the file as it is: the index, and from it the chunks
    sk_alac::CafIndex whole;
    std::string text;
    check(sk_alac::caf_index_from_file(file.data(), file.size(), &whole, &text));
    check(whole.packets.size() >= 2);
    size_t desc_at = 0, kuki_at = 0, kuki_len = 0, pakt_at = 0, pakt_len = 0, data_at = 0, data_len = 0;
    for (size_t at = 8; at + 12 <= file.size();) {
        const uint64_t size = sk_alac::be64(&file[at + 4]);
        if (!std::memcmp(&file[at], "desc", 4)) desc_at = at + 12;
        if (!std::memcmp(&file[at], "kuki", 4)) kuki_at = at + 12, kuki_len = (size_t)size;
        if (!std::memcmp(&file[at], "pakt", 4)) pakt_at = at + 12, pakt_len = (size_t)size;
        if (!std::memcmp(&file[at], "data", 4)) data_at = at + 12, data_len = (size_t)size;
        at += 12 + (size_t)size;
    }
    check(desc_at && kuki_at && pakt_at && data_at);
    check_index(whole, data_at, data_len);
    for (long it = 0; it < iterations; ++it) {
        // ---- the cookie, damaged, cut short, in each wrapping ----
        {
            std::vector<uint8_t> c(file.begin() + (ptrdiff_t)kuki_at, file.begin() + (ptrdiff_t)(kuki_at + kuki_len));
            const uint32_t how = rnd() % 3;
            if (how == 1 && c.size() >= 24) c.erase(c.begin(), c.end() - 24);      // the bare config
            if (how == 2 && c.size() >= 24) c.erase(c.begin(), c.end() - 24), c.insert(c.begin(), 4, 0);  // the MP4 payload
            if (rnd() % 4 == 0) c.resize(rnd() % (c.size() + 1));
            mutate(c.data(), c.size(), 3);
            auto p = heap(c.data(), c.size());
            sk_alac_config cfg{};
            std::string why;
            if (sk_alac::parse_cookie(p.get(), c.size(), &cfg, &why)) ++g_cookies, check_config(cfg);
            else ++g_cookie_errors, check(!why.empty());
        }
        // ---- a packet, damaged and cut short: its frame count ----
        {
            const sk_alac::PacketRange &r = whole.packets[rnd() % whole.packets.size()];
            size_t len = 1 + rnd() % 64;
            if (len > r.size) len = r.size;
            auto p = heap(&file[(size_t)r.offset], len);
            mutate(p.get(), len, 3);
            uint32_t frames = 0;
            const int rc = sk_alac::packet_frames(whole.config, p.get(), rnd() % 8 ? len : rnd() % (len + 1), &frames);
            if (rc == SK_OK) ++g_counts, check(frames >= 1 && frames <= whole.config.frame_length);
            else ++g_count_errors, check(rc == SK_ALAC_INVALID || rc == SK_ALAC_UNSUPPORTED);
        }
        // ---- the index from its parts: description, cookie and table damaged, the data range at will ----
        {
            auto d = heap(&file[desc_at], 32);
            auto k = heap(&file[kuki_at], kuki_len);
            size_t tl = rnd() % 4 ? pakt_len : rnd() % (pakt_len + 1);
            auto t = heap(&file[pakt_at], tl);
            if (rnd() % 3 == 0) mutate(d.get(), 32, 2);
            if (rnd() % 3 == 0) mutate(k.get(), kuki_len, 2);
            if (rnd() % 2 == 0) mutate(t.get(), tl, 2);
            uint64_t off = data_at, size = data_len;
            if (rnd() % 8 == 0) size = rnd() % 8 == 0 ? ~0ull - rnd() % 4 : rnd() % (2 * data_len);
            if (rnd() % 8 == 0) off = ~0ull - rnd() % 8;
            sk_alac::CafIndex ix;
            std::string why;
            if (sk_alac::caf_index(d.get(), rnd() % 16 ? 32 : rnd() % 33, k.get(), kuki_len, t.get(), tl, off, size, &ix, &why)) ++g_indexes, check_index(ix, off, size);
            else ++g_index_errors, check(!why.empty());
        }
        // ---- the whole file, damaged in its chunk headers or anywhere, or cut ----
        if (it % 4 == 0) {
            std::vector<uint8_t> s(file);
            const uint32_t how = rnd() % 4;
            if (how == 0) s[rnd() % 200] = (uint8_t)rnd();
            else if (how == 1) mutate(s.data(), s.size(), 2);
            else if (how == 2) s.resize(rnd() % s.size());
            else mutate(s.data() + pakt_at - 12, pakt_len + 12, 2);
            auto p = heap(s.data(), s.size());
            sk_alac::CafIndex ix;
            std::string why;
            if (sk_alac::caf_index_from_file(p.get(), s.size(), &ix, &why)) {
                ++g_files;
                check_config(ix.config);
                for (const sk_alac::PacketRange &r : ix.packets) check(r.size >= 1 && r.offset + r.size <= s.size());
            } else {
                ++g_file_errors, check(!why.empty());
            }
        }
    }
    std::printf("fuzz_alac ok: %ld iterations, cookies %zu / %zu rejected, frame counts %zu / %zu rejected, indexes %zu / %zu rejected, files %zu / %zu rejected\n",
                iterations, g_cookies, g_cookie_errors, g_counts, g_count_errors, g_indexes, g_index_errors, g_files, g_file_errors);
    return g_cookies && g_cookie_errors && g_counts && g_count_errors && g_indexes && g_index_errors && g_files && g_file_errors ? 0 : 1;
}

// Mutation fuzz of the host side of the FLAC path -- frame-header parse, the CRC-bounded frame scan and the incremental stream reader --
// built with AddressSanitizer + UBSan on the CPU (tests/test_flac_cpu.py::test_mutated_streams_under_sanitizers).  The bytes come from
// the network: whatever arrives, every call must come back with a status, with no out-of-bounds access and no undefined behaviour;
// every frame handed out lies inside the bytes given, within the frame bound, and its CRC-16 holds.  Every buffer handed in is a heap
// block of exactly the length named, so that a read past it is seen.
//   usage: fuzz_flac ITERATIONS file.flac
#include "../soundkit_amd/csrc/flac_stream.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#define check(cond) ((cond) ? (void)0 : (std::fprintf(stderr, "fuzz_flac: check failed at line %d\n", __LINE__), std::abort()))

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    g_seed ^= g_seed << 13, g_seed ^= g_seed >> 7, g_seed ^= g_seed << 17;
    return (uint32_t)(g_seed >> 16);
}

static size_t g_headers = 0, g_header_errors = 0, g_scanned = 0, g_scan_errors = 0, g_read = 0, g_read_errors = 0;

static void check_frame(const uint8_t *d, size_t len, const sk_flac_frame_info &f, const sk_flac_streaminfo *info) {
    check((size_t)f.offset + f.frame_bytes <= len && f.frame_bytes >= (uint32_t)f.header_bytes + 3);
    check(f.channels >= 1 && f.channels <= 8 && f.bits_per_sample >= 4 && f.bits_per_sample <= 32 && f.block_size >= 1 && f.block_size <= 65536);
    check(f.header_bytes >= 6 && f.header_bytes <= 16 && f.assignment <= 10);
    check(f.frame_bytes <= sk_flac::frame_bound(f, info) + 16);
    check(sk_flac::crc16(d + f.offset, f.frame_bytes, 0) == 0);
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
    // the file's own frames, through the reader
    std::vector<size_t> starts;
    sk_flac_streaminfo info{};
    {
        sk_flac::Reader r;
        std::vector<sk_flac_frame_info> got(4096);
        uint32_t n = 0;
        const uint8_t *data = nullptr;
        check(r.add(file.data(), file.size(), got.data(), (uint32_t)got.size(), &n, &data) && r.have_info());
        info = r.info();
        const size_t first = file.size() - r.buffered_bytes() - (n ? (size_t)got[n - 1].offset + got[n - 1].frame_bytes : 0);
        for (uint32_t i = 0; i < n; ++i) starts.push_back(first + got[i].offset);
        check(starts.size() >= 2);
    }
    for (long it = 0; it < iterations; ++it) {
        // ---- a header, damaged, cut short or not, with and without STREAMINFO ----
        {
            const size_t at = starts[rnd() % starts.size()];
            size_t len = 1 + rnd() % 20;
            if (at + len > file.size()) len = file.size() - at;
            std::unique_ptr<uint8_t[]> h(new uint8_t[len]);
            std::copy(file.begin() + (ptrdiff_t)at, file.begin() + (ptrdiff_t)(at + len), h.get());
            for (uint32_t k = rnd() % 4; k > 0; --k) h[rnd() % len] = (uint8_t)rnd();
            sk_flac_frame_info f;
            const int rc = sk_flac::parse_header(h.get(), len, rnd() & 1 ? &info : nullptr, &f);
            if (rc == SK_OK) {
                ++g_headers;
                check(f.header_bytes <= len && f.channels >= 1 && f.channels <= 8 && f.bits_per_sample >= 4 && f.bits_per_sample <= 32);
                check(f.block_size >= 1 && f.block_size <= 65536 && f.assignment <= 10);
            } else {
                ++g_header_errors;
                check(rc <= SK_FLAC_NEED_MORE && rc >= SK_FLAC_NEED_STREAMINFO);
            }
        }
        // ---- a stretch of frames, damaged, through the scan ----
        {
            const size_t from = starts[rnd() % starts.size()];
            size_t len = 1 + rnd() % 6000;
            if (from + len > file.size()) len = file.size() - from;
            std::unique_ptr<uint8_t[]> piece(new uint8_t[len]);
            std::copy(file.begin() + (ptrdiff_t)from, file.begin() + (ptrdiff_t)(from + len), piece.get());
            for (uint32_t k = rnd() % 3; k > 0; --k) piece[rnd() % len] ^= (uint8_t)(1u << (rnd() & 7));
            std::vector<sk_flac_frame_info> found(1 + rnd() % 8);
            uint32_t n = 0;
            size_t consumed = 0;
            const sk_flac_streaminfo *si = rnd() & 1 ? &info : nullptr;
            const int rc = sk_flac::scan(piece.get(), len, si, (rnd() & 1) != 0, found.data(), (uint32_t)found.size(), &n, &consumed);
            check(consumed <= len && n <= found.size());
            if (rc != SK_OK) ++g_scan_errors, check(rc <= SK_FLAC_NO_SYNC && rc >= SK_FLAC_NEED_STREAMINFO);
            for (uint32_t i = 0; i < n; ++i) {
                check_frame(piece.get(), consumed, found[i], si);
                ++g_scanned;
            }
        }
        // ---- the whole stream, damaged in the metadata or a frame, in pieces through the reader ----
        if (it % 16 == 0) {
            std::vector<uint8_t> s(file);
            const uint32_t how = rnd() % 4;
            if (how == 0) s[rnd() % 64] = (uint8_t)rnd();
            else if (how == 1) s[rnd() % s.size()] ^= (uint8_t)(1u << (rnd() & 7));
            else if (how == 2) s.resize(rnd() % s.size());
            sk_flac::Reader r;
            std::vector<sk_flac_frame_info> got(1 + rnd() % 64);
            size_t at = 0;
            bool ok = true;
            while (ok) {
                size_t len = at < s.size() ? 1 + rnd() % 3000 : 0;
                if (at + len > s.size()) len = s.size() - at;
                std::unique_ptr<uint8_t[]> piece(new uint8_t[len ? len : 1]);
                std::copy(s.begin() + (ptrdiff_t)at, s.begin() + (ptrdiff_t)(at + len), piece.get());
                uint32_t n = 0;
                const uint8_t *data = nullptr;
                ok = r.add(piece.get(), len, got.data(), (uint32_t)got.size(), &n, &data);
                at += len;
                if (!ok) {
                    check(!r.error().empty());
                    ++g_read_errors;
                    break;
                }
                for (uint32_t i = 0; i < n; ++i) {
                    check_frame(data, (size_t)got[i].offset + got[i].frame_bytes, got[i], &r.info());
                    ++g_read;
                }
                if (len == 0 && n == 0) break;
            }
        }
    }
    std::printf("fuzz_flac ok: %ld iterations, headers %zu / %zu rejected, %zu frames scanned (%zu scans failed), %zu frames read (%zu streams rejected)\n",
                iterations, g_headers, g_header_errors, g_scanned, g_scan_errors, g_read, g_read_errors);
    return g_headers && g_header_errors && g_scanned && g_scan_errors && g_read && g_read_errors ? 0 : 1;
}

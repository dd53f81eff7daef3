// Mutation fuzz of the host side of the MPEG Layer I / II path -- header parse, frame scan, the serial front of a frame, and the
// check that stands between a record and the kernel -- built with AddressSanitizer + UBSan on the CPU
// (tests/test_mp12_cpu.py::test_mutated_frames_under_sanitizers).  The bytes come from the network: whatever arrives, every
// call must come back with a status, with no out-of-bounds access and no undefined behaviour; and a frame the parse accepts
// must be one whose every sample code -- at the positions the kernel computes them, csrc/mp12_synth.hip -- ends inside the
// frame.  Every buffer handed in is a heap block of exactly the length named, so that a read past it is seen.
//   usage: fuzz_mp12 ITERATIONS file.mp2...
#include "../soundkit_amd/csrc/mp12_bitstream.cpp"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#define check(cond) ((cond) ? (void)0 : (std::fprintf(stderr, "fuzz_mp12: check failed at line %d\n", __LINE__), std::abort()))

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    g_seed ^= g_seed << 13, g_seed ^= g_seed >> 7, g_seed ^= g_seed << 17;
    return (uint32_t)(g_seed >> 16);
}

// the kernel's walk over a record: where the last bit it would fetch a code from stands
static uint64_t last_code_bit(const sk_mpa_frame_record &r) {
    uint64_t end = r.sample_bit;
    for (int g = 0; g < 12; ++g) {
        uint32_t at = 0;
        for (int sb = 0; sb < 32; ++sb)
            for (int c = 0; c < 2; ++c) {
                const bool sent = sb < r.sblimit && c < r.channels && (c == 0 || sb < r.bound);
                const int w = sent ? sk_mp12::class_bits(r.layer, r.cls[c][sb]) : 0;
                check(w >= 0);
                const uint64_t stop = (uint64_t)r.sample_bit + (uint64_t)g * r.granule_bits + at + (uint32_t)w;
                if (w && stop > end) end = stop;
                at += (uint32_t)w;
            }
        check(at == r.granule_bits);
    }
    return end;
}

static size_t g_accepted = 0, g_rejected = 0, g_scanned = 0;

static void one_frame(const std::vector<uint8_t> &bytes) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[bytes.size() ? bytes.size() : 1]);
    std::copy(bytes.begin(), bytes.end(), exact.get());
    sk_mpa_frame_info h;
    const int rc = sk_mp12::parse_header(exact.get(), bytes.size(), &h);
    if (rc != SK_OK) {
        check(rc == SK_MP3_NEED_MORE || rc == SK_MP3_NO_SYNC || rc == SK_MP3_UNSUPPORTED);
        return;
    }
    check(h.layer >= 1 && h.layer <= 3 && h.channels >= 1 && h.channels <= 2 && h.frame_bytes >= 5 && h.frame_bytes <= 2048);
    sk_mpa_frame_record r;
    const int frc = sk_mp12::parse_frame(exact.get(), bytes.size(), &h, &r);
    if (frc != SK_OK) {
        check(frc == SK_MP3_NEED_MORE || frc == SK_MP3_INVALID || frc == SK_MP3_UNSUPPORTED);
        ++g_rejected;
        return;
    }
    ++g_accepted;
    check(bytes.size() >= h.frame_bytes && r.byte_len == h.frame_bytes);
    check(sk_mp12::record_adds_up(r));
    check(last_code_bit(r) <= (uint64_t)r.byte_len * 8);
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const long iterations = std::atol(argv[1]);
    std::vector<std::vector<uint8_t>> files;
    for (int i = 2; i < argc; ++i) {
        FILE *f = std::fopen(argv[i], "rb");
        if (!f) return 2;
        std::vector<uint8_t> d;
        uint8_t buf[4096];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n);
        std::fclose(f);
        files.push_back(d);
    }
    for (long it = 0; it < iterations; ++it) {
        const std::vector<uint8_t> &file = files[rnd() % files.size()];
        // ---- a stretch of the stream, damaged, through the scan (layer known and not) ----
        size_t from = rnd() % file.size(), len = 1 + rnd() % 3000;
        if (from + len > file.size()) len = file.size() - from;
        std::vector<uint8_t> piece(file.begin() + (ptrdiff_t)from, file.begin() + (ptrdiff_t)(from + len));
        for (uint32_t k = rnd() % 6; k > 0; --k) piece[rnd() % piece.size()] ^= (uint8_t)(1u << (rnd() & 7));
        if (rnd() % 4 == 0) piece.insert(piece.begin() + (ptrdiff_t)(rnd() % piece.size()), (size_t)(rnd() % 9), (uint8_t)0xff);
        {
            std::unique_ptr<uint8_t[]> exact(new uint8_t[piece.size()]);
            std::copy(piece.begin(), piece.end(), exact.get());
            std::vector<sk_mpa_frame_info> found(16);
            uint32_t layer = rnd() % 4, n = 0;
            size_t consumed = 0;
            check(sk_mp12::scan(exact.get(), piece.size(), &layer, found.data(), (uint32_t)found.size(), &n, &consumed) == SK_OK);
            check(consumed <= piece.size() && layer <= 3);
            for (uint32_t i = 0; i < n && i < found.size(); ++i) {
                check((size_t)found[i].offset + found[i].frame_bytes <= consumed);
                check(!layer || found[i].layer == layer);
                ++g_scanned;
            }
        }
        // ---- one frame, damaged where it hurts: the header's fields, the allocation, anywhere; cut short or not ----
        const size_t first = (rnd() % (file.size() / 576)) * 576;
        std::vector<uint8_t> frame(file.begin() + (ptrdiff_t)first, file.begin() + (ptrdiff_t)std::min(file.size(), first + 2048));
        switch (rnd() % 6) {
        case 0: frame[1] = (uint8_t)(0xe0 | (rnd() & 0x1f)); break;                                  // version, layer, protection
        case 1: frame[2] = (uint8_t)rnd(); break;                                                    // bit rate, sampling rate, padding
        case 2: frame[3] = (uint8_t)rnd(); break;                                                    // mode, mode extension
        case 3: for (int k = 0; k < 24; ++k) frame[4 + rnd() % 40] = (uint8_t)rnd(); break;          // the allocation
        case 4: frame[1] = 0xff, frame[2] = (uint8_t)(rnd() | 0x10), frame[4 + rnd() % 32] = 0xff; break;  // Layer I, forbidden allocations
        default: for (uint32_t k = 1 + rnd() % 8; k > 0; --k) frame[rnd() % frame.size()] ^= (uint8_t)(1u << (rnd() & 7)); break;
        }
        if (rnd() % 3 == 0) frame.resize(rnd() % frame.size());
        one_frame(frame);
        // ---- a record made of noise must not pass the check in front of the kernel unless it adds up ----
        sk_mpa_frame_record r;
        for (size_t k = 0; k < sizeof r; ++k) ((uint8_t *)&r)[k] = (uint8_t)(rnd() % 5 == 0 ? rnd() : rnd() % 4);
        r.layer = (uint8_t)(1 + rnd() % 2), r.channels = (uint8_t)(1 + rnd() % 2), r.granules = 12;
        if (sk_mp12::record_adds_up(r)) check(last_code_bit(r) <= (uint64_t)r.byte_len * 8);
    }
    std::printf("fuzz_mp12 ok: %ld iterations, %zu frames accepted, %zu rejected, %zu found by the scan\n", iterations, g_accepted, g_rejected, g_scanned);
    return g_accepted && g_rejected && g_scanned ? 0 : 1;
}

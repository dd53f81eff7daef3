// Seeded mutation harness for the AIFF / AIFF-C walker (csrc/pcm_stream.h, AiffStream), built with -fsanitize=address,undefined by
// tests/test_aiff_stream_cpu.py.  (Test infrastructure: the product library never contains this file.)
//
//   fuzz_aiff_stream <iterations> <file>...
//
// Per iteration and file: the file's first 256 bytes with a few seeded mutations (byte flips, 32-bit big-endian fields set to edge
// values, a chunk id or a compression tag overwritten), followed by the rest of the file (a long one cut to 16 KiB, with FORM and SSND told so), fed to a fresh AiffStream in
// ragged pieces, then the finalising empty add.  Checked: no crash and no sanitizer report; every piece is a whole number of sample
// groups of the encoding the walker reports, the pieces follow each other without a gap, no piece holds more than was fed, what the
// walker holds back stays under 4096 + the largest piece fed, and a rejected stream has a text.  Prints "ok <streams that finished>
// err <streams that were rejected>".
#include "../soundkit_amd/csrc/pcm_stream.h"

#include <cstdio>
#include <cstdlib>

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(2);                                               \
        }                                                               \
    } while (0)

static bool feed(sk_pcm::AiffStream &st, const std::vector<uint8_t> &data, bool *gave) {
    size_t pos = 0;
    uint64_t next = 0;
    bool last = false;
    while (!last) {
        size_t n = 1 + rnd() % (rnd() % 4 == 0 ? 700 : 40);
        if (n > data.size() - pos) n = data.size() - pos;
        last = n == 0;  // the finalising add
        sk_pcm::Piece piece;
        std::string err;
        if (!st.add(data.data() + pos, n, piece, err)) {
            CHECK(!err.empty());
            std::string again;
            CHECK(!st.add(data.data(), 1, piece, again) && again == err);  // a failed walker stays failed
            return false;
        }
        pos += n;
        CHECK(st.buffered_bytes() < 4096 + 700);
        if (piece.len) {
            CHECK(st.have_info() && st.channels() >= 1 && st.channels() <= 32 && st.encoding() < sk_pcm::kAiffEncodings);
            const size_t group = sk_pcm::aiff_group_bytes(st.encoding(), st.channels());
            CHECK(piece.len % group == 0);
            CHECK(piece.stream_offset == next && next + piece.len <= pos);
            volatile uint8_t sink = 0;
            for (size_t i = 0; i < piece.len; ++i) sink = sink ^ piece.data[i];  // every byte is readable
            next += piece.len;
            *gave = true;
        }
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc < 3) return 1;
    const int iterations = std::atoi(argv[1]);
    long ok = 0, bad = 0;
    for (int f = 2; f < argc; ++f) {
        std::vector<uint8_t> file;
        if (FILE *fp = std::fopen(argv[f], "rb")) {
            file.resize(16384);
            const size_t got = std::fread(file.data(), 1, file.size(), fp);
            const bool cut = got == file.size() && std::fgetc(fp) != EOF;
            file.resize(got);
            std::fclose(fp);
            if (cut) {  // a long fixture: FORM and SSND are told to end where the copy does, on a whole sample of every width
                size_t at = 12;
                while (at + 8 <= 256 && std::memcmp(file.data() + at, "SSND", 4) != 0) at += 1;
                CHECK(at + 8 <= 256);
                const size_t audio = (file.size() - (at + 16)) / 24 * 24;
                file.resize(at + 16 + audio);
                const uint32_t ssnd = (uint32_t)(audio + 8), form = (uint32_t)(file.size() - 8);
                for (int k = 0; k < 4; ++k) file[at + 4 + k] = (uint8_t)(ssnd >> (24 - 8 * k)), file[4 + k] = (uint8_t)(form >> (24 - 8 * k));
            }
        }
        CHECK(file.size() > 256);
        for (int it = 0; it < iterations; ++it) {
            std::vector<uint8_t> data = file;
            const int edits = it == 0 ? 0 : 1 + (int)(rnd() % 4);
            for (int e = 0; e < edits; ++e) {
                const size_t at = rnd() % 252;
                switch (rnd() % 4) {
                case 0: data[at] ^= (uint8_t)(1u << (rnd() % 8)); break;
                case 1: data[at] = (uint8_t)rnd(); break;
                case 2: {
                    static const uint32_t edge[] = {0, 1, 3, 4, 7, 8, 9, 17, 18, 21, 22, 4096, 4097, 0x7fffffffu, 0xfffffffeu, 0xffffffffu};
                    const uint32_t v = edge[rnd() % (sizeof edge / sizeof edge[0])];
                    for (int k = 0; k < 4; ++k) data[at + k] = (uint8_t)(v >> (24 - 8 * k));
                    break;
                }
                default: {
                    static const char *ids[] = {"COMM", "SSND", "FORM", "AIFC", "AIFF", "ima4", "sowt", "fl64", "MARK", "raw "};
                    std::memcpy(data.data() + at, ids[rnd() % 10], 4);
                    break;
                }
                }
            }
            sk_pcm::AiffStream st;
            bool gave = false;
            const bool fine = feed(st, data, &gave);
            if (it == 0) CHECK(fine && gave);  // the fixture itself
            ok += fine;
            bad += !fine;
        }
    }
    std::printf("ok %ld err %ld\n", ok, bad);
    return 0;
}

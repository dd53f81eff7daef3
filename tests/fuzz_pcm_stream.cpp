// Seeded mutation harness for the WAV walker and the raw PCM framer (csrc/pcm_stream.h), built with
// -fsanitize=address,undefined by tests/test_pcm_stream_cpu.py.  (Test infrastructure: the product library never contains this file.)
//
//   fuzz_pcm_stream <iterations> <file>...
//
// Per iteration and file: the file's first 256 bytes with a few seeded mutations (byte flips, 32-bit fields set to edge values, a chunk
// id overwritten), followed by the rest of the file up to 4096 bytes, fed to a fresh WavStream in ragged pieces.  Checked: no crash and
// no sanitizer report; every piece lies inside the bytes fed so far, holds exactly those bytes, follows the piece before it without
// overlap and is a whole number of frames of the format the walker reports.  The raw framer gets the same bytes with a drawn frame
// size.  Prints "ok <streams that gave pieces> err <streams that were rejected>".
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

template <typename Stream, typename FrameBytes>
static bool feed(Stream &st, const std::vector<uint8_t> &data, FrameBytes frame_bytes, bool *gave) {
    size_t pos = 0;
    uint64_t next = 0;
    while (pos < data.size()) {
        size_t n = 1 + rnd() % (rnd() % 4 == 0 ? 700 : 40);
        if (n > data.size() - pos) n = data.size() - pos;
        sk_pcm::Piece piece;
        std::string err;
        if (!st.add(data.data() + pos, n, piece, err)) {
            CHECK(!err.empty());
            return false;
        }
        pos += n;
        if (piece.len) {
            const size_t frame = frame_bytes();
            CHECK(frame > 0 && piece.len % frame == 0);
            CHECK(piece.stream_offset >= next && piece.stream_offset + piece.len <= pos);
            CHECK(std::memcmp(piece.data, data.data() + piece.stream_offset, piece.len) == 0);
            next = piece.stream_offset + piece.len;
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
            file.resize(4096);
            file.resize(std::fread(file.data(), 1, file.size(), fp));
            std::fclose(fp);
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
                    static const uint32_t edge[] = {0, 1, 3, 15, 16, 17, 39, 40, 4096, 4097, 0x7fffffffu, 0xfffffffeu, 0xffffffffu};
                    const uint32_t v = edge[rnd() % (sizeof edge / sizeof edge[0])];
                    std::memcpy(data.data() + at, &v, 4);
                    break;
                }
                default: std::memcpy(data.data() + at, rnd() % 2 ? "data" : (rnd() % 2 ? "fmt " : "ds64"), 4); break;
                }
            }
            if (rnd() % 8 == 0) std::memcpy(data.data(), "RF64", 4);
            sk_pcm::WavStream wav;
            bool gave = false;
            const bool fine = feed(wav, data, [&] { return (size_t)(wav.bits() / 8) * wav.channels(); }, &gave);
            if (it == 0) CHECK(fine && gave);  // the fixture itself
            ok += fine && gave;
            bad += !fine;
            const size_t frame = 1 + rnd() % 9;
            sk_pcm::RawPcmStream raw(frame);
            gave = false;
            CHECK(feed(raw, data, [&] { return frame; }, &gave));
            std::string err;
            CHECK(raw.flush(err) == (data.size() % frame == 0));
        }
    }
    std::printf("ok %ld err %ld\n", ok, bad);
    return 0;
}

// Seeded mutation harness for the WAV walker's coded mode (csrc/pcm_stream.h, WavStream(true)), built with
// -fsanitize=address,undefined by tests/test_wav_coded_cpu.py.  (Test infrastructure: the product library never contains this file.)
//
//   fuzz_wav_coded <iterations> <file>...
//
// Per iteration and file: the file's header (everything up to the data chunk's payload, at most 256 bytes) with a few seeded
// mutations (byte flips, 16- and 32-bit little-endian fields set to edge values, a chunk id overwritten), followed by the rest of the
// file, fed to a fresh coded walker in ragged pieces, then an empty add.  Checked: no crash and no sanitizer report; every piece is a
// whole number of the units the walker reports (frames, for the two ADPCM tags blocks), the pieces follow each other without a gap or
// an overlap, no piece holds more than was fed, every byte of it is readable, frames per block stay within the 65 536 budget and agree
// with the block size, total_frames is the fact chunk's count or whole blocks, and a rejected stream has a text.  Prints
// "ok <streams that were walked to the end> err <streams that were rejected>".
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

static bool feed(sk_pcm::WavStream &st, const std::vector<uint8_t> &data, bool *gave) {
    size_t pos = 0;
    uint64_t next = 0;
    bool last = false, first = true;
    while (!last) {
        size_t n = 1 + rnd() % (rnd() % 4 == 0 ? 700 : 40);
        if (n > data.size() - pos) n = data.size() - pos;
        last = n == 0;
        sk_pcm::Piece piece;
        std::string err;
        if (!st.add(data.data() + pos, n, piece, err)) {
            CHECK(!err.empty() && piece.len == 0);
            return false;
        }
        pos += n;
        if (piece.len) {
            const uint32_t tag = st.tag(), ch = st.channels(), unit = st.block_align(), per = st.frames_per_block();
            CHECK(ch >= 1 && st.sample_rate() >= 1 && unit >= 1 && per >= 1 && per <= sk_pcm::kMaxWavAdpcmBlockFrames);
            CHECK(tag == 1 || tag == 2 || tag == 3 || tag == 6 || tag == 7 || tag == 0x11);
            if (st.is_adpcm()) {
                CHECK(ch <= 2 && per == sk_pcm::wav_adpcm_block_frames(tag, ch, unit));
                CHECK(tag != 2 || (st.n_coef() >= 1 && st.n_coef() <= sk_pcm::kMaxWavAdpcmCoefs));
            } else {
                CHECK(per == 1 && unit == st.bits() / 8 * ch);
                CHECK((tag != 6 && tag != 7) || st.bits() == 8);
            }
            CHECK(piece.len % unit == 0);
            CHECK((first || piece.stream_offset == next) && piece.stream_offset + piece.len <= pos);
            CHECK(st.total_frames() >= 1 && (st.fact_frames() == 0 || !st.is_adpcm() || st.total_frames() >= st.fact_frames() || st.total_frames() % per == 0));
            volatile uint8_t sink = 0;
            for (size_t i = 0; i < piece.len; ++i) sink = sink ^ piece.data[i];
            next = piece.stream_offset + piece.len;
            first = false;
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
            file.resize(65536);
            file.resize(std::fread(file.data(), 1, file.size(), fp));
            std::fclose(fp);
        }
        size_t head = 12;
        while (head + 8 <= file.size() && head + 8 <= 256 && std::memcmp(file.data() + head, "data", 4) != 0) head += 1;
        CHECK(head + 8 <= 256 && head + 8 < file.size());
        head += 8;
        for (int it = 0; it < iterations; ++it) {
            std::vector<uint8_t> data = file;
            const int edits = it == 0 ? 0 : 1 + (int)(rnd() % 4);
            for (int e = 0; e < edits; ++e) {
                const size_t at = rnd() % (head - 4);
                switch (rnd() % 5) {
                case 0: data[at] ^= (uint8_t)(1u << (rnd() % 8)); break;
                case 1: data[at] = (uint8_t)rnd(); break;
                case 2: {
                    static const uint32_t edge[] = {0, 1, 2, 3, 4, 7, 15, 16, 18, 20, 22, 50, 4096, 4097, 0x7fffffffu, 0xfffffffeu, 0xffffffffu};
                    const uint32_t v = edge[rnd() % (sizeof edge / sizeof edge[0])];
                    for (int k = 0; k < 4; ++k) data[at + k] = (uint8_t)(v >> (8 * k));
                    break;
                }
                case 3: {
                    static const uint16_t edge[] = {0, 1, 2, 3, 4, 6, 7, 8, 13, 14, 0x11, 32, 33, 255, 256, 32768, 32771, 32772, 32774, 32775, 0xfffe, 0xffff};
                    const uint16_t v = edge[rnd() % (sizeof edge / sizeof edge[0])];
                    data[at] = (uint8_t)v, data[at + 1] = (uint8_t)(v >> 8);
                    break;
                }
                default: {
                    static const char *ids[] = {"fmt ", "fact", "data", "ds64", "RIFF", "RF64", "WAVE", "LIST"};
                    std::memcpy(data.data() + at, ids[rnd() % 8], 4);
                    break;
                }
                }
            }
            sk_pcm::WavStream st(true);
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

// fuzz_mp4.cpp -- csrc/mp4_stream.h alone under AddressSanitizer + UBSan on the CPU: seeded mutations of MP4 files through the whole-file
// index (with the trim of every sample it lists) and through the streaming demuxer, whole and in pieces.  Host code only.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o fuzz_mp4 fuzz_mp4.cpp
//   usage: fuzz_mp4 ITERATIONS_PER_FILE file.mp4 ...
//
// Checked beyond the sanitizers: a refusal carries a text; every sample the index lists lies inside the file; every packet the demuxer
// gives is no larger than the input; the unmutated file gives the same packets whole and in pieces; the demuxer never holds more than
// the largest box it had to gather plus one piece.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../soundkit_amd/csrc/mp4_stream.h"

#define check(cond) ((cond) ? (void)0 : (std::fprintf(stderr, "fuzz_mp4: check failed at line %d\n", __LINE__), std::abort()))

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}

struct Result {
    bool ok = false;
    size_t packets = 0;
    uint64_t bytes = 0, hash = 1469598103934665603ull;
};

static Result demux(const std::vector<uint8_t> &file, size_t piece) {
    sk_mp4::Demuxer d;
    Result r;
    auto drain = [&] {
        while (!d.packets.empty()) {
            const sk_mp4::Packet &p = d.packets.front();
            check(p.data.size() <= file.size());
            r.packets += 1, r.bytes += p.data.size();
            for (uint8_t b : p.data) r.hash = (r.hash ^ b) * 1099511628211ull;
            r.hash = (r.hash ^ p.start) * 1099511628211ull;
            d.packets.pop_front();
        }
    };
    bool ok = true;
    for (size_t at = 0; ok && at < file.size(); at += piece) {
        ok = d.add(file.data() + at, std::min(piece, file.size() - at));
        drain();
        check(d.buffered() <= sk_mp4::kMaxMetadataBytes + 16 + piece);
    }
    if (ok) ok = d.finish();
    drain();
    check(ok == !d.failed);
    check(ok || !d.error.empty());
    check(!d.add(file.data(), 1));  // after the end or a refusal: refused
    r.ok = ok;
    return r;
}

static bool index(const std::vector<uint8_t> &file) {
    sk_mp4::Track t;
    std::string error;
    static const uint8_t none[1] = {0};
    if (!sk_mp4::index_from_file(file.empty() ? none : file.data(), file.size(), &t, &error)) {
        check(!error.empty());
        return false;
    }
    check(t.codec == sk_mp4::kCodecAac || t.codec == sk_mp4::kCodecAlac);
    check(t.timescale != 0 && t.sample_rate != 0 && t.channels != 0);
    for (size_t i = 0; i < t.samples.size(); ++i) {
        const sk_mp4::Sample &s = t.samples[i];
        check(s.offset <= file.size() && s.size <= file.size() - s.offset);
        uint32_t first = 0, count = 0;
        for (uint32_t rate : {t.sample_rate, 44100u, 1u}) {
            if (!sk_mp4::trim(t, s, 1024, rate, &first, &count, &error)) continue;
            check(count <= 1024 && first <= 1024 && first + count <= 1024);
        }
    }
    uint8_t head[7];
    sk_mp4::adts_header(t.codec_private.data(), t.codec_private.size(), t.sample_rate, t.channels, t.samples.empty() ? 0 : t.samples[0].size, head);
    check(head[0] == 0xff);
    return true;
}

int main(int argc, char **argv) {
    if (argc < 3) return std::fprintf(stderr, "usage: fuzz_mp4 ITERATIONS_PER_FILE file.mp4 ...\n"), 2;
    const long iterations = std::atol(argv[1]);
    size_t runs = 0, indexed = 0, demuxed = 0;
    for (int a = 2; a < argc; ++a) {
        std::ifstream in(argv[a], std::ios::binary);
        const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        check(!file.empty());
        // the file as it is: the same packets however it arrives
        const Result whole = demux(file, file.size());
        for (size_t piece : {(size_t)1, (size_t)7, (size_t)4096}) {
            const Result r = demux(file, piece);
            check(r.ok == whole.ok && r.packets == whole.packets && r.bytes == whole.bytes && r.hash == whole.hash);
        }
        (void)index(file);
        for (long it = 0; it < iterations; ++it) {
            std::vector<uint8_t> m = file;
            const uint32_t kind = rnd() % 6;
            const uint32_t edits = 1 + rnd() % 4;
            for (uint32_t e = 0; e < edits; ++e) {
                const size_t at = rnd() % m.size();
                if (kind == 0) m[at] = (uint8_t)rnd();                                 // a byte anywhere
                else if (kind == 1) m[at] ^= (uint8_t)(1u << (rnd() % 8));             // a bit anywhere
                else if (kind == 2) m[rnd() % std::min<size_t>(m.size(), 4096)] = (uint8_t)rnd();  // a byte near the front, where the metadata often lies
                else if (kind == 3 && m.size() - at >= 4) {                            // a 32-bit field set to an edge value
                    static const uint32_t edges[8] = {0, 1, 7, 8, 0x7fffffffu, 0x80000000u, 0xfffffff0u, 0xffffffffu};
                    const uint32_t v = edges[rnd() % 8];
                    m[at] = (uint8_t)(v >> 24), m[at + 1] = (uint8_t)(v >> 16), m[at + 2] = (uint8_t)(v >> 8), m[at + 3] = (uint8_t)v;
                } else if (kind == 4) {
                    m.resize(at + 1);                                                  // cut
                    break;
                } else if (m.size() - at >= 8) {                                       // a box name exchanged for another the parser knows
                    static const char *names[12] = {"moov", "mdat", "moof", "traf", "trun", "tfhd", "stsz", "stco", "stsc", "elst", "mvex", "trak"};
                    const char *n = names[rnd() % 12];
                    for (int k = 0; k < 4; ++k) m[at + 4 + k] = (uint8_t)n[k];
                }
            }
            indexed += index(m);
            static const size_t pieces[4] = {0, 1, 13, 1000};
            const size_t piece = pieces[rnd() % 4];
            demuxed += demux(m, piece ? piece : m.size()).ok;
            runs += 1;
        }
    }
    std::printf("fuzz_mp4 ok: %zu mutated files, %zu indexed, %zu demuxed to the end\n", runs, indexed, demuxed);
    return 0;
}

// fuzz_avi.cpp -- csrc/avi_stream.h alone under AddressSanitizer + UBSan on the CPU: seeded mutations of AVI files through the
// incremental demuxer, whole and in pieces.  Host code only.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o fuzz_avi fuzz_avi.cpp
//   usage: fuzz_avi ITERATIONS_PER_FILE file.avi ...
//
// Checked beyond the sanitizers: a refusal carries a text and stays; a packet never comes without the config; every packet is
// non-empty and no larger than the file; the queue's byte count is the packets'; a file gives the same config, packets and refusal
// however it is cut into pieces; between calls the demuxer holds no more than the file.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../soundkit_amd/csrc/avi_stream.h"

#define check(cond) ((cond) ? (void)0 : (std::fprintf(stderr, "fuzz_avi: check failed at line %d\n", __LINE__), std::abort()))

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}

struct Result {
    bool ok = false, configured = false;
    size_t packets = 0;
    uint64_t bytes = 0, hash = 1469598103934665603ull;
    std::string error;
};

static Result demux(const std::vector<uint8_t> &file, size_t piece) {
    sk_avi::Demuxer d;
    Result r;
    auto mix = [&](uint64_t v) { r.hash = (r.hash ^ v) * 1099511628211ull; };
    auto drain = [&] {
        size_t queued = 0;
        for (const sk_avi::Packet &p : d.packets) queued += p.data.size();
        check(queued == d.queued);
        while (!d.packets.empty()) {
            const sk_avi::Packet p = d.take_packet();
            check(d.configured && !p.data.empty() && p.data.size() <= file.size());
            r.packets += 1, r.bytes += p.data.size();
            for (uint8_t b : p.data) mix(b);
            mix(p.data.size());
        }
        check(d.queued == 0);
    };
    bool ok = true;
    for (size_t at = 0; ok && at < file.size(); at += piece) {
        ok = d.add(file.data() + at, std::min(piece, file.size() - at));
        drain();
        check(d.buffered() <= file.size());
    }
    if (ok) ok = d.finish();
    drain();
    check(ok == !d.failed);
    check(ok || !d.error.empty());
    check(!ok || d.configured);
    check(ok || !d.add(file.data(), 1));  // after a refusal: refused
    if (d.configured) {
        const sk_avi::Config &c = d.config;
        check(c.channels >= 1 && c.sample_rate != 0);
        mix(c.stream_index), mix(c.format_tag), mix(c.channels), mix(c.sample_rate), mix(c.bits);
    }
    r.ok = ok, r.error = d.error, r.configured = d.configured;
    return r;
}

int main(int argc, char **argv) {
    if (argc < 3) return std::fprintf(stderr, "usage: fuzz_avi ITERATIONS_PER_FILE file.avi ...\n"), 2;
    const long iterations = std::atol(argv[1]);
    size_t runs = 0, demuxed = 0, with_packets = 0;
    for (int a = 2; a < argc; ++a) {
        std::ifstream in(argv[a], std::ios::binary);
        const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        check(!file.empty());
        const Result whole = demux(file, file.size());
        check(whole.ok && whole.packets > 0);
        for (long it = -1; it < iterations; ++it) {
            std::vector<uint8_t> m = file;
            const uint32_t kind = rnd() % 7;
            const uint32_t edits = it < 0 ? 0 : 1 + rnd() % 4;  // the first round: the file as it is
            for (uint32_t e = 0; e < edits; ++e) {
                const size_t at = rnd() % m.size();
                if (kind == 0) m[at] = (uint8_t)rnd();                                 // a byte anywhere
                else if (kind == 1) m[at] ^= (uint8_t)(1u << (rnd() % 8));             // a bit anywhere
                else if (kind == 2) m[rnd() % std::min<size_t>(m.size(), 400)] = (uint8_t)rnd();  // a byte near the front, where hdrl lies
                else if (kind == 3) {                                                  // a size or id byte set to an edge value
                    static const uint8_t edges[12] = {0x00, 0x01, 0x03, 0x04, 0x07, 0x08, 0x7f, 0x80, 0xff, 'L', 'w', '0'};
                    m[at] = edges[rnd() % 12];
                } else if (kind == 4) {
                    m.resize(at + 1);                                                  // cut
                    break;
                } else if (kind == 5) {                                                // bytes lost or slipped in: every size behind is off
                    if (rnd() % 2) m.erase(m.begin() + (ptrdiff_t)at, m.begin() + (ptrdiff_t)std::min(m.size(), at + 1 + rnd() % 300));
                    else m.insert(m.begin() + (ptrdiff_t)at, 1 + rnd() % 300, (uint8_t)rnd());
                    if (m.empty()) m.push_back('R');
                } else if (m.size() - at >= 8) {                                       // a chunk header exchanged: a LIST, an audio chunk, sizes at the edges
                    static const char *const ids[6] = {"LIST", "00wb", "01wb", "RIFF", "JUNK", "movi"};
                    static const uint32_t sizes[8] = {0, 1, 3, 4, 5, 0x7fffffff, 0xffffffff, 0xfffffff8};
                    const char *id = ids[rnd() % 6];
                    const uint32_t v = rnd() % 3 ? sizes[rnd() % 8] : rnd() % 5000;
                    for (int i = 0; i < 4; ++i) m[at + i] = (uint8_t)id[i], m[at + 4 + i] = (uint8_t)(v >> (8 * i));
                }
            }
            const Result base = demux(m, m.size());
            static const size_t pieces[5] = {1, 7, 188, 1000, 4096};
            const Result cut = demux(m, pieces[rnd() % 5]);
            check(cut.ok == base.ok && cut.packets == base.packets && cut.bytes == base.bytes && cut.hash == base.hash && cut.configured == base.configured &&
                  cut.error == base.error);
            demuxed += base.ok, with_packets += base.packets > 0;
            runs += 1;
        }
    }
    std::printf("fuzz_avi ok: %zu streams, %zu demuxed to the end, %zu gave packets\n", runs, demuxed, with_packets);
    return 0;
}

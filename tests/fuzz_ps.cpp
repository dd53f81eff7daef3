// fuzz_ps.cpp -- csrc/ps_stream.h alone under AddressSanitizer + UBSan on the CPU: seeded mutations of MPEG program streams through the
// incremental demuxer in its three track modes, whole and in pieces.  Host code only.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o fuzz_ps fuzz_ps.cpp
//   usage: fuzz_ps ITERATIONS_PER_FILE file.mpg ...
//
// Checked beyond the sanitizers: a refusal carries a text and stays; a packet never comes without the config; every packet is
// non-empty, and a DVD LPCM packet a whole number of blocks; the queue's byte count is the packets'; a stream gives the same config,
// packets and refusal however it is cut into pieces; between calls the demuxer holds at most one PES packet and less than a block.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../soundkit_amd/csrc/ps_stream.h"

#define check(cond) ((cond) ? (void)0 : (std::fprintf(stderr, "fuzz_ps: check failed at line %d\n", __LINE__), std::abort()))

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

static Result demux(const std::vector<uint8_t> &file, size_t piece, uint8_t mode) {
    sk_ps::Demuxer d(mode);
    Result r;
    auto mix = [&](uint64_t v) { r.hash = (r.hash ^ v) * 1099511628211ull; };
    auto drain = [&] {
        size_t queued = 0;
        for (const sk_ps::Packet &p : d.packets) queued += p.data.size();
        check(queued == d.queued);
        while (!d.packets.empty()) {
            const sk_ps::Packet p = d.take_packet();
            check(d.configured && !p.data.empty() && p.data.size() <= file.size());
            check(d.config.kind != sk_ps::kKindLpcm || p.data.size() % d.config.block_bytes == 0);
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
        check(!ok || d.buffered() < 6 + 65536 + 96 + piece);
        check(!d.configured || d.config.kind != sk_ps::kKindLpcm || d.carry.size() < d.config.block_bytes);
    }
    if (ok) ok = d.finish();
    drain();
    check(ok == !d.failed);
    check(ok || !d.error.empty());
    check(!ok || (d.configured && d.carry.empty()));
    check(ok || !d.add(file.data(), 1));  // after a refusal: refused
    if (d.configured) {
        const sk_ps::Config &c = d.config;
        check(c.kind == sk_ps::kKindLpcm || c.kind == sk_ps::kKindMpegAudio);
        check(mode != sk_ps::kTrackLpcm || c.kind == sk_ps::kKindLpcm);
        check(mode != sk_ps::kTrackMpegAudio || c.kind == sk_ps::kKindMpegAudio);
        if (c.kind == sk_ps::kKindLpcm)
            check(c.stream_id == 0xBD && c.substream_id >= 0xA0 && c.substream_id <= 0xAF && (c.bits == 16 || c.bits == 24) && c.channels >= 1 && c.channels <= 8 &&
                  c.block_bytes == sk_ps::lpcm_block_bytes(c.bits, c.channels) && c.sample_rate >= 32000);
        else
            check(c.stream_id >= 0xC0 && c.stream_id <= 0xDF);
        mix(c.kind), mix(c.stream_id), mix(c.substream_id), mix(c.channels), mix(c.bits), mix(c.sample_rate), mix(c.block_bytes);
    }
    r.ok = ok, r.error = d.error, r.configured = d.configured;
    return r;
}

int main(int argc, char **argv) {
    if (argc < 3) return std::fprintf(stderr, "usage: fuzz_ps ITERATIONS_PER_FILE file.mpg ...\n"), 2;
    const long iterations = std::atol(argv[1]);
    size_t runs = 0, demuxed = 0, with_packets = 0;
    for (int a = 2; a < argc; ++a) {
        std::ifstream in(argv[a], std::ios::binary);
        const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        check(!file.empty());
        const Result whole = demux(file, file.size(), sk_ps::kTrackFirst);
        check(whole.ok && whole.packets > 0);
        for (long it = -1; it < iterations; ++it) {
            std::vector<uint8_t> m = file;
            const uint32_t kind = rnd() % 7;
            const uint32_t edits = it < 0 ? 0 : 1 + rnd() % 4;  // the first round: the stream as it is
            for (uint32_t e = 0; e < edits; ++e) {
                const size_t at = rnd() % m.size();
                if (kind == 0) m[at] = (uint8_t)rnd();                                 // a byte anywhere
                else if (kind == 1) m[at] ^= (uint8_t)(1u << (rnd() % 8));             // a bit anywhere
                else if (kind == 2) m[rnd() % std::min<size_t>(m.size(), 200)] = (uint8_t)rnd();  // a byte near the front: the first headers
                else if (kind == 3) {                                                  // a length, id or flag byte set to an edge value
                    static const uint8_t edges[14] = {0x00, 0x01, 0x0f, 0x20, 0x30, 0x40, 0x80, 0xa0, 0xba, 0xbd, 0xc0, 0xe0, 0xff, 0x07};
                    m[at] = edges[rnd() % 14];
                } else if (kind == 4) {
                    m.resize(at + 1);                                                  // cut
                    break;
                } else if (kind == 5) {                                                // bytes lost or slipped in: every length behind is off
                    if (rnd() % 2) m.erase(m.begin() + (ptrdiff_t)at, m.begin() + (ptrdiff_t)std::min(m.size(), at + 1 + rnd() % 300));
                    else m.insert(m.begin() + (ptrdiff_t)at, 1 + rnd() % 300, (uint8_t)rnd());
                    if (m.empty()) m.push_back(0);
                } else if (m.size() - at >= 9) {                                       // a packet head exchanged: ids, lengths, header forms
                    static const uint8_t ids[8] = {0xBD, 0xC0, 0xDF, 0xE0, 0xBA, 0xBB, 0xB9, 0xBE};
                    static const uint8_t firsts[6] = {0x81, 0x21, 0x31, 0x0f, 0x60, 0xff};
                    const uint32_t len = rnd() % 3 ? rnd() % 3000 : (rnd() % 2 ? 0 : 0xffff);
                    m[at] = 0, m[at + 1] = 0, m[at + 2] = 1, m[at + 3] = ids[rnd() % 8], m[at + 4] = (uint8_t)(len >> 8), m[at + 5] = (uint8_t)len;
                    m[at + 6] = firsts[rnd() % 6], m[at + 8] = (uint8_t)(rnd() % 12);
                }
            }
            const uint8_t mode = (uint8_t)(rnd() % 3);
            const Result base = demux(m, m.size(), mode);
            static const size_t pieces[5] = {1, 7, 188, 1000, 4096};
            const Result cut = demux(m, pieces[rnd() % 5], mode);
            check(cut.ok == base.ok && cut.packets == base.packets && cut.bytes == base.bytes && cut.hash == base.hash && cut.configured == base.configured &&
                  cut.error == base.error);
            demuxed += base.ok, with_packets += base.packets > 0;
            runs += 1;
        }
    }
    std::printf("fuzz_ps ok: %zu streams, %zu demuxed to the end, %zu gave packets\n", runs, demuxed, with_packets);
    return 0;
}

// fuzz_ts.cpp -- csrc/ts_stream.h alone under AddressSanitizer + UBSan on the CPU: seeded mutations of transport streams through the
// incremental demuxer, whole and in pieces.  Host code only.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o fuzz_ts fuzz_ts.cpp
//   usage: fuzz_ts ITERATIONS_PER_FILE file.ts ...
//
// Checked beyond the sanitizers: a refusal carries a text and stays; a packet never comes without the config; every packet is
// non-empty and no larger than a PES may be; the queue's byte count is the packets'; a stream gives the same config, packets, times and
// refusal however it is cut into pieces; between calls the demuxer holds less than five packets of input and at most one PES.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../soundkit_amd/csrc/ts_stream.h"

#define check(cond) ((cond) ? (void)0 : (std::fprintf(stderr, "fuzz_ts: check failed at line %d\n", __LINE__), std::abort()))

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
    sk_ts::Demuxer d;
    Result r;
    auto mix = [&](uint64_t v) { r.hash = (r.hash ^ v) * 1099511628211ull; };
    auto drain = [&] {
        size_t queued = 0;
        for (const sk_ts::Packet &p : d.packets) queued += p.data.size();
        check(queued == d.queued_bytes());
        while (!d.packets.empty()) {
            const sk_ts::Packet p = d.take_packet();
            check(d.configured && !p.data.empty() && p.data.size() <= sk_ts::kMaxPesBytes && p.data.size() <= file.size());
            check(p.codec != sk_ts::kCodecNone && p.continuity < 16);
            check(p.has_pts || !p.has_dts);
            r.packets += 1, r.bytes += p.data.size();
            for (uint8_t b : p.data) mix(b);
            mix(p.has_pts ? p.pts : ~0ull), mix(p.has_dts ? p.dts : ~0ull), mix(p.has_duration ? p.duration : ~0ull), mix(p.continuity), mix(p.discontinuity);
        }
        check(d.queued_bytes() == 0);
    };
    bool ok = true;
    for (size_t at = 0; ok && at < file.size(); at += piece) {
        ok = d.add(file.data() + at, std::min(piece, file.size() - at));
        drain();
        check(!ok || d.buffered() < 204 * 5 + sk_ts::kMaxPesBytes + 188);
    }
    if (ok) ok = d.finish();
    drain();
    check(ok == !d.failed);
    check(ok || !d.error.empty());
    check(!ok || d.current_pes.empty());
    check(ok || !d.add(file.data(), 1));  // after a refusal: refused
    if (d.configured) {
        const sk_ts::Config &c = d.config;
        check(c.codec != sk_ts::kCodecNone && c.pid < 8192 && (c.stride == 188 || c.stride == 192 || c.stride == 204) && c.prefix == (c.stride == 192 ? 4 : 0));
        check(!c.lpcm || (c.codec == sk_ts::kCodecPcm && c.channels == 2 && (c.bits == 16 || c.bits == 24) && c.bytes_per_frame == c.bits / 4 && c.sample_rate >= 48000));
        mix(c.codec), mix(c.format), mix(c.stream_type), mix(c.pid), mix(c.program), mix(c.stride), mix(c.has_rate ? c.sample_rate : 0), mix(c.has_channels ? c.channels : 99);
        mix(c.bits), mix(c.frames_per_packet);
    }
    r.ok = ok, r.error = d.error, r.configured = d.configured;
    return r;
}

int main(int argc, char **argv) {
    if (argc < 3) return std::fprintf(stderr, "usage: fuzz_ts ITERATIONS_PER_FILE file.ts ...\n"), 2;
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
            const uint32_t edits = it < 0 ? 0 : 1 + rnd() % 4;  // the first round: the stream as it is
            for (uint32_t e = 0; e < edits; ++e) {
                const size_t at = rnd() % m.size();
                if (kind == 0) m[at] = (uint8_t)rnd();                                 // a byte anywhere
                else if (kind == 1) m[at] ^= (uint8_t)(1u << (rnd() % 8));             // a bit anywhere
                else if (kind == 2) m[rnd() % std::min<size_t>(m.size(), 600)] = (uint8_t)rnd();  // a byte near the front, where PAT and PMT lie
                else if (kind == 3) {                                                  // a length, pointer or flag byte set to an edge value
                    static const uint8_t edges[12] = {0x00, 0x01, 0x7f, 0x80, 0xb7, 0xb8, 0xff, 0x47, 0x30, 0x20, 0xc0, 0x0f};
                    m[at] = edges[rnd() % 12];
                } else if (kind == 4) {
                    m.resize(at + 1);                                                  // cut
                    break;
                } else if (kind == 5) {                                                // bytes lost or slipped in: the sync is lost
                    if (rnd() % 2) m.erase(m.begin() + (ptrdiff_t)at, m.begin() + (ptrdiff_t)std::min(m.size(), at + 1 + rnd() % 300));
                    else m.insert(m.begin() + (ptrdiff_t)at, 1 + rnd() % 300, (uint8_t)rnd());
                    if (m.empty()) m.push_back(0x47);
                } else if (m.size() - at >= 4) {                                       // a packet header exchanged: PAT, PMT or audio PID, flags
                    static const uint32_t heads[8] = {0x47400010, 0x47410030, 0x47500011, 0x4701003f, 0x47c10010, 0x47010090, 0x47110020, 0x475fff10};
                    const uint32_t v = heads[rnd() % 8];
                    m[at] = (uint8_t)(v >> 24), m[at + 1] = (uint8_t)(v >> 16), m[at + 2] = (uint8_t)(v >> 8), m[at + 3] = (uint8_t)v;
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
    std::printf("fuzz_ts ok: %zu streams, %zu demuxed to the end, %zu gave packets\n", runs, demuxed, with_packets);
    return 0;
}

// fuzz_webm.cpp -- csrc/webm_stream.h alone under AddressSanitizer + UBSan on the CPU: seeded mutations of WebM files through the
// streaming demuxer, whole and in pieces, and of their CodecPrivate through the Vorbis header split.  Host code only.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o fuzz_webm fuzz_webm.cpp
//   usage: fuzz_webm ITERATIONS_PER_FILE file.webm ...
//
// Checked beyond the sanitizers: a refusal carries a text and stays; every packet is non-empty and no larger than the input plus its
// track's prefix; the queue's byte count is the packets'; a file gives the same packets, times and refusal however it is cut into
// pieces; the demuxer never holds more than its buffer bound; the discard-padding conversion never exceeds the decoded frames.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../soundkit_amd/csrc/webm_stream.h"

#define check(cond) ((cond) ? (void)0 : (std::fprintf(stderr, "fuzz_webm: check failed at line %d\n", __LINE__), std::abort()))

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}

struct Result {
    bool ok = false;
    size_t packets = 0, tracks = 0;
    uint64_t bytes = 0, hash = 1469598103934665603ull;
    std::string error;
};

static Result demux(const std::vector<uint8_t> &file, size_t piece) {
    sk_webm::Demuxer d;
    Result r;
    auto mix = [&](uint64_t v) { r.hash = (r.hash ^ v) * 1099511628211ull; };
    auto drain = [&] {
        size_t queued = 0;
        for (const sk_webm::Packet &p : d.packets) queued += p.data.size();
        check(queued == d.queued_bytes());
        while (!d.packets.empty()) {
            const sk_webm::Packet p = d.take_packet();
            check(d.configured && !p.data.empty());
            size_t prefix = 0;
            bool known = false;
            for (const sk_webm::Track &t : d.audio)
                if (t.number == p.track) prefix = t.prefix.size(), known = true;
            check(known && p.data.size() <= file.size() + prefix);
            check(p.has_discard || p.discard_ns == 0);
            r.packets += 1, r.bytes += p.data.size();
            for (uint8_t b : p.data) mix(b);
            mix((uint64_t)p.timestamp_ns), mix(p.has_duration ? p.duration_ns : ~0ull), mix(p.has_discard ? (uint64_t)p.discard_ns : 1ull << 63);
            if (p.has_discard) {
                uint32_t front = 0, back = 0;
                std::string text;
                if (sk_webm::discard_frames(p.discard_ns, 48000, 960, &front, &back, &text)) check(front <= 960 && back <= 960 && (front == 0 || back == 0));
                else check(!text.empty());
            }
        }
        check(d.queued_bytes() == 0);
    };
    bool ok = true;
    for (size_t at = 0; ok && at < file.size(); at += piece) {
        ok = d.add(file.data() + at, std::min(piece, file.size() - at));
        drain();
        check(d.buffered() <= sk_webm::kMaxBufferBytes);
    }
    if (ok) ok = d.finish();
    drain();
    check(ok == !d.failed);
    check(ok || !d.error.empty());
    check(!ok || (d.configured && !d.audio.empty() && d.buffered() == 0));
    check(ok || !d.add(file.data(), 1));  // after a refusal: refused
    for (const sk_webm::Track &t : d.audio) {
        check(t.kind == sk_webm::kAudio && t.codec != sk_webm::kCodecNone && t.timestamp_scale > 0);
        size_t offsets[3], sizes[3];
        std::string text;
        if (sk_webm::vorbis_headers(t.codec_private.data(), t.codec_private.size(), offsets, sizes, &text)) {
            for (int k = 0; k < 3; ++k) check(offsets[k] <= t.codec_private.size() && sizes[k] <= t.codec_private.size() - offsets[k]);
        } else {
            check(!text.empty());
        }
    }
    r.ok = ok, r.error = d.error, r.tracks = d.configured ? d.audio.size() : 0;
    return r;
}

int main(int argc, char **argv) {
    if (argc < 3) return std::fprintf(stderr, "usage: fuzz_webm ITERATIONS_PER_FILE file.webm ...\n"), 2;
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
            const uint32_t kind = rnd() % 6;
            const uint32_t edits = it < 0 ? 0 : 1 + rnd() % 4;  // the first round: the file as it is
            for (uint32_t e = 0; e < edits; ++e) {
                const size_t at = rnd() % m.size();
                if (kind == 0) m[at] = (uint8_t)rnd();                                 // a byte anywhere
                else if (kind == 1) m[at] ^= (uint8_t)(1u << (rnd() % 8));             // a bit anywhere
                else if (kind == 2) m[rnd() % std::min<size_t>(m.size(), 400)] = (uint8_t)rnd();  // a byte near the front, where the metadata lies
                else if (kind == 3) {                                                  // a size or lacing byte set to an edge value
                    static const uint8_t edges[10] = {0x00, 0x01, 0x7f, 0x80, 0x81, 0xfe, 0xff, 0x40, 0x08, 0x10};
                    m[at] = edges[rnd() % 10];
                    if (rnd() % 2 && m.size() - at >= 8)
                        for (int k = 1; k < 8; ++k) m[at + k] = 0xff;
                } else if (kind == 4) {
                    m.resize(at + 1);                                                  // cut
                    break;
                } else if (m.size() - at >= 4) {                                       // an element id exchanged for another the parser knows
                    static const uint32_t ids[12] = {0x1F43B675, 0x1654AE6B, 0x18538067, 0xA3A3A3A3, 0xA0A1A3E7, 0x75A29BFB,
                                                     0x6D806240, 0x50345033, 0x42544255, 0xAEE1B59F, 0x23E38356, 0x23314F86};
                    const uint32_t v = ids[rnd() % 12];
                    m[at] = (uint8_t)(v >> 24), m[at + 1] = (uint8_t)(v >> 16), m[at + 2] = (uint8_t)(v >> 8), m[at + 3] = (uint8_t)v;
                }
            }
            const Result base = demux(m, m.size());
            static const size_t pieces[4] = {1, 7, 13, 1000};
            const Result cut = demux(m, pieces[rnd() % 4]);
            check(cut.ok == base.ok && cut.packets == base.packets && cut.bytes == base.bytes && cut.hash == base.hash && cut.tracks == base.tracks &&
                  cut.error == base.error);
            demuxed += base.ok, with_packets += base.packets > 0;
            runs += 1;
        }
    }
    std::printf("fuzz_webm ok: %zu files, %zu demuxed to the end, %zu gave packets\n", runs, demuxed, with_packets);
    return 0;
}

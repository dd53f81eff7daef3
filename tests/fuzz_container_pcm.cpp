// fuzz_container_pcm.cpp -- the PCM and FLAC sample entries of csrc/mp4_stream.h under AddressSanitizer + UBSan on the CPU: seeded
// mutations of a file's `moov` (the sample entry, `enda` / `wave` / `dfLa`, the sample tables the runs of frames are made from) through
// the whole-file index and through the streaming demuxer in ragged pieces, of `dfLa` payloads through the normaliser, and of a CAF file's
// header chunks through csrc/caf_stream.h.  Host code only.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o fuzz_container_pcm fuzz_container_pcm.cpp
//   usage: fuzz_container_pcm ITERATIONS_PER_FILE file ...      (MOV / MP4 files with `moov` in front of `mdat`, and CAF files)
//
// Checked beyond the sanitizers: a refusal carries a text; every run the index lists lies inside the file and, for a PCM track, holds at
// most 4096 ticks and 1 MiB unless it is a single sample of the table; the demuxer hands out the index's runs, whole and in pieces, for
// every mutated file both accept; a normalised FLAC configuration begins with `fLaC`; and, before any file is read, coalesce_pcm_runs on
// hand-made tables: a gap in time splits a run as a gap in bytes does.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../soundkit_amd/csrc/caf_stream.h"
#include "../soundkit_amd/csrc/mp4_stream.h"

#define check(cond) ((cond) ? (void)0 : (std::fprintf(stderr, "fuzz_container_pcm: check failed at line %d\n", __LINE__), std::abort()))

static uint64_t g_state = 0x2545f4914f6cdd1dull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}

struct Run {
    uint64_t start;
    uint32_t size, duration;
    uint64_t hash;
};

static uint64_t fnv(const uint8_t *d, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ d[i]) * 1099511628211ull;
    return h;
}

static bool demux(const std::vector<uint8_t> &file, const size_t *pieces, size_t n_pieces, std::vector<Run> *runs) {
    sk_mp4::Demuxer d;
    runs->clear();
    auto drain = [&] {
        while (!d.packets.empty()) {
            const sk_mp4::Packet &p = d.packets.front();
            check(p.data.size() <= file.size());
            runs->push_back(Run{p.start, (uint32_t)p.data.size(), p.duration, fnv(p.data.data(), p.data.size())});
            d.packets.pop_front();
        }
    };
    bool ok = true;
    size_t k = 0;
    for (size_t at = 0; ok && at < file.size(); ++k) {
        const size_t piece = std::min(pieces[k % n_pieces], file.size() - at);
        ok = d.add(file.data() + at, piece);
        drain();
        at += piece;
    }
    if (ok) ok = d.finish();
    drain();
    check(ok == !d.failed);
    check(ok || !d.error.empty());
    return ok;
}

static bool index(const std::vector<uint8_t> &file, sk_mp4::Track *t) {
    std::string error;
    if (!sk_mp4::index_from_file(file.data(), file.size(), t, &error)) {
        check(!error.empty());
        return false;
    }
    check(t->codec >= sk_mp4::kCodecAac && t->codec <= sk_mp4::kCodecPcm);
    check(t->timescale != 0 && t->sample_rate != 0 && t->channels != 0 && t->channels <= 255 && t->bits <= 255);
    if (t->codec == sk_mp4::kCodecFlac) check(t->codec_private.size() >= 4 && std::memcmp(t->codec_private.data(), "fLaC", 4) == 0);
    for (size_t i = 0; i < t->samples.size(); ++i) {
        const sk_mp4::Sample &s = t->samples[i];
        check(s.offset <= file.size() && s.size <= file.size() - s.offset);
        uint32_t first = 0, count = 0;
        if (sk_mp4::trim(*t, s, s.duration, t->sample_rate, &first, &count, &error)) check(count == 0 || (first <= s.duration && count <= s.duration - first));
    }
    return true;
}

// a CAF file: mutations of everything in front of the data chunk's payload, then the index with its own invariants
static void fuzz_caf(const std::vector<uint8_t> &file, long iterations, size_t *runs, size_t *indexed) {
    auto index = [&](const std::vector<uint8_t> &m) {
        sk_caf::Index ix;
        std::string error;
        if (!sk_caf::index_from_file(m.data(), m.size(), &ix, &error)) {
            check(!error.empty());
            return false;
        }
        check(ix.codec == sk_caf::kCodecAlac || ix.codec == sk_caf::kCodecPcm);
        check(ix.sample_rate != 0 && ix.channels >= 1 && ix.channels <= 255 && ix.frames_per_packet != 0);
        uint64_t frames = 0;
        for (const sk_caf::Packet &p : ix.packets) {
            check(p.size != 0 && p.offset <= m.size() && p.size <= m.size() - p.offset && p.start == frames);
            if (ix.codec == sk_caf::kCodecPcm) {
                check(p.size == (uint64_t)p.frames * ix.bytes_per_frame && ix.bytes_per_frame == (ix.bits + 7) / 8 * ix.channels);
                check(p.frames <= sk_caf::kMaxRunFrames || p.frames == ix.frames_per_packet);
            }
            frames += p.frames;
        }
        check(ix.valid_frames + ix.priming_frames + ix.remainder_frames <= frames || ix.packets.empty());
        return true;
    };
    check(index(file));
    size_t head = 8;  // up to the data chunk's payload
    while (head + 12 <= file.size() && std::memcmp(&file[head], "data", 4) != 0) head += 12 + (size_t)sk_caf::be64(&file[head + 4]);
    head = std::min(head + 16, file.size());
    for (long it = 0; it < iterations; ++it) {
        std::vector<uint8_t> m = file;
        const uint32_t kind = rnd() % 4, edits = 1 + rnd() % 3;
        for (uint32_t e = 0; e < edits; ++e) {
            const size_t at = rnd() % head;
            if (kind == 0) m[at] = (uint8_t)rnd();
            else if (kind == 1) m[at] ^= (uint8_t)(1u << (rnd() % 8));
            else if (kind == 2 && head - at >= 4) {
                static const uint32_t edges[9] = {0, 1, 3, 4095, 4097, 0x100001u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
                const uint32_t v = edges[rnd() % 9];
                m[at] = (uint8_t)(v >> 24), m[at + 1] = (uint8_t)(v >> 16), m[at + 2] = (uint8_t)(v >> 8), m[at + 3] = (uint8_t)v;
            } else {
                m.resize(std::max<size_t>(at, 1));
                break;
            }
        }
        *indexed += index(m);
        *runs += 1;
    }
}

// coalesce_pcm_runs on hand-made tables: build_samples makes every start the sum of the durations before it, so a gap in time cannot be
// written into a file; the comparison is held here, beside its mirror for bytes
static void check_coalesce() {
    auto sample = [](uint64_t offset, uint32_t size, uint64_t start, uint32_t duration) {
        sk_mp4::Sample s;
        s.offset = offset, s.size = size, s.start = start, s.duration = duration;
        return s;
    };
    auto same = [](const sk_mp4::Sample &a, const sk_mp4::Sample &b) { return a.offset == b.offset && a.size == b.size && a.start == b.start && a.duration == b.duration; };
    std::vector<sk_mp4::Sample> v = {sample(100, 4, 0, 1), sample(104, 4, 1, 1), sample(108, 4, 2, 1)};  // contiguous both ways: one run
    sk_mp4::coalesce_pcm_runs(&v);
    check(v.size() == 1 && same(v[0], sample(100, 12, 0, 3)));
    v = {sample(100, 4, 0, 1), sample(104, 4, 2, 1), sample(108, 4, 3, 1)};  // contiguous in bytes, a gap in time: the run splits there
    sk_mp4::coalesce_pcm_runs(&v);
    check(v.size() == 2 && same(v[0], sample(100, 4, 0, 1)) && same(v[1], sample(104, 8, 2, 2)));
    v = {sample(100, 4, 0, 2), sample(104, 4, 1, 1)};  // the second begins before the first has ended: no merge either
    sk_mp4::coalesce_pcm_runs(&v);
    check(v.size() == 2);
    v = {sample(100, 4, 0, 1), sample(105, 4, 1, 1), sample(109, 4, 2, 1)};  // contiguous in time, a gap in bytes
    sk_mp4::coalesce_pcm_runs(&v);
    check(v.size() == 2 && same(v[0], sample(100, 4, 0, 1)) && same(v[1], sample(105, 8, 1, 2)));
    v = {sample(104, 4, 0, 1), sample(100, 4, 1, 1)};  // the second lies in front of the first
    sk_mp4::coalesce_pcm_runs(&v);
    check(v.size() == 2);
    v = {sample(0, 4 * 4000, 0, 4000), sample(4 * 4000, 4 * 96, 4000, 96), sample(4 * 4096, 4, 4096, 1)};  // the cap of 4096 ticks is reached exactly
    sk_mp4::coalesce_pcm_runs(&v);
    check(v.size() == 2 && v[0].duration == 4096 && v[1].duration == 1);
    v = {sample(0, 1048575, 0, 1), sample(1048575, 1, 1, 1), sample(1048576, 1, 2, 1)};  // and the cap of 1 MiB
    sk_mp4::coalesce_pcm_runs(&v);
    check(v.size() == 2 && v[0].size == 1048576 && v[1].size == 1);
    v.clear();
    sk_mp4::coalesce_pcm_runs(&v);
    check(v.empty());
}

int main(int argc, char **argv) {
    check_coalesce();
    if (argc < 3) return std::fprintf(stderr, "usage: fuzz_container_pcm ITERATIONS_PER_FILE file.mov ...\n"), 2;
    const long iterations = std::atol(argv[1]);
    size_t runs = 0, indexed = 0, demuxed = 0, agreed = 0, configs = 0, caf_runs = 0, caf_indexed = 0;
    static const size_t ragged[3][4] = {{1, 1, 1, 1}, {7, 4099, 3, 613}, {1000, 13, 65536, 1}};
    for (int a = 2; a < argc; ++a) {
        std::ifstream in(argv[a], std::ios::binary);
        const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        check(file.size() > 64);
        if (std::memcmp(file.data(), "caff", 4) == 0) {
            fuzz_caf(file, iterations, &caf_runs, &caf_indexed);
            continue;
        }
        // where `moov` lies: the mutations stay inside it
        size_t moov_at = 0, moov_len = 0;
        for (size_t pos = 0; file.size() - pos >= 8;) {
            sk_mp4::BoxHeader h;
            check(sk_mp4::read_box(file.data() + pos, file.size() - pos, &h) && h.size <= file.size() - pos);
            if (h.is("moov")) moov_at = pos, moov_len = (size_t)h.size;
            pos += (size_t)h.size;
        }
        check(moov_len > 16);
        // the file as it is: indexed, and the demuxer hands out the index's runs however the bytes arrive
        sk_mp4::Track whole;
        check(index(file, &whole) && !whole.samples.empty());
        for (int r = 0; r < 3; ++r) {
            std::vector<Run> got;
            check(demux(file, ragged[r], 4, &got) && got.size() == whole.samples.size());
            for (size_t i = 0; i < got.size(); ++i) {
                const sk_mp4::Sample &s = whole.samples[i];
                check(got[i].start == s.start && got[i].size == s.size && got[i].duration == s.duration && got[i].hash == fnv(file.data() + s.offset, s.size));
            }
        }
        for (long it = 0; it < iterations; ++it) {
            std::vector<uint8_t> m = file;
            const uint32_t kind = rnd() % 5, edits = 1 + rnd() % 3;
            for (uint32_t e = 0; e < edits; ++e) {
                const size_t at = moov_at + 8 + rnd() % (moov_len - 8);
                if (kind == 0) m[at] = (uint8_t)rnd();
                else if (kind == 1) m[at] ^= (uint8_t)(1u << (rnd() % 8));
                else if (kind == 2 && moov_at + moov_len - at >= 4) {  // a 32-bit field set to an edge value
                    static const uint32_t edges[10] = {0, 1, 2, 4095, 4096, 4097, 0x100000u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
                    const uint32_t v = edges[rnd() % 10];
                    m[at] = (uint8_t)(v >> 24), m[at + 1] = (uint8_t)(v >> 16), m[at + 2] = (uint8_t)(v >> 8), m[at + 3] = (uint8_t)v;
                } else if (kind == 3 && moov_at + moov_len - at >= 8) {  // a name exchanged for another the sample entry's reader knows
                    static const char *names[14] = {"sowt", "twos", "in24", "in32", "fl32", "fl64", "lpcm", "fLaC", "dfLa", "enda", "wave", "stsz", "stts", "stsc"};
                    const char *n = names[rnd() % 14];
                    for (int k = 0; k < 4; ++k) m[at + 4 + k] = (uint8_t)n[k];
                } else {  // the sound description's version field, wherever the entry lies: the 16 bits behind a known entry name + 8
                    for (size_t p = moov_at; p + 20 < moov_at + moov_len; ++p)
                        if (std::memcmp(&m[p], "stsd", 4) == 0) m[p + 4 + 8 + 8 + 8 + 1] = (uint8_t)(rnd() % 4);
                }
            }
            sk_mp4::Track t;
            const bool ix = index(m, &t);
            std::vector<Run> got;
            const bool dm = demux(m, ragged[rnd() % 3], 4, &got);
            if (ix && dm && !t.fragmented) {  // both took it: the same runs
                check(got.size() <= t.samples.size());
                size_t g = 0;
                for (const sk_mp4::Sample &s : t.samples) {  // (a run outside every mdat is indexed but never arrives)
                    if (g < got.size() && got[g].start == s.start && got[g].size == s.size && got[g].duration == s.duration &&
                        got[g].hash == fnv(m.data() + s.offset, s.size))
                        g += 1;
                }
                check(g == got.size());
                agreed += 1;
            }
            indexed += ix, demuxed += dm, runs += 1;
        }
        // dfLa payloads: slices of the moov, as they are and with their first bytes set to a block header
        for (long it = 0; it < iterations; ++it) {
            const size_t at = moov_at + rnd() % moov_len, n = std::min<size_t>(rnd() % 80, moov_at + moov_len - at);
            std::vector<uint8_t> d(file.begin() + (ptrdiff_t)at, file.begin() + (ptrdiff_t)(at + n)), out;
            if (n >= 8 && (rnd() & 1)) d[4] = (uint8_t)(rnd() & 0x81), d[5] = 0, d[6] = (uint8_t)(rnd() & 1), d[7] = (uint8_t)(33 + rnd() % 3);
            std::string error;
            if (sk_mp4::normalize_flac_config(d.data(), d.size(), &out, &error)) {
                check(out.size() >= 4 && std::memcmp(out.data(), "fLaC", 4) == 0);
                configs += 1;
            } else {
                check(!error.empty());
            }
        }
    }
    std::printf("fuzz_container_pcm ok: %zu mutated files, %zu indexed, %zu demuxed to the end, %zu with the same runs both ways, %zu configurations; "
                "%zu mutated CAF headers, %zu indexed\n", runs, indexed, demuxed, agreed, configs, caf_runs, caf_indexed);
    return 0;
}

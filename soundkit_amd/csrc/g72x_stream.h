// g72x_stream.h -- the host side of the headerless telephony streams (G.711, G.722, G.726): there is nothing to parse, so this is the
// arithmetic of a send -- how many bytes decode now, how many samples they give -- with the reference's limits and texts:
//   * G726Decoder::decode_i16's group framing (soundkit-g726/src/lib.rs:819-859): whole groups decode, a partial group waits for the
//     next send, and at the end of the stream `flush` reports what is left (lib.rs:801-810);
//   * the spawns' parameter checks (soundkit-decoder/src/lib.rs:2531-2540);
//   * the pipeline's scratch of 262 144 samples a send (lib.rs:82): a send that decodes to more ends its stream with the codec's
//     `Output buffer too small for ... decode` text, and nothing of it is decoded.
// Header-only; used by engine.cpp and pipeline.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/soundkit_amd.h"

namespace sk_g72x {

enum : int { kUlaw = 0, kAlaw = 1, kG722 = 2, kG726 = 3, kCodecs = 4 };  // enum sk_g72x_codec
constexpr size_t kScratchSamples = 262144;

// bits per code of a G.726 rate, 0 for a rate that is none
inline int g726_bits(uint32_t rate) { return rate == 16000 ? 2 : (rate == 24000 ? 3 : (rate == 32000 ? 4 : (rate == 40000 ? 5 : 0))); }
// a group is the fewest whole bytes that hold whole codes: 1 / 3 / 1 / 5 bytes giving 4 / 8 / 2 / 8 samples
inline uint32_t g726_group_bytes(int bits) { return bits == 3 ? 3 : (bits == 5 ? 5 : 1); }
inline uint32_t g726_group_samples(int bits) { return bits == 2 ? 4 : (bits == 4 ? 2 : 8); }

// bytes that must come in whole multiples, and the samples each such group gives (G.711 per channel sample, G.722 two per byte)
inline uint32_t group_bytes(int codec, int bits) { return codec == kG726 ? g726_group_bytes(bits) : 1; }
inline uint32_t group_samples(int codec, int bits) { return codec == kG726 ? g726_group_samples(bits) : (codec == kG722 ? 2 : 1); }
inline const char *codec_name(int codec) { return codec == kG726 ? "G.726" : (codec == kG722 ? "G.722" : "G.711"); }

// samples that `bytes` whole-group bytes decode to
inline uint64_t samples_of(int codec, int bits, uint64_t bytes) { return bytes / group_bytes(codec, bits) * group_samples(codec, bits); }

// the scratch limit of one send; false with the reference's text
inline bool fits_scratch(int codec, uint64_t samples, std::string *text) {
    if (samples <= kScratchSamples) return true;
    if (text) *text = std::string("Output buffer too small for ") + codec_name(codec) + " decode: need " + std::to_string(samples) + ", have " + std::to_string(kScratchSamples);
    return false;
}

// spawn_g711's checks; false with the reference's text
inline bool check_g711(uint32_t sample_rate, uint32_t channels, std::string *text) {
    const char *what = sample_rate == 0 ? "G.711 sample rate must be > 0" : (channels == 0 ? "G.711 channel count must be > 0" : nullptr);
    if (what && text) *text = what;
    return what == nullptr;
}

// what a fresh stream starts from: G726Core::default() (soundkit-g726/src/lib.rs:196-212); G.722 from all zeros, both scale factors included
inline void init_state(sk_g726_state *s) {
    *s = sk_g726_state{};
    s->yl = 34816, s->yu = 544;
    for (int k = 0; k < 6; ++k) s->dq[k] = 32;
    s->sr[0] = s->sr[1] = 32;
}
inline void init_state(sk_g722_state *s) { *s = sk_g722_state{}; }

// The G.726 group framer: bytes in, whole groups out, the rest held back for the next add.
struct G726Framer {
    uint32_t group = 1;            // bytes per group
    std::vector<uint8_t> pending;  // fewer than `group` bytes

    explicit G726Framer(int bits = 4) : group(g726_group_bytes(bits)) {}
    // how many bytes (pending + input) the next add will hand on
    size_t ready(size_t len) const { return (pending.size() + len) / group * group; }
    // appends the whole groups of pending + input to `out`, keeps the rest
    size_t add(const uint8_t *input, size_t len, std::vector<uint8_t> &out) {
        const size_t whole = ready(len), held = pending.size();
        if (whole == 0) {
            pending.insert(pending.end(), input, input + len);
            return 0;
        }
        out.insert(out.end(), pending.begin(), pending.end());
        out.insert(out.end(), input, input + (whole - held));
        pending.assign(input + (whole - held), input + len);
        return whole;
    }
    // the end of the stream: true when nothing is held back, else the reference's text
    bool flush(std::string *text) const {
        if (pending.empty()) return true;
        if (text) *text = "G.726 stream ended with " + std::to_string(pending.size()) + " trailing partial-packet byte(s)";
        return false;
    }
};

}  // namespace sk_g72x

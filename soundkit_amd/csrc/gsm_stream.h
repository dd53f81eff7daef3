// gsm_stream.h -- the host side of the GSM 06.10 full-rate streams: there is no header to parse, so this is the arithmetic of a send --
// how many bytes decode now, how many samples they give, whether libgsm would take the frames -- with the reference's limits and texts:
//   * GsmDecoder::decode_i16's packet framing (soundkit-gsm/src/lib.rs:340-392): whole packets decode (33 bytes -> 160 samples, or the
//     Microsoft framing's 65 bytes -> 320), a partial packet waits for the next send, and at the end of the stream `flush` reports
//     what is left (lib.rs:321-330);
//   * the room check that comes before anything else (lib.rs:346-358) against the pipeline's scratch of 262 144 samples a send
//     (soundkit-decoder/src/lib.rs:82);
//   * gsm_decode's one refusal: a standard frame whose first nibble is not 0xD (`GSM decoder rejected frame`, lib.rs:61-63).  A
//     Microsoft packet carries no magic: the reference writes 0xD0 itself (unpack_ms_pair), so it is never rejected.
// Header-only; used by engine.cpp and pipeline.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/soundkit_amd.h"

namespace sk_gsm {

constexpr size_t kScratchSamples = SK_G72X_MAX_SEND_SAMPLES;
constexpr uint32_t kFrameBytes = 33, kMsPacketBytes = 65, kFrameSamples = 160, kFrameBits = 260;

inline bool variant_ok(int variant) { return variant == SK_GSM_STANDARD || variant == SK_GSM_MICROSOFT; }
inline uint32_t packet_bytes(int variant) { return variant == SK_GSM_MICROSOFT ? kMsPacketBytes : kFrameBytes; }
inline uint32_t packet_samples(int variant) { return variant == SK_GSM_MICROSOFT ? 2 * kFrameSamples : kFrameSamples; }
// samples that `bytes` whole-packet bytes decode to
inline uint64_t samples_of(int variant, uint64_t bytes) { return bytes / packet_bytes(variant) * packet_samples(variant); }
// Where the frames' 260 parameter bits lie, MSB first: behind the magic nibble of every 33 bytes, or as two runs in 65 bytes -- which
// is one run of 260 bits after the other through the whole Microsoft stream.  Nothing is repacked: the kernels read them there.
inline uint32_t base_bit(int variant) { return variant == SK_GSM_MICROSOFT ? 0 : 4; }
inline uint32_t stride_bits(int variant) { return variant == SK_GSM_MICROSOFT ? kFrameBits : 8 * kFrameBytes; }

// the room of one call; false with the reference's text
inline bool fits(uint64_t samples, uint64_t have, std::string *text) {
    if (samples <= have) return true;
    if (text) *text = "Output buffer too small for GSM decode: need " + std::to_string(samples) + ", have " + std::to_string(have);
    return false;
}
inline bool fits_scratch(uint64_t samples, std::string *text) { return fits(samples, kScratchSamples, text); }

// gsm_decode's check of every standard frame of `len` whole-packet bytes; false with the reference's text
inline bool frames_accepted(int variant, const uint8_t *bytes, size_t len, std::string *text) {
    if (variant != SK_GSM_STANDARD) return true;
    for (size_t at = 0; at + kFrameBytes <= len; at += kFrameBytes) {
        if ((bytes[at] >> 4) == 0xD) continue;
        if (text) *text = "GSM decoder rejected frame";
        return false;
    }
    return true;
}

// what a fresh stream starts from (gsm_create): all zeros but nrp
inline void init_state(sk_gsm_state *s) {
    *s = sk_gsm_state{};
    s->nrp = 40;
}

// The packet framer: bytes in, whole packets out, the rest held back for the next add.
struct Framer {
    uint32_t packet = kFrameBytes;
    std::vector<uint8_t> pending;  // fewer than `packet` bytes

    explicit Framer(int variant = SK_GSM_STANDARD) : packet(packet_bytes(variant)) {}
    // how many bytes (pending + input) the next add will hand on
    size_t ready(size_t len) const { return (pending.size() + len) / packet * packet; }
    // appends the whole packets of pending + input to `out`, keeps the rest
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
        if (text) *text = "GSM stream ended with " + std::to_string(pending.size()) + " trailing partial-frame byte(s)";
        return false;
    }
};

}  // namespace sk_gsm

// mp12_internal.h -- the host side of MPEG Layer I / II (mp12_bitstream.cpp) as the rest of the library reaches it.  The C entry
// points (sk_mpa_*) are thin wrappers in engine.cpp; mp12_bitstream.cpp itself needs nothing but the public header, so that a
// harness can compile it alone (tests/fuzz_mp12.cpp).
#pragma once
#include "../../include/soundkit_amd.h"

#include <cstddef>
#include <cstdint>

namespace sk_mp12 {

int parse_header(const uint8_t *d, size_t len, sk_mpa_frame_info *out);
int scan(const uint8_t *d, size_t len, uint32_t *layer, sk_mpa_frame_info *frames, uint32_t cap, uint32_t *n_frames, size_t *consumed);
// The layer of a stream that has none yet: 1 ... 3 = that of its first CONFIRMED frame (two consistent headers one frame length apart);
// 0 = no header in sight; -1 = a Layer I / II candidate waits for the header behind it, -3 = a Layer III candidate does
int find_layer(const uint8_t *d, size_t len);
int parse_frame(const uint8_t *frame, size_t len, const sk_mpa_frame_info *h, sk_mpa_frame_record *out);
// bits of one sample triple (Layer II) or sample (Layer I) of a class, 0 for "nothing sent"; -1: no such class
int class_bits(int layer, uint8_t cls);
// what the stage call checks before a record may reach the kernel: classes, bounds, and that the last sample code ends inside byte_len
bool record_adds_up(const sk_mpa_frame_record &r);

}  // namespace sk_mp12

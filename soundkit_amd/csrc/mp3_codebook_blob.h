// mp3_codebook_blob.h -- the flattened code book of the device Huffman stage (mp3_entropy.hip), plain C++: written by
// sk_mp3_codebook_flatten (mp3_decoder.cpp, host only), uploaded by sk_mp3_set_codebook, read by k_mp3_entropy.
//
// One blob of 32-bit words: this header, then the first-level tables (kMp3L1Bits bits each, one per DISTINCT code table: the
// standard's tables 16-23 share one code set, 24-31 another), then the tables of the longer codes.  A table entry:
//   0                                               the bits are no code
//   bit 31 clear: 0x8000 | len << 16 | x << 4 | y   a code of `len` bits of this level (count1: the quadruple v w x y in bits 3-0)
//   bit 31 set:   width << 26 | word offset         all bits of this level are consumed; go on in the table at that offset of the
//                                                   blob, indexed by the next `width` (1..kMp3L1Bits) bits
// A code shorter than its level's width fills every entry it is a prefix of.  Walking the levels is walking the host's trie
// kMp3L1Bits bits at a time: the same codes, the same "no code".
#pragma once
#include <stdint.h>

namespace sk {

constexpr uint32_t kMp3L1Bits = 8;
constexpr uint32_t kMp3BlobRates = 9;
// a granule has at most 39 partitions (13 short bands x 3 windows): a count of 39 or more ends at the last line whatever the cut.
// (Parsed side information asks for 24 at most; a hand-made record may ask for any count, and gets the host's answer.)
constexpr uint32_t kMp3RegionCounts = 40;
struct Mp3CodebookHeader {
    uint32_t words;      // the whole blob
    uint32_t lds_words;  // header + first-level tables: what a block keeps in LDS while the kernel runs
    uint32_t big[32];    // xlen | linbits << 8 | word offset of the first-level table << 16 (xlen 0: a table without codes)
    uint32_t count1[2];  // word offset of the first-level table
    uint8_t slen[16][2];
    uint8_t lsf_partitions[6][3][4];
    uint8_t rates_present[12];  // [9] used
    // the line at which the first `count` scale-factor band partitions of a granule end (<= 576), per sampling rate and cut
    // (long | short | mixed): what huffman() of mp3_decoder.cpp derives from the band offsets per call
    uint16_t region[kMp3BlobRates][3][kMp3RegionCounts];
    uint32_t reserved[3];  // to a multiple of 16 bytes
};
static_assert(sizeof(Mp3CodebookHeader) % 16 == 0, "the first-level tables behind it are copied as uint4");

}  // namespace sk

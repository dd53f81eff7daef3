// vorbis_blob.h -- the layout of a Vorbis stream's device blob (32-bit words), shared by the host that builds it (vorbis_stream.h) and
// the kernels that walk it (vorbis_decode.hip).  Every index in it was checked by the host; offsets are words from the blob's start.
#pragma once
#include <stdint.h>

namespace sk_vb {

constexpr uint32_t kMaxChannels = 8;
constexpr uint32_t kMaxPosts = 65;       // floor 1: 2 + 31 partitions x ... the specification's limit on the X list
constexpr uint32_t kLutBits = 8;         // first-level Huffman lookup; longer codes go on through the tree, 32 steps at the most
constexpr uint32_t kLeaf = 0x80000000u;  // LUT entry / tree child: leaf.  LUT leaf: entry | (length - 1) << 24; tree leaf: entry
// A stream's blob may not exceed this.  The two fixtures need 50 KB (19 books, 8 500 VQ values) and 350 KB (42 books, 61 014 VQ values,
// 11 693 entries); libvorbis' largest stock setups stay below 2 MiB expanded.  4 MiB leaves room and still bounds what a hostile setup
// header (entries up to 2^24, dimensions up to 2^16) can make the host build and upload.
constexpr uint32_t kMaxBlobBytes = 4u << 20;

enum : uint32_t { H_WORDS, H_CHANNELS, H_BS0, H_BS1, H_NMODES, H_MODEBITS, H_MODES, H_MAPPINGS, H_FLOORS, H_RESIDUES, H_BOOKS, H_NBOOKS, H_SIZE = 16 };
enum : uint32_t { MODE_FLAG, MODE_MAPPING, MODE_SIZE };
enum : uint32_t { M_SUBMAPS, M_NCOUPLING, M_COUPLING /* offset of the steps: magnitude | angle << 8 */, M_MUX, M_FLOOR = M_MUX + 8, M_RESIDUE = M_FLOOR + 16,
                  M_SIZE = M_RESIDUE + 16 };
enum : uint32_t { F_VALUES, F_MULT, F_PARTS, F_PCLASS, F_CDIM = F_PCLASS + 31, F_CSUB = F_CDIM + 16, F_CMASTER = F_CSUB + 16, F_SUBBOOKS = F_CMASTER + 16,
                  F_X = F_SUBBOOKS + 128, F_LOW = F_X + 65, F_HIGH = F_LOW + 65, F_SORTED = F_HIGH + 65, F_SIZE = F_SORTED + 65 };
enum : uint32_t { R_TYPE, R_BEGIN, R_END, R_PSIZE, R_NCLASS, R_CLASSBOOK, R_BOOKS /* [64][8], 0xffffffff: none */, R_SIZE = R_BOOKS + 512 };
enum : uint32_t { B_DIMS, B_ENTRIES, B_LUTBITS, B_LUT, B_TREE, B_VQ /* 0: a scalar book */, B_SINGLE /* entry + 1 of a one-entry book, else 0 */, B_SIZE = 8 };

}  // namespace sk_vb

// ima_adpcm.h -- the IMA / DVI ADPCM step table and per-nibble arithmetic, shared by the two stages that decode it: AIFF-C's IMA4
// packets (aiff_decode.hip) and WAV's tag 0x11 blocks (wav_adpcm.hip).  The containers differ, the recurrence does not.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sk {
namespace {

__device__ const int16_t kImaStep[89] = {
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
    157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552,
    1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487,
    12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};

__device__ __forceinline__ int ima_delta(int step, uint32_t n) {
    int d = step >> 3;
    if (n & 1) d += step >> 2;
    if (n & 2) d += step >> 1;
    if (n & 4) d += step;
    return (n & 8) ? -d : d;
}
__device__ __forceinline__ int ima_next_index(int idx, uint32_t n) {
    idx += (n & 4) ? (int)(((n & 3) + 1) * 2) : -1;
    return idx < 0 ? 0 : (idx > 88 ? 88 : idx);
}
__device__ __forceinline__ int clamp_s16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

}  // namespace
}  // namespace sk

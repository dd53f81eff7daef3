// mp12_tables.h -- the normative constants of MPEG Layer I and II (ISO/IEC 11172-3 2.4.2.3, Tables B.2a-d; 13818-3 2.4.2.3,
// Table B.1): bit rates, and Layer II's bit-allocation tables as rows of quantiser step counts.  Data only.
#pragma once
#include <cstdint>

namespace sk_mp12 {

// kbit/s by bit-rate index; 0 = free format, 15 = forbidden
constexpr uint16_t kBitrateV1L1[16] = {0, 32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384, 416, 448, 0};
constexpr uint16_t kBitrateV1L2[16] = {0, 32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384, 0};
constexpr uint16_t kBitrateV2L1[16] = {0, 32, 48, 56, 64, 80, 96, 112, 128, 144, 160, 176, 192, 224, 256, 0};
constexpr uint16_t kBitrateV2L2[16] = {0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 0};  // = Layer III's LSF row

// One row of a Layer II allocation table: the allocation field's width and the step count of allocation 1, 2, ... (0: nothing sent)
struct AllocRow {
    uint8_t bits;
    uint16_t steps[15];
};
constexpr AllocRow kRows[8] = {
    /* A */ {4, {3, 7, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 16383, 32767, 65535}},
    /* B */ {4, {3, 5, 7, 9, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 65535}},
    /* C */ {3, {3, 5, 7, 9, 15, 31, 65535}},
    /* D */ {2, {3, 5, 65535}},
    /* E */ {4, {3, 5, 9, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 16383, 32767}},
    /* F */ {3, {3, 5, 9, 15, 31, 63, 127}},
    /* G */ {4, {3, 5, 7, 9, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 16383}},
    /* H */ {2, {3, 5, 9}},
};
enum Row : uint8_t { A, B, C, D, E, F, G, H };

// A table: the subband limit and the row of every subband below it
struct AllocTable {
    uint8_t sblimit;
    uint8_t row[32];
};
constexpr AllocTable kTables[5] = {
    /* B.2a */ {27, {A, A, A, B, B, B, B, B, B, B, B, C, C, C, C, C, C, C, C, C, C, C, C, D, D, D, D}},
    /* B.2b */ {30, {A, A, A, B, B, B, B, B, B, B, B, C, C, C, C, C, C, C, C, C, C, C, C, D, D, D, D, D, D, D}},
    /* B.2c */ {8, {E, E, F, F, F, F, F, F}},
    /* B.2d */ {12, {E, E, F, F, F, F, F, F, F, F, F, F}},
    /* 13818-3 B.1 */ {30, {G, G, G, G, F, F, F, F, F, F, F, H, H, H, H, H, H, H, H, H, H, H, H, H, H, H, H, H, H, H}},
};

// 11172-3 2.4.2.3: the table of an MPEG-1 Layer II frame follows from the bit rate per channel and the sampling rate
inline int layer2_table(bool lsf, uint32_t bitrate_kbps, int channels, uint32_t sample_rate) {
    if (lsf) return 4;
    const uint32_t per_channel = channels == 1 ? bitrate_kbps : bitrate_kbps / 2;
    if (per_channel < 56) return sample_rate == 32000 ? 3 : 2;
    if (per_channel >= 96 && sample_rate != 48000) return 1;
    return 0;
}

}  // namespace sk_mp12

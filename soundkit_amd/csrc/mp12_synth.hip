// mp12_synth.hip -- MPEG Layer I and II on the device for gfx950, batched over streams: sample unpacking straight from the frame's
// bytes, requantisation, and the 32-band polyphase synthesis (ISO/IEC 11172-3 2.4.3.2-3, 13818-3 2.4.3.1).
//
// In the reference this is nanomp3::Decoder::decode on a Layer I / II frame (soundkit-mp3/src/lib.rs:284; the crate's source is
// not in the tree), followed by f32_to_i16 (lib.rs:376-385).  The host has read the frame's serial front into a record
// (mp12_bitstream.cpp: quantisation class and scale factors per channel and subband, where the samples start, how wide a granule
// is) and has checked that the last code ends inside the frame.  tests/mp12_model.py is the f64 checker.
//
// One wavefront owns one (stream, channel) and walks that stream's frames of the batch in order; the polyphase FIFO V (a ring of
// 16 x 64, and its position) is the one the stream's Layer III synthesis would use and crosses HBM once per launch.  Per frame:
//   lane = 2 subband + channel, the order of the bitstream: its class's width (0 where nothing is sent, and for the second
//   channel above the joint-stereo bound, whose code is the first's) -> exclusive wave prefix sum = the bit position inside a granule;
//   lane = subband + 32 * half: takes the position of its (subband, channel) by a lane read, then unpacks granules 6 half ... 6 half + 5:
//   each code is two dword loads of the uploaded bytes and a shift; Layer II's grouped code words (3, 5, 9 steps) are split by
//   multiply-shift; sample = scalefactor * (2 code - (steps - 1)) / steps -> S[slot][subband] in LDS (36 x 32, Layer I 12 x 32);
//   36 (12) time slots as in mp3_hybrid.hip: V_i = sum_k N[i][k] S_k with lane i holding row i of N in 32 VGPRs, into the ring;
//   every lane sums its 8 window taps and lanes j, j + 32 add up to output j.  Output: interleaved f32, s16 through f32_to_i16, or the
//   scheduler tick's planar rows (planar_stride): a Layer II frame is two units of 576 PCM frames, a Layer I frame one of 384.
#include "sk_device.h"

namespace sk {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) float lds_f;
typedef __attribute__((address_space(3))) f4 lds_f4;

constexpr int kWaves = 4;

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// soundkit-mp3/src/lib.rs:376-385: (x * 32767).round(), saturating
__device__ __forceinline__ int16_t mp12_to_i16(float x) {
    const float scaled = roundf(x * 32767.0f);
    if (scaled != scaled) return 0;  // NaN: Rust's saturating `as` gives 0
    if (scaled > 32767.0f) return 32767;
    if (scaled < -32768.0f) return -32768;
    return (int16_t)scaled;
}

// bits of one triple (Layer II) or sample (Layer I) of a class; the host has rejected every class this does not know
__device__ __forceinline__ uint32_t class_width(uint32_t layer, uint32_t cls) {
    if (cls == 0) return 0;
    if (layer == 1) return cls;
    if (cls & 0x80u) return cls == 0x83u ? 5u : (cls == 0x85u ? 7u : 10u);
    return 3u * cls;
}

// n (1 ... 16) bits at bit position p of the big-endian stream `w`
__device__ __forceinline__ uint32_t fetch(const uint32_t *w, uint32_t p, uint32_t n) {
    const uint32_t i = p >> 5;
    const uint64_t v = ((uint64_t)__builtin_bswap32(w[i]) << 32) | __builtin_bswap32(w[i + 1]);
    return (uint32_t)(v >> (64u - (p & 31u) - n)) & ((1u << n) - 1u);
}

template <bool OUT16>
__global__ __launch_bounds__(kWaves * 64) void k_mp12_synth(Mp12Args a) {
    __shared__ __attribute__((aligned(16))) float smp[kWaves][36 * 32];
    __shared__ __attribute__((aligned(16))) float ring[kWaves][1024];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t task_id = blockIdx.x * kWaves + wave;
    if (task_id >= a.n_tasks) return;
    const SynthTask task = a.tasks[task_id];
    const uint32_t count = __builtin_amdgcn_readfirstlane(task.count), state = __builtin_amdgcn_readfirstlane(task.state);
    const Mp12Entry *entries = a.entries + __builtin_amdgcn_readfirstlane(task.begin);
    const int ch = state & 1;
    lds_f *S = (lds_f *)smp[wave], *rg = (lds_f *)ring[wave];

    // carried state in: the polyphase ring and its position (the Layer III overlap in front of them is not this path's)
    float *st = a.state + (size_t)state * kMp3StateFloats;
    for (int i = lane; i < 1024; i += 64) rg[i] = st[576 + i];
    uint32_t pos = __builtin_amdgcn_readfirstlane(__float_as_uint(st[1600])) & 15u;
    float nrow[32], dwin[8];
#pragma unroll
    for (int k = 0; k < 32; ++k) nrow[k] = a.matrix[lane * 32 + k];
#pragma unroll
    for (int i = 0; i < 8; ++i) dwin[i] = a.window[64 * i + lane];
    const int sb = lane & 31, half = lane >> 5;
    wave_sync();

    for (uint32_t f = 0; f < count; ++f) {
        const Mp12Entry ent = entries[f];
        const sk_mpa_frame_record *rec = a.records + __builtin_amdgcn_readfirstlane(ent.record);
        const uint32_t pcm_off = __builtin_amdgcn_readfirstlane(ent.pcm_off);
        const uint32_t layer = __builtin_amdgcn_readfirstlane((uint32_t)rec->layer);
        const uint32_t channels = __builtin_amdgcn_readfirstlane((uint32_t)rec->channels);
        const uint32_t sblimit = __builtin_amdgcn_readfirstlane((uint32_t)rec->sblimit);
        const uint32_t bound = __builtin_amdgcn_readfirstlane((uint32_t)rec->bound);
        const uint32_t granule_bits = __builtin_amdgcn_readfirstlane((uint32_t)rec->granule_bits);
        const uint32_t first_bit = __builtin_amdgcn_readfirstlane(rec->byte_offset * 8u + rec->sample_bit);

        // ---- where this lane's codes stand inside a granule ----
        const uint32_t osb = (uint32_t)lane >> 1, och = (uint32_t)lane & 1u;  // bitstream order
        const bool sent = osb < sblimit && och < channels && (och == 0 || osb < bound);
        const uint32_t w = sent ? class_width(layer, rec->cls[och][osb]) : 0u;
        uint32_t incl = w;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const uint32_t mine = 2u * (uint32_t)sb + ((channels == 2 && (uint32_t)sb < bound) ? (uint32_t)ch : 0u);
        const uint32_t at = __shfl(incl - w, (int)mine);

        const uint32_t cls = (uint32_t)sb < sblimit ? rec->cls[ch][sb] : 0u;
        const bool grouped = (cls & 0x80u) != 0;
        const uint32_t nb = grouped ? 0u : cls;
        const uint32_t steps = grouped ? (cls & 0x7fu) : ((1u << nb) - 1u);
        const float fsteps = (float)steps;
        float sf[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) sf[k] = a.scf[rec->scf[ch][sb][k] & 63u];
        const int bias = (int)steps - 1;

        // ---- unpack and requantise: this lane's six granules (slots) ----
        for (int gi = 0; gi < 6; ++gi) {
            const uint32_t g = 6u * (uint32_t)half + (uint32_t)gi;
            const uint32_t p = first_bit + g * granule_bits + at;
            if (layer == 1) {
                float v = 0.0f;
                if (cls) v = sf[0] * ((float)(2 * (int)fetch(a.bytes, p, nb) - bias) / fsteps);
                S[32 * g + sb] = v;
            } else {
                float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
                if (cls) {
                    uint32_t c0, c1, c2;
                    if (grouped) {
                        const uint32_t c = fetch(a.bytes, p, steps == 3 ? 5u : (steps == 5 ? 7u : 10u));
                        // c = c0 + steps c1 + steps^2 c2, c < 1024: the quotients by multiply-shift (exact on that range)
                        const uint32_t q = steps == 3 ? (c * 43691u) >> 17 : (steps == 5 ? (c * 52429u) >> 18 : (c * 58255u) >> 19);
                        c0 = c - q * steps;
                        c2 = steps == 3 ? (q * 43691u) >> 17 : (steps == 5 ? (q * 52429u) >> 18 : (q * 58255u) >> 19);
                        c1 = q - c2 * steps;
                    } else {
                        c0 = fetch(a.bytes, p, nb);
                        c1 = fetch(a.bytes, p + nb, nb);
                        c2 = fetch(a.bytes, p + 2u * nb, nb);
                    }
                    const float s = sf[g >> 2];
                    v0 = s * ((float)(2 * (int)c0 - bias) / fsteps);
                    v1 = s * ((float)(2 * (int)c1 - bias) / fsteps);
                    v2 = s * ((float)(2 * (int)c2 - bias) / fsteps);
                }
                S[32 * (3 * g) + sb] = v0;
                S[32 * (3 * g + 1) + sb] = v1;
                S[32 * (3 * g + 2) + sb] = v2;
            }
        }
        wave_sync();
        // ---- polyphase synthesis, 36 (Layer I: 12) time slots ----
        const int slots = layer == 1 ? 12 : 36;
        for (int ss = 0; ss < slots; ++ss) {
            pos = (pos + 1u) & 15u;  // the new vector takes the place of the oldest
            float v = 0.0f;
#pragma unroll
            for (int k4 = 0; k4 < 8; ++k4) {
                const f4 s4 = *reinterpret_cast<const lds_f4 *>(S + 32 * ss + 4 * k4);
                v += nrow[4 * k4] * s4.x;
                v += nrow[4 * k4 + 1] * s4.y;
                v += nrow[4 * k4 + 2] * s4.z;
                v += nrow[4 * k4 + 3] * s4.w;
            }
            rg[64 * pos + lane] = v;
            wave_sync();
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) acc += rg[64 * ((pos - 2u * (uint32_t)i - (uint32_t)half) & 15u) + lane] * dwin[i];
            const float sum = acc + __shfl_xor(acc, 32);
            if (half == 0) {
                const size_t out = (size_t)pcm_off + (size_t)(32 * ss + sb) * channels + ch;
                if (!OUT16 && a.planar_stride) {
                    // the tick's form: unit u of the frame (18 slots each; Layer I's one unit has 12) owns `channels` rows from
                    // row pcm_off + u * channels on, each sample as f32_to_i16(x) / 32768 -- what k_mp3_hybrid leaves for a granule
                    const uint32_t u = layer == 1 ? 0u : (uint32_t)ss / 18u, within = layer == 1 ? (uint32_t)ss : (uint32_t)ss % 18u;
                    a.pcm[((size_t)pcm_off + (size_t)u * channels + ch) * a.planar_stride + 32u * within + sb] = (float)mp12_to_i16(sum) * (1.0f / 32768.0f);
                } else if (OUT16) a.pcm16[out] = mp12_to_i16(sum);
                else a.pcm[out] = sum;
            }
            wave_sync();
        }
    }
    for (int i = lane; i < 1024; i += 64) st[576 + i] = rg[i];
    if (lane == 0) st[1600] = __uint_as_float(pos);
}

}  // namespace

hipError_t launch_mp12_synth(const Mp12Args &a, hipStream_t s) {
    if (a.n_tasks == 0) return hipSuccess;
    const uint32_t blocks = (a.n_tasks + kWaves - 1) / kWaves;
    if (a.pcm16) hipLaunchKernelGGL(k_mp12_synth<true>, dim3(blocks), dim3(kWaves * 64), 0, s, a);
    else hipLaunchKernelGGL(k_mp12_synth<false>, dim3(blocks), dim3(kWaves * 64), 0, s, a);
    return hipGetLastError();
}

}  // namespace sk

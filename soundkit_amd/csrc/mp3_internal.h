// mp3_internal.h -- what mp3_decoder.cpp shares with the translation units that drive the device Huffman stage
// (mp3_decoder_gpu.cpp, engine.cpp): the code book and decoder handle as structures, and the table of function pointers
// through which mp3_decoder.cpp reaches the GPU mode.  mp3_decoder.cpp itself references no engine entry point of the device
// stage: the harnesses that compile it alone (tests/fuzz_mp3.cpp, tests/sched_stub.cpp, tools/mp3_host_rate.cpp) link
// without them, the table stays empty there and the GPU mode reports SK_ERR_UNSUPPORTED.
#pragma once
#include "../../include/soundkit_amd.h"
#include "mp3_codebook_blob.h"

#include <cmath>
#include <cstdint>
#include <vector>

struct sk_mp3_codebook {
    struct Trie {
        std::vector<int32_t> next;  // [node][bit]: > 0 child node, <= 0: -(symbol) - 1 ... 0 = empty
        uint8_t xlen = 0, linbits = 0;
        // the next kLutBits bits of the stream -> (length << 16 | symbol + 1) of the code they start with, 0 if that code is longer
        // (or the bits are no code): one look-up for the short codes, which are the frequent ones; the trie walk for the rest
        std::vector<uint32_t> lut;
    };
    static constexpr int kLutBits = 10;
    Trie big[32], count1[2];
    sk_mp3_tables t;  // hlen / hcod pointers inside are not kept (copied into the tries)
};

struct sk_mp3_decoder {
    sk_engine *engine = nullptr;
    const sk_mp3_codebook *cb = nullptr;
    sk_mp3_codebook *own_cb = nullptr;  // the standard's tables, when the caller passed none
    std::vector<uint8_t> buffer, reservoir;
    uint32_t sample_rate = 0;  // of the first frame (Option::get_or_insert, lib.rs:203-204)
    uint8_t channels = 0;
    uint64_t frames = 0;
    uint32_t free_format_bytes = 0;  // a free-format stream's frame length once measured (sk_mp3_scan_free)
    bool gpu_entropy = false;  // sk_mp3_decoder_set_gpu_entropy: parts 2 + 3 on the device (mp3_decoder_gpu.cpp)
    bool stream_open = false;
    uint32_t stream = 0;
    uint8_t stream_channels = 0;
    // scratch of one call
    std::vector<sk_mp3_frame_info> found;
    std::vector<sk_mp3_requant_granule> granules;
    std::vector<sk_mp3_granule_desc> descs;
    std::vector<int16_t> is;
    std::vector<float> pcm;
    std::vector<int32_t> status;
    std::vector<uint8_t> staged_reservoir, main;
    struct Queued {
        uint32_t first_granule, granules;
        size_t first_sample, samples;
        bool rejected = false;  // GPU mode: a stage behind the Huffman stage rejected the frame (host mode reads the granules' statuses)
    };
    std::vector<Queued> queued;
    // GPU mode (mp3_decoder_gpu.cpp): the frames of one engine call, their main data, the verdicts
    std::vector<sk_mp3_frame_item> gpu_frames;
    std::vector<uint8_t> gpu_bytes;
    std::vector<uint32_t> gpu_streams, gpu_blob;  // gpu_blob: the decoder's code book, flattened
    std::vector<int32_t> gpu_entropy_status, gpu_stage_status;
    // Layer I / II (mp12_decoder.cpp).  mpa_layer: 0 = the stream's layer is not known yet, else that of its first confirmed frame
    uint8_t mpa_layer = 0;
    std::vector<sk_mpa_frame_info> mpa_found;
    std::vector<sk_mpa_frame_record> mpa_records;
};

namespace sk_mp3_internal {

constexpr size_t kMaxBuffered = 4u * 1024 * 1024;  // MAX_MP3_STREAM_BUFFER_BYTES, lib.rs:155
constexpr size_t kReservoirKept = 2048;            // main_data_begin reaches back 511 bytes at most

// soundkit-mp3/src/lib.rs:387-396
inline int32_t mp3_f32_to_i32(float sample) {
    const float scaled = std::round(sample * 2147483648.0f);  // i32::MAX as f32
    if (scaled > 2147483648.0f) return INT32_MAX;
    if (scaled < -2147483648.0f) return INT32_MIN;
    if (scaled != scaled) return 0;
    if (scaled >= 2147483648.0f) return INT32_MAX;  // Rust's saturating `as`
    return (int32_t)scaled;
}

enum class Out { I16, I32, F32 };


// Filled in by a static initialiser of mp3_decoder_gpu.cpp when the library is loaded.
struct GpuHooks {
    // the engine's device code book := this blob (sk_mp3_codebook_flatten); cheap when the engine holds it already
    int (*install_codebook)(sk_engine *, const uint32_t *words, size_t n_words) = nullptr;
    int (*decode)(sk_mp3_decoder *, const uint8_t *input, size_t len, void *out, size_t out_cap, size_t *written, Out kind) = nullptr;
    // Layer I / II (mp12_decoder.cpp): finds the layer of a stream that has none yet and decodes the call if the stream is Layer I / II
    // (or has to wait for the header that tells); *handled = false: a Layer III stream, the call is decode()'s as ever
    int (*decode_mpa)(sk_mp3_decoder *, const uint8_t *input, size_t len, void *out, size_t out_cap, size_t *written, Out kind, bool *handled) = nullptr;
};
GpuHooks &gpu_hooks();  // mp3_decoder.cpp

}  // namespace sk_mp3_internal

struct sk_engine;
namespace sk {
int mp3_install_codebook(sk_engine *, const uint32_t *words, size_t n_words);  // engine.cpp
}

// The same for the batch scheduler (pipeline.cpp; filled in by pipeline_mp3_gpu.cpp): with an empty table a pipeline created with
// gpu_entropy = 3 is SK_ERR_UNSUPPORTED.
namespace sk_mp3_internal {
struct PipelineGpuHooks {
    int (*install_codebook)(sk_engine *, const uint32_t *words, size_t n_words) = nullptr;
    // the WAV / raw PCM streams' tick; with these absent a PCM stream that needs a conversion ends with SK_ERR_UNSUPPORTED
    int (*tick_pcm)(sk_engine *, const sk_pcm_tick_stream *, uint32_t, const sk_pcm_unit *, uint32_t, const uint8_t *, size_t, uint8_t *, size_t,
                    sk_tick_output *, uint32_t, uint32_t *, size_t *) = nullptr;  // sk_tick_run_pcm
    size_t (*tick_pcm_out_bound)(sk_engine *, const sk_pcm_tick_stream *, uint32_t, const sk_pcm_unit *, uint32_t, uint32_t *) = nullptr;
    // the AIFF streams' tick; with these absent an AIFF stream that is not delivered as it is ends with SK_ERR_UNSUPPORTED
    int (*tick_aiff)(sk_engine *, sk_aiff_tick_stream *, uint32_t, const sk_pcm_unit *, uint32_t, const uint8_t *, size_t, uint8_t *, size_t,
                     sk_tick_output *, uint32_t, uint32_t *, size_t *) = nullptr;  // sk_tick_run_aiff
    size_t (*tick_aiff_out_bound)(sk_engine *, const sk_aiff_tick_stream *, uint32_t, const sk_pcm_unit *, uint32_t, uint32_t *) = nullptr;
    // sk_tick_run_flac / sk_tick_flac_out_bound_on: the FLAC streams' frames
    int (*tick_flac)(sk_engine *, const sk_flac_tick_stream *, uint32_t, const sk_flac_frame_info *, uint32_t, const uint8_t *, size_t, uint8_t *, size_t,
                     sk_tick_output *, uint32_t, uint32_t *, size_t *, int32_t *) = nullptr;
    size_t (*tick_flac_out_bound)(sk_engine *, const sk_flac_tick_stream *, uint32_t, const sk_flac_frame_info *, uint32_t, uint32_t *) = nullptr;
    // the engine's pool of wide PCM streams (3 ... 8 channels); with these absent such a stream is refused as before
    // Layer I / II streams: the host front (mp12_bitstream.cpp) and the tick that takes their frames; with these absent such a stream
    // ends with SK_ERR_UNSUPPORTED.  tick_mpa is also the tick of gpu_entropy = 3 (frames with main data; its Layer I / II table is null then)
    int (*mpa_find_layer)(const uint8_t *, size_t) = nullptr;  // sk_mp12::find_layer
    int (*mpa_scan)(const uint8_t *, size_t, uint32_t *, sk_mpa_frame_info *, uint32_t, uint32_t *, size_t *) = nullptr;  // sk_mpa_scan
    int (*mpa_parse_frame)(const uint8_t *, size_t, const sk_mpa_frame_info *, sk_mpa_frame_record *) = nullptr;         // sk_mpa_parse_frame
    int (*tick_mpa)(sk_engine *, const sk_tick_stream *, uint32_t, const sk_tick_input *, const sk_tick_mp3_frames *, const sk_tick_mpa_frames *, uint8_t *,
                    size_t, sk_tick_output *, uint32_t, uint32_t *, size_t *) = nullptr;  // sk_tick_run_mixed_mpa
    // sk_tick_run_alac / sk_tick_alac_out_bound_on: the ALAC streams' packets
    int (*tick_alac)(sk_engine *, const sk_alac_tick_stream *, uint32_t, const sk_alac_tick_packet *, uint32_t, const uint8_t *, size_t, uint8_t *, size_t,
                     sk_tick_output *, uint32_t, uint32_t *, size_t *, int32_t *) = nullptr;
    size_t (*tick_alac_out_bound)(sk_engine *, const sk_alac_tick_stream *, uint32_t, const sk_alac_tick_packet *, uint32_t, uint32_t *) = nullptr;
    // sk_tick_run_g72x / sk_tick_g72x_out_bound_on: the telephony streams' units
    int (*tick_g72x)(sk_engine *, const sk_g72x_tick_stream *, uint32_t, const sk_pcm_unit *, uint32_t, const uint8_t *, size_t, uint8_t *, size_t, sk_tick_output *,
                     uint32_t, uint32_t *, size_t *, sk_g726_state *, uint32_t, sk_g722_state *, uint32_t) = nullptr;
    size_t (*tick_g72x_out_bound)(sk_engine *, const sk_g72x_tick_stream *, uint32_t, const sk_pcm_unit *, uint32_t, uint32_t *) = nullptr;
    // sk_tick_run_gsm / sk_tick_gsm_out_bound_on: the GSM streams' units
    int (*tick_gsm)(sk_engine *, const sk_gsm_tick_stream *, uint32_t, const sk_pcm_unit *, uint32_t, const uint8_t *, size_t, uint8_t *, size_t, sk_tick_output *,
                    uint32_t, uint32_t *, size_t *, sk_gsm_state *, uint32_t) = nullptr;
    size_t (*tick_gsm_out_bound)(sk_engine *, const sk_gsm_tick_stream *, uint32_t, const sk_pcm_unit *, uint32_t, uint32_t *) = nullptr;
    // sk_tick_run_vorbis / sk_tick_vorbis_out_bound_on: the Vorbis streams' packets
    int (*tick_vorbis)(sk_engine *, sk_vorbis_tick_stream *, uint32_t, const sk_vorbis_tick_packet *, uint32_t, const uint8_t *, size_t, uint8_t *, size_t,
                       sk_tick_output *, uint32_t, uint32_t *, size_t *, int32_t *) = nullptr;
    size_t (*tick_vorbis_out_bound)(sk_engine *, const sk_vorbis_tick_stream *, uint32_t, const sk_vorbis_tick_packet *, uint32_t, const uint8_t *, size_t,
                                    uint32_t *) = nullptr;
    // sk_tick_run_wav_adpcm / sk_tick_wav_adpcm_out_bound_on: the WAV ADPCM streams' blocks
    int (*tick_wav_adpcm)(sk_engine *, sk_wav_adpcm_tick_stream *, uint32_t, const sk_pcm_unit *, uint32_t, const uint8_t *, size_t, uint8_t *, size_t,
                          sk_tick_output *, uint32_t, uint32_t *, size_t *, int32_t *) = nullptr;
    size_t (*tick_wav_adpcm_out_bound)(sk_engine *, const sk_wav_adpcm_tick_stream *, uint32_t, const sk_pcm_unit *, uint32_t, uint32_t *) = nullptr;
    uint32_t (*wide_pcm_streams)(const sk_engine *) = nullptr;  // sk_engine_wide_pcm_streams
    int (*enable_wide_pcm)(sk_engine *, uint32_t) = nullptr;    // sk_engine_enable_wide_pcm
};
PipelineGpuHooks &pipeline_gpu_hooks();  // pipeline.cpp
}  // namespace sk_mp3_internal

// pipeline_mp3_gpu.cpp -- what lets the batch scheduler run its MP3 streams' Huffman stage in the tick (sk_pipeline_config::gpu_entropy
// = 3) and its PCM-family and Layer I / II streams in theirs: the engine entry points pipeline.cpp must not name itself (mp3_internal.h
// says why), put into its table when the library is loaded.  Everything else of the mode is in pipeline.cpp (parse_some_mp3 stops behind
// the reservoir and stages frames + main data; the submission thread calls tick_mpa, sk_tick_run_mixed_mpa, with them).
#include "mp3_internal.h"
#include "mp12_internal.h"

namespace {

const bool g_hooked = [] {
    sk_mp3_internal::PipelineGpuHooks &hooks = sk_mp3_internal::pipeline_gpu_hooks();
    hooks.install_codebook = sk::mp3_install_codebook;
    hooks.tick_pcm = sk_tick_run_pcm;  // the WAV / raw PCM streams' tick comes the same way
    hooks.tick_pcm_out_bound = sk_tick_pcm_out_bound_on;
    hooks.tick_aiff = sk_tick_run_aiff;  // ... and the AIFF streams'
    hooks.tick_aiff_out_bound = sk_tick_aiff_out_bound_on;
    hooks.tick_wav_adpcm = sk_tick_run_wav_adpcm;  // ... and the WAV ADPCM streams'
    hooks.tick_wav_adpcm_out_bound = sk_tick_wav_adpcm_out_bound_on;
    hooks.tick_flac = sk_tick_run_flac;  // ... and the FLAC streams'
    hooks.tick_flac_out_bound = sk_tick_flac_out_bound_on;
    hooks.tick_alac = sk_tick_run_alac;  // ... and the ALAC streams'
    hooks.tick_alac_out_bound = sk_tick_alac_out_bound_on;
    hooks.tick_g72x = sk_tick_run_g72x;  // ... and the telephony streams'
    hooks.tick_g72x_out_bound = sk_tick_g72x_out_bound_on;
    hooks.tick_gsm = sk_tick_run_gsm;  // ... and the GSM streams'
    hooks.tick_gsm_out_bound = sk_tick_gsm_out_bound_on;
    hooks.tick_vorbis = sk_tick_run_vorbis;  // ... and the Vorbis streams'
    hooks.tick_vorbis_out_bound = sk_tick_vorbis_out_bound_on;
    hooks.mpa_find_layer = sk_mp12::find_layer;  // Layer I / II streams: their host front and their tick
    hooks.mpa_scan = sk_mpa_scan;
    hooks.mpa_parse_frame = sk_mpa_parse_frame;
    hooks.tick_mpa = sk_tick_run_mixed_mpa;
    hooks.wide_pcm_streams = sk_engine_wide_pcm_streams;
    hooks.enable_wide_pcm = sk_engine_enable_wide_pcm;
    return true;
}();

}  // namespace

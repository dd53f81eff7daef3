/*
 * soundkit_amd.h -- C ABI of the MI355X (gfx950) batched decode-DSP engine.
 *
 * This is the drop-in boundary for soundkit's per-frame decode DSP hot path
 * (SURVEY.md section 8).  The reference has no C FFI on this path: the three Rust
 * surfaces it would bind behind are cited per entry point below
 * (paths relative to the upstream soundkit tree).  INTEGRATION.md shows the Rust
 * `extern "C"` block and the `impl Decoder` / access-unit shims a maintainer adds.
 *
 * Conventions (mirrored from the reference):
 *  - the caller owns every buffer it passes; the engine owns per-stream carried
 *    state (overlap delay + previous window shape: dsp.rs:143-152; resampler
 *    history: soundkit-decoder lib.rs:1917-1927) in device memory;
 *  - no allocation per call once buffers have grown to the working size
 *    (soundkit-aac-lc/tests/no_alloc_decode.rs);
 *  - a bad frame fails that frame only (per-frame status word), never the batch
 *    (soundkit-decoder lib.rs:3131-3134 ends only that stream's worker);
 *  - frames of one stream inside one call are applied in array order; calls for
 *    one stream must not race (one worker per stream, lib.rs:2764); calls for
 *    different streams may come from different threads (the engine serialises
 *    submission internally).
 *  - every function returns SK_OK (0) or a negative sk_status; sk_strerror() names it.
 *
 * Pointers named d_* are DEVICE addresses on the engine's GPU; the *_dev entry
 * points enqueue on the engine's HIP stream (sk_engine_hip_stream) and return
 * without synchronising.  All other pointers are host memory and those entry
 * points return with results complete.
 *
 * One engine per GPU is the design.  A process MAY create several engines on one device (the scheduler's lanes are that), and
 * then they take turns with the device.  Why: on this platform a packed-f32 instruction delivers a wrong low half now and then while
 * another wave of its CU executes a 16x16x32 matrix instruction -- the FIR's and the resampler's (profiles/r04_lanes_corruption.md).
 * The default build contains no packed-f32 instructions, is immune (sk_kernels_use_packed_f32() == 0) and takes no turns: its
 * engines' work overlaps freely on the device.  The turns are the protection of a PACKED_F32=1 build inside a process: there, while
 * a second engine exists on the device, a tick holds the device from its first upload to its last wait, and every other compute entry point (sk_aac_plan_run_*, sk_downsample_*, sk_resampler_*,
 * sk_mp3_* synthesis) holds it for the call and WAITS for its own work before returning -- the *_dev entry points are synchronous
 * then.  Across processes nothing protects a PACKED_F32=1 build: it needs its GPU (or disjoint CUs, HSA_CU_MASK) to itself.
 */
#ifndef SOUNDKIT_AMD_H
#define SOUNDKIT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SK_AAC_FRAME_LEN 1024u /* dsp.rs:9 LONG_SPECTRUM_LEN */
#define SK_MAX_CHANNELS 2u     /* AAC-LC SCE / CPE only: decoder.rs:116-133 */
#define SK_MAX_PCM_CHANNELS 8u /* WAV / raw PCM sources on an engine with sk_engine_enable_wide_pcm; the reference sets no limit */

typedef enum sk_status {
    SK_OK = 0,
    SK_ERR_INVALID_ARG = -1,
    SK_ERR_NO_DEVICE = -2,   /* no usable gfx950 device / HIP runtime error at create */
    SK_ERR_HIP = -3,         /* a HIP call failed (sk_engine_last_hip_error) */
    SK_ERR_OOM = -4,
    SK_ERR_BAD_STREAM = -5,  /* stream id not open */
    SK_ERR_UNSUPPORTED = -6, /* e.g. resample ratio other than 48k->16k on the MFMA path */
    SK_ERR_CAPACITY = -7,    /* max_streams exhausted */
    SK_ERR_TIMEOUT = -8,     /* the device did not finish a tick within the engine's wait bound (sk_engine_set_wait_bound) */
    SK_ERR_INTERNAL = -9     /* a C++ exception other than std::bad_alloc (that one: SK_ERR_OOM) was caught at the ABI; sk_last_exception() */
} sk_status;

/* per-frame status words written by the AAC entry points */
typedef enum sk_frame_status {
    SK_FRAME_OK = 0,
    SK_FRAME_BAD_STREAM = 1,   /* stream not open */
    SK_FRAME_BAD_CHANNELS = 2, /* desc.channels != the stream's channel count */
    SK_FRAME_BAD_WINDOW = 3    /* window_sequence > 3 or window_shape > 1 */
} sk_frame_status;

/* ics.rs:7-12 WindowSequence (bitstream coding) / ics.rs:32-35 WindowShape */
enum { SK_ONLY_LONG = 0, SK_LONG_START = 1, SK_EIGHT_SHORT = 2, SK_LONG_STOP = 3 };
enum { SK_SHAPE_SINE = 0, SK_SHAPE_KBD = 1 };

typedef struct sk_engine sk_engine; /* one per GPU */

/* One decoded-but-not-yet-synthesised AAC-LC frame: what decoder.rs:336-374
 * synthesize_channel reads from IcsInfo per channel. */
typedef struct sk_aac_frame_desc {
    uint32_t stream;
    uint8_t channels;           /* 1 or 2; must equal the stream's */
    uint8_t window_sequence[2]; /* per channel */
    uint8_t window_shape[2];    /* per channel */
    uint8_t reserved[3];
} sk_aac_frame_desc;

/* ---- engine / stream lifetime ------------------------------------------- */

int sk_engine_create(int device, uint32_t max_streams, sk_engine **out);
void sk_engine_destroy(sk_engine *);
int sk_engine_device(const sk_engine *);
uint32_t sk_engine_max_streams(const sk_engine *);
/* Reserves max_wide_streams (<= max_streams) slots for PCM streams of 3 ... SK_MAX_PCM_CHANNELS channels (5.1 / 7.1 WAV, headerless
 * multichannel PCM).  Opt-in because a wide stream's resampler rows cost 8 x 96 KiB of device memory, so the caller sizes the pool;
 * an engine that never calls this behaves exactly as before.  Once per engine and before its first sk_resampler_open (which
 * allocates the rows): SK_ERR_INVALID_ARG afterwards, or when max_wide_streams is 0 or > max_streams.  With the pool, sk_stream_open takes
 * 3 ... 8 channels (one slot each, SK_ERR_CAPACITY when none is free; sk_stream_close returns it) and sk_tick_run_pcm takes such
 * sources.  A wide stream serves sk_resampler_open / _close / _process_f32 / _flush_f32, sk_stream_reset and sk_tick_run_pcm only:
 * every synthesis / AAC / MP3 entry point refuses it as it refuses a wrong channel count.  No reference counterpart (the
 * reference's worker allocates per stream). */
int sk_engine_enable_wide_pcm(sk_engine *, uint32_t max_wide_streams);
uint32_t sk_engine_wide_pcm_streams(const sk_engine *); /* the reserved count, 0 if not enabled */
void *sk_engine_hip_stream(sk_engine *); /* hipStream_t */
int sk_engine_synchronize(sk_engine *);
const char *sk_engine_last_hip_error(const sk_engine *);
/* 1 when the kernels were built with the packed-f32 vector instructions (make PACKED_F32=1), 0 in the default build.  On this
 * platform a packed-f32 instruction can deliver a wrong low half while another wave of its CU executes a 16x16x32 matrix
 * instruction (profiles/r04_lanes_corruption.md): a flavour-1 library is 2-3 % faster on the decode tail and must have its GPU to
 * itself -- no second decoding process, no GEMM workload on the same CUs; the default is immune.  No reference counterpart. */
int sk_kernels_use_packed_f32(void);
/* Diagnostics (no reference counterpart).  sk_engine_where: the stage the engine's current tick is in, as static text,
 * readable from any thread without the engine's lock ("idle" outside a tick).  sk_engine_set_wait_bound: how long a
 * tick waits for the device before it gives up with SK_ERR_TIMEOUT (default 120 s) instead of blocking for good.
 * sk_engine_debug_fail_after: the n-th HIP call from now fails as a launch failure (error-path tests; 0 disarms). */
const char *sk_engine_where(const sk_engine *);
int sk_engine_set_wait_bound(sk_engine *, double seconds);
/* Generic-ratio resampling (every pair of soundkit's common rates other than 48 -> 16 kHz) runs on the matrix cores, held to
 * the float tolerance like the 48 -> 16 kHz FIR.  exact = 1 selects the scalar form instead, whose sums keep rubato's order
 * of operations: the restated reference bit for bit, about five times slower. */
int sk_engine_set_resampler_exact(sk_engine *, int exact);
int sk_engine_debug_fail_after(sk_engine *, int n_hip_calls);
const char *sk_strerror(int status);
/* Exception barrier: no C++ exception leaves the library -- every entry point catches what is thrown below it and returns
 * SK_ERR_OOM (std::bad_alloc) or SK_ERR_INTERNAL; worker threads of the scheduler turn an exception into the error of the
 * stream they were serving (soundkit-decoder/src/lib.rs:3131-3134: an error ends that stream only).  Text of the last
 * exception caught on the calling thread ("" if none): */
const char *sk_last_exception(void);
/* Test hook: the (n+1)-th entry into the library from now throws (kind 0 std::bad_alloc, 1 std::length_error, 2 a type that
 * is no std::exception) as if an allocation inside had failed; n < 0 switches it off.  Returns the previous countdown. */
int sk_debug_throw_after(int n, int kind);
/* Test hook for the scheduler's own threads: the (n+1)-th passage of point `where` throws std::bad_alloc -- 0: inside the
 * per-stream guard of an entropy thread (that stream ends with SK_ERR_OOM, the others go on); 1 entropy thread, 2 submission
 * thread, 3 delivery thread outside any per-stream guard (the lane stops: every open stream ends with the error, later
 * spawns return it, the process lives). */
int sk_debug_throw_in_thread(int n, int where);
const char *sk_version(void);

/* AacLcDecoder::new (decoder.rs:56-78): allocates the per-channel DspChannel state
 * (delay zeroed, previous shape = Sine, dsp.rs:162-163). */
int sk_stream_open(sk_engine *, uint32_t sample_rate, uint8_t channels, uint32_t *stream_out);
int sk_stream_close(sk_engine *, uint32_t stream);
int sk_stream_reset(sk_engine *, uint32_t stream);
/* checkpoint / inspection of the carried state: delay [channels][1024] f32, prev_shape [channels] */
int sk_stream_get_state(sk_engine *, uint32_t stream, float *delay_out, uint8_t *prev_shape_out);
int sk_stream_set_state(sk_engine *, uint32_t stream, const float *delay, const uint8_t *prev_shape);

/* ---- AAC-LC synthesis: IMDCT + window + overlap-add ---------------------- */
/* Replaces AacLcDecoder::synthesize_channel (decoder.rs:336-374) =
 * DspChannel::synthesize_long_sequence / synthesize_eight_short (dsp.rs:230-338) over
 * imdct_fast (dsp.rs:476-535), for n frames at once.
 * coeffs: frame i holds desc[i].channels x 1024 f32, planar, frames packed back to back
 *         (the dequantised, stereo- and TNS-processed spectra: decoder.rs:341, 358).
 * pcm_out (f32): same packing, planar f32 = PlanarF32 (decoder.rs:22-36, 385-390).
 * pcm_out (s16): frame i holds 1024 x channels interleaved i16 = decode_aac_access_unit
 *         (soundkit-decoder lib.rs:1793-1813) with float_sample_to_i16 (lib.rs:1815-1827).
 * status_per_frame may be NULL.  Output of a frame whose status != 0 is not written. */
int sk_aac_synthesize_f32(sk_engine *, const sk_aac_frame_desc *descs, const float *coeffs, float *pcm_out,
                          uint32_t n, int32_t *status_per_frame);
int sk_aac_synthesize_s16(sk_engine *, const sk_aac_frame_desc *descs, const float *coeffs, int16_t *pcm_out,
                          uint32_t n, int32_t *status_per_frame);

/* The same, split so that a schedule can be validated/uploaded once and run on
 * device-resident spectra (the throughput path: no PCIe inside the run). */
typedef struct sk_aac_plan sk_aac_plan;
int sk_aac_plan_create(sk_engine *, const sk_aac_frame_desc *descs, uint32_t n, int32_t *status_per_frame,
                       sk_aac_plan **out);
void sk_aac_plan_destroy(sk_aac_plan *);
uint64_t sk_aac_plan_elements(const sk_aac_plan *); /* total f32 elements of coeffs / pcm */
uint32_t sk_aac_plan_frames_ok(const sk_aac_plan *);
int sk_aac_plan_run_f32_dev(sk_engine *, const sk_aac_plan *, const float *d_coeffs, float *d_pcm);
int sk_aac_plan_run_s16_dev(sk_engine *, const sk_aac_plan *, const float *d_coeffs, int16_t *d_pcm);
/* The s16 of decode_aac_access_unit (soundkit-decoder lib.rs:1793-1813: float_sample_to_i16 of every sample) written by
 * the synthesis kernel itself, PLANAR: the packing of the f32 form with two bytes per sample (channel c of frame i at
 * element (off_i + c) * 1024).  This is the intermediate of the worker's decode -> resample path -- the resampler is fed
 * these integers / 32768 (lib.rs:3563-3617) -- kept on the device at half the bytes of the f32 PCM;
 * sk_downsample_48k_16k_frames_s16_to_s16_dev reads it in place.  d_pcm16 is 8-byte aligned. */
int sk_aac_plan_run_s16_planar_dev(sk_engine *, const sk_aac_plan *, const float *d_coeffs, int16_t *d_pcm16);

/* ---- AAC-LC access-unit front-end (host cores) ------------------------------------------------
 * The entropy / side-information half of AacLcDecoder::decode_access_unit (soundkit-aac-lc/src/
 * decoder.rs:104-334): element loop, ICS info, sections, scalefactors, pulse, Huffman spectral decode
 * with dequantisation, PNS, intensity + mid/side stereo, TNS.  It stops where the GPU takes over:
 * sk_aac_decoder_parse fills the dequantised spectra [channels][1024] and the window fields of one
 * sk_aac_frame_desc (the caller sets .stream), ready for sk_aac_synthesize_* / sk_aac_plan_create.
 * Errors mirror AacLcError (error.rs:5-18); sk_aac_decoder_last_error carries the reference's message. */
typedef enum sk_aac_status {
    SK_AAC_ERR_EOF = -101,                        /* UnexpectedEof */
    SK_AAC_ERR_INVALID_AOT = -102,                /* InvalidAudioObjectType */
    SK_AAC_ERR_UNSUPPORTED_AOT = -103,            /* UnsupportedAudioObjectType */
    SK_AAC_ERR_UNSUPPORTED_SF_INDEX = -104,       /* UnsupportedSamplingFrequencyIndex */
    SK_AAC_ERR_UNSUPPORTED_CHANNEL_CONFIG = -105, /* UnsupportedChannelConfig */
    SK_AAC_ERR_UNSUPPORTED_FEATURE = -106,        /* UnsupportedFeature: callers fall back to another decoder */
    SK_AAC_ERR_INVALID_CONFIG = -107,             /* InvalidConfig */
    SK_AAC_ERR_INVALID_BITSTREAM = -108           /* InvalidBitstream */
} sk_aac_status;
typedef struct sk_aac_decoder sk_aac_decoder;
/* AacLcDecoder::from_audio_specific_config (decoder.rs:80, config.rs:139-260) */
int sk_aac_decoder_create(const uint8_t *asc, size_t asc_len, sk_aac_decoder **out);
void sk_aac_decoder_destroy(sk_aac_decoder *);
int sk_aac_decoder_info(const sk_aac_decoder *, uint32_t *sample_rate, uint8_t *channels); /* frame_info, decoder.rs:88 */
const char *sk_aac_decoder_last_error(const sk_aac_decoder *);
/* counters since creation: frames, EightShort channel-frames, LongStart/Stop channel-frames, channel-frames with TNS,
 * PNS bands, intensity bands, mid/side bands, channel-frames with pulse data (aac-wasm-bench lib.rs:1955-1986) */
int sk_aac_decoder_tool_usage(const sk_aac_decoder *, uint32_t out[8]);
int sk_aac_decoder_parse(sk_aac_decoder *, const uint8_t *access_unit, size_t len, float *coeffs /*[ch][1024]*/,
                         sk_aac_frame_desc *desc);
/* parse_adts_access_unit (soundkit-decoder/src/lib.rs:1007-1027): the 2-byte ASC and the raw access unit of
 * one ADTS frame; frame_len = bytes to the next frame header. */
/* The Huffman half of the front-end alone ("GPU dequant + stereo tools + TNS fed by i16 quantized
 * values + scalefactor bytes"): quant receives channels x 1024 i16 quantised values (pulses applied, spectral.rs:327-423,
 * 2198-2247), side a SK_AAC_UNIT_SIDE_BYTES record (section codebooks, transmitted scale factors, grouping, mid/side mask,
 * TNS filters, noise-sample count, and the verdict on the rest of the unit), desc the window fields.  Dequantisation
 * (dsp.rs:397-405), PNS, intensity + mid/side and TNS then run on the device: sk_tick_run_q.  5.6 KiB per stereo
 * access unit cross PCIe instead of 8 KiB.  A quantised magnitude beyond i16 (illegal in ISO/IEC 14496-3, which stops at
 * 8191; the reference accepts escapes up to 2^17, spectral.rs:214-228) travels in the record's list of wide values, up
 * to 48 per access unit; the 49th is SK_AAC_ERR_UNSUPPORTED_FEATURE in this mode only. */
#define SK_AAC_UNIT_SIDE_BYTES 1600u
int sk_aac_decoder_parse_q(sk_aac_decoder *, const uint8_t *access_unit, size_t len, int16_t *quant /*[ch][1024]*/,
                           void *side /*SK_AAC_UNIT_SIDE_BYTES*/, sk_aac_frame_desc *desc);
int sk_adts_parse(const uint8_t *data, size_t len, size_t *frame_len, size_t *payload_off, size_t *payload_len,
                  uint8_t asc[2]);

/* ---- the audio_packet::Decoder surface for one ADTS AAC-LC stream ------------------------------------ */
/* soundkit::audio_packet::Decoder (soundkit/src/audio_packet.rs:22-26) as soundkit-aac's AacDecoder implements it
 * (soundkit-aac/src/lib.rs:108-266) and the worker drives it (decode_i16_with_drain, soundkit-decoder lib.rs:
 * 2150-2181): each call appends `input` (<= 4 MiB per call and buffered) and decodes every whole frame that is
 * buffered and fits in `output`; *written = interleaved samples; 0 = needs more input / drained.  Call once with
 * data, then with len 0 until it returns 0.  decode_i32 is "Not implemented." in the reference and absent here. */
typedef struct sk_adts_decoder sk_adts_decoder;
int sk_adts_decoder_create(sk_engine *, sk_adts_decoder **out);
void sk_adts_decoder_destroy(sk_adts_decoder *);
int sk_adts_decoder_decode_i16(sk_adts_decoder *, const uint8_t *input, size_t len, int16_t *output, size_t out_cap,
                               size_t *written);
int sk_adts_decoder_decode_f32(sk_adts_decoder *, const uint8_t *input, size_t len, float *output, size_t out_cap,
                               size_t *written);
/* sample_rate() / channels() (lib.rs:133-139): 0 until the first frame has been decoded */
int sk_adts_decoder_info(const sk_adts_decoder *, uint32_t *sample_rate, uint8_t *channels);
const char *sk_adts_decoder_last_error(const sk_adts_decoder *);

/* dsp.rs:389-450 dequantize_signed_scaled over a batch: out[i] = sign(q)*|q|^(4/3)*2^((sf-100)/4).
 * quant: n i16 quantised values; sf_per_band_of[i]: i16 scale factor applying to value i. */
int sk_aac_dequantize_dev(sk_engine *, const int16_t *d_quant, const int16_t *d_scalefactor, float *d_out, size_t n);
int sk_aac_dequantize(sk_engine *, const int16_t *quant, const int16_t *scalefactor, float *out, size_t n);

/* ---- MPEG-1/2 Layer III hybrid synthesis ----------------------------------------------------------------
 * The transform half of what Mp3Decoder gets from nanomp3::Decoder::decode (soundkit-mp3/src/lib.rs:279-305, :284): for
 * every granule and channel, 576 requantised / stereo-processed / reordered frequency lines -> alias reduction ->
 * IMDCT 36 or 3 x 12 with the block-type windows -> overlap-add -> frequency inversion -> 32-band polyphase synthesis
 * (ISO/IEC 11172-3 2.4.3.4), 576 PCM samples out, float in +-1.0 interleaved as nanomp3 emits them, or s16 through
 * f32_to_i16 (lib.rs:376-385).  Carried state (overlap, polyphase FIFO) is per engine stream, reset by sk_stream_open /
 * sk_stream_reset.  The synthesis window D (Table B.3) is set once per engine: sk_mp3_decoder_create does it (with the
 * standard's table, csrc/mp3_iso_tables.h, unless the caller brings its own); callers of the bare stage call
 * sk_mp3_set_synthesis_window -- until then the synthesis entry points return SK_ERR_UNSUPPORTED.  Sample parity with
 * nanomp3 is unpinned (its source is absent); what pins this row is the decode of the reference's two MP3 fixtures against
 * the source PCM the reference holds for them (tests/test_mp3_fixtures_gpu.py).
 * Lines of a short block (block_type 2) are window-interleaved: X_w[m] = xr[18 sb + 3 m + w]. */
typedef struct sk_mp3_granule_desc {
    uint32_t stream;
    uint8_t channels;            /* 1 or 2; must equal the stream's */
    uint8_t block_type[2];       /* per channel: 0 normal, 1 start, 2 short, 3 stop */
    uint8_t mixed_block_flag[2]; /* per channel, meaningful with block_type 2 */
    uint8_t reserved[3];
} sk_mp3_granule_desc;
int sk_mp3_set_synthesis_window(sk_engine *, const float *d512);
/* xr: granule i holds channels x 576 f32, granules packed back to back; pcm_out: granule i holds 576 x channels
 * interleaved samples at the same packing.  A granule whose status != 0 leaves silence. */
int sk_mp3_hybrid_synthesize_f32(sk_engine *, const sk_mp3_granule_desc *descs, const float *xr, float *pcm_out, uint32_t n,
                                 int32_t *status_per_granule);
int sk_mp3_hybrid_synthesize_s16(sk_engine *, const sk_mp3_granule_desc *descs, const float *xr, int16_t *pcm_out, uint32_t n,
                                 int32_t *status_per_granule);
int sk_mp3_hybrid_synthesize_f32_dev(sk_engine *, const sk_mp3_granule_desc *descs, const float *d_xr, float *d_pcm, uint32_t n,
                                     int32_t *status_per_granule);

/* ---- MPEG Layer III: the fixed-syntax front of the bitstream half, and requantisation / stereo / reorder -------------
 * What nanomp3::Decoder::decode (soundkit-mp3/src/lib.rs:284) does between the bytes and its Huffman stage, and between that
 * stage and the hybrid synthesis above -- the parts that are closed-form syntax and arithmetic of ISO/IEC 11172-3 /
 * 13818-3.  The band tables (Table B.8) and the pre-emphasis table are set per engine and sampling rate like the synthesis
 * window (sk_mp3_decoder_create does it).  The reference's two MP3 fixtures pin the framing (tests/test_mp3_bitstream.py). */
enum sk_mp3_status {
    SK_MP3_NEED_MORE = -301,   /* not enough bytes for the header / side information / frame / reservoir */
    SK_MP3_NO_SYNC = -302,     /* not a frame header */
    SK_MP3_UNSUPPORTED = -303, /* sk_mp3_*: a Layer I / II header (sk_mpa_* read those); a free-format header whose frame length is not
                                  known (sk_mp3_scan_free measures it; Layer I / II free format is not built) */
    SK_MP3_INVALID = -304      /* a field combination the syntax forbids */
};
typedef struct sk_mp3_frame_info { /* nanomp3::FrameInfo (lib.rs:188-215 reads sample_rate, channels, bitrate) + framing */
    uint32_t offset;             /* sk_mp3_scan: position of the frame in the scanned buffer */
    uint32_t frame_bytes;        /* header to the next header */
    uint32_t sample_rate;
    uint16_t bitrate_kbps, samples_per_channel; /* 1152 (MPEG-1) or 576 (MPEG-2 / 2.5) */
    uint8_t version;             /* 1, 2 or 25 (= MPEG-2.5) */
    uint8_t channels, mode, mode_ext, has_crc, padding, granules, side_info_bytes;
} sk_mp3_frame_info;
typedef struct sk_mp3_granule_side { /* 11172-3 2.4.1.7 / 13818-3 2.4.1.7, one granule of one channel */
    uint16_t part2_3_length, big_values, scalefac_compress;
    uint8_t global_gain, window_switching, block_type, mixed_block_flag, table_select[3], subblock_gain[3], region0_count,
        region1_count, preflag, scalefac_scale, count1table_select, reserved;
} sk_mp3_granule_side;
typedef struct sk_mp3_side_info {
    uint16_t main_data_begin;
    uint8_t granules, channels;
    uint8_t scfsi[2][4];
    sk_mp3_granule_side gr[2][2]; /* [granule][channel] */
} sk_mp3_side_info;
int sk_mp3_parse_header(const uint8_t *data, size_t len, sk_mp3_frame_info *out);
int sk_mp3_parse_side_info(const uint8_t *frame, size_t len, const sk_mp3_frame_info *header, sk_mp3_side_info *out);
/* every frame of a byte stream (an ID3v2 tag in front is stepped over, garbage skipped, a header counts only if the next
 * frame's header follows it); *consumed = bytes up to the first incomplete frame */
int sk_mp3_scan(const uint8_t *data, size_t len, sk_mp3_frame_info *frames, uint32_t cap, uint32_t *n_frames, size_t *consumed);
/* The same with free-format streams (bit-rate index 0): the frame length is what lies between a header and the next two of the same
 * stream, as minimp3's mp3d_find_frame measures it (nanomp3 is its port; soundkit-mp3/src/lib.rs:284).  *free_format_bytes carries
 * that length (without the padding slot) from call to call, 0 at the start of a stream; sk_mp3_parse_header_free reads a header with
 * it.  The decoder handles and the batch scheduler use these two. */
int sk_mp3_scan_free(const uint8_t *data, size_t len, sk_mp3_frame_info *frames, uint32_t cap, uint32_t *n_frames, size_t *consumed,
                     uint32_t *free_format_bytes);
int sk_mp3_parse_header_free(const uint8_t *data, size_t len, uint32_t free_format_bytes, sk_mp3_frame_info *out);
/* the bytes parts 2 + 3 of a frame are read from: main_data_begin bytes of the reservoir + the frame's own main data */
int sk_mp3_main_data(const uint8_t *frame, size_t frame_len, const sk_mp3_frame_info *header, const sk_mp3_side_info *side,
                     const uint8_t *prev_main_data, size_t prev_len, uint8_t *out, size_t out_cap, size_t *out_len);

/* Requantisation (2.4.3.4.7.1), mid/side and MPEG-1 intensity stereo (2.4.3.4.9-10) and the short-block reorder
 * (2.4.3.4.8) for a batch of granules on the GPU: is = the Huffman stage's integers, [granule][channel][576] in bitstream
 * order; xr = what sk_mp3_hybrid_synthesize_* takes.  Band tables (Table B.8: 23 long and 14 short offsets per sampling
 * rate) and the pre-emphasis table (22 entries) come from the caller, once per engine and sampling rate. */
typedef struct sk_mp3_requant_channel {
    uint8_t global_gain, scalefac_scale, preflag, block_type, mixed_block_flag, subblock_gain[3];
    uint8_t scalefac_l[22];    /* long bands (also the long part of a mixed block) */
    uint8_t scalefac_s[13][3]; /* short bands x windows */
    uint8_t reserved;
} sk_mp3_requant_channel;
typedef struct sk_mp3_requant_granule {
    uint32_t sample_rate;
    uint8_t channels, ms_stereo, intensity_stereo, lsf; /* mode_ext bits of a joint-stereo frame; lsf: MPEG-2 / 2.5.  intensity_stereo: bit 0
                                                         * = on; bit 1 (lsf only) = intensity_scale, the low bit of the right channel's
                                                         * scalefac_compress (13818-3 2.4.3.2: i0 = 2^-1/2 instead of 2^-1/4).  In an lsf
                                                         * intensity granule bit 7 of a RIGHT-channel scale factor marks its position as
                                                         * "not intensity coded" (the largest value its field holds); the factor is bits 0-6 */
    sk_mp3_requant_channel ch[2];
} sk_mp3_requant_granule;
int sk_mp3_set_band_tables(sk_engine *, uint32_t sample_rate, const uint16_t long_offsets[23], const uint16_t short_offsets[14],
                           const uint8_t pretab[22]);
int sk_mp3_requantize(sk_engine *, const sk_mp3_requant_granule *granules, const int16_t *is, float *xr, uint32_t n,
                      int32_t *status_per_granule);
/* The two GPU stages back to back -- sk_mp3_requantize then sk_mp3_hybrid_synthesize_* with descs[i] describing the same
 * granule as granules[i] -- the frequency lines staying on the device: integers in, interleaved PCM out, one
 * synchronisation.  What sk_mp3_decoder_decode_* runs per call. */
int sk_mp3_decode_granules_f32(sk_engine *, const sk_mp3_requant_granule *granules, const sk_mp3_granule_desc *descs, const int16_t *is,
                               float *pcm_out, uint32_t n, int32_t *status_per_granule);
int sk_mp3_decode_granules_s16(sk_engine *, const sk_mp3_requant_granule *granules, const sk_mp3_granule_desc *descs, const int16_t *is,
                               int16_t *pcm_out, uint32_t n, int32_t *status_per_granule);

/* ---- MPEG Layer III: scale factors, the Huffman stage and a decoder handle in Mp3Decoder's shape ----------------------
 * Parts 2 and 3 of the main data are syntax over data tables of the standard.  They enter in the standard's own
 * presentation -- for every code its length and its bits -- and the library builds its decoding structures from that.
 * sk_mp3_iso_tables hands out the standard's tables (csrc/mp3_iso_tables.h: normative constants of ISO/IEC 11172-3 B.3 /
 * B.6 / B.7 / B.8 and 13818-3 2.4.3.2, written by tools/transcribe_iso_mp3_tables.py, which records where they were read
 * and the checks that gate them); a caller may pass any other complete prefix code set instead (the syntax tests do). */
typedef struct sk_mp3_code_table { /* one table of ISO/IEC 11172-3 Table B.7 */
    uint8_t xlen;                  /* values 0 .. xlen-1 for x and for y; 0 = table carries no codes (tables 0, 4, 14) */
    uint8_t linbits;
    const uint8_t *hlen;           /* [xlen * xlen], index x * xlen + y: code length in bits, 1..32 */
    const uint32_t *hcod;          /* the code, right-aligned */
} sk_mp3_code_table;
typedef struct sk_mp3_tables {
    sk_mp3_code_table big_values[32];
    uint8_t count1_hlen[2][16];    /* tables A and B of the count1 region, index v << 3 | w << 2 | x << 1 | y */
    uint8_t count1_hcod[2][16];
    uint8_t slen[16][2];           /* 11172-3 2.4.2.7: scalefac_compress -> slen1, slen2 */
    uint8_t lsf_partitions[6][3][4]; /* 13818-3 2.4.3.2: scale factors per partition, [row][long | short | mixed][partition] */
    uint16_t long_offsets[9][23];  /* Table B.8 by sampling rate: 44100 48000 32000 22050 24000 16000 11025 12000 8000 */
    uint16_t short_offsets[9][14];
    uint8_t rates_present[9];      /* which rows of the two arrays above are filled in */
    uint8_t pretab[22];
    float window[512];             /* Table B.3 */
} sk_mp3_tables;
typedef struct sk_mp3_codebook sk_mp3_codebook; /* validated copies + prefix-decoding tables on the host; sk_mp3_set_codebook puts
                                                 * a flattened form on an engine for the device Huffman stage */
int sk_mp3_codebook_create(const sk_mp3_tables *, sk_mp3_codebook **out); /* SK_MP3_INVALID: a code set that is no prefix code */
void sk_mp3_codebook_destroy(sk_mp3_codebook *);
int sk_mp3_iso_tables(sk_mp3_tables *out);            /* the standard's tables; hlen / hcod point to static storage */
int sk_mp3_codebook_create_iso(sk_mp3_codebook **out); /* = sk_mp3_iso_tables + sk_mp3_codebook_create */

/* One granule of one channel out of parts 2 + 3: the scale factors in sk_mp3_requantize's layout and the 576 integers. */
typedef struct sk_mp3_granule_data {
    int16_t is[576];
    uint8_t scalefac_l[22];
    uint8_t scalefac_s[13][3];
    uint8_t preflag;     /* MPEG-1: the side information's; LSF: implied by scalefac_compress */
    uint8_t intensity_scale; /* LSF intensity channel: scalefac_compress & 1 (-> sk_mp3_requant_granule::intensity_stereo bit 1); its
                              * scale factors carry bit 7 where the position is the field's largest value ("not intensity coded") */
    uint16_t part2_bits; /* what the scale factors took of part2_3_length */
    uint16_t nonzero_lines; /* lines up to and including the last decoded pair / quadruple */
    uint16_t part3_bits; /* what the accepted pairs / quadruples took; a well-formed granule: part2_bits + part3_bits == part2_3_length */
    int32_t status;      /* SK_OK | SK_MP3_INVALID (a bit pattern that is no code, values past line 576) | SK_MP3_UNSUPPORTED */
} sk_mp3_granule_data;
/* main = what sk_mp3_main_data assembled.  out[granule][channel]; previous = the same frame's granule-0 scale factors are
 * taken from out itself (scfsi). */
int sk_mp3_decode_main_data(const sk_mp3_codebook *, const sk_mp3_frame_info *header, const sk_mp3_side_info *side, const uint8_t *main,
                            size_t main_len, sk_mp3_granule_data out[2][2]);

/* ---- parts 2 + 3 on the GPU (mp3_entropy.hip) ----
 * The code book of an engine's device Huffman stage: a flattened form of the validated tries of `cb` (NULL = the standard's
 * tables) -- per distinct code table a first-level look-up on the next 8 bits, further levels for the longer codes (any
 * prefix code set sk_mp3_codebook_create accepts, codes of up to 32 bits), slen, lsf_partitions and per sampling rate the
 * region boundaries of the long / short / mixed cut.  Replaces the engine's previous one.  Until it is called the entry
 * points below return SK_ERR_UNSUPPORTED.
 * sk_mp3_codebook_flatten is the host half alone: the blob as 32-bit words (layout: csrc/mp3_codebook_blob.h);
 * *words receives the size, SK_ERR_CAPACITY if it exceeds cap (out may be NULL with cap 0 to ask for the size). */
int sk_mp3_codebook_flatten(const sk_mp3_codebook *cb, uint32_t *out, size_t cap_words, size_t *words);
int sk_mp3_set_codebook(sk_engine *, const sk_mp3_codebook *cb);
/* One frame for the device stage: header and side information as the host parsed them, and where its assembled main data
 * (sk_mp3_main_data: reservoir bytes + the frame's own) lies in the call's byte buffer.  Laid out like the access units of
 * sk_tick_run_au: byte_offset a multiple of 4, at least 8 bytes of the buffer behind every frame's data (zero by convention;
 * the kernel never takes a bit from beyond byte_len).  byte_len at most 1 MiB; an MPEG-2 / 2.5 scalefac_compress at most 511. */
typedef struct sk_mp3_frame_item {
    sk_mp3_frame_info header;
    sk_mp3_side_info side;
    uint32_t byte_offset;
    uint32_t byte_len;
} sk_mp3_frame_item;
/* The stage alone, results on the host -- the device counterpart of sk_mp3_decode_main_data, and equal to it in every
 * field: out[frame][granule][channel], only the cells a frame has are written. */
int sk_mp3_entropy_decode(sk_engine *, const sk_mp3_frame_item *frames, uint32_t n_frames, const uint8_t *main_bytes, size_t main_len,
                          sk_mp3_granule_data *out /*[n_frames][2][2]*/);
/* Huffman stage -> requantisation -> hybrid synthesis, the integers and lines staying on the device.  streams[i] is the
 * open stream frame i belongs to (frames of one stream in order).  A frame any of whose granule-channels the Huffman stage
 * rejects is dropped as the host path drops it: entropy_status[i] is that status (SK_MP3_*), the frame takes no room in
 * pcm_out and its stream's overlap / polyphase state is not touched.  The other frames' samples (samples_per_channel x
 * channels, interleaved) follow one another in pcm_out in frame order; stage_status[i] (may be NULL) is what
 * sk_mp3_decode_granules_* would have reported for the frame's granules (the first non-zero one; such a frame keeps its room,
 * filled as that function fills it).  *samples_written = samples in pcm_out, at most out_cap (else SK_ERR_CAPACITY, nothing
 * synthesised).  The statuses cross back between the first kernel and the two later ones: one synchronisation more per
 * call than sk_mp3_decode_granules_*. */
int sk_mp3_decode_frames_f32(sk_engine *, const sk_mp3_frame_item *frames, const uint32_t *streams, uint32_t n_frames, const uint8_t *main_bytes,
                             size_t main_len, float *pcm_out, size_t out_cap, int32_t *entropy_status, int32_t *stage_status,
                             size_t *samples_written);
int sk_mp3_decode_frames_s16(sk_engine *, const sk_mp3_frame_item *frames, const uint32_t *streams, uint32_t n_frames, const uint8_t *main_bytes,
                             size_t main_len, int16_t *pcm_out, size_t out_cap, int32_t *entropy_status, int32_t *stage_status,
                             size_t *samples_written);

/* Mp3Decoder (soundkit-mp3/src/lib.rs:147-374): bytes in at any chunking, interleaved PCM out.  One call decodes every
 * complete frame its input buffer holds -- framing, reservoir, scale factors and Huffman on the host, then ONE
 * requantisation launch and ONE hybrid-synthesis launch over all their granules -- subject to the reference's output rule:
 * it stops once fewer than SK_MP3_MAX_SAMPLES_PER_FRAME samples of room are left (lib.rs:300-302) and fails with
 * SK_ERR_CAPACITY if a frame does not fit (lib.rs:237-243).  Input beyond 4 MiB buffered: SK_PIPE_CHUNK_TOO_LARGE
 * (lib.rs:155, 219-227).  A frame whose main data reaches further back than the reservoir holds (a stream joined in the
 * middle) is consumed without output, as are frames the later stages reject.
 * A stream whose first confirmed frame (two consistent headers one frame length apart) is Layer I or II is decoded as that layer
 * with no switch (sk_mpa_scan, sk_mpa_parse_frame, one sk_mpa_decode_frames_* per call): 384 or 1152 samples per channel and frame,
 * the same output rules; headers of another layer are no frames of it.  Streams that start as Layer III take the path above. */
#define SK_MP3_MAX_SAMPLES_PER_FRAME 2304u
typedef struct sk_mp3_decoder sk_mp3_decoder;
/* Mp3Decoder::new, lib.rs:157.  codebook NULL = the standard's tables (what nanomp3 has built in); the decoder installs the
 * codebook's band tables and synthesis window on the engine. */
int sk_mp3_decoder_create(sk_engine *, const sk_mp3_codebook *, sk_mp3_decoder **out);
void sk_mp3_decoder_destroy(sk_mp3_decoder *);
int sk_mp3_decoder_reset(sk_mp3_decoder *);                                           /* lib.rs:180-185 */
/* on != 0: scale factors and Huffman decode run on the GPU (sk_mp3_set_codebook with the decoder's code book, then one
 * sk_mp3_decode_frames_* per call); framing, side information and the bit reservoir stay on the host.  Same samples, `written`,
 * return codes and sk_mp3_decoder_info as with the host stage, for any input at any chunking.  Default off.
 * The device code book is the ENGINE's (one at a time): a GPU-mode decoder installs its own before each call, which is safe for
 * decoders of one engine that share a code book (the usual case: the standard's) or a thread; decoders with DIFFERENT code books
 * driven from different threads need an engine each.
 * SK_ERR_UNSUPPORTED in a build without the device stage. */
int sk_mp3_decoder_set_gpu_entropy(sk_mp3_decoder *, int on);
/* sample_rate / channels are 0 until the first frame was decoded (Option::None, lib.rs:167-173); buffer_len: lib.rs:176 */
int sk_mp3_decoder_info(const sk_mp3_decoder *, uint32_t *sample_rate, uint8_t *channels, size_t *buffer_len, uint64_t *frames_decoded);
int sk_mp3_decoder_decode_i16(sk_mp3_decoder *, const uint8_t *input, size_t len, int16_t *out, size_t out_cap, size_t *written);
int sk_mp3_decoder_decode_i32(sk_mp3_decoder *, const uint8_t *input, size_t len, int32_t *out, size_t out_cap, size_t *written);
int sk_mp3_decoder_decode_f32(sk_mp3_decoder *, const uint8_t *input, size_t len, float *out, size_t out_cap, size_t *written);

/* ---- MPEG Layer I and II (ISO/IEC 11172-3 2.4.1.5-6, 13818-3 2.4.1) ------------------------------------------------------------
 * The other two layers nanomp3 decodes behind Mp3Decoder (soundkit-mp3/src/lib.rs:284).  No Huffman stage, no reservoir, no IMDCT:
 * a short serial front (allocation, scale-factor selection, scale factors) that the host reads, after which every sample code of the
 * frame stands at a computable bit position -- the kernel (csrc/mp12_synth.hip) fetches the codes from the frame's bytes as they
 * were uploaded, requantises them and runs the same 32-band polyphase synthesis, on the same per-stream FIFO, as Layer III.
 * The sk_mp3_* entry points above keep their Layer III-only answers; these know all three layers.
 * Not built (SK_MP3_UNSUPPORTED / no frame): free-format Layer I / II, MPEG-2.5 with Layer I / II (not defined by the standards),
 * CRC verification (the word is stepped over), the multichannel extension of 13818-3. */
typedef struct sk_mpa_frame_info {
    uint32_t offset;             /* sk_mpa_scan: position of the frame in the scanned buffer */
    uint32_t frame_bytes;        /* header to the next header */
    uint32_t sample_rate;
    uint16_t bitrate_kbps, samples_per_channel; /* 384 (Layer I), 1152 (Layer II), 1152 / 576 (Layer III) */
    uint8_t version;             /* 1, 2 or 25 (= MPEG-2.5, Layer III only) */
    uint8_t layer;               /* 1, 2 or 3 */
    uint8_t channels, mode, mode_ext, has_crc, padding, reserved;
} sk_mpa_frame_info;
/* SK_MP3_UNSUPPORTED: a free-format header of any layer (no length in it), MPEG-2.5 with Layer I / II */
int sk_mpa_parse_header(const uint8_t *data, size_t len, sk_mpa_frame_info *out);
/* Frames of ONE layer out of a byte stream, with sk_mp3_scan's rules (an ID3v2 tag in front is stepped over, garbage skipped, a
 * header counts only if a header of the same version, layer and sampling rate follows it one frame length on, or the data ends
 * there).  *layer in: 1 ... 3 = the stream's layer, headers of another are no frames; 0 = not known yet: the stream's layer is that of
 * its first CONFIRMED frame (the following header must be in the buffer: until it is, nothing is consumed from the candidate on),
 * and *layer receives it.  *consumed = bytes up to the first incomplete frame. */
int sk_mpa_scan(const uint8_t *data, size_t len, uint32_t *layer, sk_mpa_frame_info *frames, uint32_t cap, uint32_t *n_frames, size_t *consumed);
/* One Layer I / II frame as the kernel takes it.  cls[ch][sb], the quantisation class: 0 = nothing sent; 2 ... 16 = three (Layer I: one)
 * codes of that many bits per granule (slot), steps = 2^bits - 1; 0x80 | 3, 5 or 9 = Layer II's grouped classes, three samples of that
 * many steps in one code word of 5, 7 or 10 bits.  Above `bound` (joint stereo) both channels carry the class of the shared code.
 * scf[ch][sb][part]: the scale-factor index (0 ... 63, factor 2^(1 - i/3); the standard's table ends at 62, 63 continues the closed
 * form) of parts 0 ... 2 of the frame (Layer II: granules 0-3, 4-7, 8-11; Layer I: all three equal). */
typedef struct sk_mpa_frame_record {
    uint32_t byte_offset;        /* of the frame's first byte in the call's byte buffer: a multiple of 4, 8 bytes of room behind the frame */
    uint32_t byte_len;           /* frame_bytes */
    uint32_t sample_rate;
    uint32_t sample_bit;         /* bit offset of the first sample code from the frame's first byte */
    uint16_t granule_bits;       /* width of one granule (Layer II: a triple per subband and channel) or slot (Layer I) */
    uint8_t layer, channels, sblimit, bound;
    uint8_t granules;            /* 12 */
    uint8_t reserved;
    uint8_t cls[2][32];
    uint8_t scf[2][32][3];
} sk_mpa_frame_record;
/* header (as sk_mpa_parse_header gave it) + the frame's bytes -> record (byte_offset left 0).  SK_MP3_NEED_MORE: len < frame_bytes;
 * SK_MP3_INVALID: Layer I's forbidden allocation 15, or sample data that would end beyond the frame -- such a frame is consumed
 * without output, so the kernel never reads past a frame; SK_MP3_UNSUPPORTED: a Layer III header. */
int sk_mpa_parse_frame(const uint8_t *frame, size_t len, const sk_mpa_frame_info *header, sk_mpa_frame_record *out);
/* Sample unpacking, requantisation and polyphase synthesis of a batch of frames in ONE launch, one wavefront per (stream, channel)
 * walking its frames in order.  streams[i]: the open stream frame i belongs to (its channel count must be the record's).  A record
 * that does not add up (classes, widths and bounds are checked against byte_len before anything is launched) or names no such stream
 * gets status[i] != 0 and is dropped: no room in pcm_out, stream state untouched.  The other frames' samples (384 or 1152 x channels,
 * interleaved, float in +-1.0 or s16 through f32_to_i16) follow one another in frame order.  Needs the synthesis window
 * (sk_mp3_set_synthesis_window), else SK_ERR_UNSUPPORTED; *samples_written > out_cap: SK_ERR_CAPACITY, nothing synthesised. */
int sk_mpa_decode_frames_f32(sk_engine *, const sk_mpa_frame_record *records, const uint32_t *streams, uint32_t n_frames, const uint8_t *frame_bytes,
                             size_t bytes_len, float *pcm_out, size_t out_cap, int32_t *status, size_t *samples_written);
int sk_mpa_decode_frames_s16(sk_engine *, const sk_mpa_frame_record *records, const uint32_t *streams, uint32_t n_frames, const uint8_t *frame_bytes,
                             size_t bytes_len, int16_t *pcm_out, size_t out_cap, int32_t *status, size_t *samples_written);
/* The same with the HIP-event time of the launch alone (uploads and the copy back excluded) in *kernel_ms.  For measurements only
 * (tools/time_mp12.py): not part of what a binding needs, and the two calls above create no events. */
int sk_mpa_decode_frames_timed(sk_engine *, const sk_mpa_frame_record *records, const uint32_t *streams, uint32_t n_frames, const uint8_t *frame_bytes,
                               size_t bytes_len, int16_t *pcm_out, size_t out_cap, int32_t *status, size_t *samples_written, float *kernel_ms);

/* ---- sample-width / interleave conversion: soundkit::audio_bytes -------- */
/* Elementwise ops; n = number of OUTPUT samples.  Citations: soundkit/src/audio_bytes.rs
 * unless noted. */
typedef enum sk_pcm_op {
    SK_PCM_I16LE_TO_F32 = 0,      /* :3   i16le_to_f32 */
    SK_PCM_I16_TO_I16LE = 1,      /* :17  i16_to_i16le */
    SK_PCM_I16LE_TO_I16 = 2,      /* :25  i16le_to_i16 */
    SK_PCM_S24LE_TO_I32 = 3,      /* :36  s24le_to_i32 */
    SK_PCM_S24LE_TO_I16 = 4,      /* :51  s24le_to_i16 */
    SK_PCM_S24BE_TO_I16 = 5,      /* :66  s24be_to_i16 */
    SK_PCM_S32LE_TO_I32 = 6,      /* :81  s32le_to_i32 */
    SK_PCM_S32BE_TO_I32 = 7,      /* :91  s32be_to_i32 */
    SK_PCM_S32LE_TO_S24 = 8,      /* :101 s32le_to_s24 */
    SK_PCM_S32BE_TO_S24 = 9,      /* :112 s32be_to_s24 */
    SK_PCM_S32LE_TO_F32 = 10,     /* :123 s32le_to_f32 */
    SK_PCM_S32BE_TO_F32 = 11,     /* :134 s32be_to_f32 */
    SK_PCM_S32LE_TO_I16 = 12,     /* :145 s32le_to_i16 */
    SK_PCM_S32BE_TO_I16 = 13,     /* :156 s32be_to_i16 */
    SK_PCM_F32LE_TO_I16 = 14,     /* :167 f32le_to_i16 */
    SK_PCM_F32BE_TO_I16 = 15,     /* :178 f32be_to_i16 */
    SK_PCM_F32LE_TO_I32 = 16,     /* :189 f32le_to_i32 */
    SK_PCM_F32LE_TO_S24 = 17,     /* :205 f32le_to_s24 */
    SK_PCM_S16BE_TO_I16 = 18,     /* :222 s16be_to_i16 */
    SK_PCM_S16LE_TO_I16 = 19,     /* :231 s16le_to_i16 */
    SK_PCM_S16LE_TO_I32 = 20,     /* :240 s16le_to_i32 */
    SK_PCM_STEREO_TO_MONO_TAKE_LEFT = 21, /* :317 / :331 */
    SK_PCM_STEREO_TO_MONO_AVG = 22,       /* :344 / :360 */
    SK_PCM_VEC_F32_TO_I16 = 23,   /* soundkit/src/audio_pipeline.rs:17 */
    SK_PCM_VEC_I16_TO_F32 = 24,   /* soundkit/src/audio_pipeline.rs:29 */
    SK_PCM_VEC_I32_TO_F32 = 25,   /* soundkit/src/audio_pipeline.rs:40 */
    SK_PCM_FLOAT_TO_I16_ROUND = 26, /* soundkit-decoder/src/lib.rs:1815 float_sample_to_i16 */
    SK_PCM_MP3_F32_TO_I16 = 27,   /* soundkit-mp3/src/lib.rs:376 f32_to_i16 */
    SK_PCM_MP3_F32_TO_I32 = 28,   /* soundkit-mp3/src/lib.rs:387 f32_to_i32 */
    SK_PCM_OP_COUNT = 29
} sk_pcm_op;
int sk_pcm_op_in_bytes(int op);  /* bytes consumed per output sample */
int sk_pcm_op_out_bytes(int op); /* bytes produced per output sample */
int sk_pcm_convert(sk_engine *, int op, const void *in, void *out, size_t n);
int sk_pcm_convert_dev(sk_engine *, int op, const void *d_in, void *d_out, size_t n);

typedef enum sk_pcm_fmt {
    SK_FMT_S16LE = 0, SK_FMT_S16BE = 1, SK_FMT_S24LE = 2, SK_FMT_S24BE = 3,
    SK_FMT_S32LE = 4, SK_FMT_S32BE = 5, SK_FMT_F32LE = 6, SK_FMT_F32BE = 7
} sk_pcm_fmt;
int sk_pcm_fmt_bytes(int fmt);

/* Layout-only ops: interleave_vecs_i16 :250, deinterleave_vecs_i16 :264,
 * deinterleave_vecs_s24 :280 (widens to i32), deinterleave_vecs_f32 :296,
 * interleave_vecs_f32 (soundkit-decoder lib.rs:3685).  planar = [ch][frames]. */
int sk_pcm_interleave_i16(sk_engine *, const int16_t *planar, size_t frames, uint32_t ch, uint8_t *out);
int sk_pcm_deinterleave_i16(sk_engine *, const uint8_t *in, size_t frames, uint32_t ch, int16_t *planar);
int sk_pcm_deinterleave_s24(sk_engine *, const uint8_t *in, size_t frames, uint32_t ch, int32_t *planar);
int sk_pcm_deinterleave_f32(sk_engine *, const uint8_t *in, size_t frames, uint32_t ch, float *planar);
int sk_pcm_interleave_f32(sk_engine *, const float *planar, size_t frames, uint32_t ch, uint8_t *out);
int sk_pcm_interleave_i16_dev(sk_engine *, const int16_t *d_planar, size_t frames, uint32_t ch, uint8_t *d_out);
int sk_pcm_deinterleave_i16_dev(sk_engine *, const uint8_t *d_in, size_t frames, uint32_t ch, int16_t *d_planar);
int sk_pcm_deinterleave_s24_dev(sk_engine *, const uint8_t *d_in, size_t frames, uint32_t ch, int32_t *d_planar);
int sk_pcm_deinterleave_f32_dev(sk_engine *, const uint8_t *d_in, size_t frames, uint32_t ch, float *d_planar);
int sk_pcm_interleave_f32_dev(sk_engine *, const float *d_planar, size_t frames, uint32_t ch, uint8_t *d_out);

/* interleaved bytes -> planar f32.  variant 0 = soundkit-decoder audio_data_to_f32_channels
 * (lib.rs:3563-3617; any fmt; non-finite -> 0); variant 1 = soundkit::audio_to_f32_channels
 * (audio_pipeline.rs:74-98; LE only; s24 is divided by 2^31 as the reference does). */
int sk_pcm_bytes_to_f32_planar(sk_engine *, int variant, int fmt, const uint8_t *in, size_t frames, uint32_t ch,
                               float *planar);
int sk_pcm_bytes_to_f32_planar_dev(sk_engine *, int variant, int fmt, const uint8_t *d_in, size_t frames,
                                   uint32_t ch, float *d_planar);
/* planar f32 -> interleaved bytes: f32_channels_to_bytes (soundkit-decoder lib.rs:3619-3683);
 * fmt in {S16LE, S24LE, S32LE, F32LE} */
int sk_pcm_f32_planar_to_bytes(sk_engine *, int fmt, const float *planar, size_t frames, uint32_t ch, uint8_t *out);
int sk_pcm_f32_planar_to_bytes_dev(sk_engine *, int fmt, const float *d_planar, size_t frames, uint32_t ch,
                                   uint8_t *d_out);
/* the same for `batch` independent signals: planar [batch][ch][plane_stride] -> [batch][frames][ch] */
int sk_pcm_f32_planar_to_bytes_batch_dev(sk_engine *, int fmt, const float *d_planar, size_t batch, size_t plane_stride,
                                         size_t frames, uint32_t ch, uint8_t *d_out);
/* downmix_channels target 1 (soundkit-decoder lib.rs:3500-3509) */
int sk_pcm_downmix_mono(sk_engine *, const float *planar, size_t frames, uint32_t ch, float *mono);
int sk_pcm_downmix_mono_dev(sk_engine *, const float *d_planar, size_t frames, uint32_t ch, float *d_mono);
/* All of downmix_channels (soundkit-decoder lib.rs:3492-3561) for ch <= SK_MAX_PCM_CHANNELS, f32, the reference's operations in its
 * order: target 1 = the mean above; target 2 from more than two channels = L + 0.707 C + 0.707 Ls, R + 0.707 C + 0.707 Rs by channel
 * index (0 1 2 4 5; channels 3, 6, 7 unused), then both divided by m = max(|L|, |R|) over the whole input when m > 1 (a NaN never
 * raises m, an infinity does: inf * 0 = NaN as in the reference) -- two launches, the first reduces m on the device; any other
 * target = the first min(target, ch) channels (no upmix).  out is [min(target, ch)][frames]; frames <= 2^31 - 1; target >= 1. */
int sk_pcm_downmix(sk_engine *, const float *planar, size_t frames, uint32_t ch, uint32_t target, float *out);
int sk_pcm_downmix_dev(sk_engine *, const float *d_planar, size_t frames, uint32_t ch, uint32_t target, float *d_out);
/* exact_signed_pcm_to_i16 (soundkit-decoder lib.rs:3458-3489); fmt in {S24LE,S24BE,S32LE,S32BE} */
int sk_pcm_exact_to_i16(sk_engine *, int fmt, const uint8_t *in, size_t samples, uint8_t *out_s16le);
int sk_pcm_exact_to_i16_dev(sk_engine *, int fmt, const uint8_t *d_in, size_t samples, uint8_t *d_out_s16le);

/* ---- 48 kHz -> 16 kHz sinc FIR ------------------------------------------ */
/* Replaces soundkit::audio_pipeline::downsample_audio (audio_pipeline.rs:438-493) for the
 * 48000 -> 16000 case, where rubato's SincFixedIn<f32> (sinc_len 256, f_cutoff 0.95,
 * Linear, oversampling 256, BlackmanHarris2) has step exactly 3 and zero fractional phase:
 *   out[r][m] = sum_{p<256} h[p] * in[r][3m - 125 + p],  in[<0] = 0,
 *   m < sk_downsample_48k_16k_out_frames(frames) = ceil((frames - 132) / 3).
 * rows = independent channel signals (streams x channels), each `frames` long. */
uint32_t sk_downsample_48k_16k_out_frames(uint32_t frames);
int sk_downsample_48k_16k_taps(sk_engine *, float *taps256); /* the h[] the engine uses */
int sk_downsample_48k_16k_f32(sk_engine *, const float *in, uint32_t rows, uint32_t frames, float *out,
                              uint32_t *out_frames);
int sk_downsample_48k_16k_f32_dev(sk_engine *, const float *d_in, size_t in_stride, uint32_t rows, uint32_t frames,
                                  float *d_out, size_t out_stride, uint32_t *out_frames);

/* downsample_audio for any pair of the reference's COMMON_SAMPLE_RATES (audio_pipeline.rs:12-13): rubato
 * SincFixedIn<f32> with Linear interpolation between the two nearest of 256 sub-filters; one chunk = the
 * whole input, so out_frames = number of index steps below frames - 257 - ceil(in_hz/out_hz).
 * 48000 -> 16000 takes the MFMA path above; every other ratio the generic kernel (csrc/resample.hip).
 * out rows have capacity out_cap; *out_frames receives the frames produced per row. */
uint32_t sk_downsample_out_frames(uint32_t frames, uint32_t in_hz, uint32_t out_hz);
int sk_downsample_f32(sk_engine *, const float *in, uint32_t rows, uint32_t frames, uint32_t in_hz, uint32_t out_hz,
                      float *out, uint32_t out_cap, uint32_t *out_frames);
int sk_downsample_f32_dev(sk_engine *, const float *d_in, size_t in_stride, uint32_t rows, uint32_t frames,
                          uint32_t in_hz, uint32_t out_hz, float *d_out, size_t out_stride, uint32_t *out_frames);

/* downsample_audio over the frame-packed planar PCM that sk_aac_plan_run_f32_dev wrote, in place (no
 * repack): sample n of (stream s, channel c) is read at
 *   d_pcm[s * stream_stride + (n / 1024) * frame_stride + c * 1024 + n % 1024],   n < frames_per_stream * 1024
 * and row s * channels + c of d_out receives its sk_downsample_48k_16k_out_frames(..) outputs. */
int sk_downsample_48k_16k_frames_dev(sk_engine *, const float *d_pcm, size_t stream_stride, size_t frame_stride,
                                     uint32_t channels, uint32_t n_streams, uint32_t frames_per_stream, float *d_out,
                                     size_t out_stride, uint32_t *out_frames);

/* The same with the worker's 16-bit output stage (f32_channels_to_bytes, lib.rs:3619-3647: float_sample_to_i16) fused
 * into the FIR's epilogue: d_out[s][m][c] interleaved s16, out_stride frames per stream.  Bit-identical to
 * sk_downsample_48k_16k_frames_dev followed by sk_pcm_f32_planar_to_bytes_batch_dev(SK_FMT_S16LE). */
int sk_downsample_48k_16k_frames_s16_dev(sk_engine *, const float *d_pcm, size_t stream_stride, size_t frame_stride,
                                         uint32_t channels, uint32_t n_streams, uint32_t frames_per_stream,
                                         int16_t *d_out, size_t out_stride, uint32_t *out_frames);

/* apply_output_options' resample step on the worker's own data (lib.rs:3324-3456): audio_data_to_f32_channels
 * (s16 / 32768, lib.rs:3563-3617) -> 48k->16k sinc FIR -> f32_channels_to_bytes (float_sample_to_i16), over the planar s16
 * PCM of sk_aac_plan_run_s16_planar_dev, indexed like sk_downsample_48k_16k_frames_dev's input (strides in samples,
 * multiples of 4).  A 16-bit sample is exactly two bf16 values, so the matrix-core FIR needs two input planes and
 * 36 instead of 41 products per tile.  d_out[s][m][c] interleaved s16, out_stride frames per stream. */
int sk_downsample_48k_16k_frames_s16_to_s16_dev(sk_engine *, const int16_t *d_pcm16, size_t stream_stride, size_t frame_stride,
                                                uint32_t channels, uint32_t n_streams, uint32_t frames_per_stream,
                                                int16_t *d_out, size_t out_stride, uint32_t *out_frames);
/* the same filter output before the 16-bit stage: row s * channels + c of d_out (f32, out_stride per row) */
int sk_downsample_48k_16k_frames_s16_to_f32_dev(sk_engine *, const int16_t *d_pcm16, size_t stream_stride, size_t frame_stride,
                                                uint32_t channels, uint32_t n_streams, uint32_t frames_per_stream,
                                                float *d_out, size_t out_stride, uint32_t *out_frames);

/* The same resample step at ANY pair of the reference's COMMON_SAMPLE_RATES the matrix-core resampler takes (44.1 kHz sources
 * above all): one-shot downsample_audio over the frames_per_stream * 1024 samples of every stream -- the chunk is the whole input,
 * the index walk starts at -128, *out_frames = sk_downsample_out_frames(frames_per_stream * 1024, in_hz, out_hz), no resampler
 * state is kept.  Input exactly as sk_downsample_48k_16k_frames_s16_to_s16_dev reads it: sample n of (stream s, channel c), value
 * s16 / 32768, at d_pcm16[s * stream_stride + (n / 1024) * frame_stride + c * 1024 + n % 1024]; strides in samples, multiples of 4;
 * d_pcm16 8-byte aligned; channels 1 or 2.  The samples enter the matrix cores as two f16 planes, the effective filter of every
 * output (the blend of its two sub-filters) times 2^16 as two f16 planes, three products per window: <= 1e-6 relative RMS against
 * an f64 evaluation like the f32 route (sk_downsample_f32_dev), but not its bits.
 *   _to_s16: d_out[s][m][c] interleaved s16 = float_sample_to_i16 of the filter's f32 result, out_stride frames per stream, 8-byte
 *            aligned; frames at and beyond *out_frames are not written.
 *   _to_f32: row s * channels + c of d_out, out_stride floats per row.
 * 48000 -> 16000 is sk_downsample_48k_16k_frames_s16_to_{s16,f32}_dev.  Returns SK_ERR_UNSUPPORTED -- and writes nothing -- for
 * rates outside the common set, for a step in_hz / out_hz the matrix-core form does not take (beyond about 6.9: 88.2 and 96 kHz
 * to 8 kHz among the common rates; widen to f32 rows and call sk_downsample_f32_dev), and while sk_engine_set_resampler_exact is
 * on: this entry has no scalar form and never changes arithmetic silently.  n_streams == 0 or no output frames: SK_OK. */
int sk_downsample_frames_s16_to_s16_dev(sk_engine *, const int16_t *d_pcm16, size_t stream_stride, size_t frame_stride,
                                        uint32_t channels, uint32_t n_streams, uint32_t frames_per_stream, uint32_t in_hz,
                                        uint32_t out_hz, int16_t *d_out, size_t out_stride, uint32_t *out_frames);
int sk_downsample_frames_s16_to_f32_dev(sk_engine *, const int16_t *d_pcm16, size_t stream_stride, size_t frame_stride,
                                        uint32_t channels, uint32_t n_streams, uint32_t frames_per_stream, uint32_t in_hz,
                                        uint32_t out_hz, float *d_out, size_t out_stride, uint32_t *out_frames);

/* In a library built with packed-f32 instructions (sk_kernels_use_packed_f32() == 1) this entry point is WITHDRAWN: it returns
 * SK_ERR_UNSUPPORTED for every plan -- use the two calls -- unless SK_AAC_TAIL_ONE_LAUNCH=1 is in the environment, which is for
 * reproducing the defect only: a kernel whose waves run the synthesis with packed-f32 instructions while others of them run
 * matrix instructions on the same SIMDs is what this platform computes wrongly (profiles/r04_lanes_corruption.md); at the
 * headline batch 3 % of its samples are wrong, differently in every run.  In the default build (no packed-f32 instructions) it
 * is exact at every size.
 * sk_aac_plan_run_s16_planar_dev + sk_downsample_48k_16k_frames_s16_to_s16_dev over all frames of a plan as ONE launch
 * (decode_aac_access_unit + apply_output_options, lib.rs:1793-1813, 3324-3456): the s16 PCM between the two never crosses
 * HBM -- each channel's wave keeps its last 2048 samples as the FIR's two f16 planes in LDS and runs the FIR on them as
 * they complete.  Same arithmetic in the same order as the two calls.  For plans whose channels are all free of
 * EightShort frames and pair up (two channels of equal length), every stream with `channels` channels and
 * `frames_per_stream` frames from its frame 0; anything else returns SK_ERR_UNSUPPORTED: use the two calls.
 * stream_stride: samples between the first frames of consecutive streams in the spectra's packing (as above);
 * d_out[s][m][c] interleaved s16, out_stride frames per stream (a multiple of 4), 8-byte aligned. */
int sk_aac_plan_run_tail_s16_dev(sk_engine *, const sk_aac_plan *, const float *d_coeffs, size_t stream_stride, uint32_t channels,
                                 uint32_t frames_per_stream, int16_t *d_out, size_t out_stride, uint32_t *out_frames);

/* StreamingResampler (soundkit-decoder lib.rs:1917-2060), any pair of COMMON_SAMPLE_RATES, fixed 4096-frame
 * chunks, history kept per stream on the device.  in: n_streams x channels x frames planar
 * (stream-major); out: capacity out_cap frames per channel row; out_frames[s] receives the
 * frames produced for stream s by this call (0 until 4096 input frames have accumulated). */
int sk_resampler_open(sk_engine *, uint32_t stream, uint32_t in_hz, uint32_t out_hz);
int sk_resampler_close(sk_engine *, uint32_t stream);
int sk_resampler_process_f32(sk_engine *, const uint32_t *streams, uint32_t n_streams, const float *in,
                             uint32_t frames, float *out, uint32_t out_cap, uint32_t *out_frames);
int sk_resampler_flush_f32(sk_engine *, const uint32_t *streams, uint32_t n_streams, float *out, uint32_t out_cap,
                           uint32_t *out_frames);

/* ---- one scheduler tick: a batch of access units through the worker's output stage ---------------- */
/* For every access unit of every listed stream: decode_aac_access_unit (soundkit-decoder lib.rs:1793-1813: synthesis,
 * then float_sample_to_i16) followed by apply_output_options (lib.rs:3324-3456: fast path, or i16 -> f32 ->
 * StreamingResampler -> downmix -> f32_channels_to_bytes), one launch sequence for the whole batch.  The outputs are
 * the AudioData values the reference's pipeline_worker would have sent (lib.rs:3238-3259), per stream in order:
 * one per access unit without resampling, one per completed 4096-frame chunk with it (lib.rs:1970-2003), plus
 * the flushed tail when `flush` is set (lib.rs:2017-2058, 3307-3322). */
typedef struct sk_tick_stream {
    uint32_t stream;      /* engine stream; its access units are contiguous in descs / coeffs, streams in this order */
    uint32_t n_frames;    /* access units of this stream in the batch (may be 0 with flush) */
    uint8_t out_bits;     /* DecodeOptions::output_bits_per_sample resolved: 16 / 24 / 32 (signed little-endian) */
    uint8_t out_channels; /* DecodeOptions::output_channels resolved (source channels when None) */
    uint8_t resample;     /* 1: route through the stream's resampler (sk_resampler_open) */
    uint8_t flush;        /* 1: end of stream: flush the resampler after these frames */
    uint8_t codec;        /* SK_TICK_AAC (0) | SK_TICK_MP3: an MP3 stream's units are GRANULES (576 PCM frames each), taken in order
                           * from sk_tick_input's mp3_* arrays; only sk_tick_run_mixed accepts them */
    uint8_t reserved[3];
} sk_tick_stream;
enum { SK_TICK_AAC = 0, SK_TICK_MP3 = 1, SK_TICK_MPA = 2 /* Layer I / II: sk_tick_run_mixed_mpa; n_frames counts FRAMES */ };

typedef struct sk_tick_output {
    uint32_t stream_index; /* index into the tick's stream table */
    uint32_t frames;       /* PCM frames in this AudioData */
    uint64_t byte_offset;  /* into out_bytes (16-byte aligned) */
    uint32_t bytes;        /* frames * channels * bits / 8 */
    int32_t status;        /* 0, or the sk_frame_status of an access unit the engine rejected: the stream ends there */
    uint8_t channels, bits;
    uint16_t reserved;     /* flags: SK_TICK_OUT_FLOAT (bit 0): the samples are 32-bit floats, not signed integers (only sk_tick_run_pcm sets it) */
} sk_tick_output;
#define SK_TICK_OUT_FLOAT 1u

/* upper bounds for the two output arrays of a tick: from the table alone (a resampling stream is taken for the largest ratio there
 * is, 8 -> 48 kHz: 48 KB per chunk and output channel at 32 bits), or -- _on -- from what the engine knows of the streams (their
 * resamplers' own ratios): the scheduler sizes its pinned output buffers with the second (the first made them gigabytes) */
size_t sk_tick_out_bound(const sk_tick_stream *streams, uint32_t n_streams, uint32_t *max_outputs);
size_t sk_tick_out_bound_on(sk_engine *, const sk_tick_stream *streams, uint32_t n_streams, uint32_t *max_outputs);
/* coeffs: host memory (pinned for full overlap), packed like sk_aac_synthesize_f32's.  Blocks until out_bytes holds
 * the results.  *out_bytes_used receives the bytes written. */
int sk_tick_run(sk_engine *, const sk_tick_stream *streams, uint32_t n_streams, const sk_aac_frame_desc *descs,
                const float *coeffs, uint32_t n_frames, uint8_t *out_bytes, size_t out_cap, sk_tick_output *outputs,
                uint32_t outputs_cap, uint32_t *n_outputs, size_t *out_bytes_used);

/* One tick over streams of both codecs -- the worker's per-format dispatch (FormatDecoder::process,
 * soundkit-decoder/src/lib.rs:2222-2241) for a whole batch: the AAC streams' units in ONE of the three forms above (spectra,
 * access units, or quantised values: leave the others NULL), the MP3 streams' granules as sk_mp3_decode_granules_* takes them
 * (Huffman stage done on the host: sk_mp3_decode_main_data), listed stream by stream in the order of `streams`.  An MP3
 * granule becomes what Mp3Decoder hands the worker -- i16 through f32_to_i16 (soundkit-mp3/src/lib.rs:376-385) -- and then
 * takes the same apply_output_options path as an AAC unit (fast path, or / 32768 -> StreamingResampler -> downmix -> bytes).
 * Outputs: one AudioData per AAC access unit / MP3 granule without resampling, one per 4096-frame chunk with it.
 * The engine must hold the MP3 tables (sk_mp3_set_band_tables / sk_mp3_set_synthesis_window, or any sk_mp3_decoder_create). */
typedef struct sk_tick_input {
    const sk_aac_frame_desc *descs;          /* host front-end: descs + coeffs; quantised hand-over: descs + q_sides + q_quant */
    const float *coeffs;
    const struct sk_au_item *units;          /* GPU front-end: units + au_bytes */
    const uint8_t *au_bytes;
    size_t au_bytes_len;
    const void *q_sides;
    const int16_t *q_quant;
    uint32_t n_aac_units;
    uint32_t n_mp3_granules;
    const sk_mp3_requant_granule *mp3_granules;
    const sk_mp3_granule_desc *mp3_descs;
    const int16_t *mp3_is;                   /* [granule][channel][576], granules packed back to back */
} sk_tick_input;
int sk_tick_run_mixed(sk_engine *, const sk_tick_stream *streams, uint32_t n_streams, const sk_tick_input *in, uint8_t *out_bytes,
                      size_t out_cap, sk_tick_output *outputs, uint32_t outputs_cap, uint32_t *n_outputs, size_t *out_bytes_used);

/* sk_tick_run_mixed with the MP3 streams' Huffman stage on the device as well (sk_mp3_set_codebook first): instead of
 * mp3_granules / mp3_descs / mp3_is (leave them NULL / 0) the MP3 streams' units arrive as FRAMES with their assembled main data,
 * laid out as for sk_mp3_decode_frames_*, listed stream by stream in the order of `streams`; an MP3 stream's n_frames counts its
 * frames here.  Same outputs as sk_tick_run_mixed gives for the same streams with the host stage.  A frame any of whose
 * granule-channels the stage rejects is dropped as the host path drops it: no output record, its rows enter no resampler, the
 * stream's synthesis state is as if the frame had never been queued, and the stream goes on.  The verdicts cross back before the
 * tick is planned: one synchronisation more than sk_tick_run_mixed. */
typedef struct sk_tick_mp3_frames {
    const sk_mp3_frame_item *frames;
    uint32_t n_frames;
    const uint8_t *main_bytes;
    size_t main_len;
} sk_tick_mp3_frames;
int sk_tick_run_mixed_md(sk_engine *, const sk_tick_stream *streams, uint32_t n_streams, const sk_tick_input *in, const sk_tick_mp3_frames *md,
                         uint8_t *out_bytes, size_t out_cap, sk_tick_output *outputs, uint32_t outputs_cap, uint32_t *n_outputs,
                         size_t *out_bytes_used);

/* The same with Layer I / II streams in the tick (codec SK_TICK_MPA): their units arrive as FRAMES -- records as sk_mpa_parse_frame
 * made them and the frames' bytes, laid out as for sk_mpa_decode_frames_*, listed stream by stream in the order of `streams`; such a
 * stream's n_frames counts its frames (a budget in whole frames).  A Layer II frame becomes two units of 576 PCM frames (18 slots
 * each), a Layer I frame one of 384; each unit is one AudioData without resampling, exactly as a Layer III granule is, and takes the
 * same path from there (f32_to_i16, / 32768, resampler, downmix, bytes).  The frames of one stream are of one layer.  A record that does
 * not add up fails the call (SK_ERR_INVALID_ARG) before anything is launched: the caller's parse drops such frames.  `md` may be NULL
 * (then `in` carries the Layer III granules, if any, as for sk_tick_run_mixed); `mpa` may be NULL or empty.  sk_tick_run_mixed and
 * sk_tick_run_mixed_md are this call without Layer I / II frames.  sk_tick_out_bound* count two units per listed frame of such a stream. */
typedef struct sk_tick_mpa_frames {
    const sk_mpa_frame_record *records;
    uint32_t n_frames;
    const uint8_t *frame_bytes;
    size_t bytes_len;
} sk_tick_mpa_frames;
int sk_tick_run_mixed_mpa(sk_engine *, const sk_tick_stream *streams, uint32_t n_streams, const sk_tick_input *in, const sk_tick_mp3_frames *md,
                          const sk_tick_mpa_frames *mpa, uint8_t *out_bytes, size_t out_cap, sk_tick_output *outputs, uint32_t outputs_cap,
                          uint32_t *n_outputs, size_t *out_bytes_used);

/* ---- the tick of the WAV / raw PCM streams -------------------------------------------------------------------------- */
/* What the reference's worker does to the AudioData a WavStreamProcessor / RawPcmStreamProcessor hands it -- apply_output_options,
 * soundkit-decoder lib.rs:3324-3456 -- for every unit (= one piece of one `add`) of every listed stream, in one launch sequence:
 *   24- / 32-bit signed -> 16 bit, same rate and channels: exact_signed_pcm_to_i16 (lib.rs:3458-3489), one output per unit;
 *   any other change without a rate change: audio_data_to_f32_channels (non-finite -> 0) -> downmix_channels when out_channels <
 *     channels -> f32_channels_to_bytes, one output per unit (k_pcm_direct in registers; a source of more than two channels that is
 *     downmixed: k_pcm_wide through LDS);
 *   a rate change: bytes -> planar f32 straight into the stream's resampler rows (k_pcm_ingest / k_pcm_wide_ingest) -> the resampler
 *     rounds the other ticks use -> downmix -> bytes, one output per completed 4096-frame chunk, plus the flushed and trimmed tail with
 *     `flush`.  All rows of a wide source go through the resampler, those a downmix ignores included.
 * downmix_channels (lib.rs:3492-3561) is complete: the mean for one output channel; for two from more than two the surround
 * matrix of sk_pcm_downmix with its normalisation taken over each AudioData (one unit, or one resampled chunk); otherwise the first
 * out_channels channels.  out_channels >= channels keeps them all: there is no upmix.
 * Outputs are signed little-endian, except that 32-bit output of a float source stays float (lib.rs:3377-3382: SK_TICK_OUT_FLOAT in
 * the record's `reserved`).  A stream with nothing to change (the fast path, lib.rs:3339-3345) needs no device and is refused here
 * (SK_ERR_INVALID_ARG): its pieces are delivered as they are.
 * Limits: 1 or 2 channels, or up to SK_MAX_PCM_CHANNELS on an engine with sk_engine_enable_wide_pcm (SK_ERR_UNSUPPORTED for more, or
 * without the pool: a wide stream's resampler state is eight rows per stream, which the caller reserves), 16- / 24- / 32-bit samples
 * (the eight SK_FMT_* formats), a unit of at most 2 GiB - 1, at most 2^31 - 1 frames per stream and tick.
 * units: stream by stream in the order of `streams`; byte_offset is a multiple of 16 (the caller packs the pieces that
 * way: a lane then reads 16 samples with 16-byte loads), byte_len a whole number of frames, > 0.  A resampling stream names the
 * engine stream that holds its resampler (sk_stream_open with the source's rate and channels, sk_resampler_open); `stream` is
 * ignored otherwise.  Blocks until out_bytes holds the results.  On failure the resamplers' bookkeeping is as before the call; a
 * table the call refuses, or an out_cap / outputs_cap too small for what it would deliver, is refused before anything is queued: the
 * resamplers' rows are then as before the call too, and the same units may be sent again. */
typedef struct sk_pcm_tick_stream {
    uint32_t stream;      /* engine stream (resample = 1 only) */
    uint32_t n_units;     /* units of this stream in the tick (may be 0 with flush) */
    uint8_t format;       /* SK_FMT_* of the source */
    uint8_t channels;     /* of the source: 1 or 2; up to SK_MAX_PCM_CHANNELS with sk_engine_enable_wide_pcm */
    uint8_t out_bits;     /* DecodeOptions::output_bits_per_sample resolved: 16 / 24 / 32 */
    uint8_t out_channels; /* DecodeOptions::output_channels resolved (source channels when None) */
    uint8_t resample;     /* 1: route through the stream's resampler */
    uint8_t flush;        /* 1: end of stream: flush the resampler after these units (resample = 1 only) */
    uint8_t reserved[2];
} sk_pcm_tick_stream;
typedef struct sk_pcm_unit {
    uint64_t byte_offset; /* into `bytes`, a multiple of 16 */
    uint32_t byte_len;
    uint32_t reserved;
} sk_pcm_unit;
/* upper bounds for the two output arrays of such a tick (0 for a table sk_tick_run_pcm would refuse) */
size_t sk_tick_pcm_out_bound_on(sk_engine *, const sk_pcm_tick_stream *streams, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units,
                                uint32_t *max_outputs);
int sk_tick_run_pcm(sk_engine *, const sk_pcm_tick_stream *streams, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units,
                    const uint8_t *bytes, size_t bytes_len, uint8_t *out_bytes, size_t out_cap, sk_tick_output *outputs, uint32_t outputs_cap,
                    uint32_t *n_outputs, size_t *out_bytes_used);

/* The same tick with the entropy front-end on the GPU too (SURVEY 8f ranks 1 + 4): instead of spectra, the raw access
 * units (ADTS headers stripped) of every stream.  units[k] addresses unit k in au_bytes; units are listed stream by
 * stream in the order of `streams`, byte_offset is a multiple of 4 and every unit is followed by >= 8 zero bytes.
 * The streams must have been opened with the AudioSpecificConfig's sample rate and channel count.  A unit the
 * front-end rejects yields an output record with its sk_aac_status in `status` and ends that stream's tick, exactly
 * like a unit sk_aac_decoder_parse would have rejected on the host (same codes; the message text is host-only).
 * byte_len is at most 8192 (an ADTS frame cannot exceed 8191 bytes) and au_bytes_len at most 4 GiB - 1. */
typedef struct sk_au_item {
    uint32_t byte_offset;
    uint32_t byte_len;
} sk_au_item;
int sk_tick_run_au(sk_engine *, const sk_tick_stream *streams, uint32_t n_streams, const sk_au_item *units, uint32_t n_units,
                   const uint8_t *au_bytes, size_t au_bytes_len, uint8_t *out_bytes, size_t out_cap, sk_tick_output *outputs,
                   uint32_t outputs_cap, uint32_t *n_outputs, size_t *out_bytes_used);

/* The same tick fed by sk_aac_decoder_parse_q: per access unit the side record and the quantised i16 values (packed like
 * coeffs: unit k at the running channel count x 1024); descs as for sk_tick_run.  Dequantisation, PNS (the stream's
 * generator lives in the engine, as for sk_tick_run_au), stereo tools and TNS run on the device before the synthesis. */
int sk_tick_run_q(sk_engine *, const sk_tick_stream *streams, uint32_t n_streams, const sk_aac_frame_desc *descs,
                  const void *sides /*[n_units][SK_AAC_UNIT_SIDE_BYTES]*/, const int16_t *quant, uint32_t n_units, uint8_t *out_bytes,
                  size_t out_cap, sk_tick_output *outputs, uint32_t outputs_cap, uint32_t *n_outputs, size_t *out_bytes_used);
/* The device half of the quantised hand-over alone (what sk_aac_entropy_decode is for the full device front-end): the
 * records and integers of sk_aac_decoder_parse_q in, and back come the finished spectra [unit][channels][1024] (dequantised,
 * noise filled, intensity / mid-side, TNS: dsp.rs:397-405, spectral.rs:2408-2460, stereo.rs:114-448, tns.rs:103-276), the
 * window fields and one sk_aac_status per unit -- nothing is synthesised.  descs[k].stream names the unit's stream as
 * in sk_tick_run_q; the streams' PNS generators advance as in a tick. */
int sk_aac_expand_q_decode(sk_engine *, const uint32_t *streams, const uint32_t *units_per_stream, uint32_t n_streams,
                           const sk_aac_frame_desc *descs, const void *sides /*[n_units][SK_AAC_UNIT_SIDE_BYTES]*/, const int16_t *quant,
                           uint32_t n_units, float *coeffs_out, sk_aac_frame_desc *descs_out, int32_t *status_out);

/* The front-end alone, batched on the GPU: AacLcDecoder::decode_access_unit (soundkit-aac-lc/src/decoder.rs:104-164) up to
 * the hand-over to synthesis (decoder.rs:336) for every listed unit -- the device counterpart of sk_aac_decoder_parse.
 * Units are listed stream by stream (units_per_stream[i] of streams[i], in order), laid out as for sk_tick_run_au.
 * coeffs_out receives channels * 1024 f32 per unit, packed in unit order; descs_out[k] the stream, channel count and
 * the window_sequence / window_shape of unit k -- ready to be passed to sk_aac_synthesize_*; status_out[k] is 0 or the
 * unit's sk_aac_status (a failed unit has zero spectra; the units after it in its stream are not decoded: -199).
 * Advances each stream's PNS generator (spectral.rs:2416-2459) exactly as decoding those units does; the synthesis
 * state is untouched. */
int sk_aac_entropy_decode(sk_engine *, const uint32_t *streams, const uint32_t *units_per_stream, uint32_t n_streams,
                          const sk_au_item *units, uint32_t n_units, const uint8_t *au_bytes, size_t au_bytes_len,
                          float *coeffs_out, sk_aac_frame_desc *descs_out, int32_t *status_out);

/* ---- batch scheduler: N streams -> one submission loop per GPU ------------------------------------- */
/* Replaces one pipeline_worker thread per stream (soundkit-decoder lib.rs:2891-3038) for ADTS AAC-LC input and keeps
 * DecodePipelineHandle's contract (lib.rs:2788-2889): send never blocks and reports a full input queue (128 chunks /
 * 8 MiB), an empty chunk ends the stream (flush), at most 16 undelivered AudioData per stream (a stream whose
 * consumer does not drain it stops being scheduled: the blocking send of lib.rs:3238-3240), an error is delivered
 * after the outputs produced before it and ends that stream only (lib.rs:3131-3134).  Entropy decoding runs on
 * `entropy_threads` host threads, everything after it in sk_tick_run on the engine's GPU. */
typedef struct sk_pipeline sk_pipeline;
typedef struct sk_pipeline_config {
    uint32_t entropy_threads;            /* 0 = usable CPUs (affinity, cgroup quota) - 5, at most 64 */
    uint32_t max_streams;                /* handles open at once; 0 = 1024 (<= the engine's max_streams) */
    uint32_t max_frames_per_tick;        /* access units per GPU tick; 0 = 16384 (65536 with gpu_entropy) */
    uint32_t max_stream_frames_per_tick; /* of one stream; 0 = 8 (32 with gpu_entropy: this quota decides how full the ticks are) */
    uint32_t input_buffer;               /* chunks per input queue; 0 = DEFAULT_INPUT_BUFFER 128 (lib.rs:77) */
    uint32_t output_buffer;              /* AudioData per output queue; 0 = DEFAULT_OUTPUT_BUFFER 16 (lib.rs:78) */
    uint32_t tick_wait_us;               /* how long a non-empty batch may wait for more frames; 0 = 200 (2000 with gpu_entropy) */
    uint32_t gpu_entropy;                /* 1: the host threads only frame the ADTS stream; Huffman decode, stereo tools and TNS
                                          * run on the GPU too (sk_tick_run_au).  0 (default): host front-end (sk_tick_run).
                                          * 2: the host threads do the Huffman decode only and hand over i16 quantised values +
                                          * side records; dequantisation, PNS, stereo tools and TNS run on the GPU (sk_tick_run_q)
                                          * 3: 1, and the MP3 streams' entropy passes stop behind the bit reservoir: scale factors and
                                          * Huffman decode run in the tick (sk_tick_run_mixed_md).  SK_PIPELINE_MP3_GPU_ENTROPY=1 in the
                                          * environment makes a pipeline created with 1 behave as 3.  SK_ERR_UNSUPPORTED in a build
                                          * without the device stage */
    uint32_t lanes;                      /* engines the streams are spread over, each with its own batches and submission
                                          * thread, so that ticks overlap on the device; lane 0 is the caller's engine, the
                                          * others are created on the same device.  0 = 2 with gpu_entropy and max_streams >= two ticks' worth of
                                          * streams (4096 at the defaults), else 1; at most 8.  The engines of a device take turns with
                                          * their ticks' device work (ticks on the device at the same time were found to corrupt samples,
                                          * round 4): a lane plans, uploads and delivers while another's tick has the device.
                                          * entropy_threads and max_streams are totals, split over the lanes */
} sk_pipeline_config;

typedef struct sk_decode_options { /* DecodeOptions, lib.rs:147-151; 0 = None */
    uint32_t output_sample_rate;
    uint8_t output_bits_per_sample;
    uint8_t output_channels;
    uint16_t reserved;
} sk_decode_options;

typedef struct sk_audio_info { /* AudioData (soundkit/src/audio_types.rs:9-61) minus its bytes, or a DecodeError */
    uint32_t sampling_rate;
    uint32_t frames;
    uint32_t bytes;          /* PCM bytes (signed little-endian, interleaved), or the length of the error text */
    int32_t status;          /* error only: the sk_status / sk_aac_status behind DecodeError::DecodingFailed */
    uint8_t bits_per_sample, channel_count;
    uint8_t is_error;        /* 1: the data is the error's message and the stream has ended */
    uint8_t reserved;        /* flags: SK_AUDIO_FLOAT (EncodingFlag::PCMFloat), SK_AUDIO_BIG_ENDIAN (Endianness::BigEndian); 0 = signed little-endian */
} sk_audio_info;
#define SK_AUDIO_FLOAT 1u
#define SK_AUDIO_BIG_ENDIAN 2u

typedef struct sk_pipeline_stats {
    uint64_t ticks, frames, outputs, errors;
    uint64_t parse_ns;  /* summed over entropy threads */
    uint64_t tick_ns;   /* submission thread inside sk_tick_run */
    uint64_t idle_ns;   /* submission thread waiting for a batch */
    uint64_t deliver_ns; /* delivery thread handing outputs to the streams' queues */
    uint32_t entropy_threads; /* summed over lanes */
    uint32_t lanes;
} sk_pipeline_stats;

enum sk_pipeline_status {
    SK_PIPE_INPUT_FULL = -201,      /* DecodeError::InputBufferFull */
    SK_PIPE_CLOSED = -202,          /* DecodeError::PipelineClosed; from recv: the stream has ended and is drained */
    SK_PIPE_CHUNK_TOO_LARGE = -203  /* DecodeError::InputChunkTooLarge (> 4 MiB) */
};

int sk_pipeline_create(sk_engine *, const sk_pipeline_config *cfg /* NULL = defaults */, sk_pipeline **out);
void sk_pipeline_destroy(sk_pipeline *);
/* DecodePipeline::spawn_with_options for an ADTS AAC-LC stream (lib.rs:2590-2700, 2750-2786) */
int sk_pipeline_spawn(sk_pipeline *, const sk_decode_options *opt /* NULL = defaults */, uint32_t *handle);
/* DecodePipeline::spawn_raw_pcm_with_options (lib.rs:2469-2486): a stream of headerless PCM in the given format.  It has its
 * decoder from the start and does not detect.  SK_ERR_INVALID_ARG: the validate() of RawPcmFormat (raw_pcm.rs:117-125: rate and channels
 * > 0) or a format outside SK_FMT_*. */
typedef struct sk_raw_pcm_format {
    uint32_t sample_rate;
    uint8_t channels;
    uint8_t format;   /* SK_FMT_*: linear16 = SK_FMT_S16LE, l16 = SK_FMT_S16BE, linear32 = SK_FMT_F32LE (raw_pcm.rs:62-87) */
    uint16_t reserved;
} sk_raw_pcm_format;
int sk_pipeline_spawn_raw_pcm(sk_pipeline *, const sk_raw_pcm_format *format, const sk_decode_options *opt /* NULL = defaults */, uint32_t *handle);
/* DecodePipeline::spawn_aiff_with_options (lib.rs:2714-2724): an AIFF / AIFF-C stream with its decoder from the start -- nothing is
 * detected or gathered, every received chunk is one `add` of the walker (at most one AudioData per chunk), the end of the stream is the
 * finalising empty add.  (sk_pipeline_spawn finds such a stream by its FORM....AIFF|AIFC header too, behind the detection buffer.) */
int sk_pipeline_spawn_aiff(sk_pipeline *, const sk_decode_options *opt /* NULL = defaults */, uint32_t *handle);
int sk_pipeline_send(sk_pipeline *, uint32_t handle, const uint8_t *data, size_t len);   /* lib.rs:2795-2835 */
int sk_pipeline_finish(sk_pipeline *, uint32_t handle);                                   /* lib.rs:2838-2840 */
/* 1 = one output copied to data / info; 0 = nothing ready; SK_PIPE_CLOSED = ended and drained; SK_ERR_CAPACITY =
 * cap is smaller than info->bytes (the output stays queued).  lib.rs:2845-2858 */
int sk_pipeline_try_recv(sk_pipeline *, uint32_t handle, uint8_t *data, size_t cap, sk_audio_info *info);
int sk_pipeline_recv(sk_pipeline *, uint32_t handle, uint8_t *data, size_t cap, sk_audio_info *info, uint32_t timeout_ms);
/* For a caller that serves many handles from few threads (the reference gives every stream its own thread and a
 * blocking recv): blocks up to timeout_ms for handles that have something to receive -- outputs, or the end of their
 * stream -- and returns how many were written to `handles`.  A handle is reported once per batch of news: drain it with
 * try_recv until 0 / SK_PIPE_CLOSED; a handle left with outputs is reported again. */
int sk_pipeline_wait_outputs(sk_pipeline *, uint32_t *handles, uint32_t cap, uint32_t timeout_ms);
int sk_pipeline_cancel(sk_pipeline *, uint32_t handle); /* cancel() / Drop, lib.rs:2860-2889: frees the handle */
size_t sk_pipeline_queued_input_bytes(sk_pipeline *, uint32_t handle); /* lib.rs:2863-2866 */
int sk_pipeline_get_stats(sk_pipeline *, sk_pipeline_stats *out);
/* Where every thread of the scheduler stands, the batches, the stream table in counts and the engine's stage, as text
 * (what SK_PIPELINE_WATCHDOG=<seconds> prints when ticks stop).  Takes no lock it could block on.  Returns the length. */
size_t sk_pipeline_debug_dump(sk_pipeline *, char *buf, size_t cap);

/* ---- WAV and raw PCM stream processors (host only) --------------------------------------------------------------- */
/* WavStreamProcessor::add (soundkit/src/wav.rs:95-324) and RawPcmStreamProcessor::add / flush (soundkit/src/raw_pcm.rs:150-190), the
 * front of the scheduler's WAV / raw PCM streams, by themselves.  One `add` takes a chunk of the stream (at most 4 MiB) and gives back
 * at most one piece: the whole PCM frames available now -- *piece_len bytes (0: nothing yet) that start *piece_offset bytes into the
 * stream (counted over everything ever added), and, when `piece` is not NULL, a pointer to them that is valid until the next call on
 * the same object.  SK_PCM_ERR_STREAM: the stream is rejected; *_last_error has the reference's text. */
enum sk_pcm_stream_status { SK_PCM_ERR_STREAM = -401 };
typedef struct sk_wav_reader sk_wav_reader;
int sk_wav_reader_create(sk_wav_reader **out);
void sk_wav_reader_destroy(sk_wav_reader *);
int sk_wav_reader_add(sk_wav_reader *, const uint8_t *bytes, size_t len, uint64_t *piece_offset, size_t *piece_len, const uint8_t **piece);
/* what the fmt chunk said (zeros before it has been seen); is_float: format tag 3 (for WAVE_FORMAT_EXTENSIBLE: of the sub-format);
 * total_frames: of the data chunk as declared, 0 while unknown (wav.rs:86-93) */
int sk_wav_reader_info(const sk_wav_reader *, uint32_t *sample_rate, uint32_t *channels, uint32_t *bits, int *is_float, uint64_t *total_frames);
const char *sk_wav_reader_last_error(const sk_wav_reader *);
typedef struct sk_raw_pcm_framer sk_raw_pcm_framer;
int sk_raw_pcm_framer_create(uint32_t bytes_per_frame, sk_raw_pcm_framer **out);
void sk_raw_pcm_framer_destroy(sk_raw_pcm_framer *);
int sk_raw_pcm_framer_add(sk_raw_pcm_framer *, const uint8_t *bytes, size_t len, uint64_t *piece_offset, size_t *piece_len, const uint8_t **piece);
int sk_raw_pcm_framer_flush(sk_raw_pcm_framer *); /* end of stream: SK_PCM_ERR_STREAM when a partial frame is left */
const char *sk_raw_pcm_framer_last_error(const sk_raw_pcm_framer *);

/* ---- AIFF / AIFF-C stream walker (host only) ------------------------------------------------------------------------ */
/* AiffDecoder::add (soundkit-aiff/src/lib.rs:93-475) without its per-sample work: the FORM / COMM / SSND walk with every limit and
 * error text of the reference.  One `add` (at most 4 MiB; an EMPTY add is the finalising one, which reports a truncated stream) gives
 * at most one piece: whole sample groups as the file encodes them -- a sample, or for IMA4 one 34-byte packet per channel -- that
 * sk_aiff_decode or sk_tick_run_aiff turn into the little-endian PCM of the output contract.  *piece_offset counts sound bytes. */
enum sk_aiff_encoding {
    SK_AIFF_U8 = 0, SK_AIFF_S8, SK_AIFF_S16BE, SK_AIFF_S16LE, SK_AIFF_S24BE, SK_AIFF_S32BE, SK_AIFF_S32LE, SK_AIFF_F32BE, SK_AIFF_F64BE,
    SK_AIFF_ULAW, SK_AIFF_ALAW, SK_AIFF_IMA4,
    SK_AIFF_F64LE = 13, /* 64-bit float, little-endian: no AIFF-C file holds it; container PCM does (QuickTime `fl64` with enda = 1, CAF
                          lpcm).  12 stays unassigned: it has always been refused as unknown, and still is */
    SK_AIFF_DVD_S24 = 14 /* DVD LPCM at 24 bits (MPEG program streams): every 12-byte group holds four samples, first their four
                            big-endian 16-bit high parts, then their four low bytes; sample i leaves as the little-endian bytes
                            [g[8+i], g[2i+1], g[2i]].  A group is 12 bytes in and 12 bytes out: len is a multiple of 12 */
};
typedef struct sk_aiff_info { /* zeros (but buffered_bytes) until COMM has been read */
    uint32_t sample_rate;
    uint32_t buffered_bytes; /* AiffDecoder::buffered_bytes: held back container bytes + the incomplete sample group */
    uint8_t channels;        /* 1 ... 32 */
    uint8_t encoding;        /* enum sk_aiff_encoding: how the pieces are encoded */
    uint8_t bits;            /* the output contract: 16 / 24 / 32 */
    uint8_t is_float;        /* the output contract: 32-bit float */
} sk_aiff_info;
typedef struct sk_aiff_reader sk_aiff_reader;
int sk_aiff_reader_create(sk_aiff_reader **out);
void sk_aiff_reader_destroy(sk_aiff_reader *);
int sk_aiff_reader_add(sk_aiff_reader *, const uint8_t *bytes, size_t len, uint64_t *piece_offset, size_t *piece_len, const uint8_t **piece);
int sk_aiff_reader_info(const sk_aiff_reader *, sk_aiff_info *info);
const char *sk_aiff_reader_last_error(const sk_aiff_reader *);

/* ---- AIFF / AIFF-C decode stage (GPU) ------------------------------------------------------------------------------- */
/* decode_stream_bytes (soundkit-aiff/src/lib.rs:477-560) on the GPU (csrc/aiff_decode.hip): whole sample groups in the file's encoding
 * in, interleaved little-endian PCM of the output contract out -- u8 / s8 / mu-law / A-law / IMA4 to s16, big-endian samples
 * reversed (f32be bit for bit), f64be rounded to f32 (nearest even; subnormals kept, overflow to infinity), sowt / 23ni copied.
 * IMA4 (1 or 2 channels, 34-byte packets of 64 samples, channel after channel) carries {predictor, step_index} per channel from
 * packet to packet; `state` is that carry: read on entry, written on success (AdpcmImaState::new() is all zeros), ignored (may be
 * NULL) for the other encodings.  The carry rule is QuickTime's: a packet whose header has the carried step index and
 * a predictor within 0x7f of the carried one continues from the carried predictor; any other packet restarts from its header.
 * len is a whole number of groups (SK_ERR_INVALID_ARG otherwise, or when out_cap is too small); *out_len receives the decoded size:
 * 2 bytes a sample for the 16-bit contracts, 3 for s24be, 4 for the 32-bit and float ones, 128 bytes per IMA4 packet.
 * SK_AIFF_DVD_S24 (DVD LPCM out of an MPEG program stream, no AIFF file holds it): len is a multiple of 12, a group of four samples;
 * 12 bytes of little-endian s24 leave per group, whatever the channel count.
 * The _dev form takes 16-byte aligned device pointers and is queued on the engine's stream; it waits only for the state. */
typedef struct sk_aiff_ima_state {
    int16_t predictor;
    uint8_t step_index; /* 0 ... 88 */
    uint8_t reserved;
} sk_aiff_ima_state;
int sk_aiff_decode(sk_engine *, int encoding, uint32_t channels, const uint8_t *bytes, size_t len, uint8_t *out, size_t out_cap, size_t *out_len,
                   sk_aiff_ima_state *state /*[2]*/);
int sk_aiff_decode_dev(sk_engine *, int encoding, uint32_t channels, const uint8_t *d_bytes, size_t len, uint8_t *d_out, size_t out_cap,
                       size_t *out_len, sk_aiff_ima_state *state /*[2]*/);

/* The tick of the AIFF streams: every unit (= the piece of one sk_aiff_reader_add, packed at a 16-byte aligned offset) is first
 * decoded to the contract's PCM on the device.  A stream with nothing further to change (no rate change, out_bits = the contract's,
 * out_channels = channels) gets those bytes as its outputs, one per unit, for up to 32 channels.  Every other stream then runs
 * exactly what sk_tick_run_pcm runs on a little-endian source of the contract's format -- same kernels, records, bounds and limits
 * (1 or 2 channels, up to SK_MAX_PCM_CHANNELS with sk_engine_enable_wide_pcm).  The fields are sk_pcm_tick_stream's, except that
 * `encoding` stands where `format` does, plus the IMA4 carry, which the call updates on success and leaves alone on failure.  The
 * units of a stream chain in order. */
typedef struct sk_aiff_tick_stream {
    uint32_t stream;      /* engine stream (resample = 1 only) */
    uint32_t n_units;
    uint8_t encoding;     /* enum sk_aiff_encoding */
    uint8_t channels;     /* 1 ... 32 */
    uint8_t out_bits;     /* 16 / 24 / 32 */
    uint8_t out_channels;
    uint8_t resample;
    uint8_t flush;
    uint8_t reserved[2];
    sk_aiff_ima_state ima_state[2];
} sk_aiff_tick_stream;
size_t sk_tick_aiff_out_bound_on(sk_engine *, const sk_aiff_tick_stream *streams, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units,
                                 uint32_t *max_outputs);
int sk_tick_run_aiff(sk_engine *, sk_aiff_tick_stream *streams, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units,
                     const uint8_t *bytes, size_t bytes_len, uint8_t *out_bytes, size_t out_cap, sk_tick_output *outputs, uint32_t outputs_cap,
                     uint32_t *n_outputs, size_t *out_bytes_used);

/* ---- Compressed WAV: the coded walker (host only) and the ADPCM decode stage (GPU) ----------------------------------- */
/* A decision beyond the reference, whose WavStreamProcessor (sk_wav_reader above, unchanged) takes format tags 1, 3 and 0xFFFE only.
 * sk_wav_coded_reader is the same RIFF / RF64 walk with the same budgets and texts that additionally takes
 *   6 / 7   A-law / mu-law (8 bits per sample; otherwise `WAV G.711 requires 8 bits per sample, found N`): pieces are whole frames of
 *           `channels` bytes, which sk_aiff_decode expands with SK_AIFF_ALAW / SK_AIFF_ULAW;
 *   0x11    IMA / DVI ADPCM: nBlockAlign a multiple of 4 x channels, (nBlockAlign - 4 x channels) x 2 / channels + 1 frames a block;
 *   2       Microsoft ADPCM: nBlockAlign >= 7 x channels, (nBlockAlign - 7 x channels) x 2 / channels + 2 frames a block, wNumCoef
 *           (1 ... 32) coefficient pairs read from the fmt extension -- the file's table, never an assumed one.
 * Both ADPCM tags: 4 bits per sample, 1 or 2 channels, at most 65 536 frames a block, a wSamplesPerBlock (cbSize >= 2) that agrees
 * with the block size; pieces are whole blocks, and a data chunk that ends inside one is `WAV data chunk is not block-aligned`.  A
 * `fact` chunk in front of `data` is kept: where its dwSampleLength is neither zero nor more than the blocks hold, it is the ADPCM
 * stream's total_frames, so the padding samples of the last block can be cut.  Tags 1 / 3 / 0xFFFE behave as in sk_wav_reader.
 * Not built: ADPCM with more than two channels (`WAV ADPCM with N channels is not built: mono and stereo are`); the coded tags inside
 * WAVE_FORMAT_EXTENSIBLE, GSM 6.10 (0x31), G.726 / G.722 tags, MPEG tags 0x50 / 0x55 -- each ends as `unsupported WAV format tag N`. */
enum sk_wav_tag { SK_WAV_TAG_PCM = 1, SK_WAV_TAG_MS_ADPCM = 2, SK_WAV_TAG_FLOAT = 3, SK_WAV_TAG_ALAW = 6, SK_WAV_TAG_ULAW = 7, SK_WAV_TAG_IMA_ADPCM = 0x11 };
typedef struct sk_wav_coded_info { /* zeros until the fmt chunk has been read */
    uint32_t tag;              /* enum sk_wav_tag (for WAVE_FORMAT_EXTENSIBLE: of the sub-format) */
    uint32_t sample_rate;
    uint32_t channels;
    uint32_t bits;             /* wBitsPerSample: 4 for the ADPCM tags, 8 for G.711 */
    uint32_t is_float;
    uint32_t block_align;      /* bytes of a piece's unit: an ADPCM block, else a frame */
    uint32_t frames_per_block; /* 1 unless ADPCM */
    uint32_t n_coef;           /* Microsoft ADPCM only */
    int16_t coef[32][2];       /* {iCoef1, iCoef2} */
    uint32_t fact_frames;      /* dwSampleLength as read, 0 without a fact chunk */
    uint32_t reserved;
    uint64_t total_frames;     /* of the data chunk as declared, cut by fact for ADPCM; 0 while unknown */
} sk_wav_coded_info;
typedef struct sk_wav_coded_reader sk_wav_coded_reader;
int sk_wav_coded_reader_create(sk_wav_coded_reader **out);
void sk_wav_coded_reader_destroy(sk_wav_coded_reader *);
/* sk_wav_reader_add's signature and piece contract */
int sk_wav_coded_reader_add(sk_wav_coded_reader *, const uint8_t *bytes, size_t len, uint64_t *piece_offset, size_t *piece_len, const uint8_t **piece);
int sk_wav_coded_reader_info(const sk_wav_coded_reader *, sk_wav_coded_info *info);
const char *sk_wav_coded_reader_last_error(const sk_wav_coded_reader *);

/* Whole blocks of tag SK_WAV_TAG_IMA_ADPCM or SK_WAV_TAG_MS_ADPCM on the GPU (csrc/wav_adpcm.hip: one block-channel per lane; neither
 * form carries state from block to block): len = n x block_align bytes in, n x frames_per_block x channels interleaved little-endian
 * s16 out (*out_len), and one status per block: SK_OK, or SK_WAV_BAD_BLOCK for a block its header rules out -- an IMA step index
 * above 88, an MS bPredictor >= n_coef -- whose output is zeros; the other blocks are not touched by it.
 *   IMA: per channel {predictor s16le = first sample, step index, reserved}, then groups of 4 bytes per channel, low nibble first.
 *   MS:  bPredictor, iDelta, iSamp1, iSamp2 (each for every channel); output iSamp2, iSamp1, then the nibbles, high first (stereo:
 *        high = left); pred = (samp1 x c1 + samp2 x c2) / 256 DIVIDED, truncating toward zero, as Microsoft's text and FFmpeg do and
 *        libsndfile's shift does not; delta = AdaptationTable[n] x delta / 256 kept within 16 ... INT_MAX / 768.
 * coef / n_coef: the fmt chunk's pairs (ignored for IMA).  SK_ERR_INVALID_ARG: another tag, a block size the walker would refuse, len
 * no whole number of blocks, out_cap too small.  The _dev form takes 16-byte aligned device pointers (status: 4-byte aligned, on the
 * device too) and is queued on the engine's stream; it waits only for its job record's upload. */
enum sk_wav_status { SK_WAV_BAD_BLOCK = -1201 };
int sk_wav_adpcm_decode(sk_engine *, int tag, uint32_t channels, uint32_t block_align, const int16_t *coef /*[n_coef][2]*/, uint32_t n_coef,
                        const uint8_t *bytes, size_t len, uint8_t *out, size_t out_cap, size_t *out_len, int32_t *status_per_block);
int sk_wav_adpcm_decode_dev(sk_engine *, int tag, uint32_t channels, uint32_t block_align, const int16_t *coef /*[n_coef][2], host*/, uint32_t n_coef,
                            const uint8_t *d_bytes, size_t len, uint8_t *d_out, size_t out_cap, size_t *out_len, int32_t *d_status_per_block);

/* The tick of the WAV ADPCM streams, sk_tick_run_aiff's twin: every unit (= whole blocks, the piece of one sk_wav_coded_reader_add,
 * packed at a 16-byte aligned offset) is first decoded to s16 on the device.  A stream with nothing further to change (no rate change,
 * out_bits = 16, out_channels = channels) gets those bytes as its outputs, one per unit.  Every other stream then runs exactly what
 * sk_tick_run_pcm runs on an SK_FMT_S16LE source -- same kernels, records, bounds and limits.  The fields are sk_pcm_tick_stream's, plus
 * the stream's description and frames_left, the `fact` cap: a unit's decoded frames are cut to it before anything downstream sees
 * them; the call decrements it on success and leaves it alone on failure; SK_WAV_NO_FRAME_CAP: no cap.  A stream whose cap is used
 * up brings no more units (SK_ERR_INVALID_ARG).  Neither block form carries state, so the output does not depend on how a stream's
 * blocks are split into units or dealt out over ticks.  status_per_unit[k]: 0, or 1 + the index of the unit's first block that its
 * header rules out; such a block decodes to zeros, its unit's record -- behind a conversion every record of its stream in this
 * tick -- has status SK_WAV_BAD_BLOCK, and the caller ends that stream; the other streams are not touched by it. */
#define SK_WAV_NO_FRAME_CAP 0xFFFFFFFFFFFFFFFFull
typedef struct sk_wav_adpcm_tick_stream {
    uint32_t stream;           /* engine stream (resample = 1 only) */
    uint32_t n_units;
    uint16_t tag;              /* SK_WAV_TAG_IMA_ADPCM / SK_WAV_TAG_MS_ADPCM */
    uint8_t channels;          /* 1 or 2 */
    uint8_t out_bits;          /* 16 / 24 / 32 */
    uint8_t out_channels;
    uint8_t resample;
    uint8_t flush;
    uint8_t n_coef;            /* Microsoft ADPCM: 1 ... 32 */
    uint32_t block_align;
    uint32_t frames_per_block; /* 0, or what block_align gives */
    uint64_t frames_left;      /* in: decoded frames the stream may still give; out: less what this tick gave */
    int16_t coef[32][2];
} sk_wav_adpcm_tick_stream;
size_t sk_tick_wav_adpcm_out_bound_on(sk_engine *, const sk_wav_adpcm_tick_stream *streams, uint32_t n_streams, const sk_pcm_unit *units,
                                      uint32_t n_units, uint32_t *max_outputs);
int sk_tick_run_wav_adpcm(sk_engine *, sk_wav_adpcm_tick_stream *streams, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units,
                          const uint8_t *bytes, size_t bytes_len, uint8_t *out_bytes, size_t out_cap, sk_tick_output *outputs, uint32_t outputs_cap,
                          uint32_t *n_outputs, size_t *out_bytes_used, int32_t *status_per_unit);

/* ---- FLAC (RFC 9639): header parser, framer, stream reader (host only) ----------------------------------------------- */
/* Native FLAC streams (`fLaC`).  Not built: Ogg FLAC, FLAC in MP4, decode_f32, 32-bit frames with a side channel (33-bit samples:
 * SK_ERR_UNSUPPORTED as that frame's status), MD5 / total-sample verification at the end of a stream. */
enum sk_flac_status {
    SK_FLAC_NEED_MORE = -501,       /* the header is longer than the bytes given */
    SK_FLAC_NO_SYNC = -502,         /* the bytes do not begin with 0xFFF8 / 0xFFF9 */
    SK_FLAC_RESERVED = -503,        /* a reserved value: block-size code 0, rate code 15, depth code 3, assignment 11 ... 15, a set
                                     * reserved bit, an invalid coded number */
    SK_FLAC_BAD_CRC = -504,         /* the header's CRC-8 fails; sk_flac_scan: no span within the frame bound satisfies the CRC-16 */
    SK_FLAC_NEED_STREAMINFO = -505, /* rate code 0 or depth code 0 and no STREAMINFO was given */
    SK_FLAC_INVALID = -506,         /* a frame's status from the device stage: the subframes break the syntax or miss the frame's end */
    SK_FLAC_ERR_STREAM = -507       /* the reader / decoder rejected the stream; *_last_error has the text */
};
typedef struct sk_flac_streaminfo { /* the STREAMINFO block, RFC 9639 8.2 */
    uint32_t min_blocksize, max_blocksize, min_framesize, max_framesize; /* frame sizes: 0 = unknown */
    uint32_t sample_rate;
    uint8_t channels, bits_per_sample;
    uint16_t reserved;
    uint64_t total_samples; /* 0 = unknown */
    uint8_t md5[16];        /* of the unencoded samples; all zeros = not computed.  Reported, never checked. */
} sk_flac_streaminfo;
typedef struct sk_flac_frame_info {
    uint64_t number;         /* the coded number: the frame's (fixed block size) or its first sample's (variable) */
    uint32_t offset;         /* sk_flac_scan / reader: position of the frame in the scanned bytes */
    uint32_t frame_bytes;    /* sync code to the end of the CRC-16; 0 from sk_flac_parse_header */
    uint32_t sample_rate;
    uint32_t block_size;     /* 1 ... 65536 samples per channel */
    uint8_t header_bytes;    /* 6 ... 16, CRC-8 included */
    uint8_t channels;        /* 1 ... 8 */
    uint8_t assignment;      /* 0 ... 7 independent channels; 8 left/side, 9 side/right, 10 mid/side */
    uint8_t bits_per_sample; /* 4 ... 32 */
    uint8_t variable_blocksize;
    uint8_t reserved[3];
} sk_flac_frame_info;
/* One frame header, RFC 9639 9.1: sync, blocking strategy, the coded number (up to 36 bits), every block-size code (6 / 7 with their
 * tail bytes), every rate code (12 / 13 / 14 with theirs; 0 = STREAMINFO's), depth codes 0 (= STREAMINFO's), 8, 12, 16, 20, 24, 32,
 * assignments 0 ... 10, CRC-8.  `info` may be NULL: a header that needs it is SK_FLAC_NEED_STREAMINFO then. */
int sk_flac_parse_header(const uint8_t *data, size_t len, const sk_flac_streaminfo *info, sk_flac_frame_info *out);
/* Whole frames out of bytes that begin at a frame; stateless.  A frame ends where the next valid header (sync, parse, CRC-8) begins AND
 * the CRC-16 of the span holds, or -- with `final` != 0 -- at the end of the data if the CRC-16 holds there.  A sync pattern inside a
 * frame, even one with a valid CRC-8, is no boundary: the scan goes on.  The search is bounded: by STREAMINFO's max_framesize when it
 * has one, else by 19 + ceil((block_size * channels * (bits + 1) + channels * 40) / 8) bytes (header 16, CRC-16 2, padding 1; every
 * subframe VERBATIM at a side channel's width, with its header byte and the longest wasted-bits count).  No span within the bound:
 * SK_FLAC_BAD_CRC -- FLAC is lossless, a lost frame is not skipped.  Bytes that are no header where a frame must begin: that header's
 * status.  *consumed = bytes up to the first incomplete frame; frames beyond `cap` stay unconsumed. */
int sk_flac_scan(const uint8_t *data, size_t len, const sk_flac_streaminfo *info, int final, sk_flac_frame_info *frames, uint32_t cap,
                 uint32_t *n_frames, size_t *consumed);
/* A stream from its `fLaC` marker on, cut anywhere: the marker, the metadata blocks (STREAMINFO first, exactly 34 bytes; PADDING,
 * APPLICATION, SEEKTABLE, VORBIS_COMMENT, CUESHEET and PICTURE are skipped by count without being buffered; type 127 and a second
 * STREAMINFO are rejected), then whole frames through sk_flac_scan.  One `add` gives at most `cap` frames -- the others come with the
 * next one -- at *data + frames[i].offset, valid until the next call on the reader.  An EMPTY add is the finalising one: the last
 * frame ends with the data, and bytes that form no frame are a truncated stream.  A frame whose channel count, depth or rate
 * disagrees with STREAMINFO ends the stream.  SK_FLAC_ERR_STREAM: rejected, sk_flac_reader_last_error has the text; it stays so. */
typedef struct sk_flac_info { /* zeros (but buffered_bytes) until STREAMINFO has been read */
    sk_flac_streaminfo streaminfo;
    uint64_t frames;         /* frames handed out so far */
    uint32_t buffered_bytes; /* held back: an incomplete marker / block header / STREAMINFO / frame */
    uint8_t have_streaminfo;
    uint8_t reserved[3];
} sk_flac_info;
typedef struct sk_flac_reader sk_flac_reader;
int sk_flac_reader_create(sk_flac_reader **out);
void sk_flac_reader_destroy(sk_flac_reader *);
int sk_flac_reader_add(sk_flac_reader *, const uint8_t *bytes, size_t len, sk_flac_frame_info *frames, uint32_t cap, uint32_t *n_frames,
                       const uint8_t **data);
int sk_flac_reader_info(const sk_flac_reader *, sk_flac_info *info);
const char *sk_flac_reader_last_error(const sk_flac_reader *);

/* ---- FLAC decode stage (GPU, csrc/flac_decode.hip) ------------------------------------------------------------------- */
/* frames[i] lies at bytes + frames[i].offset (frame_bytes long, as sk_flac_scan gives them).  Output: the frames one after the other in
 * the order given, each block_size x channels samples interleaved, little-endian, in the width of its depth: <= 8 bits one byte
 * (sample + 128), 9 ... 16 two, 17 ... 24 three, 32 four.  status_per_frame[i]: SK_OK, SK_FLAC_INVALID (a reserved subframe type, a set
 * padding bit, a partition order the block size does not divide by or whose first partition is shorter than the predictor order, a
 * negative LPC shift, precision code 15, samples that end beyond the frame's bytes before its CRC or more than 7 bits short of it,
 * assignment 8 ... 10 with other than 2 channels) or SK_ERR_UNSUPPORTED (32 bits with a side channel).  A rejected frame keeps its
 * place in `out` and nothing is written there.  out_cap too small, or a frame_info outside 1 ... 8 channels / 4 ... 32 bits / 1 ... 65536
 * samples: SK_ERR_INVALID_ARG, nothing decoded.  The CRC-16 is the framer's business and is not checked again.
 * The _dev form takes 16-byte aligned device pointers and runs on the engine's stream; it waits only for the statuses. */
int sk_flac_decode_frames(sk_engine *, const sk_flac_frame_info *frames, uint32_t n, const uint8_t *bytes, uint8_t *out, size_t out_cap,
                          size_t *out_len, int32_t *status_per_frame);
int sk_flac_decode_frames_dev(sk_engine *, const sk_flac_frame_info *frames, uint32_t n, const uint8_t *d_bytes, uint8_t *d_out, size_t out_cap,
                              size_t *out_len, int32_t *status_per_frame);

/* The tick of the FLAC streams, sk_tick_run_aiff's pattern: the units are whole frames (as sk_flac_scan / the reader cut them, packed at
 * 16-byte aligned offsets: frames[k].offset into `bytes`, stream after stream), and every frame is first decoded to the contract's PCM
 * on the device.  A stream with nothing to change (no rate change, out_bits = the contract's width in bits, out_channels = channels)
 * gets those bytes as its outputs, one per frame, at any depth and for 1 ... 8 channels.  Every other stream then runs exactly what
 * sk_tick_run_pcm runs on a little-endian source of that format -- same kernels, records, bounds and limits (16 / 24 / 32-bit samples,
 * the exact 24 / 32 -> 16 path included; 3 ... 8 channels need sk_engine_enable_wide_pcm); any other depth with a conversion requested:
 * SK_ERR_UNSUPPORTED.  A refused tick leaves every stream as it was.  status_per_frame[k] is sk_flac_decode_frames': a rejected frame
 * writes nothing; its output record carries the status, and behind a conversion -- where the frame went in as silence -- every record
 * of its stream in this tick does: the stream is to be ended. */
typedef struct sk_flac_tick_stream {
    uint32_t stream;         /* engine stream (resample = 1 only) */
    uint32_t n_units;        /* frames */
    uint8_t channels;        /* 1 ... 8 */
    uint8_t bits_per_sample; /* 4 ... 32 */
    uint8_t out_bits;        /* 8 (as decoded, depth <= 8) / 16 / 24 / 32 */
    uint8_t out_channels;
    uint8_t resample;
    uint8_t flush;
    uint8_t reserved[2];
} sk_flac_tick_stream;
size_t sk_tick_flac_out_bound_on(sk_engine *, const sk_flac_tick_stream *streams, uint32_t n_streams, const sk_flac_frame_info *frames,
                                 uint32_t n_frames, uint32_t *max_outputs);
int sk_tick_run_flac(sk_engine *, const sk_flac_tick_stream *streams, uint32_t n_streams, const sk_flac_frame_info *frames, uint32_t n_frames,
                     const uint8_t *bytes, size_t bytes_len, uint8_t *out_bytes, size_t out_cap, sk_tick_output *outputs, uint32_t outputs_cap,
                     uint32_t *n_outputs, size_t *out_bytes_used, int32_t *status_per_frame);

/* FlacDecoder (soundkit-flac/src/lib.rs:122-219): bytes in at any chunking, interleaved samples out.  One call buffers its input and
 * decodes every whole frame available that fits into out_cap (SK_ERR_CAPACITY when not even the next one does); *written counts
 * interleaved samples.  A call with len = 0 fetches frames an earlier call had no room for -- in the middle of a stream as well, more
 * input may follow -- and, once none waits, is the finalising one: 0 written = nothing is left.  decode_i16 is
 * decode_i32 CLAMPED to the i16 range (lib.rs:192-193), not shifted.  A frame the device rejects or a stream the framer rejects:
 * SK_FLAC_ERR_STREAM with a text (the reference returns Err(String)); the decoder stays in error until reset. */
typedef struct sk_flac_decoder sk_flac_decoder;
int sk_flac_decoder_create(sk_engine *, sk_flac_decoder **out);
void sk_flac_decoder_destroy(sk_flac_decoder *);
int sk_flac_decoder_reset(sk_flac_decoder *);
/* sample_rate / channels / bits_per_sample are 0 until STREAMINFO has been read (Option::None) */
int sk_flac_decoder_info(const sk_flac_decoder *, uint32_t *sample_rate, uint8_t *channels, uint8_t *bits_per_sample, uint64_t *frames_decoded);
/* FlacDecoder::pending_samples (lib.rs:175): interleaved samples of the frames that wait for room.  While it is not 0 a call with
 * len = 0 only fetches them; at 0 such a call finalises the stream. */
size_t sk_flac_decoder_pending_samples(const sk_flac_decoder *);
int sk_flac_decoder_decode_i32(sk_flac_decoder *, const uint8_t *input, size_t len, int32_t *out, size_t out_cap, size_t *written);
int sk_flac_decoder_decode_i16(sk_flac_decoder *, const uint8_t *input, size_t len, int16_t *out, size_t out_cap, size_t *written);
const char *sk_flac_decoder_last_error(const sk_flac_decoder *);

/* ---- Apple Lossless (ALAC): cookie, packet header, CAF packet index (host only, csrc/alac_stream.h) ----------------------- */
/* ALAC arrives as packets that a container (CAF, MP4) has already cut, with the ALACSpecificConfig as its magic cookie.  The MP4 side
 * of the container is sk_mp4_* below: its demuxer and index hand packets and cookie to the same calls. */
enum sk_alac_status {
    SK_ALAC_INVALID = -601,     /* a packet breaks the syntax: a prediction type other than 0 / 15, a zero run past the element's end, a
                                   frame count of 0 or above the cookie's, elements whose counts differ, more or fewer channels than the
                                   cookie's, bits that end beyond the packet or 8 and more bits short of it */
    SK_ALAC_ERR_STREAM = -602,  /* a cookie, a CAF file or a packet was rejected with a text */
    SK_ALAC_UNSUPPORTED = -603  /* a CCE or PCE element (tags 2 and 5) */
};
typedef struct sk_alac_config { /* the 24-byte big-endian ALACSpecificConfig */
    uint32_t frame_length;      /* 1 ... 65536 */
    uint32_t sample_rate;       /* > 0 */
    uint32_t max_frame_bytes, avg_bit_rate;
    uint16_t max_run;
    uint8_t compatible_version;
    uint8_t bit_depth;          /* 16, 24 or 32 */
    uint8_t pb, mb, kb;         /* history multiplier, initial history, Rice limit */
    uint8_t channels;           /* 1 ... 8 */
} sk_alac_config;
/* The bare config, the MP4 `alac` FullBox payload (four zero bytes, then the config) or the QuickTime form (a 12-byte `frma` atom, then an
 * `alac` atom).  Refused with SK_ALAC_ERR_STREAM and a text in `error` (NUL-terminated, cut to error_cap; may be NULL): fewer than 24
 * bytes of config, rate 0, channels outside 1 ... 8, a depth other than 16 / 24 / 32, frame_length outside 1 ... 65536. */
int sk_alac_parse_cookie(const uint8_t *cookie, size_t len, sk_alac_config *out, char *error, size_t error_cap);
/* The frame count of a packet as its first audio element states it (DSE and FIL in front are stepped over): the size field, or
 * frame_length without one.  SK_ALAC_INVALID: no audio element, a count of 0 or above frame_length, a header beyond the packet;
 * SK_ALAC_UNSUPPORTED: a CCE or PCE comes first. */
int sk_alac_packet_frames(const sk_alac_config *, const uint8_t *packet, size_t len, uint32_t *frames);

/* CafAlacPacketIndex (soundkit-alac/src/lib.rs:38-215): `desc` (exactly 32 bytes, format `alac`), the cookie, the `pakt` table (24 bytes
 * of counts, then one big-endian base-128 size of at most 10 bytes per packet, nothing behind them; not read when desc gives a constant
 * bytes-per-packet) and where the `data` chunk's payload lies (its first 4 bytes are the edit count).  desc and cookie must agree on
 * rate, channels and -- where desc states one -- depth; the sizes must add up to the payload; no packet is empty or above 16 MiB.
 * A refusal is SK_ALAC_ERR_STREAM with its text in `error`. */
typedef struct sk_caf_alac_index sk_caf_alac_index;
typedef struct sk_caf_alac_info {
    sk_alac_config config;
    uint64_t valid_frames;
    uint32_t priming_frames, remainder_frames;
    uint32_t frames_per_packet; /* desc's: packet k begins at frame k * frames_per_packet of the timeline that priming / valid trim */
    uint32_t n_packets;
} sk_caf_alac_info;
int sk_caf_alac_index_create(const uint8_t *desc, size_t desc_len, const uint8_t *cookie, size_t cookie_len, const uint8_t *pakt, size_t pakt_len,
                             uint64_t data_offset, uint64_t data_size, sk_caf_alac_index **out, char *error, size_t error_cap);
/* the same from a whole CAF file: finds desc, kuki, pakt and data (a data chunk of size -1 runs to the end of the file) */
int sk_caf_alac_index_from_file(const uint8_t *file, size_t len, sk_caf_alac_index **out, char *error, size_t error_cap);
void sk_caf_alac_index_destroy(sk_caf_alac_index *);
int sk_caf_alac_index_info(const sk_caf_alac_index *, sk_caf_alac_info *info);
/* the packets' absolute offsets and sizes; cap < n_packets: SK_ERR_CAPACITY */
int sk_caf_alac_index_packets(const sk_caf_alac_index *, uint64_t *offsets, uint32_t *sizes, uint32_t cap);

/* ---- CAF, `lpcm` and `alac` (host, csrc/caf_stream.h) -----------------------------------------------------------------------------------
 * CafAudioIndex (soundkit-audio-demux/src/caf.rs) with its checks and texts: the chunk walk of a whole file (`caff`, version 1, flags 0;
 * desc, kuki, pakt, chan and data at most once; -1 as the size of the data chunk alone; budgets of 32 bytes, 1 MiB, 64 MiB and 1 MiB on
 * desc, kuki, pakt and chan), the description, the packet table, and the packets of the data chunk.  sk_caf_alac_index_* above stays
 * as it was.  A refusal is SK_CAF_ERR_STREAM with a text in `error` (NUL-terminated, cut to error_cap; may be NULL).
 * `lpcm`: flag bit 0 is float, bit 1 little-endian; `CAF LPCM bits per channel is zero`, `CAF float PCM must use 32-bit or 64-bit
 * samples`, `CAF LPCM requires a constant packet size`, `CAF LPCM packet geometry is not frame-aligned`, `CAF LPCM bytes per frame cannot
 * hold its channels`; any other format but `alac`: `unsupported CAF audio format NAME`.  Two things are this library's own: a frame padded
 * beyond channels x ceil(bits / 8) bytes is refused (`CAF LPCM frames padded beyond their channels are unsupported`; the reference marks
 * it unpacked and then reads it as packed), and an `lpcm` file's packets -- one frame each in common files -- are handed out as runs of
 * whole packets of at most 4096 frames and 1 MiB, so the packet budget of 8 000 000 counts runs.  An `alac` file's packets are the file's. */
enum sk_caf_status { SK_CAF_ERR_STREAM = -1301 };
enum sk_caf_codec { SK_CAF_CODEC_ALAC = 1, SK_CAF_CODEC_PCM = 2 };
typedef struct sk_caf_info {
    uint32_t codec;             /* sk_caf_codec */
    char format_id[4];          /* the description's mFormatID (no NUL) */
    uint32_t sample_rate, channels;
    uint32_t bits_per_sample;   /* 0: the description states none (alac may) */
    uint32_t format_flags;
    uint32_t big_endian, is_float, bytes_per_frame; /* lpcm; zeros for alac */
    uint32_t frames_per_packet; /* the description's: of a packet of the file, not of a run */
    uint32_t priming_frames, remainder_frames;
    uint32_t n_packets;         /* alac: the file's packets; lpcm: runs */
    uint32_t cookie_len;        /* bytes of the kuki chunk */
    uint64_t valid_frames;
} sk_caf_info;
typedef struct sk_caf_index sk_caf_index;
int sk_caf_index_from_file(const uint8_t *file, size_t len, sk_caf_index **out, char *error, size_t error_cap);
/* CafAudioIndex::from_metadata: the chunks' payloads as a caller with a seekable source read them; pakt NULL: the file holds none;
 * data_offset points at the data chunk's four-byte edit count */
int sk_caf_index_create(const uint8_t *desc, size_t desc_len, const uint8_t *cookie, size_t cookie_len, const uint8_t *pakt, size_t pakt_len,
                        uint64_t data_offset, uint64_t data_size, sk_caf_index **out, char *error, size_t error_cap);
void sk_caf_index_destroy(sk_caf_index *);
/* cookie may be NULL when cookie_cap is 0; cookie_cap < cookie_len: SK_ERR_CAPACITY (info is filled) */
int sk_caf_index_info(const sk_caf_index *, sk_caf_info *info, uint8_t *cookie, size_t cookie_cap);
/* per packet (or run): absolute offset, size, frames and the first frame's place on the file's timeline (what pcm_packet_trim counts
 * from); any array may be NULL; cap < n_packets: SK_ERR_CAPACITY */
int sk_caf_index_packets(const sk_caf_index *, uint64_t *offsets, uint32_t *sizes, uint32_t *frames, uint64_t *start_frames, uint32_t cap);

/* ---- MP4 / M4A / fragmented MP4, audio only (host, csrc/mp4_stream.h) -------------------------------------------------------------
 * The first audio track whose sample entry is `mp4a` (AAC), `alac`, `fLaC` or a PCM entry (`sowt twos in24 in32 fl32 fl64 lpcm`) is
 * chosen; video tracks and unknown boxes are stepped over by size without being buffered.  Read: 32- and 64-bit box sizes, mvhd, tkhd, edts/elst (the first media edit), mdhd, hdlr, stsd with
 * esds (descriptor tags 3, 4, 5, lengths of 1 to 4 bytes) or the `alac` child, stts, stsc, stsz (both forms), stco / co64; mvex/trex,
 * moof/traf with tfhd (base-data-offset, default-base-is-moof, default duration and size), tfdt and trun under any flag combination,
 * several traf per moof.  The layout is fragmented when moov holds mvex or its sample tables are empty.  Budgets: 4 MiB a call, 64 MiB
 * of moov or moof payload (refused from the box header), 128 MiB a sample, 8 000 000 samples a track or fragment.
 * A refusal is SK_MP4_ERR_STREAM with a text (sk_mp4_demuxer_last_error, or `error`: NUL-terminated, cut to error_cap; may be NULL).
 * Sound descriptions of version 0, 1 and 2 are read (`unsupported QuickTime audio sample-entry version N` otherwise); `enda` and `dfLa`
 * are looked for in the entry and inside `wave` / `sinf` / `schi`.  `sowt` is little-endian and `twos` big-endian at the declared width;
 * `in24 in32 fl32 fl64` are 24, 32, 32 and 64 bits, big-endian unless `enda` is 1 (`invalid QuickTime enda flag N` for any value but 0
 * and 1); `lpcm` needs version two (`QuickTime lpcm requires a version-two sample entry`) and takes its flags: bit 0 float, bit 1
 * big-endian; `non-interleaved QuickTime LPCM is unsupported` (bit 5), and for an integer entry `unsigned QuickTime LPCM is unsupported`
 * (bit 2 clear), `unpacked QuickTime LPCM is unsupported` (bit 3 clear), `aligned-high QuickTime LPCM is unsupported` (bit 4).
 * A PCM track's samples are single frames; what the index and the demuxer hand out are the same runs of frames: of a constant stsz with
 * one stts entry, per chunk at most 4096 frames and 1 MiB a run (no record per frame is made); otherwise neighbours merge while they
 * are contiguous in bytes and in time, up to the same two limits.  A `fLaC` track's codec-private data is `fLaC` followed by the
 * metadata blocks: from data that already begins so, a bare 34-byte STREAMINFO, or a `dfLa` payload (`MP4 dfLa decoder configuration
 * is truncated`, `MP4 dfLa has no leading FLAC STREAMINFO block`, `MP4 dfLa has an invalid FLAC STREAMINFO block`: refused where the
 * entry is read, so the index and the demuxer's config event fail alike and such a file gives no sample table).
 * Not read: ctts, stss, edits behind the first media edit, the `ulaw` / `alaw` / `ima4` / `raw ` entries, `chan`, video; `fLaC` and PCM
 * tracks of a fragmented file are described but not decoded by anything above this layer. */
enum sk_mp4_status { SK_MP4_ERR_STREAM = -901 };
enum sk_mp4_codec { SK_MP4_CODEC_AAC = 1, SK_MP4_CODEC_ALAC = 2, SK_MP4_CODEC_FLAC = 3, SK_MP4_CODEC_PCM = 4 };
typedef struct sk_mp4_track_info {
    uint32_t codec;        /* sk_mp4_codec; 0: no config yet (sk_mp4_demuxer_config before moov has arrived) */
    uint32_t sample_rate;  /* AAC: the AudioSpecificConfig's where its two-byte form states one, else the sample entry's */
    uint32_t channels;
    uint32_t bits_per_sample; /* the sample entry's; 0 for AAC */
    uint32_t track_id;
    uint32_t timescale;    /* of the track: what packet times and the edit are counted in */
    uint32_t sample_count; /* of the sample table; 0 in a fragmented file */
    uint32_t fragmented;
    uint32_t has_edit;     /* the first media edit of edts/elst, in the track's timescale (the duration rescaled from the movie's) */
    uint32_t private_len;  /* bytes of codec-private data: the AudioSpecificConfig, the `alac` child's payload (sk_alac_parse_cookie takes
                              it), or for FLAC `fLaC` + the metadata blocks (what the FLAC decoder is fed before the packets); 0 for PCM */
    uint64_t edit_presentation_start, edit_media_start, edit_duration;
} sk_mp4_track_info;
/* what a SK_MP4_CODEC_PCM track's bytes are: signed integers or IEEE floats, packed, interleaved.  All zero for any other codec. */
typedef struct sk_mp4_pcm_info {
    char codec_id[4];           /* the sample entry's name: `sowt`, `twos`, `in24`, `in32`, `fl32`, `fl64`, `lpcm` (no NUL) */
    uint32_t big_endian;        /* 1: big-endian, 0: little-endian */
    uint32_t is_float;
    uint32_t bits_per_sample;   /* = sk_mp4_track_info.bits_per_sample; 0: the entry states none */
    uint32_t bytes_per_frame;   /* the entry's (version one and two), else channels x ceil(bits / 8); 0: unknown */
    uint32_t frames_per_packet; /* the entry's: 1 for version zero; 0: not stated */
} sk_mp4_pcm_info;

/* The streaming demuxer: moov must come before mdat -- `MP4 mdat appears before moov; use the seekable MP4 packet API` otherwise, from
 * the mdat header alone.  Events: one config (once moov has been parsed), then the track's samples in file order as their bytes arrive.
 * A regular file's buffer is drained up to the next sample's offset; a fragmented file's samples follow their moof's trun tables.
 * _finish: `truncated MP4 box header`, `truncated MP4 box NAME`, `truncated MP4 top-level box` for what the input ended in. */
typedef struct sk_mp4_demuxer sk_mp4_demuxer;
int sk_mp4_demuxer_create(sk_mp4_demuxer **out);
void sk_mp4_demuxer_destroy(sk_mp4_demuxer *);
int sk_mp4_demuxer_add(sk_mp4_demuxer *, const uint8_t *bytes, size_t len);
int sk_mp4_demuxer_finish(sk_mp4_demuxer *);
const char *sk_mp4_demuxer_last_error(const sk_mp4_demuxer *);
/* the config event; codec_private may be NULL when private_cap is 0; private_cap < private_len: SK_ERR_CAPACITY (info is filled) */
int sk_mp4_demuxer_config(const sk_mp4_demuxer *, sk_mp4_track_info *info, uint8_t *codec_private, size_t private_cap);
/* the PCM description of the config event (zeros before moov has arrived and for a track that is not PCM) */
int sk_mp4_demuxer_pcm_info(const sk_mp4_demuxer *, sk_mp4_pcm_info *info);
/* packets waiting, the first one's size and the bytes the demuxer holds that are no packet yet */
int sk_mp4_demuxer_pending(const sk_mp4_demuxer *, uint32_t *n_packets, size_t *front_bytes, size_t *buffered_bytes);
/* takes the first waiting packet: its raw bytes, decode time and duration in the track's timescale.  None waiting: SK_ERR_BAD_STREAM;
 * cap too small: SK_ERR_CAPACITY, the packet stays */
int sk_mp4_demuxer_take(sk_mp4_demuxer *, uint8_t *out, size_t cap, size_t *len, uint64_t *start_time, uint32_t *duration);
/* sk_mp4_index_trim for a packet the demuxer gave (a fragmented file has no index): its times as sk_mp4_demuxer_take returned them */
int sk_mp4_demuxer_trim(const sk_mp4_demuxer *, uint64_t start_time, uint32_t duration, uint32_t decoded_frames, uint32_t decoded_rate, uint32_t *first,
                        uint32_t *count, char *error, size_t error_cap);

/* Mp4MediaIndex::from_file for the chosen track: moov anywhere in the file; every sample's byte range is checked against the file.  A
 * fragmented file gives its track and no samples (its packets come from the demuxer). */
typedef struct sk_mp4_index sk_mp4_index;
int sk_mp4_index_from_file(const uint8_t *file, size_t len, sk_mp4_index **out, char *error, size_t error_cap);
void sk_mp4_index_destroy(sk_mp4_index *);
int sk_mp4_index_info(const sk_mp4_index *, sk_mp4_track_info *info, uint8_t *codec_private, size_t private_cap);
int sk_mp4_index_pcm_info(const sk_mp4_index *, sk_mp4_pcm_info *info);
/* per sample: absolute offset, size, duration and decode time; any array may be NULL; cap < sample_count: SK_ERR_CAPACITY */
int sk_mp4_index_samples(const sk_mp4_index *, uint64_t *offsets, uint32_t *sizes, uint32_t *durations, uint64_t *start_times, uint32_t cap);
/* resolve_pcm_packet_trim: the frames of sample `sample`'s decoded packet (decoded_frames at decoded_rate) that the edit keeps.  The
 * start rounds up, the end down, both are clamped to decoded_frames; nothing kept: (decoded_frames, 0); no edit list: (0, decoded_frames) */
int sk_mp4_index_trim(const sk_mp4_index *, uint32_t sample, uint32_t decoded_frames, uint32_t decoded_rate, uint32_t *first, uint32_t *count,
                      char *error, size_t error_cap);
/* normalize_mp4_flac_decoder_configuration on its own: *out_len is what the result needs; out_cap smaller: SK_ERR_CAPACITY */
int sk_mp4_flac_config(const uint8_t *data, size_t len, uint8_t *out, size_t out_cap, size_t *out_len, char *error, size_t error_cap);
/* create_adts_header: the seven bytes in front of a raw AAC sample (profile from the config's object type, no CRC) */
int sk_mp4_adts_header(const uint8_t *asc, size_t asc_len, uint32_t sample_rate, uint32_t channels, size_t raw_len, uint8_t out[7]);

/* ---- WebM / Matroska, audio only (host, csrc/webm_stream.h) -------------------------------------------------------------------------
 * The streaming EBML walk of soundkit-webm's WebmAudioDemuxer with its checks, texts and budgets: the EBML header (read version, id and
 * size widths, DocType `webm` / `matroska`), a Segment of known or unknown size, Info / TimecodeScale, Tracks / TrackEntry (TrackNumber,
 * TrackType, CodecID, CodecPrivate, DefaultDuration, CodecDelay, SeekPreRoll, TrackTimestampScale, ContentEncodings -- header stripping
 * alone -- and Audio's SamplingFrequency and Channels), then Clusters of known or unknown size with Timecode, SimpleBlock, Block and
 * BlockGroup (BlockDuration, ReferenceBlock, DiscardPadding), all four lacings.  Everything else is stepped over by its size.  Reported:
 * the audio tracks whose CodecID is A_VORBIS, A_AAC, A_FLAC, A_ALAC or A_OPUS (of a repeated TrackNumber the first entry), once the first
 * Cluster header has arrived; blocks of other tracks are dropped.  Budgets: 4 MiB a call, 16 MiB a metadata element, 64 MiB a block
 * element (both from the element's header), 64 MiB + 64 KiB buffered.  A refusal is SK_WEBM_ERR_STREAM with a text
 * (sk_webm_demuxer_last_error, or `error`: NUL-terminated, cut to error_cap; may be NULL); the demuxer stays refused.
 * Not read: Cues / seeking, chained segments, EBML CRC-32, any other ContentCompression, encryption, the old A_AAC/MPEG4/... ids, video. */
enum sk_webm_status { SK_WEBM_ERR_STREAM = -1001 };
enum sk_webm_codec { SK_WEBM_CODEC_VORBIS = 1, SK_WEBM_CODEC_AAC = 2, SK_WEBM_CODEC_FLAC = 3, SK_WEBM_CODEC_ALAC = 4, SK_WEBM_CODEC_OPUS = 5 };
typedef struct sk_webm_track_info {
    uint64_t track_number;
    uint64_t codec_delay_ns, seek_pre_roll_ns;
    uint64_t default_duration_ns; /* 0: none */
    uint64_t timecode_scale_ns;   /* the Segment's: Info / TimecodeScale, 1 000 000 without one */
    double track_timestamp_scale;
    uint32_t codec;               /* sk_webm_codec */
    uint32_t sample_rate;         /* Audio / SamplingFrequency rounded; 48 000 without one */
    uint32_t channels;            /* 2 without one */
    uint32_t private_len;         /* bytes of CodecPrivate */
    uint32_t prefix_len;          /* bytes header stripping took off every frame (the demuxer has put them back) */
    uint32_t reserved;
} sk_webm_track_info;
typedef struct sk_webm_demuxer sk_webm_demuxer;
int sk_webm_demuxer_create(sk_webm_demuxer **out);
void sk_webm_demuxer_destroy(sk_webm_demuxer *);
int sk_webm_demuxer_add(sk_webm_demuxer *, const uint8_t *bytes, size_t len);
/* `truncated WebM element: N buffered bytes remain`, then `WebM source has no supported audio track` */
int sk_webm_demuxer_finish(sk_webm_demuxer *);
const char *sk_webm_demuxer_last_error(const sk_webm_demuxer *);
/* the config events: 0 tracks before the first Cluster header */
uint32_t sk_webm_demuxer_n_tracks(const sk_webm_demuxer *);
/* track `index` of them; either byte array may be NULL with a cap of 0; a cap below its length: SK_ERR_CAPACITY (info is filled) */
int sk_webm_demuxer_config(const sk_webm_demuxer *, uint32_t index, sk_webm_track_info *info, uint8_t *codec_private, size_t private_cap,
                           uint8_t *prefix, size_t prefix_cap);
/* packets waiting, the first one's size and the bytes the demuxer holds that are no packet yet */
int sk_webm_demuxer_pending(const sk_webm_demuxer *, uint32_t *n_packets, size_t *front_bytes, size_t *buffered_bytes);
typedef struct sk_webm_packet_info {
    uint64_t track_number;
    int64_t timestamp_ns;       /* (cluster + relative timecode) x TimecodeScale x TrackTimestampScale, rounded, minus CodecDelay; laced frames advance by their durations */
    uint64_t duration_ns;       /* BlockDuration / frames of the block, else DefaultDuration, else (Opus) the packet's own */
    int64_t discard_padding_ns; /* on the block's last frame: negative trims the decoded front, positive the back */
    uint32_t codec;             /* sk_webm_codec */
    uint8_t has_duration, has_discard_padding;
    uint8_t reserved[2];
} sk_webm_packet_info;
/* takes the first waiting packet.  None waiting: SK_ERR_BAD_STREAM; cap too small: SK_ERR_CAPACITY, the packet stays */
int sk_webm_demuxer_take(sk_webm_demuxer *, uint8_t *out, size_t cap, size_t *len, sk_webm_packet_info *info);
/* parse_vorbis_codec_private: an A_VORBIS CodecPrivate -> its three headers as offsets into it and sizes */
int sk_webm_vorbis_headers(const uint8_t *codec_private, size_t len, size_t offsets[3], size_t sizes[3], char *error, size_t error_cap);
/* discard_padding_frames: ceil(|padding_ns| x sample_rate / 1e9) capped at decoded_frames, off the front (negative) or the back */
int sk_webm_discard_frames(int64_t padding_ns, uint32_t sample_rate, uint32_t decoded_frames, uint32_t *front, uint32_t *back, char *error,
                           size_t error_cap);

/* ---- MPEG transport stream, audio only (host, csrc/ts_stream.h) ---------------------------------------------------------------------
 * The incremental walk of soundkit-audio-demux's MpegTsAudioDemuxer with its checks, texts and budgets: packets at stride 188, at 192
 * behind a 4-byte prefix (.m2ts) or at 204 (five syncs decide; a lost sync is searched byte by byte), the continuity counter per PID,
 * PAT (the lowest non-zero program) and PMT sections with CRC-32/MPEG-2, the first stream of the PMT whose type is known (0x0F ADTS
 * AAC, 0x11 LATM AAC, 0x03 / 0x04 MPEG audio, 0x80 Blu-ray LPCM, 0x81 / 0x87 AC-3, 0x82 DTS, 0x06 with an AC-3 descriptor or an HDMV
 * program), its PES packets with PTS / DTS unwrapped from 33 bits.  Handed out: one packet per ADTS frame, per MPEG audio frame, per
 * LOAS frame, per Blu-ray LPCM PES (without its 4-byte header), per AC-3 or DTS PES.  The output does not depend on how the bytes are
 * cut into calls.  Budgets: 4 MiB a call, 1 MiB a PES.  A refusal is SK_TS_ERR_STREAM with a text (sk_ts_demuxer_last_error); the
 * packets complete in front of it stay takeable and the demuxer stays refused.  A Blu-ray LPCM PES payload begins with four bytes:
 * 0-1 the big-endian size of what follows, byte 2 the channel assignment (high nibble) and the rate code (low nibble: 1 = 48 000,
 * 4 = 96 000, 5 = 192 000), byte 3's top two bits the depth code (1 = 16, 2 = 20, 3 = 24).  Built: stereo (channel assignment 3) at 16 or
 * 24 bits; mono, 20 bits, the multichannel assignments and a size field that disagrees with its payload are refused with texts of
 * this project's own.  Not read: PCR, video, data PIDs, any program but the one chosen. */
enum sk_ts_status { SK_TS_ERR_STREAM = -1101 };
enum sk_ts_codec { SK_TS_CODEC_AAC = 1, SK_TS_CODEC_PCM = 2, SK_TS_CODEC_AC3 = 3, SK_TS_CODEC_DTS = 4, SK_TS_CODEC_MP3 = 5, SK_TS_CODEC_MP1 = 6,
                   SK_TS_CODEC_MP2 = 7, SK_TS_CODEC_MPEG_AUDIO = 8 };
enum sk_ts_packet_format { SK_TS_FORMAT_RAW = 0, SK_TS_FORMAT_ADTS = 1, SK_TS_FORMAT_LATM = 2 };
typedef struct sk_ts_track_info {
    uint32_t codec;          /* sk_ts_codec: MPEG audio is named by its first frame's layer */
    uint32_t packet_format;  /* sk_ts_packet_format */
    uint32_t stream_type;    /* the PMT's */
    uint32_t pid, program_number;
    uint32_t packet_stride, packet_prefix; /* 188 / 0, 192 / 4, 204 / 0 */
    uint32_t sample_rate, channels;        /* of the first frame; 0 where has_rate / has_channels is 0 (LATM, AC-3, DTS) */
    uint32_t bits_per_sample, bytes_per_frame, frames_per_packet; /* Blu-ray LPCM alone (big-endian, signed, interleaved), else 0 */
    uint8_t has_rate, has_channels;
    uint8_t lpcm_header[4];  /* Blu-ray LPCM: the first PES's four header bytes */
    uint8_t reserved[2];
} sk_ts_track_info;
typedef struct sk_ts_packet_info {
    uint64_t pts, dts;       /* 90 kHz units, unwrapped; a frame behind the first of its PES is its durations later */
    uint32_t duration;       /* 90 kHz units */
    uint8_t has_pts, has_dts, has_duration;
    uint8_t continuity_counter; /* of the packet that started the PES */
    uint8_t discontinuity;      /* on the first frame of a PES that met the flag or a gap */
    uint8_t reserved[3];
} sk_ts_packet_info;
typedef struct sk_ts_demuxer sk_ts_demuxer;
int sk_ts_demuxer_create(sk_ts_demuxer **out);
void sk_ts_demuxer_destroy(sk_ts_demuxer *);
int sk_ts_demuxer_add(sk_ts_demuxer *, const uint8_t *bytes, size_t len);
/* the last PES is handed out */
int sk_ts_demuxer_finish(sk_ts_demuxer *);
const char *sk_ts_demuxer_last_error(const sk_ts_demuxer *);
/* the config event: it comes with the track's first packet.  SK_ERR_BAD_STREAM before that */
int sk_ts_demuxer_config(const sk_ts_demuxer *, sk_ts_track_info *info);
/* packets waiting, the first one's size and the bytes the demuxer holds that are no packet yet */
int sk_ts_demuxer_pending(const sk_ts_demuxer *, uint32_t *n_packets, size_t *front_bytes, size_t *buffered_bytes);
/* takes the first waiting packet.  None waiting: SK_ERR_BAD_STREAM; cap too small: SK_ERR_CAPACITY, the packet stays */
int sk_ts_demuxer_take(sk_ts_demuxer *, uint8_t *out, size_t cap, size_t *len, sk_ts_packet_info *info);
/* looks_like_mpeg_ts of the decoder: three syncs at stride 188, or at stride 192 behind four bytes.  1 / 0 */
int sk_ts_sniff(const uint8_t *bytes, size_t len);
/* a stream known to be a transport stream, for a join in mid-segment where the first bytes are no sync (the demuxer finds it);
 * sk_pipeline_spawn takes a transport stream by sk_ts_sniff itself */
int sk_pipeline_spawn_mpeg_ts(sk_pipeline *, const sk_decode_options *opt /* NULL = defaults */, uint32_t *handle);

/* ---- AVI audio demuxer (host only, csrc/avi_stream.h) --------------------------------------------------------------- */
/* What decode_avi_audio reads (soundkit-decoder/src/lib.rs:257-570) as an incremental walk, audio only: `RIFF....AVI ` and any number of
 * `RIFF....AVIX` forms; `LIST hdrl` -> `LIST strl` -> `strh` / `strf`, the first `auds` stream is the track and its index its position
 * among all strl lists; `LIST movi` chunk by chunk (never buffered whole), nested LISTs to a depth of 8; `##wb` chunks whose two hex
 * digits are the track's index are the packets, one per chunk.  Events in order: the config once `hdrl` has been read, then packets.
 * A file cut inside a chunk gives the complete chunks in front of it.  Budgets: 4 MiB a call, 1 000 000 chunks a container, 512 MiB of
 * payload, 16 MiB of `hdrl` (this project's).  A refusal is SK_AVI_ERR_STREAM with a text (sk_avi_demuxer_last_error); the events
 * complete in front of it stay takeable and the demuxer stays refused.  What the format tag means is the caller's business: 0x0001
 * integer PCM, 0x0003 float PCM, 0x0055 MPEG audio.  Not read: `idx1` / `indx`, video, text and MIDI streams. */
enum sk_avi_status { SK_AVI_ERR_STREAM = -1401 };
enum sk_demux_event { SK_DEMUX_NONE = 0, SK_DEMUX_CONFIG = 1, SK_DEMUX_PACKET = 2 };
typedef struct sk_avi_track_info {
    uint32_t stream_index;
    uint32_t sample_rate;
    uint16_t format_tag; /* WAVEFORMAT's wFormatTag */
    uint8_t channels;    /* 1 ... 255 */
    uint8_t bits;        /* wBitsPerSample, clamped to 255 */
} sk_avi_track_info;
typedef struct sk_avi_demuxer sk_avi_demuxer;
int sk_avi_demuxer_create(sk_avi_demuxer **out);
void sk_avi_demuxer_destroy(sk_avi_demuxer *);
int sk_avi_demuxer_add(sk_avi_demuxer *, const uint8_t *bytes, size_t len);
int sk_avi_demuxer_finish(sk_avi_demuxer *);
/* the next waiting event: *event = SK_DEMUX_NONE (nothing waits), SK_DEMUX_CONFIG (*info is filled) or SK_DEMUX_PACKET (*len bytes in
 * out).  cap too small for the packet: SK_ERR_CAPACITY, *len is what it needs and the packet stays */
int sk_avi_demuxer_next(sk_avi_demuxer *, int *event, sk_avi_track_info *info, uint8_t *out, size_t cap, size_t *len);
const char *sk_avi_demuxer_last_error(const sk_avi_demuxer *);

/* ---- MPEG program stream audio demuxer (host only, csrc/ps_stream.h) ------------------------------------------------- */
/* What decode_mpeg_ps_audio reads (soundkit-decoder/src/lib.rs:572-804) as an incremental walk, audio only: start codes, the pack
 * header by its own layout, every id from BB on by its 16-bit length, PES headers in the MPEG-2 and the MPEG-1 form.  DVD LPCM
 * (private_stream_1, substream A0 ... AF): the sample bytes behind the 4 + 3 header bytes leave in whole blocks (block_bytes), the
 * remainder is carried to the next packet; 16 bits: big-endian samples (SK_FMT_S16BE), 24 bits: SK_AIFF_DVD_S24's groups; 20 bits are
 * refused.  MPEG audio (C0 ... DF): the payloads, one packet each, are the elementary stream.  track_mode: SK_PS_TRACK_FIRST -- the
 * first audio packet of either kind names the track; SK_PS_TRACK_LPCM / SK_PS_TRACK_MPEG_AUDIO -- that kind alone, the other is stepped
 * over.  Beyond the reference: packets are walked by their length field, only the first LPCM substream is the track, MPEG audio is a
 * track.  Budgets: 4 MiB a call, 512 MiB of payload.  A refusal is SK_PS_ERR_STREAM with a text; the events complete in front of it
 * stay takeable and the demuxer stays refused.  Not read: AC-3 / DTS substreams, video, the system header's contents, SCR. */
enum sk_ps_status { SK_PS_ERR_STREAM = -1501 };
enum sk_ps_track_mode { SK_PS_TRACK_FIRST = 0, SK_PS_TRACK_LPCM = 1, SK_PS_TRACK_MPEG_AUDIO = 2 };
enum sk_ps_kind { SK_PS_KIND_LPCM = 1, SK_PS_KIND_MPEG_AUDIO = 2 };
typedef struct sk_ps_track_info {
    uint32_t sample_rate; /* DVD LPCM; 0 for MPEG audio, whose frames say it */
    uint32_t block_bytes; /* DVD LPCM: every packet is a whole number of these */
    uint8_t kind;         /* sk_ps_kind */
    uint8_t stream_id;    /* BD, or C0 ... DF */
    uint8_t substream_id; /* DVD LPCM: A0 ... AF */
    uint8_t channels;     /* DVD LPCM: 1 ... 8 */
    uint8_t bits;         /* DVD LPCM: 16 / 24 */
    uint8_t reserved[3];
} sk_ps_track_info;
typedef struct sk_ps_demuxer sk_ps_demuxer;
int sk_ps_demuxer_create(int track_mode, sk_ps_demuxer **out);
void sk_ps_demuxer_destroy(sk_ps_demuxer *);
int sk_ps_demuxer_add(sk_ps_demuxer *, const uint8_t *bytes, size_t len);
int sk_ps_demuxer_finish(sk_ps_demuxer *);
int sk_ps_demuxer_next(sk_ps_demuxer *, int *event, sk_ps_track_info *info, uint8_t *out, size_t cap, size_t *len); /* as sk_avi_demuxer_next */
const char *sk_ps_demuxer_last_error(const sk_ps_demuxer *);

/* ---- ALAC decode stage (GPU, csrc/alac_decode.hip)-------------------------------------------------------------------- */
/* packets[i] lies at bytes + packets[i].offset, a multiple of 16.  Output: the packets one after the other in the order given, each
 * frames x channels samples interleaved in bitstream channel order, little-endian in bit_depth / 8 bytes.  frames_per_packet[i] is what
 * sk_alac_packet_frames reads (0 where it refuses: such a packet has no place in `out`); status_per_packet[i]: SK_OK, SK_ALAC_INVALID,
 * SK_ALAC_UNSUPPORTED or SK_ERR_UNSUPPORTED (an element whose working width exceeds 32 bits: a pair at 32 bits without extra bytes).
 * A rejected packet keeps its place in `out` and nothing is written there.  An empty packet, one above 16 MiB, an offset that is no
 * multiple of 16, a config outside sk_alac_parse_cookie's limits or an out_cap too small: SK_ERR_INVALID_ARG, nothing decoded.
 * The _dev form takes 16-byte aligned device pointers, runs on the engine's stream and waits only for the statuses; there
 * frames_per_packet is an INPUT (the caller read the counts when it had the bytes; the device rejects a packet that disagrees). */
typedef struct sk_alac_packet {
    uint32_t offset, size;
} sk_alac_packet;
int sk_alac_decode_packets(sk_engine *, const sk_alac_config *, const sk_alac_packet *packets, uint32_t n, const uint8_t *bytes, uint8_t *out,
                           size_t out_cap, size_t *out_len, int32_t *status_per_packet, uint32_t *frames_per_packet);
int sk_alac_decode_packets_dev(sk_engine *, const sk_alac_config *, const sk_alac_packet *packets, uint32_t n, const uint8_t *d_bytes,
                               size_t bytes_len, uint8_t *d_out, size_t out_cap, size_t *out_len, int32_t *status_per_packet,
                               const uint32_t *frames_per_packet);

/* The tick of the ALAC streams, sk_tick_run_flac's pattern with packets as units: packets[k] lies at bytes + packets[k].offset (a
 * multiple of 16), stream after stream, packets[k].frames is what sk_alac_packet_frames read from it (the scheduler reads it when the
 * packet arrives; 0 or above the cookie's frame_length: SK_ERR_INVALID_ARG), and every packet is first decoded to PCM on the device.
 * Each stream carries its own cookie's parameters.  A stream with nothing to change (no rate change, out_bits = bit_depth, out_channels = channels)
 * gets those bytes as its outputs, one per packet, for 1 ... 8 channels.  Every other stream then runs exactly what sk_tick_run_pcm runs
 * on a little-endian source of that format -- same kernels, records, bounds and limits (the exact 24 / 32 -> 16 path included; 3 ... 8
 * channels need sk_engine_enable_wide_pcm).  A refused tick leaves every stream as it was.  status_per_packet[k] is
 * sk_alac_decode_packets': a rejected packet writes nothing; its output record carries the status, and behind a conversion -- where the
 * packet went in as silence -- every record of its stream in this tick does: the stream is to be ended. */
typedef struct sk_alac_tick_stream {
    uint32_t stream;       /* engine stream (resample = 1 only) */
    uint32_t n_units;      /* packets */
    uint32_t frame_length; /* the cookie's: frame_length, channels, bit_depth, pb, mb, kb */
    uint8_t channels;      /* 1 ... 8 */
    uint8_t bit_depth;     /* 16 / 24 / 32 */
    uint8_t pb, mb, kb;
    uint8_t out_bits;      /* 16 / 24 / 32 */
    uint8_t out_channels;
    uint8_t resample;
    uint8_t flush;
    uint8_t reserved[3];
} sk_alac_tick_stream;
typedef struct sk_alac_tick_packet {
    uint32_t offset, size;
    uint32_t frames; /* sk_alac_packet_frames' */
    uint32_t reserved;
} sk_alac_tick_packet;
size_t sk_tick_alac_out_bound_on(sk_engine *, const sk_alac_tick_stream *streams, uint32_t n_streams, const sk_alac_tick_packet *packets,
                                 uint32_t n_packets, uint32_t *max_outputs);
int sk_tick_run_alac(sk_engine *, const sk_alac_tick_stream *streams, uint32_t n_streams, const sk_alac_tick_packet *packets, uint32_t n_packets,
                     const uint8_t *bytes, size_t bytes_len, uint8_t *out_bytes, size_t out_cap, sk_tick_output *outputs, uint32_t outputs_cap,
                     uint32_t *n_outputs, size_t *out_bytes_used, int32_t *status_per_packet);

/* A scheduler stream of ALAC packets (the reference's sequential pipeline refuses ALAC containers, SEEKABLE_ALAC_REQUIRED, so nothing is
 * sniffed: the caller has the container's index and hands over the cookie -- in any of sk_alac_parse_cookie's forms -- and the packets).
 * Every sk_pipeline_send is exactly one packet; the empty send ends the stream and flushes the resampler.  One AudioData per packet, or
 * what the output options make of them (the PCM-family tick).  A packet the host or the device rejects ends its stream with
 * `Decoding failed: ALAC packet rejected: ...` and leaves its neighbours untouched.  A cookie that is refused: SK_ALAC_ERR_STREAM. */
int sk_pipeline_spawn_alac_packets(sk_pipeline *, const uint8_t *cookie, size_t cookie_len, const sk_decode_options *opt, uint32_t *handle);

/* AlacPacketDecoder (soundkit-alac/src/lib.rs:217-300): a cookie once, then one packet per call -> one AudioData's bytes (signed
 * little-endian, bit_depth / 8 bytes a sample).  An empty packet, one above 16 MiB, a packet the device rejects: SK_ALAC_ERR_STREAM with
 * a text in last_error; the decoder goes on with the next packet (packets are independent).  out_cap too small: SK_ERR_CAPACITY. */
typedef struct sk_alac_packet_decoder sk_alac_packet_decoder;
int sk_alac_packet_decoder_create(sk_engine *, const uint8_t *cookie, size_t cookie_len, sk_alac_packet_decoder **out, char *error,
                                  size_t error_cap);
void sk_alac_packet_decoder_destroy(sk_alac_packet_decoder *);
/* maximum_pcm_samples = frame_length x channels */
int sk_alac_packet_decoder_info(const sk_alac_packet_decoder *, uint32_t *sample_rate, uint8_t *channels, uint8_t *bit_depth,
                                size_t *maximum_pcm_samples);
int sk_alac_packet_decoder_decode_packet(sk_alac_packet_decoder *, const uint8_t *packet, size_t len, uint8_t *out, size_t out_cap, size_t *out_len);
const char *sk_alac_packet_decoder_last_error(const sk_alac_packet_decoder *);

/* ---- Telephony: headerless G.711, G.722 and G.726 streams (GPU, csrc/g72x_decode.hip; host arithmetic in csrc/g72x_stream.h) -- */
/* The streams of DecodePipeline::spawn_g711 / spawn_g722 / spawn_g726* (soundkit-decoder/src/lib.rs:2512-2610): no header, nothing to
 * detect -- the caller knows the codec from its transport.  Everything decodes to s16le, bit for bit what the reference's decoders
 * give.  G.711: mu-law or A-law, one byte a sample, any rate and channel count (the samples interleaved as they arrive).  G.722: the
 * 64 kbit/s mode, mono 16 kHz, two samples a byte.  G.726: 16 / 24 / 32 / 40 kbit/s, mono 8 kHz, codes packed left (MSB first, `ffmpeg
 * -f g726`) or right (LSB first, `-f g726le`) in groups of 1 / 3 / 1 / 5 bytes that give 4 / 8 / 2 / 8 samples.  Not built: G.722 at
 * 56 / 48 kbit/s or with packed codes, AMR-NB, G.729 and Speex (the reference reaches them through foreign codecs), the encoders.  GSM 06.10
 * full rate has its own block below (sk_gsm_*). */
enum sk_g72x_codec { SK_G711_ULAW = 0, SK_G711_ALAW = 1, SK_G722 = 2, SK_G726 = 3 };
enum sk_g726_packing { SK_G726_LEFT = 0, SK_G726_RIGHT = 1 };
enum sk_g72x_status {
    SK_G72X_ERR_STREAM = -701 /* a send or a stream was rejected with a text */
};
#define SK_G72X_MAX_SEND_SAMPLES 262144 /* the reference's scratch (lib.rs:82): what one send -- one unit -- may decode to */
/* The carry of a G.726 stream from call to call: G726Core (soundkit-g726/src/lib.rs:182-212), 24 words of plain data in the caller's
 * memory.  A new stream starts from sk_g726_state_init: yl 34816, yu 544, dq[] and sr[] 32, everything else 0. */
typedef struct sk_g726_state {
    int32_t yl, yu, dms, dml, ap;
    int32_t a[2], b[6], pk[2], dq[6], sr[2];
    int32_t td;
} sk_g726_state;
/* The carry of a G.722 stream: per band (low, high) the predictor of the standard's block 4 -- s, sz, r[1..2], p[1..2], a[1..2],
 * b[1..6], d[1..6] -- with the log scale factor nb and the scale factor det, then the receive QMF's 22 history entries (oldest first,
 * alternating rlow + rhigh and rlow - rhigh).  66 words.  A new stream starts from ALL ZEROS (sk_g722_state_init), both det included:
 * that is what the reference's recording pins (the C code this decoder descends from starts det at 32 / 8). */
typedef struct sk_g722_band {
    int32_t s, sz, r[2], p[2], a[2], b[6], d[6], nb, det;
} sk_g722_band;
typedef struct sk_g722_state {
    sk_g722_band band[2];
    int32_t x[22];
} sk_g722_state;
void sk_g726_state_init(sk_g726_state *);
void sk_g722_state_init(sk_g722_state *);

/* One stream's bytes, one call.  g726_rate (16000 / 24000 / 32000 / 40000) and g726_packing are read for SK_G726 only; `state` is a
 * sk_g726_state for SK_G726, a sk_g722_state for SK_G722 and unused (may be NULL) for G.711.  G.726 takes whole groups: a len that is
 * none is SK_ERR_INVALID_ARG (sk_g726_decoder_* holds the partial group back).  out receives len x 2 (G.711), len x 4 (G.722) or
 * groups x samples x 2 (G.726) bytes of s16le; an out_cap below that is SK_ERR_INVALID_ARG and nothing is written.  A call that decodes
 * to more than SK_G72X_MAX_SEND_SAMPLES samples is SK_G72X_ERR_STREAM with the reference's text in `error` (NUL-terminated, cut to
 * error_cap; may be NULL): `Output buffer too small for G.726 decode: need N, have 262144`, with the codec's own name.  The state is
 * read on entry and written on success; any failure leaves it as it was.  The _dev form takes 16-byte aligned device pointers (the
 * input is read in whole dwords up to the one that holds its last byte) and runs on the engine's stream. */
int sk_g72x_decode(sk_engine *, int codec, uint32_t g726_rate, int g726_packing, const uint8_t *bytes, size_t len, uint8_t *out, size_t out_cap,
                   size_t *out_len, void *state, char *error, size_t error_cap);
int sk_g72x_decode_dev(sk_engine *, int codec, uint32_t g726_rate, int g726_packing, const uint8_t *d_bytes, size_t len, uint8_t *d_out,
                       size_t out_cap, size_t *out_len, void *state, char *error, size_t error_cap);

/* Many streams, one launch sequence (k_g726 over the G.726 streams, k_g722_adpcm + k_g722_qmf over the G.722 streams, the G.711
 * expansion over the G.711 units).  The units are listed stream by stream in the order of `streams`; units[k] lies at bytes +
 * units[k].offset, a multiple of 16, and a stream's units are decoded in order, the state carried from one into the next.  A unit may be
 * empty; a G.726 unit holds whole groups; no unit decodes to more than SK_G72X_MAX_SEND_SAMPLES samples.  Every unit's s16le is written
 * at the next multiple of 16 bytes of `out`, in table order, and the call sets units[k].out_offset and .out_len.  streams[i].state names
 * the stream's record in g726_states (SK_G726) or g722_states (SK_G722); a record may be named by one stream only.  Anything that does
 * not add up, or an out_cap too small: SK_ERR_INVALID_ARG, nothing decoded.  The states are written on success only. */
typedef struct sk_g72x_stream {
    uint8_t codec;        /* enum sk_g72x_codec */
    uint8_t g726_packing; /* enum sk_g726_packing */
    uint8_t reserved[2];
    uint32_t g726_rate;   /* 16000 / 24000 / 32000 / 40000 */
    uint32_t n_units;
    uint32_t state;
} sk_g72x_stream;
typedef struct sk_g72x_unit {
    uint32_t offset, size;
    uint32_t out_len;    /* out: bytes */
    uint32_t reserved;
    uint64_t out_offset; /* out */
} sk_g72x_unit;
int sk_g72x_decode_batch(sk_engine *, const sk_g72x_stream *streams, uint32_t n_streams, sk_g72x_unit *units, uint32_t n_units, const uint8_t *bytes,
                         size_t bytes_len, uint8_t *out, size_t out_cap, size_t *out_len, sk_g726_state *g726_states, uint32_t n_g726_states,
                         sk_g722_state *g722_states, uint32_t n_g722_states);
int sk_g72x_decode_batch_dev(sk_engine *, const sk_g72x_stream *streams, uint32_t n_streams, sk_g72x_unit *units, uint32_t n_units,
                             const uint8_t *d_bytes, size_t bytes_len, uint8_t *d_out, size_t out_cap, size_t *out_len, sk_g726_state *g726_states,
                             uint32_t n_g726_states, sk_g722_state *g722_states, uint32_t n_g722_states);

/* The tick of the telephony streams, sk_tick_run_aiff's pattern: every unit (= what one send decodes now, packed at a 16-byte aligned
 * offset; never empty, G.726 in whole groups, at most SK_G72X_MAX_SEND_SAMPLES samples) is first decoded to s16le on the device.  A
 * stream with nothing further to change (no rate change, out_bits = 16, out_channels = channels) gets those bytes as its outputs, one
 * per unit.  Every other stream then runs exactly what sk_tick_run_pcm runs on an s16le source of that channel count -- same kernels,
 * records, bounds and limits; there a G.711 unit holds whole frames.  channels is read for G.711 (G.722 and G.726 are mono: 1).  The
 * streams' carries are named as in sk_g72x_decode_batch.  On failure, or when the tick is refused, the carries and the resamplers are
 * as they were before the call. */
typedef struct sk_g72x_tick_stream {
    uint32_t stream;      /* engine stream (resample = 1 only) */
    uint32_t n_units;
    uint32_t g726_rate;
    uint32_t state;
    uint8_t codec;        /* enum sk_g72x_codec */
    uint8_t g726_packing;
    uint8_t channels;
    uint8_t out_bits;     /* 16 / 24 / 32 */
    uint8_t out_channels;
    uint8_t resample;
    uint8_t flush;
    uint8_t reserved;
} sk_g72x_tick_stream;
size_t sk_tick_g72x_out_bound_on(sk_engine *, const sk_g72x_tick_stream *streams, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units,
                                 uint32_t *max_outputs);
int sk_tick_run_g72x(sk_engine *, const sk_g72x_tick_stream *streams, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units,
                     const uint8_t *bytes, size_t bytes_len, uint8_t *out_bytes, size_t out_cap, sk_tick_output *outputs, uint32_t outputs_cap,
                     uint32_t *n_outputs, size_t *out_bytes_used, sk_g726_state *g726_states, uint32_t n_g726_states, sk_g722_state *g722_states,
                     uint32_t n_g722_states);

/* Scheduler streams of headerless telephony audio (DecodePipeline::spawn_g711 / spawn_g722 / spawn_g726*, lib.rs:2512-2610): the stream
 * has its decoder from the spawn and detects nothing.  Every non-empty sk_pipeline_send is one decode and gives one AudioData -- 16 bits;
 * G.711 at the spawn's rate and channel count, G.722 16 kHz mono, G.726 8 kHz mono -- or what the output options make of it (the
 * PCM-family tick); a G.726 send that completes no group delivers nothing.  The empty send ends the stream: G.726 with a partial group
 * left ends alone with `Decoding failed: G.726 stream ended with N trailing partial-packet byte(s)`, G.711 and G.722 end with nothing
 * more.  A send that decodes to more than SK_G72X_MAX_SEND_SAMPLES samples ends its stream with `Decoding failed: Output buffer too small
 * for ... decode: need N, have 262144`.  G.711 of several channels: as decoded the samples leave as they came; behind a conversion a
 * send that splits a frame ends the stream with the reference's `Decoding failed: Output conversion failed: PCM data is unsupported or
 * contains a partial frame`.  sk_pipeline_spawn_g711 with a rate or a channel count of 0: SK_G72X_ERR_STREAM and the reference's text
 * (`G.711 sample rate must be > 0`, `G.711 channel count must be > 0`) in `error` (NUL-terminated, cut to error_cap; may be NULL).  A
 * rate that is no G.726 rate, a packing or a law that is none: SK_ERR_INVALID_ARG. */
int sk_pipeline_spawn_g711(sk_pipeline *, int law, uint32_t sample_rate, uint32_t channels, const sk_decode_options *opt, uint32_t *handle,
                           char *error, size_t error_cap);
int sk_pipeline_spawn_g722(sk_pipeline *, const sk_decode_options *opt, uint32_t *handle);
int sk_pipeline_spawn_g726(sk_pipeline *, uint32_t g726_rate, int g726_packing, const sk_decode_options *opt, uint32_t *handle);

/* The reference's Decoder objects (soundkit-g711 / -g722 / -g726): decode_i16, decode_i32 (= the s16 sample << 16), decode_f32 (= / 32768),
 * sample_rate / channels through _info.  `written` counts samples; an out_cap (in samples) below what the input decodes to is
 * SK_ERR_CAPACITY with `Output buffer too small for ... decode: need N, have M` in last_error and nothing consumed.  The G.726 decoder
 * holds a partial group back for the next call, and sk_g726_decoder_flush at the end of the stream is SK_G72X_ERR_STREAM with `G.726
 * stream ended with N trailing partial-packet byte(s)` when one is left.  sk_g711_decoder_create refuses a rate or a channel count of 0
 * with the reference's text in `error`.  kind: 0 = i16, 1 = i32, 2 = f32. */
typedef struct sk_g72x_decoder sk_g72x_decoder;
int sk_g711_decoder_create(sk_engine *, int law /* SK_G711_ULAW / SK_G711_ALAW */, uint32_t sample_rate, uint32_t channels, sk_g72x_decoder **out,
                           char *error, size_t error_cap);
int sk_g722_decoder_create(sk_engine *, sk_g72x_decoder **out);
int sk_g726_decoder_create(sk_engine *, uint32_t g726_rate, int g726_packing, sk_g72x_decoder **out);
void sk_g72x_decoder_destroy(sk_g72x_decoder *);
int sk_g72x_decoder_info(const sk_g72x_decoder *, int *codec, uint32_t *sample_rate, uint32_t *channels);
int sk_g72x_decoder_decode_i16(sk_g72x_decoder *, const uint8_t *input, size_t len, int16_t *out, size_t out_cap, size_t *written);
int sk_g72x_decoder_decode_i32(sk_g72x_decoder *, const uint8_t *input, size_t len, int32_t *out, size_t out_cap, size_t *written);
int sk_g72x_decoder_decode_f32(sk_g72x_decoder *, const uint8_t *input, size_t len, float *out, size_t out_cap, size_t *written);
int sk_g726_decoder_flush(sk_g72x_decoder *);
int sk_g72x_decoder_reset(sk_g72x_decoder *);
const char *sk_g72x_decoder_last_error(const sk_g72x_decoder *);

/* ---- Telephony: GSM 06.10 full-rate streams (GPU, csrc/gsm_decode.hip; host arithmetic in csrc/gsm_stream.h) --------------------- */
/* The streams of DecodePipeline::spawn_gsm (soundkit-decoder/src/lib.rs:2358) and the reference's GsmDecoder (soundkit-gsm): 13 kbit/s
 * RPE-LTP, 8 kHz mono, decoded to s16le bit for bit what libgsm's gsm_decode gives.  SK_GSM_STANDARD: packets of 33 bytes (a 0xD nibble,
 * then 260 parameter bits) that give 160 samples.  SK_GSM_MICROSOFT: packets of 65 bytes that give 320 -- the reference's framing, two
 * runs of 260 bits MSB first (unpack_ms_pair), which is NOT libgsm's LSB-first WAV-49 layout.  A standard frame whose first nibble is
 * not 0xD is refused with `GSM decoder rejected frame`; Microsoft packets carry no magic.  Shares SK_G72X_ERR_STREAM,
 * SK_G72X_MAX_SEND_SAMPLES and sk_g72x_unit with the block above.  Not built: the encoder, libgsm's WAV-49 layout, AMR-NB, G.729, Speex. */
enum sk_gsm_variant { SK_GSM_STANDARD = 0, SK_GSM_MICROSOFT = 1 };
/* The carry of a GSM stream from call to call, 138 words of plain data in the caller's memory: the long-term history (the last 120
 * reconstructed short-term residual samples, oldest first), the synthesis lattice's memory, the de-emphasis memory, the last valid lag
 * and the previous frame's decoded log-area ratios.  A new stream starts from sk_gsm_state_init: all zeros, except nrp = 40. */
typedef struct sk_gsm_state {
    int32_t dp[120];
    int32_t v[8];
    int32_t msr;
    int32_t nrp;
    int32_t larpp[8];
} sk_gsm_state;
void sk_gsm_state_init(sk_gsm_state *);

/* One stream's whole packets, one call.  A len that is no multiple of the packet size is SK_ERR_INVALID_ARG (sk_gsm_decoder_* holds the
 * partial packet back).  out receives packets x samples x 2 bytes of s16le; an out_cap below that is SK_ERR_INVALID_ARG and nothing is
 * written.  A call that decodes to more than SK_G72X_MAX_SEND_SAMPLES samples (checked first), or a standard frame without the magic
 * nibble (every frame is checked before anything is launched), is SK_G72X_ERR_STREAM with the reference's text in `error`
 * (NUL-terminated, cut to error_cap; may be NULL): `Output buffer too small for GSM decode: need N, have 262144`, `GSM decoder rejected
 * frame`.  The state is read on entry and written on success; any failure leaves it as it was and decodes nothing (the reference's
 * object has by then advanced through the frames before a rejected one; its stream ends either way).  The _dev form takes 16-byte
 * aligned device pointers (the input is read in whole dwords up to the one that holds its last byte) and runs on the engine's stream;
 * it cannot see the bytes, so the magic check is the caller's. */
int sk_gsm_decode(sk_engine *, int variant, const uint8_t *bytes, size_t len, uint8_t *out, size_t out_cap, size_t *out_len, sk_gsm_state *state,
                  char *error, size_t error_cap);
int sk_gsm_decode_dev(sk_engine *, int variant, const uint8_t *d_bytes, size_t len, uint8_t *d_out, size_t out_cap, size_t *out_len,
                      sk_gsm_state *state, char *error, size_t error_cap);

/* Many streams, one launch sequence (k_gsm_excite, then k_gsm_synth, over all streams).  The units are listed stream by stream in the
 * order of `streams`; units[k] lies at bytes + units[k].offset, a multiple of 16, and a stream's units are decoded in order, the state
 * carried from one into the next.  A unit may be empty; otherwise it holds whole packets and decodes to at most
 * SK_G72X_MAX_SEND_SAMPLES samples.  Every unit's s16le is written at the next multiple of 16 bytes of `out`, in table order, and the
 * call sets units[k].out_offset and .out_len.  streams[i].state names the stream's record in `states`; a record may be named by one
 * stream only.  Anything that does not add up, or an out_cap too small: SK_ERR_INVALID_ARG; a standard frame without the magic nibble
 * (host form; every frame is checked before anything is launched): SK_G72X_ERR_STREAM.  Either way nothing is decoded.  The states are
 * written on success only. */
typedef struct sk_gsm_stream {
    uint32_t variant; /* enum sk_gsm_variant */
    uint32_t n_units;
    uint32_t state;
} sk_gsm_stream;
int sk_gsm_decode_batch(sk_engine *, const sk_gsm_stream *streams, uint32_t n_streams, sk_g72x_unit *units, uint32_t n_units, const uint8_t *bytes,
                        size_t bytes_len, uint8_t *out, size_t out_cap, size_t *out_len, sk_gsm_state *states, uint32_t n_states);
int sk_gsm_decode_batch_dev(sk_engine *, const sk_gsm_stream *streams, uint32_t n_streams, sk_g72x_unit *units, uint32_t n_units,
                            const uint8_t *d_bytes, size_t bytes_len, uint8_t *d_out, size_t out_cap, size_t *out_len, sk_gsm_state *states,
                            uint32_t n_states);

/* The tick of the GSM streams, sk_tick_run_g72x's contract: every unit (= what one send decodes now, packed at a 16-byte aligned
 * offset; never empty, whole packets, standard frames with their magic nibble, at most SK_G72X_MAX_SEND_SAMPLES samples) is first
 * decoded to s16le on the device.  A stream with nothing further to change (no rate change, out_bits = 16, out_channels = 1) gets those
 * bytes as its outputs, one per unit.  Every other stream then runs exactly what sk_tick_run_pcm runs on an 8 kHz mono s16le source --
 * same kernels, records, bounds and limits.  The carries are named as in sk_gsm_decode_batch.  On failure, or when the tick is refused,
 * the carries and the resamplers are as they were before the call. */
typedef struct sk_gsm_tick_stream {
    uint32_t stream;      /* engine stream (resample = 1 only) */
    uint32_t n_units;
    uint32_t state;
    uint8_t variant;      /* enum sk_gsm_variant */
    uint8_t channels;     /* 1 */
    uint8_t out_bits;     /* 16 / 24 / 32 */
    uint8_t out_channels;
    uint8_t resample;
    uint8_t flush;
    uint8_t reserved[2];
} sk_gsm_tick_stream;
size_t sk_tick_gsm_out_bound_on(sk_engine *, const sk_gsm_tick_stream *streams, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units,
                                uint32_t *max_outputs);
int sk_tick_run_gsm(sk_engine *, const sk_gsm_tick_stream *streams, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units,
                    const uint8_t *bytes, size_t bytes_len, uint8_t *out_bytes, size_t out_cap, sk_tick_output *outputs, uint32_t outputs_cap,
                    uint32_t *n_outputs, size_t *out_bytes_used, sk_gsm_state *states, uint32_t n_states);

/* A scheduler stream of GSM packets (DecodePipeline::spawn_gsm): the stream has its decoder from the spawn and detects nothing.  A
 * sk_pipeline_send that completes at least one packet (with what an earlier send left) is one decode and gives one AudioData -- 8 kHz,
 * mono, 16 bits -- or what the output options make of it (the PCM-family tick); a send that completes none delivers nothing.  The empty
 * send ends the stream; with bytes left it ends alone with `Decoding failed: GSM stream ended with N trailing partial-frame byte(s)`.
 * A rejected frame or a send that decodes to more than SK_G72X_MAX_SEND_SAMPLES samples ends its stream alone with `Decoding failed: ` and
 * the decoder's text.  A variant that is neither of the two: SK_ERR_INVALID_ARG. */
int sk_pipeline_spawn_gsm(sk_pipeline *, int variant, const sk_decode_options *opt, uint32_t *handle);

/* The reference's GsmDecoder: decode_i16, decode_i32 (= the s16 sample << 16), decode_f32 (= / 32768); 8 kHz mono through _info.
 * `written` counts samples; an out_cap (in samples) below what pending + input decodes to is SK_ERR_CAPACITY with `Output buffer too
 * small for GSM decode: need N, have M` in last_error and nothing consumed.  A partial packet is held back for the next call, and
 * sk_gsm_decoder_flush at the end of the stream is SK_G72X_ERR_STREAM with `GSM stream ended with N trailing partial-frame byte(s)` when
 * one is left.  A rejected frame is SK_G72X_ERR_STREAM with its text; the call consumes nothing. */
typedef struct sk_gsm_decoder sk_gsm_decoder;
int sk_gsm_decoder_create(sk_engine *, int variant, sk_gsm_decoder **out);
void sk_gsm_decoder_destroy(sk_gsm_decoder *);
int sk_gsm_decoder_info(const sk_gsm_decoder *, int *variant, uint32_t *sample_rate, uint32_t *channels);
int sk_gsm_decoder_decode_i16(sk_gsm_decoder *, const uint8_t *input, size_t len, int16_t *out, size_t out_cap, size_t *written);
int sk_gsm_decoder_decode_i32(sk_gsm_decoder *, const uint8_t *input, size_t len, int32_t *out, size_t out_cap, size_t *written);
int sk_gsm_decoder_decode_f32(sk_gsm_decoder *, const uint8_t *input, size_t len, float *out, size_t out_cap, size_t *written);
int sk_gsm_decoder_flush(sk_gsm_decoder *);
int sk_gsm_decoder_reset(sk_gsm_decoder *);
const char *sk_gsm_decoder_last_error(const sk_gsm_decoder *);

/* ---- Ogg pages and packets (host only, csrc/ogg_stream.h) ------------------------------------------------------------------- */
/* OggPacketParser (soundkit/src/ogg.rs): bytes in any pieces in, whole packets out.  One logical stream; every page's CRC is checked;
 * budgets: 4 MiB a call, 16 MiB a packet, 16 MiB + 64 KiB buffered.  A refusal is SK_VORBIS_ERR_STREAM with the reference's text in
 * sk_ogg_parser_last_error (`Ogg CRC mismatch on page N`, `chained or multiplexed Ogg streams are unsupported`, `invalid Ogg capture
 * pattern at byte N`, `Ogg input chunk exceeds the 4194304 byte streaming budget`, ...); the parser is of no use afterwards. */
typedef struct sk_ogg_parser sk_ogg_parser;
typedef struct sk_ogg_packet_info {
    uint64_t granule_position; /* of the page, on the packet that ends it (has_granule) */
    uint32_t size;
    uint32_t serial;
    uint8_t first_in_stream, last_in_page, last_in_stream, has_granule;
    uint8_t reserved[4];
} sk_ogg_packet_info;
int sk_ogg_parser_create(sk_ogg_parser **out);
void sk_ogg_parser_destroy(sk_ogg_parser *);
int sk_ogg_parser_add(sk_ogg_parser *, const uint8_t *data, size_t len);
int sk_ogg_parser_finish(sk_ogg_parser *);
uint32_t sk_ogg_parser_pending(const sk_ogg_parser *); /* complete packets waiting */
/* the oldest waiting packet: its record, and its bytes into `data` when data_cap holds them (then it is taken off the queue;
 * otherwise SK_ERR_CAPACITY with info->size set and the packet stays).  SK_ERR_BAD_STREAM: none waiting. */
int sk_ogg_parser_take(sk_ogg_parser *, sk_ogg_packet_info *info, uint8_t *data, size_t data_cap);
const char *sk_ogg_parser_last_error(const sk_ogg_parser *);
uint32_t sk_ogg_page_crc(const uint8_t *page, size_t len);

/* ---- Vorbis I: headers and the stream's tables (host only, csrc/vorbis_stream.h) ---------------------------------------------- */
enum sk_vorbis_status {
    SK_VORBIS_NOT_AUDIO = -801,  /* per packet: the type bit says header */
    SK_VORBIS_BAD_MODE = -802,   /* per packet: a mode number the setup does not have */
    SK_VORBIS_SHORT = -803,      /* per packet: it ends inside its first bits (type, mode, window flags); also an empty packet */
    SK_VORBIS_ERR_STREAM = -804  /* a header, an Ogg stream or a call was rejected with a text */
};
typedef struct sk_vorbis_ident {
    uint32_t sample_rate;
    uint32_t bitrate_maximum, bitrate_nominal, bitrate_minimum;
    uint16_t blocksize_0, blocksize_1; /* 64 ... 8192, blocksize_0 <= blocksize_1 */
    uint8_t channels;                  /* 1 ... 255 as read; the setup refuses more than 8 */
    uint8_t reserved[3];
} sk_vorbis_ident;
/* Refusals are SK_VORBIS_ERR_STREAM with a text in `error` (NUL-terminated, cut to error_cap; may be NULL). */
int sk_vorbis_parse_ident(const uint8_t *packet, size_t len, sk_vorbis_ident *out, char *error, size_t error_cap);
int sk_vorbis_parse_comment(const uint8_t *packet, size_t len, char *error, size_t error_cap); /* walked and bounds-checked only */
/* The setup header, parsed, validated and turned into the stream's device tables (Huffman lookup + tree, VQ values expanded to f32 as
 * ((multiplicand * delta) + minimum) + last, floor, residue, mapping and mode records).  It is untrusted input: every book number,
 * class and subclass book, class book dimension, coupling channel and floor X list is checked, and a code book whose lengths are neither
 * a complete prefix code nor the one-entry case is refused.  SK_ERR_UNSUPPORTED with a text: floor type 0, more than 8 channels,
 * tables above 4 MiB. */
typedef struct sk_vorbis_setup sk_vorbis_setup;
typedef struct sk_vorbis_setup_info {
    uint32_t books, floors, residues, mappings, modes, blob_bytes;
    uint16_t blocksize_0, blocksize_1;
    uint8_t channels;
    uint8_t reserved[3];
} sk_vorbis_setup_info;
int sk_vorbis_setup_create(const sk_vorbis_ident *, const uint8_t *packet, size_t len, sk_vorbis_setup **out, char *error, size_t error_cap);
void sk_vorbis_setup_destroy(sk_vorbis_setup *);
int sk_vorbis_setup_get_info(const sk_vorbis_setup *, sk_vorbis_setup_info *info);
/* the first bits of an audio packet: SK_OK and the block size it will decode to, or the per-packet status */
int sk_vorbis_packet_blocksize(const sk_vorbis_setup *, const uint8_t *packet, size_t len, uint32_t *blocksize);

/* ---- Vorbis decode stage (GPU, csrc/vorbis_decode.hip) ------------------------------------------------------------------------- */
/* Audio packets of one or many streams in one launch sequence.  packets[] lists stream 0's packets, then stream 1's, ...; packet k lies
 * at bytes + packets[k].offset (a multiple of 16).  A stream enters with the block size of its previous accepted packet and that
 * packet's windowed right half (prev_blocksize, 0 = none; overlap = [channels][prev_blocksize / 2] f32, room for blocksize_1 / 2 a
 * channel) and leaves with both updated.  Per packet: status (SK_OK or SK_VORBIS_NOT_AUDIO / _BAD_MODE / _SHORT -- such a packet yields
 * nothing and leaves the overlap as it was) and frames (prev / 4 + this / 4; 0 for a stream's first packet ever).  The output is the
 * accepted packets' frames back to back, interleaved: s16 (x * 32768, saturated, truncated toward zero, as lewton's) or, as_f32 != 0,
 * the f32 before narrowing.  out_cap and *out_len count bytes.  An out_cap too small: SK_ERR_CAPACITY with the need in *out_len, nothing
 * decoded, the streams as they were.  A packet above 16 MiB, an offset that is no multiple of 16, a prev_blocksize that is neither of the
 * setup's block sizes: SK_ERR_INVALID_ARG.  Not built: a device-resident form of these calls. */
typedef struct sk_vorbis_stream {
    const sk_vorbis_setup *setup;
    float *overlap;
    uint32_t n_packets;
    uint32_t prev_blocksize;
} sk_vorbis_stream;
typedef struct sk_vorbis_packet {
    uint32_t offset, size;
} sk_vorbis_packet;
int sk_vorbis_decode_packets(sk_engine *, sk_vorbis_stream *streams, uint32_t n_streams, const sk_vorbis_packet *packets, uint32_t n_packets,
                             const uint8_t *bytes, size_t bytes_len, int as_f32, void *out, size_t out_cap, size_t *out_len,
                             int32_t *status_per_packet, uint32_t *frames_per_packet);
/* The entropy stage alone (k_vorbis_entropy), for tests that hold it to a model bit for bit: per packet the mode, the window flags,
 * per channel the used flag, the final Y values and the posts' "used" flags, and into `residue` the packet's [channels][blocksize / 2]
 * residue vectors as the VQ adds left them (before coupling and floor), packet after packet; a rejected packet has no place there.
 * residue_cap and *residue_len count floats. */
typedef struct sk_vorbis_packet_info {
    int32_t status;
    uint8_t mode, blockflag, prev_flag, next_flag;
    uint32_t blocksize;
    uint8_t used[8];
    int16_t final_y[8][65];
    uint8_t step2[8][65];
} sk_vorbis_packet_info;
int sk_vorbis_entropy_decode(sk_engine *, const sk_vorbis_stream *streams, uint32_t n_streams, const sk_vorbis_packet *packets, uint32_t n_packets,
                             const uint8_t *bytes, size_t bytes_len, sk_vorbis_packet_info *info, float *residue, size_t residue_cap,
                             size_t *residue_len);

/* The tick of the Vorbis streams, sk_tick_run_alac's pattern with audio packets as units: packets[k] lies at bytes + packets[k].offset (a
 * multiple of 16), stream after stream; the tick is budgeted in whole packets.  A stream's carry is the caller's, as in
 * sk_vorbis_decode_packets (overlap, prev_blocksize: read on entry, written when the tick succeeded; on failure, or when the tick is
 * refused -- an out_cap or outputs_cap below sk_tick_vorbis_out_bound_on's -- carries and resamplers are as they were).  The decode is
 * sk_vorbis_decode_packets' to s16; a stream with nothing to change behind it (no rate change, out_bits = 16, out_channels = its
 * channels) gets those bytes as its outputs, one per packet that yields frames (a stream's first packet ever and a rejected packet
 * yield none; status_per_packet says which were rejected).  Every other stream then runs exactly what sk_tick_run_pcm runs on an
 * interleaved s16le source of its channel count -- same kernels, records, bounds and limits; 3 ... 8 channels with a conversion need
 * sk_engine_enable_wide_pcm.  The output does not depend on how a stream's packets are dealt out over ticks.  keep_frames cuts a
 * packet's frames (the Ogg decoder's truncation of a stream's last packet to the final granule position); 0xffffffff keeps all.
 * skip_frames drops that many of the packet's frames at its front (Matroska's negative DiscardPadding) before keep_frames applies to
 * what is left; a packet of which nothing is left yields no output, and its overlap half is carried on as ever. */
typedef struct sk_vorbis_tick_packet {
    uint32_t offset, size;
    uint32_t keep_frames;
    uint32_t skip_frames;
} sk_vorbis_tick_packet;
typedef struct sk_vorbis_tick_stream {
    const sk_vorbis_setup *setup;
    float *overlap;          /* [channels][blocksize_1 / 2] */
    uint32_t stream;         /* engine stream (resample = 1 only) */
    uint32_t n_units;        /* packets */
    uint32_t prev_blocksize; /* 0: none yet */
    uint8_t out_bits;        /* 16 / 24 / 32 */
    uint8_t out_channels;
    uint8_t resample;
    uint8_t flush;
    uint8_t channels;        /* 0, or the setup's */
    uint8_t reserved[3];
} sk_vorbis_tick_stream;
size_t sk_tick_vorbis_out_bound_on(sk_engine *, const sk_vorbis_tick_stream *streams, uint32_t n_streams, const sk_vorbis_tick_packet *packets,
                                   uint32_t n_packets, const uint8_t *bytes, size_t bytes_len, uint32_t *max_outputs);
int sk_tick_run_vorbis(sk_engine *, sk_vorbis_tick_stream *streams, uint32_t n_streams, const sk_vorbis_tick_packet *packets, uint32_t n_packets,
                       const uint8_t *bytes, size_t bytes_len, uint8_t *out_bytes, size_t out_cap, sk_tick_output *outputs, uint32_t outputs_cap,
                       uint32_t *n_outputs, size_t *out_bytes_used, int32_t *status_per_packet);

/* Vorbis in the scheduler.  sk_pipeline_spawn takes an Ogg Vorbis stream by its first bytes: `OggS`, and the first page's first packet
 * begins `\x01vorbis` (any other Ogg stream goes the way it went before).  The Ogg walk and the three headers run on the entropy threads
 * with the Ogg parser's and the header parsers' checks and texts, every audio packet is a unit of sk_tick_run_vorbis, and each packet
 * that yields frames gives one AudioData (16 bits, or what the output options make of it), the stream's last one cut to the final granule
 * position as VorbisDecoder cuts it.  A refusal ends the stream alone with `Decoding failed: ` and the text.
 * sk_pipeline_spawn_vorbis_packets is the A_VORBIS case: the three header packets at the spawn (a refusal: the parser's status, its text
 * in `error`), then demuxed audio packets, one per sk_pipeline_send; the empty send ends the stream. */
int sk_pipeline_spawn_vorbis_packets(sk_pipeline *, const uint8_t *ident, size_t ident_len, const uint8_t *comment, size_t comment_len,
                                     const uint8_t *setup, size_t setup_len, const sk_decode_options *opt, uint32_t *handle, char *error,
                                     size_t error_cap);

/* VorbisPacketDecoder (soundkit-vorbis/src/lib.rs:46-124): the three header packets, then raw audio packets (Matroska / WebM A_VORBIS),
 * one per call.  *produced = 0 for a header (Ok(None)); 1 for an audio packet, with *written interleaved s16 samples in `out` (0 for the
 * first audio packet; out_cap, in samples, must hold maximum_samples of _info).  A refused header is its parser's status with the text
 * in _last_error and may be given again; a refused audio packet is its per-packet status, and the decoder goes on with the next. */
typedef struct sk_vorbis_packet_decoder sk_vorbis_packet_decoder;
int sk_vorbis_packet_decoder_create(sk_engine *, sk_vorbis_packet_decoder **out);
void sk_vorbis_packet_decoder_destroy(sk_vorbis_packet_decoder *);
/* SK_ERR_BAD_STREAM before the identification header */
int sk_vorbis_packet_decoder_info(const sk_vorbis_packet_decoder *, uint32_t *sample_rate, uint8_t *channels, size_t *maximum_samples);
int sk_vorbis_packet_decoder_decode_packet(sk_vorbis_packet_decoder *, const uint8_t *packet, size_t len, int16_t *out, size_t out_cap, size_t *written,
                                           int *produced);
const char *sk_vorbis_packet_decoder_last_error(const sk_vorbis_packet_decoder *);

/* VorbisDecoder (soundkit-vorbis/src/lib.rs:137-296): Ogg bytes in any pieces through _add, then _finish; *written interleaved s16
 * samples per call (0: Ok(None)), all audio packets a call completes in one launch sequence.  The reference's checks and texts:
 * `Expected Vorbis identification header as first Ogg packet`, `Unexpected second Ogg logical bitstream`, the Ogg parser's; and its
 * truncation of the stream's last packet to the final granule position, exactly as process_packet does it: cur_absgp becomes known at
 * the first audio packet that ends a page and advances by each packet's samples in between.  An out_cap (in samples) too small is
 * SK_ERR_CAPACITY with the need in *written: nothing is lost, the next call (which may add no bytes) delivers those samples first.  After
 * any other error the decoder is of no further use (the reference's falls back to expecting an identification header). */
typedef struct sk_vorbis_decoder sk_vorbis_decoder;
int sk_vorbis_decoder_create(sk_engine *, sk_vorbis_decoder **out);
void sk_vorbis_decoder_destroy(sk_vorbis_decoder *);
int sk_vorbis_decoder_info(const sk_vorbis_decoder *, uint32_t *sample_rate, uint8_t *channels);
int sk_vorbis_decoder_add(sk_vorbis_decoder *, const uint8_t *data, size_t len, int16_t *out, size_t out_cap, size_t *written);
int sk_vorbis_decoder_finish(sk_vorbis_decoder *, int16_t *out, size_t out_cap, size_t *written);
const char *sk_vorbis_decoder_last_error(const sk_vorbis_decoder *);

#ifdef __cplusplus
}
#endif
#endif /* SOUNDKIT_AMD_H */

// engine.cpp -- host side of libsoundkit_amd.so: the C ABI of include/soundkit_amd.h.
//
// One sk_engine per GPU.  It owns the per-stream carried state in HBM (overlap delay and
// previous window shape: soundkit-aac-lc/src/dsp.rs:143-152; resampler history:
// soundkit-decoder/src/lib.rs:1917-1927), the constant tables, and grow-only staging
// buffers, and turns batches of frames into per-(stream, channel) wave tasks.
// There is no CPU compute path here: without a GPU sk_engine_create fails.
#include "../../include/soundkit_amd.h"
#include "sk_abi.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <thread>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "aac_entropy_tables.h"
#include "alac_stream.h"
#include "ogg_stream.h"
#include "vorbis_stream.h"
#include "g72x_stream.h"
#include "gsm_stream.h"
#include "flac_stream.h"
#include "mp12_internal.h"
#include "pcm_stream.h"
#include "sk_device.h"

namespace {

constexpr float kPiF = 3.14159274101257324219f;  // f32 PI, as the reference uses
constexpr double kPi = 3.14159265358979323846;
constexpr uint32_t kRsChunk = 4096;  // RESAMPLE_CHUNK_SIZE, soundkit-decoder lib.rs:79
constexpr uint32_t kRsHist = 512;    // 2 * sinc_len kept in front of each chunk (rubato SincFixedIn buffer)
// A resampler row holds the history and up to five chunks of a channel: [kRsBase unused | history 512 | chunk 0 | ... | chunk 4],
// six blocks of 4096 floats.  Read with a row pitch of ONE block, chunk k of a row is the VIRTUAL row 6 * row + k of a launch:
// it starts at block k, its history (the 512 samples in front of chunk k) sits kRsBase into it, and every complete chunk of
// every stream of a call goes into one launch per resampler phase with the same per-chunk launch parameters a chunk-by-chunk
// run would use -- so a stream's samples do not depend on how its input was cut into calls (an output's place in its matrix
// tile is fixed by its chunk), while a tick needs one round of launches instead of one per chunk.
constexpr uint32_t kRsBlocks = 6;
constexpr uint32_t kRsBase = kRsChunk - kRsHist;          // 3584: where the history starts in a row
constexpr uint32_t kRsWindow = kRsHist + kRsChunk;        // what one chunk's launch may read behind its virtual row's kRsBase
constexpr uint32_t kRsMaxFill = (kRsBlocks - 1) * kRsChunk;  // samples a row can hold behind its history
constexpr uint32_t kRsRow = kRsBlocks * kRsChunk;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        size_t want = bytes + bytes / 4 + 4096;
        static const bool trace = std::getenv("SK_TICK_TRACE") != nullptr;
        const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        if (trace)
            std::fprintf(stderr, "sk_engine: device buffer regrown to %zu bytes in %.2f ms\n", want,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct StreamInfo {
    bool open = false;
    uint32_t sample_rate = 0;
    uint8_t channels = 0;
    int wide_slot = -1;  // streams of 3 ... 8 channels (sk_engine_enable_wide_pcm): which eight-row slot of the resampler rows is theirs
    // streaming resampler (soundkit-decoder lib.rs:1917-2060)
    bool rs_open = false;
    uint32_t rs_in_hz = 0, rs_out_hz = 0;
    int rs_table = -1;             // index into sk_engine::ratio_tables
    uint32_t rs_fill = 0;          // frames waiting in the chunk area
    uint64_t rs_chunks = 0;        // chunks already processed
    double rs_last_index = -128.0; // rubato SincFixedIn::last_index (relative to the next chunk's start)
};

// The time indices of one chunk's outputs in the form the generic kernel takes them (sk_device.h SincArgs): the index
// of every 128th output; the lanes redo the additions in between.
struct IndexSet {
    double last_in = 0.0, new_last = 0.0;  // rubato's last_index before / after the chunk
    uint32_t count = 0;
    std::vector<double> starts;
};

struct RatioTable {
    uint32_t in_hz = 0, out_hz = 0;
    double ratio = 0.0;
    float *d_sincs = nullptr;  // [256][256], then [256][256][2]: {sub-filter, the next one} interleaved
    // streaming: every stream of this ratio walks the same index sequence from -128, so chunk n's set is shared
    std::vector<IndexSet> chunk_sets;
};

// ---- constant tables --------------------------------------------------------------------------

void make_twiddle(int input_len, std::vector<float> &out) {  // dsp.rs:94-106
    const float nf = (float)input_len;
    const float output_scale = (1.0f / 32768.0f) / nf;
    const float twiddle_scale = std::sqrt(output_scale);
    const int fft_len = input_len / 2;
    out.resize(2 * (size_t)fft_len);
    for (int b = 0; b < fft_len; ++b) {
        const float angle = kPiF / nf * ((float)b + 0.125f);
        out[2 * b] = std::cos(angle) * twiddle_scale;
        out[2 * b + 1] = std::sin(angle) * twiddle_scale;
    }
}

void make_roots(int n, std::vector<float> &out) {  // e^{-2 pi i m / n}
    out.resize(2 * (size_t)n);
    for (int m = 0; m < n; ++m) {
        const double a = -2.0 * kPi * (double)m / (double)n;
        out[2 * m] = (float)std::cos(a);
        out[2 * m + 1] = (float)std::sin(a);
    }
}

void sine_window(int len, float *out) {  // dsp.rs:542-547
    const float scale = kPiF / (float)len;
    for (int i = 0; i < len; ++i) out[i] = std::sin(((float)i + 0.5f) * scale);
}

double bessel_i0(double x) {  // dsp.rs:572-587
    const double half = x * 0.5;
    double sum = 1.0, term = 1.0;
    for (int k = 1; k <= 64; ++k) {
        const double ratio = half / (double)k;
        term *= ratio * ratio;
        sum += term;
        if (std::fabs(term) < 1.0e-14 * sum) break;
    }
    return sum;
}

void kbd_window(int len, float alpha, float *out) {  // dsp.rs:549-570
    const int half = len / 2;
    std::vector<double> kernel((size_t)half + 1);
    const double denom_arg = kPi * (double)alpha;
    for (int i = 0; i <= half; ++i) {
        const double ratio = 2.0 * (double)i / (double)half - 1.0;
        double inner = 1.0 - ratio * ratio;
        if (inner < 0.0) inner = 0.0;
        kernel[i] = bessel_i0(denom_arg * std::sqrt(inner));
    }
    double total = 0.0;
    for (double v : kernel) total += v;
    double cumulative = 0.0;
    for (int i = 0; i < len; ++i) out[i] = 0.0f;
    for (int i = 0; i < half; ++i) {
        cumulative += kernel[i];
        out[i] = (float)std::sqrt(cumulative / total);
        out[len - 1 - i] = out[i];
    }
}

// rubato 0.14.1 make_sincs, T = f32, sinc_len 256, oversampling 256, BlackmanHarris2,
// cutoff 0.95 * ratio (ratio < 1): sub-filter 0 only (the one a zero fractional phase selects).
void make_taps_48k_16k(float *taps) {
    const size_t npoints = 256, factor = 256, tot = npoints * factor;
    const float f_cutoff = 0.95f * (float)(16000.0 / 48000.0);
    std::vector<float> y(tot);
    const float pi2 = 2.0f * kPiF, pi4 = 4.0f * kPiF, pi6 = 6.0f * kPiF, np_f = (float)tot;
    float sum = 0.0f;
    for (size_t x = 0; x < tot; ++x) {
        const float xf = (float)x;
        float w = 0.35875f - 0.48829f * std::cos(pi2 * xf / np_f) + 0.14128f * std::cos(pi4 * xf / np_f) -
                  0.01168f * std::cos(pi6 * xf / np_f);
        w = w * w;
        const float v = (xf - (float)(tot / 2)) * f_cutoff / (float)factor;
        const float sinc = v == 0.0f ? 1.0f : std::sin(v * kPiF) / (v * kPiF);
        const float val = w * sinc;
        sum += val;
        y[x] = val;
    }
    sum /= (float)factor;
    for (size_t p = 0; p < npoints; ++p) taps[p] = y[factor * p + (factor - 1)] / sum;  // sincs[0][p]
}

// rubato 0.14.1 make_sincs (T = f32): all 256 sub-filters of a ratio, sincs[sub][tap]
void make_sinc_table(double ratio, std::vector<float> &sincs) {
    const size_t npoints = 256, factor = 256, tot = npoints * factor;
    const float f_cutoff = ratio >= 1.0 ? 0.95f : 0.95f * (float)ratio;
    std::vector<float> y(tot);
    const float pi2 = 2.0f * kPiF, pi4 = 4.0f * kPiF, pi6 = 6.0f * kPiF, np_f = (float)tot;
    float sum = 0.0f;
    for (size_t x = 0; x < tot; ++x) {
        const float xf = (float)x;
        float w = 0.35875f - 0.48829f * std::cos(pi2 * xf / np_f) + 0.14128f * std::cos(pi4 * xf / np_f) -
                  0.01168f * std::cos(pi6 * xf / np_f);
        w = w * w;
        const float v = (xf - (float)(tot / 2)) * f_cutoff / (float)factor;
        const float sinc = v == 0.0f ? 1.0f : std::sin(v * kPiF) / (v * kPiF);
        const float val = w * sinc;
        sum += val;
        y[x] = val;
    }
    sum /= (float)factor;
    sincs.resize(tot);
    for (size_t p = 0; p < npoints; ++p)
        for (size_t n = 0; n < factor; ++n) sincs[(factor - n - 1) * npoints + p] = y[factor * p + n] / sum;
}

}  // namespace

struct sk_engine {
    int device = -1;
    hipStream_t stream = nullptr;
    uint32_t max_streams = 0;
    std::mutex mu;
    std::string last_hip_error;

    std::vector<StreamInfo> streams;
    std::vector<uint32_t> free_ids;

    float *d_delay = nullptr;
    uint8_t *d_prev_shape = nullptr;
    float *d_rs = nullptr;  // [max_streams * 2 + max_wide * 8][kRsRow] (kRsBlocks blocks of 4096), allocated on first sk_resampler_open
    // sk_engine_enable_wide_pcm: slots for streams of 3 ... 8 channels; slot w owns rows max_streams * 2 + w * 8 ... + 7 of d_rs
    uint32_t max_wide = 0;
    bool wide_enabled = false;
    std::vector<uint32_t> free_wide;
    uint32_t *d_wide_peak = nullptr;  // sk_pcm_downmix_dev: the one-call path's peak word
    // MP3 hybrid synthesis (mp3_hybrid.hip): tables and per-(stream, channel) state, allocated on first use
    float *d_mp3_tables = nullptr, *d_mp3_state = nullptr;
    bool mp3_window_set = false;
    // mp3_requant.hip: pow43 | root4 | is_k as floats, then the caller's band tables per sampling-rate slot
    uint8_t *d_mp3_rq = nullptr;
    uint16_t mp3_bands[sk::kMp3Rates][sk::kMp3BandRow] = {};  // [37] = long bands below line 36 (mixed blocks), 0xffff: none
    bool mp3_bands_set[sk::kMp3Rates] = {};
    // mp3_entropy.hip: the flattened code book (sk_mp3_set_codebook) on the device and as uploaded; frames | items | main data in,
    // cells | statuses out
    uint32_t *d_mp3_cb = nullptr;
    std::vector<uint32_t> mp3_cb_host;
    DevBuf mp3e_in, mp3e_out;

    // tables
    float *d_tables = nullptr;
    sk::SynthTables synth_tables{};
    float *d_pow43 = nullptr, *d_sftab = nullptr, *d_taps = nullptr, *d_zeros = nullptr;
    uint32_t *d_afrag16 = nullptr, *d_afrag_f16 = nullptr;
    std::vector<float> h_taps;
    std::vector<RatioTable> ratio_tables;

    // grow-only scratch
    DevBuf in_buf, out_buf, aux_buf, aux2_buf;
    DevBuf sinc_scratch;      // tap fragments of the matrix-core resampler (resample.hip), sized per launch
    bool sinc_exact = false;  // sk_engine_set_resampler_exact: the scalar form that keeps rubato's order of operations
    // sk_tick_run: synthesis output, resampler output, packed bytes, small-array arena (+ pinned host mirror)
    DevBuf tick_pcm, tick_res, tick_out, tick_arena, tick_au, tick_side, tick_q, tick_mp3_in, tick_mp3_xr, tick_mpa_in;
    DevBuf tick_pcm_in;  // sk_tick_run_pcm: the units' bytes as they came off the wire
    DevBuf flac_in, flac_ws, flac_out;  // sk_flac_decode_frames: frames | tables | statuses, planar i32 workspace | subframe records, PCM
    DevBuf alac_in, alac_ws, alac_out;  // sk_alac_decode_packets: packets | tables | statuses, planar i32 workspace | channel records, PCM
    DevBuf vorbis_in, vorbis_ws, vorbis_out, vorbis_tab;  // sk_vorbis_decode_packets: packets | blobs | tables | carried halves, residue | windowed PCM | classifications | records, PCM, the constants
    sk::VorbisTables vorbis_tables{};
    bool vorbis_tables_ready = false;
    DevBuf wav_tab;            // the WAV ADPCM decode stage: job table and per-block status
    DevBuf g72x_tab, g72x_ws;  // the telephony decode stage: stream / unit tables and state records, one word per G.722 byte
    DevBuf gsm_tab, gsm_ws;    // the GSM decode stage: stream / unit tables and state records, one s16 of short-term residual per sample
    DevBuf tick_aiff;    // sk_tick_run_aiff: the units decoded to the contract's PCM, what the PCM tick's body then reads
    // entropy decode on the device (sk_tick_run_au): per-stream PNS generator state and the front-end's tables
    uint32_t *d_pns = nullptr;
    void *d_ec_blob = nullptr;
    sk_ec::Tables ec_tables{};
    sk::EntropyArgs ec_args{};  // the table part of the kernel arguments (pointers, LDS blob layout)
    bool ec_ready = false;
    uint8_t *h_arena = nullptr;
    size_t h_arena_cap = 0;
    uint8_t *h_out = nullptr;     // pinned bounce buffer for a tick whose caller passed a pageable output buffer
    size_t h_out_cap = 0;
    int32_t *h_status = nullptr;  // pinned: the front-end's per-unit statuses come back here (a pageable destination would make
    size_t h_status_cap = 0;      // the "asynchronous" copy wait for the kernels inside the call, outside the tick's bounded wait)
    std::vector<uint32_t> state_count, state_task;  // plan construction scratch
    // streams opened (or reset) since the last launch: their device state is cleared by ONE launch in front of the next call
    // that touches the device (sk_stream_open used to cost a launch each: 4096 of them in front of a batch)
    std::vector<uint32_t> pending_reset;
    std::vector<uint32_t> pending_rs_reset;  // streams whose resampler rows are to be cleared (sk_resampler_open / sk_stream_reset)
    uint32_t *d_rs_reset_ids = nullptr;
    uint32_t *d_reset_ids = nullptr;
    // diagnostics: where the current tick stands (read by sk_pipeline_debug_dump without the engine's lock), the bound on
    // its waits for the device, and a failure-injection countdown for the error-path tests (sk_engine_debug_fail_after)
    std::atomic<const char *> where{"idle"};
    double sync_timeout_s = 120.0;
    std::atomic<int> fail_after{0};

    int hip_fail(hipError_t e, const char *what) {
        last_hip_error = std::string(what) + ": " + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? SK_ERR_OOM : SK_ERR_HIP;
    }
};

struct sk_aac_plan {
    sk_engine *eng = nullptr;
    uint32_t n_tasks = 0, n_entries = 0, n_frames_ok = 0;
    uint64_t elements = 0;
    sk::SynthTask *d_tasks = nullptr;
    sk::SynthEntry *d_entries = nullptr;
    sk::FrameSpan *d_spans = nullptr;
    // the tasks again, by the kernel that runs them (build_plan_host): two channels per wave without / with EightShort frames,
    // one channel per wave without / with them
    sk::SynthTask *d_pair_tasks = nullptr, *d_spair_tasks = nullptr, *d_long_tasks = nullptr, *d_walk_tasks = nullptr;
    uint32_t n_pair_tasks = 0, n_spair_tasks = 0, n_long_tasks = 0, n_walk_tasks = 0;
    uint32_t uniform_count = 0;     // frames of every task when they all have the same number (else 0)
    uint32_t uniform_channels = 0;  // channels of every stream in the plan when they all agree (else 0)
};

// First resampler row of an open stream in d_rs.  Narrow streams keep two rows each by id; a wide stream's eight lie behind them.
inline uint64_t rs_row0(const sk_engine *e, uint32_t id) {
    const int w = e->streams[id].wide_slot;
    return w < 0 ? (uint64_t)id * 2 : (uint64_t)e->max_streams * 2 + (uint64_t)w * 8;
}

#define SK_HIP(expr, what)                               \
    do {                                                  \
        hipError_t _e = (expr);                           \
        if (_e == hipSuccess && e->fail_after.load(std::memory_order_relaxed) > 0 && e->fail_after.fetch_sub(1) == 1) \
            _e = hipErrorLaunchFailure; /* injected by a test */ \
        if (_e != hipSuccess) return e->hip_fail(_e, what); \
    } while (0)

namespace {

// Engines of one process on one device never have a tick's device work in flight at the same time.  Found in round 4: with two
// engines (the scheduler's lanes) running their ticks concurrently on separate hardware queues, a third of 4096 identical streams
// came out with short bursts of slightly wrong samples (tools/debug/stream_hashes.py; none with GPU_MAX_HW_QUEUES=1, none with the
// ticks serialised, none with one engine).  Traced to the platform: packed-f32 instructions (the synthesis; stock rocFFT's as well)
// go wrong now and then while another wave of their CU executes v_mfma_f32_16x16x32_* (the FIR's) -- profiles/r04_lanes_corruption.md.
// The default build has no packed-f32 instructions any more (Makefile, PACKED_F32) and takes no turns; they stay for the build that
// has them: from the first upload of a tick to its last wait, per device.  The host's planning of a tick still overlaps the other engine's
// device work.  A process with one engine per device never waits here.
std::mutex g_device_turn[16];
std::atomic<int> g_engines_on_device[16];
// Only a library built WITH packed-f32 instructions (make PACKED_F32=1) needs the turns; the default build is immune, and there two
// lanes whose ticks overlap on the device are worth 7 % of the whole decode (11.2 -> 12.1 M access units/s, three alternations, every
// stream's hash and the bench's checksum unchanged: profiles/r04_lanes_corruption.md).  -DSK_NO_DEVICE_TURNS takes them out of a packed
// build to show what they prevent (tests/test_scale_gpu.py fails then).
#if defined(SK_NO_DEVICE_TURNS) || !SK_PACKED_F32
constexpr int kTurnFrom = 1 << 30;
#else
constexpr int kTurnFrom = 1;  // engines on a device beyond which they take turns
#endif

struct ComputeTurn {};  // tag: an entry point that launches transform or matrix-instruction kernels
struct DeviceGuard {
    explicit DeviceGuard(int dev) { (void)hipGetDevice(&prev); if (prev != dev) (void)hipSetDevice(dev); want = dev; }
    // the usual form at an entry point (engine lock held): the engine's device, and the state of the streams opened since
    // the last call is cleared before anything else is queued
    explicit DeviceGuard(sk_engine *e);
    // the same for an entry point that queues compute kernels outside a tick: while the process has several engines on the device
    // it also takes the device's turn (g_device_turn) and, before giving it back, waits for what it queued -- such a call is
    // synchronous then.  With one engine per device (the design) nothing is taken and nothing is waited for.
    DeviceGuard(sk_engine *e, ComputeTurn);
    ~DeviceGuard() {
        if (turn.owns_lock()) {
            (void)hipStreamSynchronize(turn_stream);  // an error stays on the stream: the next call of the engine reports it
            turn.unlock();
        }
        if (prev != want && prev >= 0) (void)hipSetDevice(prev);
    }
    int prev = -1, want = -1;
    std::unique_lock<std::mutex> turn;
    hipStream_t turn_stream = nullptr;
};

void flush_stream_resets(sk_engine *e) {
    hipError_t he = hipSuccess;
    if (!e->pending_rs_reset.empty() && e->d_rs) {  // the resampler rows of the streams opened since the last call, as spans of two rows: one launch
        const uint32_t n = (uint32_t)e->pending_rs_reset.size();
        if (!e->d_rs_reset_ids) he = hipMalloc((void **)&e->d_rs_reset_ids, ((size_t)e->max_streams + 4) * sizeof(uint32_t));
        if (he == hipSuccess) he = hipMemcpyAsync(e->d_rs_reset_ids, e->pending_rs_reset.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream);
        if (he == hipSuccess) he = sk::launch_zero_spans(e->d_rs, e->d_rs_reset_ids, n, 2 * kRsRow, e->stream);
        if (he != hipSuccess) (void)e->hip_fail(he, "reset resampler rows");
    }
    e->pending_rs_reset.clear();
    if (e->pending_reset.empty()) return;
    const uint32_t n = (uint32_t)e->pending_reset.size();
    he = hipSuccess;
    if (!e->d_reset_ids) he = hipMalloc((void **)&e->d_reset_ids, (size_t)e->max_streams * sizeof(uint32_t));
    // pageable source: the copy is staged before the call returns, the list can be reused at once
    if (he == hipSuccess) he = hipMemcpyAsync(e->d_reset_ids, e->pending_reset.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = sk::launch_reset_streams(e->d_delay, e->d_prev_shape, e->d_pns, e->d_reset_ids, n, e->stream);
    if (he == hipSuccess && e->d_mp3_state)  // the Layer III overlap and polyphase FIFO of both channels
        he = sk::launch_zero_spans(e->d_mp3_state, e->d_reset_ids, n, 2 * sk::kMp3StateFloats, e->stream);
    if (he != hipSuccess) (void)e->hip_fail(he, "reset stream state");  // the launch that follows reports it
    e->pending_reset.clear();
}

DeviceGuard::DeviceGuard(sk_engine *e) : DeviceGuard(e->device) { flush_stream_resets(e); }
DeviceGuard::DeviceGuard(sk_engine *e, ComputeTurn) : DeviceGuard(e->device) {
    if (g_engines_on_device[e->device & 15].load() > kTurnFrom) {
        turn = std::unique_lock<std::mutex>(g_device_turn[e->device & 15]);
        turn_stream = e->stream;
    }
    flush_stream_resets(e);
}

template <typename T>
hipError_t upload(T **dst, const std::vector<T> &src) {
    hipError_t e = hipMalloc((void **)dst, src.size() * sizeof(T));
    if (e != hipSuccess) return e;
    return hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
}

// IEEE binary16 <-> binary32 (round to nearest even, subnormals kept): the host side of the f16 tap planes
uint16_t f32_to_f16_rn(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);  // >= 65536 (not reached: taps * 2^16 < 2^15)
    if (x < 0x38800000u) {                                     // below 2^-14: subnormal half, in units of 2^-24
        float a;
        std::memcpy(&a, &x, 4);
        const float scaled = a * 16777216.0f;                  // exact
        const uint32_t q = (uint32_t)std::nearbyint(scaled);   // default rounding mode: to nearest even
        return (uint16_t)(sign | q);
    }
    const uint32_t mant = x & 0x7fffffu, exp = (x >> 23) - 112;
    uint32_t h = (exp << 10) | (mant >> 13);
    const uint32_t rem = mant & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;  // a carry out of the mantissa moves into the exponent: still right
    return (uint16_t)(sign | h);
}
float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 31u, mant = h & 0x3ffu;
    float v;
    if (exp == 0) v = (float)mant * (1.0f / 16777216.0f);
    else {
        const uint32_t bits = ((exp + 112) << 23) | (mant << 13);
        std::memcpy(&v, &bits, 4);
    }
    return sign ? -v : v;
}

int build_tables(sk_engine *e) {
    std::vector<float> tw_long, tw_short, w64, w512;
    make_twiddle(1024, tw_long);
    make_twiddle(128, tw_short);
    make_roots(64, w64);
    make_roots(512, w512);
    std::vector<float> win(2048 * 2 + 256 * 2 + 4 * 1024);
    sine_window(2048, win.data());
    kbd_window(2048, 4.0f, win.data() + 2048);
    sine_window(256, win.data() + 4096);
    kbd_window(256, 6.0f, win.data() + 4096 + 256);
    // the piecewise halves of the two transition sequences as tables (dsp.rs:353-387), so that LongStart / LongStop frames
    // run the OnlyLong code with another window pointer: [4608 + 1024 shape] = LongStart's second half {1 | short[128..256) | 0},
    // [6656 + 1024 shape] = LongStop's first half {0 | short[0..128) | 1}
    for (int shape = 0; shape < 2; ++shape) {
        const float *sh = win.data() + 4096 + 256 * shape;
        float *start2 = win.data() + 4608 + 1024 * shape, *stop1 = win.data() + 6656 + 1024 * shape;
        for (int i = 0; i < 1024; ++i) {
            start2[i] = i < 448 ? 1.0f : (i < 576 ? sh[128 + i - 448] : 0.0f);
            stop1[i] = i < 448 ? 0.0f : (i < 576 ? sh[i - 448] : 1.0f);
        }
    }

    std::vector<float> all;
    const size_t o_twl = 0, o_tws = o_twl + tw_long.size(), o_w64 = o_tws + tw_short.size(),
                 o_w512 = o_w64 + w64.size(), o_win = o_w512 + w512.size();
    all.insert(all.end(), tw_long.begin(), tw_long.end());
    all.insert(all.end(), tw_short.begin(), tw_short.end());
    all.insert(all.end(), w64.begin(), w64.end());
    all.insert(all.end(), w512.begin(), w512.end());
    all.insert(all.end(), win.begin(), win.end());
    SK_HIP(upload(&e->d_tables, all), "upload synthesis tables");
    e->synth_tables.tw_long = reinterpret_cast<const float2 *>(e->d_tables + o_twl);
    e->synth_tables.tw_short = reinterpret_cast<const float2 *>(e->d_tables + o_tws);
    e->synth_tables.w64 = reinterpret_cast<const float2 *>(e->d_tables + o_w64);
    e->synth_tables.w512 = reinterpret_cast<const float2 *>(e->d_tables + o_w512);
    e->synth_tables.win = e->d_tables + o_win;

    std::vector<float> pow43(8192), sftab(768);  // dsp.rs:420-450
    for (int v = 0; v < 8192; ++v) pow43[v] = std::pow((float)v, 4.0f / 3.0f);
    for (int sf = -256; sf <= 511; ++sf) sftab[sf + 256] = std::pow(2.0f, ((float)sf - 100.0f) * 0.25f);
    SK_HIP(upload(&e->d_pow43, pow43), "upload pow43");
    SK_HIP(upload(&e->d_sftab, sftab), "upload scalefactor table");

    e->h_taps.resize(256);
    make_taps_48k_16k(e->h_taps.data());
    SK_HIP(upload(&e->d_taps, e->h_taps), "upload taps");
    // bf16 A fragments (fir_bf16.hip): h = h1 + h2 + h3 exactly, each the top 16 bits of an f32 (truncation);
    // window s, plane k, lane l (i = l & 15, q = l >> 4), element e: tap p = 32 s + 8 q + e - 3 i - 3
    std::vector<uint32_t> afrag16((size_t)10 * 3 * 64 * 4, 0u);
    for (int s = 0; s < 10; ++s)
        for (int l = 0; l < 64; ++l)
            for (int el = 0; el < 8; ++el) {
                const int p = 32 * s + 8 * (l >> 4) + el - 3 * (l & 15) - 3;
                if (p < 0 || p >= 256) continue;
                float rest = e->h_taps[p];
                for (int k = 0; k < 3; ++k) {
                    uint32_t bits;
                    std::memcpy(&bits, &rest, 4);
                    bits &= 0xffff0000u;
                    float piece;
                    std::memcpy(&piece, &bits, 4);
                    rest -= piece;  // exact: the piece is the leading 8 significand bits of rest
                    afrag16[((size_t)(s * 3 + k) * 64 + l) * 4 + el / 2] |= (bits >> 16) << (16 * (el & 1));
                }
            }
    SK_HIP(upload(&e->d_afrag16, afrag16), "upload bf16 tap fragments");
    // f16 A fragments for s16 rows: h * 2^16 = h1 + h2 + r with h1 = f16(h * 2^16), h2 = f16(h * 2^16 - h1), both rounded to
    // nearest (|r| <= 2^-24 |h1|, or 2^-25 absolute where h2 is subnormal); same window / lane / element layout, two planes
    std::vector<uint32_t> afrag_f16((size_t)10 * 2 * 64 * 4, 0u);
    for (int s = 0; s < 10; ++s)
        for (int l = 0; l < 64; ++l)
            for (int el = 0; el < 8; ++el) {
                const int p = 32 * s + 8 * (l >> 4) + el - 3 * (l & 15) - 3;
                if (p < 0 || p >= 256) continue;
                float rest = e->h_taps[p] * 65536.0f;  // exact
                for (int k = 0; k < 2; ++k) {
                    const uint16_t hbits = f32_to_f16_rn(rest);
                    rest -= f16_to_f32(hbits);  // exact: the piece is rest rounded to 11 significand bits
                    afrag_f16[((size_t)(s * 2 + k) * 64 + l) * 4 + el / 2] |= (uint32_t)hbits << (16 * (el & 1));
                }
            }
    SK_HIP(upload(&e->d_afrag_f16, afrag_f16), "upload f16 tap fragments");
    std::vector<float> zeros(8192, 0.0f);
    SK_HIP(upload(&e->d_zeros, zeros), "upload zeros");
    return SK_OK;
}

// shared shape of every host-buffer PCM entry point: H2D, one launch, D2H, sync
template <typename Launch>
int host_roundtrip(sk_engine *e, const void *in, size_t in_bytes, void *out, size_t out_bytes, Launch launch) {
    if (!e || (in_bytes && !in) || (out_bytes && !out)) return SK_ERR_INVALID_ARG;
    if (out_bytes == 0) return SK_OK;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    SK_HIP(e->in_buf.reserve(in_bytes), "alloc staging");
    SK_HIP(e->out_buf.reserve(out_bytes), "alloc staging");
    SK_HIP(hipMemcpyAsync(e->in_buf.p, in, in_bytes, hipMemcpyHostToDevice, e->stream), "H2D pcm");
    SK_HIP(launch(e->in_buf.p, e->out_buf.p), "launch pcm kernel");
    SK_HIP(hipMemcpyAsync(out, e->out_buf.p, out_bytes, hipMemcpyDeviceToHost, e->stream), "D2H pcm");
    SK_HIP(hipStreamSynchronize(e->stream), "pcm sync");
    return SK_OK;
}

bool stream_ok(const sk_engine *e, uint32_t id) { return id < e->streams.size() && e->streams[id].open; }

}  // namespace

extern "C" {

const char *sk_version(void) try {
    sk::abi_enter();
    return "soundkit_amd 0.1.0 (gfx950)";
} catch (...) {
    (void)sk::abi_caught("sk_version");
    return sk::abi_message();
}

const char *sk_strerror(int status) try {
    sk::abi_enter();
    switch (status) {
    case SK_OK: return "ok";
    case SK_ERR_INVALID_ARG: return "invalid argument";
    case SK_ERR_NO_DEVICE: return "no usable HIP device";
    case SK_ERR_HIP: return "HIP runtime error";
    case SK_ERR_OOM: return "out of memory (device or host)";
    case SK_ERR_BAD_STREAM: return "stream is not open";
    case SK_ERR_UNSUPPORTED: return "unsupported configuration";
    case SK_ERR_CAPACITY: return "capacity exhausted (streams, handles or caller buffer)";
    case SK_PIPE_INPUT_FULL: return "Input buffer full";
    case SK_PIPE_CLOSED: return "Decode pipeline is closed";
    case SK_PIPE_CHUNK_TOO_LARGE: return "Input chunk exceeds the 4 MiB limit";
    case SK_AAC_ERR_EOF: return "unexpected end of AAC bitstream";
    case SK_AAC_ERR_INVALID_AOT: return "invalid AAC audio object type";
    case SK_AAC_ERR_UNSUPPORTED_AOT: return "unsupported AAC audio object type";
    case SK_AAC_ERR_UNSUPPORTED_SF_INDEX: return "unsupported AAC sampling frequency index";
    case SK_AAC_ERR_UNSUPPORTED_CHANNEL_CONFIG: return "unsupported AAC channel configuration";
    case SK_ERR_TIMEOUT: return "the device did not finish in time";
    case SK_ERR_INTERNAL: return "internal error (a C++ exception was caught at the ABI)";
    case SK_MP3_NEED_MORE: return "more MP3 input needed";
    case SK_MP3_NO_SYNC: return "not an MPEG audio frame header";
    case SK_MP3_UNSUPPORTED: return "unsupported MPEG audio layer or feature";
    case SK_MP3_INVALID: return "invalid MP3 side information";
    case SK_PCM_ERR_STREAM: return "WAV / raw PCM stream rejected";
    case SK_FLAC_NEED_MORE: return "more FLAC input needed";
    case SK_FLAC_NO_SYNC: return "not a FLAC frame header";
    case SK_FLAC_RESERVED: return "reserved value in a FLAC frame header";
    case SK_FLAC_BAD_CRC: return "FLAC CRC mismatch";
    case SK_FLAC_NEED_STREAMINFO: return "FLAC frame header refers to a STREAMINFO that was not given";
    case SK_FLAC_INVALID: return "invalid FLAC frame";
    case SK_FLAC_ERR_STREAM: return "FLAC stream rejected";
    case SK_ALAC_INVALID: return "invalid ALAC packet";
    case SK_ALAC_ERR_STREAM: return "ALAC stream rejected";
    case SK_ALAC_UNSUPPORTED: return "unsupported ALAC element";
    case SK_G72X_ERR_STREAM: return "telephony stream rejected";
    case SK_VORBIS_NOT_AUDIO: return "not a Vorbis audio packet";
    case SK_VORBIS_BAD_MODE: return "Vorbis packet names a mode the setup does not have";
    case SK_VORBIS_SHORT: return "Vorbis packet ends inside its first bits";
    case SK_VORBIS_ERR_STREAM: return "Ogg / Vorbis stream rejected";
    case SK_MP4_ERR_STREAM: return "MP4 stream rejected";
    case SK_CAF_ERR_STREAM: return "CAF stream rejected";
    case SK_WEBM_ERR_STREAM: return "WebM stream rejected";
    case SK_TS_ERR_STREAM: return "MPEG-TS stream rejected";
    case SK_AVI_ERR_STREAM: return "AVI stream rejected";
    case SK_PS_ERR_STREAM: return "MPEG-PS stream rejected";
    case SK_WAV_BAD_BLOCK: return "WAV ADPCM block header is invalid";
    case SK_AAC_ERR_UNSUPPORTED_FEATURE: return "unsupported AAC feature";
    case SK_AAC_ERR_INVALID_CONFIG: return "invalid AAC config";
    case SK_AAC_ERR_INVALID_BITSTREAM: return "invalid AAC bitstream";
    default: return "unknown status";
    }
} catch (...) {
    (void)sk::abi_caught("sk_strerror");
    return sk::abi_message();
}

int sk_engine_create(int device, uint32_t max_streams, sk_engine **out) try {
    sk::abi_enter();
    if (!out || max_streams == 0) return SK_ERR_INVALID_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return SK_ERR_NO_DEVICE;
    sk_engine *e = new (std::nothrow) sk_engine();
    if (!e) return SK_ERR_OOM;
    e->device = device;
    e->max_streams = max_streams;
    g_engines_on_device[device & 15].fetch_add(1);
    DeviceGuard guard(device);
    int rc = SK_OK;
    do {
        hipError_t he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
        if (he != hipSuccess) { rc = e->hip_fail(he, "hipStreamCreate"); break; }
        const size_t states = (size_t)max_streams * 2;
        he = hipMalloc((void **)&e->d_delay, states * 1024 * sizeof(float));
        if (he != hipSuccess) { rc = e->hip_fail(he, "alloc delay"); break; }
        he = hipMalloc((void **)&e->d_prev_shape, states);
        if (he != hipSuccess) { rc = e->hip_fail(he, "alloc prev_shape"); break; }
        (void)hipMemset(e->d_delay, 0, states * 1024 * sizeof(float));
        (void)hipMemset(e->d_prev_shape, 0, states);
        he = hipMalloc((void **)&e->d_pns, (size_t)max_streams * sizeof(uint32_t));
        if (he != hipSuccess) { rc = e->hip_fail(he, "alloc pns state"); break; }
        rc = build_tables(e);
        if (rc != SK_OK) break;
        e->streams.resize(max_streams);
        e->free_ids.reserve(max_streams);
        for (uint32_t i = max_streams; i-- > 0;) e->free_ids.push_back(i);
        e->state_count.assign(states, 0);
        e->state_task.assign(states, 0);
    } while (0);
    if (rc != SK_OK) {
        sk_engine_destroy(e);
        return rc;
    }
    *out = e;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_engine_create");
}

void sk_engine_destroy(sk_engine *e) try {
    sk::abi_enter();
    if (!e) return;
    g_engines_on_device[e->device & 15].fetch_sub(1);
    {
        DeviceGuard guard(e);
        if (e->stream) (void)hipStreamSynchronize(e->stream);
        if (e->d_reset_ids) (void)hipFree(e->d_reset_ids);
        if (e->d_rs_reset_ids) (void)hipFree(e->d_rs_reset_ids);
        e->sinc_scratch.release();
        for (void *p : {(void *)e->d_mp3_rq, (void *)e->d_mp3_tables, (void *)e->d_mp3_state, (void *)e->d_pns, e->d_ec_blob, (void *)e->d_delay, (void *)e->d_prev_shape, (void *)e->d_rs, (void *)e->d_wide_peak, (void *)e->d_tables,
                        (void *)e->d_pow43, (void *)e->d_sftab, (void *)e->d_taps, (void *)e->d_afrag16, (void *)e->d_afrag_f16,
                        (void *)e->d_zeros})
            if (p) (void)hipFree(p);
        for (RatioTable &t : e->ratio_tables)
            if (t.d_sincs) (void)hipFree(t.d_sincs);
        e->in_buf.release();
        e->out_buf.release();
        e->aux_buf.release();
        e->aux2_buf.release();
        e->tick_pcm.release();
        e->tick_res.release();
        e->tick_out.release();
        e->tick_arena.release();
        e->tick_au.release();
        e->tick_side.release();
        e->tick_q.release();
        e->tick_pcm_in.release();
        e->tick_aiff.release();
        e->flac_in.release();
        e->flac_ws.release();
        e->flac_out.release();
        e->alac_in.release();
        e->alac_ws.release();
        e->alac_out.release();
        e->vorbis_in.release();
        e->vorbis_ws.release();
        e->vorbis_out.release();
        e->vorbis_tab.release();
        e->g72x_tab.release();
        e->wav_tab.release();
        e->g72x_ws.release();
        e->gsm_tab.release();
        e->gsm_ws.release();
        e->mp3e_in.release();
        e->tick_mpa_in.release();
        e->mp3e_out.release();
        if (e->d_mp3_cb) (void)hipFree(e->d_mp3_cb);
        if (e->h_arena) (void)hipHostFree(e->h_arena);
        if (e->h_status) (void)hipHostFree(e->h_status);
        if (e->h_out) (void)hipHostFree(e->h_out);
        if (e->stream) (void)hipStreamDestroy(e->stream);
    }
    delete e;
} catch (...) {
    (void)sk::abi_caught("sk_engine_destroy");
}

int sk_engine_device(const sk_engine *e) try {
    sk::abi_enter();
    return e ? e->device : -1;
} catch (...) {
    return sk::abi_caught("sk_engine_device");
}
int sk_engine_enable_wide_pcm(sk_engine *e, uint32_t max_wide_streams) try {
    sk::abi_enter();
    if (!e) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    // once, and before the resampler rows exist: their allocation (the first sk_resampler_open) is sized by this
    if (e->wide_enabled || e->d_rs || max_wide_streams == 0 || max_wide_streams > e->max_streams) return SK_ERR_INVALID_ARG;
    e->free_wide.reserve(max_wide_streams);
    for (uint32_t i = max_wide_streams; i-- > 0;) e->free_wide.push_back(i);
    e->max_wide = max_wide_streams;
    e->wide_enabled = true;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_engine_enable_wide_pcm");
}

uint32_t sk_engine_wide_pcm_streams(const sk_engine *e) try {
    sk::abi_enter();
    return e ? e->max_wide : 0;
} catch (...) {
    (void)sk::abi_caught("sk_engine_wide_pcm_streams");
    return 0;
}

uint32_t sk_engine_max_streams(const sk_engine *e) try {
    sk::abi_enter();
    return e ? e->max_streams : 0;
} catch (...) {
    (void)sk::abi_caught("sk_engine_max_streams");
    return 0;
}
void *sk_engine_hip_stream(sk_engine *e) try {
    sk::abi_enter();
    return e ? (void *)e->stream : nullptr;
} catch (...) {
    (void)sk::abi_caught("sk_engine_hip_stream");
    return nullptr;
}
int sk_kernels_use_packed_f32(void) try {
    return SK_PACKED_F32;
} catch (...) {
    return sk::abi_caught("sk_kernels_use_packed_f32");
}

const char *sk_engine_last_hip_error(const sk_engine *e) try {
    sk::abi_enter();
    return e ? e->last_hip_error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_engine_last_hip_error");
    return sk::abi_message();
}

const char *sk_engine_where(const sk_engine *e) try {
    sk::abi_enter();
    return e ? e->where.load() : "";
} catch (...) {
    (void)sk::abi_caught("sk_engine_where");
    return sk::abi_message();
}

int sk_engine_debug_fail_after(sk_engine *e, int n_hip_calls) try {
    sk::abi_enter();
    if (!e || n_hip_calls < 0) return SK_ERR_INVALID_ARG;
    e->fail_after.store(n_hip_calls);
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_engine_debug_fail_after");
}

int sk_engine_set_resampler_exact(sk_engine *e, int exact) try {
    sk::abi_enter();
    if (!e) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    e->sinc_exact = exact != 0;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_engine_set_resampler_exact");
}

int sk_engine_set_wait_bound(sk_engine *e, double seconds) try {
    sk::abi_enter();
    if (!e || !(seconds > 0.0)) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    e->sync_timeout_s = seconds;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_engine_set_wait_bound");
}

int sk_engine_synchronize(sk_engine *e) try {
    sk::abi_enter();
    if (!e) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    SK_HIP(hipStreamSynchronize(e->stream), "stream synchronize");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_engine_synchronize");
}

// ---- streams --------------------------------------------------------------------------------

// queues the clearing of a stream's resampler rows (flush_stream_resets): spans of two rows, one for a narrow stream, four for a wide one
static void queue_rs_reset(sk_engine *e, uint32_t id) {
    const uint32_t span0 = (uint32_t)(rs_row0(e, id) / 2), n = e->streams[id].wide_slot < 0 ? 1 : 4;
    for (uint32_t k = 0; k < n; ++k) e->pending_rs_reset.push_back(span0 + k);
    if (e->pending_rs_reset.size() >= e->max_streams) flush_stream_resets(e);
}

static int reset_stream_state(sk_engine *e, uint32_t id) {
    // overlap delay, previous window shape and PNS generator (spectral.rs:2459): queued, cleared by one launch for all the
    // streams opened in a row (flush_stream_resets, in front of the next call that touches the device)
    e->pending_reset.push_back(id);
    if (e->pending_reset.size() >= e->max_streams) flush_stream_resets(e);  // ids repeat only across open / close cycles
    return SK_OK;
}

int sk_stream_open(sk_engine *e, uint32_t sample_rate, uint8_t channels, uint32_t *stream_out) try {
    sk::abi_enter();
    if (!e || !stream_out || channels < 1 || channels > SK_MAX_PCM_CHANNELS || sample_rate == 0) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    const bool wide = channels > SK_MAX_CHANNELS;  // PCM only, and only on an engine that reserved slots for them
    if (wide && !e->wide_enabled) return SK_ERR_INVALID_ARG;
    if (e->free_ids.empty() || (wide && e->free_wide.empty())) return SK_ERR_CAPACITY;
    const uint32_t id = e->free_ids.back();
    int rc = reset_stream_state(e, id);
    if (rc != SK_OK) return rc;
    e->free_ids.pop_back();
    StreamInfo &s = e->streams[id];
    s = StreamInfo();
    s.open = true;
    s.sample_rate = sample_rate;
    s.channels = channels;
    if (wide) s.wide_slot = (int)e->free_wide.back(), e->free_wide.pop_back();
    *stream_out = id;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_stream_open");
}

int sk_stream_close(sk_engine *e, uint32_t id) try {
    sk::abi_enter();
    if (!e) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    if (!stream_ok(e, id)) return SK_ERR_BAD_STREAM;
    if (e->streams[id].wide_slot >= 0) e->free_wide.push_back((uint32_t)e->streams[id].wide_slot);
    e->streams[id] = StreamInfo();
    e->free_ids.push_back(id);
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_stream_close");
}

int sk_stream_reset(sk_engine *e, uint32_t id) try {
    sk::abi_enter();
    if (!e) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    if (!stream_ok(e, id)) return SK_ERR_BAD_STREAM;
    DeviceGuard guard(e);
    StreamInfo &s = e->streams[id];
    s.rs_fill = 0;
    s.rs_chunks = 0;
    s.rs_last_index = -128.0;
    if (s.rs_open && e->d_rs) queue_rs_reset(e, id);  // cleared with the next call's first launch (flush_stream_resets)
    return reset_stream_state(e, id);
} catch (...) {
    return sk::abi_caught("sk_stream_reset");
}

int sk_stream_get_state(sk_engine *e, uint32_t id, float *delay_out, uint8_t *prev_shape_out) try {
    sk::abi_enter();
    if (!e || !delay_out || !prev_shape_out) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    if (!stream_ok(e, id)) return SK_ERR_BAD_STREAM;
    if (e->streams[id].channels > SK_MAX_CHANNELS) return SK_ERR_INVALID_ARG;  // a wide PCM stream has no synthesis state
    DeviceGuard guard(e);
    const uint32_t ch = e->streams[id].channels;
    SK_HIP(hipMemcpyAsync(delay_out, e->d_delay + (size_t)id * 2048, ch * 1024 * sizeof(float), hipMemcpyDeviceToHost,
                          e->stream), "get delay");
    SK_HIP(hipMemcpyAsync(prev_shape_out, e->d_prev_shape + (size_t)id * 2, ch, hipMemcpyDeviceToHost, e->stream),
           "get shape");
    SK_HIP(hipStreamSynchronize(e->stream), "get state sync");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_stream_get_state");
}

int sk_stream_set_state(sk_engine *e, uint32_t id, const float *delay, const uint8_t *prev_shape) try {
    sk::abi_enter();
    if (!e || !delay || !prev_shape) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    if (!stream_ok(e, id)) return SK_ERR_BAD_STREAM;
    if (e->streams[id].channels > SK_MAX_CHANNELS) return SK_ERR_INVALID_ARG;  // a wide PCM stream has no synthesis state
    const uint32_t ch = e->streams[id].channels;
    for (uint32_t c = 0; c < ch; ++c)
        if (prev_shape[c] > 1) return SK_ERR_INVALID_ARG;
    DeviceGuard guard(e);
    SK_HIP(hipMemcpyAsync(e->d_delay + (size_t)id * 2048, delay, ch * 1024 * sizeof(float), hipMemcpyHostToDevice,
                          e->stream), "set delay");
    SK_HIP(hipMemcpyAsync(e->d_prev_shape + (size_t)id * 2, prev_shape, ch, hipMemcpyHostToDevice, e->stream),
           "set shape");
    SK_HIP(hipStreamSynchronize(e->stream), "set state sync");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_stream_set_state");
}

// ---- AAC synthesis ----------------------------------------------------------------------------

void sk_aac_plan_destroy(sk_aac_plan *p) try {
    sk::abi_enter();
    if (!p) return;
    if (p->eng) {
        DeviceGuard guard(p->eng->device);
        if (p->d_tasks) (void)hipFree(p->d_tasks);
        if (p->d_entries) (void)hipFree(p->d_entries);
        if (p->d_spans) (void)hipFree(p->d_spans);
        if (p->d_walk_tasks) (void)hipFree(p->d_walk_tasks);
        if (p->d_long_tasks) (void)hipFree(p->d_long_tasks);
        if (p->d_pair_tasks) (void)hipFree(p->d_pair_tasks);
        if (p->d_spair_tasks) (void)hipFree(p->d_spair_tasks);
    }
    delete p;
} catch (...) {
    (void)sk::abi_caught("sk_aac_plan_destroy");
}

uint64_t sk_aac_plan_elements(const sk_aac_plan *p) try {
    sk::abi_enter();
    return p ? p->elements : 0;
} catch (...) {
    (void)sk::abi_caught("sk_aac_plan_elements");
    return 0;
}
uint32_t sk_aac_plan_frames_ok(const sk_aac_plan *p) try {
    sk::abi_enter();
    return p ? p->n_frames_ok : 0;
} catch (...) {
    (void)sk::abi_caught("sk_aac_plan_frames_ok");
    return 0;
}

}  // extern "C"

namespace {

struct HostPlan {
    std::vector<sk::SynthTask> tasks;
    std::vector<sk::SynthEntry> entries;
    std::vector<sk::FrameSpan> spans;
    std::vector<uint32_t> entry_of;  // [frame * 2 + channel] -> index into entries (valid frames only)
    // `tasks` again, by kernel (see the end of build_plan_host)
    std::vector<sk::SynthTask> pair_tasks, spair_tasks, long_tasks, walk_tasks;
    uint32_t uniform_count = 0, uniform_channels = 0;  // see sk_aac_plan
    uint32_t frames_ok = 0;
    uint64_t off1024 = 0;  // total packed size in units of 1024 f32
};

// Validates the descs and lays the batch out as one task per (stream, channel) state, frames of a state in
// array order.  Caller holds e->mu.
int build_plan_host(sk_engine *e, const sk_aac_frame_desc *descs, uint32_t n, int32_t *status, HostPlan &hp, bool windows_known = true) {
    // pass 1: validate, count entries per (stream, channel) state, in first-touch order
    std::vector<uint32_t> touched;
    std::vector<uint8_t> ok(n, 0);
    uint32_t frames_ok = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const sk_aac_frame_desc &d = descs[i];
        int32_t st = SK_FRAME_OK;
        if (!stream_ok(e, d.stream)) st = SK_FRAME_BAD_STREAM;
        else if (d.channels != e->streams[d.stream].channels || d.channels > SK_MAX_CHANNELS) st = SK_FRAME_BAD_CHANNELS;
        else {
            for (uint32_t c = 0; c < d.channels; ++c)
                if (d.window_sequence[c] > 3 || d.window_shape[c] > 1) st = SK_FRAME_BAD_WINDOW;
        }
        if (status) status[i] = st;
        if (st != SK_FRAME_OK) continue;
        ok[i] = 1;
        ++frames_ok;
        for (uint32_t c = 0; c < d.channels; ++c) {
            const uint32_t state = d.stream * 2 + c;
            if (e->state_count[state]++ == 0) touched.push_back(state);
        }
    }
    // tasks in first-touch order; entries grouped per task, array order kept inside a task
    std::vector<sk::SynthTask> &tasks = hp.tasks;
    tasks.assign(touched.size(), sk::SynthTask{});
    uint32_t n_entries = 0;
    for (size_t t = 0; t < touched.size(); ++t) {
        const uint32_t state = touched[t];
        tasks[t].state = state;
        tasks[t].begin = n_entries;
        tasks[t].count = 0;
        tasks[t].pad = 0;
        n_entries += e->state_count[state];
        e->state_task[state] = (uint32_t)t;
    }
    std::vector<sk::SynthEntry> &entries = hp.entries;
    entries.assign(n_entries, sk::SynthEntry{});
    std::vector<sk::FrameSpan> &spans = hp.spans;
    spans.clear();
    spans.reserve(frames_ok);
    hp.entry_of.assign((size_t)n * 2, 0);
    uint64_t off = 0;  // in units of 1024 f32; advances for failed frames too (packing follows the descs)
    bool bad_desc_channels = false;
    for (uint32_t i = 0; i < n; ++i) {
        const sk_aac_frame_desc &d = descs[i];
        if (ok[i]) {
            for (uint32_t c = 0; c < d.channels; ++c) {
                sk::SynthTask &t = tasks[e->state_task[d.stream * 2 + c]];
                hp.entry_of[(size_t)i * 2 + c] = t.begin + t.count;
                sk::SynthEntry &en = entries[t.begin + t.count++];
                en.off1024 = (uint32_t)(off + c);
                en.win = (uint32_t)d.window_sequence[c] | ((uint32_t)d.window_shape[c] << 2);
            }
            spans.push_back(sk::FrameSpan{(uint32_t)off, d.channels});
        }
        if (d.channels < 1 || d.channels > SK_MAX_CHANNELS) bad_desc_channels = true;
        off += d.channels;
    }
    for (uint32_t state : touched) e->state_count[state] = 0;
    if (bad_desc_channels || off > 0xffffffffull) return SK_ERR_INVALID_ARG;
    hp.frames_ok = frames_ok;
    hp.off1024 = off;
    hp.uniform_count = tasks.empty() ? 0 : tasks[0].count;
    for (const sk::SynthTask &t : tasks)
        if (t.count != hp.uniform_count) hp.uniform_count = 0;
    hp.uniform_channels = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (ok[i]) {
            if (!hp.uniform_channels) hp.uniform_channels = descs[i].channels;
            else if (hp.uniform_channels != descs[i].channels) {
                hp.uniform_channels = 0xffu;  // mixed
            }
        }
    if (hp.uniform_channels == 0xffu) hp.uniform_channels = 0;
    // Which kernel runs which task (dsp.rs:230-338: OnlyLong, LongStart and LongStop are one code path here -- the transition
    // windows are tables -- so only EightShort frames tell tasks apart):
    //   pair_tasks   two tasks of equal length without an EightShort frame share a wave (k_aac_synth_pair): normally the L and
    //                R of a stream; a task meets the nearest earlier task of its length that is still alone
    //   spair_tasks  the same for two tasks whose EightShort frames fall on the SAME frame numbers (a channel pair coded with
    //                a common window -- the usual case -- switches both channels together): the pair kernel with a wave-uniform
    //                eight-short arm.  One EightShort frame no longer sends all of a channel's frames to the one-channel kernel
    //   long_tasks   without EightShort frames, no partner: the straight-line one-channel kernel
    //   walk_tasks   everything else (and every task when the windows are not known yet: the device front-end fills them in)
    // SK_SYNTH_PAIRS=0: no pairs at all (A/B runs).
    static const bool use_pairs = [] { const char *v = std::getenv("SK_SYNTH_PAIRS"); return !(v && v[0] == '0'); }();
    hp.pair_tasks.clear();
    hp.spair_tasks.clear();
    hp.long_tasks.clear();
    hp.walk_tasks.clear();
    {
        struct Key {
            uint32_t count;
            uint64_t shorts;  // hash of the frame numbers that are EightShort (0: none)
            bool operator==(const Key &o) const { return count == o.count && shorts == o.shorts; }
        };
        struct KeyHash {
            size_t operator()(const Key &k) const { return (size_t)(k.shorts * 0x9e3779b97f4a7c15ull ^ k.count); }
        };
        std::unordered_map<Key, uint32_t, KeyHash> waiting;  // -> task index, still alone
        std::vector<Key> keys(tasks.size());
        std::vector<int32_t> partner(tasks.size(), -1);
        for (uint32_t t = 0; t < tasks.size(); ++t) {
            uint64_t h = 0;
            for (uint32_t k = 0; windows_known && k < tasks[t].count; ++k)
                if ((entries[tasks[t].begin + k].win & 3u) == 2u) h = (h ^ (k + 1)) * 0x100000001b3ull + 0x9e3779b9u;
            keys[t] = Key{tasks[t].count, h};
            if (!windows_known || !use_pairs) continue;
            auto it = waiting.find(keys[t]);
            if (it == waiting.end()) {
                waiting.emplace(keys[t], t);
                continue;
            }
            // equal hashes are not yet equal patterns: compare the frames themselves
            const uint32_t u = it->second;
            bool same = true;
            for (uint32_t k = 0; same && keys[t].shorts && k < tasks[t].count; ++k)
                same = ((entries[tasks[t].begin + k].win & 3u) == 2u) == ((entries[tasks[u].begin + k].win & 3u) == 2u);
            if (!same) continue;
            partner[t] = (int32_t)u;
            partner[u] = (int32_t)t;
            waiting.erase(it);
        }
        for (uint32_t t = 0; t < tasks.size(); ++t) {
            const bool has_short = !windows_known || keys[t].shorts != 0;
            if (partner[t] >= 0) {
                if ((uint32_t)partner[t] < t) continue;  // listed with its partner
                std::vector<sk::SynthTask> &dst = has_short ? hp.spair_tasks : hp.pair_tasks;
                dst.push_back(tasks[t]);
                dst.push_back(tasks[(uint32_t)partner[t]]);
            } else if (has_short) {
                hp.walk_tasks.push_back(tasks[t]);
            } else {
                hp.long_tasks.push_back(tasks[t]);
            }
        }
    }
    return SK_OK;
}

}  // namespace

extern "C" {

int sk_aac_plan_create(sk_engine *e, const sk_aac_frame_desc *descs, uint32_t n, int32_t *status, sk_aac_plan **out) try {
    sk::abi_enter();
    if (!e || !out || (n && !descs)) return SK_ERR_INVALID_ARG;
    *out = nullptr;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    HostPlan hp;
    int rc = build_plan_host(e, descs, n, status, hp);
    if (rc != SK_OK) return rc;

    sk_aac_plan *p = new (std::nothrow) sk_aac_plan();
    if (!p) return SK_ERR_OOM;
    p->eng = e;
    p->n_tasks = (uint32_t)hp.tasks.size();
    p->n_entries = (uint32_t)hp.entries.size();
    p->n_frames_ok = hp.frames_ok;
    p->elements = hp.off1024 * 1024;
    if (!hp.tasks.empty()) {
        hipError_t he = upload(&p->d_tasks, hp.tasks);
        if (he == hipSuccess) he = upload(&p->d_entries, hp.entries);
        if (he == hipSuccess) he = upload(&p->d_spans, hp.spans);
        if (he == hipSuccess && !hp.walk_tasks.empty()) he = upload(&p->d_walk_tasks, hp.walk_tasks);
        if (he == hipSuccess && !hp.long_tasks.empty()) he = upload(&p->d_long_tasks, hp.long_tasks);
        if (he == hipSuccess && !hp.pair_tasks.empty()) he = upload(&p->d_pair_tasks, hp.pair_tasks);
        if (he == hipSuccess && !hp.spair_tasks.empty()) he = upload(&p->d_spair_tasks, hp.spair_tasks);
        p->n_walk_tasks = (uint32_t)hp.walk_tasks.size();
        p->n_long_tasks = (uint32_t)hp.long_tasks.size();
        p->n_pair_tasks = (uint32_t)hp.pair_tasks.size();
        p->n_spair_tasks = (uint32_t)hp.spair_tasks.size();
        p->uniform_count = hp.uniform_count;
        p->uniform_channels = hp.uniform_channels;
        if (he != hipSuccess) {
            sk_aac_plan_destroy(p);
            return e->hip_fail(he, "upload plan");
        }
    }
    *out = p;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_aac_plan_create");
}

static int run_plan(sk_engine *e, const sk_aac_plan *p, const float *d_coeffs, float *d_pcm, int16_t *d_pcm16 = nullptr) {
    sk::SynthArgs a{};
    a.coeffs = d_coeffs;
    a.pcm = d_pcm;
    a.pcm16 = d_pcm16;
    a.delay = e->d_delay;
    a.prev_shape = e->d_prev_shape;
    a.entries = p->d_entries;
    a.t = e->synth_tables;
    a.only_long = 1;
    a.tasks = p->d_pair_tasks;
    a.n_tasks = p->n_pair_tasks;
    SK_HIP(sk::launch_aac_synth_pairs(a, false, e->stream), "launch aac synth (two channels per wave)");
    a.tasks = p->d_spair_tasks;
    a.n_tasks = p->n_spair_tasks;
    SK_HIP(sk::launch_aac_synth_pairs(a, true, e->stream), "launch aac synth (two channels per wave, eight-short arm)");
    a.tasks = p->d_long_tasks;
    a.n_tasks = p->n_long_tasks;
    SK_HIP(sk::launch_aac_synth(a, e->stream), "launch aac synth (one channel per wave, no EightShort)");
    a.tasks = p->d_walk_tasks;
    a.n_tasks = p->n_walk_tasks;
    a.only_long = 0;
    SK_HIP(sk::launch_aac_synth(a, e->stream), "launch aac synth");
    return SK_OK;
}

int sk_aac_plan_run_f32_dev(sk_engine *e, const sk_aac_plan *p, const float *d_coeffs, float *d_pcm) try {
    sk::abi_enter();
    if (!e || !p || p->eng != e) return SK_ERR_INVALID_ARG;
    if (p->n_tasks == 0) return SK_OK;
    if (!d_coeffs || !d_pcm) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    return run_plan(e, p, d_coeffs, d_pcm);
} catch (...) {
    return sk::abi_caught("sk_aac_plan_run_f32_dev");
}

int sk_aac_plan_run_s16_planar_dev(sk_engine *e, const sk_aac_plan *p, const float *d_coeffs, int16_t *d_pcm16) try {
    sk::abi_enter();
    if (!e || !p || p->eng != e) return SK_ERR_INVALID_ARG;
    if (p->n_tasks == 0) return SK_OK;
    if (!d_coeffs || !d_pcm16 || ((uintptr_t)d_pcm16 & 7)) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    return run_plan(e, p, d_coeffs, nullptr, d_pcm16);
} catch (...) {
    return sk::abi_caught("sk_aac_plan_run_s16_planar_dev");
}

// The decode tail as one launch (k_aac_tail): sk_aac_plan_run_s16_planar_dev followed by the one-shot
// sk_downsample_48k_16k_frames_s16_to_s16_dev over all frames of the plan, without the s16 PCM in HBM.  For plans the fused kernel
// covers -- every channel free of EightShort frames and paired (two channels of equal length: build_plan_host), every stream with
// the same channel count and the same number of frames, each stream's frames `frames_per_stream` consecutive entries from its
// frame 0; anything else: SK_ERR_UNSUPPORTED, use the two calls.
//
// In a library built WITH packed-f32 instructions (make PACKED_F32=1) the entry point is withdrawn: SK_ERR_UNSUPPORTED for every plan
// unless SK_AAC_TAIL_ONE_LAUNCH=1 is in the environment (read at each call).  The kernel has synthesis waves and matrix-instruction
// FIR work resident on the same SIMDs, which is exactly the co-residency the platform gets wrong for packed-f32 instructions
// (profiles/r04_lanes_corruption.md): bit-identical to the two launches as long as a launch is no more than a workgroup or so per
// CU (what the tests of round 3 ran), and at the headline batch 3 % of the samples wrong by up to 5000 LSB, differently in every run
// (tools/debug/fused_tail_repeats.py).  The switch is for reproducing that, not for use.  In the default build (no packed-f32
// instructions) the kernel is exact at every size and the entry point works.
int sk_aac_plan_run_tail_s16_dev(sk_engine *e, const sk_aac_plan *p, const float *d_coeffs, size_t stream_stride, uint32_t channels,
                                 uint32_t frames_per_stream, int16_t *d_out, size_t out_stride, uint32_t *out_frames) try {
    sk::abi_enter();
    if (!e || !p || p->eng != e || channels < 1 || channels > SK_MAX_CHANNELS) return SK_ERR_INVALID_ARG;
    const uint64_t samples = (uint64_t)frames_per_stream * SK_AAC_FRAME_LEN;
    if (samples > 0xfffffffcull) return SK_ERR_INVALID_ARG;
    const uint32_t n_out = sk_downsample_48k_16k_out_frames((uint32_t)samples);
    if (out_frames) *out_frames = n_out;
    if (p->n_tasks == 0) return SK_OK;
    if (p->n_spair_tasks || p->n_long_tasks || p->n_walk_tasks || p->uniform_count != frames_per_stream || p->uniform_channels != channels ||
        frames_per_stream == 0)
        return SK_ERR_UNSUPPORTED;
    if (!d_coeffs || !d_out || out_stride < n_out || out_stride % 4 || stream_stride < (size_t)channels * SK_AAC_FRAME_LEN ||
        ((uintptr_t)d_out & 7))
        return SK_ERR_INVALID_ARG;
#if SK_PACKED_F32
    {
        const char *v = std::getenv("SK_AAC_TAIL_ONE_LAUNCH");
        if (!(v && v[0] == '1' && v[1] == 0)) return SK_ERR_UNSUPPORTED;  // withdrawn in this flavour: see above
    }
#endif
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    sk::TailArgs ta{};
    ta.s.coeffs = d_coeffs;
    ta.s.delay = e->d_delay;
    ta.s.prev_shape = e->d_prev_shape;
    ta.s.entries = p->d_entries;
    ta.s.t = e->synth_tables;
    ta.s.tasks = p->d_pair_tasks;
    ta.s.n_tasks = p->n_pair_tasks;
    ta.s.only_long = 1;
    ta.afrag_f16 = e->d_afrag_f16;
    ta.out16 = d_out;
    ta.out_stride = out_stride;
    ta.stream_stride = stream_stride;
    SK_HIP(sk::launch_aac_tail(ta, e->stream), "launch decode tail (fused synthesis + fir)");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_aac_plan_run_tail_s16_dev");
}

int sk_aac_plan_run_s16_dev(sk_engine *e, const sk_aac_plan *p, const float *d_coeffs, int16_t *d_pcm) try {
    sk::abi_enter();
    if (!e || !p || p->eng != e) return SK_ERR_INVALID_ARG;
    if (p->n_tasks == 0) return SK_OK;
    if (!d_coeffs || !d_pcm) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    SK_HIP(e->aux_buf.reserve(p->elements * sizeof(float)), "alloc planar scratch");
    int rc = run_plan(e, p, d_coeffs, (float *)e->aux_buf.p);
    if (rc != SK_OK) return rc;
    SK_HIP(sk::launch_frames_to_s16((const float *)e->aux_buf.p, d_pcm, p->d_spans, p->n_frames_ok, e->stream),
           "launch s16 interleave");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_aac_plan_run_s16_dev");
}

static int synthesize_host(sk_engine *e, const sk_aac_frame_desc *descs, const float *coeffs, void *pcm_out, uint32_t n,
                           int32_t *status, bool s16) {
    if (!e || (n && (!descs || !coeffs || !pcm_out))) return SK_ERR_INVALID_ARG;
    if (n == 0) return SK_OK;
    sk_aac_plan *p = nullptr;
    int rc = sk_aac_plan_create(e, descs, n, status, &p);
    if (rc != SK_OK) return rc;
    {
        std::lock_guard<std::mutex> lock(e->mu);
        DeviceGuard guard(e, ComputeTurn{});
        const size_t elems = (size_t)p->elements;
        do {
            hipError_t he = e->in_buf.reserve(elems * sizeof(float));
            if (he == hipSuccess) he = e->out_buf.reserve(elems * sizeof(float));
            if (he != hipSuccess) { rc = e->hip_fail(he, "alloc staging"); break; }
            if (p->n_tasks == 0) break;
            he = hipMemcpyAsync(e->in_buf.p, coeffs, elems * sizeof(float), hipMemcpyHostToDevice, e->stream);
            if (he != hipSuccess) { rc = e->hip_fail(he, "H2D coeffs"); break; }
            // frames that failed validation keep the caller's bytes: bring the current contents over first
            const size_t out_bytes = elems * (s16 ? sizeof(int16_t) : sizeof(float));
            if (p->n_frames_ok != n) {
                he = hipMemcpyAsync(e->out_buf.p, pcm_out, out_bytes, hipMemcpyHostToDevice, e->stream);
                if (he != hipSuccess) { rc = e->hip_fail(he, "H2D pcm"); break; }
            }
            if (s16) {
                he = e->aux_buf.reserve(elems * sizeof(float));
                if (he != hipSuccess) { rc = e->hip_fail(he, "alloc planar scratch"); break; }
                rc = run_plan(e, p, (const float *)e->in_buf.p, (float *)e->aux_buf.p);
                if (rc != SK_OK) break;
                he = sk::launch_frames_to_s16((const float *)e->aux_buf.p, (int16_t *)e->out_buf.p, p->d_spans,
                                              p->n_frames_ok, e->stream);
                if (he != hipSuccess) { rc = e->hip_fail(he, "launch s16 interleave"); break; }
            } else {
                rc = run_plan(e, p, (const float *)e->in_buf.p, (float *)e->out_buf.p);
                if (rc != SK_OK) break;
            }
            he = hipMemcpyAsync(pcm_out, e->out_buf.p, out_bytes, hipMemcpyDeviceToHost, e->stream);
            if (he != hipSuccess) { rc = e->hip_fail(he, "D2H pcm"); break; }
            he = hipStreamSynchronize(e->stream);
            if (he != hipSuccess) { rc = e->hip_fail(he, "synthesize sync"); break; }
        } while (0);
    }
    sk_aac_plan_destroy(p);
    return rc;
}

int sk_aac_synthesize_f32(sk_engine *e, const sk_aac_frame_desc *descs, const float *coeffs, float *pcm_out, uint32_t n,
                          int32_t *status) try {
    sk::abi_enter();
    return synthesize_host(e, descs, coeffs, pcm_out, n, status, false);
} catch (...) {
    return sk::abi_caught("sk_aac_synthesize_f32");
}

int sk_aac_synthesize_s16(sk_engine *e, const sk_aac_frame_desc *descs, const float *coeffs, int16_t *pcm_out,
                          uint32_t n, int32_t *status) try {
    sk::abi_enter();
    return synthesize_host(e, descs, coeffs, pcm_out, n, status, true);
} catch (...) {
    return sk::abi_caught("sk_aac_synthesize_s16");
}

int sk_aac_dequantize_dev(sk_engine *e, const int16_t *d_quant, const int16_t *d_sf, float *d_out, size_t n) try {
    sk::abi_enter();
    if (!e || (n && (!d_quant || !d_sf || !d_out))) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    SK_HIP(sk::launch_dequantize(d_quant, d_sf, d_out, n, e->d_pow43, e->d_sftab, e->stream), "launch dequantize");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_aac_dequantize_dev");
}

int sk_aac_dequantize(sk_engine *e, const int16_t *quant, const int16_t *sf, float *out, size_t n) try {
    sk::abi_enter();
    if (!e || (n && (!quant || !sf || !out))) return SK_ERR_INVALID_ARG;
    if (n == 0) return SK_OK;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    SK_HIP(e->in_buf.reserve(n * 4), "alloc staging");
    SK_HIP(e->out_buf.reserve(n * 4), "alloc staging");
    int16_t *dq = (int16_t *)e->in_buf.p, *dsf = dq + n;
    SK_HIP(hipMemcpyAsync(dq, quant, n * 2, hipMemcpyHostToDevice, e->stream), "H2D quant");
    SK_HIP(hipMemcpyAsync(dsf, sf, n * 2, hipMemcpyHostToDevice, e->stream), "H2D sf");
    SK_HIP(sk::launch_dequantize(dq, dsf, (float *)e->out_buf.p, n, e->d_pow43, e->d_sftab, e->stream), "launch dequantize");
    SK_HIP(hipMemcpyAsync(out, e->out_buf.p, n * 4, hipMemcpyDeviceToHost, e->stream), "D2H dequant");
    SK_HIP(hipStreamSynchronize(e->stream), "dequant sync");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_aac_dequantize");
}

// ---- PCM conversion ----------------------------------------------------------------------------

static const int8_t kOpIn[SK_PCM_OP_COUNT] = {2, 2, 2, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 2, 2, 2, 4, 4, 4, 2, 4, 4, 4, 4};
static const int8_t kOpOut[SK_PCM_OP_COUNT] = {4, 2, 2, 4, 2, 2, 4, 4, 4, 4, 4, 4, 2, 2, 2, 2, 4, 4, 2, 2, 4, 2, 2, 2, 4, 4, 2, 2, 4};

int sk_pcm_op_in_bytes(int op) try {
    sk::abi_enter();
    return (op < 0 || op >= SK_PCM_OP_COUNT) ? -1 : kOpIn[op];
} catch (...) {
    return sk::abi_caught("sk_pcm_op_in_bytes");
}
int sk_pcm_op_out_bytes(int op) try {
    sk::abi_enter();
    return (op < 0 || op >= SK_PCM_OP_COUNT) ? -1 : kOpOut[op];
} catch (...) {
    return sk::abi_caught("sk_pcm_op_out_bytes");
}

int sk_pcm_fmt_bytes(int fmt) try {
    sk::abi_enter();
    switch (fmt) {
    case SK_FMT_S16LE: case SK_FMT_S16BE: return 2;
    case SK_FMT_S24LE: case SK_FMT_S24BE: return 3;
    case SK_FMT_S32LE: case SK_FMT_S32BE: case SK_FMT_F32LE: case SK_FMT_F32BE: return 4;
    default: return -1;
    }
} catch (...) {
    return sk::abi_caught("sk_pcm_fmt_bytes");
}

int sk_pcm_convert_dev(sk_engine *e, int op, const void *d_in, void *d_out, size_t n) try {
    sk::abi_enter();
    if (!e || op < 0 || op >= SK_PCM_OP_COUNT || (n && (!d_in || !d_out))) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    SK_HIP(sk::launch_pcm_convert(op, d_in, d_out, n, e->stream), "launch pcm convert");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_pcm_convert_dev");
}

int sk_pcm_convert(sk_engine *e, int op, const void *in, void *out, size_t n) try {
    sk::abi_enter();
    if (op < 0 || op >= SK_PCM_OP_COUNT) return SK_ERR_INVALID_ARG;
    return host_roundtrip(e, in, n * kOpIn[op], out, n * kOpOut[op], [&](void *di, void *dout) {
        return sk::launch_pcm_convert(op, di, dout, n, e->stream);
    });
} catch (...) {
    return sk::abi_caught("sk_pcm_convert");
}

#define SK_DEV_ENTRY(call)                              \
    do {                                                \
        std::lock_guard<std::mutex> lock(e->mu);        \
        DeviceGuard guard(e);                   \
        SK_HIP(call, "launch pcm kernel");              \
        return SK_OK;                                   \
    } while (0)

int sk_pcm_interleave_i16_dev(sk_engine *e, const int16_t *d_planar, size_t frames, uint32_t ch, uint8_t *d_out) try {
    sk::abi_enter();
    if (!e || ch == 0 || (frames && (!d_planar || !d_out))) return SK_ERR_INVALID_ARG;
    SK_DEV_ENTRY(sk::launch_interleave(d_planar, d_out, frames, ch, 2, e->stream));
} catch (...) {
    return sk::abi_caught("sk_pcm_interleave_i16_dev");
}
int sk_pcm_deinterleave_i16_dev(sk_engine *e, const uint8_t *d_in, size_t frames, uint32_t ch, int16_t *d_planar) try {
    sk::abi_enter();
    if (!e || ch == 0 || (frames && (!d_in || !d_planar))) return SK_ERR_INVALID_ARG;
    SK_DEV_ENTRY(sk::launch_deinterleave(d_in, d_planar, frames, ch, 2, e->stream));
} catch (...) {
    return sk::abi_caught("sk_pcm_deinterleave_i16_dev");
}
int sk_pcm_deinterleave_s24_dev(sk_engine *e, const uint8_t *d_in, size_t frames, uint32_t ch, int32_t *d_planar) try {
    sk::abi_enter();
    if (!e || ch == 0 || (frames && (!d_in || !d_planar))) return SK_ERR_INVALID_ARG;
    SK_DEV_ENTRY(sk::launch_deinterleave_s24(d_in, d_planar, frames, ch, e->stream));
} catch (...) {
    return sk::abi_caught("sk_pcm_deinterleave_s24_dev");
}
int sk_pcm_deinterleave_f32_dev(sk_engine *e, const uint8_t *d_in, size_t frames, uint32_t ch, float *d_planar) try {
    sk::abi_enter();
    if (!e || ch == 0 || (frames && (!d_in || !d_planar))) return SK_ERR_INVALID_ARG;
    SK_DEV_ENTRY(sk::launch_deinterleave(d_in, d_planar, frames, ch, 4, e->stream));
} catch (...) {
    return sk::abi_caught("sk_pcm_deinterleave_f32_dev");
}
int sk_pcm_interleave_f32_dev(sk_engine *e, const float *d_planar, size_t frames, uint32_t ch, uint8_t *d_out) try {
    sk::abi_enter();
    if (!e || ch == 0 || (frames && (!d_planar || !d_out))) return SK_ERR_INVALID_ARG;
    SK_DEV_ENTRY(sk::launch_interleave(d_planar, d_out, frames, ch, 4, e->stream));
} catch (...) {
    return sk::abi_caught("sk_pcm_interleave_f32_dev");
}

int sk_pcm_interleave_i16(sk_engine *e, const int16_t *planar, size_t frames, uint32_t ch, uint8_t *out) try {
    sk::abi_enter();
    if (ch == 0) return SK_ERR_INVALID_ARG;
    const size_t bytes = frames * ch * 2;
    return host_roundtrip(e, planar, bytes, out, bytes, [&](void *di, void *dout) {
        return sk::launch_interleave(di, dout, frames, ch, 2, e->stream);
    });
} catch (...) {
    return sk::abi_caught("sk_pcm_interleave_i16");
}
int sk_pcm_deinterleave_i16(sk_engine *e, const uint8_t *in, size_t frames, uint32_t ch, int16_t *planar) try {
    sk::abi_enter();
    if (ch == 0) return SK_ERR_INVALID_ARG;
    const size_t bytes = frames * ch * 2;
    return host_roundtrip(e, in, bytes, planar, bytes, [&](void *di, void *dout) {
        return sk::launch_deinterleave(di, dout, frames, ch, 2, e->stream);
    });
} catch (...) {
    return sk::abi_caught("sk_pcm_deinterleave_i16");
}
int sk_pcm_deinterleave_s24(sk_engine *e, const uint8_t *in, size_t frames, uint32_t ch, int32_t *planar) try {
    sk::abi_enter();
    if (ch == 0) return SK_ERR_INVALID_ARG;
    return host_roundtrip(e, in, frames * ch * 3, planar, frames * ch * 4, [&](void *di, void *dout) {
        return sk::launch_deinterleave_s24((const uint8_t *)di, (int32_t *)dout, frames, ch, e->stream);
    });
} catch (...) {
    return sk::abi_caught("sk_pcm_deinterleave_s24");
}
int sk_pcm_deinterleave_f32(sk_engine *e, const uint8_t *in, size_t frames, uint32_t ch, float *planar) try {
    sk::abi_enter();
    if (ch == 0) return SK_ERR_INVALID_ARG;
    const size_t bytes = frames * ch * 4;
    return host_roundtrip(e, in, bytes, planar, bytes, [&](void *di, void *dout) {
        return sk::launch_deinterleave(di, dout, frames, ch, 4, e->stream);
    });
} catch (...) {
    return sk::abi_caught("sk_pcm_deinterleave_f32");
}
int sk_pcm_interleave_f32(sk_engine *e, const float *planar, size_t frames, uint32_t ch, uint8_t *out) try {
    sk::abi_enter();
    if (ch == 0) return SK_ERR_INVALID_ARG;
    const size_t bytes = frames * ch * 4;
    return host_roundtrip(e, planar, bytes, out, bytes, [&](void *di, void *dout) {
        return sk::launch_interleave(di, dout, frames, ch, 4, e->stream);
    });
} catch (...) {
    return sk::abi_caught("sk_pcm_interleave_f32");
}

static bool to_f32_args_ok(int variant, int fmt) {
    if (variant == 0) return fmt >= SK_FMT_S16LE && fmt <= SK_FMT_F32BE;
    return variant == 1 && (fmt == SK_FMT_S16LE || fmt == SK_FMT_S24LE || fmt == SK_FMT_S32LE || fmt == SK_FMT_F32LE);
}
static bool from_f32_fmt_ok(int fmt) {
    return fmt == SK_FMT_S16LE || fmt == SK_FMT_S24LE || fmt == SK_FMT_S32LE || fmt == SK_FMT_F32LE;
}

int sk_pcm_bytes_to_f32_planar_dev(sk_engine *e, int variant, int fmt, const uint8_t *d_in, size_t frames, uint32_t ch,
                                   float *d_planar) try {
    sk::abi_enter();
    if (!e || ch == 0 || !to_f32_args_ok(variant, fmt) || (frames && (!d_in || !d_planar))) return SK_ERR_INVALID_ARG;
    SK_DEV_ENTRY(sk::launch_bytes_to_f32_planar(variant, fmt, d_in, frames, ch, d_planar, e->stream));
} catch (...) {
    return sk::abi_caught("sk_pcm_bytes_to_f32_planar_dev");
}
int sk_pcm_bytes_to_f32_planar(sk_engine *e, int variant, int fmt, const uint8_t *in, size_t frames, uint32_t ch,
                               float *planar) try {
    sk::abi_enter();
    if (ch == 0 || !to_f32_args_ok(variant, fmt)) return SK_ERR_INVALID_ARG;
    return host_roundtrip(e, in, frames * ch * sk_pcm_fmt_bytes(fmt), planar, frames * ch * 4, [&](void *di, void *dout) {
        return sk::launch_bytes_to_f32_planar(variant, fmt, (const uint8_t *)di, frames, ch, (float *)dout, e->stream);
    });
} catch (...) {
    return sk::abi_caught("sk_pcm_bytes_to_f32_planar");
}
int sk_pcm_f32_planar_to_bytes_dev(sk_engine *e, int fmt, const float *d_planar, size_t frames, uint32_t ch,
                                   uint8_t *d_out) try {
    sk::abi_enter();
    if (!e || ch == 0 || !from_f32_fmt_ok(fmt) || (frames && (!d_planar || !d_out))) return SK_ERR_INVALID_ARG;
    SK_DEV_ENTRY(sk::launch_f32_planar_to_bytes(fmt, d_planar, frames, ch, d_out, e->stream));
} catch (...) {
    return sk::abi_caught("sk_pcm_f32_planar_to_bytes_dev");
}
int sk_pcm_f32_planar_to_bytes(sk_engine *e, int fmt, const float *planar, size_t frames, uint32_t ch, uint8_t *out) try {
    sk::abi_enter();
    if (ch == 0 || !from_f32_fmt_ok(fmt)) return SK_ERR_INVALID_ARG;
    return host_roundtrip(e, planar, frames * ch * 4, out, frames * ch * sk_pcm_fmt_bytes(fmt), [&](void *di, void *dout) {
        return sk::launch_f32_planar_to_bytes(fmt, (const float *)di, frames, ch, (uint8_t *)dout, e->stream);
    });
} catch (...) {
    return sk::abi_caught("sk_pcm_f32_planar_to_bytes");
}
int sk_pcm_f32_planar_to_bytes_batch_dev(sk_engine *e, int fmt, const float *d_planar, size_t batch, size_t plane_stride,
                                         size_t frames, uint32_t ch, uint8_t *d_out) try {
    sk::abi_enter();
    if (!e || ch == 0 || !from_f32_fmt_ok(fmt) || plane_stride < frames || batch > 65535 ||
        (frames && batch && (!d_planar || !d_out)))
        return SK_ERR_INVALID_ARG;
    SK_DEV_ENTRY(sk::launch_f32_planar_to_bytes_batch(fmt, d_planar, batch, plane_stride, frames, ch, d_out, e->stream));
} catch (...) {
    return sk::abi_caught("sk_pcm_f32_planar_to_bytes_batch_dev");
}
int sk_pcm_downmix_mono_dev(sk_engine *e, const float *d_planar, size_t frames, uint32_t ch, float *d_mono) try {
    sk::abi_enter();
    if (!e || ch == 0 || (frames && (!d_planar || !d_mono))) return SK_ERR_INVALID_ARG;
    SK_DEV_ENTRY(sk::launch_downmix_mono(d_planar, frames, ch, d_mono, e->stream));
} catch (...) {
    return sk::abi_caught("sk_pcm_downmix_mono_dev");
}
int sk_pcm_downmix_mono(sk_engine *e, const float *planar, size_t frames, uint32_t ch, float *mono) try {
    sk::abi_enter();
    if (ch == 0) return SK_ERR_INVALID_ARG;
    return host_roundtrip(e, planar, frames * ch * 4, mono, frames * 4, [&](void *di, void *dout) {
        return sk::launch_downmix_mono((const float *)di, frames, ch, (float *)dout, e->stream);
    });
} catch (...) {
    return sk::abi_caught("sk_pcm_downmix_mono");
}
// downmix_channels (lib.rs:3492-3561) as one job of the wide kernels: planar rows in, min(target, ch) planar rows out.  e->mu held.
static int downmix_locked(sk_engine *e, const float *d_planar, size_t frames, uint32_t ch, uint32_t target, float *d_out) {
    sk::WideJob j{};
    j.src = d_planar, j.dst = d_out, j.src_stride = frames, j.dst_stride = frames, j.frames = (uint32_t)frames;
    j.fmt_in = j.fmt_out = sk::kWidePlanar;
    j.ch_in = (uint8_t)ch, j.ch_out = (uint8_t)std::min(target, ch);
    j.peak = sk::kWideNoPeak;
    if (j.ch_out == 2 && ch > 2) {  // the stereo branch: its peak word, cleared in stream order in front of the two launches
        if (!e->d_wide_peak) SK_HIP(hipMalloc((void **)&e->d_wide_peak, 256), "alloc downmix peak");
        SK_HIP(hipMemsetAsync(e->d_wide_peak, 0, sizeof(uint32_t), e->stream), "clear downmix peak");
        j.peak = 0;
    }
    SK_HIP(sk::launch_pcm_wide_one(j, e->d_wide_peak, e->stream), "launch downmix");
    return SK_OK;
}
static bool downmix_args_ok(size_t frames, uint32_t ch, uint32_t target) {
    return ch >= 1 && ch <= SK_MAX_PCM_CHANNELS && target >= 1 && frames <= 0x7fffffffu;
}
int sk_pcm_downmix_dev(sk_engine *e, const float *d_planar, size_t frames, uint32_t ch, uint32_t target, float *d_out) try {
    sk::abi_enter();
    if (!e || !downmix_args_ok(frames, ch, target) || (frames && (!d_planar || !d_out))) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    return downmix_locked(e, d_planar, frames, ch, target, d_out);
} catch (...) {
    return sk::abi_caught("sk_pcm_downmix_dev");
}
int sk_pcm_downmix(sk_engine *e, const float *planar, size_t frames, uint32_t ch, uint32_t target, float *out) try {
    sk::abi_enter();
    if (!e || !downmix_args_ok(frames, ch, target) || (frames && (!planar || !out))) return SK_ERR_INVALID_ARG;
    if (frames == 0) return SK_OK;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    const size_t in_bytes = frames * ch * 4, out_bytes = frames * std::min(target, ch) * 4;
    SK_HIP(e->in_buf.reserve(in_bytes), "alloc staging");
    SK_HIP(e->out_buf.reserve(out_bytes), "alloc staging");
    SK_HIP(hipMemcpyAsync(e->in_buf.p, planar, in_bytes, hipMemcpyHostToDevice, e->stream), "H2D downmix");
    const int rc = downmix_locked(e, (const float *)e->in_buf.p, frames, ch, target, (float *)e->out_buf.p);
    if (rc != SK_OK) return rc;
    SK_HIP(hipMemcpyAsync(out, e->out_buf.p, out_bytes, hipMemcpyDeviceToHost, e->stream), "D2H downmix");
    SK_HIP(hipStreamSynchronize(e->stream), "downmix sync");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_pcm_downmix");
}
static bool exact_fmt_ok(int fmt) { return fmt >= SK_FMT_S24LE && fmt <= SK_FMT_S32BE; }
int sk_pcm_exact_to_i16_dev(sk_engine *e, int fmt, const uint8_t *d_in, size_t samples, uint8_t *d_out) try {
    sk::abi_enter();
    if (!e || !exact_fmt_ok(fmt) || (samples && (!d_in || !d_out))) return SK_ERR_INVALID_ARG;
    SK_DEV_ENTRY(sk::launch_exact_to_i16(fmt, d_in, samples, d_out, e->stream));
} catch (...) {
    return sk::abi_caught("sk_pcm_exact_to_i16_dev");
}
int sk_pcm_exact_to_i16(sk_engine *e, int fmt, const uint8_t *in, size_t samples, uint8_t *out) try {
    sk::abi_enter();
    if (!exact_fmt_ok(fmt)) return SK_ERR_INVALID_ARG;
    return host_roundtrip(e, in, samples * sk_pcm_fmt_bytes(fmt), out, samples * 2, [&](void *di, void *dout) {
        return sk::launch_exact_to_i16(fmt, (const uint8_t *)di, samples, (uint8_t *)dout, e->stream);
    });
} catch (...) {
    return sk::abi_caught("sk_pcm_exact_to_i16");
}

// ---- 48 kHz -> 16 kHz FIR ----------------------------------------------------------------------

uint32_t sk_downsample_48k_16k_out_frames(uint32_t frames) try {
    sk::abi_enter();
    // rubato SincFixedIn: idx starts at -128, advances by 3 before each output, loop runs while
    // idx < frames - 257 - 3
    if (frames <= 132) return 0;
    return (frames - 132 + 2) / 3;
} catch (...) {
    (void)sk::abi_caught("sk_downsample_48k_16k_out_frames");
    return 0;
}

int sk_downsample_48k_16k_taps(sk_engine *e, float *taps256) try {
    sk::abi_enter();
    if (!e || !taps256) return SK_ERR_INVALID_ARG;
    std::memcpy(taps256, e->h_taps.data(), 256 * sizeof(float));
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_downsample_48k_16k_taps");
}

static sk::FirArgs fir_base(sk_engine *e) {
    sk::FirArgs a{};
    a.zeros = e->d_zeros;
    a.afrag16 = e->d_afrag16;
    a.afrag_f16 = e->d_afrag_f16;
    a.taps = e->d_taps;
    return a;
}

int sk_downsample_48k_16k_f32_dev(sk_engine *e, const float *d_in, size_t in_stride, uint32_t rows, uint32_t frames,
                                  float *d_out, size_t out_stride, uint32_t *out_frames) try {
    sk::abi_enter();
    if (!e) return SK_ERR_INVALID_ARG;
    const uint32_t n_out = sk_downsample_48k_16k_out_frames(frames);
    if (out_frames) *out_frames = n_out;
    if (rows == 0 || n_out == 0) return SK_OK;
    if (!d_in || !d_out || in_stride < frames || out_stride < n_out) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    sk::FirArgs a = fir_base(e);
    a.in = d_in;
    a.out = d_out;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.rows = rows;
    a.in_frames = frames;
    a.in_origin = 0;
    a.out_first = 0;
    a.out_count = n_out;
    SK_HIP(sk::launch_fir_48k_16k(a, e->stream), "launch fir");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_downsample_48k_16k_f32_dev");
}

int sk_downsample_48k_16k_frames_dev(sk_engine *e, const float *d_pcm, size_t stream_stride, size_t frame_stride,
                                     uint32_t channels, uint32_t n_streams, uint32_t frames_per_stream, float *d_out,
                                     size_t out_stride, uint32_t *out_frames) try {
    sk::abi_enter();
    if (!e || channels < 1 || channels > SK_MAX_CHANNELS) return SK_ERR_INVALID_ARG;
    const uint64_t samples = (uint64_t)frames_per_stream * SK_AAC_FRAME_LEN;
    if (samples > 0xfffffffcull) return SK_ERR_INVALID_ARG;
    const uint32_t n_out = sk_downsample_48k_16k_out_frames((uint32_t)samples);
    if (out_frames) *out_frames = n_out;
    if (n_streams == 0 || n_out == 0) return SK_OK;
    if (!d_pcm || !d_out || out_stride < n_out || frame_stride < (size_t)channels * SK_AAC_FRAME_LEN)
        return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    sk::FirArgs a = fir_base(e);
    a.in = d_pcm;
    a.out = d_out;
    a.in_stride = 0;
    a.out_stride = out_stride;
    a.in_block = SK_AAC_FRAME_LEN;
    a.in_ch = channels;
    a.in_block_stride = frame_stride;
    a.in_group_stride = stream_stride;
    a.rows = n_streams * channels;
    a.in_frames = (uint32_t)samples;
    a.in_origin = 0;
    a.out_first = 0;
    a.out_count = n_out;
    SK_HIP(sk::launch_fir_48k_16k(a, e->stream), "launch fir (frame-packed input)");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_downsample_48k_16k_frames_dev");
}

int sk_downsample_48k_16k_frames_s16_dev(sk_engine *e, const float *d_pcm, size_t stream_stride, size_t frame_stride,
                                         uint32_t channels, uint32_t n_streams, uint32_t frames_per_stream, int16_t *d_out,
                                         size_t out_stride, uint32_t *out_frames) try {
    sk::abi_enter();
    if (!e || channels < 1 || channels > SK_MAX_CHANNELS) return SK_ERR_INVALID_ARG;
    const uint64_t samples = (uint64_t)frames_per_stream * SK_AAC_FRAME_LEN;
    if (samples > 0xfffffffcull) return SK_ERR_INVALID_ARG;
    const uint32_t n_out = sk_downsample_48k_16k_out_frames((uint32_t)samples);
    if (out_frames) *out_frames = n_out;
    if (n_streams == 0 || n_out == 0) return SK_OK;
    if (!d_pcm || !d_out || out_stride < n_out || frame_stride < (size_t)channels * SK_AAC_FRAME_LEN)
        return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    sk::FirArgs a = fir_base(e);
    a.in = d_pcm;
    a.out = nullptr;
    a.out16 = d_out;
    a.out16_stride = out_stride;
    a.out16_ch = channels;
    a.in_stride = 0;
    a.out_stride = 0;
    a.in_block = SK_AAC_FRAME_LEN;
    a.in_ch = channels;
    a.in_block_stride = frame_stride;
    a.in_group_stride = stream_stride;
    a.rows = n_streams * channels;
    a.in_frames = (uint32_t)samples;
    a.in_origin = 0;
    a.out_first = 0;
    a.out_count = n_out;
    SK_HIP(sk::launch_fir_48k_16k(a, e->stream), "launch fir (frame-packed input, s16 output)");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_downsample_48k_16k_frames_s16_dev");
}

static int fir_from_s16(sk_engine *e, const int16_t *d_pcm16, size_t stream_stride, size_t frame_stride, uint32_t channels,
                        uint32_t n_streams, uint32_t frames_per_stream, int16_t *d_out16, float *d_out32, size_t out_stride,
                        uint32_t *out_frames);

int sk_downsample_48k_16k_frames_s16_to_s16_dev(sk_engine *e, const int16_t *d_pcm16, size_t stream_stride, size_t frame_stride,
                                                uint32_t channels, uint32_t n_streams, uint32_t frames_per_stream, int16_t *d_out,
                                                size_t out_stride, uint32_t *out_frames) try {
    sk::abi_enter();
    return fir_from_s16(e, d_pcm16, stream_stride, frame_stride, channels, n_streams, frames_per_stream, d_out, nullptr, out_stride,
                        out_frames);
} catch (...) {
    return sk::abi_caught("sk_downsample_48k_16k_frames_s16_to_s16_dev");
}

int sk_downsample_48k_16k_frames_s16_to_f32_dev(sk_engine *e, const int16_t *d_pcm16, size_t stream_stride, size_t frame_stride,
                                                uint32_t channels, uint32_t n_streams, uint32_t frames_per_stream, float *d_out,
                                                size_t out_stride, uint32_t *out_frames) try {
    sk::abi_enter();
    return fir_from_s16(e, d_pcm16, stream_stride, frame_stride, channels, n_streams, frames_per_stream, nullptr, d_out, out_stride,
                        out_frames);
} catch (...) {
    return sk::abi_caught("sk_downsample_48k_16k_frames_s16_to_f32_dev");
}

static int fir_from_s16(sk_engine *e, const int16_t *d_pcm16, size_t stream_stride, size_t frame_stride, uint32_t channels,
                        uint32_t n_streams, uint32_t frames_per_stream, int16_t *d_out, float *d_out32, size_t out_stride,
                        uint32_t *out_frames) {
    if (!e || channels < 1 || channels > SK_MAX_CHANNELS) return SK_ERR_INVALID_ARG;
    const uint64_t samples = (uint64_t)frames_per_stream * SK_AAC_FRAME_LEN;
    if (samples > 0xfffffffcull) return SK_ERR_INVALID_ARG;
    const uint32_t n_out = sk_downsample_48k_16k_out_frames((uint32_t)samples);
    if (out_frames) *out_frames = n_out;
    if (n_streams == 0 || n_out == 0) return SK_OK;
    if (!d_pcm16 || (!d_out && !d_out32) || out_stride < n_out || frame_stride < (size_t)channels * SK_AAC_FRAME_LEN ||
        stream_stride % 4 || frame_stride % 4 || ((uintptr_t)d_pcm16 & 7))
        return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    sk::FirArgs a = fir_base(e);
    a.in16 = d_pcm16;
    if (d_out) {
        a.out16 = d_out;
        a.out16_stride = out_stride;
        a.out16_ch = channels;
    } else {
        a.out = d_out32;
        a.out_stride = out_stride;
    }
    a.in_block = SK_AAC_FRAME_LEN;
    a.in_ch = channels;
    a.in_block_stride = frame_stride;
    a.in_group_stride = stream_stride;
    a.rows = n_streams * channels;
    a.in_frames = (uint32_t)samples;
    a.out_count = n_out;
    SK_HIP(sk::launch_fir_48k_16k(a, e->stream), "launch fir (s16 frame-packed input, s16 output)");
    return SK_OK;
}

int sk_downsample_48k_16k_f32(sk_engine *e, const float *in, uint32_t rows, uint32_t frames, float *out,
                              uint32_t *out_frames) try {
    sk::abi_enter();
    if (!e) return SK_ERR_INVALID_ARG;
    const uint32_t n_out = sk_downsample_48k_16k_out_frames(frames);
    if (out_frames) *out_frames = n_out;
    if (rows == 0 || n_out == 0) return SK_OK;
    if (!in || !out) return SK_ERR_INVALID_ARG;
    const size_t in_stride = ((size_t)frames + 3) & ~(size_t)3, out_stride = ((size_t)n_out + 3) & ~(size_t)3;
    {
        std::lock_guard<std::mutex> lock(e->mu);
        DeviceGuard guard(e);
        SK_HIP(e->in_buf.reserve(rows * in_stride * 4), "alloc staging");
        SK_HIP(e->out_buf.reserve(rows * out_stride * 4), "alloc staging");
        SK_HIP(hipMemcpy2DAsync(e->in_buf.p, in_stride * 4, in, (size_t)frames * 4, (size_t)frames * 4, rows,
                                hipMemcpyHostToDevice, e->stream), "H2D fir input");
    }
    int rc = sk_downsample_48k_16k_f32_dev(e, (const float *)e->in_buf.p, in_stride, rows, frames, (float *)e->out_buf.p,
                                           out_stride, nullptr);
    if (rc != SK_OK) return rc;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    SK_HIP(hipMemcpy2DAsync(out, (size_t)n_out * 4, e->out_buf.p, out_stride * 4, (size_t)n_out * 4, rows,
                            hipMemcpyDeviceToHost, e->stream), "D2H fir output");
    SK_HIP(hipStreamSynchronize(e->stream), "fir sync");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_downsample_48k_16k_f32");
}

}  // extern "C" (helpers below are C++)

// ---- StreamingResampler (soundkit-decoder lib.rs:1917-2060) ------------------------------------
// Per stream the engine keeps rubato's SincFixedIn buffer in HBM: d_rs[stream*2 + ch][512 + 4096]
// (2*sinc_len of history + one chunk).  A call appends input to every stream's chunk area, and every
// time chunks fill up, all streams whose resampler is in the same state are processed by ONE launch
// (row-indirected): the MFMA FIR for 48k->16k, the generic sinc kernel otherwise.

static const uint32_t kCommonRates[9] = {8000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000};  // audio_pipeline.rs:12-13
static bool common_rate(uint32_t hz) {
    for (uint32_t r : kCommonRates)
        if (r == hz) return true;
    return false;
}

static int ratio_table_for(sk_engine *e, uint32_t in_hz, uint32_t out_hz, int *index) {
    for (size_t i = 0; i < e->ratio_tables.size(); ++i)
        if (e->ratio_tables[i].in_hz == in_hz && e->ratio_tables[i].out_hz == out_hz) {
            *index = (int)i;
            return SK_OK;
        }
    RatioTable t;
    t.in_hz = in_hz;
    t.out_hz = out_hz;
    t.ratio = (double)out_hz / (double)in_hz;
    std::vector<float> sincs;
    make_sinc_table(t.ratio, sincs);
    // behind the table, the same taps as pairs {sub-filter s, sub-filter s + 1} for the packed form of the two dot products
    // of an output (resample.hip: dot_pair_packed)
    sincs.resize(3 * 65536);
    for (size_t sub = 0; sub < 256; ++sub)
        for (size_t i = 0; i < 256; ++i) {
            sincs[65536 + 2 * (sub * 256 + i)] = sincs[sub * 256 + i];
            sincs[65536 + 2 * (sub * 256 + i) + 1] = sincs[((sub + 1) & 255) * 256 + i];
        }
    SK_HIP(upload(&t.d_sincs, sincs), "upload sinc table");
    e->ratio_tables.push_back(t);
    *index = (int)e->ratio_tables.size() - 1;
    return SK_OK;
}

// rubato SincFixedIn::process_into_buffer index walk for one chunk of `chunk` frames
static void chunk_indices(double ratio, double last_index, uint32_t chunk, std::vector<double> &idx, double *new_last) {
    const double t_ratio = 1.0 / ratio;
    const long end_idx = (long)chunk - 257 - (long)std::ceil(t_ratio);
    double i = last_index;
    idx.clear();
    while (i < (double)end_idx) {
        i += t_ratio;
        idx.push_back(i);
    }
    *new_last = i - (double)chunk;
}

static void make_index_set(double ratio, double last_index, uint32_t chunk, IndexSet &set) {
    std::vector<double> idx;
    chunk_indices(ratio, last_index, chunk, idx, &set.new_last);
    set.last_in = last_index;
    set.count = (uint32_t)idx.size();
    set.starts.clear();
    for (size_t k = 0; k < idx.size(); k += 32) set.starts.push_back(idx[k]);  // every 32nd output: SincArgs::set_starts
}

// set of streaming chunk number n of a ratio (memoised: chunk n starts where chunk n - 1 ended)
static const IndexSet &streaming_set(RatioTable &tab, uint64_t n) {
    while (tab.chunk_sets.size() <= n) {
        const double last = tab.chunk_sets.empty() ? -128.0 : tab.chunk_sets.back().new_last;
        tab.chunk_sets.emplace_back();
        make_index_set(tab.ratio, last, kRsChunk, tab.chunk_sets.back());
    }
    return tab.chunk_sets[(size_t)n];
}

extern "C" {

uint32_t sk_downsample_out_frames(uint32_t frames, uint32_t in_hz, uint32_t out_hz) try {
    sk::abi_enter();
    if (!in_hz || !out_hz) return 0;
    std::vector<double> idx;
    double nl = 0.0;
    chunk_indices((double)out_hz / (double)in_hz, -128.0, frames, idx, &nl);
    return (uint32_t)idx.size();
} catch (...) {
    (void)sk::abi_caught("sk_downsample_out_frames");
    return 0;
}

int sk_downsample_f32_dev(sk_engine *e, const float *d_in, size_t in_stride, uint32_t rows, uint32_t frames,
                          uint32_t in_hz, uint32_t out_hz, float *d_out, size_t out_stride, uint32_t *out_frames) try {
    sk::abi_enter();
    if (!e) return SK_ERR_INVALID_ARG;
    if (!common_rate(in_hz) || !common_rate(out_hz)) return SK_ERR_UNSUPPORTED;
    if (in_hz == 48000 && out_hz == 16000)
        return sk_downsample_48k_16k_f32_dev(e, d_in, in_stride, rows, frames, d_out, out_stride, out_frames);
    IndexSet set;
    make_index_set((double)out_hz / (double)in_hz, -128.0, frames, set);
    const uint32_t n_out = set.count;
    if (out_frames) *out_frames = n_out;
    if (rows == 0 || n_out == 0) return SK_OK;
    if (!d_in || !d_out || in_stride < frames || out_stride < n_out) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    int table = -1;
    int rc = ratio_table_for(e, in_hz, out_hz, &table);
    if (rc != SK_OK) return rc;
    const size_t starts_bytes = (set.starts.size() * sizeof(double) + 255) & ~(size_t)255;
    SK_HIP(e->aux2_buf.reserve(starts_bytes + 4096), "alloc index scratch");
    SK_HIP(hipMemcpyAsync(e->aux2_buf.p, set.starts.data(), set.starts.size() * sizeof(double), hipMemcpyHostToDevice, e->stream),
           "upload time indices");
    SK_HIP(hipMemcpyAsync((uint8_t *)e->aux2_buf.p + starts_bytes, &set.count, sizeof(uint32_t), hipMemcpyHostToDevice, e->stream),
           "upload output count");
    sk::SincArgs a{};
    a.in = d_in;
    a.in_stride = in_stride;
    a.out = d_out;
    a.out_stride = out_stride;
    a.sincs = e->ratio_tables[(size_t)table].d_sincs;
    a.set_starts = (const double *)e->aux2_buf.p;
    a.set_count = (const uint32_t *)((const uint8_t *)e->aux2_buf.p + starts_bytes);
    a.starts_stride = (uint32_t)set.starts.size();
    a.step = 1.0 / e->ratio_tables[(size_t)table].ratio;
    a.in_frames = frames;
    a.out_count = n_out;
    a.in_origin = 0;
    a.n_sets = 1;
    a.exact = e->sinc_exact;
    if (!a.exact) {
        const size_t want = sk::sinc_mfma_scratch_bytes(1, n_out, a.step);
        // want == 0: a ratio the matrix-core form does not take (decided by the ratio alone).  A failed allocation is an
        // error, never a silent change of arithmetic: the same row must get the same bits alone or in any batch.
        if (want) {
            SK_HIP(e->sinc_scratch.reserve(want), "alloc resampler tap fragments");
            a.scratch = e->sinc_scratch.p, a.scratch_bytes = e->sinc_scratch.cap;
        }
    }
    const uint32_t rows_per_launch = 65535u * sk::sinc_rows_per_block();  // grid.y limit
    for (uint32_t r0 = 0; r0 < rows; r0 += rows_per_launch) {
        sk::SincArgs part = a;
        part.rows = std::min<uint32_t>(rows_per_launch, rows - r0);
        part.in = d_in + (size_t)r0 * in_stride;
        part.out = d_out + (size_t)r0 * out_stride;
        SK_HIP(sk::launch_sinc_resample(part, e->stream), "launch sinc resample");
    }
    SK_HIP(hipStreamSynchronize(e->stream), "resample sync");  // the index set lives in host memory until the copy is done
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_downsample_f32_dev");
}

// The one-shot resampler of the device-resident decode tail at any ratio of the common rates the matrix-core form takes: planar
// s16 frames in (sk_aac_plan_run_s16_planar_dev's layout), interleaved s16 or f32 rows out.  48 -> 16 kHz is the fixed filter's own
// pair of entry points.  No scalar form behind it: exact mode and the steep ratios are refused, never computed another way.
static int sinc_from_s16(sk_engine *e, const int16_t *d_pcm16, size_t stream_stride, size_t frame_stride, uint32_t channels,
                         uint32_t n_streams, uint32_t frames_per_stream, uint32_t in_hz, uint32_t out_hz, int16_t *d_out16,
                         float *d_out32, size_t out_stride, uint32_t *out_frames) {
    if (!e || channels < 1 || channels > SK_MAX_CHANNELS) return SK_ERR_INVALID_ARG;
    if (!common_rate(in_hz) || !common_rate(out_hz)) return SK_ERR_UNSUPPORTED;
    if (in_hz == 48000 && out_hz == 16000)
        return fir_from_s16(e, d_pcm16, stream_stride, frame_stride, channels, n_streams, frames_per_stream, d_out16, d_out32, out_stride,
                            out_frames);
    const uint64_t samples = (uint64_t)frames_per_stream * SK_AAC_FRAME_LEN;
    if (samples > 0x7ffff000ull) return SK_ERR_INVALID_ARG;  // 32-bit sample indices inside the kernels
    const double ratio = (double)out_hz / (double)in_hz, step = 1.0 / ratio;
    IndexSet set;
    make_index_set(ratio, -128.0, (uint32_t)samples, set);
    const uint32_t n_out = set.count;
    if (out_frames) *out_frames = n_out;
    if (e->sinc_exact) return SK_ERR_UNSUPPORTED;
    if (n_streams == 0 || n_out == 0) return SK_OK;
    const size_t want = sk::sinc_mfma_scratch_bytes(1, n_out, step);
    if (!want) return SK_ERR_UNSUPPORTED;  // a step the matrix-core form does not take (decided by the ratio alone)
    if ((uint64_t)n_streams * channels > 0xffffffffull) return SK_ERR_INVALID_ARG;
    if (!d_pcm16 || (!d_out16 && !d_out32) || out_stride < n_out || frame_stride < (size_t)channels * SK_AAC_FRAME_LEN ||
        stream_stride % 4 || frame_stride % 4 || ((uintptr_t)d_pcm16 & 7) || (d_out16 && ((uintptr_t)d_out16 & 7)) ||
        (d_out32 && ((uintptr_t)d_out32 & 3)))
        return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    int table = -1;
    int rc = ratio_table_for(e, in_hz, out_hz, &table);
    if (rc != SK_OK) return rc;
    const size_t starts_bytes = (set.starts.size() * sizeof(double) + 255) & ~(size_t)255;
    SK_HIP(e->aux2_buf.reserve(starts_bytes + 4096), "alloc index scratch");
    SK_HIP(hipMemcpyAsync(e->aux2_buf.p, set.starts.data(), set.starts.size() * sizeof(double), hipMemcpyHostToDevice, e->stream),
           "upload time indices");
    SK_HIP(hipMemcpyAsync((uint8_t *)e->aux2_buf.p + starts_bytes, &set.count, sizeof(uint32_t), hipMemcpyHostToDevice, e->stream),
           "upload output count");
    // a failed allocation is an error, never another arithmetic (see sk_downsample_f32_dev)
    SK_HIP(e->sinc_scratch.reserve(want), "alloc resampler tap fragments");
    sk::SincS16Args a{};
    a.stream_stride = stream_stride;
    a.frame_stride = frame_stride;
    a.channels = channels;
    a.in_frames = (uint32_t)samples;
    a.out_stride = out_stride;
    a.sincs = e->ratio_tables[(size_t)table].d_sincs;
    a.set_starts = (const double *)e->aux2_buf.p;
    a.set_count = (const uint32_t *)((const uint8_t *)e->aux2_buf.p + starts_bytes);
    a.starts_stride = (uint32_t)set.starts.size();
    a.step = 1.0 / e->ratio_tables[(size_t)table].ratio;
    a.out_count = n_out;
    a.scratch = e->sinc_scratch.p, a.scratch_bytes = e->sinc_scratch.cap;
    // rows beyond the grid limit of sk_downsample_f32_dev's launches go in parts (an even number of rows each: whole streams)
    const uint64_t rows = (uint64_t)n_streams * channels;
    const uint64_t rows_per_launch = 65535ull * sk::sinc_rows_per_block();
    for (uint64_t r0 = 0; r0 < rows; r0 += rows_per_launch) {
        sk::SincS16Args part = a;
        part.rows = (uint32_t)std::min<uint64_t>(rows_per_launch, rows - r0);
        const size_t stream0 = (size_t)(r0 / channels);
        part.in16 = d_pcm16 + stream0 * stream_stride;
        if (d_out16) part.out16 = d_out16 + stream0 * out_stride * channels;
        else part.out32 = d_out32 + (size_t)r0 * out_stride;
        SK_HIP(sk::launch_sinc_rows_s16(part, e->stream), "launch sinc resample (s16 frame rows)");
    }
    SK_HIP(hipStreamSynchronize(e->stream), "resample sync");  // the index set lives in host memory until the copy is done
    return SK_OK;
}

int sk_downsample_frames_s16_to_s16_dev(sk_engine *e, const int16_t *d_pcm16, size_t stream_stride, size_t frame_stride, uint32_t channels,
                                        uint32_t n_streams, uint32_t frames_per_stream, uint32_t in_hz, uint32_t out_hz, int16_t *d_out,
                                        size_t out_stride, uint32_t *out_frames) try {
    sk::abi_enter();
    return sinc_from_s16(e, d_pcm16, stream_stride, frame_stride, channels, n_streams, frames_per_stream, in_hz, out_hz, d_out, nullptr,
                         out_stride, out_frames);
} catch (...) {
    return sk::abi_caught("sk_downsample_frames_s16_to_s16_dev");
}

int sk_downsample_frames_s16_to_f32_dev(sk_engine *e, const int16_t *d_pcm16, size_t stream_stride, size_t frame_stride, uint32_t channels,
                                        uint32_t n_streams, uint32_t frames_per_stream, uint32_t in_hz, uint32_t out_hz, float *d_out,
                                        size_t out_stride, uint32_t *out_frames) try {
    sk::abi_enter();
    return sinc_from_s16(e, d_pcm16, stream_stride, frame_stride, channels, n_streams, frames_per_stream, in_hz, out_hz, nullptr, d_out,
                         out_stride, out_frames);
} catch (...) {
    return sk::abi_caught("sk_downsample_frames_s16_to_f32_dev");
}

int sk_downsample_f32(sk_engine *e, const float *in, uint32_t rows, uint32_t frames, uint32_t in_hz, uint32_t out_hz,
                      float *out, uint32_t out_cap, uint32_t *out_frames) try {
    sk::abi_enter();
    if (!e) return SK_ERR_INVALID_ARG;
    if (!common_rate(in_hz) || !common_rate(out_hz)) return SK_ERR_UNSUPPORTED;
    const uint32_t n_out = sk_downsample_out_frames(frames, in_hz, out_hz);
    if (out_frames) *out_frames = n_out;
    if (rows == 0 || n_out == 0) return SK_OK;
    if (!in || !out || out_cap < n_out) return SK_ERR_INVALID_ARG;
    const size_t in_stride = ((size_t)frames + 3) & ~(size_t)3, out_stride = ((size_t)n_out + 3) & ~(size_t)3;
    {
        std::lock_guard<std::mutex> lock(e->mu);
        DeviceGuard guard(e);
        SK_HIP(e->in_buf.reserve(rows * in_stride * 4), "alloc staging");
        SK_HIP(e->out_buf.reserve(rows * out_stride * 4), "alloc staging");
        SK_HIP(hipMemcpy2DAsync(e->in_buf.p, in_stride * 4, in, (size_t)frames * 4, (size_t)frames * 4, rows,
                                hipMemcpyHostToDevice, e->stream), "H2D resample input");
    }
    int rc = sk_downsample_f32_dev(e, (const float *)e->in_buf.p, in_stride, rows, frames, in_hz, out_hz,
                                   (float *)e->out_buf.p, out_stride, nullptr);
    if (rc != SK_OK) return rc;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    SK_HIP(hipMemcpy2DAsync(out, (size_t)out_cap * 4, e->out_buf.p, out_stride * 4, (size_t)n_out * 4, rows,
                            hipMemcpyDeviceToHost, e->stream), "D2H resample output");
    SK_HIP(hipStreamSynchronize(e->stream), "resample sync");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_downsample_f32");
}

// ---- MPEG Layer III hybrid synthesis (mp3_hybrid.hip) -------------------------------------------------------------------
namespace {

constexpr size_t kMp3Imdct = 4 * 36 * 20, kMp3Matrix = 64 * 32, kMp3Window = 512;

// ISO/IEC 11172-3 2.4.3.4.10.2-3: the IMDCT of each block type with its window folded in, as a 36 x 18 matrix (rows
// padded to 20); block type 2 = three 12-point transforms of the window-interleaved lines, placed at 6 w + 6
void mp3_imdct_matrices(std::vector<float> &out) {
    const double pi = 3.14159265358979323846;
    out.assign(kMp3Imdct, 0.0f);
    for (int bt = 0; bt < 4; ++bt)
        for (int i = 0; i < 36; ++i)
            for (int k = 0; k < 18; ++k) {
                double v = 0.0;
                if (bt != 2) {
                    double w;
                    if (bt == 0) w = std::sin(pi / 36 * (i + 0.5));
                    else if (bt == 1) w = i < 18 ? std::sin(pi / 36 * (i + 0.5)) : (i < 24 ? 1.0 : (i < 30 ? std::sin(pi / 12 * (i - 18 + 0.5)) : 0.0));
                    else w = i < 6 ? 0.0 : (i < 12 ? std::sin(pi / 12 * (i - 6 + 0.5)) : (i < 18 ? 1.0 : std::sin(pi / 36 * (i + 0.5))));
                    v = std::cos(pi / 72 * (2 * i + 1 + 18) * (2 * k + 1)) * w;
                } else {
                    const int w = k % 3, m = k / 3, p = i - 6 * w - 6;
                    if (p >= 0 && p < 12) v = std::cos(pi / 24 * (2 * p + 1 + 6) * (2 * m + 1)) * std::sin(pi / 12 * (p + 0.5));
                }
                out[((size_t)bt * 36 + i) * 20 + k] = (float)v;
            }
}

int ensure_mp3(sk_engine *e) {
    if (e->d_mp3_tables) return SK_OK;
    const double pi = 3.14159265358979323846;
    std::vector<float> t;
    mp3_imdct_matrices(t);
    for (int i = 0; i < 64; ++i)
        for (int k = 0; k < 32; ++k) t.push_back((float)std::cos((16 + i) * (2 * k + 1) * pi / 64));
    t.resize(kMp3Imdct + kMp3Matrix + kMp3Window, 0.0f);  // the window stays zero until the caller sets it
    static const double c[8] = {-0.6, -0.535, -0.33, -0.185, -0.095, -0.041, -0.0142, -0.0037};  // ISO 11172-3 Table B.9
    for (int i = 0; i < 8; ++i) t.push_back((float)(1.0 / std::sqrt(1.0 + c[i] * c[i])));
    for (int i = 0; i < 8; ++i) t.push_back((float)(c[i] / std::sqrt(1.0 + c[i] * c[i])));
    for (int i = 0; i < 64; ++i) t.push_back((float)std::pow(2.0, 1.0 - i / 3.0));  // Layer I / II scale factors (11172-3 Table B.1 in closed form)
    SK_HIP(hipMalloc((void **)&e->d_mp3_tables, t.size() * sizeof(float)), "alloc mp3 tables");
    SK_HIP(hipMemcpy(e->d_mp3_tables, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice), "upload mp3 tables");
    const size_t state_bytes = (size_t)e->max_streams * 2 * sk::kMp3StateFloats * sizeof(float);
    SK_HIP(hipMalloc((void **)&e->d_mp3_state, state_bytes), "alloc mp3 state");
    SK_HIP(hipMemset(e->d_mp3_state, 0, state_bytes), "clear mp3 state");
    return SK_OK;
}

// e->mu held, device selected
// rows (device_ptrs only): where granule i's first channel sits in xr / pcm_out, in 576-line rows, when the granules are not
// packed back to back (sk_mp3_decode_frames_*: the rows of dropped frames lie in between)
int mp3_synthesize_locked(sk_engine *e, const sk_mp3_granule_desc *descs, const float *xr, void *pcm_out, uint32_t n, int32_t *status,
                          bool s16, bool device_ptrs, const uint32_t *rows = nullptr) {
    int rc = ensure_mp3(e);
    if (rc != SK_OK) return rc;
    if (!e->mp3_window_set) return SK_ERR_UNSUPPORTED;  // no synthesis window: sk_mp3_set_synthesis_window first
    // one task per (stream, channel), granules in array order (the AAC plan's layout with 576-line units)
    std::vector<uint32_t> touched;
    std::vector<uint8_t> ok(n, 0);
    // a call with a channel count outside 1..2 is rejected as a whole -- before the loop below starts counting in
    // state_count, which the AAC plan builder shares and expects to find all-zero
    for (uint32_t i = 0; i < n; ++i)
        if (descs[i].channels < 1 || descs[i].channels > SK_MAX_CHANNELS) return SK_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i) {
        const sk_mp3_granule_desc &d = descs[i];
        int32_t st = SK_FRAME_OK;
        if (!stream_ok(e, d.stream)) st = SK_FRAME_BAD_STREAM;
        else if (d.channels != e->streams[d.stream].channels) st = SK_FRAME_BAD_CHANNELS;
        else
            for (uint32_t c = 0; c < d.channels; ++c)
                if (d.block_type[c] > 3 || d.mixed_block_flag[c] > 1) st = SK_FRAME_BAD_WINDOW;
        if (status) status[i] = st;
        if (st != SK_FRAME_OK) continue;
        ok[i] = 1;
        for (uint32_t c = 0; c < d.channels; ++c)
            if (e->state_count[d.stream * 2 + c]++ == 0) touched.push_back(d.stream * 2 + c);
    }
    std::vector<sk::SynthTask> tasks(touched.size());
    uint32_t n_entries = 0;
    for (size_t t = 0; t < touched.size(); ++t) {
        tasks[t] = sk::SynthTask{touched[t], n_entries, 0, 0};
        n_entries += e->state_count[touched[t]];
        e->state_task[touched[t]] = (uint32_t)t;
    }
    std::vector<sk::SynthEntry> entries(n_entries);
    uint64_t off = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const sk_mp3_granule_desc &d = descs[i];
        if (ok[i])
            for (uint32_t c = 0; c < d.channels; ++c) {
                sk::SynthTask &t = tasks[e->state_task[d.stream * 2 + c]];
                entries[t.begin + t.count++] = sk::SynthEntry{(uint32_t)((rows ? rows[i] : off) + c), (uint32_t)d.block_type[c] | ((uint32_t)d.mixed_block_flag[c] << 2) |
                                                                                       ((uint32_t)(d.channels - 1) << 3) | (c << 4)};
            }
        off += d.channels;
    }
    for (uint32_t state : touched) e->state_count[state] = 0;
    if (off * 576 > 0xffffffffull) return SK_ERR_INVALID_ARG;
    const size_t elems = (size_t)off * 576, out_bytes = elems * (s16 ? sizeof(int16_t) : sizeof(float));
    sk::Mp3Args a{};
    a.state = e->d_mp3_state;
    a.n_tasks = (uint32_t)tasks.size();
    a.imdct = e->d_mp3_tables;
    a.matrix = a.imdct + kMp3Imdct;
    a.window = a.matrix + kMp3Matrix;
    a.cs_ca = a.window + kMp3Window;
    SK_HIP(e->aux2_buf.reserve(tasks.size() * sizeof(sk::SynthTask) + entries.size() * sizeof(sk::SynthEntry) + 512), "alloc mp3 schedule");
    sk::SynthTask *d_tasks = (sk::SynthTask *)e->aux2_buf.p;
    sk::SynthEntry *d_entries = (sk::SynthEntry *)((uint8_t *)e->aux2_buf.p + ((tasks.size() * sizeof(sk::SynthTask) + 255) & ~(size_t)255));
    SK_HIP(hipMemcpyAsync(d_tasks, tasks.data(), tasks.size() * sizeof(sk::SynthTask), hipMemcpyHostToDevice, e->stream), "H2D mp3 tasks");
    SK_HIP(hipMemcpyAsync(d_entries, entries.data(), entries.size() * sizeof(sk::SynthEntry), hipMemcpyHostToDevice, e->stream),
           "H2D mp3 entries");
    SK_HIP(hipStreamSynchronize(e->stream), "mp3 schedule sync");  // the vectors go out of scope
    a.tasks = d_tasks;
    a.entries = d_entries;
    if (device_ptrs) {
        a.xr = xr;
        if (s16) a.pcm16 = (int16_t *)pcm_out;
        else a.pcm = (float *)pcm_out;
        if (!tasks.empty()) SK_HIP(sk::launch_mp3_hybrid(a, e->stream), "launch mp3 hybrid synthesis");
        return SK_OK;
    }
    SK_HIP(e->in_buf.reserve(elems * sizeof(float) + 16), "alloc mp3 input");
    SK_HIP(e->out_buf.reserve(elems * sizeof(float) + 16), "alloc mp3 output");
    SK_HIP(hipMemcpyAsync(e->in_buf.p, xr, elems * sizeof(float), hipMemcpyHostToDevice, e->stream), "H2D mp3 lines");
    SK_HIP(hipMemsetAsync(e->out_buf.p, 0, out_bytes, e->stream), "clear mp3 output");  // rejected granules stay silent
    a.xr = (const float *)e->in_buf.p;
    if (s16) a.pcm16 = (int16_t *)e->out_buf.p;
    else a.pcm = (float *)e->out_buf.p;
    if (!tasks.empty()) SK_HIP(sk::launch_mp3_hybrid(a, e->stream), "launch mp3 hybrid synthesis");
    SK_HIP(hipMemcpyAsync(pcm_out, e->out_buf.p, out_bytes, hipMemcpyDeviceToHost, e->stream), "D2H mp3 pcm");
    SK_HIP(hipStreamSynchronize(e->stream), "mp3 sync");
    return SK_OK;
}

int mp3_synthesize(sk_engine *e, const sk_mp3_granule_desc *descs, const float *xr, void *pcm_out, uint32_t n, int32_t *status,
                   bool s16, bool device_ptrs) {
    if (!e || (n && (!descs || !xr || !pcm_out))) return SK_ERR_INVALID_ARG;
    if (n == 0) return SK_OK;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    return mp3_synthesize_locked(e, descs, xr, pcm_out, n, status, s16, device_ptrs);
}

}  // namespace

int sk_mp3_set_synthesis_window(sk_engine *e, const float *d512) try {
    sk::abi_enter();
    if (!e || !d512) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    const int rc = ensure_mp3(e);
    if (rc != SK_OK) return rc;
    SK_HIP(hipMemcpy(e->d_mp3_tables + kMp3Imdct + kMp3Matrix, d512, kMp3Window * sizeof(float), hipMemcpyHostToDevice), "upload mp3 window");
    e->mp3_window_set = true;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_mp3_set_synthesis_window");
}

int sk_mp3_hybrid_synthesize_f32(sk_engine *e, const sk_mp3_granule_desc *descs, const float *xr, float *pcm_out, uint32_t n,
                                 int32_t *status) try {
    sk::abi_enter();
    return mp3_synthesize(e, descs, xr, pcm_out, n, status, false, false);
} catch (...) {
    return sk::abi_caught("sk_mp3_hybrid_synthesize_f32");
}

int sk_mp3_hybrid_synthesize_s16(sk_engine *e, const sk_mp3_granule_desc *descs, const float *xr, int16_t *pcm_out, uint32_t n,
                                 int32_t *status) try {
    sk::abi_enter();
    return mp3_synthesize(e, descs, xr, pcm_out, n, status, true, false);
} catch (...) {
    return sk::abi_caught("sk_mp3_hybrid_synthesize_s16");
}

int sk_mp3_hybrid_synthesize_f32_dev(sk_engine *e, const sk_mp3_granule_desc *descs, const float *d_xr, float *d_pcm, uint32_t n,
                                     int32_t *status) try {
    sk::abi_enter();
    return mp3_synthesize(e, descs, d_xr, d_pcm, n, status, false, true);
} catch (...) {
    return sk::abi_caught("sk_mp3_hybrid_synthesize_f32_dev");
}

// ---- Layer III requantisation / stereo / reorder (mp3_requant.hip) -----------------------------------------------------------
namespace {

constexpr size_t kRqFloats = sk::kMp3Pow43 + 4 + 8;
constexpr size_t kRqBandsAt = kRqFloats * sizeof(float), kRqPretabAt = kRqBandsAt + sk::kMp3Rates * sk::kMp3BandRow * sizeof(uint16_t),
                 kRqMapAt = (kRqPretabAt + sk::kMp3Rates * 24 + 255) & ~(size_t)255, kRqBytes = kRqMapAt + sk::kMp3Rates * 3 * 576 * sizeof(uint32_t);

int mp3_rate_slot(uint32_t hz) {
    static const uint32_t rates[sk::kMp3Rates] = {44100, 48000, 32000, 22050, 24000, 16000, 11025, 12000, 8000};
    for (uint32_t i = 0; i < sk::kMp3Rates; ++i)
        if (rates[i] == hz) return (int)i;
    return -1;
}

int ensure_mp3_requant(sk_engine *e) {
    if (e->d_mp3_rq) return SK_OK;
    const double pi = 3.14159265358979323846;
    std::vector<uint8_t> blob(kRqBytes, 0);
    float *f = (float *)blob.data();
    for (uint32_t v = 0; v < sk::kMp3Pow43; ++v) f[v] = (float)std::pow((double)v, 4.0 / 3.0);
    for (int i = 0; i < 4; ++i) f[sk::kMp3Pow43 + i] = (float)std::pow(2.0, i / 4.0);
    for (int i = 0; i < 7; ++i) {
        const double t = i == 6 ? 0.0 : std::tan(i * pi / 12);
        f[sk::kMp3Pow43 + 4 + i] = i == 6 ? 1.0f : (float)(t / (1.0 + t));  // is_pos 6: tan = infinity, all of it goes left
    }
    SK_HIP(hipMalloc((void **)&e->d_mp3_rq, kRqBytes), "alloc mp3 requantisation tables");
    SK_HIP(hipMemcpy(e->d_mp3_rq, blob.data(), kRqBytes, hipMemcpyHostToDevice), "upload mp3 requantisation tables");
    return SK_OK;
}

}  // namespace

int sk_mp3_set_band_tables(sk_engine *e, uint32_t sample_rate, const uint16_t *long_offsets, const uint16_t *short_offsets,
                           const uint8_t *pretab) try {
    sk::abi_enter();
    if (!e || !long_offsets || !short_offsets || !pretab) return SK_ERR_INVALID_ARG;
    const int slot = mp3_rate_slot(sample_rate);
    if (slot < 0) return SK_ERR_UNSUPPORTED;
    // a partition of the 576 lines (long) / of the 192 lines of one window (short): the kernel's searches rely on it
    if (long_offsets[0] != 0 || long_offsets[22] != 576 || short_offsets[0] != 0 || short_offsets[13] != 192) return SK_ERR_INVALID_ARG;
    for (int i = 0; i < 22; ++i)
        if (long_offsets[i] >= long_offsets[i + 1]) return SK_ERR_INVALID_ARG;
    for (int i = 0; i < 13; ++i)
        if (short_offsets[i] >= short_offsets[i + 1]) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    const int rc = ensure_mp3_requant(e);
    if (rc != SK_OK) return rc;
    uint16_t *row = e->mp3_bands[slot];
    std::memset(row, 0, sizeof e->mp3_bands[slot]);
    std::memcpy(row, long_offsets, 23 * sizeof(uint16_t));
    std::memcpy(row + 23, short_offsets, 14 * sizeof(uint16_t));
    // a mixed block is long below line 36 and short from there on: possible only if both tables have a boundary there
    row[37] = 0xffff;
    bool short_at_36 = false;
    for (int i = 0; i < 14; ++i) short_at_36 |= 3 * short_offsets[i] == 36;
    for (int i = 0; i < 23; ++i)
        if (long_offsets[i] == 36 && short_at_36) row[37] = (uint16_t)i;
    uint8_t pre[24] = {};
    std::memcpy(pre, pretab, 22);
    SK_HIP(hipMemcpy(e->d_mp3_rq + kRqBandsAt + (size_t)slot * sk::kMp3BandRow * sizeof(uint16_t), row, sk::kMp3BandRow * sizeof(uint16_t),
                     hipMemcpyHostToDevice),
           "upload mp3 band table");
    SK_HIP(hipMemcpy(e->d_mp3_rq + kRqPretabAt + (size_t)slot * 24, pre, 24, hipMemcpyHostToDevice), "upload mp3 pre-emphasis table");
    // where every bitstream-order line sits, for the three ways a granule can be cut up (mp3_requant.hip)
    std::vector<uint32_t> map(3 * 576, 0);
    for (int layout = 0; layout < 3; ++layout)
        for (int i = 0; i < 576; ++i) {
            const bool short_line = layout == 1 || (layout == 2 && i >= 36);
            uint32_t band = 0, win = 0, dest = (uint32_t)i;
            if (!short_line) {
                while (band < 21 && long_offsets[band + 1] <= i) ++band;
            } else {
                while (band < 12 && 3 * short_offsets[band + 1] <= i) ++band;
                const int begin = short_offsets[band], width = short_offsets[band + 1] - begin, rel = i - 3 * begin;
                const int w = rel / width;
                win = (uint32_t)w + 1;
                dest = (uint32_t)(3 * (begin + rel - w * width) + w);
            }
            map[(size_t)layout * 576 + i] = dest | (band << 10) | (win << 15);
        }
    SK_HIP(hipMemcpy(e->d_mp3_rq + kRqMapAt + (size_t)slot * 3 * 576 * sizeof(uint32_t), map.data(), map.size() * sizeof(uint32_t), hipMemcpyHostToDevice),
           "upload mp3 line map");
    e->mp3_bands_set[slot] = true;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_mp3_set_band_tables");
}

namespace {

// what the kernel gets of one granule, and the host's verdict on it (a rejected granule: slot 0xff, the kernel writes silence)
int32_t mp3_requant_record(const sk_engine *e, const sk_mp3_requant_granule &g, uint32_t off, sk::Mp3RequantRecord &r) {
    std::memset(&r, 0, sizeof r);
    r.off = off;
    r.channels = g.channels;
    const int slot = mp3_rate_slot(g.sample_rate);
    const bool joint = g.channels == 2 && (g.ms_stereo || g.intensity_stereo);
    int32_t st = SK_OK;
    if (slot < 0 || !e->mp3_bands_set[slot]) st = SK_MP3_UNSUPPORTED;  // no band table for this rate: sk_mp3_set_band_tables first
    for (uint32_t c = 0; c < g.channels && st == SK_OK; ++c) {
        const sk_mp3_requant_channel &ch = g.ch[c];
        if (ch.block_type > 3 || ch.mixed_block_flag > 1 || ch.scalefac_scale > 1 || ch.preflag > 1 || (ch.mixed_block_flag && ch.block_type != 2))
            st = SK_MP3_INVALID;
        else if (ch.mixed_block_flag && e->mp3_bands[slot][37] == 0xffff) st = SK_MP3_UNSUPPORTED;
    }
    if (st == SK_OK && joint) {
        // the stereo step pairs line i of one channel with line i of the other: both must be cut up the same way
        if ((g.ch[0].block_type == 2) != (g.ch[1].block_type == 2) || g.ch[0].mixed_block_flag != g.ch[1].mixed_block_flag) st = SK_MP3_INVALID;
    }
    r.slot = st == SK_OK ? (uint8_t)slot : 0xff;
    r.flags = joint ? (uint8_t)((g.ms_stereo ? 1 : 0) | (g.intensity_stereo ? 2 : 0) | (g.lsf ? 4 : 0) | ((g.intensity_stereo & 2) ? 8 : 0)) : 0;
    r.ch[0] = g.ch[0];
    if (g.channels == 2) r.ch[1] = g.ch[1];
    return st;
}

// e->mu held, device selected: records + integers up, the kernel; the lines stay on the device in e->out_buf.  pcm_bytes: room
// the caller wants in e->in_buf afterwards (the kernel is done with it by then in stream order) -- reserved HERE, before
// anything is enqueued, because DevBuf::reserve frees what it replaces.
int mp3_requantize_locked(sk_engine *e, const sk_mp3_requant_granule *granules, const int16_t *is, uint32_t n, int32_t *status, size_t pcm_bytes,
                          size_t *lines_out) {
    int rc = ensure_mp3_requant(e);
    if (rc != SK_OK) return rc;
    std::vector<sk::Mp3RequantRecord> records(n);
    uint64_t off = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const int32_t st = mp3_requant_record(e, granules[i], (uint32_t)off, records[i]);
        off += granules[i].channels;
        if (status) status[i] = st;
    }
    if (off * 576 > 0xffffffffull) return SK_ERR_INVALID_ARG;
    const size_t lines = (size_t)off * 576, rec_bytes = (size_t)n * sizeof(sk::Mp3RequantRecord);
    const size_t is_at = (rec_bytes + 255) & ~(size_t)255;
    SK_HIP(e->in_buf.reserve(std::max(is_at + lines * sizeof(int16_t), pcm_bytes) + 16), "alloc mp3 requantisation input");
    SK_HIP(e->out_buf.reserve(lines * sizeof(float) + 16), "alloc mp3 requantisation output");
    uint8_t *d_in = (uint8_t *)e->in_buf.p;
    SK_HIP(hipMemcpyAsync(d_in, records.data(), rec_bytes, hipMemcpyHostToDevice, e->stream), "H2D mp3 granule records");
    SK_HIP(hipMemcpyAsync(d_in + is_at, is, lines * sizeof(int16_t), hipMemcpyHostToDevice, e->stream), "H2D mp3 quantised lines");
    SK_HIP(hipStreamSynchronize(e->stream), "mp3 requantisation upload");  // the records go out of scope
    sk::Mp3RequantArgs a{};
    a.records = (const sk::Mp3RequantRecord *)d_in;
    a.is = (const int16_t *)(d_in + is_at);
    a.xr = (float *)e->out_buf.p;
    a.n = n;
    a.pow43 = (const float *)e->d_mp3_rq;
    a.root4 = a.pow43 + sk::kMp3Pow43;
    a.is_k = a.root4 + 4;
    a.bands = (const uint16_t *)(e->d_mp3_rq + kRqBandsAt);
    a.pretab = e->d_mp3_rq + kRqPretabAt;
    a.line_map = (const uint32_t *)(e->d_mp3_rq + kRqMapAt);
    SK_HIP(sk::launch_mp3_requant(a, e->stream), "launch mp3 requantisation");
    *lines_out = lines;
    return SK_OK;
}

// requantisation and hybrid synthesis back to back, the lines never leaving the device: what sk_mp3_decoder_decode_* runs
int mp3_decode_granules(sk_engine *e, const sk_mp3_requant_granule *granules, const sk_mp3_granule_desc *descs, const int16_t *is, void *pcm_out,
                        uint32_t n, int32_t *status, bool s16) {
    if (!e || (n && (!granules || !descs || !is || !pcm_out))) return SK_ERR_INVALID_ARG;
    if (n == 0) return SK_OK;
    size_t rows = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (granules[i].channels < 1 || granules[i].channels > 2 || descs[i].channels != granules[i].channels) return SK_ERR_INVALID_ARG;
        rows += granules[i].channels;
    }
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    const size_t pcm_bytes = rows * 576 * (s16 ? sizeof(int16_t) : sizeof(float));
    size_t lines = 0;
    std::vector<int32_t> requant_status(n, 0);
    int rc = mp3_requantize_locked(e, granules, is, n, requant_status.data(), pcm_bytes, &lines);
    if (rc != SK_OK) return rc;
    SK_HIP(hipMemsetAsync(e->in_buf.p, 0, pcm_bytes, e->stream), "clear mp3 output");  // granules the synthesis rejects stay silent
    rc = mp3_synthesize_locked(e, descs, (const float *)e->out_buf.p, e->in_buf.p, n, status, s16, true);
    if (rc != SK_OK) return rc;
    SK_HIP(hipMemcpyAsync(pcm_out, e->in_buf.p, pcm_bytes, hipMemcpyDeviceToHost, e->stream), "D2H mp3 pcm");
    SK_HIP(hipStreamSynchronize(e->stream), "mp3 decode sync");
    if (status)
        for (uint32_t i = 0; i < n; ++i)
            if (status[i] == SK_OK) status[i] = requant_status[i];
    return SK_OK;
}

}  // namespace

// ---- Layer III parts 2 + 3 on the device (mp3_entropy.hip) -------------------------------------------------------------------

namespace {

// Lanes of a wave that carry a granule-channel: 64 >> shift.  A wave runs the union of its lanes' paths and until its slowest
// lane is done; fewer items per wave means more waves to hide the table and bitstream latencies behind (the same trade as
// EntropyArgs::lane_shift).  SK_MP3_ENTROPY_LANE_SHIFT=0..3 overrides the default for measurements (profiles/r05_mp3_entropy.md).
uint32_t mp3_entropy_lane_shift() {
    static const uint32_t shift = [] {
        const char *s = std::getenv("SK_MP3_ENTROPY_LANE_SHIFT");
        const int v = s ? std::atoi(s) : 0;
        return (uint32_t)(v < 0 ? 0 : (v > 3 ? 3 : v));
    }();
    return shift;
}

// INVALID_ARG for a frame list the kernel must not see; *rows = 576-line rows of all frames together
int mp3_check_frames(const sk_mp3_frame_item *frames, uint32_t n, size_t main_len, uint64_t *rows) {
    if (main_len > 0xffffffffull - 16) return SK_ERR_INVALID_ARG;
    uint64_t r = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const sk_mp3_frame_item &f = frames[i];
        if (f.side.granules < 1 || f.side.granules > 2 || f.side.channels < 1 || f.side.channels > 2) return SK_ERR_INVALID_ARG;
        // (a 13818-3 scalefac_compress has 9 bits: beyond that the scale-factor lengths it stands for exceed a word)
        if (f.header.version != 1)
            for (int c = 0; c < f.side.channels; ++c)
                if (f.side.gr[0][c].scalefac_compress > 511) return SK_ERR_INVALID_ARG;
        if ((f.byte_offset & 3u) || f.byte_len > (1u << 20) || (uint64_t)f.byte_offset + f.byte_len + 8 > main_len) return SK_ERR_INVALID_ARG;
        r += (uint64_t)f.side.granules * f.side.channels;
    }
    if (r * 576 > 0xffffffffull || (uint64_t)n * 4 > 0xffffffffull) return SK_ERR_INVALID_ARG;
    *rows = r;
    return SK_OK;
}

struct Mp3EntropyOut {  // where a launch left its results (e->mp3e_out)
    sk::Mp3EntropyCell *cells = nullptr;
    int32_t *status = nullptr;  // [n_frames * 4]
};

// e->mu held, device selected, frames checked.  Frame i's integers go to d_is + (first_row[i] + granule * channels + channel) * 576;
// with d_records its scale factors go to record first_record[i] + granule.  Returns with the kernel queued.
// bytes == nullptr: the main data of the engine's previous launch is still in place (same main_len), only the frame list differs.
int mp3_entropy_launch(sk_engine *e, const sk_mp3_frame_item *frames, uint32_t n, const uint8_t *bytes, size_t main_len, int16_t *d_is,
                       const uint32_t *first_row, sk::Mp3RequantRecord *d_records, const uint32_t *first_record, Mp3EntropyOut *out) {
    if (!e->d_mp3_cb) return SK_ERR_UNSUPPORTED;  // no code book on this engine: sk_mp3_set_codebook first
    std::vector<sk::Mp3EntropyItem> items;
    items.reserve((size_t)n * 4);
    for (uint32_t i = 0; i < n; ++i) {
        const sk_mp3_side_info &side = frames[i].side;
        for (uint32_t gr = 0; gr < side.granules; ++gr)
            for (uint32_t ch = 0; ch < side.channels; ++ch)
                items.push_back(sk::Mp3EntropyItem{i, first_row[i] + gr * side.channels + ch, d_records ? first_record[i] + gr : 0xffffffffu, (uint8_t)gr, (uint8_t)ch, {0, 0}});
    }
    // a wave's lanes should have about the same number of codes to read: longest granule-channels first
    std::stable_sort(items.begin(), items.end(), [&](const sk::Mp3EntropyItem &a, const sk::Mp3EntropyItem &b) {
        return frames[a.frame].side.gr[a.gr][a.ch].part2_3_length > frames[b.frame].side.gr[b.gr][b.ch].part2_3_length;
    });
    auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t frames_bytes = (size_t)n * sizeof(sk_mp3_frame_item), items_bytes = items.size() * sizeof(sk::Mp3EntropyItem);
    // main data | frames | items: the main data first, so that a second launch over fewer frames finds it where it was
    const size_t bytes_at = 0, frames_at = up256(main_len + 16), items_at = frames_at + up256(frames_bytes);
    const size_t cells_bytes = (size_t)n * 4 * sizeof(sk::Mp3EntropyCell), status_at = up256(cells_bytes);
    if (!bytes && e->mp3e_in.cap < items_at + items_bytes) return SK_ERR_INTERNAL;  // (a first launch over more frames made the room)
    SK_HIP(e->mp3e_in.reserve(items_at + items_bytes + 16), "alloc mp3 entropy input");
    SK_HIP(e->mp3e_out.reserve(status_at + (size_t)n * 4 * sizeof(int32_t)), "alloc mp3 entropy output");
    uint8_t *d_in = (uint8_t *)e->mp3e_in.p, *d_out = (uint8_t *)e->mp3e_out.p;
    SK_HIP(hipMemcpyAsync(d_in + frames_at, frames, frames_bytes, hipMemcpyHostToDevice, e->stream), "H2D mp3 frames");
    SK_HIP(hipMemcpyAsync(d_in + items_at, items.data(), items_bytes, hipMemcpyHostToDevice, e->stream), "H2D mp3 entropy items");
    if (bytes) SK_HIP(hipMemcpyAsync(d_in + bytes_at, bytes, main_len, hipMemcpyHostToDevice, e->stream), "H2D mp3 main data");
    SK_HIP(hipMemsetAsync(d_out, 0, status_at + (size_t)n * 4 * sizeof(int32_t), e->stream), "clear mp3 entropy cells");
    SK_HIP(hipStreamSynchronize(e->stream), "mp3 entropy upload");  // the items go out of scope
    sk::Mp3EntropyArgs a{};
    a.blob = e->d_mp3_cb;
    a.lds_words = ((const sk::Mp3CodebookHeader *)e->mp3_cb_host.data())->lds_words;
    a.frames = (const sk_mp3_frame_item *)(d_in + frames_at);
    a.bytes = d_in + bytes_at;
    a.items = (const sk::Mp3EntropyItem *)(d_in + items_at);
    a.n_items = (uint32_t)items.size();
    a.lane_shift = mp3_entropy_lane_shift();
    a.is = d_is;
    a.records = d_records;
    a.cells = (sk::Mp3EntropyCell *)d_out;
    a.status = (int32_t *)(d_out + status_at);
    SK_HIP(sk::launch_mp3_entropy(a, e->stream), "launch mp3 entropy");
    out->cells = a.cells;
    out->status = a.status;
    return SK_OK;
}

int mp3_decode_frames(sk_engine *e, const sk_mp3_frame_item *frames, const uint32_t *streams, uint32_t n, const uint8_t *bytes, size_t main_len,
                      void *pcm_out, size_t out_cap, int32_t *entropy_status, int32_t *stage_status, size_t *written, bool s16) {
    if (!e || !written || (n && (!frames || !streams || !bytes || !entropy_status)) || (out_cap && !pcm_out)) return SK_ERR_INVALID_ARG;
    *written = 0;
    if (n == 0) return SK_OK;
    uint64_t rows = 0;
    int rc = mp3_check_frames(frames, n, main_len, &rows);
    if (rc != SK_OK) return rc;
    for (uint32_t i = 0; i < n; ++i)
        if (frames[i].header.channels != frames[i].side.channels || frames[i].header.granules != frames[i].side.granules) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    rc = ensure_mp3(e);
    if (rc == SK_OK) rc = ensure_mp3_requant(e);
    if (rc != SK_OK) return rc;
    if (!e->mp3_window_set) return SK_ERR_UNSUPPORTED;  // no synthesis window: sk_mp3_set_synthesis_window first
    if (!e->d_mp3_cb) return SK_ERR_UNSUPPORTED;        // no code book: sk_mp3_set_codebook first

    // every frame's granules as the host path would queue them -- the fields that come out of the side information; the
    // scale factors and preflag are the kernel's to fill in
    std::vector<sk::Mp3RequantRecord> records;
    std::vector<sk_mp3_granule_desc> descs;
    std::vector<int32_t> requant_status;
    std::vector<uint32_t> first_row(n), first_record(n);
    uint32_t row = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const sk_mp3_frame_info &h = frames[i].header;
        const sk_mp3_side_info &side = frames[i].side;
        const bool joint = h.mode == 1;
        first_row[i] = row;
        first_record[i] = (uint32_t)records.size();
        for (int gr = 0; gr < side.granules; ++gr) {
            sk_mp3_requant_granule g;
            std::memset(&g, 0, sizeof g);
            g.sample_rate = h.sample_rate;
            g.channels = side.channels;
            g.ms_stereo = joint && (h.mode_ext & 2);
            g.intensity_stereo = joint && (h.mode_ext & 1);
            g.lsf = h.version != 1;
            // sk_mp3_granule_data::intensity_scale of the right channel: scalefac_compress & 1 (13818-3 2.4.3.2)
            if (g.lsf && g.intensity_stereo && side.channels == 2 && (side.gr[gr][1].scalefac_compress & 1)) g.intensity_stereo |= 2;
            sk_mp3_granule_desc desc;
            std::memset(&desc, 0, sizeof desc);
            desc.stream = streams[i];
            desc.channels = side.channels;
            for (int ch = 0; ch < side.channels; ++ch) {
                const sk_mp3_granule_side &s = side.gr[gr][ch];
                sk_mp3_requant_channel &c = g.ch[ch];
                c.global_gain = s.global_gain, c.scalefac_scale = s.scalefac_scale, c.preflag = g.lsf ? 0 : s.preflag;
                c.block_type = s.block_type, c.mixed_block_flag = s.mixed_block_flag;
                std::memcpy(c.subblock_gain, s.subblock_gain, 3);
                desc.block_type[ch] = s.block_type, desc.mixed_block_flag[ch] = s.mixed_block_flag;
            }
            sk::Mp3RequantRecord r;
            requant_status.push_back(mp3_requant_record(e, g, row, r));
            records.push_back(r);
            descs.push_back(desc);
            row += side.channels;
        }
    }
    const uint32_t n_granules = (uint32_t)records.size();
    const size_t width = s16 ? sizeof(int16_t) : sizeof(float);
    const size_t rec_bytes = (size_t)n_granules * sizeof(sk::Mp3RequantRecord), is_at = (rec_bytes + 255) & ~(size_t)255;
    const size_t lines = (size_t)rows * 576;
    // e->in_buf: records | integers, and once the requantisation has read them, the PCM (in stream order); e->out_buf: the lines
    SK_HIP(e->in_buf.reserve(std::max(is_at + lines * sizeof(int16_t), lines * width) + 16), "alloc mp3 frames input");
    SK_HIP(e->out_buf.reserve(lines * sizeof(float) + 16), "alloc mp3 frames lines");
    uint8_t *d_in = (uint8_t *)e->in_buf.p;
    SK_HIP(hipMemcpyAsync(d_in, records.data(), rec_bytes, hipMemcpyHostToDevice, e->stream), "H2D mp3 granule records");
    Mp3EntropyOut eo;
    rc = mp3_entropy_launch(e, frames, n, bytes, main_len, (int16_t *)(d_in + is_at), first_row.data(), (sk::Mp3RequantRecord *)d_in, first_record.data(), &eo);
    if (rc != SK_OK) return rc;
    std::vector<int32_t> cell_status((size_t)n * 4);
    SK_HIP(hipMemcpyAsync(cell_status.data(), eo.status, cell_status.size() * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream), "D2H mp3 entropy statuses");
    SK_HIP(hipStreamSynchronize(e->stream), "mp3 entropy sync");  // the one synchronisation the host stage does not need

    // a frame any of whose granule-channels failed is dropped: no samples, no synthesis, its stream's state untouched
    std::vector<sk_mp3_granule_desc> kept_descs;
    std::vector<uint32_t> kept_rows, kept_granule;
    size_t samples = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const sk_mp3_side_info &side = frames[i].side;
        int32_t worst = SK_OK;
        for (int gr = 0; gr < side.granules; ++gr)
            for (int ch = 0; ch < side.channels; ++ch)
                if (worst == SK_OK) worst = cell_status[(size_t)i * 4 + gr * 2 + ch];
        entropy_status[i] = worst;
        if (stage_status) stage_status[i] = SK_OK;
        if (worst != SK_OK) continue;
        for (int gr = 0; gr < side.granules; ++gr) {
            kept_descs.push_back(descs[first_record[i] + gr]);
            kept_rows.push_back(first_row[i] + (uint32_t)gr * side.channels);
            kept_granule.push_back(first_record[i] + gr);
        }
        samples += (size_t)side.granules * side.channels * 576;
    }
    if (samples > out_cap) return SK_ERR_CAPACITY;
    if (kept_descs.empty()) return SK_OK;

    sk::Mp3RequantArgs a{};
    a.records = (const sk::Mp3RequantRecord *)d_in;
    a.is = (const int16_t *)(d_in + is_at);
    a.xr = (float *)e->out_buf.p;
    a.n = n_granules;
    a.pow43 = (const float *)e->d_mp3_rq;
    a.root4 = a.pow43 + sk::kMp3Pow43;
    a.is_k = a.root4 + 4;
    a.bands = (const uint16_t *)(e->d_mp3_rq + kRqBandsAt);
    a.pretab = e->d_mp3_rq + kRqPretabAt;
    a.line_map = (const uint32_t *)(e->d_mp3_rq + kRqMapAt);
    SK_HIP(sk::launch_mp3_requant(a, e->stream), "launch mp3 requantisation");
    SK_HIP(hipMemsetAsync(e->in_buf.p, 0, lines * width, e->stream), "clear mp3 output");  // granules the synthesis rejects stay silent
    std::vector<int32_t> synth_status(kept_descs.size(), 0);
    rc = mp3_synthesize_locked(e, kept_descs.data(), (const float *)e->out_buf.p, e->in_buf.p, (uint32_t)kept_descs.size(), synth_status.data(), s16, true,
                               kept_rows.data());
    if (rc != SK_OK) return rc;
    // the surviving frames' PCM sits at their rows: runs of neighbours leave in one copy each
    size_t out_at = 0;
    for (uint32_t i = 0; i < n;) {
        if (entropy_status[i] != SK_OK) {
            ++i;
            continue;
        }
        uint32_t j = i;
        size_t run = 0;
        while (j < n && entropy_status[j] == SK_OK) run += (size_t)frames[j].side.granules * frames[j].side.channels * 576, ++j;
        SK_HIP(hipMemcpyAsync((uint8_t *)pcm_out + out_at * width, d_in + (size_t)first_row[i] * 576 * width, run * width, hipMemcpyDeviceToHost, e->stream), "D2H mp3 pcm");
        out_at += run;
        i = j;
    }
    SK_HIP(hipStreamSynchronize(e->stream), "mp3 frames sync");
    if (stage_status) {
        size_t k = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (entropy_status[i] != SK_OK) continue;
            for (int gr = 0; gr < frames[i].side.granules; ++gr, ++k) {
                const int32_t st = synth_status[k] != SK_OK ? synth_status[k] : requant_status[kept_granule[k]];
                if (stage_status[i] == SK_OK) stage_status[i] = st;
            }
        }
    }
    *written = samples;
    return SK_OK;
}


// ---- MPEG Layer I / II (mp12_synth.hip): frames' bytes and records in, PCM out, one launch ------------------------------------
// e->in_buf: bytes | records | tasks | entries; e->out_buf: the PCM of the frames that are launched, in frame order
int mpa_decode_frames(sk_engine *e, const sk_mpa_frame_record *records, const uint32_t *streams, uint32_t n, const uint8_t *bytes, size_t bytes_len,
                      void *pcm_out, size_t out_cap, int32_t *status, size_t *written, bool s16, float *kernel_ms) {
    if (!e || !written || (n && (!records || !streams || !bytes || !status)) || (out_cap && !pcm_out)) return SK_ERR_INVALID_ARG;
    *written = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n == 0) return SK_OK;
    if (bytes_len > (1u << 28)) return SK_ERR_INVALID_ARG;  // bit positions are 32-bit
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    int rc = ensure_mp3(e);
    if (rc != SK_OK) return rc;
    if (!e->mp3_window_set) return SK_ERR_UNSUPPORTED;  // no synthesis window: sk_mp3_set_synthesis_window first

    // what may reach the kernel: a record that adds up, inside the byte buffer with its 8 bytes of room, for an open stream of its shape
    std::vector<uint32_t> touched;
    std::vector<uint32_t> pcm_off(n, 0);
    uint64_t samples = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const sk_mpa_frame_record &r = records[i];
        int32_t st = SK_OK;
        if (!sk_mp12::record_adds_up(r) || (r.byte_offset & 3u) || (uint64_t)r.byte_offset + r.byte_len + 8 > bytes_len) st = SK_MP3_INVALID;
        else if (!stream_ok(e, streams[i])) st = SK_FRAME_BAD_STREAM;
        else if (r.channels != e->streams[streams[i]].channels) st = SK_FRAME_BAD_CHANNELS;
        status[i] = st;
        if (st != SK_OK) continue;
        pcm_off[i] = (uint32_t)samples;
        samples += (uint64_t)(r.layer == 1 ? 384u : 1152u) * r.channels;
        if (samples > 0xffffffffull) break;
    }
    if (samples > 0xffffffffull) return SK_ERR_INVALID_ARG;
    if (samples > out_cap) return SK_ERR_CAPACITY;
    if (samples == 0) return SK_OK;
    for (uint32_t i = 0; i < n; ++i)
        if (status[i] == SK_OK)
            for (uint32_t c = 0; c < records[i].channels; ++c)
                if (e->state_count[streams[i] * 2 + c]++ == 0) touched.push_back(streams[i] * 2 + c);
    std::vector<sk::SynthTask> tasks(touched.size());
    uint32_t n_entries = 0;
    for (size_t t = 0; t < touched.size(); ++t) {
        tasks[t] = sk::SynthTask{touched[t], n_entries, 0, 0};
        n_entries += e->state_count[touched[t]];
        e->state_task[touched[t]] = (uint32_t)t;
    }
    std::vector<sk::Mp12Entry> entries(n_entries);
    for (uint32_t i = 0; i < n; ++i)
        if (status[i] == SK_OK)
            for (uint32_t c = 0; c < records[i].channels; ++c) {
                sk::SynthTask &t = tasks[e->state_task[streams[i] * 2 + c]];
                entries[t.begin + t.count++] = sk::Mp12Entry{i, pcm_off[i]};
            }
    for (uint32_t state : touched) e->state_count[state] = 0;

    auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t width = s16 ? sizeof(int16_t) : sizeof(float);
    const size_t rec_at = up256(bytes_len + 16), rec_bytes = (size_t)n * sizeof(sk_mpa_frame_record);
    const size_t tasks_at = up256(rec_at + rec_bytes), tasks_bytes = tasks.size() * sizeof(sk::SynthTask);
    const size_t entries_at = up256(tasks_at + tasks_bytes), entries_bytes = entries.size() * sizeof(sk::Mp12Entry);
    SK_HIP(e->in_buf.reserve(entries_at + entries_bytes + 16), "alloc mp12 input");
    SK_HIP(e->out_buf.reserve((size_t)samples * width + 16), "alloc mp12 output");
    uint8_t *d_in = (uint8_t *)e->in_buf.p;
    SK_HIP(hipMemcpyAsync(d_in, bytes, bytes_len, hipMemcpyHostToDevice, e->stream), "H2D mp12 frame bytes");
    SK_HIP(hipMemcpyAsync(d_in + rec_at, records, rec_bytes, hipMemcpyHostToDevice, e->stream), "H2D mp12 records");
    SK_HIP(hipMemcpyAsync(d_in + tasks_at, tasks.data(), tasks_bytes, hipMemcpyHostToDevice, e->stream), "H2D mp12 tasks");
    SK_HIP(hipMemcpyAsync(d_in + entries_at, entries.data(), entries_bytes, hipMemcpyHostToDevice, e->stream), "H2D mp12 entries");
    SK_HIP(hipStreamSynchronize(e->stream), "mp12 upload");  // the vectors go out of scope
    sk::Mp12Args a{};
    a.records = (const sk_mpa_frame_record *)(d_in + rec_at);
    a.bytes = (const uint32_t *)d_in;
    if (s16) a.pcm16 = (int16_t *)e->out_buf.p;
    else a.pcm = (float *)e->out_buf.p;
    a.state = e->d_mp3_state;
    a.tasks = (const sk::SynthTask *)(d_in + tasks_at);
    a.entries = (const sk::Mp12Entry *)(d_in + entries_at);
    a.n_tasks = (uint32_t)tasks.size();
    a.matrix = e->d_mp3_tables + kMp3Imdct;
    a.window = a.matrix + kMp3Matrix;
    a.scf = a.window + kMp3Window + 16;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (kernel_ms) {
        SK_HIP(hipEventCreate(&ev0), "mp12 event");
        const hipError_t he = hipEventCreate(&ev1);
        if (he != hipSuccess) {
            (void)hipEventDestroy(ev0);
            return e->hip_fail(he, "mp12 event");
        }
        (void)hipEventRecord(ev0, e->stream);
    }
    hipError_t he = sk::launch_mp12_synth(a, e->stream);
    if (kernel_ms && he == hipSuccess) he = hipEventRecord(ev1, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(pcm_out, e->out_buf.p, (size_t)samples * width, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (kernel_ms) {
        if (he == hipSuccess) he = hipEventElapsedTime(kernel_ms, ev0, ev1);
        (void)hipEventDestroy(ev0);
        (void)hipEventDestroy(ev1);
    }
    if (he != hipSuccess) return e->hip_fail(he, "mp12 synthesis");
    *written = (size_t)samples;
    return SK_OK;
}

}  // namespace

extern "C++" {
namespace sk {

// The engine's device code book := this blob (sk_mp3_codebook_flatten).  Nothing is uploaded when the engine holds it already,
// so that a decoder handle or a scheduler lane may call this before every batch.
int mp3_install_codebook(sk_engine *e, const uint32_t *words, size_t n_words) {
    if (!e || !words || n_words < sizeof(Mp3CodebookHeader) / 4) return SK_ERR_INVALID_ARG;
    const Mp3CodebookHeader &h = *(const Mp3CodebookHeader *)words;
    if (h.words != n_words || h.lds_words > n_words || h.lds_words < sizeof(Mp3CodebookHeader) / 4 || (h.lds_words & 3u) ||
        h.lds_words > sizeof(Mp3CodebookHeader) / 4 + (34u << kMp3L1Bits))
        return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    if (e->d_mp3_cb && e->mp3_cb_host.size() == n_words && std::memcmp(e->mp3_cb_host.data(), words, n_words * sizeof(uint32_t)) == 0) return SK_OK;
    DeviceGuard guard(e);
    SK_HIP(hipStreamSynchronize(e->stream), "mp3 code book: wait for the kernels that read the old one");
    uint32_t *fresh = nullptr;
    SK_HIP(hipMalloc((void **)&fresh, n_words * sizeof(uint32_t) + 16), "alloc mp3 code book");
    const hipError_t he = hipMemcpy(fresh, words, n_words * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (he != hipSuccess) {
        (void)hipFree(fresh);
        return e->hip_fail(he, "upload mp3 code book");
    }
    if (e->d_mp3_cb) (void)hipFree(e->d_mp3_cb);
    e->d_mp3_cb = fresh;
    e->mp3_cb_host.assign(words, words + n_words);
    return SK_OK;
}

}  // namespace sk
}  // extern "C++"

extern "C" {

int sk_mp3_set_codebook(sk_engine *e, const sk_mp3_codebook *cb) try {
    sk::abi_enter();
    if (!e) return SK_ERR_INVALID_ARG;
    sk_mp3_codebook *own = nullptr;
    if (!cb) {
        const int rc = sk_mp3_codebook_create_iso(&own);
        if (rc != SK_OK) return rc;
        cb = own;
    }
    struct Guard {
        sk_mp3_codebook *p;
        ~Guard() { sk_mp3_codebook_destroy(p); }
    } guard{own};
    size_t words = 0;
    int rc = sk_mp3_codebook_flatten(cb, nullptr, 0, &words);
    if (rc != SK_OK && rc != SK_ERR_CAPACITY) return rc;
    std::vector<uint32_t> blob(words);
    rc = sk_mp3_codebook_flatten(cb, blob.data(), blob.size(), &words);
    if (rc != SK_OK) return rc;
    return sk::mp3_install_codebook(e, blob.data(), blob.size());
} catch (...) {
    return sk::abi_caught("sk_mp3_set_codebook");
}

int sk_mp3_entropy_decode(sk_engine *e, const sk_mp3_frame_item *frames, uint32_t n, const uint8_t *bytes, size_t main_len, sk_mp3_granule_data *out) try {
    sk::abi_enter();
    if (!e || (n && (!frames || !bytes || !out))) return SK_ERR_INVALID_ARG;
    if (n == 0) return SK_OK;
    uint64_t rows = 0;
    int rc = mp3_check_frames(frames, n, main_len, &rows);
    if (rc != SK_OK) return rc;
    std::vector<uint32_t> first_row(n);
    uint32_t row = 0;
    for (uint32_t i = 0; i < n; ++i) first_row[i] = row, row += (uint32_t)frames[i].side.granules * frames[i].side.channels;
    std::vector<int16_t> is((size_t)rows * 576);
    std::vector<sk::Mp3EntropyCell> cells((size_t)n * 4);
    {
        std::lock_guard<std::mutex> lock(e->mu);
        DeviceGuard guard(e, ComputeTurn{});
        SK_HIP(e->in_buf.reserve(is.size() * sizeof(int16_t) + 16), "alloc mp3 entropy integers");
        Mp3EntropyOut eo;
        rc = mp3_entropy_launch(e, frames, n, bytes, main_len, (int16_t *)e->in_buf.p, first_row.data(), nullptr, nullptr, &eo);
        if (rc != SK_OK) return rc;
        SK_HIP(hipMemcpyAsync(is.data(), e->in_buf.p, is.size() * sizeof(int16_t), hipMemcpyDeviceToHost, e->stream), "D2H mp3 integers");
        SK_HIP(hipMemcpyAsync(cells.data(), eo.cells, cells.size() * sizeof(sk::Mp3EntropyCell), hipMemcpyDeviceToHost, e->stream), "D2H mp3 entropy cells");
        SK_HIP(hipStreamSynchronize(e->stream), "mp3 entropy sync");
    }
    for (uint32_t i = 0; i < n; ++i) {
        const sk_mp3_side_info &side = frames[i].side;
        for (uint32_t gr = 0; gr < side.granules; ++gr)
            for (uint32_t ch = 0; ch < side.channels; ++ch) {
                const sk::Mp3EntropyCell &c = cells[(size_t)i * 4 + gr * 2 + ch];
                sk_mp3_granule_data &g = out[(size_t)i * 4 + gr * 2 + ch];
                std::memset(&g, 0, sizeof g);
                std::memcpy(g.is, is.data() + ((size_t)first_row[i] + gr * side.channels + ch) * 576, sizeof g.is);
                std::memcpy(g.scalefac_l, c.scalefac_l, sizeof g.scalefac_l);
                std::memcpy(g.scalefac_s, c.scalefac_s, sizeof g.scalefac_s);
                g.preflag = c.preflag, g.intensity_scale = c.intensity_scale;
                g.part2_bits = c.part2_bits, g.nonzero_lines = c.nonzero_lines, g.part3_bits = c.part3_bits;
                g.status = c.status;
            }
    }
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_mp3_entropy_decode");
}

int sk_mp3_decode_frames_f32(sk_engine *e, const sk_mp3_frame_item *frames, const uint32_t *streams, uint32_t n, const uint8_t *bytes, size_t main_len,
                             float *pcm_out, size_t out_cap, int32_t *entropy_status, int32_t *stage_status, size_t *written) try {
    sk::abi_enter();
    return mp3_decode_frames(e, frames, streams, n, bytes, main_len, pcm_out, out_cap, entropy_status, stage_status, written, false);
} catch (...) {
    return sk::abi_caught("sk_mp3_decode_frames_f32");
}

int sk_mp3_decode_frames_s16(sk_engine *e, const sk_mp3_frame_item *frames, const uint32_t *streams, uint32_t n, const uint8_t *bytes, size_t main_len,
                             int16_t *pcm_out, size_t out_cap, int32_t *entropy_status, int32_t *stage_status, size_t *written) try {
    sk::abi_enter();
    return mp3_decode_frames(e, frames, streams, n, bytes, main_len, pcm_out, out_cap, entropy_status, stage_status, written, true);
} catch (...) {
    return sk::abi_caught("sk_mp3_decode_frames_s16");
}

// ---- MPEG Layer I / II: the host front (mp12_bitstream.cpp) and the stage call (mp12_synth.hip) ----
int sk_mpa_parse_header(const uint8_t *d, size_t len, sk_mpa_frame_info *out) try {
    sk::abi_enter();
    return sk_mp12::parse_header(d, len, out);
} catch (...) {
    return sk::abi_caught("sk_mpa_parse_header");
}

int sk_mpa_scan(const uint8_t *d, size_t len, uint32_t *layer, sk_mpa_frame_info *frames, uint32_t cap, uint32_t *n_frames, size_t *consumed) try {
    sk::abi_enter();
    return sk_mp12::scan(d, len, layer, frames, cap, n_frames, consumed);
} catch (...) {
    return sk::abi_caught("sk_mpa_scan");
}

int sk_mpa_parse_frame(const uint8_t *frame, size_t len, const sk_mpa_frame_info *h, sk_mpa_frame_record *out) try {
    sk::abi_enter();
    return sk_mp12::parse_frame(frame, len, h, out);
} catch (...) {
    return sk::abi_caught("sk_mpa_parse_frame");
}

int sk_mpa_decode_frames_f32(sk_engine *e, const sk_mpa_frame_record *records, const uint32_t *streams, uint32_t n, const uint8_t *bytes, size_t bytes_len,
                             float *pcm_out, size_t out_cap, int32_t *status, size_t *written) try {
    sk::abi_enter();
    return mpa_decode_frames(e, records, streams, n, bytes, bytes_len, pcm_out, out_cap, status, written, false, nullptr);
} catch (...) {
    return sk::abi_caught("sk_mpa_decode_frames_f32");
}

int sk_mpa_decode_frames_s16(sk_engine *e, const sk_mpa_frame_record *records, const uint32_t *streams, uint32_t n, const uint8_t *bytes, size_t bytes_len,
                             int16_t *pcm_out, size_t out_cap, int32_t *status, size_t *written) try {
    sk::abi_enter();
    return mpa_decode_frames(e, records, streams, n, bytes, bytes_len, pcm_out, out_cap, status, written, true, nullptr);
} catch (...) {
    return sk::abi_caught("sk_mpa_decode_frames_s16");
}

int sk_mpa_decode_frames_timed(sk_engine *e, const sk_mpa_frame_record *records, const uint32_t *streams, uint32_t n, const uint8_t *bytes, size_t bytes_len,
                               int16_t *pcm_out, size_t out_cap, int32_t *status, size_t *written, float *kernel_ms) try {
    sk::abi_enter();
    if (!kernel_ms) return SK_ERR_INVALID_ARG;
    return mpa_decode_frames(e, records, streams, n, bytes, bytes_len, pcm_out, out_cap, status, written, true, kernel_ms);
} catch (...) {
    return sk::abi_caught("sk_mpa_decode_frames_timed");
}

}  // extern "C"

int sk_mp3_requantize(sk_engine *e, const sk_mp3_requant_granule *granules, const int16_t *is, float *xr, uint32_t n, int32_t *status) try {
    sk::abi_enter();
    if (!e || (n && (!granules || !is || !xr))) return SK_ERR_INVALID_ARG;
    if (n == 0) return SK_OK;
    for (uint32_t i = 0; i < n; ++i)
        if (granules[i].channels < 1 || granules[i].channels > 2) return SK_ERR_INVALID_ARG;  // the layout of is / xr depends on it
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    size_t lines = 0;
    const int rc = mp3_requantize_locked(e, granules, is, n, status, 0, &lines);
    if (rc != SK_OK) return rc;
    SK_HIP(hipMemcpyAsync(xr, e->out_buf.p, lines * sizeof(float), hipMemcpyDeviceToHost, e->stream), "D2H mp3 lines");
    SK_HIP(hipStreamSynchronize(e->stream), "mp3 requantisation sync");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_mp3_requantize");
}

int sk_mp3_decode_granules_f32(sk_engine *e, const sk_mp3_requant_granule *granules, const sk_mp3_granule_desc *descs, const int16_t *is,
                               float *pcm_out, uint32_t n, int32_t *status) try {
    sk::abi_enter();
    return mp3_decode_granules(e, granules, descs, is, pcm_out, n, status, false);
} catch (...) {
    return sk::abi_caught("sk_mp3_decode_granules_f32");
}

int sk_mp3_decode_granules_s16(sk_engine *e, const sk_mp3_requant_granule *granules, const sk_mp3_granule_desc *descs, const int16_t *is,
                               int16_t *pcm_out, uint32_t n, int32_t *status) try {
    sk::abi_enter();
    return mp3_decode_granules(e, granules, descs, is, pcm_out, n, status, true);
} catch (...) {
    return sk::abi_caught("sk_mp3_decode_granules_s16");
}

int sk_resampler_open(sk_engine *e, uint32_t id, uint32_t in_hz, uint32_t out_hz) try {
    sk::abi_enter();
    if (!e) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    if (!stream_ok(e, id)) return SK_ERR_BAD_STREAM;
    if (!common_rate(in_hz) || !common_rate(out_hz)) return SK_ERR_UNSUPPORTED;  // as downsample_audio rejects them
    // the plain guard: opening a resampler queues nothing per stream -- a scheduler opens thousands in a row, and their rows
    // (like their synthesis state) are cleared by ONE launch in front of the next call that touches the device
    DeviceGuard guard(e->device);
    if (!e->d_rs) {
        const size_t bytes = ((size_t)e->max_streams * 2 + (size_t)e->max_wide * 8) * kRsRow * sizeof(float);
        SK_HIP(hipMalloc((void **)&e->d_rs, bytes), "alloc resampler history");
        SK_HIP(hipMemsetAsync(e->d_rs, 0, bytes, e->stream), "clear resampler history");
    }
    int table = -1;
    int rc = ratio_table_for(e, in_hz, out_hz, &table);
    if (rc != SK_OK) return rc;
    StreamInfo &s = e->streams[id];
    s.rs_open = true;
    s.rs_in_hz = in_hz;
    s.rs_out_hz = out_hz;
    s.rs_table = table;
    s.rs_fill = 0;
    s.rs_chunks = 0;
    s.rs_last_index = -128.0;
    queue_rs_reset(e, id);
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_resampler_open");
}

int sk_resampler_close(sk_engine *e, uint32_t id) try {
    sk::abi_enter();
    if (!e) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    if (!stream_ok(e, id)) return SK_ERR_BAD_STREAM;
    e->streams[id].rs_open = false;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_resampler_close");
}

}  // extern "C"

namespace {

struct RsCall {  // one stream's slot in a batched call
    uint32_t id = 0, channels = 0;
    size_t row0 = 0;        // first row of this stream in the call's input / output arrays
    uint32_t consumed = 0;  // input frames appended so far
    uint32_t produced = 0;  // output frames produced so far
    uint32_t trim = 0;      // flush only: frames to drop from the end of the last chunk's output
    std::vector<std::pair<uint32_t, uint32_t>> outs;  // (column, frames) of every chunk processed so far, in order: the AudioData boundaries
};

// bump allocator over a device scratch buffer for the small per-round arrays
struct AuxArena {
    uint8_t *base = nullptr;
    size_t cap = 0, used = 0;
    uint8_t *host = nullptr;  // optional pinned mirror of the same capacity: uploads then need no sync before v is reused
    template <typename T>
    hipError_t put(const std::vector<T> &v, hipStream_t st, const T **out) {
        const size_t bytes = (v.size() * sizeof(T) + 255) & ~(size_t)255;
        if (used + bytes > cap) return hipErrorOutOfMemory;
        *out = reinterpret_cast<const T *>(base + used);
        const void *src = v.data();
        if (host) {
            std::memcpy(host + used, v.data(), v.size() * sizeof(T));
            src = host + used;
        }
        used += bytes;
        if (v.empty()) return hipSuccess;
        return hipMemcpyAsync((void *)*out, src, v.size() * sizeof(T), hipMemcpyHostToDevice, st);
    }
    // the same for an array the kernels write to as well
    template <typename T>
    hipError_t put_rw(const std::vector<T> &v, hipStream_t st, T **out) {
        const T *p = nullptr;
        const size_t at = used;
        const hipError_t he = put(v, st, &p);
        *out = he == hipSuccess ? reinterpret_cast<T *>(base + at) : nullptr;
        return he;
    }
};

// Runs every COMPLETE chunk of every stream of `ready` through its resampler: one launch per resampler state that chunks share
// (the three phases of the 48 -> 16 k FIR; one launch for every other ratio, with a time-index set per row), the chunks as virtual
// rows (kRsBlocks above).  Outputs go to d_out (row stride out_stride) behind each stream's `produced` column, chunk after chunk;
// what is left of the row (history + incomplete chunk) slides to the front; state advances.
int rs_process_ready(sk_engine *e, std::vector<RsCall> &calls, const std::vector<size_t> &ready, float *d_out,
                     size_t out_stride, uint32_t out_cap, AuxArena &aux) {
    struct Item {  // one complete chunk of one stream
        size_t ci;
        uint32_t k, col, count, set_index;
        double last, new_last;
        uint64_t chunk_no;
        int table;
        bool fir;
    };
    struct Key {
        int table;
        double last;
        bool operator<(const Key &o) const { return table != o.table ? table < o.table : last < o.last; }
    };
    struct Phase {  // what a 48 -> 16 k chunk that starts at a given time index produces
        uint32_t count;
        double new_last, idx0;
    };
    std::vector<Item> items;
    std::map<Key, Phase> phases;
    std::map<Key, std::vector<size_t>> groups;  // -> indices into items
    std::vector<double> idx, starts;
    for (size_t ci : ready) {
        RsCall &c = calls[ci];
        const StreamInfo &s = e->streams[c.id];
        const RatioTable &tab = e->ratio_tables[(size_t)s.rs_table];
        const bool fir = s.rs_in_hz == 48000 && s.rs_out_hz == 16000;
        const uint32_t n_chunks = s.rs_fill / kRsChunk;
        double last = s.rs_last_index;
        uint32_t col = c.produced;
        for (uint32_t k = 0; k < n_chunks; ++k) {
            Item it{};
            it.ci = ci, it.k = k, it.col = col, it.last = last, it.chunk_no = s.rs_chunks + k, it.table = s.rs_table, it.fir = fir;
            if (fir) {  // the integer-step FIR only cares where the chunk's first output sits relative to the chunk (three phases)
                const Key key{s.rs_table, last};
                auto ph = phases.find(key);
                if (ph == phases.end()) {
                    double new_last = 0.0;
                    chunk_indices(tab.ratio, last, kRsChunk, idx, &new_last);
                    ph = phases.emplace(key, Phase{(uint32_t)idx.size(), new_last, idx.empty() ? 0.0 : idx[0]}).first;
                }
                it.count = ph->second.count;
                it.new_last = ph->second.new_last;
                groups[key].push_back(items.size());
            } else {  // the generic kernel takes a time-index set per row: chunks of any age share one launch (sets filled in below)
                groups[Key{s.rs_table, 0.0}].push_back(items.size());
            }
            if (!fir) {
                // count and new_last come from the chunk's index set; the shared walk is extended here, pointers are taken later
                RatioTable &mut_tab = e->ratio_tables[(size_t)s.rs_table];
                const IndexSet &set = streaming_set(mut_tab, it.chunk_no);
                if (set.last_in == last) {
                    it.count = set.count, it.new_last = set.new_last;
                } else {  // a stream whose state does not sit on the shared walk
                    IndexSet own;
                    make_index_set(tab.ratio, last, kRsChunk, own);
                    it.count = own.count, it.new_last = own.new_last;
                }
            }
            if ((uint64_t)col + it.count > out_cap) return SK_ERR_INVALID_ARG;
            col += it.count;
            last = it.new_last;
            items.push_back(it);
        }
    }
    std::vector<uint32_t> row_map, out_off, row_set, set_count, g_map, g_off, g_set;
    for (auto &g : groups) {
        RatioTable &tab = e->ratio_tables[(size_t)g.first.table];
        const bool fir = tab.in_hz == 48000 && tab.out_hz == 16000;
        std::map<uint64_t, uint32_t> local_set;  // generic: chunk number -> set index in this launch
        std::vector<const IndexSet *> sets;
        std::vector<IndexSet> odd_sets;          // chunks whose state does not sit on the shared walk
        odd_sets.reserve(g.second.size());
        uint32_t max_count = 0;
        if (!fir) {  // extend the shared walk first: the loop below keeps pointers into it
            uint64_t deepest = 0;
            for (size_t ii : g.second) deepest = std::max(deepest, items[ii].chunk_no);
            (void)streaming_set(tab, deepest);
        }
        row_map.clear();
        out_off.clear();
        row_set.clear();
        for (size_t ii : g.second) {
            Item &it = items[ii];
            const RsCall &c = calls[it.ci];
            if (!fir) {
                const IndexSet *set = &streaming_set(tab, it.chunk_no);
                if (set->last_in != it.last) {
                    odd_sets.emplace_back();
                    make_index_set(tab.ratio, it.last, kRsChunk, odd_sets.back());
                    set = &odd_sets.back();
                    it.set_index = (uint32_t)sets.size();
                    sets.push_back(set);
                } else {
                    auto f = local_set.find(it.chunk_no);
                    if (f == local_set.end()) {
                        f = local_set.emplace(it.chunk_no, (uint32_t)sets.size()).first;
                        sets.push_back(set);
                    }
                    it.set_index = f->second;
                }
            }
            max_count = std::max(max_count, it.count);
            for (uint32_t ch = 0; ch < c.channels; ++ch) {
                const uint64_t off = (uint64_t)(c.row0 + ch) * out_stride + it.col;
                if (off > 0xffffffffull) return SK_ERR_INVALID_ARG;
                row_map.push_back((uint32_t)(rs_row0(e, c.id) + ch) * kRsBlocks + it.k);  // the chunk as a virtual row of one block's pitch
                out_off.push_back((uint32_t)off);
                row_set.push_back(it.set_index);
            }
        }
        if (!max_count) continue;
        const uint32_t *d_map = nullptr, *d_off = nullptr;
        uint32_t n_launch_rows = (uint32_t)row_map.size();
        if (fir) {
            SK_HIP(aux.put(row_map, e->stream, &d_map), "upload row map");
            SK_HIP(aux.put(out_off, e->stream, &d_off), "upload out offsets");
            // integer time base: output m sits at index 3m - 125.  Any origin works as long as output
            // out_first + j reads the row at chunk-relative index idx[0] + 3j (+ kRsBase + kRsHist of pad and history in front)
            // ... and the origin that makes the row's sample 0 fall on a multiple of four lets the kernel stage with
            // 16-byte loads (a function of the chunk's own phase only, so a stream's samples do not depend on
            // which launch it shares, nor on how many chunks of it the launch holds)
            const double idx0 = phases.at(g.first).idx0;
            const int64_t fixed = 125 + (int64_t)std::llround(idx0) + (int64_t)kRsHist;
            uint32_t first = 1024;
            while ((3 * (int64_t)first - fixed) & 3) ++first;
            sk::FirArgs a = fir_base(e);
            a.in = e->d_rs;
            a.in_stride = kRsChunk;
            a.rows = (uint32_t)row_map.size();
            a.in_frames = kRsBase + kRsWindow;
            a.in_origin = (int32_t)(3 * (int64_t)first - 125 - (int64_t)std::llround(idx0) - (int64_t)kRsHist - (int64_t)kRsBase);
            a.out = d_out;
            a.out_stride = 0;
            a.row_map = d_map;
            a.out_off = d_off;
            a.out_first = first;
            a.out_count = max_count;
            SK_HIP(sk::launch_fir_48k_16k(a, e->stream), "launch streaming fir");
        } else {
            uint32_t stride = 0;
            for (const IndexSet *set : sets) stride = std::max<uint32_t>(stride, (uint32_t)set->starts.size());
            starts.assign((size_t)stride * sets.size(), 0.0);
            set_count.clear();
            for (size_t i = 0; i < sets.size(); ++i) {
                std::copy(sets[i]->starts.begin(), sets[i]->starts.end(), starts.begin() + (ptrdiff_t)(i * stride));
                set_count.push_back(sets[i]->count);
            }
            // the generic kernel's workgroups take 64 consecutive rows that share their index set: rows ordered by set,
            // each set's rows padded to a multiple of that with rows that read and write nothing (row_map 0xffffffff)
            {
                const uint32_t per_block = sk::sinc_rows_per_block();
                std::vector<uint32_t> order(row_map.size());
                for (uint32_t r = 0; r < order.size(); ++r) order[r] = r;
                std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return row_set[x] < row_set[y]; });
                g_map.clear(), g_off.clear(), g_set.clear();  // function-level: they outlive the asynchronous uploads below
                for (size_t k = 0; k < order.size(); ++k) {
                    if (k > 0 && row_set[order[k]] != row_set[order[k - 1]])
                        while (g_map.size() % per_block) {
                            g_map.push_back(0xffffffffu);
                            g_off.push_back(0);
                            g_set.push_back(g_set.back());
                        }
                    g_map.push_back(row_map[order[k]]);
                    g_off.push_back(out_off[order[k]]);
                    g_set.push_back(row_set[order[k]]);
                }
                SK_HIP(aux.put(g_map, e->stream, &d_map), "upload row map (grouped by index set)");
                SK_HIP(aux.put(g_off, e->stream, &d_off), "upload out offsets (grouped by index set)");
                row_set.swap(g_set);
                n_launch_rows = (uint32_t)g_map.size();
            }
            const double *d_starts = nullptr;
            const uint32_t *d_count = nullptr, *d_set = nullptr;
            SK_HIP(aux.put(starts, e->stream, &d_starts), "upload time indices");
            SK_HIP(aux.put(set_count, e->stream, &d_count), "upload output counts");
            SK_HIP(aux.put(row_set, e->stream, &d_set), "upload row sets");
            sk::SincArgs a{};
            a.in = e->d_rs;
            a.in_stride = kRsChunk;
            a.out = d_out;
            a.out_stride = 0;
            a.sincs = tab.d_sincs;
            a.set_starts = d_starts;
            a.set_count = d_count;
            a.row_set = d_set;
            a.starts_stride = stride;
            a.step = 1.0 / tab.ratio;
            a.row_map = d_map;
            a.out_off = d_off;
            a.rows = n_launch_rows;
            a.in_frames = kRsBase + kRsWindow;
            a.out_count = max_count;
            a.in_origin = -(int32_t)(kRsHist + kRsBase);  // indices are relative to the chunk start; the virtual row starts kRsBase + 512 earlier
            a.n_sets = (uint32_t)sets.size();
            a.exact = e->sinc_exact;
            if (!a.exact) {
                const size_t want = sk::sinc_mfma_scratch_bytes(a.n_sets, max_count, a.step);
                if (want) {  // a failed allocation is an error, not another arithmetic (see sk_downsample_f32_dev)
                    SK_HIP(e->sinc_scratch.reserve(want), "alloc resampler tap fragments");
                    a.scratch = e->sinc_scratch.p, a.scratch_bytes = e->sinc_scratch.cap;
                }
            }
            const uint32_t rows_per_launch = 65535u * sk::sinc_rows_per_block();  // grid.y limit; a multiple of the block's rows
            for (uint32_t r0 = 0; r0 < a.rows; r0 += rows_per_launch) {
                sk::SincArgs part = a;
                part.rows = std::min<uint32_t>(rows_per_launch, a.rows - r0);
                part.row_map = d_map + r0;
                part.out_off = d_off + r0;
                part.row_set = d_set + r0;
                SK_HIP(sk::launch_sinc_resample(part, e->stream), "launch sinc resample");
            }
        }
    }
    // state, AudioData boundaries, and the slide: what is behind the processed chunks -- their last 512 samples (the next chunk's
    // history, rubato's copy_within) and the incomplete chunk -- moves to the front of the row.  Source and destination overlap
    // only when one chunk went and more than 3584 samples stay: such a row is moved in two launches, the second for the part whose
    // destination the first one's source covered.
    std::vector<sk::RowCopy> slides, tails;
    for (const Item &it : items) {
        RsCall &c = calls[it.ci];
        c.outs.emplace_back(it.col, it.count);
        c.produced = it.col + it.count;
    }
    for (size_t ci : ready) {
        RsCall &c = calls[ci];
        StreamInfo &s = e->streams[c.id];
        const uint32_t n_chunks = s.rs_fill / kRsChunk;
        if (!n_chunks) continue;
        const uint32_t rest = s.rs_fill - n_chunks * kRsChunk, len = kRsHist + rest, gap = n_chunks * kRsChunk;
        for (uint32_t ch = 0; ch < c.channels; ++ch) {
            const uint64_t row = (rs_row0(e, c.id) + ch) * kRsRow + kRsBase;
            slides.push_back(sk::RowCopy{row + gap, row, std::min(len, gap), 0});
            if (len > gap) tails.push_back(sk::RowCopy{row + 2ull * gap, row + gap, len - gap, 0});
        }
        s.rs_chunks += n_chunks;
        s.rs_fill = rest;
    }
    for (const Item &it : items) e->streams[calls[it.ci].id].rs_last_index = it.new_last;  // items of a stream are in chunk order: the last one wins
    for (std::vector<sk::RowCopy> *jobs : {&slides, &tails}) {
        if (jobs->empty()) continue;
        const sk::RowCopy *d_jobs = nullptr;
        SK_HIP(aux.put(*jobs, e->stream, &d_jobs), "upload slide jobs");
        for (size_t j0 = 0; j0 < jobs->size(); j0 += 65535)
            SK_HIP(sk::launch_row_copies(e->d_rs, e->d_rs, d_jobs + j0, (uint32_t)std::min<size_t>(65535, jobs->size() - j0), e->stream),
                   "slide resampler rows");
    }
    return SK_OK;
}

int rs_collect(sk_engine *e, const uint32_t *streams, uint32_t n_streams, std::vector<RsCall> &calls, size_t *total_rows) {
    calls.resize(n_streams);
    size_t rows = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        if (!stream_ok(e, streams[i]) || !e->streams[streams[i]].rs_open) return SK_ERR_BAD_STREAM;
        for (uint32_t k = 0; k < i; ++k)
            if (streams[k] == streams[i]) return SK_ERR_INVALID_ARG;  // a stream may appear once per call
        calls[i].id = streams[i];
        calls[i].channels = e->streams[streams[i]].channels;
        calls[i].row0 = rows;
        rows += calls[i].channels;
    }
    *total_rows = rows;
    return SK_OK;
}

}  // namespace

extern "C" {

int sk_resampler_process_f32(sk_engine *e, const uint32_t *streams, uint32_t n_streams, const float *in, uint32_t frames,
                             float *out, uint32_t out_cap, uint32_t *out_frames) try {
    sk::abi_enter();
    if (!e || (n_streams && (!streams || !out_frames)) || (frames && n_streams && !in)) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    std::vector<RsCall> calls;
    size_t total_rows = 0;
    int rc = rs_collect(e, streams, n_streams, calls, &total_rows);
    if (rc != SK_OK) return rc;
    if (total_rows == 0) return SK_OK;
    const size_t out_stride = ((size_t)out_cap + 3) & ~(size_t)3;
    SK_HIP(e->in_buf.reserve(total_rows * (size_t)frames * 4 + 16), "alloc staging");
    SK_HIP(e->out_buf.reserve(total_rows * out_stride * 4 + 16), "alloc staging");
    SK_HIP(e->aux2_buf.reserve(total_rows * 256 + (1 << 20)), "alloc round scratch");
    if (frames)
        SK_HIP(hipMemcpyAsync(e->in_buf.p, in, total_rows * (size_t)frames * 4, hipMemcpyHostToDevice, e->stream),
               "H2D resampler input");
    std::vector<sk::RowCopy> jobs;
    std::vector<size_t> ready;
    for (;;) {
        AuxArena aux{(uint8_t *)e->aux2_buf.p, e->aux2_buf.cap, 0};
        jobs.clear();
        ready.clear();
        for (size_t ci = 0; ci < calls.size(); ++ci) {
            RsCall &c = calls[ci];
            StreamInfo &s = e->streams[c.id];
            const uint32_t take = std::min(frames - c.consumed, kRsMaxFill - s.rs_fill);  // up to five chunks per round
            if (take) {
                for (uint32_t ch = 0; ch < c.channels; ++ch)
                    jobs.push_back(sk::RowCopy{(uint64_t)(c.row0 + ch) * frames + c.consumed,
                                               (rs_row0(e, c.id) + ch) * kRsRow + kRsBase + kRsHist + s.rs_fill, take, 0});
                s.rs_fill += take;
                c.consumed += take;
            }
            if (s.rs_fill >= kRsChunk) ready.push_back(ci);
        }
        if (jobs.empty() && ready.empty()) break;
        if (!jobs.empty()) {
            const sk::RowCopy *d_jobs = nullptr;
            SK_HIP(aux.put(jobs, e->stream, &d_jobs), "upload append jobs");
            for (size_t j0 = 0; j0 < jobs.size(); j0 += 65535)
                SK_HIP(sk::launch_row_copies((const float *)e->in_buf.p, e->d_rs, d_jobs + j0,
                                             (uint32_t)std::min<size_t>(65535, jobs.size() - j0), e->stream), "append chunk");
        }
        if (!ready.empty()) {
            rc = rs_process_ready(e, calls, ready, (float *)e->out_buf.p, out_stride, out_cap, aux);
            if (rc != SK_OK) return rc;
        }
        SK_HIP(hipStreamSynchronize(e->stream), "resampler round sync");  // the round's host arrays may now be reused
    }
    size_t max_prod = 0;
    for (size_t ci = 0; ci < calls.size(); ++ci) {
        out_frames[ci] = calls[ci].produced;
        max_prod = std::max<size_t>(max_prod, calls[ci].produced);
    }
    if (max_prod)
        SK_HIP(hipMemcpy2DAsync(out, (size_t)out_cap * 4, e->out_buf.p, out_stride * 4, max_prod * 4, total_rows,
                                hipMemcpyDeviceToHost, e->stream), "D2H resampler output");
    SK_HIP(hipStreamSynchronize(e->stream), "resampler sync");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_resampler_process_f32");
}

int sk_resampler_flush_f32(sk_engine *e, const uint32_t *streams, uint32_t n_streams, float *out, uint32_t out_cap,
                           uint32_t *out_frames) try {
    sk::abi_enter();
    if (!e || (n_streams && (!streams || !out_frames || !out))) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e, ComputeTurn{});
    std::vector<RsCall> calls;
    size_t total_rows = 0;
    int rc = rs_collect(e, streams, n_streams, calls, &total_rows);
    if (rc != SK_OK) return rc;
    if (total_rows == 0) return SK_OK;
    const size_t out_stride = ((size_t)out_cap + 3) & ~(size_t)3;
    SK_HIP(e->out_buf.reserve(total_rows * out_stride * 4 + 16), "alloc staging");
    SK_HIP(e->aux2_buf.reserve(total_rows * 256 + (1 << 20)), "alloc round scratch");
    AuxArena aux{(uint8_t *)e->aux2_buf.p, e->aux2_buf.cap, 0};
    // process_partial: the chunk is zero-padded to 4096 (lib.rs:2020-2031, 2048-2052)
    std::vector<sk::RowCopy> pads;
    std::vector<size_t> ready;
    for (size_t ci = 0; ci < calls.size(); ++ci) {
        RsCall &c = calls[ci];
        StreamInfo &s = e->streams[c.id];
        const uint32_t remaining = s.rs_fill, padded = kRsChunk - remaining;
        if (remaining > 0 && padded > 0)  // lib.rs:2032-2039
            c.trim = (uint32_t)std::llround(((double)padded * (double)s.rs_out_hz) / (double)s.rs_in_hz);
        for (uint32_t ch = 0; ch < c.channels && padded; ++ch)
            for (uint32_t o = 0; o < padded; o += 8192)
                pads.push_back(sk::RowCopy{0, (rs_row0(e, c.id) + ch) * kRsRow + kRsBase + kRsHist + remaining + o,
                                           std::min<uint32_t>(8192, padded - o), 0});
        s.rs_fill = kRsChunk;
        ready.push_back(ci);
    }
    if (!pads.empty()) {
        const sk::RowCopy *d_pads = nullptr;
        SK_HIP(aux.put(pads, e->stream, &d_pads), "upload pad jobs");
        for (size_t j0 = 0; j0 < pads.size(); j0 += 65535)
            SK_HIP(sk::launch_row_copies(e->d_zeros, e->d_rs, d_pads + j0, (uint32_t)std::min<size_t>(65535, pads.size() - j0),
                                         e->stream), "pad chunk");
    }
    rc = rs_process_ready(e, calls, ready, (float *)e->out_buf.p, out_stride, out_cap, aux);
    if (rc != SK_OK) return rc;
    size_t max_prod = 0;
    for (size_t ci = 0; ci < calls.size(); ++ci) {
        const uint32_t got = calls[ci].produced > calls[ci].trim ? calls[ci].produced - calls[ci].trim : 0;
        out_frames[ci] = got;
        max_prod = std::max<size_t>(max_prod, got);
    }
    if (max_prod)
        SK_HIP(hipMemcpy2DAsync(out, (size_t)out_cap * 4, e->out_buf.p, out_stride * 4, max_prod * 4, total_rows,
                                hipMemcpyDeviceToHost, e->stream), "D2H flush output");
    SK_HIP(hipStreamSynchronize(e->stream), "flush sync");
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_resampler_flush_f32");
}

}  // extern "C"

// ---- one scheduler tick on the device -----------------------------------------------------------------
// decode_aac_access_unit (soundkit-decoder lib.rs:1793-1813) followed by apply_output_options
// (lib.rs:3324-3456) for every access unit of every stream in the batch, with the AudioData boundaries the
// worker would have pushed to its output channel (lib.rs:3238-3259).

namespace {

struct TickCall {           // one sk_tick_stream
    uint32_t ch = 0;        // source channels
    uint32_t first = 0;     // index of its first desc
    uint32_t good = 0;      // frames before the first rejected one (all of them if none is rejected)
    int32_t bad_status = 0; // status of that rejected frame
    int rs_call = -1;       // index into the RsCall vector when the stream resamples
    std::vector<std::pair<uint32_t, uint32_t>> chunks;  // (column, frames) of each resampled AudioData
    bool mp3 = false;       // SK_TICK_MP3: `first` indexes the tick's granules, a unit is a granule
    uint32_t ulen = 1024;   // PCM frames per unit: 1024 (AAC access unit) or 576 (MP3 granule); a unit's channel rows are 1024 floats apart
};

struct TickMp3Frames {  // sk_tick_run_mixed_md: the granules' integers and scale factors are still Huffman codes -- the frames that
                        // survived the first pass (tick_impl_md), whose main data is on the device already (e->mp3e_in)
    const sk_mp3_frame_item *frames = nullptr;
    uint32_t n = 0;
    size_t main_len = 0;
    const uint32_t *first_row = nullptr, *first_record = nullptr;  // per frame: its first 576-line row / granule among the tick's
};
struct TickMp3 {  // the MP3 part of sk_tick_input
    const sk_mp3_requant_granule *granules = nullptr;
    const sk_mp3_granule_desc *descs = nullptr;
    const int16_t *is = nullptr;
    uint32_t n = 0;
    const TickMp3Frames *md = nullptr;  // instead of `is` (and of the granules' scale factors and preflag)
    // Layer I / II streams (SK_TICK_MPA): the LAST n_mpa_units entries of granules / descs are their units (channels and stream filled
    // in, nothing else), in the order of the streams; `mpa` says which frame each belongs to
    uint32_t n_mpa_units = 0;
    const struct TickMpa *mpa = nullptr;
};
struct TickMpa {
    std::vector<sk_mpa_frame_record> records;  // checked (record_adds_up, inside the byte buffer)
    std::vector<uint32_t> stream;              // per frame: its engine stream
    std::vector<uint32_t> first_unit;          // per frame: its first unit among the n_mpa_units
    std::vector<uint16_t> unit_len;            // per unit: 576 or 384
    const uint8_t *bytes = nullptr;
    size_t bytes_len = 0;
};

}  // namespace

namespace {

// What a tick can hand back at most.  A resampling stream emits one AudioData per completed 4096-frame chunk (+ one carried chunk + the
// flush); everything else one per unit (1024 PCM frames at most).  With the engine at hand the frames of a chunk follow from the
// stream's own ratio; without it they are taken for the largest ratio there is (8 kHz -> 48 kHz).  (The tick lays its output out before
// it launches anything and refuses a buffer that is too small: the bound only has to be one.)
size_t tick_out_bound(const sk_engine *e, const sk_tick_stream *ts, uint32_t n_streams, uint32_t *max_outputs) {
    size_t bytes = 0;
    uint64_t outs = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        const uint64_t n = ts[i].codec == SK_TICK_MPA ? 2ull * ts[i].n_frames : ts[i].n_frames;  // a Layer II frame is two units
        const uint64_t width = (ts[i].out_bits == 16 || ts[i].out_bits == 24 || ts[i].out_bits == 32) ? ts[i].out_bits / 8u : 4u;
        const uint64_t frame_bytes = width * ((ts[i].out_channels == 1 || ts[i].out_channels == 2) ? ts[i].out_channels : 2u);
        if (ts[i].resample) {
            uint64_t chunk_frames = 4096 * 6 + 2;
            if (e && ts[i].stream < e->streams.size()) {
                const StreamInfo &s = e->streams[ts[i].stream];
                if (s.open && s.rs_open && s.rs_in_hz) chunk_frames = (uint64_t)(4096.0 * (double)s.rs_out_hz / (double)s.rs_in_hz) + 8;
            }
            const uint64_t chunks = n / 4 + 2;
            bytes += chunks * (chunk_frames * frame_bytes + 16) + 16;
            outs += chunks + 1;
        } else {
            bytes += n * (1024 * frame_bytes + 16) + 16;
            outs += n + 1;
        }
    }
    if (max_outputs) *max_outputs = (uint32_t)std::min<uint64_t>(outs, 0xffffffffu);
    return bytes;
}

}  // namespace

extern "C" {

size_t sk_tick_out_bound(const sk_tick_stream *ts, uint32_t n_streams, uint32_t *max_outputs) try {
    sk::abi_enter();
    if (!ts && n_streams) return 0;
    return tick_out_bound(nullptr, ts, n_streams, max_outputs);
} catch (...) {
    (void)sk::abi_caught("sk_tick_out_bound");
    return 0;
}

size_t sk_tick_out_bound_on(sk_engine *e, const sk_tick_stream *ts, uint32_t n_streams, uint32_t *max_outputs) try {
    sk::abi_enter();
    if (!e || (!ts && n_streams)) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return tick_out_bound(e, ts, n_streams, max_outputs);
} catch (...) {
    (void)sk::abi_caught("sk_tick_out_bound_on");
    return 0;
}

}  // extern "C"

namespace {

// the front-end's tables, flattened and uploaded once
int ensure_entropy_tables(sk_engine *e) {
    static_assert(sk_ec::kHostPow43Len == sk_ec::kPow43Len, "host table and device bound must agree");
    if (e->ec_ready) return SK_OK;
    const sk_ec::HostTables &h = sk_ec::host_tables();
    auto pad = [](size_t n) { return (n + 255) & ~(size_t)255; };
    for (int b = 0; b < 12; ++b)
        if (h.primary_bits[b] != sk_ec::kPrimaryBits) return SK_ERR_INVALID_ARG;
    // LDS part first (index block, Huffman tables, tuples, scale-factor multipliers, band offsets), then what stays in
    // global memory
    const size_t b_meta = 0, b_lut = b_meta + pad(h.meta.size() * 4), b_tup = b_lut + pad(h.lut.size() * 4),
                 b_sf = b_tup + pad(h.tuples.size() * 8), b_swb = b_sf + pad(h.sf_mult.size() * 4),
                 b_plo = b_swb + pad(h.swb.size() * 2), lds_end = b_plo + pad(sk_ec::kPow43Lo * 4), b_pow = lds_end, b_is = b_pow + pad(h.pow43.size() * 4),
                 b_tns = b_is + pad(h.is_mult.size() * 4), b_sfw = b_tns + pad(h.tns_sin.size() * 4), b_isw = b_sfw + pad(h.sf_wide.size() * 4),
                 total = b_isw + pad(h.is_wide.size() * 4);
    std::vector<uint8_t> blob(total, 0);
    std::memcpy(blob.data() + b_meta, h.meta.data(), h.meta.size() * 4);
    std::memcpy(blob.data() + b_lut, h.lut.data(), h.lut.size() * 4);
    std::memcpy(blob.data() + b_tup, h.tuples.data(), h.tuples.size() * 8);
    std::memcpy(blob.data() + b_pow, h.pow43.data(), h.pow43.size() * 4);
    std::memcpy(blob.data() + b_plo, h.pow43.data(), sk_ec::kPow43Lo * 4);
    std::memcpy(blob.data() + b_sf, h.sf_mult.data(), h.sf_mult.size() * 4);
    std::memcpy(blob.data() + b_is, h.is_mult.data(), h.is_mult.size() * 4);
    std::memcpy(blob.data() + b_tns, h.tns_sin.data(), h.tns_sin.size() * 4);
    std::memcpy(blob.data() + b_swb, h.swb.data(), h.swb.size() * 2);
    std::memcpy(blob.data() + b_sfw, h.sf_wide.data(), h.sf_wide.size() * 4);
    std::memcpy(blob.data() + b_isw, h.is_wide.data(), h.is_wide.size() * 4);
    SK_HIP(hipMalloc(&e->d_ec_blob, total), "alloc entropy tables");
    SK_HIP(hipMemcpy(e->d_ec_blob, blob.data(), total, hipMemcpyHostToDevice), "upload entropy tables");
    const uint8_t *base = (const uint8_t *)e->d_ec_blob;
    sk_ec::Tables &t = e->ec_tables;
    t.meta = (const uint32_t *)(base + b_meta);
    t.lut = (const uint32_t *)(base + b_lut);
    t.tuples = (const uint64_t *)(base + b_tup);
    t.swb = (const uint16_t *)(base + b_swb);
    t.pow43 = (const float *)(base + b_pow);
    t.pow43_lo = (const float *)(base + b_plo);
    t.sf_mult = (const float *)(base + b_sf);
    t.is_mult = (const float *)(base + b_is);
    t.tns_sin = (const float *)(base + b_tns);
    t.sf_wide = (const float *)(base + b_sfw);
    t.is_wide = (const float *)(base + b_isw);
    sk::EntropyArgs &ea = e->ec_args;
    ea.t = t;
    ea.lds_blob = base;
    ea.lds_bytes = (uint32_t)lds_end;
    ea.lds_meta_off = (uint32_t)b_meta;
    ea.lds_lut_off = (uint32_t)b_lut;
    ea.lds_tuple_off = (uint32_t)b_tup;
    ea.lds_sf_off = (uint32_t)b_sf;
    ea.lds_swb_off = (uint32_t)b_swb;
    ea.lds_pow_off = (uint32_t)b_plo;
    e->ec_ready = true;
    return SK_OK;
}

int sf_index_of(uint32_t rate) {
    static const uint32_t rates[13] = {96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 7350};
    for (int i = 0; i < 13; ++i)
        if (rates[i] == rate) return i;
    return -1;
}

// Both tick entry points.  units == nullptr: the spectra come from the host (descs / coeffs).  Otherwise the access
// units themselves do, and the front-end runs on the device before the synthesis.
constexpr uint32_t kMaxAccessUnitBytes = 8192;

// The tick's waits for the device.  hipStreamSynchronize has no bound: a launch that never finishes (or a completion the
// runtime never sees) would park the scheduler's submission thread for good with nothing on record.  Polling the stream
// turns that into SK_ERR_TIMEOUT with the stage in sk_engine_last_hip_error; the poll interval (tens of microseconds) is
// noise against a tick of milliseconds.
int wait_stream(sk_engine *e, const char *what) {
    e->where.store(what);
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    for (;;) {
        const hipError_t q = hipStreamQuery(e->stream);
        if (q == hipSuccess) return SK_OK;
        if (q != hipErrorNotReady) return e->hip_fail(q, what);
        if (++spins < 64) {
            std::this_thread::yield();
            continue;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(20));
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > e->sync_timeout_s) {
            e->last_hip_error = std::string(what) + ": the device did not finish within the engine's wait bound";
            return SK_ERR_TIMEOUT;
        }
    }
}

struct TickWhere {  // marks the engine as inside a tick for sk_engine_where; "idle" again on every exit
    sk_engine *e;
    explicit TickWhere(sk_engine *eng) : e(eng) { e->where.store("tick: host planning"); }
    ~TickWhere() { e->where.store("idle"); }
};

struct EntropyProbe {  // sk_aac_entropy_decode: stop after the front-end and hand its results to the caller
    float *spectra;
    sk_aac_frame_desc *descs;
    int32_t *status;
};

// The MP3 granules of a tick (e->mu held, device selected): requantisation + joint stereo + reorder, then the hybrid synthesis,
// queued on e->stream with no synchronisation.  Channel row r of the granules (their channels in array order) lands at
// pcm_rows + r * 1024 (576 samples), each sample as f32_to_i16(x) / 32768 -- Mp3Decoder's i16 AudioData as the f32
// audio_data_to_f32_channels makes of it.  status[g]: 0, or why granule g cannot be decoded (its stream ends there).
int tick_mp3_queue(sk_engine *e, const TickMp3 &mp3, float *pcm_rows, AuxArena &aux, std::vector<int32_t> &status) {
    int rc = ensure_mp3(e);
    if (rc == SK_OK) rc = ensure_mp3_requant(e);
    if (rc != SK_OK) return rc;
    if (!e->mp3_window_set) return SK_ERR_UNSUPPORTED;  // no Table B.3 on this engine: sk_mp3_decoder_create / sk_mp3_set_synthesis_window first
    const uint32_t n = mp3.n - mp3.n_mpa_units;  // the Layer I / II units behind them are tick_mpa_queue's
    status.assign(mp3.n, 0);
    std::vector<sk::Mp3RequantRecord> records(n);
    std::vector<uint32_t> touched;
    uint64_t off = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const sk_mp3_requant_granule &g = mp3.granules[i];
        const sk_mp3_granule_desc &d = mp3.descs[i];
        sk::Mp3RequantRecord &r = records[i];
        std::memset(&r, 0, sizeof r);
        r.off = (uint32_t)off;
        r.channels = g.channels;
        off += g.channels;
        const int slot = mp3_rate_slot(g.sample_rate);
        const bool joint = g.channels == 2 && (g.ms_stereo || g.intensity_stereo);
        int32_t st = SK_OK;
        if (slot < 0 || !e->mp3_bands_set[slot]) st = SK_MP3_UNSUPPORTED;
        for (uint32_t c = 0; c < g.channels && st == SK_OK; ++c) {
            const sk_mp3_requant_channel &ch = g.ch[c];
            if (ch.block_type > 3 || ch.mixed_block_flag > 1 || ch.scalefac_scale > 1 || ch.preflag > 1 || (ch.mixed_block_flag && ch.block_type != 2) ||
                d.block_type[c] != ch.block_type || d.mixed_block_flag[c] != ch.mixed_block_flag)
                st = SK_MP3_INVALID;
            else if (ch.mixed_block_flag && e->mp3_bands[slot][37] == 0xffff) st = SK_MP3_UNSUPPORTED;
        }
        if (st == SK_OK && joint) {
            if ((g.ch[0].block_type == 2) != (g.ch[1].block_type == 2) || g.ch[0].mixed_block_flag != g.ch[1].mixed_block_flag) st = SK_MP3_INVALID;
        }
        status[i] = st;
        r.slot = st == SK_OK ? (uint8_t)slot : 0xff;
        r.flags = joint ? (uint8_t)((g.ms_stereo ? 1 : 0) | (g.intensity_stereo ? 2 : 0) | (g.lsf ? 4 : 0) | ((g.intensity_stereo & 2) ? 8 : 0)) : 0;
        r.ch[0] = g.ch[0];
        if (g.channels == 2) r.ch[1] = g.ch[1];
        if (st == SK_OK)
            for (uint32_t c = 0; c < d.channels; ++c)
                if (e->state_count[d.stream * 2 + c]++ == 0) touched.push_back(d.stream * 2 + c);
    }
    std::vector<sk::SynthTask> tasks(touched.size());
    uint32_t n_entries = 0;
    for (size_t t = 0; t < touched.size(); ++t) {
        tasks[t] = sk::SynthTask{touched[t], n_entries, 0, 0};
        n_entries += e->state_count[touched[t]];
        e->state_task[touched[t]] = (uint32_t)t;
    }
    std::vector<sk::SynthEntry> entries(n_entries);
    for (uint32_t i = 0; i < n; ++i) {
        const sk_mp3_granule_desc &d = mp3.descs[i];
        if (status[i] != SK_OK) continue;
        for (uint32_t c = 0; c < d.channels; ++c) {
            sk::SynthTask &t = tasks[e->state_task[d.stream * 2 + c]];
            entries[t.begin + t.count++] = sk::SynthEntry{records[i].off + c, (uint32_t)d.block_type[c] | ((uint32_t)d.mixed_block_flag[c] << 2) |
                                                                                   ((uint32_t)(d.channels - 1) << 3) | (c << 4)};
        }
    }
    for (uint32_t state : touched) e->state_count[state] = 0;
    const size_t lines = (size_t)off * 576;
    SK_HIP(e->tick_mp3_in.reserve(lines * sizeof(int16_t) + 16), "alloc tick mp3 quantised lines");
    SK_HIP(e->tick_mp3_xr.reserve(lines * sizeof(float) + 16), "alloc tick mp3 lines");
    sk::Mp3RequantArgs q{};
    SK_HIP(aux.put(records, e->stream, &q.records), "upload tick mp3 granule records");
    if (mp3.md) {  // the Huffman stage writes the integers where the host's would have been copied to, and the scale factors into the records
        Mp3EntropyOut eo;
        rc = mp3_entropy_launch(e, mp3.md->frames, mp3.md->n, nullptr, mp3.md->main_len, (int16_t *)e->tick_mp3_in.p, mp3.md->first_row,
                                const_cast<sk::Mp3RequantRecord *>(q.records), mp3.md->first_record, &eo);
        if (rc != SK_OK) return rc;
    } else {
        SK_HIP(hipMemcpyAsync(e->tick_mp3_in.p, mp3.is, lines * sizeof(int16_t), hipMemcpyHostToDevice, e->stream), "H2D tick mp3 quantised lines");
    }
    q.is = (const int16_t *)e->tick_mp3_in.p;
    q.xr = (float *)e->tick_mp3_xr.p;
    q.n = n;
    q.pow43 = (const float *)e->d_mp3_rq;
    q.root4 = q.pow43 + sk::kMp3Pow43;
    q.is_k = q.root4 + 4;
    q.bands = (const uint16_t *)(e->d_mp3_rq + kRqBandsAt);
    q.pretab = e->d_mp3_rq + kRqPretabAt;
    q.line_map = (const uint32_t *)(e->d_mp3_rq + kRqMapAt);
    SK_HIP(sk::launch_mp3_requant(q, e->stream), "launch tick mp3 requantisation");
    if (tasks.empty()) return SK_OK;
    sk::Mp3Args a{};
    a.xr = (const float *)e->tick_mp3_xr.p;
    a.pcm = pcm_rows;
    a.planar_stride = 1024;
    a.state = e->d_mp3_state;
    SK_HIP(aux.put(tasks, e->stream, &a.tasks), "upload tick mp3 tasks");
    SK_HIP(aux.put(entries, e->stream, &a.entries), "upload tick mp3 entries");
    a.n_tasks = (uint32_t)tasks.size();
    a.imdct = e->d_mp3_tables;
    a.matrix = a.imdct + kMp3Imdct;
    a.window = a.matrix + kMp3Matrix;
    a.cs_ca = a.window + kMp3Window;
    SK_HIP(sk::launch_mp3_hybrid(a, e->stream), "launch tick mp3 hybrid synthesis");
    return SK_OK;
}

// The Layer I / II frames of a tick (e->mu held, device selected): one k_mp12_synth launch in its planar form, queued on e->stream with
// no synchronisation.  Their units' channel rows follow the Layer III granules' rows in pcm_rows, in unit order.
int tick_mpa_queue(sk_engine *e, const TickMp3 &mp3, float *pcm_rows, AuxArena &aux) {
    int rc = ensure_mp3(e);
    if (rc != SK_OK) return rc;
    if (!e->mp3_window_set) return SK_ERR_UNSUPPORTED;  // no Table B.3 on this engine
    const TickMpa &m = *mp3.mpa;
    const uint32_t n_l3 = mp3.n - mp3.n_mpa_units, n = (uint32_t)m.records.size();
    uint64_t l3_rows = 0;
    for (uint32_t g = 0; g < n_l3; ++g) l3_rows += mp3.granules[g].channels;
    std::vector<uint64_t> unit_row(mp3.n_mpa_units + 1, l3_rows);
    for (uint32_t u = 0; u < mp3.n_mpa_units; ++u) unit_row[u + 1] = unit_row[u] + mp3.granules[n_l3 + u].channels;
    std::vector<uint32_t> touched;
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t c = 0; c < m.records[i].channels; ++c)
            if (e->state_count[m.stream[i] * 2 + c]++ == 0) touched.push_back(m.stream[i] * 2 + c);
    std::vector<sk::SynthTask> tasks(touched.size());
    uint32_t n_entries = 0;
    for (size_t t = 0; t < touched.size(); ++t) {
        tasks[t] = sk::SynthTask{touched[t], n_entries, 0, 0};
        n_entries += e->state_count[touched[t]];
        e->state_task[touched[t]] = (uint32_t)t;
    }
    std::vector<sk::Mp12Entry> entries(n_entries);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t c = 0; c < m.records[i].channels; ++c) {
            sk::SynthTask &t = tasks[e->state_task[m.stream[i] * 2 + c]];
            entries[t.begin + t.count++] = sk::Mp12Entry{i, (uint32_t)unit_row[m.first_unit[i]]};
        }
    for (uint32_t state : touched) e->state_count[state] = 0;
    if (tasks.empty()) return SK_OK;
    SK_HIP(e->tick_mpa_in.reserve(m.bytes_len + 16), "alloc tick mpa frame bytes");
    SK_HIP(hipMemcpyAsync(e->tick_mpa_in.p, m.bytes, m.bytes_len, hipMemcpyHostToDevice, e->stream), "H2D tick mpa frame bytes");
    sk::Mp12Args a{};
    SK_HIP(aux.put(m.records, e->stream, &a.records), "upload tick mpa records");
    SK_HIP(aux.put(tasks, e->stream, &a.tasks), "upload tick mpa tasks");
    SK_HIP(aux.put(entries, e->stream, &a.entries), "upload tick mpa entries");
    a.bytes = (const uint32_t *)e->tick_mpa_in.p;
    a.pcm = pcm_rows;
    a.planar_stride = 1024;
    a.state = e->d_mp3_state;
    a.n_tasks = (uint32_t)tasks.size();
    a.matrix = e->d_mp3_tables + kMp3Imdct;
    a.window = a.matrix + kMp3Matrix;
    a.scf = a.window + kMp3Window + 16;
    SK_HIP(sk::launch_mp12_synth(a, e->stream), "launch tick mpa synthesis");
    return SK_OK;
}

// Queues the copy of a tick's packed output to the caller's buffer.  Into pinned memory the copy is queued like a kernel and the
// bounded wait that follows is the tick's only wait.  A caller's pageable buffer would make hipMemcpyAsync itself wait for everything
// queued so far, unbounded: such a buffer (the scheduler's are pinned; a test's numpy array is not) gets the bytes through the
// engine's pinned bounce buffer: *bounce is then where they arrive, to be copied to `out` after the wait.
int tick_queue_d2h(sk_engine *e, uint8_t *out, const uint8_t *d_out, size_t bytes, uint8_t **bounce) {
    *bounce = nullptr;
    hipPointerAttribute_t pa{};
    const bool pinned = hipPointerGetAttributes(&pa, out) == hipSuccess && pa.type == hipMemoryTypeHost;
    if (!pinned) (void)hipGetLastError();
    if (!pinned) {
        if (e->h_out_cap < bytes) {
            if (e->h_out) (void)hipHostFree(e->h_out);
            e->h_out = nullptr;
            e->h_out_cap = 0;
            SK_HIP(hipHostMalloc((void **)&e->h_out, bytes + bytes / 4 + 4096, hipHostMallocDefault), "alloc pinned output bounce");
            e->h_out_cap = bytes + bytes / 4 + 4096;
        }
        *bounce = e->h_out;
    }
    SK_HIP(hipMemcpyAsync(*bounce ? *bounce : out, d_out, bytes, hipMemcpyDeviceToHost, e->stream), "D2H tick output");
    return SK_OK;
}

// The resampler rounds of a tick, shared by tick_body (decoded units: row copies) and tick_pcm_body (PCM units: k_pcm_ingest).  A row
// holds kRsMaxFill samples behind its history, so a stream's input of a tick goes down in rounds: queue what fits, one launch for all
// streams, rs_process_ready, again.  Then the flush of the streams that end (StreamingResampler::flush, lib.rs:2017-2058).
struct RsRounds {
    std::function<uint32_t(size_t ci)> total_in;  // input frames call ci's stream brings in this tick
    // queue the frames [calls[ci].consumed, + take) of call ci for rows that hold `fill` frames; returns how many it queued
    // (1 ... take: a source may prefer to cut elsewhere)
    std::function<uint32_t(size_t ci, uint32_t take, uint32_t fill)> append;
    std::function<int()> launch;  // upload and launch what append has queued since the last launch (SK_OK when nothing was)
    std::function<bool(size_t ci)> flush;  // the stream of call ci ends with this tick
    std::function<std::vector<std::pair<uint32_t, uint32_t>> &(size_t ci)> chunks;  // where call ci's AudioData boundaries go
    std::function<void(int)> sub;  // section timer (SK_TICK_TRACE)
};

int rs_run_rounds(sk_engine *e, std::vector<RsCall> &calls, float *d_res, size_t res_stride, uint32_t res_cap, AuxArena &aux, const RsRounds &h) {
    std::vector<size_t> ready;
    std::vector<uint32_t> before;
    int rc = SK_OK;
    for (;;) {
        ready.clear();
        bool queued = false;
        for (size_t ci = 0; ci < calls.size(); ++ci) {
            RsCall &c = calls[ci];
            StreamInfo &s = e->streams[c.id];
            const uint32_t take = std::min(h.total_in(ci) - c.consumed, kRsMaxFill - s.rs_fill);  // a tick's units of a stream: one round
            if (take) {
                const uint32_t got = h.append(ci, take, s.rs_fill);
                if (got == 0 || got > take) return SK_ERR_INTERNAL;
                s.rs_fill += got;
                c.consumed += got;
                queued = true;
            }
            if (s.rs_fill >= kRsChunk) ready.push_back(ci);
        }
        h.sub(0);
        if (!queued && ready.empty()) break;
        rc = h.launch();
        if (rc != SK_OK) return rc;
        h.sub(1);
        if (!ready.empty()) {
            rc = rs_process_ready(e, calls, ready, d_res, res_stride, res_cap, aux);
            if (rc != SK_OK) return rc;
            h.sub(2);
            for (size_t ci : ready) {  // one AudioData per chunk (lib.rs:1979-2003), empty ones are not sent
                RsCall &c = calls[ci];
                for (const auto &o : c.outs)
                    if (o.second) h.chunks(ci).emplace_back(o.first, o.second);
                c.outs.clear();
            }
        }
    }
    // end of stream: StreamingResampler::flush (lib.rs:2017-2058); a stream that failed is not flushed
    std::vector<sk::RowCopy> pads;
    ready.clear();
    for (size_t ci = 0; ci < calls.size(); ++ci) {
        if (!h.flush(ci)) continue;
        RsCall &c = calls[ci];
        StreamInfo &s = e->streams[c.id];
        const uint32_t remaining = s.rs_fill, padded = kRsChunk - remaining;
        c.trim = 0;
        if (remaining > 0 && padded > 0)
            c.trim = (uint32_t)std::llround(((double)padded * (double)s.rs_out_hz) / (double)s.rs_in_hz);
        for (uint32_t ch = 0; ch < c.channels && padded; ++ch)
            for (uint32_t o = 0; o < padded; o += 8192)
                pads.push_back(sk::RowCopy{0, (rs_row0(e, c.id) + ch) * kRsRow + kRsBase + kRsHist + remaining + o,
                                           std::min<uint32_t>(8192, padded - o), 0});
        s.rs_fill = kRsChunk;
        ready.push_back(ci);
    }
    if (!ready.empty()) {
        if (!pads.empty()) {
            const sk::RowCopy *d_pads = nullptr;
            SK_HIP(aux.put(pads, e->stream, &d_pads), "upload tick pad jobs");
            for (size_t j0 = 0; j0 < pads.size(); j0 += 65535)
                SK_HIP(sk::launch_row_copies(e->d_zeros, e->d_rs, d_pads + j0,
                                             (uint32_t)std::min<size_t>(65535, pads.size() - j0), e->stream), "tick pad chunk");
        }
        before.clear();
        for (size_t ci : ready) before.push_back(calls[ci].produced);
        rc = rs_process_ready(e, calls, ready, d_res, res_stride, res_cap, aux);
        if (rc != SK_OK) return rc;
        for (size_t k = 0; k < ready.size(); ++k) {
            const RsCall &c = calls[ready[k]];
            const uint32_t got = c.produced - before[k];
            if (got > c.trim) h.chunks(ready[k]).emplace_back(before[k], got - c.trim);
        }
    }
    return SK_OK;
}

int tick_body(sk_engine *e, const sk_tick_stream *ts, uint32_t n_streams, const sk_aac_frame_desc *descs, const float *coeffs,
              const sk_au_item *units, const uint8_t *au_bytes, size_t au_len, uint32_t n_frames, uint8_t *out, size_t out_cap,
              sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes, const EntropyProbe *probe,
              const uint8_t *q_sides, const int16_t *q_quant, const TickMp3 &mp3) {
    const bool au_mode = units != nullptr;
    const bool q_mode = q_sides != nullptr;  // quantised hand-over: descs from the host, spectra rebuilt on the device
    std::vector<sk_aac_frame_desc> au_descs;
    if (!e || !n_outs || (n_streams && !ts)) return SK_ERR_INVALID_ARG;
    if (!au_mode && !q_mode && n_frames && (!descs || !coeffs)) return SK_ERR_INVALID_ARG;
    if (q_mode && n_frames && (!descs || !q_quant)) return SK_ERR_INVALID_ARG;
    if (au_mode && n_frames && !au_bytes) return SK_ERR_INVALID_ARG;
    if (mp3.n_mpa_units > mp3.n || (mp3.n_mpa_units && !mp3.mpa)) return SK_ERR_INVALID_ARG;
    const uint32_t n_l3 = mp3.n - mp3.n_mpa_units;  // the Layer III granules come first, the Layer I / II units behind them
    if (mp3.n && (!mp3.granules || !mp3.descs)) return SK_ERR_INVALID_ARG;
    if (n_l3 && !mp3.is && !mp3.md) return SK_ERR_INVALID_ARG;
    *n_outs = 0;
    if (out_bytes) *out_bytes = 0;
    if (n_streams == 0) return n_frames == 0 && mp3.n == 0 ? SK_OK : SK_ERR_INVALID_ARG;
    DeviceGuard guard(e);
    if (au_mode) {  // the descs are implied: every unit of a stream carries that stream's channel count
        uint64_t total = 0;
        for (uint32_t i = 0; i < n_streams; ++i) total += ts[i].codec != SK_TICK_AAC ? 0 : ts[i].n_frames;
        if (total != n_frames) return SK_ERR_INVALID_ARG;
        if (au_len > 0xffffffffull) return SK_ERR_INVALID_ARG;  // unit offsets and the bit reader count in 32 bits
        au_descs.resize(n_frames);
        uint32_t k = 0;
        for (uint32_t i = 0; i < n_streams; ++i) {
            if (!stream_ok(e, ts[i].stream)) return SK_ERR_BAD_STREAM;
            if (e->streams[ts[i].stream].channels > SK_MAX_CHANNELS) return SK_ERR_INVALID_ARG;  // a wide PCM stream decodes nothing
            if (ts[i].codec != SK_TICK_AAC) continue;
            for (uint32_t f = 0; f < ts[i].n_frames; ++f, ++k) {
                au_descs[k] = sk_aac_frame_desc{};
                au_descs[k].stream = ts[i].stream;
                au_descs[k].channels = e->streams[ts[i].stream].channels;
                // an ADTS frame is at most 8191 bytes (13-bit frame_length); nothing longer can be an access unit
                if (units[k].byte_len > kMaxAccessUnitBytes) return SK_ERR_INVALID_ARG;
                if (units[k].byte_offset % 4 || (size_t)units[k].byte_offset + units[k].byte_len + 8 > au_len) return SK_ERR_INVALID_ARG;
            }
        }
        descs = au_descs.data();
    }
    static const bool trace = std::getenv("SK_TICK_TRACE") != nullptr;  // per-section host times on stderr
    using TClock = std::chrono::steady_clock;
    TClock::time_point t_mark = TClock::now();
    double t_sec[6] = {0, 0, 0, 0, 0, 0};
    double t_au[3] = {0, 0, 0};  // au mode, inside section 1: host work until the launches are queued | waiting for them | reading the statuses
    double t_rs[4] = {0, 0, 0, 0};  // inside section 2: append jobs built | uploaded + launched | rs_process_ready | the rest
    TClock::time_point t_sub = t_mark;
    auto sub = [&](int k) {
        const TClock::time_point now = TClock::now();
        t_rs[k] += std::chrono::duration<double, std::milli>(now - t_sub).count();
        t_sub = now;
    };
    auto lap = [&](int k) {
        const TClock::time_point now = TClock::now();
        t_sec[k] += std::chrono::duration<double, std::milli>(now - t_mark).count();
        t_mark = now;
    };

    // ---- validate the stream table ----
    std::vector<TickCall> tc(n_streams);
    {
        std::vector<uint8_t> seen(e->streams.size(), 0);
        uint64_t total = 0, total_mp3 = 0, total_mpa = 0;
        for (uint32_t i = 0; i < n_streams; ++i) {
            const sk_tick_stream &t = ts[i];
            if (!stream_ok(e, t.stream)) return SK_ERR_BAD_STREAM;
            if (e->streams[t.stream].channels > SK_MAX_CHANNELS) return SK_ERR_INVALID_ARG;  // a wide PCM stream decodes nothing
            if (seen[t.stream]++) return SK_ERR_INVALID_ARG;  // a stream appears once per tick
            if (t.out_bits != 16 && t.out_bits != 24 && t.out_bits != 32) return SK_ERR_INVALID_ARG;
            if (t.out_channels == 0) return SK_ERR_INVALID_ARG;
            if (t.resample && !e->streams[t.stream].rs_open) return SK_ERR_BAD_STREAM;
            if (t.codec == SK_TICK_MPA) {  // (n_frames counts UNITS here: the entry point made them of the stream's frames)
                if (total_mpa + t.n_frames > mp3.n_mpa_units) return SK_ERR_INVALID_ARG;
                tc[i].ch = e->streams[t.stream].channels;
                for (uint32_t f = 0; f < t.n_frames; ++f) {
                    const uint32_t g = n_l3 + (uint32_t)total_mpa + f;
                    if (mp3.descs[g].stream != t.stream || mp3.descs[g].channels != tc[i].ch || mp3.granules[g].channels != tc[i].ch) return SK_ERR_INVALID_ARG;
                    if (mp3.mpa->unit_len[total_mpa + f] != mp3.mpa->unit_len[total_mpa]) return SK_ERR_INVALID_ARG;  // one layer per stream
                }
                tc[i].first = n_l3 + (uint32_t)total_mpa;
                tc[i].mp3 = true;
                tc[i].ulen = t.n_frames ? mp3.mpa->unit_len[total_mpa] : 576;
                total_mpa += t.n_frames;
                continue;
            }
            if (t.codec == SK_TICK_MP3) {  // its units are the next n_frames granules
                if (total_mp3 + t.n_frames > n_l3) return SK_ERR_INVALID_ARG;
                tc[i].ch = e->streams[t.stream].channels;
                for (uint32_t f = 0; f < t.n_frames; ++f) {
                    const uint32_t g = (uint32_t)total_mp3 + f;
                    if (mp3.descs[g].stream != t.stream || mp3.descs[g].channels != tc[i].ch || mp3.granules[g].channels != tc[i].ch) return SK_ERR_INVALID_ARG;
                }
                tc[i].first = (uint32_t)total_mp3;
                tc[i].mp3 = true;
                tc[i].ulen = 576;
                total_mp3 += t.n_frames;
                continue;
            }
            if (t.codec != SK_TICK_AAC) return SK_ERR_INVALID_ARG;
            if (total + t.n_frames > n_frames) return SK_ERR_INVALID_ARG;
            for (uint32_t f = 0; f < t.n_frames; ++f)
                if (descs[total + f].stream != t.stream) return SK_ERR_INVALID_ARG;
            tc[i].ch = e->streams[t.stream].channels;
            tc[i].first = (uint32_t)total;
            total += t.n_frames;
        }
        if (total != n_frames || total_mp3 != n_l3 || total_mpa != mp3.n_mpa_units) return SK_ERR_INVALID_ARG;
    }

    // ---- synthesis of the whole batch ----
    std::vector<int32_t> status(n_frames, 0);
    bool status_pinned = false;  // the device front-ends' statuses arrive in e->h_status and are copied over after the wait
    HostPlan hp;
    int rc = build_plan_host(e, descs, n_frames, status.data(), hp, !au_mode);  // au mode: the windows are not known yet
    if (rc != SK_OK) return rc;
    std::vector<uint64_t> off1024(n_frames + 1, 0);
    for (uint32_t i = 0; i < n_frames; ++i) off1024[i + 1] = off1024[i] + descs[i].channels;
    // the MP3 granules' channel rows follow the AAC units' in the PCM staging buffer (rows of 1024 floats, 576 of them used)
    std::vector<uint64_t> mp3_row(mp3.n + 1, 0);
    mp3_row[0] = hp.off1024;
    for (uint32_t g = 0; g < mp3.n; ++g) mp3_row[g + 1] = mp3_row[g] + mp3.granules[g].channels;
    const uint64_t total_rows = mp3_row[mp3.n];
    if (total_rows * 1024 > 0xffffffffull) return SK_ERR_INVALID_ARG;
    auto unit_row = [&](uint32_t i, uint32_t f) { return tc[i].mp3 ? mp3_row[tc[i].first + f] : off1024[tc[i].first + f]; };
    for (uint32_t i = 0; i < n_streams; ++i) {
        tc[i].good = ts[i].n_frames;
        if (tc[i].mp3) continue;  // decided when the granules are queued (tick_mp3 below)
        for (uint32_t f = 0; f < ts[i].n_frames; ++f)
            if (status[tc[i].first + f] != 0) {
                tc[i].good = f;
                tc[i].bad_status = status[tc[i].first + f];
                break;
            }
    }
    lap(0);
    // from here to the tick's last wait the device belongs to this engine (see g_device_turn)
    std::unique_lock<std::mutex> turn;
    if (g_engines_on_device[e->device & 15].load() > kTurnFrom) turn = std::unique_lock<std::mutex>(g_device_turn[e->device & 15]);
    const size_t elems = (size_t)hp.off1024 * 1024;
    const size_t arena_bytes = ((size_t)16 << 20) + (size_t)n_frames * 512 + (size_t)n_streams * 1024 + (size_t)mp3.n * 512;
    SK_HIP(e->in_buf.reserve(elems * 4 + 16), "alloc tick coeffs");
    SK_HIP(e->tick_pcm.reserve((size_t)total_rows * 1024 * 4 + 16), "alloc tick pcm");
    SK_HIP(e->tick_arena.reserve(arena_bytes), "alloc tick arena");
    if (e->h_arena_cap < e->tick_arena.cap) {
        if (e->h_arena) (void)hipHostFree(e->h_arena);
        e->h_arena = nullptr;
        e->h_arena_cap = 0;
        SK_HIP(hipHostMalloc((void **)&e->h_arena, e->tick_arena.cap, hipHostMallocDefault), "alloc pinned arena");
        e->h_arena_cap = e->tick_arena.cap;
    }
    AuxArena aux{(uint8_t *)e->tick_arena.p, e->tick_arena.cap, 0, e->h_arena};
    float *d_pcm = (float *)e->tick_pcm.p;
    if (mp3.n) {  // queued in front of the AAC work: nothing below waits for it separately
        std::vector<int32_t> mp3_status;
        mp3_status.assign(mp3.n, 0);
        if (n_l3) rc = tick_mp3_queue(e, mp3, d_pcm + (size_t)hp.off1024 * 1024, aux, mp3_status);
        if (rc != SK_OK) return rc;
        if (mp3.n_mpa_units) rc = tick_mpa_queue(e, mp3, d_pcm + (size_t)hp.off1024 * 1024, aux);  // checked records: no unit of theirs fails
        if (rc != SK_OK) return rc;
        for (uint32_t i = 0; i < n_streams; ++i) {
            if (!tc[i].mp3) continue;
            for (uint32_t f = 0; f < ts[i].n_frames; ++f)
                if (mp3_status[tc[i].first + f] != 0) {
                    tc[i].good = f;
                    tc[i].bad_status = mp3_status[tc[i].first + f];
                    break;
                }
        }
    }
    if (!hp.tasks.empty()) {
        sk::SynthArgs a{};
        a.coeffs = (const float *)e->in_buf.p;
        a.pcm = d_pcm;
        a.delay = e->d_delay;
        a.prev_shape = e->d_prev_shape;
        SK_HIP(aux.put(hp.tasks, e->stream, &a.tasks), "upload tick tasks");
        SK_HIP(aux.put(hp.entries, e->stream, &a.entries), "upload tick entries");
        a.n_tasks = (uint32_t)hp.tasks.size();
        a.t = e->synth_tables;
        if (!au_mode && !q_mode) {
            SK_HIP(hipMemcpyAsync(e->in_buf.p, coeffs, elems * 4, hipMemcpyHostToDevice, e->stream), "H2D tick coeffs");
        } else {
            // the front-end on the device: one lane per stream, spectra straight into the synthesis input
            rc = ensure_entropy_tables(e);
            if (rc != SK_OK) return rc;
            if (q_mode) {  // the host's integers and side records instead of the access units
                SK_HIP(e->tick_au.reserve((size_t)n_frames * sizeof(sk_ec::WireUnit) + 16), "alloc tick side records");
                SK_HIP(e->tick_q.reserve(elems * sizeof(int16_t) + 16), "alloc tick quantised values");
                SK_HIP(hipMemcpyAsync(e->tick_au.p, q_sides, (size_t)n_frames * sizeof(sk_ec::WireUnit), hipMemcpyHostToDevice, e->stream),
                       "H2D side records");
                SK_HIP(hipMemcpyAsync(e->tick_q.p, q_quant, elems * sizeof(int16_t), hipMemcpyHostToDevice, e->stream), "H2D quantised values");
            } else {
                SK_HIP(e->tick_au.reserve(au_len + 16), "alloc tick access units");
                SK_HIP(hipMemcpyAsync(e->tick_au.p, au_bytes, au_len, hipMemcpyHostToDevice, e->stream), "H2D access units");
            }
            std::vector<sk::EntropyUnit> eu(n_frames);
            std::vector<sk::EntropyTask> et;
            for (uint32_t i = 0; i < n_streams; ++i) {
                if (ts[i].n_frames == 0 || tc[i].mp3) continue;
                const StreamInfo &si = e->streams[ts[i].stream];
                et.push_back(sk::EntropyTask{ts[i].stream, tc[i].first, ts[i].n_frames, sf_index_of(si.sample_rate), si.channels});
                for (uint32_t f = 0; f < ts[i].n_frames; ++f) {
                    const uint32_t k = tc[i].first + f;
                    eu[k] = sk::EntropyUnit{q_mode ? 0u : units[k].byte_offset / 4, q_mode ? 0u : units[k].byte_len, (uint32_t)off1024[k],
                                            {hp.entry_of[(size_t)k * 2], hp.entry_of[(size_t)k * 2 + (si.channels > 1 ? 1 : 0)]},
                                            (uint32_t)et.size() - 1};
                }
            }
            std::vector<int32_t> st_init(n_frames, 0);
            sk::EntropyArgs ea = e->ec_args;
            ea.words = q_mode ? (const uint32_t *)e->d_zeros : (const uint32_t *)e->tick_au.p;
            ea.wire = q_mode ? (const sk_ec::WireUnit *)e->tick_au.p : nullptr;
            ea.quant = q_mode ? (const int16_t *)e->tick_q.p : nullptr;
            SK_HIP(aux.put(eu, e->stream, &ea.units), "upload entropy units");
            SK_HIP(aux.put(et, e->stream, &ea.tasks), "upload entropy tasks");
            const int32_t *d_status = nullptr;
            SK_HIP(aux.put(st_init, e->stream, &d_status), "upload entropy status");
            ea.n_tasks = (uint32_t)et.size();
            ea.pns_state = e->d_pns;
            ea.coeffs = (float *)e->in_buf.p;
            ea.entries = const_cast<sk::SynthEntry *>(a.entries);
            ea.status = const_cast<int32_t *>(d_status);
            {
                SK_HIP(e->tick_side.reserve((size_t)n_frames * (sizeof(sk_ec::Scratch) + sizeof(uint32_t)) + 128),
                       "alloc entropy side information");
                ea.n_units = n_frames;
                // units per wave: 16 up to two waves per SIMD (2048 waves), then 32, then 64 -- a wave runs the union of its
                // lanes' paths, a SIMD with one wave has every latency in the open, and past a couple of waves per SIMD the
                // vector issue rate is the limit (a wave instruction costs the same with 16 lanes populated as with 64).
                // tools/prof_entropy_tick.sh, parse + finish: 22 400 units 4.17 / 3.26 / 3.03 ms at 64 / 32 / 16 per wave,
                // 54 400 units 4.17 / 3.37 / 3.62 ms (SK_ENTROPY_LANE_SHIFT forces a value)
                static const int forced_shift = [] {
                    const char *v = std::getenv("SK_ENTROPY_LANE_SHIFT");
                    return v && v[0] >= '0' && v[0] <= '4' ? (int)(v[0] - '0') : -1;
                }();
                ea.lane_shift = forced_shift >= 0 ? (uint32_t)forced_shift : (n_frames <= 32768 ? 2u : (n_frames <= 131072 ? 1u : 0u));
                // slot -> unit, by size (a counting sort on byte_len / 8): a wave's lanes then carry units with about the same
                // number of codewords instead of waiting for the largest of 32 arbitrary ones.  SK_ENTROPY_UNSORTED=1: as given.
                static const bool unsorted = std::getenv("SK_ENTROPY_UNSORTED") != nullptr;
                if (!q_mode && !unsorted && n_frames > 64) {
                    std::vector<uint32_t> order(n_frames), start(1026, 0);
                    for (uint32_t k = 0; k < n_frames; ++k) ++start[std::min<uint32_t>(eu[k].byte_len >> 3, 1023) + 1];
                    for (uint32_t b = 1; b < 1026; ++b) start[b] += start[b - 1];
                    for (uint32_t k = 0; k < n_frames; ++k) order[start[std::min<uint32_t>(eu[k].byte_len >> 3, 1023)]++] = k;
                    SK_HIP(aux.put(order, e->stream, &ea.order), "upload entropy unit order");
                }
                ea.side = (sk_ec::Scratch *)e->tick_side.p;
                ea.pns_start = (uint32_t *)((uint8_t *)e->tick_side.p + (((size_t)n_frames * sizeof(sk_ec::Scratch) + 15) & ~(size_t)15));
                SK_HIP(sk::launch_aac_entropy_parallel(ea, e->stream), "launch entropy decode");
            }
            if (e->h_status_cap < n_frames) {
                if (e->h_status) (void)hipHostFree(e->h_status);
                e->h_status = nullptr;
                e->h_status_cap = 0;
                const size_t want = (size_t)n_frames + (size_t)n_frames / 2 + 1024;
                SK_HIP(hipHostMalloc((void **)&e->h_status, want * sizeof(int32_t), hipHostMallocDefault), "alloc pinned status");
                e->h_status_cap = want;
            }
            SK_HIP(hipMemcpyAsync(e->h_status, d_status, (size_t)n_frames * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream),
                   "D2H entropy status");
            status_pinned = true;
        }
        if (probe) {  // the front-end alone: spectra, window fields and statuses back to the caller, nothing synthesised
            std::vector<sk::SynthEntry> got(hp.entries.size());
            SK_HIP(hipMemcpyAsync(got.data(), a.entries, got.size() * sizeof(sk::SynthEntry), hipMemcpyDeviceToHost, e->stream),
                   "D2H entropy window fields");
            SK_HIP(hipMemcpyAsync(probe->spectra, e->in_buf.p, elems * 4, hipMemcpyDeviceToHost, e->stream), "D2H entropy spectra");
            SK_HIP(hipStreamSynchronize(e->stream), "entropy sync");
            if (status_pinned) std::memcpy(status.data(), e->h_status, (size_t)n_frames * sizeof(int32_t));
            for (uint32_t k = 0; k < n_frames; ++k) {
                probe->status[k] = status[k];
                probe->descs[k] = descs[k];
                for (uint32_t c = 0; c < descs[k].channels; ++c) {
                    const uint32_t win = got[hp.entry_of[(size_t)k * 2 + c]].win;
                    probe->descs[k].window_sequence[c] = (uint8_t)(win & 3u);
                    probe->descs[k].window_shape[c] = (uint8_t)((win >> 2) & 1u);
                }
            }
            return SK_OK;
        }
        a.only_long = 1;
        if (!hp.pair_tasks.empty()) {
            SK_HIP(aux.put(hp.pair_tasks, e->stream, &a.tasks), "upload tick pair tasks");
            a.n_tasks = (uint32_t)hp.pair_tasks.size();
            SK_HIP(sk::launch_aac_synth_pairs(a, false, e->stream), "launch tick synth (two channels per wave)");
        }
        if (!hp.spair_tasks.empty()) {
            SK_HIP(aux.put(hp.spair_tasks, e->stream, &a.tasks), "upload tick pair tasks with EightShort frames");
            a.n_tasks = (uint32_t)hp.spair_tasks.size();
            SK_HIP(sk::launch_aac_synth_pairs(a, true, e->stream), "launch tick synth (two channels per wave, eight-short arm)");
        }
        if (!hp.long_tasks.empty()) {
            SK_HIP(aux.put(hp.long_tasks, e->stream, &a.tasks), "upload tick tasks without EightShort frames");
            a.n_tasks = (uint32_t)hp.long_tasks.size();
            SK_HIP(sk::launch_aac_synth(a, e->stream), "launch tick synth (one channel per wave, no EightShort)");
        }
        if (!hp.walk_tasks.empty()) {
            SK_HIP(aux.put(hp.walk_tasks, e->stream, &a.tasks), "upload tick walk tasks");
            a.n_tasks = (uint32_t)hp.walk_tasks.size();
            a.only_long = 0;
            SK_HIP(sk::launch_aac_synth(a, e->stream), "launch tick synth");
        }
        if (au_mode || q_mode) {  // which units failed decides what the later stages may use
            const TClock::time_point q0 = TClock::now();
            t_au[0] = std::chrono::duration<double, std::milli>(q0 - t_mark).count();
            rc = wait_stream(e, "tick: waiting for the front-end kernels and the synthesis (mid-tick status read-back)");
            if (rc != SK_OK) return rc;
            if (status_pinned) std::memcpy(status.data(), e->h_status, (size_t)n_frames * sizeof(int32_t));
            e->where.store("tick: resampler rounds, pack");
            t_au[1] = std::chrono::duration<double, std::milli>(TClock::now() - q0).count();
            for (uint32_t i = 0; i < n_streams; ++i) {
                if (tc[i].mp3) continue;
                tc[i].good = ts[i].n_frames;
                tc[i].bad_status = 0;
                for (uint32_t f = 0; f < ts[i].n_frames; ++f)
                    if (status[tc[i].first + f] != 0) {
                        tc[i].good = f;
                        tc[i].bad_status = status[tc[i].first + f];
                        break;
                    }
            }
        }
    }

    lap(1);
    t_sub = t_mark;
    // ---- streaming resamplers ----
    std::vector<RsCall> calls;
    std::vector<uint32_t> call_stream;  // RsCall -> index into ts
    size_t res_rows = 0;
    uint32_t res_cap = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        if (!ts[i].resample) continue;
        const StreamInfo &s = e->streams[ts[i].stream];
        RsCall c;
        c.id = ts[i].stream;
        c.channels = tc[i].ch;
        c.row0 = res_rows;
        res_rows += c.channels;
        tc[i].rs_call = (int)calls.size();
        calls.push_back(c);
        call_stream.push_back(i);
        const uint64_t max_chunks = ((uint64_t)s.rs_fill + (uint64_t)tc[i].good * tc[i].ulen) / kRsChunk + 1;
        const uint64_t per_chunk = (uint64_t)std::ceil((double)kRsChunk * (double)s.rs_out_hz / (double)s.rs_in_hz) + 2;
        if (max_chunks * per_chunk > 0x7fffffffull) return SK_ERR_INVALID_ARG;
        res_cap = std::max<uint32_t>(res_cap, (uint32_t)(max_chunks * per_chunk));
    }
    const size_t res_stride = ((size_t)res_cap + 3) & ~(size_t)3;
    float *d_res = nullptr;
    if (!calls.empty()) {
        if (res_rows * res_stride > 0xffffffffull) return SK_ERR_INVALID_ARG;
        SK_HIP(e->tick_res.reserve(res_rows * res_stride * 4 + 16), "alloc tick resampler output");
        d_res = (float *)e->tick_res.p;
        std::vector<sk::RowCopy> jobs;
        sub(3);
        RsRounds rounds;
        rounds.total_in = [&](size_t ci) { return tc[call_stream[ci]].good * tc[call_stream[ci]].ulen; };
        rounds.append = [&](size_t ci, uint32_t take, uint32_t fill) {
            const RsCall &c = calls[ci];
            const TickCall &t = tc[call_stream[ci]];
            uint32_t consumed = c.consumed;
            const uint32_t taken = take;
            // Pieces never straddle a unit of the packed synthesis output.  Whole units whose rows lie a constant distance apart
            // (the usual case: a stream's units of a tick) go down as ONE job per channel.
            size_t run_at = 0;        // index in `jobs` of the open run's first channel, valid while run_pieces > 0
            uint32_t run_pieces = 0;
            uint64_t run_row = 0, run_stride = 0;
            while (take) {
                const uint32_t frame = consumed / t.ulen, within = consumed % t.ulen;
                const uint32_t n = std::min(take, t.ulen - within);
                const uint64_t row = unit_row(call_stream[ci], frame);
                const bool whole = within == 0 && n == t.ulen;
                bool joined = false;
                if (whole && run_pieces) {
                    const uint64_t stride = row - run_row;  // (of a row above the run's last one; anything else starts a new run)
                    if (row > run_row && (run_pieces == 1 || stride == run_stride) && stride * 1024 <= 0xffffffffull) {
                        for (uint32_t ch = 0; ch < c.channels; ++ch) {
                            jobs[run_at + ch].pieces += 1;
                            jobs[run_at + ch].src_stride = (uint32_t)(stride * 1024);
                        }
                        run_stride = stride, run_row = row, run_pieces += 1;
                        joined = true;
                    }
                }
                if (!joined) {
                    run_at = jobs.size();
                    for (uint32_t ch = 0; ch < c.channels; ++ch)  // MP3 rows hold q / 32768 already: a plain copy
                        jobs.push_back(sk::RowCopy{(row + ch) * 1024 + within, (rs_row0(e, c.id) + ch) * kRsRow + kRsBase + kRsHist + fill, n,
                                                   t.mp3 ? 0u : 1u});
                    run_pieces = whole ? 1 : 0;
                    run_row = row;
                }
                fill += n;
                consumed += n;
                take -= n;
            }
            return taken;
        };
        rounds.launch = [&]() -> int {
            if (jobs.empty()) return SK_OK;
            const sk::RowCopy *d_jobs = nullptr;
            SK_HIP(aux.put(jobs, e->stream, &d_jobs), "upload tick append jobs");
            for (size_t j0 = 0; j0 < jobs.size(); j0 += 65535)
                SK_HIP(sk::launch_row_copies(d_pcm, e->d_rs, d_jobs + j0, (uint32_t)std::min<size_t>(65535, jobs.size() - j0),
                                             e->stream), "tick append chunk");
            jobs.clear();
            return SK_OK;
        };
        rounds.flush = [&](size_t ci) { return ts[call_stream[ci]].flush && tc[call_stream[ci]].good == ts[call_stream[ci]].n_frames; };
        rounds.chunks = [&](size_t ci) -> std::vector<std::pair<uint32_t, uint32_t>> & { return tc[call_stream[ci]].chunks; };
        rounds.sub = sub;
        rc = rs_run_rounds(e, calls, d_res, res_stride, res_cap, aux, rounds);
        if (rc != SK_OK) return rc;
    }

    sub(3);
    lap(2);
    // ---- output records and the pack jobs that fill them ----
    std::vector<sk::PackJob> packs;
    uint32_t n_rec = 0, max_pack_frames = 0;
    size_t cursor = 0;
    uint8_t *d_out = nullptr;
    auto emit = [&](uint32_t stream_index, uint32_t frames, uint32_t ch_out, uint32_t bits, int32_t st) -> sk_tick_output * {
        if (n_rec >= outs_cap) return nullptr;
        sk_tick_output &o = outs[n_rec++];
        o.stream_index = stream_index;
        o.frames = frames;
        o.channels = (uint8_t)ch_out;
        o.bits = (uint8_t)bits;
        o.reserved = 0;
        o.status = st;
        o.bytes = frames * ch_out * (bits / 8);
        o.byte_offset = cursor;
        cursor += ((size_t)o.bytes + 15) & ~(size_t)15;
        return &o;
    };
    // first pass sizes the output, second creates the jobs (the device buffer may move when it grows)
    for (int pass = 0; pass < 2; ++pass) {
        n_rec = 0;
        cursor = 0;
        for (uint32_t i = 0; i < n_streams; ++i) {
            const sk_tick_stream &t = ts[i];
            const uint32_t ch = tc[i].ch;
            const uint32_t ch_out = t.out_channels < ch ? t.out_channels : ch;
            if (!t.resample) {
                const StreamInfo &s = e->streams[t.stream];
                (void)s;
                const bool direct = t.out_bits == 16 && t.out_channels == ch;
                const uint32_t ulen = tc[i].ulen;
                const uint8_t mode = tc[i].mp3 ? (uint8_t)sk::kPackFromQ : (uint8_t)(direct ? sk::kPackDirect : sk::kPackViaS16);
                for (uint32_t f = 0; f < tc[i].good; ++f) {
                    sk_tick_output *o = emit(i, ulen, ch_out, t.out_bits, 0);
                    if (!o) return SK_ERR_INVALID_ARG;
                    if (pass) {
                        const float *src = d_pcm + unit_row(i, f) * 1024;
                        packs.push_back(sk::PackJob{src, src + 1024, d_out + o->byte_offset, ulen, (uint8_t)ch, (uint8_t)ch_out, t.out_bits, mode});
                        max_pack_frames = std::max<uint32_t>(max_pack_frames, ulen);
                    }
                }
            } else {
                const RsCall &c = calls[(size_t)tc[i].rs_call];
                for (const auto &chunk : tc[i].chunks) {
                    sk_tick_output *o = emit(i, chunk.second, ch_out, t.out_bits, 0);
                    if (!o) return SK_ERR_INVALID_ARG;
                    if (pass) {
                        const float *src = d_res + c.row0 * res_stride + chunk.first;
                        packs.push_back(sk::PackJob{src, src + res_stride, d_out + o->byte_offset, chunk.second, (uint8_t)ch,
                                                    (uint8_t)ch_out, t.out_bits, (uint8_t)sk::kPackPlain});
                        max_pack_frames = std::max(max_pack_frames, chunk.second);
                    }
                }
            }
            if (tc[i].good != t.n_frames)  // the frame the engine rejected: Err(DecodingFailed) ends the stream
                if (!emit(i, 0, ch_out, t.out_bits, tc[i].bad_status)) return SK_ERR_INVALID_ARG;
        }
        if (pass == 0) {
            if (cursor > out_cap || (cursor && !out)) return SK_ERR_INVALID_ARG;
            SK_HIP(e->tick_out.reserve(cursor + 16), "alloc tick output");
            d_out = (uint8_t *)e->tick_out.p;
        }
    }
    uint8_t *bounce = nullptr;
    if (!packs.empty()) {
        const sk::PackJob *d_packs = nullptr;
        SK_HIP(aux.put(packs, e->stream, &d_packs), "upload pack jobs");
        SK_HIP(sk::launch_pack_jobs(d_packs, (uint32_t)packs.size(), max_pack_frames, e->stream), "launch pack");
        rc = tick_queue_d2h(e, out, d_out, cursor, &bounce);
        if (rc != SK_OK) return rc;
    }
    lap(3);
    rc = wait_stream(e, "tick: waiting for the device at the end of the tick");
    if (rc != SK_OK) return rc;
    if (bounce) std::memcpy(out, bounce, cursor);
    lap(4);
    if (trace)
        std::fprintf(stderr, "sk_tick_run: %u streams %u frames | plan %.2f  h2d+synth %.2f  resample %.2f  pack %.2f  sync %.2f ms | au: queue %.2f wait %.2f | resample: jobs %.2f copies %.2f process %.2f rest %.2f\n",
                     n_streams, n_frames, t_sec[0], t_sec[1], t_sec[2], t_sec[3], t_sec[4], t_au[0], t_au[1], t_rs[0], t_rs[1], t_rs[2], t_rs[3]);
    *n_outs = n_rec;
    if (out_bytes) *out_bytes = cursor;
    return SK_OK;
}

// The host-side state a tick advances -- the streaming resamplers' fill, chunk count and time index -- as it stood before the tick
struct RsSaved {
    struct Saved {
        uint32_t id, fill;
        uint64_t chunks;
        double last;
    };
    std::vector<Saved> saved;
    void add(const sk_engine *e, uint32_t id) {
        if (!stream_ok(e, id) || !e->streams[id].rs_open) return;
        const StreamInfo &s = e->streams[id];
        saved.push_back(Saved{id, s.rs_fill, s.rs_chunks, s.rs_last_index});
    }
    void restore(sk_engine *e) const {
        for (const Saved &v : saved) {
            StreamInfo &s = e->streams[v.id];
            s.rs_fill = v.fill;
            s.rs_chunks = v.chunks;
            s.rs_last_index = v.last;
        }
    }
};

// The tick proper (tick_body) under the engine's lock, with the host-side state it advances -- the streaming resamplers'
// fill, chunk count and time index -- put back when it fails part-way: a failed launch leaves the batch's streams to be
// ended by the caller, and the engine's bookkeeping must not have run ahead of what the device did.
int tick_impl_locked(sk_engine *e, const sk_tick_stream *ts, uint32_t n_streams, const sk_aac_frame_desc *descs, const float *coeffs,
                     const sk_au_item *units, const uint8_t *au_bytes, size_t au_len, uint32_t n_frames, uint8_t *out, size_t out_cap,
                     sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes, const EntropyProbe *probe,
                     const uint8_t *q_sides, const int16_t *q_quant, const TickMp3 &mp3);

int tick_impl(sk_engine *e, const sk_tick_stream *ts, uint32_t n_streams, const sk_aac_frame_desc *descs, const float *coeffs,
              const sk_au_item *units, const uint8_t *au_bytes, size_t au_len, uint32_t n_frames, uint8_t *out, size_t out_cap,
              sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes, const EntropyProbe *probe = nullptr,
              const uint8_t *q_sides = nullptr, const int16_t *q_quant = nullptr, const TickMp3 &mp3 = TickMp3{}) {
    if (!e) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    return tick_impl_locked(e, ts, n_streams, descs, coeffs, units, au_bytes, au_len, n_frames, out, out_cap, outs, outs_cap, n_outs, out_bytes, probe,
                            q_sides, q_quant, mp3);
}

// e->mu held
int tick_impl_locked(sk_engine *e, const sk_tick_stream *ts, uint32_t n_streams, const sk_aac_frame_desc *descs, const float *coeffs,
                     const sk_au_item *units, const uint8_t *au_bytes, size_t au_len, uint32_t n_frames, uint8_t *out, size_t out_cap,
                     sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes, const EntropyProbe *probe,
                     const uint8_t *q_sides, const int16_t *q_quant, const TickMp3 &mp3) {
    TickWhere where(e);
    RsSaved saved;
    for (uint32_t i = 0; ts && i < n_streams; ++i)
        if (ts[i].resample) saved.add(e, ts[i].stream);
    const int rc = tick_body(e, ts, n_streams, descs, coeffs, units, au_bytes, au_len, n_frames, out, out_cap, outs, outs_cap, n_outs,
                             out_bytes, probe, q_sides, q_quant, mp3);
    if (rc != SK_OK) {
        saved.restore(e);
        if (n_outs) *n_outs = 0;
        if (out_bytes) *out_bytes = 0;
        // whatever was queued before the failure must be off the stream before the caller reuses its buffers
        if (rc != SK_ERR_TIMEOUT) (void)hipStreamSynchronize(e->stream);
    }
    return rc;
}


// ---- sk_tick_run_pcm: the tick of the WAV / raw PCM streams ------------------------------------------------------------------

struct PcmCall {  // one sk_pcm_tick_stream
    uint32_t first = 0;        // index of its first unit
    uint32_t frame_bytes = 0;  // of the source
    uint32_t total_frames = 0;
    uint32_t ch_out = 0;
    uint8_t fmt_out = 0;       // SK_FMT_S16LE / S24LE / S32LE / F32LE
    bool exact = false, float_out = false;
    int rs_call = -1;
    uint32_t unit = 0, within = 0;  // where the resampler rounds stand: unit (relative to first) and frame inside it
    std::vector<std::pair<uint32_t, uint32_t>> chunks;  // (column, frames) of each resampled AudioData
};

// sk_tick_run_aiff: what stands in front of the PCM tick's body.  The body's stream table and units describe the DECODED PCM (a
// little-endian source of the contract's format, laid out in tick_aiff); `bytes` are the source-encoded units.
struct AiffTick {
    const sk_aiff_tick_stream *as = nullptr;
    const sk_pcm_unit *src_units = nullptr;  // the caller's units, into `bytes`
    size_t decoded_len = 0;                  // of the decoded layout
    std::vector<uint8_t> plain;              // per stream: nothing to change behind the decode -- the decoded bytes are its outputs, one per unit
    std::vector<uint32_t> states;            // out: 2 per stream, what k_aiff_ima4 left ((uint16_t)predictor | step_index << 16)
    // sk_tick_run_flac: another decode in the place of the AIFF one -- the same two passes to the same destinations; d_src = the uploaded units
    std::function<int(bool as_is, const std::function<uint8_t *(uint32_t, uint32_t)> &dst_of, const uint8_t *d_src)> decode;
};

bool pcm_fmt_is_float(int fmt) { return fmt == SK_FMT_F32LE || fmt == SK_FMT_F32BE; }
uint32_t pcm_fmt_bits(int fmt) { return fmt <= SK_FMT_S16BE ? 16 : (fmt <= SK_FMT_S24BE ? 24 : 32); }

// Checks the table and fills in what follows from it.  SK_OK, or the status sk_tick_run_pcm returns.
int pcm_tick_plan(const sk_engine *e, const sk_pcm_tick_stream *ts, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units, size_t bytes_len,
                  std::vector<PcmCall> &pc, const uint8_t *plain = nullptr) {
    pc.assign(n_streams, PcmCall{});
    std::vector<uint8_t> seen(e->streams.size(), 0);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        const sk_pcm_tick_stream &t = ts[i];
        PcmCall &c = pc[i];
        if (t.format > SK_FMT_F32BE) return SK_ERR_INVALID_ARG;
        if (t.channels == 0 || t.out_channels == 0) return SK_ERR_INVALID_ARG;
        // 3 ... 8 channels: only an engine that reserved the slots for them (sk_engine_enable_wide_pcm) takes them
        const bool as_is = plain && plain[i];  // a decoded AIFF stream with nothing further to change: any channel count, no device work here
        if (!as_is && t.channels > SK_MAX_CHANNELS && (t.channels > SK_MAX_PCM_CHANNELS || !e->wide_enabled)) return SK_ERR_UNSUPPORTED;
        if (t.out_bits != 16 && t.out_bits != 24 && t.out_bits != 32) return SK_ERR_INVALID_ARG;
        const uint32_t bits = pcm_fmt_bits(t.format);
        // the fast path (lib.rs:3339-3345) needs no device: such a stream's pieces are delivered as they are, by the caller
        if (!as_is && !t.resample && t.out_bits == bits && t.out_channels == t.channels) return SK_ERR_INVALID_ARG;
        if (t.resample) {
            if (!stream_ok(e, t.stream) || !e->streams[t.stream].rs_open || e->streams[t.stream].channels != t.channels) return SK_ERR_BAD_STREAM;
            if (seen[t.stream]++) return SK_ERR_INVALID_ARG;  // a stream appears once per tick
        } else if (t.flush) {
            return SK_ERR_INVALID_ARG;
        }
        c.first = (uint32_t)at;
        c.frame_bytes = bits / 8 * t.channels;
        c.ch_out = t.out_channels < t.channels ? t.out_channels : t.channels;
        c.float_out = t.out_bits == 32 && pcm_fmt_is_float(t.format);  // lib.rs:3377-3382
        c.fmt_out = (uint8_t)(c.float_out ? SK_FMT_F32LE : (t.out_bits == 16 ? SK_FMT_S16LE : (t.out_bits == 24 ? SK_FMT_S24LE : SK_FMT_S32LE)));
        c.exact = !t.resample && t.out_channels == t.channels && t.out_bits == 16 && !pcm_fmt_is_float(t.format) && bits > 16;  // lib.rs:3349-3356
        if (at + t.n_units > n_units) return SK_ERR_INVALID_ARG;
        uint64_t frames = 0;
        for (uint32_t u = 0; u < t.n_units; ++u) {
            const sk_pcm_unit &un = units[at + u];
            // (a decoded AIFF unit that is delivered as it is holds whole samples, not necessarily whole frames: the reference's decoder
            // emits every complete sample of an `add`)
            if (un.byte_offset % 16 || un.byte_len == 0 || un.byte_len > 0x7fffffffu || (!as_is && un.byte_len % c.frame_bytes)) return SK_ERR_INVALID_ARG;
            if (un.byte_offset > bytes_len || un.byte_len > bytes_len - un.byte_offset) return SK_ERR_INVALID_ARG;
            frames += un.byte_len / c.frame_bytes;
        }
        if (frames > 0x7fffffffull) return SK_ERR_INVALID_ARG;
        c.total_frames = (uint32_t)frames;
        at += t.n_units;
    }
    return at == n_units ? SK_OK : SK_ERR_INVALID_ARG;
}

// frames one 4096-frame chunk of this stream's resampler can produce (+ slack)
uint64_t pcm_chunk_out_frames(const StreamInfo &s) {
    return (uint64_t)std::ceil((double)kRsChunk * (double)s.rs_out_hz / (double)s.rs_in_hz) + 2;
}

// the bound of a table pcm_tick_plan took: plain arithmetic per stream, no walk over the resamplers' chunks
size_t pcm_planned_out_bound(const sk_engine *e, const sk_pcm_tick_stream *ts, uint32_t n_streams, const std::vector<PcmCall> &pc, uint32_t *max_outputs,
                             const uint8_t *plain) {
    size_t bytes = 0;
    uint64_t outs = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        const uint64_t frame_out = (uint64_t)ts[i].out_bits / 8 * pc[i].ch_out;
        if (ts[i].resample) {
            const StreamInfo &s = e->streams[ts[i].stream];
            const uint64_t chunks = ((uint64_t)s.rs_fill + pc[i].total_frames) / kRsChunk + 1;  // + the flush
            bytes += chunks * (pcm_chunk_out_frames(s) * frame_out + 16) + 16;
            outs += chunks;
        } else {
            // (+ a frame per unit: a decoded AIFF unit delivered as it is may end inside a frame)
            bytes += ((uint64_t)pc[i].total_frames + (plain && plain[i] ? ts[i].n_units : 0)) * frame_out + (uint64_t)ts[i].n_units * 16 + 16;
            outs += ts[i].n_units;
        }
    }
    if (max_outputs) *max_outputs = (uint32_t)std::min<uint64_t>(outs + 1, 0xffffffffu);
    return bytes;
}

size_t tick_pcm_out_bound(const sk_engine *e, const sk_pcm_tick_stream *ts, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units,
                          uint32_t *max_outputs, const uint8_t *plain = nullptr) {
    std::vector<PcmCall> pc;
    if (max_outputs) *max_outputs = 0;
    if (pcm_tick_plan(e, ts, n_streams, units, n_units, (size_t)-1, pc, plain) != SK_OK) return 0;
    return pcm_planned_out_bound(e, ts, n_streams, pc, max_outputs, plain);
}

int tick_pcm_body(sk_engine *e, const sk_pcm_tick_stream *ts, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units, const uint8_t *bytes,
                  size_t bytes_len, uint8_t *out, size_t out_cap, sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes,
                  AiffTick *aiff = nullptr) {
    if (!e || !n_outs || (n_streams && !ts) || (n_units && (!units || !bytes))) return SK_ERR_INVALID_ARG;
    *n_outs = 0;
    if (out_bytes) *out_bytes = 0;
    if (n_streams == 0) return n_units == 0 ? SK_OK : SK_ERR_INVALID_ARG;
    DeviceGuard guard(e);
    std::vector<PcmCall> pc;
    int rc = pcm_tick_plan(e, ts, n_streams, units, n_units, aiff ? aiff->decoded_len : bytes_len, pc, aiff ? aiff->plain.data() : nullptr);
    if (rc != SK_OK) return rc;

    // ---- what the tick will deliver, before anything is queued: the resampler rounds rewrite their streams' rows on the device, which
    // the bookkeeping put back after a failure does not undo, so an output that is too small is refused here, with the rows untouched.
    // The records are those of the passes below; a resampled chunk's frames follow from the stream's time index alone.  A caller that
    // brings the bound of sk_tick_pcm_out_bound_on, as the scheduler does, is spared the walk ----
    uint32_t bound_recs = 0;
    const size_t bound_bytes = pcm_planned_out_bound(e, ts, n_streams, pc, &bound_recs, aiff ? aiff->plain.data() : nullptr);
    if (!out || out_cap < bound_bytes || outs_cap < bound_recs) {
        uint64_t need_bytes = 0, need_recs = 0;
        std::vector<double> idx;
        std::map<std::pair<int, double>, std::pair<uint64_t, double>> walked;  // (ratio table, time index) -> (frames, next time index): streams in step share it
        auto chunk_frames = [&](int table, double &last) -> uint64_t {
            auto w = walked.find({table, last});
            if (w == walked.end()) {
                double next = 0.0;
                chunk_indices(e->ratio_tables[(size_t)table].ratio, last, kRsChunk, idx, &next);
                w = walked.emplace(std::make_pair(table, last), std::make_pair((uint64_t)idx.size(), next)).first;
            }
            last = w->second.second;
            return w->second.first;
        };
        auto record = [&](uint64_t bytes) { need_recs += 1, need_bytes += (bytes + 15) & ~15ull; };
        for (uint32_t i = 0; i < n_streams; ++i) {
            const sk_pcm_tick_stream &t = ts[i];
            const PcmCall &c = pc[i];
            const uint64_t frame_out = (uint64_t)(t.out_bits / 8) * c.ch_out;
            if (aiff && aiff->plain[i]) {
                for (uint32_t u = 0; u < t.n_units; ++u) record(units[c.first + u].byte_len);
            } else if (!t.resample) {
                for (uint32_t u = 0; u < t.n_units; ++u) record(units[c.first + u].byte_len / c.frame_bytes * frame_out);
            } else {
                const StreamInfo &s = e->streams[t.stream];
                const uint64_t have = (uint64_t)s.rs_fill + c.total_frames;
                double last = s.rs_last_index;
                for (uint64_t k = 0; k < have / kRsChunk; ++k)
                    if (const uint64_t frames = chunk_frames(s.rs_table, last)) record(frames * frame_out);
                if (t.flush) {  // rs_run_rounds: the rest padded to a chunk, the padding's share trimmed
                    const uint64_t remaining = have % kRsChunk, padded = kRsChunk - remaining;
                    const uint64_t trim = remaining ? (uint64_t)std::llround(((double)padded * (double)s.rs_out_hz) / (double)s.rs_in_hz) : 0;
                    const uint64_t frames = chunk_frames(s.rs_table, last);
                    if (frames > trim) record((frames - trim) * frame_out);
                }
            }
        }
        if (need_bytes > out_cap || (need_bytes && !out) || need_recs > outs_cap) return SK_ERR_INVALID_ARG;
    }

    // from here to the tick's last wait the device belongs to this engine (see g_device_turn)
    std::unique_lock<std::mutex> turn;
    if (g_engines_on_device[e->device & 15].load() > kTurnFrom) turn = std::unique_lock<std::mutex>(g_device_turn[e->device & 15]);

    // ---- the resampling streams' calls and what they can produce ----
    std::vector<RsCall> calls;
    std::vector<uint32_t> call_stream;  // RsCall -> index into ts
    size_t res_rows = 0;
    uint32_t res_cap = 0;
    uint64_t chunk_bound = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        if (!ts[i].resample) continue;
        const StreamInfo &s = e->streams[ts[i].stream];
        RsCall c;
        c.id = ts[i].stream;
        c.channels = ts[i].channels;
        c.row0 = res_rows;
        res_rows += c.channels;
        pc[i].rs_call = (int)calls.size();
        calls.push_back(c);
        call_stream.push_back(i);
        const uint64_t max_chunks = ((uint64_t)s.rs_fill + pc[i].total_frames) / kRsChunk + 1;
        if (max_chunks * pcm_chunk_out_frames(s) > 0x7fffffffull) return SK_ERR_INVALID_ARG;
        res_cap = std::max<uint32_t>(res_cap, (uint32_t)(max_chunks * pcm_chunk_out_frames(s)));
        chunk_bound += max_chunks;
    }
    const size_t res_stride = ((size_t)res_cap + 3) & ~(size_t)3;
    if (res_rows * res_stride > 0xffffffffull) return SK_ERR_INVALID_ARG;

    const size_t arena_bytes = ((size_t)4 << 20) + (size_t)n_units * 256 + (size_t)n_streams * 1024 + (size_t)chunk_bound * 512;
    SK_HIP(e->tick_pcm_in.reserve(bytes_len + 64), "alloc tick pcm input");
    SK_HIP(e->tick_arena.reserve(arena_bytes), "alloc tick arena");
    if (e->h_arena_cap < e->tick_arena.cap) {
        if (e->h_arena) (void)hipHostFree(e->h_arena);
        e->h_arena = nullptr;
        e->h_arena_cap = 0;
        SK_HIP(hipHostMalloc((void **)&e->h_arena, e->tick_arena.cap, hipHostMallocDefault), "alloc pinned arena");
        e->h_arena_cap = e->tick_arena.cap;
    }
    AuxArena aux{(uint8_t *)e->tick_arena.p, e->tick_arena.cap, 0, e->h_arena};
    const uint8_t *d_in = (const uint8_t *)e->tick_pcm_in.p;
    e->where.store("tick (pcm): upload, ingest, resampler rounds");
    if (bytes_len) SK_HIP(hipMemcpyAsync(e->tick_pcm_in.p, bytes, bytes_len, hipMemcpyHostToDevice, e->stream), "H2D tick pcm bytes");

    // ---- AIFF: every unit to the contract's PCM first (aiff_decode.hip).  The streams that go on through the body decode into
    // tick_aiff, which the body then reads in the place of the uploaded bytes; the others decode straight into their output records ----
    std::vector<std::pair<const uint32_t *, std::vector<uint32_t>>> aiff_states;  // (pinned states, AiffImaStream -> index into ts) per launch
    auto aiff_decode = [&](bool as_is, const std::function<uint8_t *(uint32_t, uint32_t)> &dst_of) -> int {
        if (aiff->decode) return aiff->decode(as_is, dst_of, (const uint8_t *)e->tick_pcm_in.p);
        std::vector<sk::AiffElemJob> elems;
        std::vector<sk::AiffImaStream> imas;
        std::vector<sk::AiffImaUnit> ima_units;
        std::vector<uint32_t> ima_of;  // AiffImaStream -> index into ts
        uint32_t max_samples = 0;
        const uint8_t *d_src = (const uint8_t *)e->tick_pcm_in.p;
        for (uint32_t i = 0; i < n_streams; ++i) {
            if ((aiff->plain[i] != 0) != as_is) continue;
            const sk_aiff_tick_stream &a = aiff->as[i];
            const size_t group = sk_pcm::aiff_group_bytes(a.encoding, a.channels);
            if (a.encoding == SK_AIFF_IMA4) {
                sk::AiffImaStream st{};
                st.first_unit = (uint32_t)ima_units.size(), st.n_units = a.n_units, st.channels = a.channels;
                for (int c = 0; c < 2; ++c) st.predictor[c] = a.ima_state[c].predictor, st.step_index[c] = a.ima_state[c].step_index;
                imas.push_back(st);
                ima_of.push_back(i);
            }
            for (uint32_t u = 0; u < a.n_units; ++u) {
                const sk_pcm_unit &un = aiff->src_units[pc[i].first + u];
                if (a.encoding == SK_AIFF_IMA4) {
                    ima_units.push_back(sk::AiffImaUnit{d_src + un.byte_offset, dst_of(i, u), (uint32_t)(un.byte_len / group), 0});
                } else {
                    const uint32_t samples = (uint32_t)(un.byte_len / group) * sk_pcm::aiff_group_samples(a.encoding);
                    elems.push_back(sk::AiffElemJob{d_src + un.byte_offset, dst_of(i, u), samples, a.encoding});
                    max_samples = std::max(max_samples, samples);
                }
            }
        }
        if (!elems.empty()) {
            const sk::AiffElemJob *d_jobs = nullptr;
            SK_HIP(aux.put(elems, e->stream, &d_jobs), "upload tick aiff jobs");
            SK_HIP(sk::launch_aiff_elem(d_jobs, (uint32_t)elems.size(), max_samples, e->stream), "tick aiff decode");
        }
        if (!imas.empty()) {
            const sk::AiffImaStream *d_streams = nullptr;
            const sk::AiffImaUnit *d_units = nullptr;
            uint32_t *d_states = nullptr;
            const std::vector<uint32_t> zeros(imas.size() * 2, 0);
            SK_HIP(aux.put(imas, e->stream, &d_streams), "upload tick aiff ima4 streams");
            SK_HIP(aux.put(ima_units, e->stream, &d_units), "upload tick aiff ima4 units");
            SK_HIP(aux.put_rw(zeros, e->stream, &d_states), "upload tick aiff ima4 states");
            SK_HIP(sk::launch_aiff_ima4(d_streams, (uint32_t)imas.size(), d_units, d_states, e->stream), "tick aiff ima4 decode");
            // the states come back through the arena's pinned mirror; they are read behind the tick's last wait
            const uint32_t *h_states = (const uint32_t *)(aux.host + ((const uint8_t *)d_states - aux.base));
            SK_HIP(hipMemcpyAsync((void *)h_states, d_states, zeros.size() * 4, hipMemcpyDeviceToHost, e->stream), "D2H tick aiff ima4 states");
            aiff_states.push_back({h_states, std::move(ima_of)});
        }
        return SK_OK;
    };
    if (aiff) {
        SK_HIP(e->tick_aiff.reserve(aiff->decoded_len + 64), "alloc tick aiff decoded");
        uint8_t *d_dec = (uint8_t *)e->tick_aiff.p;
        rc = aiff_decode(false, [&](uint32_t i, uint32_t u) { return d_dec + units[pc[i].first + u].byte_offset; });
        if (rc != SK_OK) return rc;
        d_in = d_dec;
    }

    // ---- streaming resamplers: k_pcm_ingest in the place of the row copies ----
    float *d_res = nullptr;
    if (!calls.empty()) {
        SK_HIP(e->tick_res.reserve(res_rows * res_stride * 4 + 16), "alloc tick resampler output");
        d_res = (float *)e->tick_res.p;
        std::vector<sk::PcmIngestJob> jobs;
        std::vector<sk::PcmWideIngestJob> wide_jobs;  // sources of more than two channels
        uint32_t max_samples = 0, max_wide_frames = 0;
        RsRounds rounds;
        rounds.total_in = [&](size_t ci) { return pc[call_stream[ci]].total_frames; };
        rounds.append = [&](size_t ci, uint32_t take, uint32_t fill) {
            const uint32_t i = call_stream[ci];
            PcmCall &c = pc[i];
            uint32_t taken = 0;
            while (take) {
                const sk_pcm_unit &un = units[c.first + c.unit];
                const uint32_t left = un.byte_len / c.frame_bytes - c.within;
                uint32_t n = std::min(take, left);
                // a unit that does not fit is cut where its next piece starts 16-byte aligned again (c.within stays a multiple of kPcmCutFrames)
                if (n < left) n &= ~(sk::kPcmCutFrames - 1);
                if (n == 0) break;
                const uint8_t *src = d_in + un.byte_offset + (size_t)c.within * c.frame_bytes;
                float *row = e->d_rs + rs_row0(e, calls[ci].id) * kRsRow + kRsBase + kRsHist + fill;
                if (ts[i].channels > SK_MAX_CHANNELS) {
                    sk::PcmWideIngestJob j{};
                    j.src = src, j.dst = row, j.row_stride = kRsRow, j.frames = n, j.fmt = ts[i].format, j.ch = ts[i].channels;
                    wide_jobs.push_back(j);
                    max_wide_frames = std::max(max_wide_frames, n);
                } else {
                    sk::PcmIngestJob j{};
                    j.src = src;
                    j.dst0 = row;
                    j.dst1 = j.dst0 + kRsRow;
                    j.frames = n;
                    j.fmt = ts[i].format;
                    j.ch = ts[i].channels;
                    jobs.push_back(j);
                    max_samples = std::max(max_samples, n * ts[i].channels);
                }
                fill += n, taken += n, take -= n;
                c.within += n;
                if (n != left) break;  // the rest of this unit goes down in the next round
                c.unit += 1, c.within = 0;
            }
            return taken;
        };
        rounds.launch = [&]() -> int {
            if (!jobs.empty()) {
                const sk::PcmIngestJob *d_jobs = nullptr;
                SK_HIP(aux.put(jobs, e->stream, &d_jobs), "upload tick pcm ingest jobs");
                SK_HIP(sk::launch_pcm_ingest(d_jobs, (uint32_t)jobs.size(), max_samples, e->stream), "tick pcm ingest");
                jobs.clear();
                max_samples = 0;
            }
            if (!wide_jobs.empty()) {
                const sk::PcmWideIngestJob *d_jobs = nullptr;
                SK_HIP(aux.put(wide_jobs, e->stream, &d_jobs), "upload tick pcm wide ingest jobs");
                SK_HIP(sk::launch_pcm_wide_ingest(d_jobs, (uint32_t)wide_jobs.size(), max_wide_frames, e->stream), "tick pcm wide ingest");
                wide_jobs.clear();
                max_wide_frames = 0;
            }
            return SK_OK;
        };
        rounds.flush = [&](size_t ci) { return ts[call_stream[ci]].flush != 0; };
        rounds.chunks = [&](size_t ci) -> std::vector<std::pair<uint32_t, uint32_t>> & { return pc[call_stream[ci]].chunks; };
        rounds.sub = [](int) {};
        rc = rs_run_rounds(e, calls, d_res, res_stride, res_cap, aux, rounds);
        if (rc != SK_OK) return rc;
    }

    // ---- output records, and the jobs that fill them ----
    e->where.store("tick (pcm): direct conversion, pack");
    std::vector<sk::PcmDirectJob> directs;
    std::vector<sk::PackJob> packs;
    // sources of more than two channels: every downmix without a rate change, and every pack behind the resampler rounds.  A job whose
    // output is the stereo branch's owns a word of `peaks`, zeroed with the upload, for the first of its two launches.
    std::vector<sk::WideJob> wides[2];  // [0] planar rows in (the pack), [1] interleaved bytes in (the direct conversion)
    uint32_t n_peaks = 0, n_wide_peaks[2] = {0, 0}, max_wide_frames[2] = {0, 0};
    uint32_t n_rec = 0, max_pack_frames = 0, max_direct_samples = 0;
    size_t cursor = 0;
    uint8_t *d_out = nullptr;
    auto emit = [&](uint32_t stream_index, uint32_t frames, const PcmCall &c, uint32_t bits) -> sk_tick_output * {
        if (n_rec >= outs_cap) return nullptr;
        sk_tick_output &o = outs[n_rec++];
        o.stream_index = stream_index;
        o.frames = frames;
        o.channels = (uint8_t)c.ch_out;
        o.bits = (uint8_t)bits;
        o.reserved = c.float_out ? SK_TICK_OUT_FLOAT : 0;
        o.status = 0;
        o.bytes = frames * c.ch_out * (bits / 8);
        o.byte_offset = cursor;
        cursor += ((size_t)o.bytes + 15) & ~(size_t)15;
        return &o;
    };
    std::vector<uint64_t> aiff_out(aiff ? n_units : 0, 0);  // AIFF streams delivered as decoded: where each unit's record lies in d_out
    // first pass sizes the output, second creates the jobs (the device buffer may move when it grows)
    for (int pass = 0; pass < 2; ++pass) {
        n_rec = 0;
        cursor = 0;
        n_peaks = 0;
        n_wide_peaks[0] = n_wide_peaks[1] = 0;
        for (uint32_t i = 0; i < n_streams; ++i) {
            const sk_pcm_tick_stream &t = ts[i];
            const PcmCall &c = pc[i];
            const bool wide = t.channels > SK_MAX_CHANNELS;
            auto wide_job = [&](const void *src, uint64_t src_stride, uint8_t fmt_in, sk_tick_output *o, uint32_t frames) {
                sk::WideJob j{};
                j.src = src, j.src_stride = src_stride, j.dst = d_out + o->byte_offset, j.frames = frames;
                j.fmt_in = fmt_in, j.fmt_out = c.fmt_out, j.ch_in = t.channels, j.ch_out = (uint8_t)c.ch_out;
                const int kind = fmt_in != sk::kWidePlanar;
                j.peak = sk::kWideNoPeak;
                if (c.ch_out == 2) j.peak = n_peaks++, n_wide_peaks[kind] += 1;
                wides[kind].push_back(j);
                max_wide_frames[kind] = std::max(max_wide_frames[kind], frames);
            };
            if (aiff && aiff->plain[i]) {  // the decode writes these records itself, behind the passes
                for (uint32_t u = 0; u < t.n_units; ++u) {
                    const uint32_t len = units[c.first + u].byte_len;
                    sk_tick_output *o = emit(i, len / c.frame_bytes, c, t.out_bits);
                    if (!o) return SK_ERR_INVALID_ARG;
                    cursor += (((size_t)len + 15) & ~(size_t)15) - (((size_t)o->bytes + 15) & ~(size_t)15);  // every sample of the unit, a last incomplete frame included
                    o->bytes = len;
                    if (pass) aiff_out[c.first + u] = o->byte_offset;
                }
            } else if (!t.resample) {
                for (uint32_t u = 0; u < t.n_units; ++u) {
                    const sk_pcm_unit &un = units[c.first + u];
                    const uint32_t frames = un.byte_len / c.frame_bytes;
                    sk_tick_output *o = emit(i, frames, c, t.out_bits);
                    if (!o) return SK_ERR_INVALID_ARG;
                    if (pass && wide && c.ch_out < t.channels) {
                        wide_job(d_in + un.byte_offset, 0, t.format, o, frames);
                    } else if (pass) {
                        sk::PcmDirectJob j{};
                        j.src = d_in + un.byte_offset;
                        j.dst = d_out + o->byte_offset;
                        j.frames = frames;
                        j.fmt_in = t.format, j.fmt_out = c.fmt_out, j.ch_in = t.channels, j.ch_out = (uint8_t)c.ch_out;
                        j.exact = c.exact ? 1 : 0;
                        directs.push_back(j);
                        max_direct_samples = std::max(max_direct_samples, frames * t.channels);
                    }
                }
            } else {
                const RsCall &rs = calls[(size_t)c.rs_call];
                for (const auto &chunk : c.chunks) {
                    sk_tick_output *o = emit(i, chunk.second, c, t.out_bits);
                    if (!o) return SK_ERR_INVALID_ARG;
                    if (pass && wide) {
                        wide_job(d_res + rs.row0 * res_stride + chunk.first, res_stride, sk::kWidePlanar, o, chunk.second);
                    } else if (pass) {
                        const float *src = d_res + rs.row0 * res_stride + chunk.first;
                        packs.push_back(sk::PackJob{src, src + res_stride, d_out + o->byte_offset, chunk.second, t.channels, (uint8_t)c.ch_out, t.out_bits,
                                                    (uint8_t)(c.float_out ? sk::kPackPlainF32 : sk::kPackPlain)});
                        max_pack_frames = std::max(max_pack_frames, chunk.second);
                    }
                }
            }
        }
        if (pass == 0) {
            if (cursor > out_cap || (cursor && !out)) return SK_ERR_INVALID_ARG;
            SK_HIP(e->tick_out.reserve(cursor + 16), "alloc tick output");
            d_out = (uint8_t *)e->tick_out.p;
        }
    }
    if (aiff) {
        rc = aiff_decode(true, [&](uint32_t i, uint32_t u) { return d_out + aiff_out[pc[i].first + u]; });
        if (rc != SK_OK) return rc;
    }
    if (!directs.empty()) {
        const sk::PcmDirectJob *d_jobs = nullptr;
        SK_HIP(aux.put(directs, e->stream, &d_jobs), "upload tick pcm direct jobs");
        SK_HIP(sk::launch_pcm_direct(d_jobs, (uint32_t)directs.size(), max_direct_samples, e->stream), "tick pcm direct");
    }
    if (!packs.empty()) {
        const sk::PackJob *d_packs = nullptr;
        SK_HIP(aux.put(packs, e->stream, &d_packs), "upload pack jobs");
        SK_HIP(sk::launch_pack_jobs(d_packs, (uint32_t)packs.size(), max_pack_frames, e->stream), "launch pack");
    }
    if (!wides[0].empty() || !wides[1].empty()) {
        uint32_t *d_peaks = nullptr;
        const std::vector<uint32_t> zeros(n_peaks, 0);
        SK_HIP(aux.put_rw(zeros, e->stream, &d_peaks), "upload tick pcm wide peaks");
        for (int kind = 0; kind < 2; ++kind) {
            if (wides[kind].empty()) continue;
            const sk::WideJob *d_wides = nullptr;
            SK_HIP(aux.put(wides[kind], e->stream, &d_wides), "upload tick pcm wide jobs");
            SK_HIP(sk::launch_pcm_wide(d_wides, (uint32_t)wides[kind].size(), n_wide_peaks[kind], max_wide_frames[kind], kind == 1, d_peaks, e->stream),
                   "tick pcm wide");
        }
    }
    uint8_t *bounce = nullptr;
    if (cursor) {
        rc = tick_queue_d2h(e, out, d_out, cursor, &bounce);
        if (rc != SK_OK) return rc;
    }
    rc = wait_stream(e, "tick (pcm): waiting for the device at the end of the tick");
    if (rc != SK_OK) return rc;
    for (const auto &got : aiff_states)
        for (size_t k = 0; k < got.second.size(); ++k)
            aiff->states[2 * got.second[k]] = got.first[2 * k], aiff->states[2 * got.second[k] + 1] = got.first[2 * k + 1];
    if (bounce) std::memcpy(out, bounce, cursor);
    *n_outs = n_rec;
    if (out_bytes) *out_bytes = cursor;
    return SK_OK;
}

// tick_pcm_body under the engine's lock; the resamplers' host bookkeeping is put back when it fails, as tick_impl_locked does
int tick_pcm_impl(sk_engine *e, const sk_pcm_tick_stream *ts, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units, const uint8_t *bytes,
                  size_t bytes_len, uint8_t *out, size_t out_cap, sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes,
                  AiffTick *aiff = nullptr) {
    if (!e) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    TickWhere where(e);
    RsSaved saved;
    for (uint32_t i = 0; ts && i < n_streams; ++i)
        if (ts[i].resample) saved.add(e, ts[i].stream);
    const int rc = tick_pcm_body(e, ts, n_streams, units, n_units, bytes, bytes_len, out, out_cap, outs, outs_cap, n_outs, out_bytes, aiff);
    if (rc != SK_OK) {
        saved.restore(e);
        if (n_outs) *n_outs = 0;
        if (out_bytes) *out_bytes = 0;
        // whatever was queued before the failure must be off the stream before the caller reuses its buffers
        if (rc != SK_ERR_TIMEOUT) (void)hipStreamSynchronize(e->stream);
    }
    return rc;
}

// sk_tick_run_aiff / sk_tick_aiff_out_bound_on: checks the AIFF table and derives what the PCM tick's body works on -- per stream a
// little-endian source of the contract's format, per unit where its decoded PCM lies (16-byte aligned, unit after unit).
struct AiffDerived {
    std::vector<sk_pcm_tick_stream> ts;
    std::vector<sk_pcm_unit> units;
    AiffTick tick;
};
int aiff_tick_derive(const sk_aiff_tick_stream *as, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units, size_t bytes_len, AiffDerived &d) {
    d.ts.assign(n_streams, sk_pcm_tick_stream{});
    d.units.assign(n_units, sk_pcm_unit{});
    d.tick.as = as, d.tick.src_units = units;
    d.tick.plain.assign(n_streams, 0);
    d.tick.states.assign((size_t)n_streams * 2, 0);
    uint64_t at = 0, cursor = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        const sk_aiff_tick_stream &a = as[i];
        if (!sk_pcm::aiff_encoding_known(a.encoding) || a.channels == 0 || a.channels > sk_pcm::kMaxAiffChannels) return SK_ERR_INVALID_ARG;
        if (a.encoding == SK_AIFF_IMA4 && (a.channels > 2 || a.ima_state[0].step_index > 88 || a.ima_state[1].step_index > 88)) return SK_ERR_INVALID_ARG;
        const uint32_t bits = sk_pcm::aiff_contract_bits(a.encoding);
        sk_pcm_tick_stream &t = d.ts[i];
        t.stream = a.stream, t.n_units = a.n_units, t.channels = a.channels, t.out_bits = a.out_bits, t.out_channels = a.out_channels;
        t.resample = a.resample, t.flush = a.flush;
        t.format = (uint8_t)(sk_pcm::aiff_contract_float(a.encoding) ? SK_FMT_F32LE : (bits == 16 ? SK_FMT_S16LE : (bits == 24 ? SK_FMT_S24LE : SK_FMT_S32LE)));
        d.tick.plain[i] = !a.resample && a.out_bits == bits && a.out_channels == a.channels;
        if (at + a.n_units > n_units) return SK_ERR_INVALID_ARG;
        const uint64_t group = sk_pcm::aiff_group_bytes(a.encoding, a.channels), group_out = sk_pcm::aiff_group_out_bytes(a.encoding, a.channels);
        for (uint32_t u = 0; u < a.n_units; ++u) {
            const sk_pcm_unit &un = units[at + u];
            if (un.byte_offset % 16 || un.byte_len == 0 || un.byte_len % group) return SK_ERR_INVALID_ARG;
            if (un.byte_offset > bytes_len || un.byte_len > bytes_len - un.byte_offset) return SK_ERR_INVALID_ARG;
            const uint64_t decoded = un.byte_len / group * group_out;
            if (decoded > 0x7fffffffull) return SK_ERR_INVALID_ARG;
            d.units[at + u] = sk_pcm_unit{cursor, (uint32_t)decoded, 0};
            cursor += (decoded + 15) & ~15ull;
        }
        at += a.n_units;
    }
    d.tick.decoded_len = (size_t)cursor;
    return at == n_units ? SK_OK : SK_ERR_INVALID_ARG;
}

// sk_tick_run_mixed_md: the MP3 streams' units arrive as frames with main data (ts[i].n_frames = frames of stream i).  A first
// pass of k_mp3_entropy gives every frame's verdict (one synchronisation: a dropped frame changes its stream's unit count, which the
// tick's plan is made from); the frames that decode become the tick's granules, and the tick runs the stage a second time over them,
// straight into its integer rows and granule records (0.35 ms per 131 072 granule-channels each time, the main data uploaded once).
// The Layer I / II streams' frames (sk_tick_run_mixed_mpa) as the units tick_body plans with: per frame two entries (Layer I: one) for
// the end of the granule / desc arrays, and per stream its unit count.  Every record is checked here; one that does not add up fails the call.
struct TickMpaBuild {
    TickMpa m;
    std::vector<sk_mp3_requant_granule> granules;
    std::vector<sk_mp3_granule_desc> descs;
    std::vector<uint32_t> units_of;  // per entry of ts (0 for the other codecs)
};
int mpa_build(const sk_tick_stream *ts, uint32_t n_streams, const sk_tick_mpa_frames *mpa, TickMpaBuild &b) {
    uint64_t listed = 0;
    for (uint32_t i = 0; i < n_streams; ++i)
        if (ts[i].codec == SK_TICK_MPA) listed += ts[i].n_frames;
    const uint32_t n = mpa ? mpa->n_frames : 0;
    if (listed != n) return SK_ERR_INVALID_ARG;
    b.units_of.assign(n_streams, 0);
    if (n == 0) return SK_OK;
    if (!mpa->records || !mpa->frame_bytes || mpa->bytes_len > (1u << 28)) return SK_ERR_INVALID_ARG;
    b.m.bytes = mpa->frame_bytes, b.m.bytes_len = mpa->bytes_len;
    uint32_t at = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        if (ts[i].codec != SK_TICK_MPA) continue;
        for (uint32_t k = 0; k < ts[i].n_frames; ++k, ++at) {
            const sk_mpa_frame_record &r = mpa->records[at];
            if (!sk_mp12::record_adds_up(r) || (r.byte_offset & 3u) || (uint64_t)r.byte_offset + r.byte_len + 8 > mpa->bytes_len) return SK_ERR_INVALID_ARG;
            b.m.records.push_back(r);
            b.m.stream.push_back(ts[i].stream);
            b.m.first_unit.push_back((uint32_t)b.m.unit_len.size());
            const uint32_t units = r.layer == 1 ? 1 : 2;
            for (uint32_t u = 0; u < units; ++u) {
                sk_mp3_requant_granule g;
                std::memset(&g, 0, sizeof g);
                g.sample_rate = r.sample_rate, g.channels = r.channels;
                sk_mp3_granule_desc d;
                std::memset(&d, 0, sizeof d);
                d.stream = ts[i].stream, d.channels = r.channels;
                b.granules.push_back(g);
                b.descs.push_back(d);
                b.m.unit_len.push_back(r.layer == 1 ? 384 : 576);
            }
            b.units_of[i] += units;
        }
    }
    return SK_OK;
}

int tick_impl_md(sk_engine *e, const sk_tick_stream *ts, uint32_t n_streams, const sk_tick_input *in, const sk_tick_mp3_frames *md, uint8_t *out,
                 size_t out_cap, sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes, const TickMpaBuild *mb = nullptr) {
    if (!e || !in || !md || !n_outs || (n_streams && !ts) || (md->n_frames && (!md->frames || !md->main_bytes))) return SK_ERR_INVALID_ARG;
    if (in->n_mp3_granules || in->mp3_granules || in->mp3_is) return SK_ERR_INVALID_ARG;  // the MP3 units in ONE form
    const uint32_t n = md->n_frames;
    uint64_t rows_all = 0, listed = 0;
    int rc = mp3_check_frames(md->frames, n, md->main_len, &rows_all);
    if (rc != SK_OK) return rc;
    for (uint32_t i = 0; i < n_streams; ++i)
        if (ts[i].codec == SK_TICK_MP3) listed += ts[i].n_frames;
    if (listed != n) return SK_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i)
        if (md->frames[i].header.channels != md->frames[i].side.channels || md->frames[i].header.granules != md->frames[i].side.granules) return SK_ERR_INVALID_ARG;
    const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lock(e->mu);
    const std::chrono::steady_clock::time_point t_locked = std::chrono::steady_clock::now();
    std::chrono::steady_clock::time_point t_queued = t_locked;
    std::vector<int32_t> cell_status((size_t)n * 4);
    if (n) {
        DeviceGuard guard(e);
        std::vector<uint32_t> first_row(n);
        uint32_t row = 0;
        for (uint32_t i = 0; i < n; ++i) first_row[i] = row, row += (uint32_t)md->frames[i].side.granules * md->frames[i].side.channels;
        SK_HIP(e->tick_mp3_in.reserve((size_t)rows_all * 576 * sizeof(int16_t) + 16), "alloc tick mp3 quantised lines");
        Mp3EntropyOut eo;
        rc = mp3_entropy_launch(e, md->frames, n, md->main_bytes, md->main_len, (int16_t *)e->tick_mp3_in.p, first_row.data(), nullptr, nullptr, &eo);
        if (rc != SK_OK) return rc;
        t_queued = std::chrono::steady_clock::now();
        SK_HIP(hipMemcpyAsync(cell_status.data(), eo.status, cell_status.size() * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream), "D2H tick mp3 entropy statuses");
        SK_HIP(hipStreamSynchronize(e->stream), "tick mp3 entropy sync");
    }
    const std::chrono::steady_clock::time_point t_verdicts = std::chrono::steady_clock::now();
    // the frames that decode, as the granules sk_tick_run_mixed takes (what comes from the side information; the stage fills in the rest)
    std::vector<sk_tick_stream> kept_ts(ts, ts + n_streams);
    std::vector<sk_mp3_frame_item> kept;
    std::vector<uint32_t> first_row, first_record;
    std::vector<sk_mp3_requant_granule> granules;
    std::vector<sk_mp3_granule_desc> descs;
    uint32_t at = 0, row = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        if (ts[i].codec != SK_TICK_MP3) continue;
        uint32_t units = 0;
        for (uint32_t k = 0; k < ts[i].n_frames; ++k, ++at) {
            const sk_mp3_frame_item &f = md->frames[at];
            bool ok = true;
            for (int gr = 0; gr < f.side.granules; ++gr)
                for (int ch = 0; ch < f.side.channels; ++ch) ok = ok && cell_status[(size_t)at * 4 + gr * 2 + ch] == SK_OK;
            if (!ok) continue;  // dropped as the host path drops it: no unit, no output record, the stream goes on
            kept.push_back(f);
            first_row.push_back(row);
            first_record.push_back((uint32_t)granules.size());
            const bool joint = f.header.mode == 1;
            for (int gr = 0; gr < f.side.granules; ++gr) {
                sk_mp3_requant_granule g;
                std::memset(&g, 0, sizeof g);
                g.sample_rate = f.header.sample_rate;
                g.channels = f.side.channels;
                g.ms_stereo = joint && (f.header.mode_ext & 2);
                g.intensity_stereo = joint && (f.header.mode_ext & 1);
                g.lsf = f.header.version != 1;
                if (g.lsf && g.intensity_stereo && f.side.channels == 2 && (f.side.gr[gr][1].scalefac_compress & 1)) g.intensity_stereo |= 2;
                sk_mp3_granule_desc d;
                std::memset(&d, 0, sizeof d);
                d.stream = ts[i].stream;
                d.channels = f.side.channels;
                for (int ch = 0; ch < f.side.channels; ++ch) {
                    const sk_mp3_granule_side &gs = f.side.gr[gr][ch];
                    sk_mp3_requant_channel &c = g.ch[ch];
                    c.global_gain = gs.global_gain, c.scalefac_scale = gs.scalefac_scale, c.preflag = g.lsf ? 0 : gs.preflag;
                    c.block_type = gs.block_type, c.mixed_block_flag = gs.mixed_block_flag;
                    std::memcpy(c.subblock_gain, gs.subblock_gain, 3);
                    d.block_type[ch] = gs.block_type, d.mixed_block_flag[ch] = gs.mixed_block_flag;
                }
                granules.push_back(g);
                descs.push_back(d);
                row += f.side.channels;
                units += 1;
            }
        }
        kept_ts[i].n_frames = units;
    }
    static const bool trace = std::getenv("SK_TICK_TRACE") != nullptr;
    if (trace) {
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        std::fprintf(stderr, "sk_tick: mp3 huffman stage in the tick: %u frames, %u dropped | lock %.2f  upload+queue %.2f  verdicts %.2f  granules %.2f ms\n", n,
                     n - (uint32_t)kept.size(), ms(t_begin, t_locked), ms(t_locked, t_queued), ms(t_queued, t_verdicts), ms(t_verdicts, std::chrono::steady_clock::now()));
    }
    TickMp3Frames frames_form;
    frames_form.frames = kept.data(), frames_form.n = (uint32_t)kept.size(), frames_form.main_len = md->main_len;
    frames_form.first_row = first_row.data(), frames_form.first_record = first_record.data();
    TickMp3 mp3;
    if (mb && !mb->granules.empty()) {  // the Layer I / II units go behind the granules
        granules.insert(granules.end(), mb->granules.begin(), mb->granules.end());
        descs.insert(descs.end(), mb->descs.begin(), mb->descs.end());
        for (uint32_t i = 0; i < n_streams; ++i)
            if (ts[i].codec == SK_TICK_MPA) kept_ts[i].n_frames = mb->units_of[i];
        mp3.n_mpa_units = (uint32_t)mb->granules.size();
        mp3.mpa = &mb->m;
    }
    mp3.granules = granules.data(), mp3.descs = descs.data(), mp3.n = (uint32_t)granules.size();
    mp3.md = &frames_form;
    return tick_impl_locked(e, kept_ts.data(), n_streams, in->descs, in->coeffs, in->units, in->au_bytes, in->au_bytes_len, in->n_aac_units, out, out_cap, outs,
                            outs_cap, n_outs, out_bytes, nullptr, (const uint8_t *)in->q_sides, in->q_quant, mp3);
}

// Every mixed form of the tick: sk_tick_run_mixed (md and mpa null), sk_tick_run_mixed_md (mpa null), sk_tick_run_mixed_mpa.
int tick_mixed(sk_engine *e, const sk_tick_stream *ts, uint32_t n_streams, const sk_tick_input *in, const sk_tick_mp3_frames *md,
               const sk_tick_mpa_frames *mpa, uint8_t *out, size_t out_cap, sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs,
               size_t *out_bytes) {
    if (!in || (n_streams && !ts)) return SK_ERR_INVALID_ARG;
    const int forms = (in->coeffs ? 1 : 0) + (in->units ? 1 : 0) + (in->q_sides ? 1 : 0);
    if (forms > 1 || (in->n_aac_units && forms == 0)) return SK_ERR_INVALID_ARG;  // the AAC units in ONE form
    if (in->q_sides && in->n_aac_units && (!in->q_quant || !in->descs)) return SK_ERR_INVALID_ARG;
    TickMpaBuild mb;
    const int rc = mpa_build(ts, n_streams, mpa, mb);
    if (rc != SK_OK) return rc;
    if (md) return tick_impl_md(e, ts, n_streams, in, md, out, out_cap, outs, outs_cap, n_outs, out_bytes, &mb);
    TickMp3 mp3;
    if (mb.granules.empty()) {  // no Layer I / II frames: the caller's arrays as they are
        mp3.granules = in->mp3_granules, mp3.descs = in->mp3_descs, mp3.is = in->mp3_is, mp3.n = in->n_mp3_granules;
        for (uint32_t g = 0; g < mp3.n && mp3.granules; ++g)
            if (mp3.granules[g].channels < 1 || mp3.granules[g].channels > 2) return SK_ERR_INVALID_ARG;
        return tick_impl(e, ts, n_streams, in->descs, in->coeffs, in->units, in->au_bytes, in->au_bytes_len, in->n_aac_units, out, out_cap, outs, outs_cap,
                         n_outs, out_bytes, nullptr, (const uint8_t *)in->q_sides, in->q_quant, mp3);
    }
    // the Layer III granules as `in` brings them, the Layer I / II units behind them
    if (in->n_mp3_granules && (!in->mp3_granules || !in->mp3_descs)) return SK_ERR_INVALID_ARG;
    for (uint32_t g = 0; g < in->n_mp3_granules; ++g)
        if (in->mp3_granules[g].channels < 1 || in->mp3_granules[g].channels > 2) return SK_ERR_INVALID_ARG;
    std::vector<sk_mp3_requant_granule> granules(in->mp3_granules, in->mp3_granules + in->n_mp3_granules);
    std::vector<sk_mp3_granule_desc> descs(in->mp3_descs, in->mp3_descs + in->n_mp3_granules);
    granules.insert(granules.end(), mb.granules.begin(), mb.granules.end());
    descs.insert(descs.end(), mb.descs.begin(), mb.descs.end());
    std::vector<sk_tick_stream> units_ts(ts, ts + n_streams);  // a Layer I / II stream's units are counted from its frames
    for (uint32_t i = 0; i < n_streams; ++i)
        if (ts[i].codec == SK_TICK_MPA) units_ts[i].n_frames = mb.units_of[i];
    mp3.granules = granules.data(), mp3.descs = descs.data(), mp3.is = in->mp3_is, mp3.n = (uint32_t)granules.size();
    mp3.n_mpa_units = (uint32_t)mb.granules.size();
    mp3.mpa = &mb.m;
    return tick_impl(e, units_ts.data(), n_streams, in->descs, in->coeffs, in->units, in->au_bytes, in->au_bytes_len, in->n_aac_units, out, out_cap, outs,
                     outs_cap, n_outs, out_bytes, nullptr, (const uint8_t *)in->q_sides, in->q_quant, mp3);
}

}  // namespace

extern "C" {

int sk_tick_run(sk_engine *e, const sk_tick_stream *ts, uint32_t n_streams, const sk_aac_frame_desc *descs,
                const float *coeffs, uint32_t n_frames, uint8_t *out, size_t out_cap, sk_tick_output *outs,
                uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes) try {
    sk::abi_enter();
    return tick_impl(e, ts, n_streams, descs, coeffs, nullptr, nullptr, 0, n_frames, out, out_cap, outs, outs_cap, n_outs, out_bytes);
} catch (...) {
    return sk::abi_caught("sk_tick_run");
}

int sk_tick_run_q(sk_engine *e, const sk_tick_stream *ts, uint32_t n_streams, const sk_aac_frame_desc *descs, const void *sides,
                  const int16_t *quant, uint32_t n_units, uint8_t *out, size_t out_cap, sk_tick_output *outs, uint32_t outs_cap,
                  uint32_t *n_outs, size_t *out_bytes) try {
    sk::abi_enter();
    if (n_units && (!sides || !quant || !descs)) return SK_ERR_INVALID_ARG;
    static const uint8_t none[8] = {0};
    return tick_impl(e, ts, n_streams, descs, nullptr, nullptr, nullptr, 0, n_units, out, out_cap, outs, outs_cap, n_outs, out_bytes, nullptr,
                     sides ? (const uint8_t *)sides : none, quant);
} catch (...) {
    return sk::abi_caught("sk_tick_run_q");
}

int sk_tick_run_mixed(sk_engine *e, const sk_tick_stream *ts, uint32_t n_streams, const sk_tick_input *in, uint8_t *out, size_t out_cap,
                      sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes) try {
    sk::abi_enter();
    return tick_mixed(e, ts, n_streams, in, nullptr, nullptr, out, out_cap, outs, outs_cap, n_outs, out_bytes);
} catch (...) {
    return sk::abi_caught("sk_tick_run_mixed");
}

int sk_tick_run_mixed_md(sk_engine *e, const sk_tick_stream *ts, uint32_t n_streams, const sk_tick_input *in, const sk_tick_mp3_frames *md, uint8_t *out,
                         size_t out_cap, sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes) try {
    sk::abi_enter();
    if (!md) return SK_ERR_INVALID_ARG;
    return tick_mixed(e, ts, n_streams, in, md, nullptr, out, out_cap, outs, outs_cap, n_outs, out_bytes);
} catch (...) {
    return sk::abi_caught("sk_tick_run_mixed_md");
}

int sk_tick_run_mixed_mpa(sk_engine *e, const sk_tick_stream *ts, uint32_t n_streams, const sk_tick_input *in, const sk_tick_mp3_frames *md,
                          const sk_tick_mpa_frames *mpa, uint8_t *out, size_t out_cap, sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs,
                          size_t *out_bytes) try {
    sk::abi_enter();
    return tick_mixed(e, ts, n_streams, in, md, mpa, out, out_cap, outs, outs_cap, n_outs, out_bytes);
} catch (...) {
    return sk::abi_caught("sk_tick_run_mixed_mpa");
}

size_t sk_tick_pcm_out_bound_on(sk_engine *e, const sk_pcm_tick_stream *ts, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units,
                                uint32_t *max_outputs) try {
    sk::abi_enter();
    if (max_outputs) *max_outputs = 0;
    if (!e || (!ts && n_streams) || (!units && n_units)) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return tick_pcm_out_bound(e, ts, n_streams, units, n_units, max_outputs);
} catch (...) {
    (void)sk::abi_caught("sk_tick_pcm_out_bound_on");
    return 0;
}

int sk_tick_run_pcm(sk_engine *e, const sk_pcm_tick_stream *ts, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units, const uint8_t *bytes,
                    size_t bytes_len, uint8_t *out, size_t out_cap, sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes) try {
    sk::abi_enter();
    return tick_pcm_impl(e, ts, n_streams, units, n_units, bytes, bytes_len, out, out_cap, outs, outs_cap, n_outs, out_bytes);
} catch (...) {
    return sk::abi_caught("sk_tick_run_pcm");
}

size_t sk_tick_aiff_out_bound_on(sk_engine *e, const sk_aiff_tick_stream *as, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units,
                                 uint32_t *max_outputs) try {
    sk::abi_enter();
    if (max_outputs) *max_outputs = 0;
    if (!e || (!as && n_streams) || (!units && n_units)) return 0;
    AiffDerived d;
    if (aiff_tick_derive(as, n_streams, units, n_units, (size_t)-1, d) != SK_OK) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return tick_pcm_out_bound(e, d.ts.data(), n_streams, d.units.data(), n_units, max_outputs, d.tick.plain.data());
} catch (...) {
    (void)sk::abi_caught("sk_tick_aiff_out_bound_on");
    return 0;
}

int sk_tick_run_aiff(sk_engine *e, sk_aiff_tick_stream *as, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units, const uint8_t *bytes,
                     size_t bytes_len, uint8_t *out, size_t out_cap, sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes) try {
    sk::abi_enter();
    if (!e || !n_outs || (n_streams && !as) || (n_units && (!units || !bytes))) return SK_ERR_INVALID_ARG;
    AiffDerived d;
    int rc = aiff_tick_derive(as, n_streams, units, n_units, bytes_len, d);
    if (rc != SK_OK) {
        *n_outs = 0;
        if (out_bytes) *out_bytes = 0;
        return rc;
    }
    rc = tick_pcm_impl(e, d.ts.data(), n_streams, d.units.data(), n_units, bytes, bytes_len, out, out_cap, outs, outs_cap, n_outs, out_bytes, &d.tick);
    if (rc != SK_OK) return rc;
    for (uint32_t i = 0; i < n_streams; ++i) {  // a failed call leaves the states as they were
        if (as[i].encoding != SK_AIFF_IMA4 || as[i].n_units == 0) continue;
        for (int c = 0; c < 2; ++c) {
            as[i].ima_state[c].predictor = (int16_t)(d.tick.states[2 * i + c] & 0xffff);
            as[i].ima_state[c].step_index = (uint8_t)(d.tick.states[2 * i + c] >> 16);
        }
    }
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_tick_run_aiff");
}

// one stream's bytes, one call: a table of one job in front of the same kernels
static int aiff_decode_one(sk_engine *e, int encoding, uint32_t channels, const uint8_t *bytes, bool on_device, size_t len, uint8_t *out, size_t out_cap,
                           size_t *out_len, sk_aiff_ima_state *state) {
    if (!e || !out_len || !sk_pcm::aiff_encoding_known(encoding) || channels == 0 || channels > sk_pcm::kMaxAiffChannels) return SK_ERR_INVALID_ARG;
    *out_len = 0;
    const bool ima = encoding == SK_AIFF_IMA4;
    if (ima && (channels > 2 || !state || state[0].step_index > 88 || state[1].step_index > 88)) return SK_ERR_INVALID_ARG;
    const size_t group = sk_pcm::aiff_group_bytes(encoding, channels), group_out = sk_pcm::aiff_group_out_bytes(encoding, channels);
    const uint32_t per_group = sk_pcm::aiff_group_samples(encoding);
    if (len % group || len / group > 0x7fffffffu / per_group || (len && (!bytes || !out))) return SK_ERR_INVALID_ARG;
    const size_t groups = len / group, need = groups * group_out;
    if (need > out_cap) return SK_ERR_INVALID_ARG;
    if (on_device && (((uintptr_t)bytes | (uintptr_t)out) & 15)) return SK_ERR_INVALID_ARG;
    if (groups == 0) return SK_OK;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    const size_t table_at = on_device ? 0 : (len + 15) & ~(size_t)15;
    SK_HIP(e->in_buf.reserve(table_at + 256), "alloc staging");
    const uint8_t *d_src = bytes;
    uint8_t *d_dst = out;
    if (!on_device) {
        SK_HIP(e->out_buf.reserve(need), "alloc staging");
        SK_HIP(hipMemcpyAsync(e->in_buf.p, bytes, len, hipMemcpyHostToDevice, e->stream), "H2D aiff");
        d_src = (const uint8_t *)e->in_buf.p, d_dst = (uint8_t *)e->out_buf.p;
    }
    uint8_t *table = (uint8_t *)e->in_buf.p + table_at;
    uint32_t got[2] = {0, 0};
    if (ima) {
        struct { sk::AiffImaStream st; sk::AiffImaUnit un; uint32_t states[2]; uint32_t pad[2]; } t{};
        t.st.first_unit = 0, t.st.n_units = 1, t.st.channels = (uint8_t)channels;
        for (int c = 0; c < 2; ++c) t.st.predictor[c] = state[c].predictor, t.st.step_index[c] = state[c].step_index;
        t.un = sk::AiffImaUnit{d_src, d_dst, (uint32_t)groups, 0};
        SK_HIP(hipMemcpyAsync(table, &t, sizeof t, hipMemcpyHostToDevice, e->stream), "H2D aiff ima4 table");
        SK_HIP(hipStreamSynchronize(e->stream), "aiff table sync");  // t leaves scope with this block
        SK_HIP(sk::launch_aiff_ima4((const sk::AiffImaStream *)table, 1, (const sk::AiffImaUnit *)(table + offsetof(decltype(t), un)),
                                    (uint32_t *)(table + offsetof(decltype(t), states)), e->stream), "launch aiff ima4");
        SK_HIP(hipMemcpyAsync(got, table + offsetof(decltype(t), states), sizeof got, hipMemcpyDeviceToHost, e->stream), "D2H aiff ima4 states");
    } else {
        const sk::AiffElemJob job{d_src, d_dst, (uint32_t)groups * per_group, (uint32_t)encoding};
        SK_HIP(hipMemcpyAsync(table, &job, sizeof job, hipMemcpyHostToDevice, e->stream), "H2D aiff job");
        SK_HIP(hipStreamSynchronize(e->stream), "aiff table sync");
        SK_HIP(sk::launch_aiff_elem((const sk::AiffElemJob *)table, 1, (uint32_t)groups * per_group, e->stream), "launch aiff decode");
    }
    if (!on_device) SK_HIP(hipMemcpyAsync(out, d_dst, need, hipMemcpyDeviceToHost, e->stream), "D2H aiff");
    SK_HIP(hipStreamSynchronize(e->stream), "aiff sync");
    if (ima)
        for (int c = 0; c < 2; ++c) state[c].predictor = (int16_t)(got[c] & 0xffff), state[c].step_index = (uint8_t)(got[c] >> 16);
    *out_len = need;
    return SK_OK;
}

int sk_aiff_decode(sk_engine *e, int encoding, uint32_t channels, const uint8_t *bytes, size_t len, uint8_t *out, size_t out_cap, size_t *out_len,
                   sk_aiff_ima_state *state) try {
    sk::abi_enter();
    return aiff_decode_one(e, encoding, channels, bytes, false, len, out, out_cap, out_len, state);
} catch (...) {
    return sk::abi_caught("sk_aiff_decode");
}

int sk_aiff_decode_dev(sk_engine *e, int encoding, uint32_t channels, const uint8_t *d_bytes, size_t len, uint8_t *d_out, size_t out_cap, size_t *out_len,
                       sk_aiff_ima_state *state) try {
    sk::abi_enter();
    return aiff_decode_one(e, encoding, channels, d_bytes, true, len, d_out, out_cap, out_len, state);
} catch (...) {
    return sk::abi_caught("sk_aiff_decode_dev");
}

// n_blocks x frames x channels s16 must stay a 31-bit byte count (keep_frames and the lane index are 32-bit)
static bool need_overflows(uint64_t n_blocks, uint32_t frames, uint32_t channels) { return n_blocks * frames * channels * 2 > 0x7fffffffull; }

// whole blocks of one WAV ADPCM stream, one call: a table of one job in front of k_wav_ima / k_wav_ms (wav_adpcm.hip)
static int wav_adpcm_decode_one(sk_engine *e, int tag, uint32_t channels, uint32_t block_align, const int16_t *coef, uint32_t n_coef, const uint8_t *bytes,
                                bool on_device, size_t len, uint8_t *out, size_t out_cap, size_t *out_len, int32_t *status) {
    static_assert(SK_WAV_BAD_BLOCK == sk::kWavAdpcmBadBlock, "the kernels' status is the header's");
    if (!e || !out_len) return SK_ERR_INVALID_ARG;
    *out_len = 0;
    if (tag != SK_WAV_TAG_IMA_ADPCM && tag != SK_WAV_TAG_MS_ADPCM) return SK_ERR_INVALID_ARG;
    const uint32_t frames = sk_pcm::wav_adpcm_block_frames((uint32_t)tag, channels, block_align);
    if (frames == 0 || frames > sk_pcm::kMaxWavAdpcmBlockFrames) return SK_ERR_INVALID_ARG;
    if (tag == SK_WAV_TAG_MS_ADPCM && (!coef || n_coef < 1 || n_coef > sk_pcm::kMaxWavAdpcmCoefs)) return SK_ERR_INVALID_ARG;
    if (len % block_align || need_overflows(len / block_align, frames, channels) || (len && (!bytes || !out || !status))) return SK_ERR_INVALID_ARG;
    const size_t n_blocks = len / block_align, need = n_blocks * frames * channels * 2;
    if (need > out_cap) return SK_ERR_INVALID_ARG;
    if (on_device && (((uintptr_t)bytes | (uintptr_t)out) & 15 || ((uintptr_t)status & 3))) return SK_ERR_INVALID_ARG;
    if (n_blocks == 0) return SK_OK;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    sk::WavAdpcmJob job{};
    job.src = bytes, job.dst = out, job.status = status;
    const size_t status_at = (need + 15) & ~(size_t)15;
    SK_HIP(e->wav_tab.reserve(sizeof job), "alloc wav adpcm job");
    if (!on_device) {
        SK_HIP(e->in_buf.reserve(len), "alloc staging");
        SK_HIP(e->out_buf.reserve(status_at + n_blocks * sizeof(int32_t)), "alloc staging");
        SK_HIP(hipMemcpyAsync(e->in_buf.p, bytes, len, hipMemcpyHostToDevice, e->stream), "H2D wav adpcm");
        job.src = (const uint8_t *)e->in_buf.p, job.dst = (uint8_t *)e->out_buf.p, job.status = (int32_t *)((uint8_t *)e->out_buf.p + status_at);
    }
    job.n_blocks = (uint32_t)n_blocks, job.block_align = block_align, job.frames_per_block = frames;
    job.keep_frames = (uint32_t)(n_blocks * frames);
    job.tag = (uint16_t)tag, job.channels = (uint8_t)channels;
    if (tag == SK_WAV_TAG_MS_ADPCM) {
        job.n_coef = (uint8_t)n_coef;
        std::memcpy(job.coef, coef, (size_t)n_coef * 2 * sizeof(int16_t));
    }
    SK_HIP(hipMemcpyAsync(e->wav_tab.p, &job, sizeof job, hipMemcpyHostToDevice, e->stream), "H2D wav adpcm job");
    SK_HIP(hipStreamSynchronize(e->stream), "wav adpcm job sync");  // job leaves scope with this call
    SK_HIP(sk::launch_wav_adpcm((const sk::WavAdpcmJob *)e->wav_tab.p, 1, tag == SK_WAV_TAG_IMA_ADPCM, (uint32_t)(n_blocks * channels), e->stream),
           "launch wav adpcm");
    if (!on_device) {
        SK_HIP(hipMemcpyAsync(out, job.dst, need, hipMemcpyDeviceToHost, e->stream), "D2H wav adpcm");
        SK_HIP(hipMemcpyAsync(status, job.status, n_blocks * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream), "D2H wav adpcm status");
        SK_HIP(hipStreamSynchronize(e->stream), "wav adpcm sync");
    }
    *out_len = need;
    return SK_OK;
}

int sk_wav_adpcm_decode(sk_engine *e, int tag, uint32_t channels, uint32_t block_align, const int16_t *coef, uint32_t n_coef, const uint8_t *bytes, size_t len,
                        uint8_t *out, size_t out_cap, size_t *out_len, int32_t *status_per_block) try {
    sk::abi_enter();
    return wav_adpcm_decode_one(e, tag, channels, block_align, coef, n_coef, bytes, false, len, out, out_cap, out_len, status_per_block);
} catch (...) {
    return sk::abi_caught("sk_wav_adpcm_decode");
}

int sk_wav_adpcm_decode_dev(sk_engine *e, int tag, uint32_t channels, uint32_t block_align, const int16_t *coef, uint32_t n_coef, const uint8_t *d_bytes,
                            size_t len, uint8_t *d_out, size_t out_cap, size_t *out_len, int32_t *d_status_per_block) try {
    sk::abi_enter();
    return wav_adpcm_decode_one(e, tag, channels, block_align, coef, n_coef, d_bytes, true, len, d_out, out_cap, out_len, d_status_per_block);
} catch (...) {
    return sk::abi_caught("sk_wav_adpcm_decode_dev");
}

// sk_tick_run_wav_adpcm / sk_tick_wav_adpcm_out_bound_on: checks the table and derives what the PCM tick's body works on, as
// aiff_tick_derive does -- per stream an s16le source, per unit where its decoded frames lie (16-byte aligned, unit after unit; a unit
// that the `fact` cap cuts is that much shorter) -- and the decode that stands in front of the body: one launch per tag and pass.
struct WavAdpcmDerived {
    std::vector<sk_pcm_tick_stream> ts;
    std::vector<sk_pcm_unit> units;     // the decoded layout
    std::vector<uint32_t> first;        // per stream: its first unit
    std::vector<uint32_t> frames;       // per unit: frames kept
    std::vector<uint32_t> block0;       // per unit: its first block's place in the status array
    std::vector<uint64_t> left_after;   // per stream: frames_left behind this tick
    std::vector<sk::WavAdpcmJob> jobs;  // as uploaded, pass after pass
    std::vector<int32_t> status;        // per block, read back behind the tick's last wait
    uint32_t n_blocks = 0;
    AiffTick tick;
};

static int wav_adpcm_tick_derive(const sk_wav_adpcm_tick_stream *ws, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units, size_t bytes_len,
                                 WavAdpcmDerived &d) {
    d.ts.assign(n_streams, sk_pcm_tick_stream{});
    d.units.assign(n_units, sk_pcm_unit{});
    d.first.assign(n_streams, 0);
    d.frames.assign(n_units, 0);
    d.block0.assign(n_units, 0);
    d.left_after.assign(n_streams, 0);
    d.tick.plain.assign(n_streams, 0);
    d.tick.states.assign((size_t)n_streams * 2, 0);
    uint64_t at = 0, cursor = 0, blocks = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        const sk_wav_adpcm_tick_stream &w = ws[i];
        if (w.tag != SK_WAV_TAG_IMA_ADPCM && w.tag != SK_WAV_TAG_MS_ADPCM) return SK_ERR_INVALID_ARG;
        const uint32_t per = sk_pcm::wav_adpcm_block_frames(w.tag, w.channels, w.block_align);
        if (per == 0 || per > sk_pcm::kMaxWavAdpcmBlockFrames || (w.frames_per_block && w.frames_per_block != per)) return SK_ERR_INVALID_ARG;
        if (w.tag == SK_WAV_TAG_MS_ADPCM && (w.n_coef < 1 || w.n_coef > sk_pcm::kMaxWavAdpcmCoefs)) return SK_ERR_INVALID_ARG;
        sk_pcm_tick_stream &t = d.ts[i];
        t.stream = w.stream, t.n_units = w.n_units, t.channels = w.channels, t.out_bits = w.out_bits, t.out_channels = w.out_channels;
        t.resample = w.resample, t.flush = w.flush, t.format = SK_FMT_S16LE;
        d.tick.plain[i] = !w.resample && w.out_bits == 16 && w.out_channels == w.channels;
        d.first[i] = (uint32_t)at;
        if (at + w.n_units > n_units) return SK_ERR_INVALID_ARG;
        uint64_t left = w.frames_left;
        for (uint32_t u = 0; u < w.n_units; ++u) {
            const sk_pcm_unit &un = units[at + u];
            if (un.byte_offset % 16 || un.byte_len == 0 || un.byte_len % w.block_align) return SK_ERR_INVALID_ARG;
            if (un.byte_offset > bytes_len || un.byte_len > bytes_len - un.byte_offset) return SK_ERR_INVALID_ARG;
            const uint64_t n_blocks = un.byte_len / w.block_align;
            if (need_overflows(n_blocks, per, w.channels)) return SK_ERR_INVALID_ARG;
            const uint64_t keep = std::min<uint64_t>(n_blocks * per, left);
            if (keep == 0) return SK_ERR_INVALID_ARG;  // a stream whose cap is used up has no more units
            if (left != UINT64_MAX) left -= keep;
            d.frames[at + u] = (uint32_t)keep, d.block0[at + u] = (uint32_t)blocks;
            d.units[at + u] = sk_pcm_unit{cursor, (uint32_t)(keep * w.channels * 2), 0};
            cursor += (keep * w.channels * 2 + 15) & ~15ull;
            blocks += n_blocks;
        }
        d.left_after[i] = left;
        at += w.n_units;
    }
    if (cursor > 0x7fffffffull || blocks > 0x3fffffffull) return SK_ERR_INVALID_ARG;
    d.tick.decoded_len = (size_t)cursor;
    d.n_blocks = (uint32_t)blocks;
    return at == n_units ? SK_OK : SK_ERR_INVALID_ARG;
}

// one pass of the decode in front of the body: the units of the streams whose `plain` is as_is, each to where dst_of puts it.
// wav_tab holds every unit's job (pass after pass) and behind them every block's status.
static int wav_adpcm_tick_decode(sk_engine *e, const sk_wav_adpcm_tick_stream *ws, const sk_pcm_unit *units, WavAdpcmDerived &d, bool as_is,
                                 const std::function<uint8_t *(uint32_t, uint32_t)> &dst_of, const uint8_t *d_src) {
    const size_t n_units = d.units.size(), status_at = (n_units * sizeof(sk::WavAdpcmJob) + 15) & ~(size_t)15;
    if (d.jobs.capacity() < n_units) {  // the first pass: both passes' room at once, so that nothing moves under a queued launch
        d.jobs.reserve(n_units);
        d.status.assign(d.n_blocks, 0);
        SK_HIP(e->wav_tab.reserve(status_at + (size_t)d.n_blocks * sizeof(int32_t) + 64), "alloc tick wav adpcm tables");
    }
    int32_t *d_status = (int32_t *)((uint8_t *)e->wav_tab.p + status_at);
    for (int ima = 0; ima < 2; ++ima) {
        const size_t begin = d.jobs.size();
        uint32_t max_lanes = 0;
        for (uint32_t i = 0; i < (uint32_t)d.ts.size(); ++i) {
            const sk_wav_adpcm_tick_stream &w = ws[i];
            if ((d.tick.plain[i] != 0) != as_is || (w.tag == SK_WAV_TAG_IMA_ADPCM) != (ima != 0)) continue;
            for (uint32_t u = 0; u < w.n_units; ++u) {
                const uint32_t g = d.first[i] + u;
                sk::WavAdpcmJob job{};
                job.src = d_src + units[g].byte_offset, job.dst = dst_of(i, u), job.status = d_status + d.block0[g];
                job.n_blocks = units[g].byte_len / w.block_align, job.block_align = w.block_align;
                job.frames_per_block = sk_pcm::wav_adpcm_block_frames(w.tag, w.channels, w.block_align);
                job.keep_frames = d.frames[g], job.tag = w.tag, job.channels = w.channels;
                if (!ima) {
                    job.n_coef = w.n_coef;
                    std::memcpy(job.coef, w.coef, (size_t)w.n_coef * 2 * sizeof(int16_t));
                }
                max_lanes = std::max(max_lanes, job.n_blocks * w.channels);
                d.jobs.push_back(job);
            }
        }
        const size_t n = d.jobs.size() - begin;
        if (n == 0) continue;
        sk::WavAdpcmJob *d_jobs = (sk::WavAdpcmJob *)e->wav_tab.p + begin;
        SK_HIP(hipMemcpyAsync(d_jobs, d.jobs.data() + begin, n * sizeof(sk::WavAdpcmJob), hipMemcpyHostToDevice, e->stream), "H2D tick wav adpcm jobs");
        SK_HIP(sk::launch_wav_adpcm(d_jobs, (uint32_t)n, ima != 0, max_lanes, e->stream), "tick wav adpcm decode");
    }
    // every block's status so far, read behind the tick's last wait (the second pass brings the whole array again, complete then)
    if (d.n_blocks) SK_HIP(hipMemcpyAsync(d.status.data(), d_status, (size_t)d.n_blocks * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream), "D2H tick wav adpcm status");
    return SK_OK;
}

size_t sk_tick_wav_adpcm_out_bound_on(sk_engine *e, const sk_wav_adpcm_tick_stream *ws, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units,
                                      uint32_t *max_outputs) try {
    sk::abi_enter();
    if (max_outputs) *max_outputs = 0;
    if (!e || (!ws && n_streams) || (!units && n_units)) return 0;
    WavAdpcmDerived d;
    if (wav_adpcm_tick_derive(ws, n_streams, units, n_units, (size_t)-1, d) != SK_OK) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return tick_pcm_out_bound(e, d.ts.data(), n_streams, d.units.data(), n_units, max_outputs, d.tick.plain.data());
} catch (...) {
    (void)sk::abi_caught("sk_tick_wav_adpcm_out_bound_on");
    return 0;
}

int sk_tick_run_wav_adpcm(sk_engine *e, sk_wav_adpcm_tick_stream *ws, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units, const uint8_t *bytes,
                          size_t bytes_len, uint8_t *out, size_t out_cap, sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes,
                          int32_t *status_per_unit) try {
    sk::abi_enter();
    if (!e || !n_outs || (n_streams && !ws) || (n_units && (!units || !bytes || !status_per_unit))) return SK_ERR_INVALID_ARG;
    *n_outs = 0;
    if (out_bytes) *out_bytes = 0;
    WavAdpcmDerived d;
    int rc = wav_adpcm_tick_derive(ws, n_streams, units, n_units, bytes_len, d);
    if (rc != SK_OK) return rc;
    d.tick.decode = [&](bool as_is, const std::function<uint8_t *(uint32_t, uint32_t)> &dst_of, const uint8_t *d_src) {
        return wav_adpcm_tick_decode(e, ws, units, d, as_is, dst_of, d_src);
    };
    rc = tick_pcm_impl(e, d.ts.data(), n_streams, d.units.data(), n_units, bytes, bytes_len, out, out_cap, outs, outs_cap, n_outs, out_bytes, &d.tick);
    if (rc != SK_OK) return rc;  // frames_left is the caller's record: untouched
    for (uint32_t i = 0; i < n_streams; ++i) {
        ws[i].frames_left = d.left_after[i];
        for (uint32_t u = 0; u < ws[i].n_units; ++u) {  // a unit's status: 0, or 1 + the index of its first block that its header rules out
            const uint32_t g = d.first[i] + u, n = units[g].byte_len / ws[i].block_align;
            status_per_unit[g] = 0;
            for (uint32_t b = 0; b < n && status_per_unit[g] == 0; ++b)
                if (d.status[d.block0[g] + b] != 0) status_per_unit[g] = (int32_t)(b + 1);
        }
    }
    // the records of a stream delivered as decoded correspond to its units; a unit with a bad block marks its record, or -- behind a
    // conversion, where records and units do not correspond -- every record of its stream in this tick
    std::vector<uint32_t> seen(n_streams, 0);
    for (uint32_t k = 0; k < *n_outs; ++k) {
        sk_tick_output &o = outs[k];
        const uint32_t i = o.stream_index;
        if (d.tick.plain[i]) {
            if (status_per_unit[d.first[i] + seen[i]++] != 0) o.status = SK_WAV_BAD_BLOCK;
        } else {
            for (uint32_t u = 0; u < ws[i].n_units && o.status == 0; ++u)
                if (status_per_unit[d.first[i] + u] != 0) o.status = SK_WAV_BAD_BLOCK;
        }
    }
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_tick_run_wav_adpcm");
}

int sk_aac_entropy_decode(sk_engine *e, const uint32_t *streams, const uint32_t *units_per_stream, uint32_t n_streams,
                          const sk_au_item *units, uint32_t n_units, const uint8_t *au_bytes, size_t au_bytes_len, float *coeffs_out,
                          sk_aac_frame_desc *descs_out, int32_t *status_out) try {
    sk::abi_enter();
    if (!e || (n_streams && (!streams || !units_per_stream)) || (n_units && (!units || !coeffs_out || !descs_out || !status_out)))
        return SK_ERR_INVALID_ARG;
    if (n_units == 0) return SK_OK;
    std::vector<sk_tick_stream> ts(n_streams);
    for (uint32_t i = 0; i < n_streams; ++i) ts[i] = sk_tick_stream{streams[i], units_per_stream[i], 16, 1, 0, 0};
    const EntropyProbe probe{coeffs_out, descs_out, status_out};
    uint32_t n_outs = 0;
    return tick_impl(e, ts.data(), n_streams, nullptr, nullptr, units, au_bytes, au_bytes_len, n_units, nullptr, 0, nullptr, 0, &n_outs,
                     nullptr, &probe);
} catch (...) {
    return sk::abi_caught("sk_aac_entropy_decode");
}

int sk_aac_expand_q_decode(sk_engine *e, const uint32_t *streams, const uint32_t *units_per_stream, uint32_t n_streams,
                           const sk_aac_frame_desc *descs, const void *sides, const int16_t *quant, uint32_t n_units, float *coeffs_out,
                           sk_aac_frame_desc *descs_out, int32_t *status_out) try {
    sk::abi_enter();
    if (!e || (n_streams && (!streams || !units_per_stream)) ||
        (n_units && (!descs || !sides || !quant || !coeffs_out || !descs_out || !status_out)))
        return SK_ERR_INVALID_ARG;
    if (n_units == 0) return SK_OK;
    std::vector<sk_tick_stream> ts(n_streams);
    for (uint32_t i = 0; i < n_streams; ++i) ts[i] = sk_tick_stream{streams[i], units_per_stream[i], 16, 1, 0, 0};
    const EntropyProbe probe{coeffs_out, descs_out, status_out};
    uint32_t n_outs = 0;
    return tick_impl(e, ts.data(), n_streams, descs, nullptr, nullptr, nullptr, 0, n_units, nullptr, 0, nullptr, 0, &n_outs, nullptr, &probe,
                     (const uint8_t *)sides, quant);
} catch (...) {
    return sk::abi_caught("sk_aac_expand_q_decode");
}

int sk_tick_run_au(sk_engine *e, const sk_tick_stream *ts, uint32_t n_streams, const sk_au_item *units, uint32_t n_units,
                   const uint8_t *au_bytes, size_t au_bytes_len, uint8_t *out, size_t out_cap, sk_tick_output *outs,
                   uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes) try {
    sk::abi_enter();
    if (n_units && !units) return SK_ERR_INVALID_ARG;
    static const sk_au_item none{};
    return tick_impl(e, ts, n_streams, nullptr, nullptr, units ? units : &none, au_bytes, au_bytes_len, n_units, out, out_cap, outs,
                     outs_cap, n_outs, out_bytes);
} catch (...) {
    return sk::abi_caught("sk_tick_run_au");
}

}  // extern "C"

// ---- FLAC (flac_stream.h, flac_decode.hip) ----------------------------------------------------------------------------------------

namespace {

inline uint32_t flac_width(uint32_t bits, uint32_t mode) {
    return mode == sk::kFlacOutI32 ? 4u : mode == sk::kFlacOutI16Clamp ? 2u : (bits <= 8 ? 1u : bits <= 16 ? 2u : bits <= 24 ? 3u : 4u);
}

// the three launches over every frame of a call; mode = how k_flac_output writes (the contract's bytes, i32, i16 clamped)
int flac_decode_frames(sk_engine *e, const sk_flac_frame_info *frames, uint32_t n, const uint8_t *bytes, bool on_device, uint8_t *out, size_t out_cap,
                       size_t *out_len, int32_t *status, uint32_t mode) {
    if (!e || !out_len || (n && (!frames || !bytes || !out || !status))) return SK_ERR_INVALID_ARG;
    *out_len = 0;
    if (n == 0) return SK_OK;
    std::vector<sk::FlacFrame> table(n);
    uint64_t need = 0, ws_words = 0, bytes_len = 0, n_subs = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const sk_flac_frame_info &f = frames[i];
        if (f.channels == 0 || f.channels > 8 || f.bits_per_sample < 4 || f.bits_per_sample > 32 || f.block_size == 0 || f.block_size > 65536 ||
            f.header_bytes < 6 || f.frame_bytes < (uint32_t)f.header_bytes + 3 || f.frame_bytes > (1u << 24))  // STREAMINFO counts a frame's bytes in 24 bits
            return SK_ERR_INVALID_ARG;
        sk::FlacFrame &t = table[i];
        t.byte_offset = f.offset, t.byte_len = f.frame_bytes, t.block_size = f.block_size, t.ws_offset = (uint32_t)ws_words;
        t.out_offset = need, t.sub0 = (uint32_t)n_subs;
        t.header_bytes = f.header_bytes, t.channels = f.channels, t.assignment = f.assignment, t.bits = f.bits_per_sample;
        need += (uint64_t)f.block_size * f.channels * flac_width(f.bits_per_sample, mode);
        ws_words += (uint64_t)f.block_size * f.channels;
        n_subs += f.channels;
        bytes_len = std::max<uint64_t>(bytes_len, (uint64_t)f.offset + f.frame_bytes);
        if (ws_words > 0x3fffffffu || bytes_len > 0x7fffffffu) return SK_ERR_INVALID_ARG;
    }
    if (need > out_cap) return SK_ERR_INVALID_ARG;
    if (on_device && (((uintptr_t)bytes | (uintptr_t)out) & 15)) return SK_ERR_INVALID_ARG;
    std::vector<uint32_t> by_length(n);
    for (uint32_t i = 0; i < n; ++i) by_length[i] = i;
    std::stable_sort(by_length.begin(), by_length.end(), [&](uint32_t a, uint32_t b) { return frames[a].frame_bytes > frames[b].frame_bytes; });

    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    // flac_in: [bytes (host form)] | frame table | order | statuses, each part 16-byte aligned
    const auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t at_table = on_device ? 0 : up16((size_t)bytes_len), at_order = at_table + up16(n * sizeof(sk::FlacFrame)),
                 at_status = at_order + up16(n * sizeof(uint32_t)), in_len = at_status + up16(n * sizeof(int32_t));
    const size_t at_subs = up16((size_t)ws_words * 4), ws_len = at_subs + (size_t)n_subs * sizeof(sk::FlacSubframe);
    SK_HIP(e->flac_in.reserve(in_len), "alloc flac input");
    SK_HIP(e->flac_ws.reserve(ws_len), "alloc flac workspace");
    uint8_t *d_in = (uint8_t *)e->flac_in.p, *d_ws = (uint8_t *)e->flac_ws.p, *d_out = out;
    const uint8_t *d_bytes = bytes;
    if (!on_device) {
        SK_HIP(e->flac_out.reserve((size_t)need), "alloc flac output");
        d_out = (uint8_t *)e->flac_out.p;
        SK_HIP(hipMemcpyAsync(d_in, bytes, (size_t)bytes_len, hipMemcpyHostToDevice, e->stream), "H2D flac frames");
        d_bytes = d_in;
    }
    SK_HIP(hipMemcpyAsync(d_in + at_table, table.data(), n * sizeof(sk::FlacFrame), hipMemcpyHostToDevice, e->stream), "H2D flac table");
    SK_HIP(hipMemcpyAsync(d_in + at_order, by_length.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream), "H2D flac order");
    // a record that no accepted frame wrote names no frame
    SK_HIP(hipMemsetAsync(d_ws + at_subs, 0xff, (size_t)n_subs * sizeof(sk::FlacSubframe), e->stream), "clear flac records");
    const sk::FlacFrame *d_table = (const sk::FlacFrame *)(d_in + at_table);
    sk::FlacSubframe *d_subs = (sk::FlacSubframe *)(d_ws + at_subs);
    int32_t *d_status = (int32_t *)(d_in + at_status);
    SK_HIP(sk::launch_flac_residual(d_table, (const uint32_t *)(d_in + at_order), n, d_bytes, (uint32_t)bytes_len, (int32_t *)d_ws, d_subs, d_status,
                                    e->stream), "launch flac residual");
    SK_HIP(sk::launch_flac_restore(d_subs, (uint32_t)n_subs, (int32_t *)d_ws, d_status, e->stream), "launch flac restore");
    SK_HIP(sk::launch_flac_output(d_table, n, d_subs, (const int32_t *)d_ws, d_status, d_out, mode, e->stream), "launch flac output");
    SK_HIP(hipMemcpyAsync(status, d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream), "D2H flac statuses");
    SK_HIP(hipStreamSynchronize(e->stream), "flac sync");  // table and by_length leave scope with the call
    if (!on_device) {
        // a rejected frame's place in the caller's buffer stays as it was: the accepted frames are copied one run at a time
        uint32_t i = 0;
        while (i < n) {
            if (status[i] != 0) {
                ++i;
                continue;
            }
            uint32_t j = i;
            while (j < n && status[j] == 0) ++j;
            const uint64_t from = table[i].out_offset, to = j < n ? table[j].out_offset : need;
            SK_HIP(hipMemcpyAsync(out + from, d_out + from, (size_t)(to - from), hipMemcpyDeviceToHost, e->stream), "D2H flac");
            i = j;
        }
        SK_HIP(hipStreamSynchronize(e->stream), "flac sync");
    }
    *out_len = (size_t)need;
    return SK_OK;
}

// sk_tick_run_flac / sk_tick_flac_out_bound_on: checks the table and derives what the PCM tick's body works on, as aiff_tick_derive does --
// per stream a little-endian source of the contract's format, per frame where its decoded PCM lies (16-byte aligned, frame after frame)
// -- and the decode that stands in front of the body: the three launches of flac_decode.hip over the frames of each pass.
struct FlacDerived {
    std::vector<sk_pcm_tick_stream> ts;
    std::vector<sk_pcm_unit> units;   // the decoded layout
    std::vector<uint32_t> first;      // per stream: its first frame
    AiffTick tick;
    // what the two passes (streams that go on through the body, streams delivered as decoded) upload and get back: alive until the
    // tick's last wait
    std::vector<sk::FlacFrame> table[2];
    std::vector<uint32_t> order[2], index[2];  // index: row of the table -> frame of the call
    std::vector<int32_t> status[2];
};

int flac_tick_derive(const sk_flac_tick_stream *fs, uint32_t n_streams, const sk_flac_frame_info *frames, uint32_t n_frames, size_t bytes_len,
                     FlacDerived &d) {
    d.ts.assign(n_streams, sk_pcm_tick_stream{});
    d.units.assign(n_frames, sk_pcm_unit{});
    d.first.assign(n_streams, 0);
    d.tick.plain.assign(n_streams, 0);
    d.tick.states.assign((size_t)n_streams * 2, 0);
    uint64_t at = 0, cursor = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        const sk_flac_tick_stream &f = fs[i];
        if (f.channels == 0 || f.channels > 8 || f.bits_per_sample < 4 || f.bits_per_sample > 32) return SK_ERR_INVALID_ARG;
        const uint32_t width = flac_width(f.bits_per_sample, sk::kFlacOutContract);
        const bool plain = !f.resample && f.out_bits == width * 8 && f.out_channels == f.channels;
        // anything to change: what sk_tick_run_pcm takes, i.e. samples that fill their 16 / 24 / 32 bits
        if (!plain && f.bits_per_sample != 16 && f.bits_per_sample != 24 && f.bits_per_sample != 32) return SK_ERR_UNSUPPORTED;
        sk_pcm_tick_stream &t = d.ts[i];
        t.stream = f.stream, t.n_units = f.n_units, t.channels = f.channels, t.resample = f.resample, t.flush = f.flush;
        // a stream delivered as decoded is planned as s16 whatever its width: its records are rewritten behind the body
        t.out_bits = plain ? 16 : f.out_bits, t.out_channels = f.out_channels;
        t.format = (uint8_t)(plain || width == 2 ? SK_FMT_S16LE : (width == 3 ? SK_FMT_S24LE : SK_FMT_S32LE));
        d.tick.plain[i] = plain;
        d.first[i] = (uint32_t)at;
        if (at + f.n_units > n_frames) return SK_ERR_INVALID_ARG;
        for (uint32_t u = 0; u < f.n_units; ++u) {
            const sk_flac_frame_info &fr = frames[at + u];
            if (fr.channels != f.channels || fr.bits_per_sample != f.bits_per_sample || fr.block_size == 0 || fr.block_size > 65536 || fr.header_bytes < 6 ||
                fr.frame_bytes < (uint32_t)fr.header_bytes + 3 || fr.frame_bytes > (1u << 24) || fr.offset % 16)
                return SK_ERR_INVALID_ARG;
            if (fr.offset > bytes_len || fr.frame_bytes > bytes_len - fr.offset) return SK_ERR_INVALID_ARG;
            const uint64_t decoded = (uint64_t)fr.block_size * f.channels * width;
            d.units[at + u] = sk_pcm_unit{cursor, (uint32_t)decoded, 0};
            cursor += (decoded + 15) & ~15ull;
        }
        at += f.n_units;
    }
    if (cursor > 0x7fffffffull || bytes_len > 0x7fffffffull) return SK_ERR_INVALID_ARG;
    d.tick.decoded_len = (size_t)cursor;
    return at == n_frames ? SK_OK : SK_ERR_INVALID_ARG;
}

// one pass of the decode in front of the body: the frames of the streams whose `plain` is as_is, each to where dst_of puts it
int flac_tick_decode(sk_engine *e, const sk_flac_frame_info *frames, uint32_t n_frames, size_t bytes_len, FlacDerived &d, bool as_is,
                     const std::function<uint8_t *(uint32_t, uint32_t)> &dst_of, const uint8_t *d_src) {
    const int p = as_is ? 1 : 0;
    std::vector<sk::FlacFrame> &table = d.table[p];
    std::vector<uint32_t> &order = d.order[p], &index = d.index[p];
    std::vector<uint8_t *> dst;
    for (uint32_t i = 0; i < (uint32_t)d.ts.size(); ++i) {
        if ((d.tick.plain[i] != 0) != as_is) continue;
        for (uint32_t u = 0; u < d.ts[i].n_units; ++u) index.push_back(d.first[i] + u), dst.push_back(dst_of(i, u));
    }
    const uint32_t n = (uint32_t)index.size();
    if (n == 0) return SK_OK;
    uint8_t *base = *std::min_element(dst.begin(), dst.end());
    if (!as_is) {
        // what a rejected frame leaves for the body to convert is silence, not whatever an earlier tick had there
        size_t extent = 0;
        for (uint32_t k = 0; k < n; ++k) extent = std::max(extent, (size_t)(dst[k] - base) + d.units[index[k]].byte_len);
        SK_HIP(hipMemsetAsync(base, 0, extent, e->stream), "clear tick flac decoded");
    }
    uint64_t ws_words = 0, n_subs = 0;
    table.resize(n);
    for (uint32_t k = 0; k < n; ++k) {
        const sk_flac_frame_info &f = frames[index[k]];
        sk::FlacFrame &t = table[k];
        t.byte_offset = f.offset, t.byte_len = f.frame_bytes, t.block_size = f.block_size, t.ws_offset = (uint32_t)ws_words;
        t.out_offset = (uint64_t)(dst[k] - base), t.sub0 = (uint32_t)n_subs;
        t.header_bytes = f.header_bytes, t.channels = f.channels, t.assignment = f.assignment, t.bits = f.bits_per_sample;
        ws_words += (uint64_t)f.block_size * f.channels;
        n_subs += f.channels;
    }
    if (ws_words > 0x3fffffffu) return SK_ERR_INVALID_ARG;
    order.resize(n);
    for (uint32_t k = 0; k < n; ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return table[a].byte_len > table[b].byte_len; });
    // each pass has its own part of flac_in, sized for every frame of the call: table | order | statuses
    const auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t at_order = up16(n_frames * sizeof(sk::FlacFrame)), at_status = at_order + up16(n_frames * sizeof(uint32_t)),
                 part = at_status + up16(n_frames * sizeof(int32_t));
    const size_t at_subs = up16((size_t)ws_words * 4);
    SK_HIP(e->flac_in.reserve(2 * part), "alloc tick flac tables");
    SK_HIP(e->flac_ws.reserve(at_subs + (size_t)n_subs * sizeof(sk::FlacSubframe)), "alloc tick flac workspace");
    uint8_t *d_in = (uint8_t *)e->flac_in.p + (size_t)p * part, *d_ws = (uint8_t *)e->flac_ws.p;
    SK_HIP(hipMemcpyAsync(d_in, table.data(), n * sizeof(sk::FlacFrame), hipMemcpyHostToDevice, e->stream), "H2D tick flac table");
    SK_HIP(hipMemcpyAsync(d_in + at_order, order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream), "H2D tick flac order");
    SK_HIP(hipMemsetAsync(d_ws + at_subs, 0xff, (size_t)n_subs * sizeof(sk::FlacSubframe), e->stream), "clear tick flac records");
    const sk::FlacFrame *d_table = (const sk::FlacFrame *)d_in;
    sk::FlacSubframe *d_subs = (sk::FlacSubframe *)(d_ws + at_subs);
    int32_t *d_status = (int32_t *)(d_in + at_status);
    SK_HIP(sk::launch_flac_residual(d_table, (const uint32_t *)(d_in + at_order), n, d_src, (uint32_t)bytes_len, (int32_t *)d_ws, d_subs, d_status, e->stream),
           "tick flac residual");
    SK_HIP(sk::launch_flac_restore(d_subs, (uint32_t)n_subs, (int32_t *)d_ws, d_status, e->stream), "tick flac restore");
    SK_HIP(sk::launch_flac_output(d_table, n, d_subs, (const int32_t *)d_ws, d_status, base, sk::kFlacOutContract, e->stream), "tick flac output");
    d.status[p].assign(n, 0);
    SK_HIP(hipMemcpyAsync(d.status[p].data(), d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream), "D2H tick flac statuses");
    return SK_OK;
}

}  // namespace

// FlacDecoder: the reader in front of the decode stage.  Frames wait in `pending` (their bytes packed one after the other) until a
// call has room for them.
struct sk_flac_decoder {
    sk_engine *eng = nullptr;
    sk_flac::Reader reader;
    std::vector<sk_flac_frame_info> pending;  // offsets into pending_bytes
    std::vector<uint8_t> pending_bytes;
    size_t next = 0;  // first pending frame not decoded yet
    uint64_t frames_decoded = 0;
    bool failed = false;
    std::string error;
    std::vector<uint8_t> staging;
    std::vector<int32_t> status;
};

namespace {

int flac_decoder_fail(sk_flac_decoder *d, const std::string &text) {
    d->failed = true;
    d->error = text;
    return SK_FLAC_ERR_STREAM;
}

int flac_decoder_decode(sk_flac_decoder *d, const uint8_t *input, size_t len, void *out, size_t out_cap, size_t *written, uint32_t mode) {
    if (!d || !written || (len && !input) || (out_cap && !out)) return SK_ERR_INVALID_ARG;
    *written = 0;
    if (d->failed) return SK_FLAC_ERR_STREAM;
    // Everything the reader can cut out of its buffer and the input, a table of 256 frames at a time.  An empty input finalises the
    // reader only when no frame waits for room: until then a call without input is the caller fetching what an earlier call could
    // not give it, in the middle of the stream as well.
    const bool finalise = len == 0 && d->next == d->pending.size();
    if (len != 0 || finalise) {
        sk_flac_frame_info got[256];
        for (bool first = true;; first = false) {
            uint32_t n = 0;
            const uint8_t *data = nullptr;
            if (!d->reader.feed(first ? input : nullptr, first ? len : 0, finalise, got, 256, &n, &data)) return flac_decoder_fail(d, d->reader.error());
            for (uint32_t i = 0; i < n; ++i) {
                sk_flac_frame_info f = got[i];
                const size_t at = (d->pending_bytes.size() + 15) & ~(size_t)15;
                d->pending_bytes.resize(at);
                d->pending_bytes.insert(d->pending_bytes.end(), data + f.offset, data + f.offset + f.frame_bytes);
                f.offset = (uint32_t)at;
                d->pending.push_back(f);
            }
            if (n < 256) break;
        }
    }
    // whole frames that fit
    const size_t sample_bytes = mode == sk::kFlacOutI32 ? 4 : 2;
    size_t take = 0, samples = 0;
    while (d->next + take < d->pending.size()) {
        const sk_flac_frame_info &f = d->pending[d->next + take];
        const size_t more = (size_t)f.block_size * f.channels;
        if (samples + more > out_cap) break;
        samples += more, ++take;
    }
    if (take == 0) return d->next < d->pending.size() ? SK_ERR_CAPACITY : SK_OK;
    d->status.assign(take, 0);
    d->staging.resize(samples * sample_bytes);
    size_t out_len = 0;
    const int rc = flac_decode_frames(d->eng, d->pending.data() + d->next, (uint32_t)take, d->pending_bytes.data(), false, d->staging.data(),
                                      d->staging.size(), &out_len, d->status.data(), mode);
    if (rc != SK_OK) return rc;
    for (size_t i = 0; i < take; ++i)
        if (d->status[i] != 0)
            return flac_decoder_fail(d, "FLAC frame " + std::to_string(d->frames_decoded + i) + ": " +
                                            (d->status[i] == SK_ERR_UNSUPPORTED ? "32-bit samples with a side channel are not supported"
                                                                                : "the subframes break the syntax or miss the frame's end"));
    std::memcpy(out, d->staging.data(), out_len);
    d->frames_decoded += take;
    d->next += take;
    if (d->next == d->pending.size()) d->pending.clear(), d->pending_bytes.clear(), d->next = 0;
    *written = samples;
    return SK_OK;
}

}  // namespace

extern "C" {

int sk_flac_parse_header(const uint8_t *data, size_t len, const sk_flac_streaminfo *info, sk_flac_frame_info *out) try {
    sk::abi_enter();
    if ((len && !data) || !out) return SK_ERR_INVALID_ARG;
    return sk_flac::parse_header(data, len, info, out);
} catch (...) {
    return sk::abi_caught("sk_flac_parse_header");
}

int sk_flac_scan(const uint8_t *data, size_t len, const sk_flac_streaminfo *info, int final, sk_flac_frame_info *frames, uint32_t cap,
                 uint32_t *n_frames, size_t *consumed) try {
    sk::abi_enter();
    if ((len && !data) || (cap && !frames) || !n_frames || !consumed || len > 0x7fffffffu) return SK_ERR_INVALID_ARG;
    return sk_flac::scan(data, len, info, final != 0, frames, cap, n_frames, consumed);
} catch (...) {
    return sk::abi_caught("sk_flac_scan");
}

int sk_flac_reader_create(sk_flac_reader **out) try {
    sk::abi_enter();
    if (!out) return SK_ERR_INVALID_ARG;
    *out = new sk_flac_reader();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_flac_reader_create");
}

void sk_flac_reader_destroy(sk_flac_reader *r) try {
    sk::abi_enter();
    delete r;
} catch (...) {
    (void)sk::abi_caught("sk_flac_reader_destroy");
}

int sk_flac_reader_add(sk_flac_reader *r, const uint8_t *bytes, size_t len, sk_flac_frame_info *frames, uint32_t cap, uint32_t *n_frames,
                       const uint8_t **data) try {
    sk::abi_enter();
    if (!r || (len && !bytes) || (cap && !frames) || !n_frames || len > 0x7fffffffu) return SK_ERR_INVALID_ARG;
    return r->reader.add(bytes, len, frames, cap, n_frames, data) ? SK_OK : SK_FLAC_ERR_STREAM;
} catch (...) {
    return sk::abi_caught("sk_flac_reader_add");
}

int sk_flac_reader_info(const sk_flac_reader *r, sk_flac_info *info) try {
    sk::abi_enter();
    if (!r || !info) return SK_ERR_INVALID_ARG;
    std::memset(info, 0, sizeof *info);
    info->buffered_bytes = (uint32_t)r->reader.buffered_bytes();
    info->frames = r->reader.frames();
    if (r->reader.have_info()) info->streaminfo = r->reader.info(), info->have_streaminfo = 1;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_flac_reader_info");
}

const char *sk_flac_reader_last_error(const sk_flac_reader *r) try {
    sk::abi_enter();
    return r ? r->reader.error().c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_flac_reader_last_error");
    return "";
}

int sk_flac_decode_frames(sk_engine *e, const sk_flac_frame_info *frames, uint32_t n, const uint8_t *bytes, uint8_t *out, size_t out_cap,
                          size_t *out_len, int32_t *status_per_frame) try {
    sk::abi_enter();
    return flac_decode_frames(e, frames, n, bytes, false, out, out_cap, out_len, status_per_frame, sk::kFlacOutContract);
} catch (...) {
    return sk::abi_caught("sk_flac_decode_frames");
}

int sk_flac_decode_frames_dev(sk_engine *e, const sk_flac_frame_info *frames, uint32_t n, const uint8_t *d_bytes, uint8_t *d_out, size_t out_cap,
                              size_t *out_len, int32_t *status_per_frame) try {
    sk::abi_enter();
    return flac_decode_frames(e, frames, n, d_bytes, true, d_out, out_cap, out_len, status_per_frame, sk::kFlacOutContract);
} catch (...) {
    return sk::abi_caught("sk_flac_decode_frames_dev");
}

size_t sk_tick_flac_out_bound_on(sk_engine *e, const sk_flac_tick_stream *fs, uint32_t n_streams, const sk_flac_frame_info *frames, uint32_t n_frames,
                                 uint32_t *max_outputs) try {
    sk::abi_enter();
    if (max_outputs) *max_outputs = 0;
    if (!e || (!fs && n_streams) || (!frames && n_frames)) return 0;
    FlacDerived d;
    if (flac_tick_derive(fs, n_streams, frames, n_frames, 0x7fffffffu, d) != SK_OK) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return tick_pcm_out_bound(e, d.ts.data(), n_streams, d.units.data(), n_frames, max_outputs, d.tick.plain.data());
} catch (...) {
    (void)sk::abi_caught("sk_tick_flac_out_bound_on");
    return 0;
}

int sk_tick_run_flac(sk_engine *e, const sk_flac_tick_stream *fs, uint32_t n_streams, const sk_flac_frame_info *frames, uint32_t n_frames,
                     const uint8_t *bytes, size_t bytes_len, uint8_t *out, size_t out_cap, sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs,
                     size_t *out_bytes, int32_t *status_per_frame) try {
    sk::abi_enter();
    if (!e || !n_outs || (n_streams && !fs) || (n_frames && (!frames || !bytes || !status_per_frame))) return SK_ERR_INVALID_ARG;
    *n_outs = 0;
    if (out_bytes) *out_bytes = 0;
    FlacDerived d;
    int rc = flac_tick_derive(fs, n_streams, frames, n_frames, bytes_len, d);
    if (rc != SK_OK) return rc;
    d.tick.decode = [&](bool as_is, const std::function<uint8_t *(uint32_t, uint32_t)> &dst_of, const uint8_t *d_src) {
        return flac_tick_decode(e, frames, n_frames, bytes_len, d, as_is, dst_of, d_src);
    };
    rc = tick_pcm_impl(e, d.ts.data(), n_streams, d.units.data(), n_frames, bytes, bytes_len, out, out_cap, outs, outs_cap, n_outs, out_bytes, &d.tick);
    if (rc != SK_OK) return rc;
    for (int p = 0; p < 2; ++p)
        for (size_t k = 0; k < d.index[p].size(); ++k) status_per_frame[d.index[p][k]] = d.status[p][k];
    // the records of a stream delivered as decoded say what its frames are; a rejected frame marks its record, or -- behind a
    // conversion, where records and frames do not correspond -- every record of its stream in this tick
    std::vector<uint32_t> seen(n_streams, 0);
    for (uint32_t k = 0; k < *n_outs; ++k) {
        sk_tick_output &o = outs[k];
        const uint32_t i = o.stream_index;
        if (d.tick.plain[i]) {
            const uint32_t g = d.first[i] + seen[i]++;
            o.frames = frames[g].block_size, o.channels = fs[i].channels, o.status = status_per_frame[g];
            o.bits = (uint8_t)(flac_width(fs[i].bits_per_sample, sk::kFlacOutContract) * 8);
        } else {
            for (uint32_t u = 0; u < fs[i].n_units && o.status == 0; ++u) o.status = status_per_frame[d.first[i] + u];
        }
    }
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_tick_run_flac");
}

int sk_flac_decoder_create(sk_engine *e, sk_flac_decoder **out) try {
    sk::abi_enter();
    if (!e || !out) return SK_ERR_INVALID_ARG;
    *out = new sk_flac_decoder();
    (*out)->eng = e;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_flac_decoder_create");
}

void sk_flac_decoder_destroy(sk_flac_decoder *d) try {
    sk::abi_enter();
    delete d;
} catch (...) {
    (void)sk::abi_caught("sk_flac_decoder_destroy");
}

int sk_flac_decoder_reset(sk_flac_decoder *d) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    sk_engine *e = d->eng;
    *d = sk_flac_decoder();
    d->eng = e;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_flac_decoder_reset");
}

int sk_flac_decoder_info(const sk_flac_decoder *d, uint32_t *sample_rate, uint8_t *channels, uint8_t *bits_per_sample, uint64_t *frames_decoded) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    const bool have = d->reader.have_info();
    if (sample_rate) *sample_rate = have ? d->reader.info().sample_rate : 0;
    if (channels) *channels = have ? d->reader.info().channels : 0;
    if (bits_per_sample) *bits_per_sample = have ? d->reader.info().bits_per_sample : 0;
    if (frames_decoded) *frames_decoded = d->frames_decoded;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_flac_decoder_info");
}

size_t sk_flac_decoder_pending_samples(const sk_flac_decoder *d) try {
    sk::abi_enter();
    size_t n = 0;
    for (size_t k = d ? d->next : 0; d && k < d->pending.size(); ++k) n += (size_t)d->pending[k].block_size * d->pending[k].channels;
    return n;
} catch (...) {
    (void)sk::abi_caught("sk_flac_decoder_pending_samples");
    return 0;
}

int sk_flac_decoder_decode_i32(sk_flac_decoder *d, const uint8_t *input, size_t len, int32_t *out, size_t out_cap, size_t *written) try {
    sk::abi_enter();
    return flac_decoder_decode(d, input, len, out, out_cap, written, sk::kFlacOutI32);
} catch (...) {
    return sk::abi_caught("sk_flac_decoder_decode_i32");
}

int sk_flac_decoder_decode_i16(sk_flac_decoder *d, const uint8_t *input, size_t len, int16_t *out, size_t out_cap, size_t *written) try {
    sk::abi_enter();
    return flac_decoder_decode(d, input, len, out, out_cap, written, sk::kFlacOutI16Clamp);
} catch (...) {
    return sk::abi_caught("sk_flac_decoder_decode_i16");
}

const char *sk_flac_decoder_last_error(const sk_flac_decoder *d) try {
    sk::abi_enter();
    return d ? d->error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_flac_decoder_last_error");
    return "";
}

}  // extern "C"

// ---- ALAC (alac_stream.h, alac_decode.hip) ----------------------------------------------------------------------------------------

struct sk_caf_alac_index {
    sk_alac::CafIndex index;
};

struct sk_alac_packet_decoder {
    sk_engine *eng = nullptr;
    sk_alac_config config{};
    std::string error;
};

namespace {

void alac_text(char *error, size_t cap, const std::string &text) {
    if (!error || cap == 0) return;
    const size_t n = std::min(cap - 1, text.size());
    std::memcpy(error, text.data(), n);
    error[n] = 0;
}

// what one run of the three kernels works on: packets of any number of cookies, each with its place in the bytes, the workspace and
// the output.  add() is called per packet in the order of the output; the statuses start as what the host said (a packet whose frame
// count it could not read is not handed to a lane) and come back as the device's.
struct AlacBatch {
    std::vector<sk::AlacParams> cfgs;
    std::vector<sk::AlacPacket> table;
    std::vector<uint32_t> order, lanes;
    std::vector<int32_t> status;
    uint64_t ws_words = 0;
    uint32_t n_recs = 0;

    uint32_t add_config(const sk_alac_config &c) {
        sk::AlacParams p{};
        p.frame_length = c.frame_length, p.bit_depth = c.bit_depth, p.pb = c.pb, p.mb = c.mb, p.kb = c.kb, p.channels = c.channels;
        for (uint32_t i = 0; i < cfgs.size(); ++i)
            if (std::memcmp(&cfgs[i], &p, sizeof p) == 0) return i;
        cfgs.push_back(p);
        return (uint32_t)cfgs.size() - 1;
    }
    // frames = 0: refused by the host with host_status
    void add(uint32_t cfg, uint32_t offset, uint32_t size, uint32_t frames, uint64_t out_offset, int32_t host_status) {
        const uint32_t ch = cfgs[cfg].channels, k = (uint32_t)table.size();
        sk::AlacPacket t{};
        t.byte_offset = offset, t.byte_len = size, t.frames = frames, t.ws_offset = (uint32_t)ws_words, t.rec0 = n_recs, t.cfg = cfg;
        t.out_offset = out_offset;
        table.push_back(t);
        status.push_back(frames ? (int32_t)SK_ALAC_INVALID : host_status);
        if (!frames) return;
        order.push_back(k);
        for (uint32_t c = 0; c < ch; ++c) lanes.push_back(k << 3 | c);
        ws_words += (uint64_t)frames * ch;
        n_recs += ch;
    }
    static size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
    // the tables' device form: configs | packet table | order | lanes | statuses
    size_t tables_len() const {
        return up16(cfgs.size() * sizeof(sk::AlacParams)) + up16(table.size() * sizeof(sk::AlacPacket)) + up16(order.size() * 4) + up16(lanes.size() * 4) +
               up16(status.size() * 4);
    }
    size_t ws_len() const { return up16((size_t)ws_words * 4) + (size_t)n_recs * sizeof(sk::AlacChannel); }
};

// uploads the tables to d_tables (tables_len() bytes), runs the three launches with the workspace at d_ws (ws_len() bytes) and asks for
// the statuses back into b.status; everything on e->stream, nothing waited for.  b must live until the stream has been waited for.
int alac_launch(sk_engine *e, AlacBatch &b, uint8_t *d_tables, uint8_t *d_ws, const uint8_t *d_bytes, uint32_t bytes_len, uint8_t *d_out) {
    const uint32_t n = (uint32_t)b.table.size();
    if (n == 0) return SK_OK;
    if (b.ws_words > 0x3fffffffu || n > (1u << 28)) return SK_ERR_INVALID_ARG;
    std::stable_sort(b.order.begin(), b.order.end(), [&](uint32_t x, uint32_t y) { return b.table[x].byte_len > b.table[y].byte_len; });
    const size_t at_table = AlacBatch::up16(b.cfgs.size() * sizeof(sk::AlacParams)), at_order = at_table + AlacBatch::up16(n * sizeof(sk::AlacPacket)),
                 at_lanes = at_order + AlacBatch::up16(b.order.size() * 4), at_status = at_lanes + AlacBatch::up16(b.lanes.size() * 4);
    SK_HIP(hipMemcpyAsync(d_tables, b.cfgs.data(), b.cfgs.size() * sizeof(sk::AlacParams), hipMemcpyHostToDevice, e->stream), "H2D alac configs");
    SK_HIP(hipMemcpyAsync(d_tables + at_table, b.table.data(), n * sizeof(sk::AlacPacket), hipMemcpyHostToDevice, e->stream), "H2D alac table");
    if (!b.order.empty()) {
        SK_HIP(hipMemcpyAsync(d_tables + at_order, b.order.data(), b.order.size() * 4, hipMemcpyHostToDevice, e->stream), "H2D alac order");
        SK_HIP(hipMemcpyAsync(d_tables + at_lanes, b.lanes.data(), b.lanes.size() * 4, hipMemcpyHostToDevice, e->stream), "H2D alac lanes");
    }
    SK_HIP(hipMemcpyAsync(d_tables + at_status, b.status.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, e->stream), "H2D alac statuses");
    const sk::AlacParams *d_cfgs = (const sk::AlacParams *)d_tables;
    const sk::AlacPacket *d_table = (const sk::AlacPacket *)(d_tables + at_table);
    sk::AlacChannel *d_recs = (sk::AlacChannel *)(d_ws + AlacBatch::up16((size_t)b.ws_words * 4));
    int32_t *d_status = (int32_t *)(d_tables + at_status);
    SK_HIP(sk::launch_alac_entropy(d_cfgs, d_table, (const uint32_t *)(d_tables + at_order), (uint32_t)b.order.size(), d_bytes, bytes_len, (int32_t *)d_ws,
                                   d_recs, d_status, e->stream), "launch alac entropy");
    SK_HIP(sk::launch_alac_predict(d_table, (const uint32_t *)(d_tables + at_lanes), (uint32_t)b.lanes.size(), d_recs, (int32_t *)d_ws, d_status, e->stream),
           "launch alac predict");
    SK_HIP(sk::launch_alac_output(d_cfgs, d_table, n, d_recs, (const int32_t *)d_ws, d_status, d_bytes, d_out, e->stream), "launch alac output");
    SK_HIP(hipMemcpyAsync(b.status.data(), d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream), "D2H alac statuses");
    return SK_OK;
}

// sk_alac_decode_packets[_dev].  Host form: `frames_out` is written (sk_alac_packet_frames per packet); device form: `frames_in` is read.
int alac_decode_packets(sk_engine *e, const sk_alac_config *cfg, const sk_alac_packet *packets, uint32_t n, const uint8_t *bytes, size_t dev_bytes_len,
                        bool on_device, uint8_t *out, size_t out_cap, size_t *out_len, int32_t *status, uint32_t *frames_out, const uint32_t *frames_in) {
    if (!e || !cfg || !out_len || (n && (!packets || !bytes || !out || !status || !(on_device ? (const void *)frames_in : (const void *)frames_out))))
        return SK_ERR_INVALID_ARG;
    *out_len = 0;
    std::string text;
    if (!sk_alac::validate(*cfg, &text)) return SK_ERR_INVALID_ARG;
    if (n == 0) return SK_OK;
    const uint32_t ch = cfg->channels, width = cfg->bit_depth / 8u;
    AlacBatch b;
    const uint32_t c0 = b.add_config(*cfg);
    std::vector<uint32_t> frames(n);
    uint64_t need = 0, bytes_len = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const sk_alac_packet &p = packets[i];
        if (p.size == 0 || p.size > sk_alac::kMaxPacketBytes || (p.offset & 15u)) return SK_ERR_INVALID_ARG;
        bytes_len = std::max<uint64_t>(bytes_len, (uint64_t)p.offset + p.size);
        if (bytes_len > 0x7fffffffu || (on_device && bytes_len > dev_bytes_len)) return SK_ERR_INVALID_ARG;
        uint32_t f = 0;
        int32_t host = SK_ALAC_INVALID;
        if (on_device) {
            f = frames_in[i];
            if (f > cfg->frame_length) return SK_ERR_INVALID_ARG;
        } else if ((host = sk_alac::packet_frames(*cfg, bytes + p.offset, p.size, &f)) != SK_OK) {
            f = 0;
        }
        frames[i] = f;
        b.add(c0, p.offset, p.size, f, need, host);
        need += (uint64_t)f * ch * width;
        if (b.ws_words > 0x3fffffffu) return SK_ERR_INVALID_ARG;
    }
    if (need > out_cap) return SK_ERR_INVALID_ARG;
    if (on_device && (((uintptr_t)bytes | (uintptr_t)out) & 15)) return SK_ERR_INVALID_ARG;

    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    // alac_in: [bytes (host form)] | the batch's tables
    const size_t at_tables = on_device ? 0 : AlacBatch::up16((size_t)bytes_len);
    SK_HIP(e->alac_in.reserve(at_tables + b.tables_len()), "alloc alac input");
    SK_HIP(e->alac_ws.reserve(b.ws_len()), "alloc alac workspace");
    uint8_t *d_in = (uint8_t *)e->alac_in.p, *d_out = out;
    const uint8_t *d_bytes = bytes;
    if (!on_device) {
        SK_HIP(e->alac_out.reserve(std::max<size_t>((size_t)need, 16)), "alloc alac output");
        d_out = (uint8_t *)e->alac_out.p;
        SK_HIP(hipMemcpyAsync(d_in, bytes, (size_t)bytes_len, hipMemcpyHostToDevice, e->stream), "H2D alac packets");
        d_bytes = d_in;
    }
    const int rc = alac_launch(e, b, d_in + at_tables, (uint8_t *)e->alac_ws.p, d_bytes, (uint32_t)(on_device ? dev_bytes_len : bytes_len), d_out);
    if (rc != SK_OK) return rc;
    SK_HIP(hipStreamSynchronize(e->stream), "alac sync");  // the tables leave scope with the call
    for (uint32_t i = 0; i < n; ++i) status[i] = b.status[i];
    if (!on_device) {
        // a rejected packet's place in the caller's buffer stays as it was: the accepted packets are copied one run at a time
        uint32_t i = 0;
        while (i < n) {
            if (status[i] != 0) {
                ++i;
                continue;
            }
            uint32_t j = i;
            while (j < n && status[j] == 0) ++j;
            const uint64_t from = b.table[i].out_offset, to = j < n ? b.table[j].out_offset : need;
            SK_HIP(hipMemcpyAsync(out + from, d_out + from, (size_t)(to - from), hipMemcpyDeviceToHost, e->stream), "D2H alac");
            i = j;
        }
        SK_HIP(hipStreamSynchronize(e->stream), "alac sync");
        for (uint32_t k = 0; k < n; ++k) frames_out[k] = frames[k];
    }
    *out_len = (size_t)need;
    return SK_OK;
}

// sk_tick_run_alac / sk_tick_alac_out_bound_on: checks the table and derives what the PCM tick's body works on, as flac_tick_derive does --
// per stream a little-endian source of the cookie's format, per packet where its decoded PCM lies (16-byte aligned, packet after packet)
// -- and the decode that stands in front of the body: the three launches of alac_decode.hip over the packets of each pass.
struct AlacDerived {
    std::vector<sk_pcm_tick_stream> ts;
    std::vector<sk_pcm_unit> units;  // the decoded layout
    std::vector<uint32_t> first;     // per stream: its first packet
    AiffTick tick;
    // what the two passes (streams that go on through the body, streams delivered as decoded) upload and get back: alive until the
    // tick's last wait
    AlacBatch batch[2];
    std::vector<uint32_t> index[2];  // row of the batch -> packet of the call
    size_t part = 0, ws_len = 0;     // of alac_in per pass, of alac_ws: sized for every packet of the call
};

sk_alac_config alac_row_config(const sk_alac_tick_stream &a) {
    sk_alac_config c{};
    c.frame_length = a.frame_length, c.sample_rate = 1, c.bit_depth = a.bit_depth, c.pb = a.pb, c.mb = a.mb, c.kb = a.kb, c.channels = a.channels;
    return c;
}

int alac_tick_derive(const sk_alac_tick_stream *as, uint32_t n_streams, const sk_alac_tick_packet *packets, uint32_t n_packets, size_t bytes_len,
                     AlacDerived &d) {
    d.ts.assign(n_streams, sk_pcm_tick_stream{});
    d.units.assign(n_packets, sk_pcm_unit{});
    d.first.assign(n_streams, 0);
    d.tick.plain.assign(n_streams, 0);
    d.tick.states.assign((size_t)n_streams * 2, 0);
    uint64_t at = 0, cursor = 0, ws_words = 0, recs = 0;
    std::string text;
    for (uint32_t i = 0; i < n_streams; ++i) {
        const sk_alac_tick_stream &a = as[i];
        if (!sk_alac::validate(alac_row_config(a), &text)) return SK_ERR_INVALID_ARG;
        const uint32_t width = a.bit_depth / 8u, ch = a.channels;
        const bool plain = !a.resample && a.out_bits == a.bit_depth && a.out_channels == ch;
        sk_pcm_tick_stream &t = d.ts[i];
        t.stream = a.stream, t.n_units = a.n_units, t.channels = (uint8_t)ch, t.resample = a.resample, t.flush = a.flush;
        // a stream delivered as decoded is planned as s16 whatever its width: its records are rewritten behind the body
        t.out_bits = plain ? 16 : a.out_bits, t.out_channels = a.out_channels;
        t.format = (uint8_t)(plain || width == 2 ? SK_FMT_S16LE : (width == 3 ? SK_FMT_S24LE : SK_FMT_S32LE));
        d.tick.plain[i] = plain;
        d.first[i] = (uint32_t)at;
        if (at + a.n_units > n_packets) return SK_ERR_INVALID_ARG;
        for (uint32_t u = 0; u < a.n_units; ++u) {
            const sk_alac_tick_packet &p = packets[at + u];
            const uint32_t f = p.frames;
            if (p.size == 0 || p.size > sk_alac::kMaxPacketBytes || p.offset % 16 || f == 0 || f > a.frame_length) return SK_ERR_INVALID_ARG;
            if (p.offset > bytes_len || p.size > bytes_len - p.offset) return SK_ERR_INVALID_ARG;
            const uint64_t decoded = (uint64_t)f * ch * width;
            d.units[at + u] = sk_pcm_unit{cursor, (uint32_t)decoded, 0};
            cursor += (decoded + 15) & ~15ull;
            ws_words += (uint64_t)f * ch;
            recs += ch;
        }
        at += a.n_units;
    }
    if (cursor > 0x7fffffffull || bytes_len > 0x7fffffffull || ws_words > 0x3fffffffull) return SK_ERR_INVALID_ARG;
    d.tick.decoded_len = (size_t)cursor;
    d.part = AlacBatch::up16(n_streams * sizeof(sk::AlacParams)) + AlacBatch::up16(n_packets * sizeof(sk::AlacPacket)) + 2 * AlacBatch::up16(n_packets * 4) +
             AlacBatch::up16((size_t)recs * 4);
    d.ws_len = AlacBatch::up16((size_t)ws_words * 4) + (size_t)recs * sizeof(sk::AlacChannel);
    return at == n_packets ? SK_OK : SK_ERR_INVALID_ARG;
}

// one pass of the decode in front of the body: the packets of the streams whose `plain` is as_is, each to where dst_of puts it
int alac_tick_decode(sk_engine *e, const sk_alac_tick_stream *as, const sk_alac_tick_packet *packets, size_t bytes_len, AlacDerived &d, bool as_is,
                     const std::function<uint8_t *(uint32_t, uint32_t)> &dst_of, const uint8_t *d_src) {
    const int p = as_is ? 1 : 0;
    AlacBatch &b = d.batch[p];
    std::vector<uint32_t> &index = d.index[p];
    std::vector<uint8_t *> dst;
    std::vector<uint32_t> cfg_of;
    for (uint32_t i = 0; i < (uint32_t)d.ts.size(); ++i) {
        if ((d.tick.plain[i] != 0) != as_is || d.ts[i].n_units == 0) continue;
        const uint32_t c = b.add_config(alac_row_config(as[i]));
        for (uint32_t u = 0; u < d.ts[i].n_units; ++u) index.push_back(d.first[i] + u), dst.push_back(dst_of(i, u)), cfg_of.push_back(c);
    }
    const uint32_t n = (uint32_t)index.size();
    if (n == 0) return SK_OK;
    uint8_t *base = *std::min_element(dst.begin(), dst.end());
    if (!as_is) {
        // what a rejected packet leaves for the body to convert is silence, not whatever an earlier tick had there
        size_t extent = 0;
        for (uint32_t k = 0; k < n; ++k) extent = std::max(extent, (size_t)(dst[k] - base) + d.units[index[k]].byte_len);
        SK_HIP(hipMemsetAsync(base, 0, extent, e->stream), "clear tick alac decoded");
    }
    for (uint32_t k = 0; k < n; ++k) {
        const sk_alac_tick_packet &pk = packets[index[k]];
        b.add(cfg_of[k], pk.offset, pk.size, pk.frames, (uint64_t)(dst[k] - base), SK_ALAC_INVALID);
    }
    // both passes' tables have their own part of alac_in; the workspace is shared, the passes follow each other on the stream
    SK_HIP(e->alac_in.reserve(2 * d.part), "alloc tick alac tables");
    SK_HIP(e->alac_ws.reserve(d.ws_len), "alloc tick alac workspace");
    return alac_launch(e, b, (uint8_t *)e->alac_in.p + (size_t)p * d.part, (uint8_t *)e->alac_ws.p, d_src, (uint32_t)bytes_len, base);
}

}  // namespace

extern "C" {

int sk_alac_parse_cookie(const uint8_t *cookie, size_t len, sk_alac_config *out, char *error, size_t error_cap) try {
    sk::abi_enter();
    if ((len && !cookie) || !out) return SK_ERR_INVALID_ARG;
    std::string text;
    alac_text(error, error_cap, "");
    if (sk_alac::parse_cookie(cookie, len, out, &text)) return SK_OK;
    alac_text(error, error_cap, text);
    return SK_ALAC_ERR_STREAM;
} catch (...) {
    return sk::abi_caught("sk_alac_parse_cookie");
}

int sk_alac_packet_frames(const sk_alac_config *cfg, const uint8_t *packet, size_t len, uint32_t *frames) try {
    sk::abi_enter();
    if (!cfg || (len && !packet) || !frames) return SK_ERR_INVALID_ARG;
    *frames = 0;
    return sk_alac::packet_frames(*cfg, packet, len, frames);
} catch (...) {
    return sk::abi_caught("sk_alac_packet_frames");
}

int sk_caf_alac_index_create(const uint8_t *desc, size_t desc_len, const uint8_t *cookie, size_t cookie_len, const uint8_t *pakt, size_t pakt_len,
                             uint64_t data_offset, uint64_t data_size, sk_caf_alac_index **out, char *error, size_t error_cap) try {
    sk::abi_enter();
    if ((desc_len && !desc) || (cookie_len && !cookie) || (pakt_len && !pakt) || !out) return SK_ERR_INVALID_ARG;
    *out = nullptr;
    alac_text(error, error_cap, "");
    std::unique_ptr<sk_caf_alac_index> ix(new sk_caf_alac_index());
    std::string text;
    if (!sk_alac::caf_index(desc, desc_len, cookie, cookie_len, pakt, pakt_len, data_offset, data_size, &ix->index, &text)) {
        alac_text(error, error_cap, text);
        return SK_ALAC_ERR_STREAM;
    }
    *out = ix.release();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_caf_alac_index_create");
}

int sk_caf_alac_index_from_file(const uint8_t *file, size_t len, sk_caf_alac_index **out, char *error, size_t error_cap) try {
    sk::abi_enter();
    if ((len && !file) || !out) return SK_ERR_INVALID_ARG;
    *out = nullptr;
    alac_text(error, error_cap, "");
    std::unique_ptr<sk_caf_alac_index> ix(new sk_caf_alac_index());
    std::string text;
    if (!sk_alac::caf_index_from_file(file, len, &ix->index, &text)) {
        alac_text(error, error_cap, text);
        return SK_ALAC_ERR_STREAM;
    }
    *out = ix.release();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_caf_alac_index_from_file");
}

void sk_caf_alac_index_destroy(sk_caf_alac_index *ix) try {
    sk::abi_enter();
    delete ix;
} catch (...) {
    (void)sk::abi_caught("sk_caf_alac_index_destroy");
}

int sk_caf_alac_index_info(const sk_caf_alac_index *ix, sk_caf_alac_info *info) try {
    sk::abi_enter();
    if (!ix || !info) return SK_ERR_INVALID_ARG;
    std::memset(info, 0, sizeof *info);
    info->config = ix->index.config;
    info->valid_frames = ix->index.valid_frames;
    info->priming_frames = ix->index.priming_frames, info->remainder_frames = ix->index.remainder_frames;
    info->frames_per_packet = ix->index.frames_per_packet;
    info->n_packets = (uint32_t)ix->index.packets.size();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_caf_alac_index_info");
}

int sk_caf_alac_index_packets(const sk_caf_alac_index *ix, uint64_t *offsets, uint32_t *sizes, uint32_t cap) try {
    sk::abi_enter();
    if (!ix || (cap && (!offsets || !sizes))) return SK_ERR_INVALID_ARG;
    if (cap < ix->index.packets.size()) return SK_ERR_CAPACITY;
    for (size_t i = 0; i < ix->index.packets.size(); ++i) offsets[i] = ix->index.packets[i].offset, sizes[i] = ix->index.packets[i].size;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_caf_alac_index_packets");
}

int sk_alac_decode_packets(sk_engine *e, const sk_alac_config *cfg, const sk_alac_packet *packets, uint32_t n, const uint8_t *bytes, uint8_t *out,
                           size_t out_cap, size_t *out_len, int32_t *status_per_packet, uint32_t *frames_per_packet) try {
    sk::abi_enter();
    return alac_decode_packets(e, cfg, packets, n, bytes, 0, false, out, out_cap, out_len, status_per_packet, frames_per_packet, nullptr);
} catch (...) {
    return sk::abi_caught("sk_alac_decode_packets");
}

int sk_alac_decode_packets_dev(sk_engine *e, const sk_alac_config *cfg, const sk_alac_packet *packets, uint32_t n, const uint8_t *d_bytes,
                               size_t bytes_len, uint8_t *d_out, size_t out_cap, size_t *out_len, int32_t *status_per_packet,
                               const uint32_t *frames_per_packet) try {
    sk::abi_enter();
    return alac_decode_packets(e, cfg, packets, n, d_bytes, bytes_len, true, d_out, out_cap, out_len, status_per_packet, nullptr, frames_per_packet);
} catch (...) {
    return sk::abi_caught("sk_alac_decode_packets_dev");
}

size_t sk_tick_alac_out_bound_on(sk_engine *e, const sk_alac_tick_stream *as, uint32_t n_streams, const sk_alac_tick_packet *packets, uint32_t n_packets,
                                 uint32_t *max_outputs) try {
    sk::abi_enter();
    if (max_outputs) *max_outputs = 0;
    if (!e || (!as && n_streams) || (!packets && n_packets)) return 0;
    AlacDerived d;
    if (alac_tick_derive(as, n_streams, packets, n_packets, 0x7fffffffu, d) != SK_OK) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return tick_pcm_out_bound(e, d.ts.data(), n_streams, d.units.data(), n_packets, max_outputs, d.tick.plain.data());
} catch (...) {
    (void)sk::abi_caught("sk_tick_alac_out_bound_on");
    return 0;
}

int sk_tick_run_alac(sk_engine *e, const sk_alac_tick_stream *as, uint32_t n_streams, const sk_alac_tick_packet *packets, uint32_t n_packets,
                     const uint8_t *bytes, size_t bytes_len, uint8_t *out, size_t out_cap, sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs,
                     size_t *out_bytes, int32_t *status_per_packet) try {
    sk::abi_enter();
    if (!e || !n_outs || (n_streams && !as) || (n_packets && (!packets || !bytes || !status_per_packet))) return SK_ERR_INVALID_ARG;
    *n_outs = 0;
    if (out_bytes) *out_bytes = 0;
    AlacDerived d;
    int rc = alac_tick_derive(as, n_streams, packets, n_packets, bytes_len, d);
    if (rc != SK_OK) return rc;
    d.tick.decode = [&](bool as_is, const std::function<uint8_t *(uint32_t, uint32_t)> &dst_of, const uint8_t *d_src) {
        return alac_tick_decode(e, as, packets, bytes_len, d, as_is, dst_of, d_src);
    };
    rc = tick_pcm_impl(e, d.ts.data(), n_streams, d.units.data(), n_packets, bytes, bytes_len, out, out_cap, outs, outs_cap, n_outs, out_bytes, &d.tick);
    if (rc != SK_OK) return rc;
    for (int p = 0; p < 2; ++p)
        for (size_t k = 0; k < d.index[p].size(); ++k) status_per_packet[d.index[p][k]] = d.batch[p].status[k];
    // the records of a stream delivered as decoded say what its packets are; a rejected packet marks its record, or -- behind a
    // conversion, where records and packets do not correspond -- every record of its stream in this tick
    std::vector<uint32_t> seen(n_streams, 0);
    for (uint32_t k = 0; k < *n_outs; ++k) {
        sk_tick_output &o = outs[k];
        const uint32_t i = o.stream_index;
        if (d.tick.plain[i]) {
            const uint32_t g = d.first[i] + seen[i]++;
            o.frames = packets[g].frames, o.channels = as[i].channels, o.status = status_per_packet[g];
            o.bits = as[i].bit_depth;
        } else {
            for (uint32_t u = 0; u < as[i].n_units && o.status == 0; ++u) o.status = status_per_packet[d.first[i] + u];
        }
    }
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_tick_run_alac");
}

int sk_alac_packet_decoder_create(sk_engine *e, const uint8_t *cookie, size_t cookie_len, sk_alac_packet_decoder **out, char *error,
                                  size_t error_cap) try {
    sk::abi_enter();
    if (!e || (cookie_len && !cookie) || !out) return SK_ERR_INVALID_ARG;
    *out = nullptr;
    alac_text(error, error_cap, "");
    std::unique_ptr<sk_alac_packet_decoder> d(new sk_alac_packet_decoder());
    std::string text;
    if (!sk_alac::parse_cookie(cookie, cookie_len, &d->config, &text)) {
        alac_text(error, error_cap, text);
        return SK_ALAC_ERR_STREAM;
    }
    d->eng = e;
    *out = d.release();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_alac_packet_decoder_create");
}

void sk_alac_packet_decoder_destroy(sk_alac_packet_decoder *d) try {
    sk::abi_enter();
    delete d;
} catch (...) {
    (void)sk::abi_caught("sk_alac_packet_decoder_destroy");
}

int sk_alac_packet_decoder_info(const sk_alac_packet_decoder *d, uint32_t *sample_rate, uint8_t *channels, uint8_t *bit_depth,
                                size_t *maximum_pcm_samples) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    if (sample_rate) *sample_rate = d->config.sample_rate;
    if (channels) *channels = d->config.channels;
    if (bit_depth) *bit_depth = d->config.bit_depth;
    if (maximum_pcm_samples) *maximum_pcm_samples = (size_t)d->config.frame_length * d->config.channels;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_alac_packet_decoder_info");
}

int sk_alac_packet_decoder_decode_packet(sk_alac_packet_decoder *d, const uint8_t *packet, size_t len, uint8_t *out, size_t out_cap,
                                         size_t *out_len) try {
    sk::abi_enter();
    if (!d || (len && !packet) || !out_len || (out_cap && !out)) return SK_ERR_INVALID_ARG;
    *out_len = 0;
    const auto fail = [&](const std::string &text) {
        d->error = text;
        return (int)SK_ALAC_ERR_STREAM;
    };
    if (len == 0) return fail("ALAC packet is empty");
    if (len > sk_alac::kMaxPacketBytes) return fail("ALAC packet exceeds the " + std::to_string(sk_alac::kMaxPacketBytes) + " byte budget");
    uint32_t frames = 0;
    if (const int rc = sk_alac::packet_frames(d->config, packet, len, &frames)) return fail("ALAC packet: " + std::string(sk_strerror(rc)));
    if ((size_t)frames * d->config.channels * (d->config.bit_depth / 8u) > out_cap) return SK_ERR_CAPACITY;
    const sk_alac_packet one{0, (uint32_t)len};
    int32_t status = 0;
    uint32_t got = 0;
    const int rc = alac_decode_packets(d->eng, &d->config, &one, 1, packet, 0, false, out, out_cap, out_len, &status, &got, nullptr);
    if (rc != SK_OK) return rc;
    if (status != SK_OK) {
        *out_len = 0;
        return fail("ALAC packet: " + std::string(sk_strerror(status)));
    }
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_alac_packet_decoder_decode_packet");
}

const char *sk_alac_packet_decoder_last_error(const sk_alac_packet_decoder *d) try {
    sk::abi_enter();
    return d ? d->error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_alac_packet_decoder_last_error");
    return "";
}

}  // extern "C"

// ---- Telephony: G.711, G.722, G.726 (g72x_stream.h, g72x_decode.hip) --------------------------------------------------------------

struct sk_g72x_decoder {
    sk_engine *eng = nullptr;
    int codec = SK_G726;
    uint32_t sample_rate = 8000, channels = 1, g726_rate = 32000;
    int packing = SK_G726_LEFT;
    sk_g726_state s726{};
    sk_g722_state s722{};
    sk_g72x::G726Framer framer;
    std::vector<uint8_t> bytes;  // what a call decodes
    std::vector<int16_t> pcm;    // decode_i32 / decode_f32: the s16 they follow from
    std::string error;
};

namespace {

static_assert(sizeof(sk_g726_state) == sk::kG726StateWords * 4 && sizeof(sk_g722_state) == sk::kG722StateWords * 4, "the states are the device records");

size_t g72x_up16(size_t v) { return (v + 15) & ~(size_t)15; }

// What one launch sequence of the stage works on.  begin() a stream, then unit() for each of its units in order.  The state records go
// in with the streams and come back into the same vectors; the batch must live until the stream has been waited for.
struct G72xBatch {
    std::vector<sk::G72xStream> s726, s722;
    std::vector<sk::G72xUnit> units;
    std::vector<sk::AiffElemJob> g711;
    std::vector<int32_t> st726, st722;
    uint32_t g711_max = 0, g722_max = 0;
    uint64_t ws_words = 0;
    int codec = 0;

    void begin(int c, int bits, int packing, const void *state) {
        codec = c;
        if (c != SK_G722 && c != SK_G726) return;
        sk::G72xStream s{};
        s.first_unit = (uint32_t)units.size(), s.bits = (uint8_t)bits, s.packing = (uint8_t)packing;
        const int32_t *w = (const int32_t *)state;
        if (c == SK_G726) {
            s.state = (uint32_t)s726.size();
            s726.push_back(s);
            st726.insert(st726.end(), w, w + sk::kG726StateWords);
        } else {
            s.state = (uint32_t)s722.size(), s.ws_offset = (uint32_t)ws_words;
            s722.push_back(s);
            st722.insert(st722.end(), w, w + sk::kG722StateWords);
        }
    }
    void unit(const uint8_t *src, uint8_t *dst, uint32_t bytes) {
        if (codec == SK_G711_ULAW || codec == SK_G711_ALAW) {
            if (bytes == 0) return;
            g711.push_back(sk::AiffElemJob{src, dst, bytes, (uint32_t)(codec == SK_G711_ULAW ? SK_AIFF_ULAW : SK_AIFF_ALAW)});
            g711_max = std::max(g711_max, bytes);
            return;
        }
        units.push_back(sk::G72xUnit{src, dst, bytes, 0});
        sk::G72xStream &s = codec == SK_G726 ? s726.back() : s722.back();
        s.n_units += 1;
        if (codec == SK_G722) s.total_bytes += bytes, ws_words += bytes, g722_max = std::max(g722_max, s.total_bytes);
    }
    // the device form of the tables: streams | units | G.711 jobs | records in | records out
    static size_t tables_bound(size_t n_streams, size_t n_units) {
        return 2 * g72x_up16(n_streams * sizeof(sk::G72xStream)) + g72x_up16(n_units * sizeof(sk::G72xUnit)) + g72x_up16(n_units * sizeof(sk::AiffElemJob)) +
               4 * g72x_up16(n_streams * sk::kG722StateWords * 4);
    }
};

// uploads the tables to d_tab (tables_bound of the batch's counts), runs the launches with the workspace at d_ws (ws_words words) and
// asks for the records back; everything on e->stream, nothing waited for
int g72x_launch(sk_engine *e, G72xBatch &b, uint8_t *d_tab, uint32_t *d_ws) {
    size_t at = 0;
    const auto place = [&](size_t bytes) {
        uint8_t *d = d_tab + at;
        at += g72x_up16(bytes);
        return d;
    };
    uint8_t *d_units = place(b.units.size() * sizeof(sk::G72xUnit));
    if (!b.units.empty())
        SK_HIP(hipMemcpyAsync(d_units, b.units.data(), b.units.size() * sizeof(sk::G72xUnit), hipMemcpyHostToDevice, e->stream), "H2D g72x units");
    if (!b.g711.empty()) {
        uint8_t *d_jobs = place(b.g711.size() * sizeof(sk::AiffElemJob));
        SK_HIP(hipMemcpyAsync(d_jobs, b.g711.data(), b.g711.size() * sizeof(sk::AiffElemJob), hipMemcpyHostToDevice, e->stream), "H2D g711 jobs");
        SK_HIP(sk::launch_aiff_elem((const sk::AiffElemJob *)d_jobs, (uint32_t)b.g711.size(), b.g711_max, e->stream), "launch g711 expand");
    }
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<sk::G72xStream> &streams = pass ? b.s722 : b.s726;
        std::vector<int32_t> &records = pass ? b.st722 : b.st726;
        if (streams.empty()) continue;
        uint8_t *d_streams = place(streams.size() * sizeof(sk::G72xStream));
        int32_t *d_in = (int32_t *)place(records.size() * 4), *d_out = (int32_t *)place(records.size() * 4);
        SK_HIP(hipMemcpyAsync(d_streams, streams.data(), streams.size() * sizeof(sk::G72xStream), hipMemcpyHostToDevice, e->stream), "H2D g72x streams");
        SK_HIP(hipMemcpyAsync(d_in, records.data(), records.size() * 4, hipMemcpyHostToDevice, e->stream), "H2D g72x states");
        if (pass)
            SK_HIP(sk::launch_g722((const sk::G72xStream *)d_streams, (uint32_t)streams.size(), (const sk::G72xUnit *)d_units, d_in, d_out, d_ws, b.g722_max,
                                   e->stream), "launch g722");
        else
            SK_HIP(sk::launch_g726((const sk::G72xStream *)d_streams, (uint32_t)streams.size(), (const sk::G72xUnit *)d_units, d_in, d_out, e->stream),
                   "launch g726");
        SK_HIP(hipMemcpyAsync(records.data(), d_out, records.size() * 4, hipMemcpyDeviceToHost, e->stream), "D2H g72x states");
    }
    return SK_OK;
}

void g72x_text(char *error, size_t cap, const std::string &text) {
    if (!error || cap == 0) return;
    const size_t n = std::min(cap - 1, text.size());
    std::memcpy(error, text.data(), n);
    error[n] = 0;
}

// the stream rows' checks shared by the batch and the tick; bits = 0 for the codecs without a rate
bool g72x_row_ok(int codec, uint32_t g726_rate, int packing, int *bits) {
    *bits = 0;
    if (codec < 0 || codec >= sk_g72x::kCodecs) return false;
    if (codec != SK_G726) return true;
    *bits = sk_g72x::g726_bits(g726_rate);
    return *bits != 0 && (packing == SK_G726_LEFT || packing == SK_G726_RIGHT);
}

// sk_g72x_decode_batch[_dev]
int g72x_decode_batch(sk_engine *e, const sk_g72x_stream *streams, uint32_t n_streams, sk_g72x_unit *units, uint32_t n_units, const uint8_t *bytes,
                      size_t bytes_len, bool on_device, uint8_t *out, size_t out_cap, size_t *out_len, sk_g726_state *s726, uint32_t n726, sk_g722_state *s722,
                      uint32_t n722) {
    if (!e || !out_len || (n_streams && !streams) || (n_units && !units) || (bytes_len && !bytes) || (n726 && !s726) || (n722 && !s722)) return SK_ERR_INVALID_ARG;
    *out_len = 0;
    if (bytes_len > 0x7fffffffull) return SK_ERR_INVALID_ARG;
    if (on_device && (((uintptr_t)bytes | (uintptr_t)out) & 15)) return SK_ERR_INVALID_ARG;
    // ---- the table, and where every unit's samples go ----
    std::vector<uint8_t> named726(n726, 0), named722(n722, 0);
    std::vector<int> bits_of(n_streams, 0);
    std::vector<uint64_t> out_at(n_units, 0);
    std::vector<uint32_t> out_bytes(n_units, 0);
    uint64_t at = 0, cursor = 0, need = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        const sk_g72x_stream &s = streams[i];
        if (!g72x_row_ok(s.codec, s.g726_rate, s.g726_packing, &bits_of[i])) return SK_ERR_INVALID_ARG;
        if (s.codec == SK_G726 && (s.state >= n726 || named726[s.state]++)) return SK_ERR_INVALID_ARG;
        if (s.codec == SK_G722 && (s.state >= n722 || named722[s.state]++)) return SK_ERR_INVALID_ARG;
        if (at + s.n_units > n_units) return SK_ERR_INVALID_ARG;
        const uint32_t group = sk_g72x::group_bytes(s.codec, bits_of[i]);
        for (uint32_t u = 0; u < s.n_units; ++u) {
            const sk_g72x_unit &un = units[at + u];
            if (un.offset % 16 || un.size % group || un.offset > bytes_len || un.size > bytes_len - un.offset) return SK_ERR_INVALID_ARG;
            const uint64_t samples = sk_g72x::samples_of(s.codec, bits_of[i], un.size);
            if (samples > sk_g72x::kScratchSamples) return SK_ERR_INVALID_ARG;
            out_at[at + u] = cursor, out_bytes[at + u] = (uint32_t)(samples * 2);
            if (samples) need = cursor + samples * 2;
            cursor += g72x_up16((size_t)samples * 2);
        }
        at += s.n_units;
    }
    if (at != n_units || need > out_cap || (need && !out)) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    const uint8_t *d_src = bytes;
    uint8_t *d_dst = out;
    if (!on_device) {
        SK_HIP(e->in_buf.reserve(bytes_len + 64), "alloc staging");
        SK_HIP(e->out_buf.reserve((size_t)cursor + 64), "alloc staging");
        if (bytes_len) SK_HIP(hipMemcpyAsync(e->in_buf.p, bytes, bytes_len, hipMemcpyHostToDevice, e->stream), "H2D g72x bytes");
        if (n_units > 1 && need) SK_HIP(hipMemsetAsync(e->out_buf.p, 0, (size_t)need, e->stream), "clear g72x staging");
        d_src = (const uint8_t *)e->in_buf.p, d_dst = (uint8_t *)e->out_buf.p;
    }
    G72xBatch b;
    at = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        const sk_g72x_stream &s = streams[i];
        b.begin(s.codec, bits_of[i], s.g726_packing, s.codec == SK_G726 ? (const void *)&s726[s.state] : (s.codec == SK_G722 ? (const void *)&s722[s.state] : nullptr));
        for (uint32_t u = 0; u < s.n_units; ++u) b.unit(d_src + units[at + u].offset, d_dst + out_at[at + u], units[at + u].size);
        at += s.n_units;
    }
    SK_HIP(e->g72x_tab.reserve(G72xBatch::tables_bound(n_streams, n_units) + 64), "alloc g72x tables");
    SK_HIP(e->g72x_ws.reserve((size_t)b.ws_words * 4 + 64), "alloc g72x workspace");
    int rc = g72x_launch(e, b, (uint8_t *)e->g72x_tab.p, (uint32_t *)e->g72x_ws.p);
    if (rc == SK_OK && !on_device && need) {
        // one copy up to the end of the last unit's samples (a copy per unit costs 12 us each: 50 ms at 4096 units); the alignment
        // gaps between the units were cleared with the staging buffer
        const hipError_t err = hipMemcpyAsync(out, d_dst, (size_t)need, hipMemcpyDeviceToHost, e->stream);
        if (err != hipSuccess) rc = e->hip_fail(err, "D2H g72x");
    }
    const hipError_t waited = hipStreamSynchronize(e->stream);  // the tables leave scope with the call
    if (rc != SK_OK) return rc;
    SK_HIP(waited, "g72x sync");
    for (uint32_t i = 0, k6 = 0, k2 = 0; i < n_streams; ++i) {
        if (streams[i].codec == SK_G726) std::memcpy(&s726[streams[i].state], &b.st726[(size_t)k6++ * sk::kG726StateWords], sizeof(sk_g726_state));
        if (streams[i].codec == SK_G722) std::memcpy(&s722[streams[i].state], &b.st722[(size_t)k2++ * sk::kG722StateWords], sizeof(sk_g722_state));
    }
    for (uint32_t k = 0; k < n_units; ++k) units[k].out_offset = out_at[k], units[k].out_len = out_bytes[k];
    *out_len = (size_t)need;
    return SK_OK;
}

// sk_g72x_decode[_dev]: a table of one stream with one unit
int g72x_decode_one(sk_engine *e, int codec, uint32_t rate, int packing, const uint8_t *bytes, size_t len, bool on_device, uint8_t *out, size_t out_cap,
                    size_t *out_len, void *state, char *error, size_t error_cap) {
    g72x_text(error, error_cap, "");
    int bits = 0;
    if (!e || !out_len || !g72x_row_ok(codec, rate, packing, &bits) || (len && !bytes) || ((codec == SK_G726 || codec == SK_G722) && !state)) return SK_ERR_INVALID_ARG;
    *out_len = 0;
    if (len > 0x7fffffffull || len % sk_g72x::group_bytes(codec, bits)) return SK_ERR_INVALID_ARG;
    std::string text;
    if (!sk_g72x::fits_scratch(codec, sk_g72x::samples_of(codec, bits, len), &text)) {
        g72x_text(error, error_cap, text);
        return SK_G72X_ERR_STREAM;
    }
    sk_g72x_stream s{};
    s.codec = (uint8_t)codec, s.g726_packing = (uint8_t)packing, s.g726_rate = rate, s.n_units = 1, s.state = 0;
    sk_g72x_unit u{};
    u.size = (uint32_t)len;
    return g72x_decode_batch(e, &s, 1, &u, 1, bytes, len, on_device, out, out_cap, out_len, (sk_g726_state *)state, codec == SK_G726 ? 1 : 0,
                             (sk_g722_state *)state, codec == SK_G722 ? 1 : 0);
}

// sk_tick_run_g72x / sk_tick_g72x_out_bound_on: checks the table and derives what the PCM tick's body works on, as aiff_tick_derive does --
// per stream an s16le source, per unit where its decoded samples lie (16-byte aligned, unit after unit) -- and the decode that stands in
// front of the body: one launch sequence of the stage over the units of each pass.
struct G72xDerived {
    std::vector<sk_pcm_tick_stream> ts;
    std::vector<sk_pcm_unit> units;  // the decoded layout
    std::vector<uint32_t> first;     // per stream: its first unit
    std::vector<int> bits;
    AiffTick tick;
    G72xBatch batch[2];              // streams that go on through the body, streams delivered as decoded: alive until the tick's last wait
    std::vector<uint32_t> of[2][2];  // [pass][0: G.726, 1: G.722]: record of the batch -> index into the stream table
    size_t part = 0;                 // of g72x_tab per pass
    uint64_t ws_words = 0;
};

int g72x_tick_derive(const sk_g72x_tick_stream *gs, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units, size_t bytes_len, bool records,
                     uint32_t n726, uint32_t n722, G72xDerived &d) {
    d.ts.assign(n_streams, sk_pcm_tick_stream{});
    d.units.assign(n_units, sk_pcm_unit{});
    d.first.assign(n_streams, 0);
    d.bits.assign(n_streams, 0);
    d.tick.plain.assign(n_streams, 0);
    d.tick.states.assign((size_t)n_streams * 2, 0);
    // (the bound is asked for without the records: nothing is named then)
    std::vector<uint8_t> named726(records ? n726 : 0, 0), named722(records ? n722 : 0, 0);
    uint64_t at = 0, cursor = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        const sk_g72x_tick_stream &g = gs[i];
        if (!g72x_row_ok(g.codec, g.g726_rate, g.g726_packing, &d.bits[i])) return SK_ERR_INVALID_ARG;
        const bool g711 = g.codec == SK_G711_ULAW || g.codec == SK_G711_ALAW;
        if (g.channels == 0 || (!g711 && g.channels != 1)) return SK_ERR_INVALID_ARG;
        if (records && g.codec == SK_G726 && (g.state >= n726 || named726[g.state]++)) return SK_ERR_INVALID_ARG;
        if (records && g.codec == SK_G722 && (g.state >= n722 || named722[g.state]++)) return SK_ERR_INVALID_ARG;
        sk_pcm_tick_stream &t = d.ts[i];
        t.stream = g.stream, t.n_units = g.n_units, t.channels = g.channels, t.out_bits = g.out_bits, t.out_channels = g.out_channels;
        t.resample = g.resample, t.flush = g.flush, t.format = SK_FMT_S16LE;
        d.tick.plain[i] = !g.resample && g.out_bits == 16 && g.out_channels == g.channels;
        d.first[i] = (uint32_t)at;
        if (at + g.n_units > n_units) return SK_ERR_INVALID_ARG;
        const uint32_t group = sk_g72x::group_bytes(g.codec, d.bits[i]);
        for (uint32_t u = 0; u < g.n_units; ++u) {
            const sk_pcm_unit &un = units[at + u];
            if (un.byte_offset % 16 || un.byte_len == 0 || un.byte_len % group) return SK_ERR_INVALID_ARG;
            if (un.byte_offset > bytes_len || un.byte_len > bytes_len - un.byte_offset) return SK_ERR_INVALID_ARG;
            const uint64_t samples = sk_g72x::samples_of(g.codec, d.bits[i], un.byte_len);
            if (samples > sk_g72x::kScratchSamples) return SK_ERR_INVALID_ARG;
            d.units[at + u] = sk_pcm_unit{cursor, (uint32_t)(samples * 2), 0};
            cursor += g72x_up16((size_t)samples * 2);
            if (g.codec == SK_G722) d.ws_words += un.byte_len;
        }
        at += g.n_units;
    }
    if (cursor > 0x7fffffffull || (bytes_len > 0x7fffffffull && bytes_len != (size_t)-1)) return SK_ERR_INVALID_ARG;
    d.tick.decoded_len = (size_t)cursor;
    d.part = G72xBatch::tables_bound(n_streams, n_units) + 64;
    return at == n_units ? SK_OK : SK_ERR_INVALID_ARG;
}

// one pass of the decode in front of the body: the units of the streams whose `plain` is as_is, each to where dst_of puts it
int g72x_tick_decode(sk_engine *e, const sk_g72x_tick_stream *gs, const sk_pcm_unit *units, const sk_g726_state *s726, const sk_g722_state *s722,
                     G72xDerived &d, bool as_is, const std::function<uint8_t *(uint32_t, uint32_t)> &dst_of, const uint8_t *d_src) {
    const int p = as_is ? 1 : 0;
    G72xBatch &b = d.batch[p];
    for (uint32_t i = 0; i < (uint32_t)d.ts.size(); ++i) {
        if ((d.tick.plain[i] != 0) != as_is || d.ts[i].n_units == 0) continue;
        const sk_g72x_tick_stream &g = gs[i];
        b.begin(g.codec, d.bits[i], g.g726_packing, g.codec == SK_G726 ? (const void *)&s726[g.state] : (g.codec == SK_G722 ? (const void *)&s722[g.state] : nullptr));
        if (g.codec == SK_G726) d.of[p][0].push_back(i);
        if (g.codec == SK_G722) d.of[p][1].push_back(i);
        for (uint32_t u = 0; u < g.n_units; ++u) b.unit(d_src + units[d.first[i] + u].byte_offset, dst_of(i, u), units[d.first[i] + u].byte_len);
    }
    if (b.units.empty() && b.g711.empty()) return SK_OK;
    // both passes' tables have their own part of g72x_tab; the workspace is shared, the passes follow each other on the stream
    SK_HIP(e->g72x_tab.reserve(2 * d.part), "alloc tick g72x tables");
    SK_HIP(e->g72x_ws.reserve((size_t)d.ws_words * 4 + 64), "alloc tick g72x workspace");
    return g72x_launch(e, b, (uint8_t *)e->g72x_tab.p + (size_t)p * d.part, (uint32_t *)e->g72x_ws.p);
}

int g72x_decoder_fail(sk_g72x_decoder *d, int rc, const std::string &text) {
    d->error = text;
    return rc;
}

// decode_i16 of the three Decoder objects: `written` samples into out (cap samples)
int g72x_decoder_decode(sk_g72x_decoder *d, const uint8_t *input, size_t len, int16_t *out, size_t out_cap, size_t *written) {
    if (!d || (len && !input) || !written || (out_cap && !out)) return SK_ERR_INVALID_ARG;
    *written = 0;
    const int bits = d->codec == SK_G726 ? sk_g72x::g726_bits(d->g726_rate) : 0;
    const size_t take = d->codec == SK_G726 ? d->framer.ready(len) : len;
    const uint64_t samples = sk_g72x::samples_of(d->codec, bits, take);
    if (samples > out_cap)
        return g72x_decoder_fail(d, SK_ERR_CAPACITY, std::string("Output buffer too small for ") + sk_g72x::codec_name(d->codec) + " decode: need " +
                                                         std::to_string(samples) + ", have " + std::to_string(out_cap));
    if (samples > 0x3fffffffull) return SK_ERR_INVALID_ARG;
    const uint8_t *src = input;
    sk_g72x::G726Framer after = d->framer;  // the framer moves on only when the decode succeeds
    if (d->codec == SK_G726) {
        d->bytes.clear();
        after.add(input, len, d->bytes);  // nothing completes a group: the bytes wait, nothing is decoded
        src = d->bytes.data();
    }
    // a Decoder object is not the pipeline: its output is the caller's, so a call may exceed the pipeline's scratch -- in pieces of
    // whole groups, the carry handed from piece to piece and kept only when all of them decoded
    sk_g72x_stream s{};
    s.codec = (uint8_t)d->codec, s.g726_packing = (uint8_t)d->packing, s.g726_rate = d->g726_rate, s.n_units = 1;
    sk_g726_state st726 = d->s726;
    sk_g722_state st722 = d->s722;
    const size_t piece = sk_g72x::kScratchSamples / sk_g72x::group_samples(d->codec, bits) * sk_g72x::group_bytes(d->codec, bits);
    size_t done = 0, got = 0;
    while (done < take) {
        const size_t n = std::min(piece, take - done);
        sk_g72x_unit u{};
        u.size = (uint32_t)n;
        size_t out_len = 0;
        const int rc = g72x_decode_batch(d->eng, &s, 1, &u, 1, src + done, n, false, (uint8_t *)(out + got), (out_cap - got) * 2, &out_len,
                                         d->codec == SK_G726 ? &st726 : nullptr, d->codec == SK_G726 ? 1 : 0, d->codec == SK_G722 ? &st722 : nullptr,
                                         d->codec == SK_G722 ? 1 : 0);
        if (rc != SK_OK) return rc;
        done += n, got += out_len / 2;
    }
    d->s726 = st726, d->s722 = st722, d->framer = after;
    *written = got;
    return SK_OK;
}

// decode_i32 / decode_f32: the s16 decode into the decoder's own buffer, then `widen` sample for sample
template <typename T, typename F>
int g72x_decoder_decode_as(sk_g72x_decoder *d, const uint8_t *input, size_t len, T *out, size_t out_cap, size_t *written, F widen) {
    if (!d || !written || (out_cap && !out)) return SK_ERR_INVALID_ARG;
    d->pcm.resize(out_cap);
    const int rc = g72x_decoder_decode(d, input, len, d->pcm.data(), out_cap, written);
    if (rc != SK_OK) return rc;
    for (size_t i = 0; i < *written; ++i) out[i] = widen(d->pcm[i]);
    return SK_OK;
}

}  // namespace

extern "C" {

void sk_g726_state_init(sk_g726_state *s) try {
    sk::abi_enter();
    if (s) sk_g72x::init_state(s);
} catch (...) {
    (void)sk::abi_caught("sk_g726_state_init");
}

void sk_g722_state_init(sk_g722_state *s) try {
    sk::abi_enter();
    if (s) sk_g72x::init_state(s);
} catch (...) {
    (void)sk::abi_caught("sk_g722_state_init");
}

int sk_g72x_decode(sk_engine *e, int codec, uint32_t g726_rate, int g726_packing, const uint8_t *bytes, size_t len, uint8_t *out, size_t out_cap,
                   size_t *out_len, void *state, char *error, size_t error_cap) try {
    sk::abi_enter();
    return g72x_decode_one(e, codec, g726_rate, g726_packing, bytes, len, false, out, out_cap, out_len, state, error, error_cap);
} catch (...) {
    return sk::abi_caught("sk_g72x_decode");
}

int sk_g72x_decode_dev(sk_engine *e, int codec, uint32_t g726_rate, int g726_packing, const uint8_t *d_bytes, size_t len, uint8_t *d_out, size_t out_cap,
                       size_t *out_len, void *state, char *error, size_t error_cap) try {
    sk::abi_enter();
    return g72x_decode_one(e, codec, g726_rate, g726_packing, d_bytes, len, true, d_out, out_cap, out_len, state, error, error_cap);
} catch (...) {
    return sk::abi_caught("sk_g72x_decode_dev");
}

int sk_g72x_decode_batch(sk_engine *e, const sk_g72x_stream *streams, uint32_t n_streams, sk_g72x_unit *units, uint32_t n_units, const uint8_t *bytes,
                         size_t bytes_len, uint8_t *out, size_t out_cap, size_t *out_len, sk_g726_state *g726_states, uint32_t n_g726_states,
                         sk_g722_state *g722_states, uint32_t n_g722_states) try {
    sk::abi_enter();
    return g72x_decode_batch(e, streams, n_streams, units, n_units, bytes, bytes_len, false, out, out_cap, out_len, g726_states, n_g726_states, g722_states,
                             n_g722_states);
} catch (...) {
    return sk::abi_caught("sk_g72x_decode_batch");
}

int sk_g72x_decode_batch_dev(sk_engine *e, const sk_g72x_stream *streams, uint32_t n_streams, sk_g72x_unit *units, uint32_t n_units, const uint8_t *d_bytes,
                             size_t bytes_len, uint8_t *d_out, size_t out_cap, size_t *out_len, sk_g726_state *g726_states, uint32_t n_g726_states,
                             sk_g722_state *g722_states, uint32_t n_g722_states) try {
    sk::abi_enter();
    return g72x_decode_batch(e, streams, n_streams, units, n_units, d_bytes, bytes_len, true, d_out, out_cap, out_len, g726_states, n_g726_states, g722_states,
                             n_g722_states);
} catch (...) {
    return sk::abi_caught("sk_g72x_decode_batch_dev");
}

size_t sk_tick_g72x_out_bound_on(sk_engine *e, const sk_g72x_tick_stream *gs, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units,
                                 uint32_t *max_outputs) try {
    sk::abi_enter();
    if (max_outputs) *max_outputs = 0;
    if (!e || (!gs && n_streams) || (!units && n_units)) return 0;
    G72xDerived d;
    if (g72x_tick_derive(gs, n_streams, units, n_units, (size_t)-1, false, 0, 0, d) != SK_OK) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return tick_pcm_out_bound(e, d.ts.data(), n_streams, d.units.data(), n_units, max_outputs, d.tick.plain.data());
} catch (...) {
    (void)sk::abi_caught("sk_tick_g72x_out_bound_on");
    return 0;
}

int sk_tick_run_g72x(sk_engine *e, const sk_g72x_tick_stream *gs, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units, const uint8_t *bytes,
                     size_t bytes_len, uint8_t *out, size_t out_cap, sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes,
                     sk_g726_state *g726_states, uint32_t n_g726_states, sk_g722_state *g722_states, uint32_t n_g722_states) try {
    sk::abi_enter();
    if (!e || !n_outs || (n_streams && !gs) || (n_units && (!units || !bytes)) || (n_g726_states && !g726_states) || (n_g722_states && !g722_states))
        return SK_ERR_INVALID_ARG;
    *n_outs = 0;
    if (out_bytes) *out_bytes = 0;
    G72xDerived d;
    int rc = g72x_tick_derive(gs, n_streams, units, n_units, bytes_len, true, n_g726_states, n_g722_states, d);
    if (rc != SK_OK) return rc;
    d.tick.decode = [&](bool as_is, const std::function<uint8_t *(uint32_t, uint32_t)> &dst_of, const uint8_t *d_src) {
        return g72x_tick_decode(e, gs, units, g726_states, g722_states, d, as_is, dst_of, d_src);
    };
    rc = tick_pcm_impl(e, d.ts.data(), n_streams, d.units.data(), n_units, bytes, bytes_len, out, out_cap, outs, outs_cap, n_outs, out_bytes, &d.tick);
    if (rc != SK_OK) return rc;  // the carries are the caller's records: untouched
    for (int p = 0; p < 2; ++p) {
        for (size_t k = 0; k < d.of[p][0].size(); ++k)
            std::memcpy(&g726_states[gs[d.of[p][0][k]].state], &d.batch[p].st726[k * sk::kG726StateWords], sizeof(sk_g726_state));
        for (size_t k = 0; k < d.of[p][1].size(); ++k)
            std::memcpy(&g722_states[gs[d.of[p][1][k]].state], &d.batch[p].st722[k * sk::kG722StateWords], sizeof(sk_g722_state));
    }
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_tick_run_g72x");
}

int sk_g711_decoder_create(sk_engine *e, int law, uint32_t sample_rate, uint32_t channels, sk_g72x_decoder **out, char *error, size_t error_cap) try {
    sk::abi_enter();
    if (!e || !out || (law != SK_G711_ULAW && law != SK_G711_ALAW)) return SK_ERR_INVALID_ARG;
    *out = nullptr;
    g72x_text(error, error_cap, "");
    std::string text;
    if (!sk_g72x::check_g711(sample_rate, channels, &text)) {
        g72x_text(error, error_cap, text);
        return SK_G72X_ERR_STREAM;
    }
    std::unique_ptr<sk_g72x_decoder> d(new sk_g72x_decoder());
    d->eng = e, d->codec = law, d->sample_rate = sample_rate, d->channels = channels;
    *out = d.release();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_g711_decoder_create");
}

int sk_g722_decoder_create(sk_engine *e, sk_g72x_decoder **out) try {
    sk::abi_enter();
    if (!e || !out) return SK_ERR_INVALID_ARG;
    std::unique_ptr<sk_g72x_decoder> d(new sk_g72x_decoder());
    d->eng = e, d->codec = SK_G722, d->sample_rate = 16000, d->channels = 1;
    *out = d.release();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_g722_decoder_create");
}

int sk_g726_decoder_create(sk_engine *e, uint32_t g726_rate, int g726_packing, sk_g72x_decoder **out) try {
    sk::abi_enter();
    int bits = 0;
    if (!e || !out || !g72x_row_ok(SK_G726, g726_rate, g726_packing, &bits)) return SK_ERR_INVALID_ARG;
    std::unique_ptr<sk_g72x_decoder> d(new sk_g72x_decoder());
    d->eng = e, d->codec = SK_G726, d->sample_rate = 8000, d->channels = 1, d->g726_rate = g726_rate, d->packing = g726_packing;
    d->framer = sk_g72x::G726Framer(bits);
    sk_g726_state_init(&d->s726);
    *out = d.release();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_g726_decoder_create");
}

void sk_g72x_decoder_destroy(sk_g72x_decoder *d) try {
    sk::abi_enter();
    delete d;
} catch (...) {
    (void)sk::abi_caught("sk_g72x_decoder_destroy");
}

int sk_g72x_decoder_info(const sk_g72x_decoder *d, int *codec, uint32_t *sample_rate, uint32_t *channels) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    if (codec) *codec = d->codec;
    if (sample_rate) *sample_rate = d->sample_rate;
    if (channels) *channels = d->channels;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_g72x_decoder_info");
}

int sk_g72x_decoder_decode_i16(sk_g72x_decoder *d, const uint8_t *input, size_t len, int16_t *out, size_t out_cap, size_t *written) try {
    sk::abi_enter();
    return g72x_decoder_decode(d, input, len, out, out_cap, written);
} catch (...) {
    return sk::abi_caught("sk_g72x_decoder_decode_i16");
}

int sk_g72x_decoder_decode_i32(sk_g72x_decoder *d, const uint8_t *input, size_t len, int32_t *out, size_t out_cap, size_t *written) try {
    sk::abi_enter();
    return g72x_decoder_decode_as(d, input, len, out, out_cap, written, [](int16_t v) { return (int32_t)((uint32_t)(int32_t)v << 16); });
} catch (...) {
    return sk::abi_caught("sk_g72x_decoder_decode_i32");
}

int sk_g72x_decoder_decode_f32(sk_g72x_decoder *d, const uint8_t *input, size_t len, float *out, size_t out_cap, size_t *written) try {
    sk::abi_enter();
    return g72x_decoder_decode_as(d, input, len, out, out_cap, written, [](int16_t v) { return (float)v / 32768.0f; });
} catch (...) {
    return sk::abi_caught("sk_g72x_decoder_decode_f32");
}

int sk_g726_decoder_flush(sk_g72x_decoder *d) try {
    sk::abi_enter();
    if (!d || d->codec != SK_G726) return SK_ERR_INVALID_ARG;
    std::string text;
    if (d->framer.flush(&text)) return SK_OK;
    return g72x_decoder_fail(d, SK_G72X_ERR_STREAM, text);
} catch (...) {
    return sk::abi_caught("sk_g726_decoder_flush");
}

int sk_g72x_decoder_reset(sk_g72x_decoder *d) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    sk_g726_state_init(&d->s726);
    sk_g722_state_init(&d->s722);
    d->framer.pending.clear();
    d->error.clear();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_g72x_decoder_reset");
}

const char *sk_g72x_decoder_last_error(const sk_g72x_decoder *d) try {
    sk::abi_enter();
    return d ? d->error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_g72x_decoder_last_error");
    return "";
}

}  // extern "C"

// ---- Telephony: GSM 06.10 full rate (gsm_stream.h, gsm_decode.hip) -----------------------------------------------------------------

struct sk_gsm_decoder {
    sk_engine *eng = nullptr;
    int variant = SK_GSM_STANDARD;
    sk_gsm_state state{};
    sk_gsm::Framer framer;
    std::vector<uint8_t> bytes;  // what a call decodes
    std::vector<int16_t> pcm;    // decode_i32 / decode_f32: the s16 they follow from
    std::string error;
};

namespace {

static_assert(sizeof(sk_gsm_state) == sk::kGsmStateWords * 4, "the state is the device record");

// What one launch sequence of the stage works on.  begin() a stream, then unit() for each of its units in order.  The state records go
// in with the streams and come back into the same vector; the batch must live until the stream has been waited for.
struct GsmBatch {
    std::vector<sk::GsmStream> streams;
    std::vector<sk::GsmUnit> units;
    std::vector<int32_t> states;
    uint64_t ws_samples = 0;

    void begin(int variant, const sk_gsm_state *state) {
        sk::GsmStream s{};
        s.first_unit = (uint32_t)units.size(), s.state = (uint32_t)streams.size(), s.ws_offset = (uint32_t)ws_samples;
        s.base_bit = sk_gsm::base_bit(variant), s.stride_bits = sk_gsm::stride_bits(variant);
        streams.push_back(s);
        const int32_t *w = (const int32_t *)state;
        states.insert(states.end(), w, w + sk::kGsmStateWords);
    }
    void unit(int variant, const uint8_t *src, uint8_t *dst, uint32_t bytes) {
        const uint32_t frames = (uint32_t)(sk_gsm::samples_of(variant, bytes) / sk_gsm::kFrameSamples);
        units.push_back(sk::GsmUnit{src, dst, bytes, frames});
        streams.back().n_units += 1;
        ws_samples += (uint64_t)frames * sk_gsm::kFrameSamples;
    }
    // the device form of the tables: streams | units | records in | records out
    static size_t tables_bound(size_t n_streams, size_t n_units) {
        return g72x_up16(n_streams * sizeof(sk::GsmStream)) + g72x_up16(n_units * sizeof(sk::GsmUnit)) + 2 * g72x_up16(n_streams * sk::kGsmStateWords * 4);
    }
};

// uploads the tables to d_tab (tables_bound of the batch's counts), runs the two kernels with the workspace at d_ws (ws_samples s16)
// and asks for the records back; everything on e->stream, nothing waited for
int gsm_launch(sk_engine *e, GsmBatch &b, uint8_t *d_tab, int16_t *d_ws) {
    if (b.streams.empty()) return SK_OK;
    size_t at = 0;
    const auto place = [&](size_t bytes) {
        uint8_t *d = d_tab + at;
        at += g72x_up16(bytes);
        return d;
    };
    uint8_t *d_streams = place(b.streams.size() * sizeof(sk::GsmStream));
    uint8_t *d_units = place(b.units.size() * sizeof(sk::GsmUnit));
    int32_t *d_in = (int32_t *)place(b.states.size() * 4), *d_out = (int32_t *)place(b.states.size() * 4);
    SK_HIP(hipMemcpyAsync(d_streams, b.streams.data(), b.streams.size() * sizeof(sk::GsmStream), hipMemcpyHostToDevice, e->stream), "H2D gsm streams");
    if (!b.units.empty())
        SK_HIP(hipMemcpyAsync(d_units, b.units.data(), b.units.size() * sizeof(sk::GsmUnit), hipMemcpyHostToDevice, e->stream), "H2D gsm units");
    SK_HIP(hipMemcpyAsync(d_in, b.states.data(), b.states.size() * 4, hipMemcpyHostToDevice, e->stream), "H2D gsm states");
    SK_HIP(sk::launch_gsm((const sk::GsmStream *)d_streams, (uint32_t)b.streams.size(), (const sk::GsmUnit *)d_units, d_in, d_out, d_ws, e->stream), "launch gsm");
    SK_HIP(hipMemcpyAsync(b.states.data(), d_out, b.states.size() * 4, hipMemcpyDeviceToHost, e->stream), "D2H gsm states");
    return SK_OK;
}

// sk_gsm_decode_batch[_dev]
int gsm_decode_batch(sk_engine *e, const sk_gsm_stream *streams, uint32_t n_streams, sk_g72x_unit *units, uint32_t n_units, const uint8_t *bytes,
                     size_t bytes_len, bool on_device, uint8_t *out, size_t out_cap, size_t *out_len, sk_gsm_state *states, uint32_t n_states) {
    if (!e || !out_len || (n_streams && (!streams || !states)) || (n_units && !units) || (bytes_len && !bytes)) return SK_ERR_INVALID_ARG;
    *out_len = 0;
    if (bytes_len > 0x7fffffffull) return SK_ERR_INVALID_ARG;
    if (on_device && (((uintptr_t)bytes | (uintptr_t)out) & 15)) return SK_ERR_INVALID_ARG;
    // ---- the table, and where every unit's samples go ----
    std::vector<uint8_t> named(n_states, 0);
    std::vector<uint64_t> out_at(n_units, 0);
    std::vector<uint32_t> out_bytes(n_units, 0);
    uint64_t at = 0, cursor = 0, need = 0;
    bool rejected = false;
    for (uint32_t i = 0; i < n_streams; ++i) {
        const sk_gsm_stream &s = streams[i];
        if (!sk_gsm::variant_ok((int)s.variant) || s.state >= n_states || named[s.state]++) return SK_ERR_INVALID_ARG;
        if (at + s.n_units > n_units) return SK_ERR_INVALID_ARG;
        for (uint32_t u = 0; u < s.n_units; ++u) {
            const sk_g72x_unit &un = units[at + u];
            if (un.offset % 16 || un.size % sk_gsm::packet_bytes((int)s.variant) || un.offset > bytes_len || un.size > bytes_len - un.offset) return SK_ERR_INVALID_ARG;
            const uint64_t samples = sk_gsm::samples_of((int)s.variant, un.size);
            if (samples > sk_gsm::kScratchSamples) return SK_ERR_INVALID_ARG;
            if (!on_device && !sk_gsm::frames_accepted((int)s.variant, bytes + un.offset, un.size, nullptr)) rejected = true;
            out_at[at + u] = cursor, out_bytes[at + u] = (uint32_t)(samples * 2);
            if (samples) need = cursor + samples * 2;
            cursor += g72x_up16((size_t)samples * 2);
        }
        at += s.n_units;
    }
    if (at != n_units || need > out_cap || (need && !out)) return SK_ERR_INVALID_ARG;
    if (rejected) return SK_G72X_ERR_STREAM;
    std::lock_guard<std::mutex> lock(e->mu);
    DeviceGuard guard(e);
    const uint8_t *d_src = bytes;
    uint8_t *d_dst = out;
    if (!on_device) {
        SK_HIP(e->in_buf.reserve(bytes_len + 64), "alloc staging");
        SK_HIP(e->out_buf.reserve((size_t)cursor + 64), "alloc staging");
        if (bytes_len) SK_HIP(hipMemcpyAsync(e->in_buf.p, bytes, bytes_len, hipMemcpyHostToDevice, e->stream), "H2D gsm bytes");
        d_src = (const uint8_t *)e->in_buf.p, d_dst = (uint8_t *)e->out_buf.p;
    }
    GsmBatch b;
    at = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        const sk_gsm_stream &s = streams[i];
        b.begin((int)s.variant, &states[s.state]);
        for (uint32_t u = 0; u < s.n_units; ++u) b.unit((int)s.variant, d_src + units[at + u].offset, d_dst + out_at[at + u], units[at + u].size);
        at += s.n_units;
    }
    SK_HIP(e->gsm_tab.reserve(GsmBatch::tables_bound(n_streams, n_units) + 64), "alloc gsm tables");
    SK_HIP(e->gsm_ws.reserve((size_t)b.ws_samples * 2 + 64), "alloc gsm workspace");
    int rc = gsm_launch(e, b, (uint8_t *)e->gsm_tab.p, (int16_t *)e->gsm_ws.p);
    if (rc == SK_OK && !on_device && need) {
        // one copy up to the end of the last unit's samples; every unit is whole frames of 320 bytes, so there are no gaps between them
        const hipError_t err = hipMemcpyAsync(out, d_dst, (size_t)need, hipMemcpyDeviceToHost, e->stream);
        if (err != hipSuccess) rc = e->hip_fail(err, "D2H gsm");
    }
    const hipError_t waited = hipStreamSynchronize(e->stream);  // the tables leave scope with the call
    if (rc != SK_OK) return rc;
    SK_HIP(waited, "gsm sync");
    for (uint32_t i = 0; i < n_streams; ++i) std::memcpy(&states[streams[i].state], &b.states[(size_t)i * sk::kGsmStateWords], sizeof(sk_gsm_state));
    for (uint32_t k = 0; k < n_units; ++k) units[k].out_offset = out_at[k], units[k].out_len = out_bytes[k];
    *out_len = (size_t)need;
    return SK_OK;
}

// sk_gsm_decode[_dev]: a table of one stream with one unit
int gsm_decode_one(sk_engine *e, int variant, const uint8_t *bytes, size_t len, bool on_device, uint8_t *out, size_t out_cap, size_t *out_len,
                   sk_gsm_state *state, char *error, size_t error_cap) {
    g72x_text(error, error_cap, "");
    if (!e || !out_len) return SK_ERR_INVALID_ARG;
    *out_len = 0;
    if (!sk_gsm::variant_ok(variant) || (len && !bytes) || !state) return SK_ERR_INVALID_ARG;
    if (len > 0x7fffffffull || len % sk_gsm::packet_bytes(variant)) return SK_ERR_INVALID_ARG;
    std::string text;
    if (!sk_gsm::fits_scratch(sk_gsm::samples_of(variant, len), &text) || (!on_device && !sk_gsm::frames_accepted(variant, bytes, len, &text))) {
        g72x_text(error, error_cap, text);
        return SK_G72X_ERR_STREAM;
    }
    sk_gsm_stream s{};
    s.variant = (uint32_t)variant, s.n_units = 1, s.state = 0;
    sk_g72x_unit u{};
    u.size = (uint32_t)len;
    return gsm_decode_batch(e, &s, 1, &u, 1, bytes, len, on_device, out, out_cap, out_len, state, 1);
}

// sk_tick_run_gsm / sk_tick_gsm_out_bound_on: checks the table and derives what the PCM tick's body works on, as g72x_tick_derive does --
// per stream an 8 kHz mono s16le source, per unit where its decoded samples lie (16-byte aligned, unit after unit) -- and the decode
// that stands in front of the body: one launch sequence of the stage over the units of each pass.
struct GsmDerived {
    std::vector<sk_pcm_tick_stream> ts;
    std::vector<sk_pcm_unit> units;  // the decoded layout
    std::vector<uint32_t> first;     // per stream: its first unit
    AiffTick tick;
    GsmBatch batch[2];               // streams that go on through the body, streams delivered as decoded: alive until the tick's last wait
    std::vector<uint32_t> of[2];     // [pass]: record of the batch -> index into the stream table
    size_t part = 0;                 // of gsm_tab per pass
    uint64_t ws_samples = 0;
};

// bytes: the units' bytes on the host, or null when only the bound is asked for (nothing is named or read then)
int gsm_tick_derive(const sk_gsm_tick_stream *gs, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units, const uint8_t *bytes, size_t bytes_len,
                    uint32_t n_states, GsmDerived &d) {
    d.ts.assign(n_streams, sk_pcm_tick_stream{});
    d.units.assign(n_units, sk_pcm_unit{});
    d.first.assign(n_streams, 0);
    d.tick.plain.assign(n_streams, 0);
    d.tick.states.assign((size_t)n_streams * 2, 0);
    std::vector<uint8_t> named(bytes ? n_states : 0, 0);
    uint64_t at = 0, cursor = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        const sk_gsm_tick_stream &g = gs[i];
        if (!sk_gsm::variant_ok(g.variant) || g.channels != 1) return SK_ERR_INVALID_ARG;
        if (bytes && (g.state >= n_states || named[g.state]++)) return SK_ERR_INVALID_ARG;
        sk_pcm_tick_stream &t = d.ts[i];
        t.stream = g.stream, t.n_units = g.n_units, t.channels = 1, t.out_bits = g.out_bits, t.out_channels = g.out_channels;
        t.resample = g.resample, t.flush = g.flush, t.format = SK_FMT_S16LE;
        d.tick.plain[i] = !g.resample && g.out_bits == 16 && g.out_channels == 1;
        d.first[i] = (uint32_t)at;
        if (at + g.n_units > n_units) return SK_ERR_INVALID_ARG;
        for (uint32_t u = 0; u < g.n_units; ++u) {
            const sk_pcm_unit &un = units[at + u];
            if (un.byte_offset % 16 || un.byte_len == 0 || un.byte_len % sk_gsm::packet_bytes(g.variant)) return SK_ERR_INVALID_ARG;
            if (un.byte_offset > bytes_len || un.byte_len > bytes_len - un.byte_offset) return SK_ERR_INVALID_ARG;
            const uint64_t samples = sk_gsm::samples_of(g.variant, un.byte_len);
            if (samples > sk_gsm::kScratchSamples) return SK_ERR_INVALID_ARG;
            if (bytes && !sk_gsm::frames_accepted(g.variant, bytes + un.byte_offset, un.byte_len, nullptr)) return SK_ERR_INVALID_ARG;
            d.units[at + u] = sk_pcm_unit{cursor, (uint32_t)(samples * 2), 0};
            cursor += g72x_up16((size_t)samples * 2);
            d.ws_samples += samples;
        }
        at += g.n_units;
    }
    if (cursor > 0x7fffffffull || (bytes_len > 0x7fffffffull && bytes_len != (size_t)-1)) return SK_ERR_INVALID_ARG;
    d.tick.decoded_len = (size_t)cursor;
    d.part = GsmBatch::tables_bound(n_streams, n_units) + 64;
    return at == n_units ? SK_OK : SK_ERR_INVALID_ARG;
}

// one pass of the decode in front of the body: the units of the streams whose `plain` is as_is, each to where dst_of puts it
int gsm_tick_decode(sk_engine *e, const sk_gsm_tick_stream *gs, const sk_pcm_unit *units, const sk_gsm_state *states, GsmDerived &d, bool as_is,
                    const std::function<uint8_t *(uint32_t, uint32_t)> &dst_of, const uint8_t *d_src) {
    const int p = as_is ? 1 : 0;
    GsmBatch &b = d.batch[p];
    for (uint32_t i = 0; i < (uint32_t)d.ts.size(); ++i) {
        if ((d.tick.plain[i] != 0) != as_is || d.ts[i].n_units == 0) continue;
        const sk_gsm_tick_stream &g = gs[i];
        b.begin(g.variant, &states[g.state]);
        d.of[p].push_back(i);
        for (uint32_t u = 0; u < g.n_units; ++u) b.unit(g.variant, d_src + units[d.first[i] + u].byte_offset, dst_of(i, u), units[d.first[i] + u].byte_len);
    }
    if (b.streams.empty()) return SK_OK;
    // both passes' tables have their own part of gsm_tab; the workspace is shared, the passes follow each other on the stream
    SK_HIP(e->gsm_tab.reserve(2 * d.part), "alloc tick gsm tables");
    SK_HIP(e->gsm_ws.reserve((size_t)d.ws_samples * 2 + 64), "alloc tick gsm workspace");
    return gsm_launch(e, b, (uint8_t *)e->gsm_tab.p + (size_t)p * d.part, (int16_t *)e->gsm_ws.p);
}

int gsm_decoder_fail(sk_gsm_decoder *d, int rc, const std::string &text) {
    d->error = text;
    return rc;
}

// GsmDecoder::decode_i16: `written` samples into out (cap samples)
int gsm_decoder_decode(sk_gsm_decoder *d, const uint8_t *input, size_t len, int16_t *out, size_t out_cap, size_t *written) {
    if (!d || (len && !input) || !written || (out_cap && !out)) return SK_ERR_INVALID_ARG;
    *written = 0;
    const size_t take = d->framer.ready(len);
    const uint64_t samples = sk_gsm::samples_of(d->variant, take);
    std::string text;
    if (!sk_gsm::fits(samples, out_cap, &text)) return gsm_decoder_fail(d, SK_ERR_CAPACITY, text);  // before anything else, as the reference does
    if (samples > 0x3fffffffull) return SK_ERR_INVALID_ARG;
    sk_gsm::Framer after = d->framer;  // the framer moves on only when the decode succeeds
    d->bytes.clear();
    after.add(input, len, d->bytes);  // nothing completes a packet: the bytes wait, nothing is decoded
    if (!sk_gsm::frames_accepted(d->variant, d->bytes.data(), take, &text)) return gsm_decoder_fail(d, SK_G72X_ERR_STREAM, text);
    // a Decoder object is not the pipeline: its output is the caller's, so a call may exceed the pipeline's scratch -- in pieces of
    // whole packets, the carry handed from piece to piece and kept only when all of them decoded
    sk_gsm_stream s{};
    s.variant = (uint32_t)d->variant, s.n_units = 1;
    sk_gsm_state st = d->state;
    const size_t piece = sk_gsm::kScratchSamples / sk_gsm::packet_samples(d->variant) * sk_gsm::packet_bytes(d->variant);
    size_t done = 0, got = 0;
    while (done < take) {
        const size_t n = std::min(piece, take - done);
        sk_g72x_unit u{};
        u.size = (uint32_t)n;
        size_t out_len = 0;
        const int rc = gsm_decode_batch(d->eng, &s, 1, &u, 1, d->bytes.data() + done, n, false, (uint8_t *)(out + got), (out_cap - got) * 2, &out_len, &st, 1);
        if (rc != SK_OK) return rc;
        done += n, got += out_len / 2;
    }
    d->state = st, d->framer = after;
    *written = got;
    return SK_OK;
}

// decode_i32 / decode_f32: the s16 decode into the decoder's own buffer, then `widen` sample for sample
template <typename T, typename F>
int gsm_decoder_decode_as(sk_gsm_decoder *d, const uint8_t *input, size_t len, T *out, size_t out_cap, size_t *written, F widen) {
    if (!d || !written || (out_cap && !out)) return SK_ERR_INVALID_ARG;
    d->pcm.resize(out_cap);
    const int rc = gsm_decoder_decode(d, input, len, d->pcm.data(), out_cap, written);
    if (rc != SK_OK) return rc;
    for (size_t i = 0; i < *written; ++i) out[i] = widen(d->pcm[i]);
    return SK_OK;
}

}  // namespace

extern "C" {

void sk_gsm_state_init(sk_gsm_state *s) try {
    sk::abi_enter();
    if (s) sk_gsm::init_state(s);
} catch (...) {
    (void)sk::abi_caught("sk_gsm_state_init");
}

int sk_gsm_decode(sk_engine *e, int variant, const uint8_t *bytes, size_t len, uint8_t *out, size_t out_cap, size_t *out_len, sk_gsm_state *state, char *error,
                  size_t error_cap) try {
    sk::abi_enter();
    return gsm_decode_one(e, variant, bytes, len, false, out, out_cap, out_len, state, error, error_cap);
} catch (...) {
    return sk::abi_caught("sk_gsm_decode");
}

int sk_gsm_decode_dev(sk_engine *e, int variant, const uint8_t *d_bytes, size_t len, uint8_t *d_out, size_t out_cap, size_t *out_len, sk_gsm_state *state,
                      char *error, size_t error_cap) try {
    sk::abi_enter();
    return gsm_decode_one(e, variant, d_bytes, len, true, d_out, out_cap, out_len, state, error, error_cap);
} catch (...) {
    return sk::abi_caught("sk_gsm_decode_dev");
}

int sk_gsm_decode_batch(sk_engine *e, const sk_gsm_stream *streams, uint32_t n_streams, sk_g72x_unit *units, uint32_t n_units, const uint8_t *bytes,
                        size_t bytes_len, uint8_t *out, size_t out_cap, size_t *out_len, sk_gsm_state *states, uint32_t n_states) try {
    sk::abi_enter();
    return gsm_decode_batch(e, streams, n_streams, units, n_units, bytes, bytes_len, false, out, out_cap, out_len, states, n_states);
} catch (...) {
    return sk::abi_caught("sk_gsm_decode_batch");
}

int sk_gsm_decode_batch_dev(sk_engine *e, const sk_gsm_stream *streams, uint32_t n_streams, sk_g72x_unit *units, uint32_t n_units, const uint8_t *d_bytes,
                            size_t bytes_len, uint8_t *d_out, size_t out_cap, size_t *out_len, sk_gsm_state *states, uint32_t n_states) try {
    sk::abi_enter();
    return gsm_decode_batch(e, streams, n_streams, units, n_units, d_bytes, bytes_len, true, d_out, out_cap, out_len, states, n_states);
} catch (...) {
    return sk::abi_caught("sk_gsm_decode_batch_dev");
}

size_t sk_tick_gsm_out_bound_on(sk_engine *e, const sk_gsm_tick_stream *gs, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units,
                                uint32_t *max_outputs) try {
    sk::abi_enter();
    if (max_outputs) *max_outputs = 0;
    if (!e || (!gs && n_streams) || (!units && n_units)) return 0;
    GsmDerived d;
    if (gsm_tick_derive(gs, n_streams, units, n_units, nullptr, (size_t)-1, 0, d) != SK_OK) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return tick_pcm_out_bound(e, d.ts.data(), n_streams, d.units.data(), n_units, max_outputs, d.tick.plain.data());
} catch (...) {
    (void)sk::abi_caught("sk_tick_gsm_out_bound_on");
    return 0;
}

int sk_tick_run_gsm(sk_engine *e, const sk_gsm_tick_stream *gs, uint32_t n_streams, const sk_pcm_unit *units, uint32_t n_units, const uint8_t *bytes,
                    size_t bytes_len, uint8_t *out, size_t out_cap, sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes,
                    sk_gsm_state *states, uint32_t n_states) try {
    sk::abi_enter();
    if (!e || !n_outs || (n_streams && (!gs || !states)) || (n_units && (!units || !bytes))) return SK_ERR_INVALID_ARG;
    *n_outs = 0;
    if (out_bytes) *out_bytes = 0;
    GsmDerived d;
    static const uint8_t none = 0;  // a tick without units reads no bytes, but still names its records
    int rc = gsm_tick_derive(gs, n_streams, units, n_units, bytes ? bytes : &none, bytes_len, n_states, d);
    if (rc != SK_OK) return rc;
    d.tick.decode = [&](bool as_is, const std::function<uint8_t *(uint32_t, uint32_t)> &dst_of, const uint8_t *d_src) {
        return gsm_tick_decode(e, gs, units, states, d, as_is, dst_of, d_src);
    };
    rc = tick_pcm_impl(e, d.ts.data(), n_streams, d.units.data(), n_units, bytes, bytes_len, out, out_cap, outs, outs_cap, n_outs, out_bytes, &d.tick);
    if (rc != SK_OK) return rc;  // the carries are the caller's records: untouched
    for (int p = 0; p < 2; ++p)
        for (size_t k = 0; k < d.of[p].size(); ++k) std::memcpy(&states[gs[d.of[p][k]].state], &d.batch[p].states[k * sk::kGsmStateWords], sizeof(sk_gsm_state));
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_tick_run_gsm");
}

int sk_gsm_decoder_create(sk_engine *e, int variant, sk_gsm_decoder **out) try {
    sk::abi_enter();
    if (!e || !out || !sk_gsm::variant_ok(variant)) return SK_ERR_INVALID_ARG;
    std::unique_ptr<sk_gsm_decoder> d(new sk_gsm_decoder());
    d->eng = e, d->variant = variant;
    d->framer = sk_gsm::Framer(variant);
    sk_gsm::init_state(&d->state);
    *out = d.release();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_gsm_decoder_create");
}

void sk_gsm_decoder_destroy(sk_gsm_decoder *d) try {
    sk::abi_enter();
    delete d;
} catch (...) {
    (void)sk::abi_caught("sk_gsm_decoder_destroy");
}

int sk_gsm_decoder_info(const sk_gsm_decoder *d, int *variant, uint32_t *sample_rate, uint32_t *channels) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    if (variant) *variant = d->variant;
    if (sample_rate) *sample_rate = 8000;
    if (channels) *channels = 1;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_gsm_decoder_info");
}

int sk_gsm_decoder_decode_i16(sk_gsm_decoder *d, const uint8_t *input, size_t len, int16_t *out, size_t out_cap, size_t *written) try {
    sk::abi_enter();
    return gsm_decoder_decode(d, input, len, out, out_cap, written);
} catch (...) {
    return sk::abi_caught("sk_gsm_decoder_decode_i16");
}

int sk_gsm_decoder_decode_i32(sk_gsm_decoder *d, const uint8_t *input, size_t len, int32_t *out, size_t out_cap, size_t *written) try {
    sk::abi_enter();
    return gsm_decoder_decode_as(d, input, len, out, out_cap, written, [](int16_t v) { return (int32_t)((uint32_t)(int32_t)v << 16); });
} catch (...) {
    return sk::abi_caught("sk_gsm_decoder_decode_i32");
}

int sk_gsm_decoder_decode_f32(sk_gsm_decoder *d, const uint8_t *input, size_t len, float *out, size_t out_cap, size_t *written) try {
    sk::abi_enter();
    return gsm_decoder_decode_as(d, input, len, out, out_cap, written, [](int16_t v) { return (float)v / 32768.0f; });
} catch (...) {
    return sk::abi_caught("sk_gsm_decoder_decode_f32");
}

int sk_gsm_decoder_flush(sk_gsm_decoder *d) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    std::string text;
    if (d->framer.flush(&text)) return SK_OK;
    return gsm_decoder_fail(d, SK_G72X_ERR_STREAM, text);
} catch (...) {
    return sk::abi_caught("sk_gsm_decoder_flush");
}

int sk_gsm_decoder_reset(sk_gsm_decoder *d) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    sk_gsm::init_state(&d->state);
    d->framer.pending.clear();
    d->error.clear();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_gsm_decoder_reset");
}

const char *sk_gsm_decoder_last_error(const sk_gsm_decoder *d) try {
    sk::abi_enter();
    return d ? d->error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_gsm_decoder_last_error");
    return "";
}

}  // extern "C"

// ---- Ogg and Vorbis (ogg_stream.h, vorbis_stream.h, vorbis_decode.hip) ------------------------------------------------------------

struct sk_ogg_parser {
    sk_ogg::Parser parser;
    std::string error;
    bool dead = false;
};

static_assert(sizeof(sk_vorbis_packet_info) == sizeof(sk::VorbisInfo) && offsetof(sk_vorbis_packet_info, final_y) == offsetof(sk::VorbisInfo, final_y) &&
                  offsetof(sk_vorbis_packet_info, step2) == offsetof(sk::VorbisInfo, step2),
              "the kernel writes the public record");

namespace {

// the engine's Vorbis constants, made on first use (engine lock held): the inverse-dB table -- the geometric series from 1.0649863e-07
// to 1 in 255 steps -- and per block size 64 ... 8192 the window's rising half, the IMDCT's twiddles and the FFT's roots, all computed
// in f64 and rounded to f32
int vorbis_tables(sk_engine *e) {
    if (e->vorbis_tables_ready) return SK_OK;
    std::vector<float> h(256);
    const double first = 1.0649863e-07;
    for (int i = 0; i < 256; ++i) h[i] = (float)(first * std::pow(1.0 / first, i / 255.0));
    size_t at_slope[8], at_tw[8], at_root[8];
    for (int k = 0; k < 8; ++k) {
        const uint32_t n = 64u << k, half = n / 2, n4 = n / 4;
        at_slope[k] = h.size();
        for (uint32_t i = 0; i < half; ++i) {
            const double s = std::sin((i + 0.5) / (2.0 * half) * M_PI);
            h.push_back((float)std::sin(M_PI / 2 * (s * s)));
        }
        at_tw[k] = h.size();
        for (uint32_t j = 0; j < n4; ++j) {
            const double a = -M_PI * (8.0 * j + 1.0) / (8.0 * half);
            h.push_back((float)std::cos(a)), h.push_back((float)std::sin(a));
        }
        at_root[k] = h.size();
        for (uint32_t m = 0; m < n4 / 2; ++m) {
            const double a = -2.0 * M_PI * m / n4;
            h.push_back((float)std::cos(a)), h.push_back((float)std::sin(a));
        }
    }
    SK_HIP(e->vorbis_tab.reserve(h.size() * 4), "alloc vorbis constants");
    SK_HIP(hipMemcpyAsync(e->vorbis_tab.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, e->stream), "H2D vorbis constants");
    SK_HIP(hipStreamSynchronize(e->stream), "vorbis constants sync");
    const float *d = (const float *)e->vorbis_tab.p;
    e->vorbis_tables.inverse_db = d;
    for (int k = 0; k < 8; ++k) {
        e->vorbis_tables.slope[k] = d + at_slope[k];
        e->vorbis_tables.twiddle[k] = (const float2 *)(d + at_tw[k]);
        e->vorbis_tables.root[k] = (const float2 *)(d + at_root[k]);
    }
    e->vorbis_tables_ready = true;
    return SK_OK;
}

enum VorbisWhat { kVorbisS16 = 0, kVorbisF32 = 1, kVorbisEntropy = 2 };

// the tick's form of the decode: the samples stay on the device, packet k's at base + 2 * offsets[k] (s16); the caller holds the engine's
// lock and its device
struct VorbisDevDst {
    uint8_t *base = nullptr;
    std::vector<uint64_t> offsets;  // per packet of the call, in samples
    std::vector<uint32_t> keep;     // per packet: at most so many of its frames (0xffffffff: all) ...
    std::vector<uint32_t> skip;     // ... of those behind the first skip[k]
};

// the frames a packet of `full` frames gives once `skip` have gone off its front and at most `keep` of the rest stay
inline uint32_t vorbis_kept(uint32_t full, uint32_t skip, uint32_t keep) { return std::min(full - std::min(full, skip), keep); }

// sk_vorbis_decode_packets and sk_vorbis_entropy_decode.  The host reads every packet's first bits itself (sk_vorbis::packet_head), so the
// place of every packet in the workspaces and in the output is known before anything is launched.  The host decides: a packet it refuses
// gets no lane and keeps the host's status.  The device reads the bits of the accepted packets again as a guard; should it ever
// disagree, the call is SK_ERR_INTERNAL.
int vorbis_run(sk_engine *e, sk_vorbis_stream *streams, uint32_t n_streams, const sk_vorbis_packet *packets, uint32_t n_packets, const uint8_t *bytes,
               size_t bytes_len, VorbisWhat what, void *out, size_t out_cap, size_t *out_len, int32_t *status, uint32_t *frames,
               sk_vorbis_packet_info *info, const VorbisDevDst *dev = nullptr) {
    if (!e || !out_len || (n_streams && !streams) || (n_packets && (!packets || !bytes || (!out && !dev)))) return SK_ERR_INVALID_ARG;
    if (what == kVorbisEntropy ? (n_packets && !info) : (n_packets && (!status || !frames))) return SK_ERR_INVALID_ARG;
    *out_len = 0;
    if (bytes_len > 0x7fffff00u) return SK_ERR_INVALID_ARG;
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    std::vector<sk::VorbisPacket> table(n_packets);
    std::vector<uint32_t> order, blobs;
    std::vector<int32_t> head_status(n_packets, 0);
    std::vector<std::pair<const sk_vorbis_setup *, uint32_t>> blob_of;
    std::vector<sk::VorbisCarry> carries(n_streams);  // offset: the stream's part of the carry buffer, entering and leaving
    uint64_t res_floats = 0, pcm_floats = 0, cls_bytes = 0, carry_floats = 0, out_samples = 0, at = 0;
    uint32_t max_channels = 0;
    for (uint32_t s = 0; s < n_streams; ++s) {
        sk_vorbis_stream &st = streams[s];
        if (!st.setup || (uint64_t)at + st.n_packets > n_packets) return SK_ERR_INVALID_ARG;
        const sk_vorbis::Setup &su = st.setup->setup;
        if (st.prev_blocksize && st.prev_blocksize != su.bs[0] && st.prev_blocksize != su.bs[1]) return SK_ERR_INVALID_ARG;
        if (what != kVorbisEntropy && !st.overlap) return SK_ERR_INVALID_ARG;
        uint32_t blob = 0xffffffffu;
        for (auto &b : blob_of)
            if (b.first == st.setup) blob = b.second;
        if (blob == 0xffffffffu) {
            blob = (uint32_t)blobs.size();
            blob_of.emplace_back(st.setup, blob);
            blobs.insert(blobs.end(), su.blob.begin(), su.blob.end());
            if (blobs.size() > (1u << 28)) return SK_ERR_CAPACITY;
        }
        const uint32_t ch = su.channels;
        max_channels = std::max(max_channels, ch);
        carries[s] = {0xffffffffu, (uint32_t)carry_floats};
        carry_floats += (uint64_t)ch * (su.bs[1] / 2);
        uint32_t prev_n = st.prev_blocksize, prev_pcm = carries[s].offset, prev_in_carry = 1;
        for (uint32_t k = 0; k < st.n_packets; ++k, ++at) {
            const sk_vorbis_packet &p = packets[at];
            if ((p.offset & 15u) || p.size > sk_vorbis::kMaxPacketBytes || (uint64_t)p.offset + p.size > bytes_len) return SK_ERR_INVALID_ARG;
            sk::VorbisPacket &t = table[at];
            t = sk::VorbisPacket{};
            t.byte_offset = p.offset, t.byte_len = p.size, t.blob = blob, t.channels = ch;
            sk_vorbis::PacketHead h;
            head_status[at] = sk_vorbis::packet_head(su, bytes + p.offset, p.size, &h);
            if (head_status[at] != sk_vorbis::kOk) continue;
            t.n = h.n;
            t.res_offset = (uint32_t)res_floats, t.cls_offset = (uint32_t)cls_bytes, t.pcm_offset = (uint32_t)pcm_floats;
            res_floats += (uint64_t)ch * (h.n / 2), cls_bytes += up16((uint64_t)ch * (h.n / 2)), pcm_floats += (uint64_t)ch * h.n;
            t.prev_n = prev_n, t.prev_pcm = prev_pcm, t.prev_in_carry = prev_in_carry;
            t.out_frames = prev_n ? prev_n / 4 + h.n / 4 : 0;
            if (dev) {
                t.out_skip = std::min(t.out_frames, dev->skip[at]);
                t.out_frames = vorbis_kept(t.out_frames, dev->skip[at], dev->keep[at]);
            }
            t.out_offset = dev ? dev->offsets[at] : out_samples;
            out_samples += (uint64_t)t.out_frames * ch;
            prev_n = h.n, prev_pcm = t.pcm_offset + h.n / 2, prev_in_carry = 0;
            carries[s].packet = (uint32_t)at;
            order.push_back((uint32_t)at);
            if (res_floats > 0x3fffffffu || pcm_floats > 0x3fffffffu || cls_bytes > 0x7fffffffu) return SK_ERR_CAPACITY;
        }
    }
    if (at != n_packets) return SK_ERR_INVALID_ARG;
    const size_t width = what == kVorbisS16 ? 2 : 4;
    const uint64_t need = what == kVorbisEntropy ? res_floats * 4 : out_samples * width;
    if (!dev && need > out_cap) {  // nothing decoded, nothing carried: the caller comes again with room
        *out_len = (size_t)(what == kVorbisEntropy ? need / 4 : need);
        return SK_ERR_CAPACITY;
    }
    if (n_packets == 0) return SK_OK;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return table[x].byte_len > table[y].byte_len; });

    std::unique_lock<std::mutex> lock(e->mu, std::defer_lock);
    std::unique_ptr<DeviceGuard> guard;
    if (!dev) {
        lock.lock();
        guard.reset(new DeviceGuard(e));
    }
    if (const int rc = vorbis_tables(e)) return rc;
    // vorbis_in: bytes (16 readable bytes behind them) | blobs | packet table | order | carried halves | carry records
    const size_t at_blobs = up16(bytes_len + 16), at_table = at_blobs + up16(blobs.size() * 4), at_order = at_table + up16(table.size() * sizeof(sk::VorbisPacket)),
                 at_carry = at_order + up16(order.size() * 4 + 4), at_crec = at_carry + up16((size_t)carry_floats * 4 + 4),
                 in_len = at_crec + up16(carries.size() * sizeof(sk::VorbisCarry) + 4);
    // vorbis_ws: residue vectors | windowed halves | classifications | records
    const size_t at_pcm = up16((size_t)res_floats * 4 + 4), at_cls = at_pcm + up16((size_t)pcm_floats * 4 + 4), at_info = at_cls + up16((size_t)cls_bytes + 4),
                 ws_len = at_info + (size_t)n_packets * sizeof(sk::VorbisInfo);
    SK_HIP(e->vorbis_in.reserve(in_len), "alloc vorbis input");
    SK_HIP(e->vorbis_ws.reserve(ws_len), "alloc vorbis workspace");
    if (!dev) SK_HIP(e->vorbis_out.reserve(std::max<size_t>((size_t)need, 16)), "alloc vorbis output");
    uint8_t *d_in = (uint8_t *)e->vorbis_in.p, *d_ws = (uint8_t *)e->vorbis_ws.p;
    SK_HIP(hipMemsetAsync(d_in + (bytes_len & ~(size_t)3), 0, at_blobs - (bytes_len & ~(size_t)3), e->stream), "clear vorbis padding");
    SK_HIP(hipMemcpyAsync(d_in, bytes, bytes_len, hipMemcpyHostToDevice, e->stream), "H2D vorbis packets");
    SK_HIP(hipMemcpyAsync(d_in + at_blobs, blobs.data(), blobs.size() * 4, hipMemcpyHostToDevice, e->stream), "H2D vorbis blobs");
    SK_HIP(hipMemcpyAsync(d_in + at_table, table.data(), table.size() * sizeof(sk::VorbisPacket), hipMemcpyHostToDevice, e->stream), "H2D vorbis table");
    if (!order.empty()) SK_HIP(hipMemcpyAsync(d_in + at_order, order.data(), order.size() * 4, hipMemcpyHostToDevice, e->stream), "H2D vorbis order");
    std::vector<float> h_carry;  // every stream's half in one copy each way: thousands of small copies cost more than the kernels
    if (what != kVorbisEntropy) {
        h_carry.assign((size_t)carry_floats, 0.0f);
        for (uint32_t s = 0; s < n_streams; ++s)
            if (streams[s].prev_blocksize)
                std::memcpy(&h_carry[carries[s].offset], streams[s].overlap, (size_t)streams[s].setup->setup.channels * (streams[s].prev_blocksize / 2) * 4);
        SK_HIP(hipMemcpyAsync(d_in + at_carry, h_carry.data(), h_carry.size() * 4, hipMemcpyHostToDevice, e->stream), "H2D vorbis overlap");
        SK_HIP(hipMemcpyAsync(d_in + at_crec, carries.data(), carries.size() * sizeof(sk::VorbisCarry), hipMemcpyHostToDevice, e->stream), "H2D vorbis carries");
    }
    SK_HIP(hipMemsetAsync(d_ws, 0, at_pcm, e->stream), "clear vorbis residue");
    SK_HIP(hipMemsetAsync(d_ws + at_info, 0, (size_t)n_packets * sizeof(sk::VorbisInfo), e->stream), "clear vorbis records");
    const sk::VorbisPacket *d_table = (const sk::VorbisPacket *)(d_in + at_table);
    const uint32_t *d_blobs = (const uint32_t *)(d_in + at_blobs);
    sk::VorbisInfo *d_info = (sk::VorbisInfo *)(d_ws + at_info);
    float *d_res = (float *)d_ws, *d_pcm = (float *)(d_ws + at_pcm);
    SK_HIP(sk::launch_vorbis_entropy(d_table, (const uint32_t *)(d_in + at_order), (uint32_t)order.size(), d_blobs, d_in, d_res, d_ws + at_cls, d_info, e->stream),
           "launch vorbis entropy");
    if (what == kVorbisEntropy) {
        std::vector<sk::VorbisInfo> h_info(n_packets);
        SK_HIP(hipMemcpyAsync(h_info.data(), d_info, (size_t)n_packets * sizeof(sk::VorbisInfo), hipMemcpyDeviceToHost, e->stream), "D2H vorbis records");
        if (res_floats) SK_HIP(hipMemcpyAsync(out, d_res, (size_t)res_floats * 4, hipMemcpyDeviceToHost, e->stream), "D2H vorbis residue");
        SK_HIP(hipStreamSynchronize(e->stream), "vorbis sync");
        for (uint32_t i = 0; i < n_packets; ++i) {
            std::memcpy(&info[i], &h_info[i], sizeof(sk::VorbisInfo));
            if (head_status[i] != 0) info[i].status = head_status[i];
        }
        *out_len = (size_t)res_floats;
        return SK_OK;
    }
    SK_HIP(sk::launch_vorbis_spectrum(d_table, n_packets, d_blobs, d_info, d_res, e->vorbis_tables, e->stream), "launch vorbis spectrum");
    SK_HIP(sk::launch_vorbis_imdct(d_table, n_packets, d_blobs, d_info, d_res, d_pcm, max_channels, e->vorbis_tables, e->stream), "launch vorbis imdct");
    SK_HIP(sk::launch_vorbis_ola(d_table, n_packets, d_info, d_pcm, (const float *)(d_in + at_carry), dev ? (void *)dev->base : e->vorbis_out.p, what == kVorbisF32,
                                 e->stream),
           "launch vorbis ola");
    SK_HIP(sk::launch_vorbis_carry(d_table, (const sk::VorbisCarry *)(d_in + at_crec), n_streams, d_pcm, (float *)(d_in + at_carry), e->stream),
           "launch vorbis carry");
    SK_HIP(hipMemcpyAsync(h_carry.data(), d_in + at_carry, h_carry.size() * 4, hipMemcpyDeviceToHost, e->stream), "D2H vorbis overlap");
    std::vector<int32_t> d_status(n_packets);  // the records' status words alone: a record is 1 580 bytes
    SK_HIP(hipMemcpy2DAsync(d_status.data(), 4, d_info, sizeof(sk::VorbisInfo), 4, n_packets, hipMemcpyDeviceToHost, e->stream), "D2H vorbis statuses");
    if (need && !dev) SK_HIP(hipMemcpyAsync(out, e->vorbis_out.p, (size_t)need, hipMemcpyDeviceToHost, e->stream), "D2H vorbis PCM");
    SK_HIP(hipStreamSynchronize(e->stream), "vorbis sync");
    for (uint32_t i = 0; i < n_packets; ++i) {
        status[i] = head_status[i] != 0 ? head_status[i] : d_status[i];
        frames[i] = status[i] == 0 ? table[i].out_frames : 0;
        if (head_status[i] == 0 && d_status[i] != 0) return SK_ERR_INTERNAL;  // the device read other first bits than the host
    }
    // the halves the streams leave with: the right half of each stream's last accepted packet
    for (uint32_t s = 0; s < n_streams; ++s) {
        if (carries[s].packet == 0xffffffffu) continue;
        const sk::VorbisPacket &t = table[carries[s].packet];
        std::memcpy(streams[s].overlap, &h_carry[carries[s].offset], (size_t)t.channels * (t.n / 2) * 4);
        streams[s].prev_blocksize = t.n;
    }
    *out_len = (size_t)need;
    return SK_OK;
}


// sk_tick_run_vorbis / sk_tick_vorbis_out_bound_on: what stands in front of the PCM tick's body.  The host reads every packet's first
// bits, so the frames each packet yields (prev / 4 + this / 4; none for a stream's first packet ever and for a refused one) are known:
// the packets that yield frames are the body's units, interleaved s16le of the stream's channel count, 16-byte aligned one after the
// other.  The decode works on copies of the streams' carries; they become the caller's only when the whole tick succeeded.
struct VorbisDerived {
    std::vector<sk_pcm_tick_stream> ts;
    std::vector<sk_pcm_unit> units;         // the decoded layout: one per packet that yields frames
    std::vector<uint32_t> first_packet;     // per stream
    std::vector<uint32_t> unit_of;          // per packet: its unit within its stream, or 0xffffffff
    std::vector<uint32_t> packet_of;        // per unit of the call: its packet
    std::vector<uint32_t> frames;           // per packet
    std::vector<int32_t> status;            // per packet: the host's reading, then the decode's
    std::vector<std::vector<float>> overlap;
    std::vector<uint32_t> prev;
    AiffTick tick;
};

int vorbis_tick_derive(const sk_vorbis_tick_stream *vs, uint32_t n_streams, const sk_vorbis_tick_packet *packets, uint32_t n_packets, const uint8_t *bytes,
                       size_t bytes_len, VorbisDerived &d) {
    d.ts.assign(n_streams, sk_pcm_tick_stream{});
    d.units.clear(), d.packet_of.clear();
    d.first_packet.assign(n_streams, 0);
    d.unit_of.assign(n_packets, 0xffffffffu);
    d.frames.assign(n_packets, 0);
    d.status.assign(n_packets, 0);
    d.overlap.assign(n_streams, {});
    d.prev.assign(n_streams, 0);
    d.tick.plain.assign(n_streams, 0);
    d.tick.states.assign((size_t)n_streams * 2, 0);
    uint64_t at = 0, cursor = 0;
    for (uint32_t i = 0; i < n_streams; ++i) {
        const sk_vorbis_tick_stream &v = vs[i];
        if (!v.setup || !v.overlap || at + v.n_units > n_packets) return SK_ERR_INVALID_ARG;
        const sk_vorbis::Setup &su = v.setup->setup;
        if (v.prev_blocksize && v.prev_blocksize != su.bs[0] && v.prev_blocksize != su.bs[1]) return SK_ERR_INVALID_ARG;
        const uint32_t ch = su.channels;
        if (v.channels && v.channels != ch) return SK_ERR_INVALID_ARG;
        d.first_packet[i] = (uint32_t)at;
        d.prev[i] = v.prev_blocksize;
        d.overlap[i].assign(v.overlap, v.overlap + (size_t)ch * (su.bs[1] / 2));
        uint32_t prev = v.prev_blocksize, n_units = 0;
        for (uint32_t u = 0; u < v.n_units; ++u, ++at) {
            const sk_vorbis_tick_packet &p = packets[at];
            if ((p.offset & 15u) || p.size > sk_vorbis::kMaxPacketBytes || (uint64_t)p.offset + p.size > bytes_len) return SK_ERR_INVALID_ARG;
            sk_vorbis::PacketHead h;
            d.status[at] = sk_vorbis::packet_head(su, bytes + p.offset, p.size, &h);
            if (d.status[at] != sk_vorbis::kOk) continue;
            d.frames[at] = vorbis_kept(prev ? prev / 4 + h.n / 4 : 0, p.skip_frames, p.keep_frames);
            prev = h.n;
            if (!d.frames[at]) continue;
            const uint64_t decoded = (uint64_t)d.frames[at] * ch * 2;
            d.unit_of[at] = n_units++;
            d.packet_of.push_back((uint32_t)at);
            d.units.push_back(sk_pcm_unit{cursor, (uint32_t)decoded, 0});
            cursor += (decoded + 15) & ~15ull;
        }
        sk_pcm_tick_stream &t = d.ts[i];
        t.stream = v.stream, t.n_units = n_units, t.channels = (uint8_t)ch, t.out_bits = v.out_bits, t.out_channels = v.out_channels;
        t.resample = v.resample, t.flush = v.flush, t.format = SK_FMT_S16LE;
        d.tick.plain[i] = !v.resample && v.out_bits == 16 && v.out_channels == ch;
    }
    if (cursor > 0x7fffffffull || bytes_len > 0x7fffff00ull) return SK_ERR_INVALID_ARG;
    d.tick.decoded_len = (size_t)cursor;
    return at == n_packets ? SK_OK : SK_ERR_INVALID_ARG;
}

// one pass of the decode in front of the body: every packet of the streams whose `plain` is as_is (also of a stream that yields nothing
// in this tick: its carry moves on), each packet's frames to where dst_of puts its unit
int vorbis_tick_decode(sk_engine *e, const sk_vorbis_tick_stream *vs, const sk_vorbis_tick_packet *packets, const uint8_t *bytes, size_t bytes_len, VorbisDerived &d,
                       bool as_is, const std::function<uint8_t *(uint32_t, uint32_t)> &dst_of) {
    std::vector<sk_vorbis_stream> sub;
    std::vector<uint32_t> sub_of, index;
    std::vector<sk_vorbis_packet> subp;
    std::vector<uint8_t *> dst;
    std::vector<uint32_t> keep, skip;
    uint8_t *base = nullptr;
    for (uint32_t i = 0; i < (uint32_t)d.ts.size(); ++i) {
        if ((d.tick.plain[i] != 0) != as_is || vs[i].n_units == 0) continue;
        sub.push_back(sk_vorbis_stream{vs[i].setup, d.overlap[i].data(), vs[i].n_units, d.prev[i]});
        sub_of.push_back(i);
        for (uint32_t u = 0; u < vs[i].n_units; ++u) {
            const uint32_t g = d.first_packet[i] + u;
            uint8_t *to = d.unit_of[g] != 0xffffffffu ? dst_of(i, d.unit_of[g]) : nullptr;
            if (to && (!base || to < base)) base = to;
            index.push_back(g), subp.push_back(sk_vorbis_packet{packets[g].offset, packets[g].size}), dst.push_back(to), keep.push_back(packets[g].keep_frames), skip.push_back(packets[g].skip_frames);
        }
    }
    if (sub.empty()) return SK_OK;
    VorbisDevDst dev;
    dev.base = base;
    dev.offsets.assign(dst.size(), 0);
    dev.keep = keep;
    dev.skip = skip;
    for (size_t k = 0; k < dst.size(); ++k)
        if (dst[k]) dev.offsets[k] = (uint64_t)(dst[k] - base) / 2;
    std::vector<int32_t> status(index.size(), 0);
    std::vector<uint32_t> frames(index.size(), 0);
    size_t len = 0;
    const int rc = vorbis_run(e, sub.data(), (uint32_t)sub.size(), subp.data(), (uint32_t)subp.size(), bytes, bytes_len, kVorbisS16, nullptr, 0, &len,
                              status.data(), frames.data(), nullptr, &dev);
    if (rc != SK_OK) return rc;
    for (size_t k = 0; k < index.size(); ++k) {
        if (frames[k] != d.frames[index[k]]) return SK_ERR_INTERNAL;  // the plan and the decode read the same first bits
        d.status[index[k]] = status[k];
    }
    for (size_t k = 0; k < sub.size(); ++k) d.prev[sub_of[k]] = sub[k].prev_blocksize;
    return SK_OK;
}

void vorbis_text(char *error, size_t cap, const std::string &text) {
    if (!error || cap == 0) return;
    const size_t n = std::min(cap - 1, text.size());
    std::memcpy(error, text.data(), n);
    error[n] = 0;
}

}  // namespace

extern "C" {

int sk_ogg_parser_create(sk_ogg_parser **out) try {
    sk::abi_enter();
    if (!out) return SK_ERR_INVALID_ARG;
    *out = new sk_ogg_parser();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_ogg_parser_create");
}

void sk_ogg_parser_destroy(sk_ogg_parser *p) try {
    sk::abi_enter();
    delete p;
} catch (...) {
    (void)sk::abi_caught("sk_ogg_parser_destroy");
}

int sk_ogg_parser_add(sk_ogg_parser *p, const uint8_t *data, size_t len) try {
    sk::abi_enter();
    if (!p || (len && !data)) return SK_ERR_INVALID_ARG;
    if (p->dead) return SK_VORBIS_ERR_STREAM;
    if (p->parser.add(data, len, &p->error)) return SK_OK;
    p->dead = true;
    return SK_VORBIS_ERR_STREAM;
} catch (...) {
    return sk::abi_caught("sk_ogg_parser_add");
}

int sk_ogg_parser_finish(sk_ogg_parser *p) try {
    sk::abi_enter();
    if (!p) return SK_ERR_INVALID_ARG;
    if (p->dead) return SK_VORBIS_ERR_STREAM;
    if (p->parser.finish(&p->error)) return SK_OK;
    p->dead = true;
    return SK_VORBIS_ERR_STREAM;
} catch (...) {
    return sk::abi_caught("sk_ogg_parser_finish");
}

uint32_t sk_ogg_parser_pending(const sk_ogg_parser *p) try {
    sk::abi_enter();
    return p ? (uint32_t)p->parser.pending.size() : 0;
} catch (...) {
    (void)sk::abi_caught("sk_ogg_parser_pending");
    return 0;
}

int sk_ogg_parser_take(sk_ogg_parser *p, sk_ogg_packet_info *info, uint8_t *data, size_t data_cap) try {
    sk::abi_enter();
    if (!p || !info) return SK_ERR_INVALID_ARG;
    if (p->parser.pending.empty()) return SK_ERR_BAD_STREAM;
    const sk_ogg::Packet &k = p->parser.pending.front();
    *info = sk_ogg_packet_info{};
    info->granule_position = k.granule_position, info->size = (uint32_t)k.data.size(), info->serial = k.serial;
    info->first_in_stream = k.first_in_stream, info->last_in_page = k.last_in_page, info->last_in_stream = k.last_in_stream, info->has_granule = k.has_granule;
    if (k.data.size() > data_cap || (!data && !k.data.empty())) return SK_ERR_CAPACITY;
    if (!k.data.empty()) std::memcpy(data, k.data.data(), k.data.size());
    p->parser.pending.pop_front();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_ogg_parser_take");
}

const char *sk_ogg_parser_last_error(const sk_ogg_parser *p) try {
    sk::abi_enter();
    return p ? p->error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_ogg_parser_last_error");
    return "";
}

uint32_t sk_ogg_page_crc(const uint8_t *page, size_t len) try {
    sk::abi_enter();
    return page ? sk_ogg::page_crc(page, len) : 0;
} catch (...) {
    (void)sk::abi_caught("sk_ogg_page_crc");
    return 0;
}

int sk_vorbis_parse_ident(const uint8_t *packet, size_t len, sk_vorbis_ident *out, char *error, size_t error_cap) try {
    sk::abi_enter();
    if ((len && !packet) || !out) return SK_ERR_INVALID_ARG;
    vorbis_text(error, error_cap, "");
    sk_vorbis::Ident id;
    std::string text;
    if (const int rc = sk_vorbis::parse_ident(packet, len, &id, &text)) {
        vorbis_text(error, error_cap, text);
        return rc;
    }
    *out = sk_vorbis_ident{};
    out->sample_rate = id.sample_rate, out->bitrate_maximum = id.bitrate_maximum, out->bitrate_nominal = id.bitrate_nominal;
    out->bitrate_minimum = id.bitrate_minimum, out->blocksize_0 = id.blocksize_0, out->blocksize_1 = id.blocksize_1, out->channels = id.channels;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_vorbis_parse_ident");
}

int sk_vorbis_parse_comment(const uint8_t *packet, size_t len, char *error, size_t error_cap) try {
    sk::abi_enter();
    if (len && !packet) return SK_ERR_INVALID_ARG;
    vorbis_text(error, error_cap, "");
    std::string text;
    const int rc = sk_vorbis::parse_comment(packet, len, &text);
    if (rc) vorbis_text(error, error_cap, text);
    return rc;
} catch (...) {
    return sk::abi_caught("sk_vorbis_parse_comment");
}

int sk_vorbis_setup_create(const sk_vorbis_ident *ident, const uint8_t *packet, size_t len, sk_vorbis_setup **out, char *error, size_t error_cap) try {
    sk::abi_enter();
    if (!ident || (len && !packet) || !out) return SK_ERR_INVALID_ARG;
    *out = nullptr;
    vorbis_text(error, error_cap, "");
    const uint32_t b0 = ident->blocksize_0, b1 = ident->blocksize_1;
    if (ident->channels == 0 || b0 < 64 || b1 > 8192 || b0 > b1 || (b0 & (b0 - 1)) || (b1 & (b1 - 1))) return SK_ERR_INVALID_ARG;
    sk_vorbis::Ident id;
    id.sample_rate = ident->sample_rate, id.blocksize_0 = ident->blocksize_0, id.blocksize_1 = ident->blocksize_1, id.channels = ident->channels;
    std::unique_ptr<sk_vorbis_setup> s(new sk_vorbis_setup());
    std::string text;
    if (const int rc = sk_vorbis::parse_setup(packet, len, id, &s->setup, &text)) {
        vorbis_text(error, error_cap, text);
        return rc;
    }
    *out = s.release();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_vorbis_setup_create");
}

void sk_vorbis_setup_destroy(sk_vorbis_setup *s) try {
    sk::abi_enter();
    delete s;
} catch (...) {
    (void)sk::abi_caught("sk_vorbis_setup_destroy");
}

int sk_vorbis_setup_get_info(const sk_vorbis_setup *s, sk_vorbis_setup_info *info) try {
    sk::abi_enter();
    if (!s || !info) return SK_ERR_INVALID_ARG;
    *info = sk_vorbis_setup_info{};
    const sk_vorbis::Setup &u = s->setup;
    info->books = (uint32_t)u.books.size(), info->floors = (uint32_t)u.floors.size(), info->residues = (uint32_t)u.residues.size();
    info->mappings = (uint32_t)u.mappings.size(), info->modes = (uint32_t)u.modes.size(), info->blob_bytes = (uint32_t)(u.blob.size() * 4);
    info->blocksize_0 = (uint16_t)u.bs[0], info->blocksize_1 = (uint16_t)u.bs[1], info->channels = (uint8_t)u.channels;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_vorbis_setup_get_info");
}

int sk_vorbis_packet_blocksize(const sk_vorbis_setup *s, const uint8_t *packet, size_t len, uint32_t *blocksize) try {
    sk::abi_enter();
    if (!s || (len && !packet) || !blocksize) return SK_ERR_INVALID_ARG;
    sk_vorbis::PacketHead h;
    const int rc = sk_vorbis::packet_head(s->setup, packet, len, &h);
    *blocksize = rc ? 0 : h.n;
    return rc;
} catch (...) {
    return sk::abi_caught("sk_vorbis_packet_blocksize");
}

int sk_vorbis_decode_packets(sk_engine *e, sk_vorbis_stream *streams, uint32_t n_streams, const sk_vorbis_packet *packets, uint32_t n_packets,
                             const uint8_t *bytes, size_t bytes_len, int as_f32, void *out, size_t out_cap, size_t *out_len, int32_t *status_per_packet,
                             uint32_t *frames_per_packet) try {
    sk::abi_enter();
    return vorbis_run(e, streams, n_streams, packets, n_packets, bytes, bytes_len, as_f32 ? kVorbisF32 : kVorbisS16, out, out_cap, out_len, status_per_packet,
                      frames_per_packet, nullptr);
} catch (...) {
    return sk::abi_caught("sk_vorbis_decode_packets");
}

size_t sk_tick_vorbis_out_bound_on(sk_engine *e, const sk_vorbis_tick_stream *vs, uint32_t n_streams, const sk_vorbis_tick_packet *packets, uint32_t n_packets,
                                   const uint8_t *bytes, size_t bytes_len, uint32_t *max_outputs) try {
    sk::abi_enter();
    if (max_outputs) *max_outputs = 0;
    if (!e || (!vs && n_streams) || (n_packets && (!packets || !bytes))) return 0;
    VorbisDerived d;
    if (vorbis_tick_derive(vs, n_streams, packets, n_packets, bytes, bytes_len, d) != SK_OK) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return tick_pcm_out_bound(e, d.ts.data(), n_streams, d.units.data(), (uint32_t)d.units.size(), max_outputs, d.tick.plain.data());
} catch (...) {
    (void)sk::abi_caught("sk_tick_vorbis_out_bound_on");
    return 0;
}

int sk_tick_run_vorbis(sk_engine *e, sk_vorbis_tick_stream *vs, uint32_t n_streams, const sk_vorbis_tick_packet *packets, uint32_t n_packets, const uint8_t *bytes,
                       size_t bytes_len, uint8_t *out, size_t out_cap, sk_tick_output *outs, uint32_t outs_cap, uint32_t *n_outs, size_t *out_bytes,
                       int32_t *status_per_packet) try {
    sk::abi_enter();
    if (!e || !n_outs || (n_streams && !vs) || (n_packets && (!packets || !bytes || !status_per_packet))) return SK_ERR_INVALID_ARG;
    *n_outs = 0;
    if (out_bytes) *out_bytes = 0;
    VorbisDerived d;
    int rc = vorbis_tick_derive(vs, n_streams, packets, n_packets, bytes, bytes_len, d);
    if (rc != SK_OK) return rc;
    d.tick.decode = [&](bool as_is, const std::function<uint8_t *(uint32_t, uint32_t)> &dst_of, const uint8_t *) {
        return vorbis_tick_decode(e, vs, packets, bytes, bytes_len, d, as_is, dst_of);
    };
    rc = tick_pcm_impl(e, d.ts.data(), n_streams, d.units.data(), (uint32_t)d.units.size(), bytes, bytes_len, out, out_cap, outs, outs_cap, n_outs, out_bytes,
                       &d.tick);
    if (rc != SK_OK) return rc;  // the carries are the caller's: untouched
    for (uint32_t i = 0; i < n_streams; ++i) {
        std::memcpy(vs[i].overlap, d.overlap[i].data(), d.overlap[i].size() * 4);
        vs[i].prev_blocksize = d.prev[i];
    }
    for (uint32_t g = 0; g < n_packets; ++g) status_per_packet[g] = d.status[g];
    // the records of a stream delivered as decoded say what its packets are: one per packet that yielded frames
    std::vector<uint32_t> seen(n_streams, 0), first_unit(n_streams, 0);
    for (uint32_t i = 1; i < n_streams; ++i) first_unit[i] = first_unit[i - 1] + d.ts[i - 1].n_units;
    for (uint32_t k = 0; k < *n_outs; ++k) {
        sk_tick_output &o = outs[k];
        const uint32_t i = o.stream_index;
        if (!d.tick.plain[i]) continue;
        const uint32_t g = d.packet_of[first_unit[i] + seen[i]++];
        o.frames = d.frames[g], o.channels = d.ts[i].channels, o.bits = 16, o.status = 0;
    }
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_tick_run_vorbis");
}

int sk_vorbis_entropy_decode(sk_engine *e, const sk_vorbis_stream *streams, uint32_t n_streams, const sk_vorbis_packet *packets, uint32_t n_packets,
                             const uint8_t *bytes, size_t bytes_len, sk_vorbis_packet_info *info, float *residue, size_t residue_cap, size_t *residue_len) try {
    sk::abi_enter();
    if (residue_cap > SIZE_MAX / 4) return SK_ERR_INVALID_ARG;
    return vorbis_run(e, const_cast<sk_vorbis_stream *>(streams), n_streams, packets, n_packets, bytes, bytes_len, kVorbisEntropy, residue, residue_cap * 4,
                      residue_len, nullptr, nullptr, info);
} catch (...) {
    return sk::abi_caught("sk_vorbis_entropy_decode");
}

}  // extern "C"

// ---- VorbisPacketDecoder and VorbisDecoder (soundkit-vorbis/src/lib.rs) over the calls above -----------------------------------------

struct sk_vorbis_packet_decoder {
    sk_engine *eng = nullptr;
    int headers = 0;  // header packets taken: 0 ... 3
    sk_vorbis::Ident ident;
    std::unique_ptr<sk_vorbis_setup> setup;
    std::vector<float> overlap;
    uint32_t prev_blocksize = 0;
    std::string error;

    // the three headers in order; SK_OK or the parser's status with its text in error
    int header(const uint8_t *p, size_t len) {
        int rc = SK_OK;
        if (headers == 0) {
            rc = sk_vorbis::parse_ident(p, len, &ident, &error);
        } else if (headers == 1) {
            rc = sk_vorbis::parse_comment(p, len, &error);
        } else {
            std::unique_ptr<sk_vorbis_setup> s(new sk_vorbis_setup());
            rc = sk_vorbis::parse_setup(p, len, ident, &s->setup, &error);
            if (rc == SK_OK) {
                setup = std::move(s);
                overlap.assign((size_t)ident.channels * (ident.blocksize_1 / 2), 0.0f);
            }
        }
        if (rc == SK_OK) ++headers;
        return rc;
    }
};

struct sk_vorbis_decoder {
    sk_vorbis_packet_decoder dec;
    sk_ogg::Parser parser;
    uint32_t serial = 0;
    bool have_absgp = false, dead = false;
    uint64_t absgp = 0;
    std::vector<int16_t> pending;  // samples a call could not hand over (SK_ERR_CAPACITY): the next call's first
    std::string error;
};

namespace {

// the audio packets of one call through sk_vorbis_decode_packets' body -> their samples, one vector per packet
int vorbis_decode_some(sk_vorbis_packet_decoder &d, const std::vector<const std::vector<uint8_t> *> &packets, std::vector<std::vector<int16_t>> *out,
                       std::vector<int32_t> *status) {
    const uint32_t n = (uint32_t)packets.size();
    std::vector<uint8_t> bytes;
    std::vector<sk_vorbis_packet> table(n);
    for (uint32_t i = 0; i < n; ++i) {
        bytes.resize((bytes.size() + 15) & ~(size_t)15);
        table[i] = {(uint32_t)bytes.size(), (uint32_t)packets[i]->size()};
        bytes.insert(bytes.end(), packets[i]->begin(), packets[i]->end());
    }
    if (bytes.empty()) bytes.resize(16);
    const uint32_t ch = d.ident.channels;
    std::vector<int16_t> pcm((size_t)n * (d.ident.blocksize_1 / 2) * ch + 8);
    std::vector<uint32_t> frames(n);
    status->assign(n, 0);
    sk_vorbis_stream st{d.setup.get(), d.overlap.data(), n, d.prev_blocksize};
    size_t used = 0;
    const int rc = vorbis_run(d.eng, &st, 1, table.data(), n, bytes.data(), bytes.size(), kVorbisS16, pcm.data(), pcm.size() * 2, &used, status->data(),
                              frames.data(), nullptr);
    if (rc != SK_OK) return rc;
    d.prev_blocksize = st.prev_blocksize;
    out->clear();
    size_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        out->emplace_back(pcm.begin() + (ptrdiff_t)at, pcm.begin() + (ptrdiff_t)(at + (size_t)frames[i] * ch));
        at += (size_t)frames[i] * ch;
    }
    return SK_OK;
}

// VorbisDecoder::process_packet over the packets that became complete, the audio ones in one launch sequence
int vorbis_decoder_process(sk_vorbis_decoder *d, std::vector<int16_t> *samples) {
    auto fail = [&](int rc, const std::string &text) {
        d->error = text, d->dead = true;
        d->parser.pending.clear();
        return rc;
    };
    std::vector<sk_ogg::Packet> audio;
    while (!d->parser.pending.empty()) {
        sk_ogg::Packet p = std::move(d->parser.pending.front());
        d->parser.pending.pop_front();
        if (d->dec.headers == 0) {
            if (!p.first_in_stream) return fail(SK_VORBIS_ERR_STREAM, "Expected Vorbis identification header as first Ogg packet");
            if (const int rc = d->dec.header(p.data.data(), p.data.size())) return fail(rc, d->dec.error);
            d->serial = p.serial;
            continue;
        }
        if (p.serial != d->serial) return fail(SK_VORBIS_ERR_STREAM, "Unexpected second Ogg logical bitstream");
        if (d->dec.headers < 3) {
            if (const int rc = d->dec.header(p.data.data(), p.data.size())) return fail(rc, d->dec.error);
        } else {
            audio.push_back(std::move(p));
        }
    }
    if (audio.empty()) return SK_OK;
    std::vector<const std::vector<uint8_t> *> ptrs;
    for (auto &p : audio) ptrs.push_back(&p.data);
    std::vector<std::vector<int16_t>> pcm;
    std::vector<int32_t> status;
    if (const int rc = vorbis_decode_some(d->dec, ptrs, &pcm, &status)) return fail(rc, sk_strerror(rc));
    const uint32_t ch = d->dec.ident.channels;
    for (size_t i = 0; i < audio.size(); ++i) {
        if (status[i] != 0) return fail(status[i], std::string("Vorbis packet: ") + sk_strerror(status[i]));
        size_t frames = pcm[i].size() / ch;
        // the reference's truncation: only once cur_absgp is known, only on the stream's last packet
        if (d->have_absgp && audio[i].last_in_stream && audio[i].has_granule) {
            const uint64_t left = audio[i].granule_position > d->absgp ? audio[i].granule_position - d->absgp : 0;
            if (left < frames) frames = (size_t)left;
        }
        if (audio[i].last_in_page) {
            if (audio[i].has_granule) d->have_absgp = true, d->absgp = audio[i].granule_position;
        } else if (d->have_absgp) {
            d->absgp += frames;
        }
        samples->insert(samples->end(), pcm[i].begin(), pcm[i].begin() + (ptrdiff_t)(frames * ch));
    }
    return SK_OK;
}

// hands `samples` (behind what an earlier call left pending) to the caller, or keeps them for the next call
int vorbis_decoder_deliver(sk_vorbis_decoder *d, std::vector<int16_t> &samples, int16_t *out, size_t out_cap, size_t *written) {
    d->pending.insert(d->pending.end(), samples.begin(), samples.end());
    *written = d->pending.size();
    if (d->pending.size() > out_cap || (!out && !d->pending.empty())) {
        d->error = "Output buffer too small for Vorbis decode: need " + std::to_string(d->pending.size()) + ", have " + std::to_string(out_cap);
        return SK_ERR_CAPACITY;
    }
    if (!d->pending.empty()) std::memcpy(out, d->pending.data(), d->pending.size() * 2);
    d->pending.clear();
    return SK_OK;
}

}  // namespace

extern "C" {

int sk_vorbis_packet_decoder_create(sk_engine *e, sk_vorbis_packet_decoder **out) try {
    sk::abi_enter();
    if (!e || !out) return SK_ERR_INVALID_ARG;
    *out = new sk_vorbis_packet_decoder();
    (*out)->eng = e;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_vorbis_packet_decoder_create");
}

void sk_vorbis_packet_decoder_destroy(sk_vorbis_packet_decoder *d) try {
    sk::abi_enter();
    delete d;
} catch (...) {
    (void)sk::abi_caught("sk_vorbis_packet_decoder_destroy");
}

int sk_vorbis_packet_decoder_info(const sk_vorbis_packet_decoder *d, uint32_t *sample_rate, uint8_t *channels, size_t *maximum_samples) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    if (d->headers == 0) return SK_ERR_BAD_STREAM;
    if (sample_rate) *sample_rate = d->ident.sample_rate;
    if (channels) *channels = d->ident.channels;
    if (maximum_samples) *maximum_samples = (size_t)d->ident.channels * (d->ident.blocksize_1 / 2);
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_vorbis_packet_decoder_info");
}

int sk_vorbis_packet_decoder_decode_packet(sk_vorbis_packet_decoder *d, const uint8_t *packet, size_t len, int16_t *out, size_t out_cap, size_t *written,
                                           int *produced) try {
    sk::abi_enter();
    if (!d || (len && !packet) || !written || !produced) return SK_ERR_INVALID_ARG;
    *written = 0, *produced = 0;
    d->error.clear();
    if (len > sk_ogg::kMaxPacketBytes) {
        d->error = "Vorbis packet exceeds the " + std::to_string(sk_ogg::kMaxPacketBytes) + " byte budget";
        return SK_VORBIS_ERR_STREAM;
    }
    if (d->headers < 3) return d->header(packet, len);
    if (out_cap < (size_t)d->ident.channels * (d->ident.blocksize_1 / 2) || !out) {
        d->error = "Output buffer too small for Vorbis decode";
        return SK_ERR_CAPACITY;
    }
    const std::vector<uint8_t> one(packet, packet + len);
    std::vector<std::vector<int16_t>> pcm;
    std::vector<int32_t> status;
    if (const int rc = vorbis_decode_some(*d, {&one}, &pcm, &status)) return rc;
    if (status[0] != 0) {
        d->error = std::string("Vorbis packet: ") + sk_strerror(status[0]);
        return status[0];
    }
    if (!pcm[0].empty()) std::memcpy(out, pcm[0].data(), pcm[0].size() * 2);
    *written = pcm[0].size(), *produced = 1;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_vorbis_packet_decoder_decode_packet");
}

const char *sk_vorbis_packet_decoder_last_error(const sk_vorbis_packet_decoder *d) try {
    sk::abi_enter();
    return d ? d->error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_vorbis_packet_decoder_last_error");
    return "";
}

int sk_vorbis_decoder_create(sk_engine *e, sk_vorbis_decoder **out) try {
    sk::abi_enter();
    if (!e || !out) return SK_ERR_INVALID_ARG;
    *out = new sk_vorbis_decoder();
    (*out)->dec.eng = e;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_vorbis_decoder_create");
}

void sk_vorbis_decoder_destroy(sk_vorbis_decoder *d) try {
    sk::abi_enter();
    delete d;
} catch (...) {
    (void)sk::abi_caught("sk_vorbis_decoder_destroy");
}

int sk_vorbis_decoder_info(const sk_vorbis_decoder *d, uint32_t *sample_rate, uint8_t *channels) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    if (d->dec.headers == 0) return SK_ERR_BAD_STREAM;
    if (sample_rate) *sample_rate = d->dec.ident.sample_rate;
    if (channels) *channels = d->dec.ident.channels;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_vorbis_decoder_info");
}

int sk_vorbis_decoder_add(sk_vorbis_decoder *d, const uint8_t *data, size_t len, int16_t *out, size_t out_cap, size_t *written) try {
    sk::abi_enter();
    if (!d || (len && !data) || !written) return SK_ERR_INVALID_ARG;
    *written = 0;
    if (d->dead) return SK_VORBIS_ERR_STREAM;
    if (!d->parser.add(data, len, &d->error)) {
        d->dead = true;
        return SK_VORBIS_ERR_STREAM;
    }
    std::vector<int16_t> samples;
    if (const int rc = vorbis_decoder_process(d, &samples)) return rc;
    return vorbis_decoder_deliver(d, samples, out, out_cap, written);
} catch (...) {
    return sk::abi_caught("sk_vorbis_decoder_add");
}

int sk_vorbis_decoder_finish(sk_vorbis_decoder *d, int16_t *out, size_t out_cap, size_t *written) try {
    sk::abi_enter();
    if (!d || !written) return SK_ERR_INVALID_ARG;
    *written = 0;
    if (d->dead) return SK_VORBIS_ERR_STREAM;
    std::vector<int16_t> samples;
    if (d->pending.empty()) {  // a repeated finish after SK_ERR_CAPACITY only delivers
        if (!d->parser.finish(&d->error)) {
            d->dead = true;
            return SK_VORBIS_ERR_STREAM;
        }
        if (const int rc = vorbis_decoder_process(d, &samples)) return rc;
    }
    return vorbis_decoder_deliver(d, samples, out, out_cap, written);
} catch (...) {
    return sk::abi_caught("sk_vorbis_decoder_finish");
}

const char *sk_vorbis_decoder_last_error(const sk_vorbis_decoder *d) try {
    sk::abi_enter();
    return d ? d->error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_vorbis_decoder_last_error");
    return "";
}

}  // extern "C"

extern "C" {

const char *sk_last_exception(void) { return sk::abi_message(); }

int sk_debug_throw_after(int n, int kind) {
    sk::g_abi_throw_kind.store(kind < 0 || kind > 2 ? 0 : kind, std::memory_order_relaxed);
    return sk::g_abi_throw_after.exchange(n < 0 ? -1 : n, std::memory_order_relaxed);
}

}  // extern "C"

// pipeline.cpp -- the batch scheduler: N ADTS AAC-LC streams -> one submission loop on one GPU.
//
// Replaces one `pipeline_worker` OS thread per stream (soundkit-decoder/src/lib.rs:2891-3038) while keeping the
// handle's contract (lib.rs:2788-2889): bounded input queue (128 chunks / 8 MiB, `send` never blocks and reports
// InputBufferFull), bounded output queue (16 AudioData: a stream whose consumer does not drain it stops being
// scheduled -- the blocking send of lib.rs:3238-3240), empty chunk = end of stream (flush), an error ends that
// stream only after the outputs produced before it (lib.rs:3131-3134).
//
//   send() -> per-stream input queue -> entropy workers (host threads, one stream at a time each: ADTS framing +
//   AAC-LC front-end, csrc/aac_frontend.cpp) -> the tick batch (pinned host memory) -> submission thread:
//   sk_tick_run (H2D, synthesis, s16, resampler, downmix, pack, D2H) -> per-stream output queues -> try_recv().
//
// Three batches rotate: the workers fill one while the GPU runs the second and the delivery thread hands out the
// results of the third.  A stream contributes at most
// `max_stream_frames_per_tick` access units to a batch and is not scheduled again until that batch has been
// delivered, so its frames reach the engine in order and its outputs never overtake each other.
#include "../../include/soundkit_amd.h"
#include "sk_abi.h"
#include "mp3_internal.h"  // sk_mp3_internal::PipelineGpuHooks: how this file reaches the device Huffman stage and the PCM tick
#include "alac_stream.h"
#include "caf_stream.h"
#include "ogg_stream.h"
#include "vorbis_stream.h"
#include "g72x_stream.h"
#include "gsm_stream.h"
#include "flac_stream.h"
#include "mp4_stream.h"
#include "webm_stream.h"
#include "ts_stream.h"
#include "avi_stream.h"
#include "ps_stream.h"
#include "pcm_stream.h"    // the WAV walker and the raw PCM framer

#include <hip/hip_runtime.h>

#include <sched.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

namespace {

constexpr size_t kMaxInputChunkBytes = 4u * 1024 * 1024;   // MAX_INPUT_CHUNK_BYTES, lib.rs:80
constexpr size_t kMaxQueuedInputBytes = 8u * 1024 * 1024;  // MAX_QUEUED_INPUT_BYTES, lib.rs:81
constexpr uint32_t kNoStream = 0xffffffffu;

struct Output {
    bool is_error = false;
    int32_t status = 0;
    uint32_t rate = 0, frames = 0;
    uint8_t bits = 0, channels = 0;
    uint8_t flags = 0;          // SK_AUDIO_FLOAT | SK_AUDIO_BIG_ENDIAN (sk_audio_info::reserved)
    std::vector<uint8_t> data;  // PCM bytes, or the error text
};

struct PStream {
    std::mutex mu;
    std::condition_variable cv_out;
    // guarded by mu
    bool open = false, busy = false, queued = false, finished = false, cancelled = false;
    bool out_listed = false;  // the handle sits in the pipeline's OutQueue (or has been handed to a waiter and not taken from since)
    std::deque<std::vector<uint8_t>> in;
    std::deque<Output> out;
    sk_decode_options opt{};
    std::atomic<size_t> queued_bytes{0};
    // owned by whichever worker holds the stream (busy)
    std::vector<uint8_t> pending;
    size_t pending_pos = 0;
    bool saw_eof = false;
    bool more = false;  // the last pass stopped at its frame limit: schedulable even with an empty input queue
    sk_aac_decoder *fe = nullptr;
    uint8_t asc[2] = {0, 0};
    uint32_t rate = 0, engine_stream = kNoStream;
    uint8_t channels = 0;
    bool resample = false;
    // which decoder the stream's first bytes select (detect_and_init_decoder, soundkit-decoder/src/lib.rs:3041-3053): 0 not known yet
    uint8_t codec = 0;
    std::vector<uint8_t> mp3_reservoir;  // main data of the frames seen so far (main_data_begin reaches back into it)
    uint32_t mp3_free_format = 0;        // a free-format stream's frame length once measured (sk_mp3_scan_free)
    uint8_t mpa_layer = 0;               // an MPEG audio stream's layer: that of its first confirmed frame, 0 = not known yet
    // WAV / raw PCM streams (FormatDecoder::Wav / RawPcm, lib.rs:2292-2297): the stream processor, and what its first piece decided
    std::unique_ptr<sk_pcm::WavStream> wav;
    std::unique_ptr<sk_pcm::RawPcmStream> raw;
    // a WAV stream of a coded tag (the walker's coded mode, beyond the reference): A-law / mu-law pieces are units of the AIFF tick
    // (aiff_enc says which), ADPCM blocks units of the ADPCM tick.  The fact cap is counted twice: by the worker that cuts the pieces
    // to it, and by the submission thread, whose count goes into the stream's row when its tick runs and comes back from it.
    bool wav_g711 = false, wav_adpcm = false;
    uint64_t wav_parse_left = 0, wav_tick_left = 0;
    // AIFF / AIFF-C streams (FormatDecoder::Aiff): the container walker; its pieces are source-encoded, the AIFF tick decodes them.
    // The IMA4 carry belongs to the submission thread: it goes into the stream's row when its tick runs and comes back from it.
    std::unique_ptr<sk_pcm::AiffStream> aiff;
    uint8_t aiff_enc = 0;
    bool aiff_plain = false;  // nothing to change behind the decode
    sk_aiff_ima_state aiff_ima[2] = {};
    // FLAC streams (FormatDecoder::Flac): the reader; its frames are the units of the FLAC tick, which decodes them in front of what the
    // PCM tick would do.  flac_plain: nothing to change behind the decode (one AudioData per frame, in the depth STREAMINFO names)
    std::unique_ptr<sk_flac::Reader> flac;
    bool flac_plain = false;
    // ALAC packet streams (sk_pipeline_spawn_alac_packets): the cookie; every chunk is one packet, the unit of the ALAC tick, which decodes
    // it in front of what the PCM tick would do.  alac_plain: nothing to change behind the decode (one AudioData per packet)
    bool alac = false, alac_plain = false;
    sk_alac_config alac_cfg{};
    // headerless telephony streams (sk_pipeline_spawn_g711 / _g722 / _g726): the decoder's parameters come with the spawn; what a send
    // decodes now is one unit of the telephony tick, which decodes it in front of what the PCM tick would do.  The G.726 framer holds a
    // partial group back (worker thread); the codec's carry goes into every tick and comes back from it (submission thread)
    bool g72x = false;
    uint8_t g72x_codec = 0, g726_packing = 0;
    uint32_t g72x_rate = 0, g726_rate = 0;  // g72x_rate: the AudioData's sample rate
    uint8_t g72x_channels = 1;
    sk_g72x::G726Framer g726_framer;
    sk_g726_state g726_state{};
    sk_g722_state g722_state{};
    // GSM 06.10 streams (sk_pipeline_spawn_gsm): the same shape -- the framer holds a partial packet back (worker thread), the carry
    // goes into every tick and comes back from it (submission thread)
    bool gsm = false;
    uint8_t gsm_variant = 0;
    sk_gsm::Framer gsm_framer;
    sk_gsm_state gsm_state{};
    // Vorbis streams: Ogg bytes the sniffing spawn took by their first page (vorbis_ogg: the page and packet parser runs on the worker
    // thread) or demuxed packets (sk_pipeline_spawn_vorbis_packets: the three headers came with the spawn, every send is one audio
    // packet).  Audio packets are the units of the Vorbis tick.  Worker thread: the headers, the block size of the last packet read
    // (the frames a packet yields follow from it) and the Ogg decoder's granule bookkeeping.  Submission thread: the carry -- the block
    // size of the last packet DECODED and its overlap half -- goes into every tick and comes back from it
    bool vorbis = false, vorbis_ogg = false, ogg_finished = false, vorbis_have_absgp = false;
    int vorbis_headers = 0;
    std::unique_ptr<sk_ogg::Parser> ogg;
    sk_vorbis::Ident vorbis_ident;
    std::shared_ptr<sk_vorbis_setup> vorbis_setup;
    std::vector<float> vorbis_overlap;
    uint32_t vorbis_prev = 0, vorbis_parse_prev = 0, ogg_serial = 0;
    uint64_t vorbis_absgp = 0;
    // MP4 / M4A streams (the sniffing spawn took them by their `ftyp`): the demuxer runs on the worker thread; every AAC sample leaves it
    // wrapped in an ADTS header and is appended to `pending`, where the ADTS pass finds it as it finds an ADTS stream's frame.  mp4_error:
    // what ends the stream once the frames in front of it have gone; mp4_done: nothing more is pulled
    std::unique_ptr<sk_mp4::Demuxer> mp4;
    bool mp4_checked = false, mp4_done = false, mp4_flac_head = false;  // mp4_flac_head: a `fLaC` track's configuration has still to go to the reader
    std::string mp4_error;
    // WebM / Matroska streams (taken by their EBML magic): the demuxer runs on the worker thread.  At the first Cluster its single audio
    // track decides where the frames go (webm_open), and the stream is from then on a Vorbis stream whose packets come from the demuxer,
    // an ADTS stream (every frame wrapped in seven bytes, as an MP4 sample is) or a native FLAC stream (the CodecPrivate, then the
    // frames).  webm_error: what ends the stream once the units in front of it have gone; webm_done: nothing more is pulled
    std::unique_ptr<sk_webm::Demuxer> webm;
    bool webm_routed = false, webm_done = false, webm_flac_head = false;
    uint32_t webm_rate = 0, webm_channels = 0;  // A_AAC: the AudioSpecificConfig's, for the ADTS headers
    std::string webm_error;
    // MPEG transport streams (taken by sk_ts::sniff, or sk_pipeline_spawn_mpeg_ts): the demuxer runs on the worker thread.  The config
    // that comes with the track's first packet decides where the packets go (ts_open): ADTS frames and MPEG audio frames are appended to
    // `pending`, where the ADTS pass and the MPEG audio passes find them as they find an elementary stream's (pull_input goes through
    // the demuxer); a Blu-ray LPCM stream is a raw PCM stream whose pieces are the PES payloads.  ts_error: what ends the stream once the
    // units in front of it have gone; ts_done: nothing more is pulled
    std::unique_ptr<sk_ts::Demuxer> ts;
    bool ts_routed = false, ts_done = false;
    std::string ts_error;
    // AVI and MPEG program streams (taken by their magic): the demuxer runs on the worker thread.  Its config event decides what the
    // stream is from there on (avi_open / ps_open): a PCM track a raw PCM stream whose pieces are the demuxer's packets -- source-encoded
    // where raw_enc says so (AVI's 8-bit samples, DVD LPCM's 24-bit groups: units of the AIFF tick, aiff_enc says which) -- and an MPEG
    // audio track an MPEG audio stream, the payloads appended to `pending` as a transport stream's are.  cont_error: what ends the stream
    // once the units in front of it have gone; cont_done: nothing more is pulled
    std::unique_ptr<sk_avi::Demuxer> avi;
    std::unique_ptr<sk_ps::Demuxer> ps;
    bool cont_routed = false, cont_done = false, raw_enc = false;
    std::string cont_error;
    std::vector<uint8_t> cont_piece;  // the packet a PCM pass is working through
    size_t cont_piece_pos = 0;
    sk_raw_pcm_format raw_format{};  // sk_pipeline_spawn_raw_pcm's
    bool pcm_detected = false;       // WAV: the detection buffer has gone through the processor
    uint8_t pcm_route = 0;           // 0 not decided yet, kPcmFast: pieces are delivered as they are, kPcmTick: units of the PCM tick
    uint8_t pcm_fmt = 0, pcm_flags = 0;  // SK_FMT_* of the source (kPcmTick) / SK_AUDIO_* of its pieces
    uint8_t pcm_bits = 0;
    uint32_t pcm_fill = 0;           // frames waiting in the resampler's chunk, mirrored for the output-room estimate
};
constexpr uint8_t kCodecAac = 1, kCodecMp3 = 2, kCodecWav = 3, kCodecRawPcm = 4, kCodecAiff = 5, kCodecFlac = 6, kCodecAlac = 7, kCodecG72x = 8, kCodecGsm = 9, kCodecVorbis = 10, kCodecMp4 = 11, kCodecWebm = 12, kCodecTs = 13, kCodecAvi = 14, kCodecPs = 15;
constexpr uint8_t kPcmFast = 1, kPcmTick = 2, kPcmAiffTick = 3, kPcmFlacTick = 4, kPcmAlacTick = 5, kPcmG72xTick = 6, kPcmGsmTick = 7, kPcmVorbisTick = 8, kPcmWavAdpcmTick = 9;  // kPcmAiffTick: units of the AIFF tick (decode, then whatever the PCM tick would do)
// The PCM input of one tick (and so of one worker pass): pieces are staged in a pinned buffer of this size per batch, each at a
// 16-byte aligned offset.  A piece is never split: one `add` takes at most 4 MiB and returns at most that plus a carried partial frame.
constexpr size_t kPcmTickBytes = 32u * 1024 * 1024;
constexpr size_t kMaxMp4QueuedBytes = 4u * 1024 * 1024;  // MAX_AAC_BUFFERED_BYTES (soundkit-aac/src/lib.rs:22): AacDecoderMp4's queue of ADTS frames
constexpr size_t kMaxWebmQueuedBytes = 16u * 1024 * 1024;  // what a WebM stream's demuxer may hold as packets between two passes (half a tick's staging buffer)
constexpr size_t kMinDetectionBytes = 8192, kMaxDetectionBytes = 65536;  // MIN_ / MAX_DETECTION_BYTES, lib.rs:75-76

struct BatchEntry {  // bookkeeping beside one sk_tick_stream
    uint32_t handle = 0;
    bool eof = false;
    bool failed = false;
    int32_t fail_status = 0;
    std::string fail_msg;
    // quantised hand-over only: the access units of this pass as they came off the wire, so that a status the device finds
    // (stereo tools, TNS, the unit's tail) can be given the reference's message by parsing them again on the host
    std::vector<uint8_t> raw;
    std::vector<uint32_t> raw_len;
    // a WAV / raw PCM stream's pass: it has no row in the AAC / MP3 tick; `pre` are the pieces of a fast-path stream (lib.rs:3339-3345),
    // delivered as they are, in front of whatever the PCM tick gives the entry (nothing, for such a stream)
    bool pcm = false, pcm_row = false;  // pcm_row: it has a row in the batch's PCM tick
    std::vector<Output> pre;
};

// The table of one PCM-family tick (WAV / raw PCM, AIFF, FLAC): a row per stream that brings units or ends a resampler, the units stream
// after stream (their offsets into Batch::pcm_bytes), entry[row] = the row's batch entry, and -- submission thread -- the records the
// tick's bound call allows it
template <class Row, class Unit>
struct TickTable {
    std::vector<Row> rows;
    std::vector<Unit> units;
    std::vector<uint32_t> entry;
    uint32_t max_out = 0;
    void clear() {
        rows.clear();
        units.clear();
        entry.clear();
        max_out = 0;
    }
};

struct Batch {
    float *coeffs = nullptr;  // pinned
    size_t coeff_cap = 0, n_floats = 0;
    std::vector<sk_aac_frame_desc> descs;  // sized once (max_frames_per_tick): workers fill disjoint ranges without the lock
    size_t n_descs = 0;
    // gpu_entropy mode: the raw access units instead of spectra (each unit 4-byte aligned, >= 8 zero bytes after it)
    uint8_t *au_bytes = nullptr;  // pinned
    size_t au_cap = 0, au_used = 0;
    std::vector<sk_au_item> units;  // sized once, indexed like descs
    std::vector<sk_tick_stream> ts;
    std::vector<BatchEntry> entries;
    // MP3 streams' granules (their units), in the order of their streams in ts; sized by ensure_mp3 at the first MP3 stream
    std::vector<sk_mp3_requant_granule> mp3_gr;
    std::vector<sk_mp3_granule_desc> mp3_desc;
    int16_t *mp3_is = nullptr;  // pinned: [granule][channel][576], 2 x 576 per granule reserved
    size_t n_mp3 = 0, mp3_rows = 0;
    // the same streams with the Huffman stage on the device (sk_lane::mp3_gpu): frames whose main data lies in au_bytes, and how
    // many of them each entry of ts brought (ts itself keeps counting granules: the budget and the output bound are in granules)
    std::vector<sk_mp3_frame_item> mp3_frames;
    std::vector<uint32_t> mp3_frames_of;
    size_t n_mp3_frames = 0;
    // Layer I / II streams' frames (sk_tick_run_mixed_mpa through pipeline_gpu_hooks()), in the order of their streams in ts: records and
    // the frames' bytes (each 4-byte aligned, 8 bytes of room behind it); appended under batch_mu, they are small
    std::vector<sk_mpa_frame_record> mpa_recs;
    std::vector<uint8_t> mpa_bytes;
    // WAV / raw PCM streams' pieces (sk_tick_run_pcm through pipeline_gpu_hooks()), AIFF streams' pieces (sk_tick_run_aiff) and FLAC streams'
    // frames (sk_tick_run_flac): all staged in pcm_bytes (pinned, ensure_pcm), a table per tick; the statuses the device gives the frames
    uint8_t *pcm_bytes = nullptr;
    size_t pcm_cap = 0, pcm_used = 0;
    TickTable<sk_pcm_tick_stream, sk_pcm_unit> pcm_ts;
    TickTable<sk_aiff_tick_stream, sk_pcm_unit> aiff_ts;
    TickTable<sk_wav_adpcm_tick_stream, sk_pcm_unit> wav_ts;  // WAV ADPCM streams' blocks (sk_tick_run_wav_adpcm)
    std::vector<int32_t> wav_status;
    TickTable<sk_flac_tick_stream, sk_flac_frame_info> flac_ts;
    std::vector<int32_t> flac_status;
    TickTable<sk_alac_tick_stream, sk_alac_tick_packet> alac_ts;  // ALAC streams' packets (sk_tick_run_alac)
    std::vector<int32_t> alac_status;
    TickTable<sk_g72x_tick_stream, sk_pcm_unit> g72x_ts;  // telephony streams' units (sk_tick_run_g72x); row k's carry is record k of both arrays
    std::vector<sk_g726_state> g726_states;
    std::vector<sk_g722_state> g722_states;
    TickTable<sk_gsm_tick_stream, sk_pcm_unit> gsm_ts;  // GSM streams' units (sk_tick_run_gsm); row k's carry is record k
    std::vector<sk_gsm_state> gsm_states;
    TickTable<sk_vorbis_tick_stream, sk_vorbis_tick_packet> vorbis_ts;  // Vorbis streams' packets (sk_tick_run_vorbis); the carry is the stream's own
    std::vector<int32_t> vorbis_status;
    uint32_t writers = 0;  // claims whose memcpy is still running
    // the tick's results, handed from the submission thread to the delivery thread
    uint8_t *out_pinned = nullptr;
    size_t out_pinned_cap = 0;
    std::vector<sk_tick_output> recs;
    std::vector<uint32_t> row_of;  // tick row -> entry
    std::vector<uint32_t> entry_row;  // entry -> tick row, kNoStream for a stream that never reached the device
    std::vector<uint32_t> rec_begin;  // tick row -> its first output record (rows + 1 entries)
    uint32_t n_out = 0;
    int rc = SK_OK;
    uint32_t next_slice = 0, slices_done = 0;  // delivery threads share a batch row-wise (guarded by batch_mu)
    void clear() {
        n_floats = 0;
        n_descs = 0;
        au_used = 0;
        n_mp3 = 0;
        mp3_rows = 0;
        n_mp3_frames = 0;
        mp3_frames_of.clear();
        mpa_recs.clear();
        mpa_bytes.clear();
        pcm_used = 0;
        pcm_ts.clear();
        aiff_ts.clear();
        wav_ts.clear();
        flac_ts.clear();
        alac_ts.clear();
        g72x_ts.clear();
        gsm_ts.clear();
        vorbis_ts.clear();
        ts.clear();
        entries.clear();
        row_of.clear();
        entry_row.clear();
        rec_begin.clear();
        n_out = 0;
        rc = SK_OK;
        next_slice = slices_done = 0;
    }
};

}  // namespace

// handles with something to receive (outputs or the end of the stream), for callers that serve many handles; one queue
// for all lanes of a pipeline, holding public handles
struct OutQueue {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<uint32_t> ready;
    bool stop = false;
};

// One lane = one engine + the threads and batches that feed it.  A pipeline is one or more lanes behind one handle
// space: ticks of different engines overlap on the device (a tick is a chain of dependent launches with a
// synchronisation at its end), which one lane's submission thread cannot do by itself.
struct sk_lane {
    sk_engine *engine = nullptr;
    OutQueue *oq = nullptr;
    uint32_t lane_index = 0, n_lanes = 1;  // public handle = handle * n_lanes + lane_index
    sk_pipeline_config cfg{};
    std::vector<std::unique_ptr<PStream>> streams;
    std::mutex handles_mu;
    std::vector<uint32_t> free_handles;

    std::mutex rq_mu;
    std::condition_variable rq_cv;
    std::deque<uint32_t> ready;

    std::mutex batch_mu;
    std::condition_variable batch_cv;   // submission thread: work arrived / writers done
    std::condition_variable room_cv;    // workers: the filling batch has room again
    size_t au_pass_budget = 0;          // gpu_entropy: access-unit bytes one worker pass may stage (= what an empty batch holds)
    std::atomic<size_t> out_cap_seen{0};  // the largest pinned output buffer a batch of this lane has asked for
    static constexpr int kBatches = 3;  // one filling, one on the GPU, one being delivered
    Batch batches[kBatches];
    int filling = 0;
    std::deque<int> free_batches, to_deliver;
    std::condition_variable deliver_cv;
    bool stop = false;
    std::atomic<int> fatal{0};  // != 0: a thread of the lane died of an exception (lane_fatal); every stream got that error
    // MP3: the standard's tables, made (and installed on the engine) when the first MP3 stream shows up
    std::mutex mp3_mu;
    sk_mp3_codebook *mp3_cb = nullptr;
    std::atomic<bool> mp3_ready{false};
    // gpu_entropy = 3: the MP3 streams' passes stop behind the bit reservoir; scale factors and Huffman codes are the tick's
    // (sk_tick_run_mixed_mpa, reached through pipeline_gpu_hooks()).  cfg.gpu_entropy holds 1 then: the AAC streams' mode.
    bool mp3_gpu = false;
    std::vector<uint32_t> mp3_blob;  // mp3_cb flattened for the device (sk_mp3_codebook_flatten)
    // WAV / raw PCM: the batches' pinned byte buffers, made when the first stream that needs the PCM tick shows up
    std::mutex pcm_mu;
    std::atomic<bool> pcm_ready{false};

    std::vector<std::thread> workers;
    std::thread submitter;
    std::vector<std::thread> deliverers;
    uint32_t n_deliver = 1;

    std::atomic<uint64_t> n_ticks{0}, n_frames{0}, n_outputs{0}, n_errors{0}, parse_ns{0}, tick_ns{0}, idle_ns{0}, deliver_ns{0};
    // SK_PIPELINE_WATCHDOG=<seconds>: a thread that prints where everybody stands when no tick has finished for that long
    std::thread watchdog;
    std::atomic<int> submit_where{0};     // 0 waits for work, 1 lets the batch fill, 2 waits for writers / a free batch, 3 in the tick, 4 hands over
    std::atomic<uint32_t> workers_waiting_room{0}, workers_waiting_ready{0}, workers_parsing{0}, deliverers_waiting{0};
};

namespace {

using Clock = std::chrono::steady_clock;
uint64_t ns_since(Clock::time_point t0) {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() - t0).count();
}

// call with s.mu held: true = the stream has work, is free and is not in the ready queue yet (now marked as queued)
bool mark_schedulable(sk_lane *p, PStream &s) {
    if (!s.open || s.busy || s.queued || s.finished || s.cancelled) return false;
    if ((s.in.empty() && !s.more) || s.out.size() >= p->cfg.output_buffer) return false;
    s.queued = true;
    return true;
}

// call with s.mu held
void maybe_schedule(sk_lane *p, PStream &s, uint32_t handle) {
    if (!mark_schedulable(p, s)) return;
    {
        std::lock_guard<std::mutex> lk(p->rq_mu);
        p->ready.push_back(handle);
    }
    p->rq_cv.notify_one();
}

// Gives back what a stream holds outside the scheduler.  Two threads can get here for the same stream -- the delivery
// thread for a stream that has just finished, and a caller cancelling that same handle the moment it saw the end -- so the
// resources are taken over under the stream's lock and released once.
void release_device_side(sk_lane *p, PStream &s) {
    uint32_t engine_stream;
    sk_aac_decoder *fe;
    {
        std::lock_guard<std::mutex> lk(s.mu);
        engine_stream = s.engine_stream;
        s.engine_stream = kNoStream;
        fe = s.fe;
        s.fe = nullptr;
        s.pending.clear();
        s.pending.shrink_to_fit();
        s.pending_pos = 0;
        s.mp3_reservoir.clear();
        s.mp3_reservoir.shrink_to_fit();
        s.wav.reset();
        s.raw.reset();
        s.aiff.reset();
        s.flac.reset();
    }
    if (engine_stream != kNoStream) (void)sk_stream_close(p->engine, engine_stream);  // also drops its resampler
    if (fe) sk_aac_decoder_destroy(fe);
}

struct Parsed {  // what one worker pass produced for one stream
    uint32_t n_frames = 0;
    size_t n_floats = 0;
    size_t n_au_bytes = 0;  // gpu_entropy: bytes staged (units padded as the device wants them)
    bool eof = false, failed = false;
    bool budget_stop = false;  // stopped early because the staged bytes reached what one batch can take
    int32_t fail_status = 0;
    std::string fail_msg;
    std::vector<uint8_t> raw;  // quantised hand-over: the pass's access units, kept for the error text (BatchEntry::raw)
    std::vector<uint32_t> raw_len;
    // an MP3 stream's pass: n_frames counts GRANULES (the tick's units for such a stream)
    bool mp3 = false;
    std::vector<sk_mp3_requant_granule> mp3_gr;
    std::vector<sk_mp3_granule_desc> mp3_desc;
    std::vector<int16_t> mp3_is;
    // ... or, with the Huffman stage on the device, its frames (byte_offset into mp3_bytes; n_au_bytes = mp3_bytes.size())
    std::vector<sk_mp3_frame_item> mp3_frames;
    std::vector<uint8_t> mp3_bytes;
    // a Layer I / II stream's pass: n_frames counts FRAMES (whole frames are what such a stream is budgeted in); byte_offset into mpa_bytes
    bool mpa = false;
    std::vector<sk_mpa_frame_record> mpa_recs;
    std::vector<uint8_t> mpa_bytes;
    // a WAV / raw PCM stream's pass (n_frames stays 0): pieces for the PCM tick, each at a 16-byte aligned offset of pcm_bytes, or --
    // fast path -- finished outputs; `more`: the pass stopped at a limit with input left
    bool pcm = false, more = false;
    std::vector<uint8_t> pcm_bytes;
    std::vector<sk_pcm_unit> pcm_units;
    std::vector<sk_flac_frame_info> flac_frames;  // a FLAC stream's pass: one per unit, offset into pcm_bytes
    std::vector<sk_alac_tick_packet> alac_packets;  // an ALAC stream's pass: one per unit, offset into pcm_bytes
    std::vector<sk_vorbis_tick_packet> vorbis_packets;  // a Vorbis stream's pass: one per unit, offset into pcm_bytes
    std::vector<Output> pre;
    bool fail(int32_t st, const std::string &msg) {  // the pass ends its stream with this error; false, for a caller that returns it
        failed = true;
        fail_status = st;
        fail_msg = msg;
        return false;
    }
};

// What a routed transport stream's demuxer has handed out joins `pending`: ADTS frames and MPEG audio frames one after the other are the
// elementary stream.  (A Blu-ray LPCM track's packets wait in the demuxer as the pieces of the PCM pass.)
void ts_drain(PStream &s) {
    if (!s.ts_routed || s.codec == kCodecRawPcm) return;
    if (s.pending_pos > 0 && s.pending_pos >= s.pending.size() / 2) {  // compact
        s.pending.erase(s.pending.begin(), s.pending.begin() + (ptrdiff_t)s.pending_pos);
        s.pending_pos = 0;
    }
    while (!s.ts->packets.empty()) {
        const sk_ts::Packet pk = s.ts->take_packet();
        s.pending.insert(s.pending.end(), pk.data.begin(), pk.data.end());
    }
}

// A transport stream's demuxer takes a chunk, or (end) the end of the input.  A refusal is kept for when the units in front of it have
// gone, and ends the input: the passes see the end of their elementary stream.
void ts_feed(PStream &s, const uint8_t *data, size_t len, bool end) {
    sk_ts::Demuxer &t = *s.ts;
    if (end) {
        s.ts_done = true;
        (void)t.finish();
    } else {
        (void)t.add(data, len);
    }
    if (t.failed && s.ts_error.empty()) s.ts_error = t.error;
    ts_drain(s);
    if (!s.ts_error.empty()) s.ts_done = s.saw_eof = true;
}

// pull_input for a transport stream
int ts_pull(PStream &s) {
    if (s.ts_done) return 0;
    std::vector<uint8_t> chunk;
    {
        std::lock_guard<std::mutex> lk(s.mu);
        if (s.in.empty()) return 0;
        chunk = std::move(s.in.front());
        s.in.pop_front();
    }
    if (chunk.empty()) {
        s.saw_eof = true;
        ts_feed(s, nullptr, 0, true);
        return -1;
    }
    s.queued_bytes.fetch_sub(chunk.size());
    ts_feed(s, chunk.data(), chunk.size(), false);
    return 1;
}

// The same three for an AVI or a program stream.  cont_take: the demuxer's first waiting packet, into `out`
bool cont_has_packets(const PStream &s) { return s.avi ? !s.avi->packets.empty() : !s.ps->packets.empty(); }
void cont_take(PStream &s, std::vector<uint8_t> &out) {
    if (s.avi) out = s.avi->take_packet().data;
    else out = s.ps->take_packet().data;
}
void cont_drain(PStream &s) {
    if (!s.cont_routed || s.codec == kCodecRawPcm) return;
    if (s.pending_pos > 0 && s.pending_pos >= s.pending.size() / 2) {  // compact
        s.pending.erase(s.pending.begin(), s.pending.begin() + (ptrdiff_t)s.pending_pos);
        s.pending_pos = 0;
    }
    std::vector<uint8_t> data;
    while (cont_has_packets(s)) {
        cont_take(s, data);
        s.pending.insert(s.pending.end(), data.begin(), data.end());
    }
}
void cont_feed(PStream &s, const uint8_t *data, size_t len, bool end) {
    if (end) s.cont_done = true;
    const bool ok = s.avi ? (end ? s.avi->finish() : s.avi->add(data, len)) : (end ? s.ps->finish() : s.ps->add(data, len));
    if (!ok && s.cont_error.empty()) s.cont_error = s.avi ? s.avi->error : s.ps->error;
    cont_drain(s);
    if (!s.cont_error.empty()) s.cont_done = s.saw_eof = true;
}
int cont_pull(PStream &s) {
    if (s.cont_done) return 0;
    std::vector<uint8_t> chunk;
    {
        std::lock_guard<std::mutex> lk(s.mu);
        if (s.in.empty()) return 0;
        chunk = std::move(s.in.front());
        s.in.pop_front();
    }
    if (chunk.empty()) {
        s.saw_eof = true;
        cont_feed(s, nullptr, 0, true);
        return -1;
    }
    s.queued_bytes.fetch_sub(chunk.size());
    cont_feed(s, chunk.data(), chunk.size(), false);
    return 1;
}

// 1 = a chunk was appended to s.pending, 0 = nothing queued right now, -1 = the end-of-stream marker was taken (s.saw_eof set)
int pull_input(PStream &s) {
    if (s.ts) return ts_pull(s);  // (1: a chunk went through the demuxer, whatever it handed out)
    if (s.avi || s.ps) return cont_pull(s);
    std::vector<uint8_t> chunk;
    bool got = false;
    {
        std::lock_guard<std::mutex> lk(s.mu);
        if (!s.in.empty()) {
            chunk = std::move(s.in.front());
            s.in.pop_front();
            got = true;
        }
    }
    if (!got) return 0;
    if (chunk.empty()) {
        s.saw_eof = true;
        return -1;
    }
    s.queued_bytes.fetch_sub(chunk.size());
    if (s.pending_pos > 0 && s.pending_pos >= s.pending.size() / 2) {  // compact
        s.pending.erase(s.pending.begin(), s.pending.begin() + (ptrdiff_t)s.pending_pos);
        s.pending_pos = 0;
    }
    s.pending.insert(s.pending.end(), chunk.begin(), chunk.end());
    return 1;
}

// An MP4 stream's demuxer output joins `pending` as ADTS frames.  The config event comes first and decides what the stream is from there
// on: a `fLaC` track makes it a FLAC stream and an integer or f32 PCM track a raw PCM stream (s.codec changes; parse_some sends the pass
// to that stream's parser, which takes the packets from the demuxer).  No edit trim is applied, as none is for AAC.  Any other track
// that is not AAC, or an
// AudioSpecificConfig the AAC-LC config check refuses (sk_aac_decoder_create: explicit SBR or PS, another object type, 960-sample frames, a
// program config element, more than two channels), ends the stream before any audio.  AacDecoderMp4's queue budget holds.
void mp4_drain(PStream &s) {
    sk_mp4::Demuxer &m = *s.mp4;
    if (m.have_track && !s.mp4_checked && s.mp4_error.empty()) {
        s.mp4_checked = true;
        const sk_mp4::Track &t = m.track;
        if ((t.codec == sk_mp4::kCodecFlac || t.codec == sk_mp4::kCodecPcm) && t.fragmented) {  // described, not decoded: as decode_file says
            s.mp4_error = std::string("fragmented MP4 ") + (t.codec == sk_mp4::kCodecFlac ? "flac" : "pcm") + " tracks are not built";
        } else if (t.codec == sk_mp4::kCodecFlac) {  // as a WebM A_FLAC track: the configuration, then the packets, are a native FLAC stream
            s.codec = kCodecFlac;
            s.mp4_flac_head = true;
        } else if (t.codec == sk_mp4::kCodecPcm) {  // as a transport stream's LPCM: a raw PCM stream of the entry's format
            const uint32_t width = (t.bits + 7) / 8 * t.channels;
            if (t.pcm.is_float && t.bits == 64) {
                s.mp4_error = "MP4 64-bit float PCM is not decoded in a stream; decode the whole file (decode_file)";
            } else if ((t.bits != 16 && t.bits != 24 && t.bits != 32) || (t.pcm.is_float && t.bits != 32)) {
                s.mp4_error = "unsupported container PCM sample depth: " + std::to_string(t.bits);
            } else if (t.pcm.bytes_per_frame != width) {
                s.mp4_error = "MP4 PCM frames of " + std::to_string(t.pcm.bytes_per_frame) + " bytes are not " + std::to_string(t.channels) +
                              " channels of " + std::to_string(t.bits) + " packed bits";
            } else {
                const int le = t.pcm.is_float ? SK_FMT_F32LE : (t.bits == 16 ? SK_FMT_S16LE : (t.bits == 24 ? SK_FMT_S24LE : SK_FMT_S32LE));
                s.codec = kCodecRawPcm;
                s.raw_format = sk_raw_pcm_format{t.sample_rate, (uint8_t)t.channels, (uint8_t)(le + (t.pcm.big_endian ? 1 : 0)), 0};
                s.raw.reset(new sk_pcm::RawPcmStream(width));
            }
        } else if (t.codec != sk_mp4::kCodecAac) {
            s.mp4_error = "MP4/M4A audio track is not AAC";
        } else {
            static const uint8_t none[1] = {0};
            const std::vector<uint8_t> &asc = m.track.codec_private;
            sk_aac_decoder *probe = nullptr;
            const int rc = sk_aac_decoder_create(asc.empty() ? none : asc.data(), asc.size(), &probe);
            if (rc != SK_OK) s.mp4_error = std::string("AAC-LC decoder init: ") + sk_strerror(rc);
            sk_aac_decoder_destroy(probe);
        }
    }
    while (s.codec == kCodecMp4 && !m.packets.empty()) {  // (a FLAC or PCM track's packets wait in the demuxer for their pass)
        if (s.mp4_error.empty()) {
            const std::vector<uint8_t> &raw = m.packets.front().data;
            if (raw.size() + 7 > 8191) {
                s.mp4_error = "MP4 AAC sample of " + std::to_string(raw.size()) + " bytes exceeds an ADTS frame";
            } else if (s.pending.size() - s.pending_pos + raw.size() + 7 > kMaxMp4QueuedBytes) {
                s.mp4_error = "MP4 AAC packet queue exceeds the " + std::to_string(kMaxMp4QueuedBytes) + " byte streaming budget";
            } else {
                uint8_t head[7];
                sk_mp4::adts_header(m.track.codec_private.data(), m.track.codec_private.size(), m.track.sample_rate, m.track.channels, raw.size(), head);
                s.pending.insert(s.pending.end(), head, head + 7);
                s.pending.insert(s.pending.end(), raw.begin(), raw.end());
            }
        }
        m.packets.pop_front();
    }
    if (m.failed && s.mp4_error.empty()) s.mp4_error = m.error;
    if (!s.mp4_error.empty()) s.mp4_done = true;
}

// pull_input for an MP4 stream: the chunk goes through the demuxer; the end-of-stream marker finishes it
int pull_mp4(PStream &s) {
    if (s.mp4_done) return 0;
    std::vector<uint8_t> chunk;
    {
        std::lock_guard<std::mutex> lk(s.mu);
        if (s.in.empty()) return 0;
        chunk = std::move(s.in.front());
        s.in.pop_front();
    }
    if (s.pending_pos > 0 && s.pending_pos >= s.pending.size() / 2) {  // compact
        s.pending.erase(s.pending.begin(), s.pending.begin() + (ptrdiff_t)s.pending_pos);
        s.pending_pos = 0;
    }
    if (chunk.empty()) {
        s.saw_eof = true;
        s.mp4_done = true;
        (void)s.mp4->finish();
    } else {
        s.queued_bytes.fetch_sub(chunk.size());
        (void)s.mp4->add(chunk.data(), chunk.size());
    }
    mp4_drain(s);
    return chunk.empty() ? -1 : 1;
}

// A WebM stream's demuxer takes a chunk, or (end) the end of the input.  A refusal is kept for when the units in front of it have gone;
// so is a queue of packets beyond the budget (frames far smaller than their header-stripping prefix can make one out of a 4 MiB chunk).
void webm_feed(PStream &s, const uint8_t *data, size_t len, bool end) {
    sk_webm::Demuxer &w = *s.webm;
    if (end) {
        s.webm_done = true;
        (void)w.finish();
    } else {
        (void)w.add(data, len);
    }
    if (w.failed && s.webm_error.empty()) s.webm_error = w.error;
    if (s.webm_error.empty() && w.queued_bytes() > kMaxWebmQueuedBytes)
        s.webm_error = "WebM packet queue exceeds the " + std::to_string(kMaxWebmQueuedBytes) + " byte streaming budget";
    if (!s.webm_error.empty()) s.webm_done = true;
}

// pull_input for a WebM stream: the chunk goes through the demuxer; the end-of-stream marker finishes it
int webm_pull(PStream &s) {
    if (s.webm_done) return 0;
    std::vector<uint8_t> chunk;
    {
        std::lock_guard<std::mutex> lk(s.mu);
        if (s.in.empty()) return 0;
        chunk = std::move(s.in.front());
        s.in.pop_front();
    }
    if (chunk.empty()) {
        s.saw_eof = true;
        webm_feed(s, nullptr, 0, true);
        return -1;
    }
    s.queued_bytes.fetch_sub(chunk.size());
    webm_feed(s, chunk.data(), chunk.size(), false);
    return 1;
}

// An A_AAC track's frames join `pending` as ADTS frames, as an MP4 track's samples do (mp4_drain), under the same queue budget
void webm_drain_aac(PStream &s) {
    sk_webm::Demuxer &w = *s.webm;
    if (s.pending_pos > 0 && s.pending_pos >= s.pending.size() / 2) {  // compact
        s.pending.erase(s.pending.begin(), s.pending.begin() + (ptrdiff_t)s.pending_pos);
        s.pending_pos = 0;
    }
    const std::vector<uint8_t> &asc = w.audio.front().codec_private;
    while (!w.packets.empty()) {
        if (s.webm_error.empty()) {
            const std::vector<uint8_t> &raw = w.packets.front().data;
            if (raw.size() + 7 > 8191) {
                s.webm_error = "WebM AAC frame of " + std::to_string(raw.size()) + " bytes exceeds an ADTS frame";
            } else if (s.pending.size() - s.pending_pos + raw.size() + 7 > kMaxMp4QueuedBytes) {
                s.webm_error = "WebM AAC packet queue exceeds the " + std::to_string(kMaxMp4QueuedBytes) + " byte streaming budget";
            } else {
                uint8_t head[7];
                sk_mp4::adts_header(asc.data(), asc.size(), s.webm_rate, s.webm_channels, raw.size(), head);
                s.pending.insert(s.pending.end(), head, head + 7);
                s.pending.insert(s.pending.end(), raw.begin(), raw.end());
            }
        }
        w.pop_packet();
    }
    if (!s.webm_error.empty()) s.webm_done = true;
}

// An A_FLAC track's bytes as a native FLAC stream: the CodecPrivate (`fLaC` and the metadata blocks) once, then the frames
void webm_flac_bytes(PStream &s, std::vector<uint8_t> &out) {
    sk_webm::Demuxer &w = *s.webm;
    if (s.webm_flac_head) {
        s.webm_flac_head = false;
        out = w.audio.front().codec_private;
    }
    while (!w.packets.empty()) {
        out.insert(out.end(), w.packets.front().data.begin(), w.packets.front().data.end());
        w.pop_packet();
    }
}

// The same for a `fLaC` track of an MP4 stream: the normalised `dfLa` once, then the samples (one frame each)
void mp4_flac_bytes(PStream &s, std::vector<uint8_t> &out) {
    sk_mp4::Demuxer &m = *s.mp4;
    if (s.mp4_flac_head) {
        s.mp4_flac_head = false;
        out = m.track.codec_private;
    }
    while (!m.packets.empty()) {
        out.insert(out.end(), m.packets.front().data.begin(), m.packets.front().data.end());
        m.packets.pop_front();
    }
}

// The tables an MP3 stream needs: the code book for the host's Huffman stage, band tables and synthesis window on the engine;
// the batches get their granule arrays.  Once per lane, at the first MP3 stream.
int ensure_mp3(sk_lane *p);
}  // namespace
namespace sk_mp3_internal {
PipelineGpuHooks &pipeline_gpu_hooks() {
    static PipelineGpuHooks hooks;
    return hooks;
}
}  // namespace sk_mp3_internal
namespace {

// What the stream's first bytes are (detect_audio at lib.rs:3042 looks at magic numbers; on this path two formats exist):
// an ID3v2 tag or an MPEG audio sync with a layer field -> MP3; an ADTS sync (layer bits 00) -> AAC.  0 = not enough bytes yet.
// eof: the stream has ended, so the one rule that waits for bytes which may never decide anything (the transport stream's) does not.
uint8_t sniff_codec(const uint8_t *d, size_t n, bool eof) {
    // 1A 45 DF A3 -> WebM / Matroska (AudioType::Webm); fewer bytes that match so far: wait.  Before the MPEG sync scan, which would
    // find a sync somewhere inside the file
    static const uint8_t ebml[4] = {0x1A, 0x45, 0xDF, 0xA3};
    if (n > 0 && std::memcmp(d, ebml, std::min<size_t>(n, 4)) == 0) return n < 4 ? 0 : kCodecWebm;
    // ....ftyp -> MP4 / M4A (AudioType::M4A, looks_like_mp4: 12 bytes); fewer bytes that may still become that: wait
    if (n >= 8 && std::memcmp(d + 4, "ftyp", 4) == 0) return n < 12 ? 0 : kCodecMp4;
    if (n > 4 && n < 8 && std::memcmp(d + 4, "ftyp", n - 4) == 0) return 0;
    // RIFF....WAVE / RF64....WAVE -> WAV (AudioType::Wav, lib.rs:3090-3093); fewer than 12 bytes that may still become that: wait
    if (n >= 4 && (std::memcmp(d, "RIFF", 4) == 0 || std::memcmp(d, "RF64", 4) == 0)) {
        if (n < 12) return 0;
        if (std::memcmp(d + 8, "WAVE", 4) == 0) return kCodecWav;
        if (sk_avi::sniff(d, n)) return kCodecAvi;  // RIFF....AVI  (looks_like_avi)
    } else if (n > 0 && n < 4 && (std::memcmp(d, "RIFF", n) == 0 || std::memcmp(d, "RF64", n) == 0)) {
        return 0;
    }
    // FORM....AIFF / FORM....AIFC -> AIFF (AudioType::Aiff, lib.rs:3099-3102); the same wait
    if (n >= 4 && std::memcmp(d, "FORM", 4) == 0) {
        if (n < 12) return 0;
        if (std::memcmp(d + 8, "AIFF", 4) == 0 || std::memcmp(d + 8, "AIFC", 4) == 0) return kCodecAiff;
    } else if (n > 0 && n < 4 && std::memcmp(d, "FORM", n) == 0) {
        return 0;
    }
    // OggS, and the first page's first packet begins \x01vorbis -> Ogg Vorbis (AudioType::OggVorbis); a page header or a packet start
    // not complete yet: wait.  Any other Ogg stream goes the way it always went
    if (n >= 4 && std::memcmp(d, "OggS", 4) == 0) {
        if (n < 27 || n < 27 + (size_t)d[26] + 7) return 0;
        if (std::memcmp(d + 27 + d[26], "\x01vorbis", 7) == 0) return kCodecVorbis;
    } else if (n > 0 && n < 4 && std::memcmp(d, "OggS", n) == 0) {
        return 0;
    }
    // fLaC -> native FLAC (AudioType::Flac); fewer than 4 bytes that match so far: wait
    if (n >= 4 && std::memcmp(d, "fLaC", 4) == 0) return kCodecFlac;
    if (n > 0 && n < 4 && std::memcmp(d, "fLaC", n) == 0) return 0;
    // 00 00 01 BA -> an MPEG program stream (looks_like_mpeg_ps), before the rules that would find a sync inside it; fewer than 4 bytes
    // that match so far: wait
    static const uint8_t pack[4] = {0x00, 0x00, 0x01, 0xBA};
    if (n > 0 && std::memcmp(d, pack, std::min<size_t>(n, 4)) == 0) return n < 4 ? 0 : kCodecPs;
    // an MPEG transport stream (looks_like_mpeg_ts: three syncs at stride 188, or at 192 behind four bytes), before the MPEG sync scan,
    // which would stop at the first FF Fx inside some PES payload.  A 47 where the first sync would be: wait for the 389 bytes that
    // settle it, unless the stream has ended; a stream that is none goes on to the rules below as it always did
    if (sk_ts::sniff(d, n)) return kCodecTs;
    if (!eof && n < 389 && n > 0 && (d[0] == 0x47 || (n > 4 && d[4] == 0x47))) return 0;
    if (n >= 3 && d[0] == 'I' && d[1] == 'D' && d[2] == '3') return kCodecMp3;
    for (size_t i = 0; i + 1 < n; ++i)
        if (d[i] == 0xff && (d[i + 1] & 0xe0) == 0xe0) return ((d[i + 1] >> 1) & 3) == 0 ? kCodecAac : kCodecMp3;
    return n >= 8192 ? kCodecAac : 0;  // no sync in 8 KiB: let the ADTS path resynchronise (it ends the stream at EOF)
}

// An MP3 stream's pass (nanomp3 inside Mp3Decoder::decode_i16, soundkit-mp3/src/lib.rs:279-305, up to its Huffman stage): frame
// sync, header, side information, bit reservoir, scale factors and Huffman codes on this thread; what is left -- requantisation,
// stereo, reorder, hybrid synthesis -- are the granules handed to the tick.  A frame that cannot be decoded (the reservoir
// does not reach back far enough, damaged Huffman data, a feature not built) is consumed without output, as sk_mp3_decoder_*
// does.  At most `limit` granules per pass.
void parse_some_mp3(sk_lane *p, PStream &s, uint32_t limit, Parsed &r) {
    r.mp3 = true;
    int rc = ensure_mp3(p);
    if (rc != SK_OK) {
        r.fail(rc, std::string("Decoding failed: MP3 tables: ") + sk_strerror(rc));
        return;
    }
    std::vector<sk_mp3_frame_info> found(64);
    std::vector<uint8_t> main;
    constexpr size_t kReservoirKept = 2048;
    while (r.n_frames < limit && !r.failed) {
        const size_t avail = s.pending.size() - s.pending_pos;
        uint32_t n_found = 0;
        size_t scanned = 0;
        // the free-format length: s.mp3_free_format is the one in force at pending_pos (behind the last frame taken); the scan's own
        // end state replaces it only when everything scanned is consumed
        uint32_t free_format_scan = s.mp3_free_format;
        if (avail >= 4) {
            free_format_scan = s.mp3_free_format;
            rc = sk_mp3_scan_free(s.pending.data() + s.pending_pos, avail, found.data(), (uint32_t)found.size(), &n_found, &scanned, &free_format_scan);
            if (rc != SK_OK) {
                r.fail(rc, std::string("Decoding failed: ") + sk_strerror(rc));
                break;
            }
            if (n_found > found.size()) n_found = (uint32_t)found.size();
        }
        if (n_found == 0) {
            s.pending_pos += scanned;  // garbage in front of an incomplete frame goes
            s.mp3_free_format = free_format_scan;
            if (s.saw_eof) {
                r.eof = true;
                break;
            }
            const int got = pull_input(s);
            if (got == 0) break;  // needs more input
            continue;
        }
        size_t consumed = 0;
        for (uint32_t k = 0; k < n_found && !r.failed; ++k) {
            const sk_mp3_frame_info &h = found[k];
            if (r.n_frames + h.granules > limit) {
                r.budget_stop = true;
                break;
            }
            const uint8_t *frame = s.pending.data() + s.pending_pos + h.offset;
            const size_t head = 4u + (h.has_crc ? 2u : 0u) + h.side_info_bytes;
            sk_mp3_side_info side;
            bool ok = sk_mp3_parse_side_info(frame, h.frame_bytes, &h, &side) == SK_OK;
            size_t main_len = 0;
            main.resize(s.mp3_reservoir.size() + h.frame_bytes);
            if (ok) ok = sk_mp3_main_data(frame, h.frame_bytes, &h, &side, s.mp3_reservoir.data(), s.mp3_reservoir.size(), main.data(), main.size(), &main_len) == SK_OK;
            sk_mp3_granule_data data[2][2];
            if (ok && !p->mp3_gpu) ok = sk_mp3_decode_main_data(p->mp3_cb, &h, &side, main.data(), main_len, data) == SK_OK;
            if (ok && p->mp3_gpu && r.n_frames > 0 && r.mp3_bytes.size() + main_len + 12 > p->au_pass_budget) {  // what one batch can take
                r.budget_stop = true;
                break;
            }
            const bool joint = h.mode == 1;
            if (ok) {
                if (s.engine_stream == kNoStream) {  // the first frame that decodes fixes rate and channels (lib.rs:203-204)
                    s.rate = h.sample_rate;
                    s.channels = h.channels;
                    rc = sk_stream_open(p->engine, s.rate, s.channels, &s.engine_stream);
                    if (rc != SK_OK) {
                        r.fail(rc, std::string("Decoding failed: engine stream: ") + sk_strerror(rc));
                        break;
                    }
                    const uint32_t target = s.opt.output_sample_rate ? s.opt.output_sample_rate : s.rate;
                    s.resample = target != s.rate;
                    if (s.resample) {
                        rc = sk_resampler_open(p->engine, s.engine_stream, s.rate, target);
                        if (rc != SK_OK) {
                            s.resample = false;  // no resampler: the failed pass's row in the tick must not ask for one (the tick would refuse every stream in it)
                            r.fail(rc, "Decoding failed: Failed to create resampler: unsupported rate pair");
                            break;
                        }
                    }
                } else if (h.channels != s.channels || h.sample_rate != s.rate) {
                    r.fail(SK_MP3_UNSUPPORTED, "Decoding failed: MP3 sample rate or channel count changed mid-stream");
                    break;
                }
                if (p->mp3_gpu) {  // the pass ends behind the reservoir: the frame and its main data go to the tick as they are
                    sk_mp3_frame_item item;
                    std::memset(&item, 0, sizeof item);
                    item.header = h;
                    item.side = side;
                    item.byte_offset = (uint32_t)r.mp3_bytes.size();
                    item.byte_len = (uint32_t)main_len;
                    r.mp3_bytes.insert(r.mp3_bytes.end(), main.data(), main.data() + main_len);
                    r.mp3_bytes.resize((r.mp3_bytes.size() + 8 + 3) & ~(size_t)3, 0);  // 4-byte aligned, >= 8 zero bytes behind it
                    r.mp3_frames.push_back(item);
                    r.n_frames += h.granules;
                    r.n_au_bytes = r.mp3_bytes.size();
                }
                for (int gr = 0; gr < h.granules && !p->mp3_gpu; ++gr) {
                    sk_mp3_requant_granule g;
                    std::memset(&g, 0, sizeof g);
                    g.sample_rate = h.sample_rate;
                    g.channels = h.channels;
                    g.ms_stereo = joint && (h.mode_ext & 2);
                    g.intensity_stereo = joint && (h.mode_ext & 1);
                    g.lsf = h.version != 1;
                    if (g.lsf && g.intensity_stereo && h.channels == 2 && data[gr][1].intensity_scale) g.intensity_stereo |= 2;
                    sk_mp3_granule_desc d;
                    std::memset(&d, 0, sizeof d);
                    d.stream = s.engine_stream;
                    d.channels = h.channels;
                    for (int ch = 0; ch < h.channels; ++ch) {
                        const sk_mp3_granule_side &gs = side.gr[gr][ch];
                        const sk_mp3_granule_data &src = data[gr][ch];
                        sk_mp3_requant_channel &c = g.ch[ch];
                        c.global_gain = gs.global_gain, c.scalefac_scale = gs.scalefac_scale, c.preflag = src.preflag;
                        c.block_type = gs.block_type, c.mixed_block_flag = gs.mixed_block_flag;
                        std::memcpy(c.subblock_gain, gs.subblock_gain, 3);
                        std::memcpy(c.scalefac_l, src.scalefac_l, 22);
                        std::memcpy(c.scalefac_s, src.scalefac_s, 39);
                        d.block_type[ch] = gs.block_type, d.mixed_block_flag[ch] = gs.mixed_block_flag;
                        r.mp3_is.insert(r.mp3_is.end(), src.is, src.is + 576);
                    }
                    r.mp3_gr.push_back(g);
                    r.mp3_desc.push_back(d);
                    r.n_frames += 1;
                }
            }
            // whatever became of the frame, its own main data is what later frames reach back into
            if (h.frame_bytes > head) s.mp3_reservoir.insert(s.mp3_reservoir.end(), frame + head, frame + h.frame_bytes);
            if (s.mp3_reservoir.size() > 4 * kReservoirKept) s.mp3_reservoir.erase(s.mp3_reservoir.begin(), s.mp3_reservoir.end() - (ptrdiff_t)kReservoirKept);
            consumed = h.offset + h.frame_bytes;
            if ((frame[2] >> 4) == 0) s.mp3_free_format = h.frame_bytes - h.padding;
            if (k + 1 == n_found && n_found < found.size()) consumed = scanned, s.mp3_free_format = free_format_scan;
        }
        s.pending_pos += consumed;
        if (r.budget_stop) break;
    }
}

// A Layer I / II stream's pass (nanomp3 inside Mp3Decoder::decode_i16 on such a frame, up to the samples): frame sync and header, then
// the frame's serial front -- allocation, scale-factor selection, scale factors -- read into a record on this thread, where it is
// cheap; the samples stay in the frame's bytes and are the tick's (k_mp12_synth).  A frame the parse rejects (Layer I's allocation 15,
// samples that would end beyond the frame) is consumed without output.  At most `limit` FRAMES per pass: a frame is never split
// between passes or ticks.
void parse_some_mpa(sk_lane *p, PStream &s, uint32_t limit, Parsed &r) {
    r.mpa = true;
    const sk_mp3_internal::PipelineGpuHooks &hooks = sk_mp3_internal::pipeline_gpu_hooks();
    if (!hooks.mpa_scan || !hooks.mpa_parse_frame || !hooks.tick_mpa) {
        r.fail(SK_ERR_UNSUPPORTED, "Decoding failed: MPEG Layer I / II needs the device tick, which this build lacks");
        return;
    }
    int rc = ensure_mp3(p);  // the synthesis window is the engine's Layer III one
    if (rc != SK_OK) {
        r.fail(rc, std::string("Decoding failed: MP3 tables: ") + sk_strerror(rc));
        return;
    }
    std::vector<sk_mpa_frame_info> found(64);
    while (r.n_frames < limit && !r.failed) {
        const size_t avail = s.pending.size() - s.pending_pos;
        uint32_t n_found = 0, layer = s.mpa_layer;
        size_t scanned = 0;
        if (avail >= 4) {
            rc = hooks.mpa_scan(s.pending.data() + s.pending_pos, avail, &layer, found.data(), (uint32_t)found.size(), &n_found, &scanned);
            if (rc != SK_OK) {
                r.fail(rc, std::string("Decoding failed: ") + sk_strerror(rc));
                break;
            }
            if (n_found > found.size()) n_found = (uint32_t)found.size();
        }
        if (n_found == 0) {
            s.pending_pos += scanned;  // garbage in front of an incomplete frame goes
            if (s.saw_eof) {
                r.eof = true;
                break;
            }
            if (pull_input(s) == 0) break;  // needs more input
            continue;
        }
        size_t consumed = 0;
        for (uint32_t k = 0; k < n_found && !r.failed; ++k) {
            const sk_mpa_frame_info &h = found[k];
            if (r.n_frames + 1 > limit) {
                r.budget_stop = true;
                break;
            }
            const uint8_t *frame = s.pending.data() + s.pending_pos + h.offset;
            sk_mpa_frame_record rec;
            if (hooks.mpa_parse_frame(frame, h.frame_bytes, &h, &rec) == SK_OK) {
                if (s.engine_stream == kNoStream) {  // the first frame that decodes fixes rate and channels (lib.rs:203-204)
                    s.rate = h.sample_rate;
                    s.channels = h.channels;
                    rc = sk_stream_open(p->engine, s.rate, s.channels, &s.engine_stream);
                    if (rc != SK_OK) {
                        r.fail(rc, std::string("Decoding failed: engine stream: ") + sk_strerror(rc));
                        break;
                    }
                    const uint32_t target = s.opt.output_sample_rate ? s.opt.output_sample_rate : s.rate;
                    s.resample = target != s.rate;
                    if (s.resample) {
                        rc = sk_resampler_open(p->engine, s.engine_stream, s.rate, target);
                        if (rc != SK_OK) {
                            s.resample = false;  // no resampler: the failed pass's row in the tick must not ask for one (the tick would refuse every stream in it)
                            r.fail(rc, "Decoding failed: Failed to create resampler: unsupported rate pair");
                            break;
                        }
                    }
                } else if (h.channels != s.channels || h.sample_rate != s.rate) {
                    r.fail(SK_MP3_UNSUPPORTED, "Decoding failed: MP3 sample rate or channel count changed mid-stream");
                    break;
                }
                rec.byte_offset = (uint32_t)r.mpa_bytes.size();
                r.mpa_bytes.insert(r.mpa_bytes.end(), frame, frame + h.frame_bytes);
                r.mpa_bytes.resize((r.mpa_bytes.size() + 8 + 3) & ~(size_t)3, 0);  // 4-byte aligned, >= 8 zero bytes behind it
                r.mpa_recs.push_back(rec);
                r.n_frames += 1;
            }
            consumed = h.offset + h.frame_bytes;
            if (k + 1 == n_found && n_found < found.size()) consumed = scanned;
        }
        s.pending_pos += consumed;
        if (r.budget_stop) break;
    }
    if (r.n_frames >= limit) r.budget_stop = true;  // the pass met its frame limit: there may be more (worker_body: s.more)
}


// The batches' pinned buffers for PCM pieces.  Once per lane, at the first stream that needs the PCM tick.
int ensure_pcm(sk_lane *p) {
    if (p->pcm_ready.load(std::memory_order_acquire)) return SK_OK;
    std::lock_guard<std::mutex> lk(p->pcm_mu);
    if (p->pcm_ready.load(std::memory_order_relaxed)) return SK_OK;
    std::lock_guard<std::mutex> bl(p->batch_mu);  // no claim can name these buffers yet: a PCM pass stages units only behind this function
    for (Batch &b : p->batches) {
        if (b.pcm_bytes) continue;
        if (hipHostMalloc((void **)&b.pcm_bytes, kPcmTickBytes + 64, hipHostMallocPortable) != hipSuccess) {
            b.pcm_bytes = nullptr;
            return SK_ERR_OOM;
        }
        b.pcm_cap = kPcmTickBytes;
    }
    p->pcm_ready.store(true, std::memory_order_release);
    return SK_OK;
}

// The first piece of a WAV / raw PCM stream fixes what apply_output_options (lib.rs:3324-3456) does with all of them: nothing
// (the fast path), or a conversion -- the PCM tick's, which needs the stream's format among SK_FMT_*, one or two channels (up to
// eight on an engine with the pool of wide streams) and,
// for a rate change, an engine stream with a resampler.  false: the stream has failed (r says how).
bool pcm_open(sk_lane *p, PStream &s, Parsed &r) {
    uint32_t rate, channels, bits;
    bool is_float, big_endian = false;
    if (s.gsm) {  // GsmDecoder's: 8 kHz mono, create_audio_data_i16
        rate = 8000, channels = 1, bits = 16, is_float = false;
    } else if (s.g72x) {  // the spawn's: create_audio_data_i16(d.sample_rate(), d.channels(), ...), always 16 bits
        rate = s.g72x_rate, channels = s.g72x_channels, bits = 16, is_float = false;
    } else if (s.vorbis) {  // the identification header's; VorbisDecoder hands out s16
        rate = s.vorbis_ident.sample_rate, channels = s.vorbis_ident.channels, bits = 16, is_float = false;
    } else if (s.alac) {  // the cookie's
        rate = s.alac_cfg.sample_rate, channels = s.alac_cfg.channels, bits = s.alac_cfg.bit_depth, is_float = false;
    } else if (s.flac) {  // STREAMINFO's: the AudioData of a FLAC frame carries the stream's own depth (create_audio_data_i32_with_bits, lib.rs:3191-3236)
        rate = s.flac->info().sample_rate, channels = s.flac->info().channels, bits = s.flac->info().bits_per_sample, is_float = false;
    } else if (s.aiff) {  // what the decoder emits (the output contract), not what the file holds: apply_output_options sees only that
        rate = s.aiff->sample_rate(), channels = s.aiff->channels(), bits = s.aiff->bits(), is_float = s.aiff->is_float();
        s.aiff_enc = (uint8_t)s.aiff->encoding();
    } else if (s.wav) {
        rate = s.wav->sample_rate(), channels = s.wav->channels(), bits = s.wav->bits(), is_float = s.wav->is_float();
        const uint32_t tag = s.wav->tag();
        s.wav_g711 = tag == SK_WAV_TAG_ALAW || tag == SK_WAV_TAG_ULAW;
        s.wav_adpcm = s.wav->is_adpcm();
        if (s.wav_g711 || s.wav_adpcm) bits = 16;  // what the decode emits, as for AIFF-C
        if (s.wav_g711) s.aiff_enc = tag == SK_WAV_TAG_ALAW ? SK_AIFF_ALAW : SK_AIFF_ULAW;
        if (s.wav_adpcm) s.wav_parse_left = s.wav_tick_left = s.wav->total_frames();
    } else if (s.raw_enc) {  // a container's source-encoded PCM: what the AIFF tick makes of it
        rate = s.raw_format.sample_rate, channels = s.raw_format.channels;
        bits = sk_pcm::aiff_contract_bits(s.aiff_enc), is_float = false;
    } else {
        const int f = s.raw_format.format;
        rate = s.raw_format.sample_rate, channels = s.raw_format.channels;
        bits = f <= SK_FMT_S16BE ? 16 : (f <= SK_FMT_S24BE ? 24 : 32);
        is_float = f >= SK_FMT_F32LE;
        big_endian = (f & 1) != 0;
    }
    if (channels > 255 || bits > 255) return r.fail(SK_ERR_UNSUPPORTED, "Decoding failed: WAV channel count or sample width above 255");
    s.rate = rate;
    s.channels = (uint8_t)channels;
    s.pcm_bits = (uint8_t)bits;
    s.pcm_flags = (uint8_t)((is_float ? SK_AUDIO_FLOAT : 0) | (big_endian ? SK_AUDIO_BIG_ENDIAN : 0));
    const uint32_t target_rate = s.opt.output_sample_rate ? s.opt.output_sample_rate : rate;
    const uint32_t target_bits = s.opt.output_bits_per_sample ? s.opt.output_bits_per_sample : bits;
    const uint32_t target_channels = s.opt.output_channels ? s.opt.output_channels : channels;
    const sk_mp3_internal::PipelineGpuHooks &hooks = sk_mp3_internal::pipeline_gpu_hooks();
    if (s.flac && (!hooks.tick_flac || !hooks.tick_flac_out_bound))
        return r.fail(SK_ERR_UNSUPPORTED, "Decoding failed: FLAC decoding needs the device tick, which this build lacks");
    if (s.flac && target_rate == rate && target_bits == bits && target_channels == channels) {  // every frame has per-sample work: the tick's
        const int rc = ensure_pcm(p);
        if (rc != SK_OK) return r.fail(rc, std::string("Decoding failed: PCM staging buffers: ") + sk_strerror(rc));
        s.pcm_route = kPcmFlacTick;
        s.flac_plain = true;
        return true;
    }
    if (s.g72x && (!hooks.tick_g72x || !hooks.tick_g72x_out_bound))
        return r.fail(SK_ERR_UNSUPPORTED, "Decoding failed: telephony decoding needs the device tick, which this build lacks");
    if (s.g72x && target_rate == rate && target_bits == bits && target_channels == channels) {  // every byte has per-sample work: the tick's
        const int rc = ensure_pcm(p);
        if (rc != SK_OK) return r.fail(rc, std::string("Decoding failed: PCM staging buffers: ") + sk_strerror(rc));
        s.pcm_route = kPcmG72xTick;
        return true;
    }
    if (s.gsm && (!hooks.tick_gsm || !hooks.tick_gsm_out_bound))
        return r.fail(SK_ERR_UNSUPPORTED, "Decoding failed: GSM decoding needs the device tick, which this build lacks");
    if (s.gsm && target_rate == rate && target_bits == bits && target_channels == channels) {  // every frame has per-sample work: the tick's
        const int rc = ensure_pcm(p);
        if (rc != SK_OK) return r.fail(rc, std::string("Decoding failed: PCM staging buffers: ") + sk_strerror(rc));
        s.pcm_route = kPcmGsmTick;
        return true;
    }
    if (s.vorbis && (!hooks.tick_vorbis || !hooks.tick_vorbis_out_bound))
        return r.fail(SK_ERR_UNSUPPORTED, "Decoding failed: Vorbis decoding needs the device tick, which this build lacks");
    if (s.vorbis && target_rate == rate && target_bits == bits && target_channels == channels) {  // every packet has per-sample work: the tick's
        const int rc = ensure_pcm(p);
        if (rc != SK_OK) return r.fail(rc, std::string("Decoding failed: PCM staging buffers: ") + sk_strerror(rc));
        s.pcm_route = kPcmVorbisTick;
        return true;
    }
    if (s.wav_adpcm && (!hooks.tick_wav_adpcm || !hooks.tick_wav_adpcm_out_bound))
        return r.fail(SK_ERR_UNSUPPORTED, "Decoding failed: WAV ADPCM decoding needs the device tick, which this build lacks");
    if (s.wav_adpcm && target_rate == rate && target_bits == bits && target_channels == channels) {  // every block has per-sample work: the tick's
        const int rc = ensure_pcm(p);
        if (rc != SK_OK) return r.fail(rc, std::string("Decoding failed: PCM staging buffers: ") + sk_strerror(rc));
        s.pcm_route = kPcmWavAdpcmTick;
        return true;
    }
    if (s.alac && (!hooks.tick_alac || !hooks.tick_alac_out_bound))
        return r.fail(SK_ERR_UNSUPPORTED, "Decoding failed: ALAC decoding needs the device tick, which this build lacks");
    if (s.alac && target_rate == rate && target_bits == bits && target_channels == channels) {  // every packet has per-sample work: the tick's
        const int rc = ensure_pcm(p);
        if (rc != SK_OK) return r.fail(rc, std::string("Decoding failed: PCM staging buffers: ") + sk_strerror(rc));
        s.pcm_route = kPcmAlacTick;
        s.alac_plain = true;
        return true;
    }
    if (target_rate == rate && target_bits == bits && target_channels == channels) {
        // sowt / 23ni are the contract's bytes already; every other encoding has per-sample work, which is the tick's
        if ((!s.aiff && !s.wav_g711 && !s.raw_enc) || (s.aiff && (s.aiff_enc == SK_AIFF_S16LE || s.aiff_enc == SK_AIFF_S32LE))) {
            s.pcm_route = kPcmFast;
            return true;
        }
        if (!hooks.tick_aiff || !hooks.tick_aiff_out_bound) return r.fail(SK_ERR_UNSUPPORTED, "Decoding failed: AIFF decoding needs the device tick, which this build lacks");
        const int rc = ensure_pcm(p);
        if (rc != SK_OK) return r.fail(rc, std::string("Decoding failed: PCM staging buffers: ") + sk_strerror(rc));
        s.pcm_route = kPcmAiffTick;
        s.aiff_plain = true;
        return true;
    }
    // audio_data_to_f32_channels (lib.rs:3563-3617) and exact_signed_pcm_to_i16 take 16 / 24 / 32-bit samples
    if (is_float && bits != 32) return r.fail(SK_PCM_ERR_STREAM, "Decoding failed: Output conversion failed: floating-point PCM must contain 32-bit samples");
    if (bits != 16 && bits != 24 && bits != 32)
        return r.fail(SK_PCM_ERR_STREAM, "Decoding failed: Output conversion failed: PCM data is unsupported or contains a partial frame");
    // 3 ... 8 channels: the tick takes them on an engine whose pool of wide streams was reserved (sk_engine_enable_wide_pcm)
    if (channels > SK_MAX_CHANNELS && (channels > SK_MAX_PCM_CHANNELS || !hooks.wide_pcm_streams || hooks.wide_pcm_streams(p->engine) == 0))
        return r.fail(SK_ERR_UNSUPPORTED, "Decoding failed: conversion of PCM with more than 2 channels is not supported");
    if (!hooks.tick_pcm || !hooks.tick_pcm_out_bound || ((s.aiff || s.wav_g711 || s.raw_enc) && (!hooks.tick_aiff || !hooks.tick_aiff_out_bound)))
        return r.fail(SK_ERR_UNSUPPORTED, "Decoding failed: PCM conversion needs the device tick, which this build lacks");
    s.pcm_fmt = (uint8_t)((bits == 16 ? SK_FMT_S16LE : (bits == 24 ? SK_FMT_S24LE : (is_float ? SK_FMT_F32LE : SK_FMT_S32LE))) + (big_endian ? 1 : 0));
    int rc = ensure_pcm(p);
    if (rc != SK_OK) return r.fail(rc, std::string("Decoding failed: PCM staging buffers: ") + sk_strerror(rc));
    s.resample = target_rate != rate;
    if (s.resample) {
        rc = sk_stream_open(p->engine, rate, s.channels, &s.engine_stream);
        if (rc != SK_OK) return r.fail(rc, std::string("Decoding failed: engine stream: ") + sk_strerror(rc));
        rc = sk_resampler_open(p->engine, s.engine_stream, rate, target_rate);
        if (rc != SK_OK) return r.fail(rc, "Decoding failed: Failed to create resampler: unsupported rate pair");
    }
    s.pcm_route = s.vorbis ? kPcmVorbisTick : s.gsm ? kPcmGsmTick : s.g72x ? kPcmG72xTick : s.alac ? kPcmAlacTick : (s.flac ? kPcmFlacTick : (s.aiff || s.wav_g711 || s.raw_enc ? kPcmAiffTick : (s.wav_adpcm ? kPcmWavAdpcmTick : kPcmTick)));
    return true;
}

// One unit of a PCM-family pass is staged: its bytes at the next 16-byte aligned offset of r.pcm_bytes (returned), its entry in
// r.pcm_units, and the AudioData it will give counted into `outputs` -- one, or through the resampler one per completed 4096-frame chunk
size_t stage_unit(Parsed &r, PStream &s, const uint8_t *data, size_t len, uint32_t frames, uint32_t &outputs) {
    const size_t at = (r.pcm_bytes.size() + 15) & ~(size_t)15;
    r.pcm_bytes.resize(at);
    r.pcm_bytes.insert(r.pcm_bytes.end(), data, data + len);
    r.pcm_units.push_back(sk_pcm_unit{at, (uint32_t)len, 0});
    if (s.resample) {
        outputs += (s.pcm_fill + frames) / 4096;
        s.pcm_fill = (s.pcm_fill + frames) % 4096;
    } else {
        outputs += 1;
    }
    return at;
}

// A telephony stream's pass (sk_pipeline_spawn_g711 / _g722 / _g726): decode_i16_with_drain's shape (lib.rs:2150-2181, 2310-2345) --
// every non-empty send is one decode and gives one AudioData, or nothing where a G.726 send completes no group.  What a send decodes
// now is one unit of the telephony tick.  A send above the reference's scratch ends the stream with the decoder's text; the end of
// the stream is G726Decoder::flush (a partial group left: its text) or, for G.711 and G.722, an empty decode that gives nothing.
void parse_some_g72x(sk_lane *p, PStream &s, uint32_t room, Parsed &r) {
    r.pcm = true;
    const uint32_t per_pass = std::min<uint32_t>(std::max<uint32_t>(p->cfg.max_stream_frames_per_tick, 1), 65536);
    const int bits = s.g72x_codec == SK_G726 ? sk_g72x::g726_bits(s.g726_rate) : 0;
    uint32_t outputs = 0;
    if (!s.pcm_route && !pcm_open(p, s, r)) return;
    const bool plain = !s.resample && (s.opt.output_bits_per_sample ? s.opt.output_bits_per_sample : 16u) == 16u &&
                       (s.opt.output_channels ? s.opt.output_channels : s.channels) == s.channels;
    std::vector<uint8_t> whole;
    while (!r.failed) {
        if (s.saw_eof) {
            std::string text;
            if (s.g72x_codec == SK_G726 && !s.g726_framer.flush(&text)) r.fail(SK_G72X_ERR_STREAM, "Decoding failed: " + text);
            else r.eof = true;
            break;
        }
        std::vector<uint8_t> chunk;
        {
            std::lock_guard<std::mutex> lk(s.mu);
            if (s.in.empty()) break;
            const size_t next = s.in.front().size();
            if (next && (outputs >= room || r.pcm_units.size() >= per_pass || (!r.pcm_units.empty() && r.pcm_bytes.size() + next + 4096 > kPcmTickBytes))) {
                r.more = true;
                break;
            }
            chunk = std::move(s.in.front());
            s.in.pop_front();
        }
        if (chunk.empty()) {
            s.saw_eof = true;
            continue;
        }
        s.queued_bytes.fetch_sub(chunk.size());
        const uint8_t *data = chunk.data();
        size_t len = chunk.size();
        std::string text;
        if (s.g72x_codec == SK_G726) {
            // the scratch is checked before anything is taken: the reference's decoder returns its error with the pending bytes as they were
            if (!sk_g72x::fits_scratch(SK_G726, sk_g72x::samples_of(SK_G726, bits, s.g726_framer.ready(len)), &text)) {
                r.fail(SK_G72X_ERR_STREAM, "Decoding failed: " + text);
                break;
            }
            whole.clear();
            len = s.g726_framer.add(data, len, whole);
            data = whole.data();
            if (len == 0) continue;  // no group completed: nothing is delivered for this send
        } else if (!sk_g72x::fits_scratch(s.g72x_codec, sk_g72x::samples_of(s.g72x_codec, 0, len), &text)) {
            r.fail(SK_G72X_ERR_STREAM, "Decoding failed: " + text);
            break;
        }
        const uint64_t samples = sk_g72x::samples_of(s.g72x_codec, bits, len);
        // G.711 of several channels: as decoded the samples leave as they came (create_audio_data_i16 checks nothing); a conversion
        // refuses a send that splits a frame, with audio_data_to_f32_channels' text (lib.rs:3569-3574)
        if (!plain && samples % s.channels != 0) {
            r.fail(SK_PCM_ERR_STREAM, "Decoding failed: Output conversion failed: PCM data is unsupported or contains a partial frame");
            break;
        }
        stage_unit(r, s, data, len, (uint32_t)(samples / s.channels), outputs);
    }
    r.pcm_bytes.resize((r.pcm_bytes.size() + 15) & ~(size_t)15);
}

// A GSM stream's pass (sk_pipeline_spawn_gsm): the same decode_i16_with_drain shape (lib.rs:2358-2422) -- a send that completes at least
// one packet is one decode and gives one AudioData, a send that completes none gives nothing.  What a send decodes now is one unit of
// the GSM tick.  GsmDecoder::decode_i16 checks its room first (a send above the reference's scratch ends the stream with its text,
// the pending bytes as they were), then gsm_decode every frame (a standard frame without the magic nibble ends the stream); the end of
// the stream is GsmDecoder::flush (a partial packet left: its text).
void parse_some_gsm(sk_lane *p, PStream &s, uint32_t room, Parsed &r) {
    r.pcm = true;
    const uint32_t per_pass = std::min<uint32_t>(std::max<uint32_t>(p->cfg.max_stream_frames_per_tick, 1), 65536);
    uint32_t outputs = 0;
    if (!s.pcm_route && !pcm_open(p, s, r)) return;
    std::vector<uint8_t> whole;
    while (!r.failed) {
        if (s.saw_eof) {
            std::string text;
            if (!s.gsm_framer.flush(&text)) r.fail(SK_G72X_ERR_STREAM, "Decoding failed: " + text);
            else r.eof = true;
            break;
        }
        std::vector<uint8_t> chunk;
        {
            std::lock_guard<std::mutex> lk(s.mu);
            if (s.in.empty()) break;
            const size_t next = s.in.front().size();
            if (next && (outputs >= room || r.pcm_units.size() >= per_pass || (!r.pcm_units.empty() && r.pcm_bytes.size() + next + 4096 > kPcmTickBytes))) {
                r.more = true;
                break;
            }
            chunk = std::move(s.in.front());
            s.in.pop_front();
        }
        if (chunk.empty()) {
            s.saw_eof = true;
            continue;
        }
        s.queued_bytes.fetch_sub(chunk.size());
        std::string text;
        if (!sk_gsm::fits_scratch(sk_gsm::samples_of(s.gsm_variant, s.gsm_framer.ready(chunk.size())), &text)) {
            r.fail(SK_G72X_ERR_STREAM, "Decoding failed: " + text);
            break;
        }
        whole.clear();
        const size_t len = s.gsm_framer.add(chunk.data(), chunk.size(), whole);
        if (len == 0) continue;  // no packet completed: nothing is delivered for this send
        if (!sk_gsm::frames_accepted(s.gsm_variant, whole.data(), len, &text)) {
            r.fail(SK_G72X_ERR_STREAM, "Decoding failed: " + text);
            break;
        }
        stage_unit(r, s, whole.data(), len, (uint32_t)sk_gsm::samples_of(s.gsm_variant, len), outputs);
    }
    r.pcm_bytes.resize((r.pcm_bytes.size() + 15) & ~(size_t)15);
}

// An ALAC stream's pass: every chunk is one packet (sk_pipeline_spawn_alac_packets), and whole packets are what the stream is budgeted in
// -- `room` AudioData (one per packet, or one per completed 4096-frame chunk through the resampler), the units of one stream in a tick and
// the bytes one tick takes.  The host reads the packet's frame count (alac_stream.h) so that its place in the tick is known; a packet it
// cannot read one from, an empty one behind which more follows or one above 16 MiB ends the stream with its text.
void parse_some_alac(sk_lane *p, PStream &s, uint32_t room, Parsed &r) {
    r.pcm = true;
    const uint32_t per_pass = std::min<uint32_t>(std::max<uint32_t>(p->cfg.max_stream_frames_per_tick, 1), 65536);
    uint32_t outputs = 0;
    if (!s.pcm_route && !pcm_open(p, s, r)) return;
    while (!r.failed) {
        if (s.saw_eof) {
            r.eof = true;
            break;
        }
        std::vector<uint8_t> chunk;
        {
            std::lock_guard<std::mutex> lk(s.mu);
            if (s.in.empty()) break;
            const size_t next = s.in.front().size();
            if (next && (outputs >= room || r.pcm_units.size() >= per_pass || (!r.pcm_units.empty() && r.pcm_bytes.size() + next + 4096 > kPcmTickBytes))) {
                r.more = true;
                break;
            }
            chunk = std::move(s.in.front());
            s.in.pop_front();
        }
        if (chunk.empty()) {
            s.saw_eof = true;
            continue;
        }
        s.queued_bytes.fetch_sub(chunk.size());
        if (chunk.size() > sk_alac::kMaxPacketBytes) {
            r.fail(SK_ALAC_ERR_STREAM, "Decoding failed: ALAC packet exceeds the " + std::to_string(sk_alac::kMaxPacketBytes) + " byte budget");
            break;
        }
        uint32_t frames = 0;
        const int rc = sk_alac::packet_frames(s.alac_cfg, chunk.data(), chunk.size(), &frames);
        if (rc != SK_OK) {
            r.fail(rc, rc == SK_ALAC_UNSUPPORTED ? "Decoding failed: ALAC packet rejected: a CCE or PCE element is not supported"
                                                 : "Decoding failed: ALAC packet rejected: the elements break the syntax or miss the packet's end");
            break;
        }
        const size_t at = stage_unit(r, s, chunk.data(), chunk.size(), frames, outputs);
        r.alac_packets.push_back(sk_alac_tick_packet{(uint32_t)at, (uint32_t)chunk.size(), frames, 0});
    }
    r.pcm_bytes.resize((r.pcm_bytes.size() + 15) & ~(size_t)15);
}

// A Vorbis stream's pass.  From Ogg (the sniffing spawn): the chunks go through the page and packet parser, the first three packets are
// the headers (VorbisDecoder::process_packet: the first must open the logical stream, every later one carry its serial), and the
// stream joins the PCM family once the setup header is in.  From packets (sk_pipeline_spawn_vorbis_packets): the headers came with the
// spawn and every chunk is one audio packet.  Either way whole audio packets are what the stream is budgeted in.  The host reads a
// packet's first bits (vorbis_stream.h), so the frames it will yield are known here -- none for the stream's first packet -- and with
// them the Ogg decoder's cut of the last packet to the final granule position.  A packet whose first bits are refused ends the stream
// with its text, as read_audio_packet_generic's error does.  From WebM (webm_open has read the headers out of the CodecPrivate): the
// chunks go through the demuxer and every frame it hands out is one audio packet; a frame's DiscardPadding becomes the tick's
// skip_frames / keep_frames through the reference's conversion, at the identification header's rate.
bool vorbis_header(PStream &s, Parsed &r, const uint8_t *d, size_t n) {
        std::string text;
        int rc;
        if (s.vorbis_headers == 0) {
            rc = sk_vorbis::parse_ident(d, n, &s.vorbis_ident, &text);
        } else if (s.vorbis_headers == 1) {
            rc = sk_vorbis::parse_comment(d, n, &text);
        } else {
            std::shared_ptr<sk_vorbis_setup> su = std::make_shared<sk_vorbis_setup>();
            rc = sk_vorbis::parse_setup(d, n, s.vorbis_ident, &su->setup, &text);
            if (rc == SK_OK) {
                s.vorbis_setup = su;
                s.vorbis_overlap.assign((size_t)s.vorbis_ident.channels * (s.vorbis_ident.blocksize_1 / 2), 0.0f);
            }
        }
        if (rc != SK_OK) return r.fail(rc, "Decoding failed: " + text);
        ++s.vorbis_headers;
        return true;
}

void parse_some_vorbis(sk_lane *p, PStream &s, uint32_t room, Parsed &r) {
    r.pcm = true;
    const uint32_t per_pass = std::min<uint32_t>(std::max<uint32_t>(p->cfg.max_stream_frames_per_tick, 1), 65536);
    uint32_t outputs = 0;
    auto header = [&](const uint8_t *d, size_t n) -> bool { return vorbis_header(s, r, d, n); };
    auto audio = [&](const uint8_t *d, size_t n, const sk_ogg::Packet *op, const sk_webm::Packet *wp = nullptr) -> bool {
        if (!s.pcm_route && !pcm_open(p, s, r)) return false;
        if (n > sk_vorbis::kMaxPacketBytes) return r.fail(SK_VORBIS_ERR_STREAM, "Decoding failed: Vorbis packet exceeds the " + std::to_string(sk_vorbis::kMaxPacketBytes) + " byte budget");
        sk_vorbis::PacketHead h;
        const int rc = sk_vorbis::packet_head(s.vorbis_setup->setup, d, n, &h);
        if (rc != SK_OK) return r.fail(rc, std::string("Decoding failed: Vorbis packet rejected: ") + sk_strerror(rc));
        uint32_t frames = s.vorbis_parse_prev ? s.vorbis_parse_prev / 4 + h.n / 4 : 0, keep = 0xffffffffu, skip = 0;
        s.vorbis_parse_prev = h.n;
        if (wp && wp->has_discard) {  // decode_vorbis: [front, max(frames - back, front)) of the packet's frames stays
            uint32_t front, back;
            std::string text;
            if (!sk_webm::discard_frames(wp->discard_ns, s.vorbis_ident.sample_rate, frames, &front, &back, &text)) return r.fail(SK_WEBM_ERR_STREAM, "Decoding failed: " + text);
            skip = front, frames -= front + back, keep = frames;
        }
        if (op) {  // process_packet's bookkeeping: cur_absgp is known from the first audio packet that ends a page
            if (s.vorbis_have_absgp && op->last_in_stream && op->has_granule) {
                const uint64_t left = op->granule_position > s.vorbis_absgp ? op->granule_position - s.vorbis_absgp : 0;
                if (left < frames) frames = (uint32_t)left, keep = frames;
            }
            if (op->last_in_page) {
                if (op->has_granule) s.vorbis_have_absgp = true, s.vorbis_absgp = op->granule_position;
            } else if (s.vorbis_have_absgp) {
                s.vorbis_absgp += frames;
            }
        }
        const uint32_t before = outputs;
        const size_t at = stage_unit(r, s, d, n, frames, outputs);
        if (!frames) outputs = before;  // such a packet gives no AudioData
        r.vorbis_packets.push_back(sk_vorbis_tick_packet{(uint32_t)at, (uint32_t)n, keep, skip});
        return true;
    };
    auto full = [&](size_t next) {
        return outputs >= room || r.pcm_units.size() >= per_pass || (!r.pcm_units.empty() && r.pcm_bytes.size() + next + 4096 > kPcmTickBytes);
    };
    if (s.vorbis_ogg && s.pending.size() > s.pending_pos) {  // the pending bytes of the detection go in first
        std::string text;
        const bool ok = s.ogg->add(s.pending.data() + s.pending_pos, s.pending.size() - s.pending_pos, &text);
        s.pending.clear();
        s.pending.shrink_to_fit();
        s.pending_pos = 0;
        if (!ok) r.fail(SK_VORBIS_ERR_STREAM, "Decoding failed: " + text);
    }
    while (!r.failed) {
        if (s.vorbis_ogg && !s.ogg->pending.empty()) {
            if (full(s.ogg->pending.front().data.size())) {
                r.more = true;
                break;
            }
            const sk_ogg::Packet pk = std::move(s.ogg->pending.front());
            s.ogg->pending.pop_front();
            if (s.vorbis_headers == 0) {
                if (!pk.first_in_stream) {
                    r.fail(SK_VORBIS_ERR_STREAM, "Decoding failed: Expected Vorbis identification header as first Ogg packet");
                    break;
                }
                s.ogg_serial = pk.serial;
                if (!header(pk.data.data(), pk.data.size())) break;
                continue;
            }
            if (pk.serial != s.ogg_serial) {
                r.fail(SK_VORBIS_ERR_STREAM, "Decoding failed: Unexpected second Ogg logical bitstream");
                break;
            }
            if (s.vorbis_headers < 3 ? !header(pk.data.data(), pk.data.size()) : !audio(pk.data.data(), pk.data.size(), &pk)) break;
            continue;
        }
        if (s.webm) {
            if (!s.webm->packets.empty()) {
                if (full(s.webm->packets.front().data.size())) {
                    r.more = true;
                    break;
                }
                const sk_webm::Packet pk = s.webm->take_packet();
                if (!audio(pk.data.data(), pk.data.size(), nullptr, &pk)) break;
                continue;
            }
            if (!s.webm_error.empty()) {  // every complete packet has gone: what the demuxer refused
                r.fail(SK_WEBM_ERR_STREAM, "Decoding failed: " + s.webm_error);
                break;
            }
            if (s.webm_done) {
                r.eof = true;
                break;
            }
            {
                std::lock_guard<std::mutex> lk(s.mu);
                if (s.in.empty()) break;
                if (!s.in.front().empty() && full(0)) {
                    r.more = true;
                    break;
                }
            }
            if (webm_pull(s) == 0) break;
            continue;
        }
        if (s.saw_eof) {
            if (s.vorbis_ogg && !s.ogg_finished) {  // OggPacketParser::finish: a truncated page or packet, a missing EOS
                s.ogg_finished = true;
                std::string text;
                if (!s.ogg->finish(&text)) r.fail(SK_VORBIS_ERR_STREAM, "Decoding failed: " + text);
                continue;
            }
            r.eof = true;
            break;
        }
        std::vector<uint8_t> chunk;
        {
            std::lock_guard<std::mutex> lk(s.mu);
            if (s.in.empty()) break;
            if (!s.in.front().empty() && full(s.vorbis_ogg ? 0 : s.in.front().size())) {
                r.more = true;
                break;
            }
            chunk = std::move(s.in.front());
            s.in.pop_front();
        }
        if (chunk.empty()) {
            s.saw_eof = true;
            continue;
        }
        s.queued_bytes.fetch_sub(chunk.size());
        if (s.vorbis_ogg) {
            std::string text;
            if (!s.ogg->add(chunk.data(), chunk.size(), &text)) r.fail(SK_VORBIS_ERR_STREAM, "Decoding failed: " + text);
        } else if (!audio(chunk.data(), chunk.size(), nullptr)) {
            break;
        }
    }
    r.pcm_bytes.resize((r.pcm_bytes.size() + 15) & ~(size_t)15);
}

// A transport stream up to its track's first packet: the demuxer starts with the bytes of the detection, and the config that comes with
// the first packet decides what the stream is from here on (consume_mpeg_ts_events, soundkit-decoder/src/lib.rs:946: the first
// configuration is taken or refused).  ADTS AAC: an ADTS stream.  MPEG audio: an MPEG audio stream of the first frame's layer -- all three
// layers, where the reference's decode side takes Layer II alone.  Blu-ray LPCM: a raw PCM stream of big-endian samples at the header's
// rate.  LATM, AC-3, DTS: the reference's refusal.  false: more input is needed, or the stream has failed (r says how).
bool ts_open(PStream &s, Parsed &r) {
    if (!s.ts) {
        s.ts.reset(new sk_ts::Demuxer());
        const std::vector<uint8_t> head(s.pending.begin() + (ptrdiff_t)s.pending_pos, s.pending.end());
        s.pending.clear();
        s.pending_pos = 0;
        for (size_t at = 0; at < head.size() && !s.ts_done; at += 1u << 20) ts_feed(s, head.data() + at, std::min<size_t>(1u << 20, head.size() - at), false);
        if (s.saw_eof && !s.ts_done) ts_feed(s, nullptr, 0, true);
    }
    sk_ts::Demuxer &t = *s.ts;
    while (!t.configured) {
        if (!s.ts_error.empty()) return r.fail(SK_TS_ERR_STREAM, "Invalid input format: " + s.ts_error);
        if (s.ts_done) return r.fail(SK_TS_ERR_STREAM, "Invalid input format: MPEG-TS has no supported audio track");
        if (ts_pull(s) == 0) return false;
    }
    const sk_ts::Config &c = t.config;
    if (c.codec == sk_ts::kCodecAac && c.format == sk_ts::kFormatAdts) {
        s.codec = kCodecAac;
    } else if (c.codec == sk_ts::kCodecMp3 || c.codec == sk_ts::kCodecMp2 || c.codec == sk_ts::kCodecMp1) {
        s.codec = kCodecMp3;
        if (sk_mp3_internal::pipeline_gpu_hooks().mpa_find_layer) s.mpa_layer = c.codec == sk_ts::kCodecMp3 ? 3 : (c.codec == sk_ts::kCodecMp2 ? 2 : 1);
    } else if (c.codec == sk_ts::kCodecPcm && c.lpcm) {
        s.codec = kCodecRawPcm;
        s.raw_format = sk_raw_pcm_format{c.sample_rate, c.channels, (uint8_t)(c.bits == 16 ? SK_FMT_S16BE : SK_FMT_S24BE), 0};
        s.raw.reset(new sk_pcm::RawPcmStream(c.bytes_per_frame));
    } else {
        return r.fail(SK_TS_ERR_STREAM, std::string("Invalid input format: unsupported MPEG-TS audio codec ") + sk_ts::codec_name(c.codec));
    }
    s.ts_routed = true;
    ts_drain(s);  // the packets that came with the config go where the route says
    return true;
}

// An AVI or a program stream up to its config event: the demuxer starts with the bytes of the detection.  false: more input is needed, or
// the stream has failed (r says how).
bool cont_begin(PStream &s, Parsed &r, int32_t status, const char *none) {
    if (!s.avi && !s.ps) {
        if (s.codec == kCodecAvi) s.avi.reset(new sk_avi::Demuxer());
        else s.ps.reset(new sk_ps::Demuxer(sk_ps::kTrackFirst));
        const std::vector<uint8_t> head(s.pending.begin() + (ptrdiff_t)s.pending_pos, s.pending.end());
        s.pending.clear();
        s.pending_pos = 0;
        for (size_t at = 0; at < head.size() && !s.cont_done; at += 1u << 20) cont_feed(s, head.data() + at, std::min<size_t>(1u << 20, head.size() - at), false);
        if (s.saw_eof && !s.cont_done) cont_feed(s, nullptr, 0, true);
    }
    while (!(s.avi ? s.avi->configured : s.ps->configured)) {
        if (!s.cont_error.empty()) return r.fail(status, "Invalid input format: " + s.cont_error);
        if (s.cont_done) return r.fail(status, std::string("Invalid input format: ") + none);
        if (cont_pull(s) == 0) return false;
    }
    return true;
}

// An AVI stream becomes what its track is (decode_avi_audio's two matches on the format tag, lib.rs:288-308): integer PCM at 16 / 24 / 32
// bits and 32-bit float a raw PCM stream of that little-endian format, every `##wb` chunk's whole frames one piece and a partial frame
// carried to the next chunk (the framer's); 8-bit PCM a stream of the AIFF tick with SK_AIFF_U8; MPEG audio an MPEG audio stream.
bool avi_open(PStream &s, Parsed &r) {
    if (!cont_begin(s, r, SK_AVI_ERR_STREAM, "AVI has no audio stream")) return false;
    const sk_avi::Config &c = s.avi->config;
    char tag[8];
    std::snprintf(tag, sizeof tag, "%04x", (unsigned)c.format_tag);
    if (c.format_tag == 0x0001 || c.format_tag == 0x0003) {
        const bool is_float = c.format_tag == 0x0003;
        if (is_float && c.bits != 32) return r.fail(SK_AVI_ERR_STREAM, "Invalid input format: unsupported AVI float PCM depth " + std::to_string(c.bits));
        if (!is_float && c.bits != 8 && c.bits != 16 && c.bits != 24 && c.bits != 32)
            return r.fail(SK_AVI_ERR_STREAM, "Invalid input format: unsupported AVI integer PCM depth " + std::to_string(c.bits));
        if (c.bits == 8 && c.channels > sk_pcm::kMaxAiffChannels)
            return r.fail(SK_AVI_ERR_STREAM, "Invalid input format: AVI 8-bit PCM with more than " + std::to_string(sk_pcm::kMaxAiffChannels) + " channels is not built");
        s.codec = kCodecRawPcm;
        const uint8_t fmt = (uint8_t)(is_float ? SK_FMT_F32LE : (c.bits == 24 ? SK_FMT_S24LE : (c.bits == 32 ? SK_FMT_S32LE : SK_FMT_S16LE)));
        s.raw_format = sk_raw_pcm_format{c.sample_rate, c.channels, fmt, 0};
        if (c.bits == 8) s.raw_enc = true, s.aiff_enc = SK_AIFF_U8;
        s.raw.reset(new sk_pcm::RawPcmStream((size_t)c.channels * (c.bits / 8)));
    } else if (c.format_tag == 0x0055) {
        s.codec = kCodecMp3;
    } else if (c.format_tag >= 0x0160 && c.format_tag <= 0x0163) {
        return r.fail(SK_AVI_ERR_STREAM, "Invalid input format: AVI WMA decoding is not implemented");
    } else if (c.format_tag == 0x2000) {
        return r.fail(SK_AVI_ERR_STREAM, "Invalid input format: AVI AC-3 audio is not built");
    } else {
        return r.fail(SK_AVI_ERR_STREAM, std::string("Invalid input format: unsupported AVI audio format tag 0x") + tag);
    }
    s.cont_routed = true;
    cont_drain(s);
    return true;
}

// A program stream becomes what its track is: DVD LPCM at 16 bits a raw PCM stream of big-endian samples, at 24 bits a stream of the
// AIFF tick with SK_AIFF_DVD_S24 whose pieces are whole blocks; MPEG audio an MPEG audio stream.
bool ps_open(PStream &s, Parsed &r) {
    if (!cont_begin(s, r, SK_PS_ERR_STREAM, "MPEG-PS has no supported DVD LPCM track")) return false;
    const sk_ps::Config &c = s.ps->config;
    if (c.kind == sk_ps::kKindLpcm) {
        s.codec = kCodecRawPcm;
        s.raw_format = sk_raw_pcm_format{c.sample_rate, c.channels, (uint8_t)(c.bits == 16 ? SK_FMT_S16BE : SK_FMT_S24LE), 0};
        if (c.bits == 24) s.raw_enc = true, s.aiff_enc = SK_AIFF_DVD_S24;
        s.raw.reset(new sk_pcm::RawPcmStream(c.block_bytes));
    } else {
        s.codec = kCodecMp3;
    }
    s.cont_routed = true;
    cont_drain(s);
    return true;
}

// A WebM stream up to its first Cluster: the demuxer starts with the bytes of the detection, and the first audio track it reports
// decides what the stream is from here on (WebmDecoder::configure: the first configuration is taken or refused, a second one is
// refused).  A_VORBIS: the three headers out of the CodecPrivate go through the steps an Ogg stream's go through.  A_AAC: the
// CodecPrivate is an AudioSpecificConfig and meets the AAC-LC config check, as an MP4 track's does.  A_FLAC: the CodecPrivate is `fLaC`
// and the metadata blocks.  Anything else is what the reference says in a build without that codec.  false: more input is needed, or
// the stream has failed (r says how).
bool webm_open(PStream &s, Parsed &r) {
    if (!s.webm) {
        s.webm.reset(new sk_webm::Demuxer());
        const std::vector<uint8_t> head(s.pending.begin() + (ptrdiff_t)s.pending_pos, s.pending.end());
        s.pending.clear();
        s.pending_pos = 0;
        for (size_t at = 0; at < head.size() && !s.webm_done; at += 1u << 20) webm_feed(s, head.data() + at, std::min<size_t>(1u << 20, head.size() - at), false);
        if (s.saw_eof && !s.webm_done) webm_feed(s, nullptr, 0, true);
    }
    sk_webm::Demuxer &w = *s.webm;
    while (!w.configured || w.audio.empty()) {
        if (!s.webm_error.empty()) return r.fail(SK_WEBM_ERR_STREAM, "Decoding failed: " + s.webm_error);
        if (webm_pull(s) == 0) return false;
    }
    const sk_webm::Track &t = w.audio.front();
    const std::vector<uint8_t> &priv = t.codec_private;
    std::string text;
    if (t.codec == sk_webm::kCodecVorbis) {
        size_t offsets[3], sizes[3];
        if (!sk_webm::vorbis_headers(priv.data(), priv.size(), offsets, sizes, &text)) return r.fail(SK_WEBM_ERR_STREAM, "Decoding failed: " + text);
        s.vorbis = s.pcm_detected = true;
        for (int k = 0; k < 3; ++k)
            if (!vorbis_header(s, r, priv.data() + offsets[k], sizes[k])) return false;
        s.codec = kCodecVorbis;
    } else if (t.codec == sk_webm::kCodecAac) {
        if (!sk_mp4::asc_rate_channels(priv.data(), priv.size(), &s.webm_rate, &s.webm_channels))
            return r.fail(SK_WEBM_ERR_STREAM, "Decoding failed: WebM A_AAC CodecPrivate holds no AudioSpecificConfig with a rate of the table");
        sk_aac_decoder *probe = nullptr;
        const int rc = sk_aac_decoder_create(priv.data(), priv.size(), &probe);
        sk_aac_decoder_destroy(probe);
        if (rc != SK_OK) return r.fail(rc, std::string("Decoding failed: AAC-LC decoder init: ") + sk_strerror(rc));
        s.codec = kCodecAac;
    } else if (t.codec == sk_webm::kCodecFlac) {
        if (priv.size() < 42 || std::memcmp(priv.data(), "fLaC", 4) != 0)
            return r.fail(SK_WEBM_ERR_STREAM, "Decoding failed: WebM A_FLAC CodecPrivate holds no fLaC marker and STREAMINFO block");
        s.webm_flac_head = true;
        s.codec = kCodecFlac;
    } else {
        return r.fail(SK_WEBM_ERR_STREAM, "Decoding failed: unsupported or disabled WebM codec: " + t.codec_id);
    }
    if (w.audio.size() > 1) return r.fail(SK_WEBM_ERR_STREAM, "Decoding failed: WebM decoder received more than one audio configuration");
    s.webm_routed = true;
    if (s.codec == kCodecAac) webm_drain_aac(s);
    return true;
}

// A FLAC stream's pass: the reader cuts whole frames out of the chunks (marker and metadata first), and whole frames are what the
// stream is budgeted in -- `room` AudioData (one per frame, or one per completed 4096-frame chunk through the resampler) and the units
// of one stream in a tick.  Frames the reader holds beyond that come with the next pass (r.more).  A stream the reader rejects ends
// with its text; the frames in front of the damage have gone out with the passes before.
void parse_some_flac(sk_lane *p, PStream &s, uint32_t room, Parsed &r) {
    r.pcm = true;
    if (!s.flac) {
        s.flac.reset(new sk_flac::Reader());
        s.pcm_detected = true;
    }
    const uint32_t per_pass = std::min<uint32_t>(std::max<uint32_t>(p->cfg.max_stream_frames_per_tick, 1), 65536);
    uint32_t outputs = 0;
    std::vector<sk_flac_frame_info> got;
    // true: go on; the frames of one feed (all of them: the reader has let go of them) are staged
    auto feed = [&](const uint8_t *data, size_t len, bool final) -> bool {
        const uint32_t cap = per_pass - (uint32_t)r.pcm_units.size();
        got.resize(cap);
        uint32_t n = 0;
        const uint8_t *base = nullptr;
        if (!s.flac->feed(data, len, final, got.data(), cap, &n, &base)) {
            r.fail(SK_FLAC_ERR_STREAM, "Decoding failed: " + s.flac->error());
            return false;
        }
        if (n && !s.pcm_route && !pcm_open(p, s, r)) return false;
        for (uint32_t k = 0; k < n; ++k) {
            sk_flac_frame_info f = got[k];
            f.offset = (uint32_t)stage_unit(r, s, base + f.offset, f.frame_bytes, f.block_size, outputs);
            r.flac_frames.push_back(f);
        }
        if (n == cap) r.more = true;  // the reader may hold further frames
        return true;
    };
    // what a feed can stage: everything the reader holds, each frame padded to 16 bytes
    auto fits = [&](size_t next) {
        return r.pcm_bytes.size() + s.flac->buffered_bytes() + next + 16 * (size_t)per_pass + 4096 <= kPcmTickBytes;
    };
    // an A_FLAC track of a WebM stream: the chunks go through the demuxer, and what it hands out -- the CodecPrivate, then the frames --
    // is the native stream the reader takes.  A feed gets at most the demuxer's queue budget
    std::vector<uint8_t> demuxed;
    auto container_bytes = [&] { s.webm ? webm_flac_bytes(s, demuxed) : mp4_flac_bytes(s, demuxed); };  // (an MP4 `fLaC` track: the same)
    if (s.webm || s.mp4) {
        if (s.more && !feed(nullptr, 0, s.saw_eof && s.flac->finalised())) return;  // frames left over by the pass before
        if (!r.more) container_bytes();  // (else they stay with the demuxer for the next pass)
        if (!demuxed.empty() && !feed(demuxed.data(), demuxed.size(), false)) return;
    } else if (s.pending.size() > s.pending_pos) {  // the pending bytes of the detection (parse_some gathered them) go in first
        std::vector<uint8_t> first(s.pending.begin() + (ptrdiff_t)s.pending_pos, s.pending.end());
        s.pending.clear();
        s.pending.shrink_to_fit();
        s.pending_pos = 0;
        if (!feed(first.data(), first.size(), false)) return;
    } else if (s.more && !feed(nullptr, 0, s.saw_eof && s.flac->finalised())) {  // frames left over by the pass before
        return;
    }
    while (!r.failed && !r.more) {
        if (outputs >= room || r.pcm_units.size() >= per_pass) {
            r.more = true;
            break;
        }
        if (s.saw_eof) {  // the finalising feed: the last frame ends with the data; a truncated tail ends the stream with its text
            if (!feed(nullptr, 0, true)) break;
            if (!r.more) r.eof = true;
            break;
        }
        std::vector<uint8_t> chunk;
        {
            std::lock_guard<std::mutex> lk(s.mu);
            if (s.in.empty()) break;
            if (!s.in.front().empty() && !r.pcm_units.empty() && !fits(s.webm ? kMaxWebmQueuedBytes : (s.mp4 ? s.mp4->buffered() : 0) + s.in.front().size())) {
                r.more = true;
                break;
            }
            chunk = std::move(s.in.front());
            s.in.pop_front();
        }
        if (s.webm) {  // the frames in front of a refusal are fed; the last of them waits in the reader for its end and goes with the stream
            if (chunk.empty()) s.saw_eof = true;
            else s.queued_bytes.fetch_sub(chunk.size());
            webm_feed(s, chunk.data(), chunk.size(), chunk.empty());
            demuxed.clear();
            webm_flac_bytes(s, demuxed);
            if (!demuxed.empty() && !feed(demuxed.data(), demuxed.size(), false)) break;
            if (!s.webm_error.empty()) r.fail(SK_WEBM_ERR_STREAM, "Decoding failed: " + s.webm_error);
            continue;
        }
        if (s.mp4) {  // the same for an MP4 stream
            if (chunk.empty()) {
                s.saw_eof = s.mp4_done = true;
                (void)s.mp4->finish();
            } else {
                s.queued_bytes.fetch_sub(chunk.size());
                (void)s.mp4->add(chunk.data(), chunk.size());
            }
            if (s.mp4->failed && s.mp4_error.empty()) s.mp4_error = s.mp4->error;
            demuxed.clear();
            mp4_flac_bytes(s, demuxed);
            if (!demuxed.empty() && !feed(demuxed.data(), demuxed.size(), false)) break;
            if (!s.mp4_error.empty()) r.fail(SK_MP4_ERR_STREAM, "Decoding failed: " + s.mp4_error);
            continue;
        }
        if (chunk.empty()) {
            s.saw_eof = true;
            continue;
        }
        s.queued_bytes.fetch_sub(chunk.size());
        if (!feed(chunk.data(), chunk.size(), false)) break;
    }
    r.pcm_bytes.resize((r.pcm_bytes.size() + 15) & ~(size_t)15);
}

// A WAV / raw PCM stream's pass.  Unit boundaries are the reference worker's: one `process` per received chunk, each giving at most one
// piece (lib.rs:3006-3029); a WAV stream's first `process` is the detection buffer -- chunks gathered until kMinDetectionBytes are there
// or the stream ends, at most kMaxDetectionBytes of them -- and the rest of the chunk that completed it a second one (lib.rs:2926-3003).
// `room` bounds the outputs of the pass (one per piece, or one per completed 4096-frame chunk through the resampler); a piece is
// never split, so the last one may overshoot.
void parse_some_pcm(sk_lane *p, PStream &s, uint32_t room, Parsed &r) {
    r.pcm = true;
    uint32_t outputs = 0;
    // A piece of whole ADPCM blocks: cut to the blocks the fact cap still needs, and to the blocks in front of the first one its header
    // rules out -- those are staged as a unit, then the stream ends with the block's text.
    auto process_wav_adpcm = [&](const sk_pcm::Piece &piece) -> bool {
        const uint32_t align = s.wav->block_align(), per = s.wav->frames_per_block(), tag = s.wav->tag();
        size_t blocks = piece.len / align;
        blocks = (size_t)std::min<uint64_t>(blocks, (s.wav_parse_left + per - 1) / per);  // what lies behind the cap is padding
        std::string bad;
        for (size_t k = 0; k < blocks && bad.empty(); ++k) {
            const uint8_t *blk = piece.data + k * align;
            for (uint32_t c = 0; c < s.channels && bad.empty(); ++c) {
                if (tag == SK_WAV_TAG_IMA_ADPCM && blk[4 * c + 2] > 88)
                    bad = "WAV IMA ADPCM block step index " + std::to_string(blk[4 * c + 2]) + " exceeds 88";
                if (tag == SK_WAV_TAG_MS_ADPCM && blk[c] >= s.wav->n_coef())
                    bad = "WAV MS ADPCM block predictor " + std::to_string(blk[c]) + " exceeds the " + std::to_string(s.wav->n_coef()) + " coefficient sets";
            }
            if (!bad.empty()) blocks = k;
        }
        if (blocks) {
            const uint32_t frames = (uint32_t)std::min<uint64_t>((uint64_t)blocks * per, s.wav_parse_left);
            s.wav_parse_left -= frames;
            stage_unit(r, s, piece.data, blocks * align, frames, outputs);
        }
        if (!bad.empty()) r.fail(SK_PCM_ERR_STREAM, "Decoding failed: " + bad);
        return bad.empty();
    };
    auto process = [&](const uint8_t *data, size_t len) -> bool {
        sk_pcm::Piece piece;
        std::string err;
        const bool ok = s.aiff ? s.aiff->add(data, len, piece, err) : (s.wav ? s.wav->add(data, len, piece, err) : s.raw->add(data, len, piece, err));
        if (!ok) {
            r.fail(SK_PCM_ERR_STREAM, "Decoding failed: " + err);
            return false;
        }
        if (piece.len == 0) return true;
        if (!s.pcm_route && !pcm_open(p, s, r)) return false;
        if (s.wav_adpcm) return process_wav_adpcm(piece);
        // (an AIFF piece is source-encoded: its frames follow from its sample groups; so is a G.711 WAV's, a byte a sample)
        const uint32_t frame_bytes = (uint32_t)s.pcm_bits / 8 * s.channels;
        const uint32_t frames = s.wav_g711 ? (uint32_t)(piece.len / s.channels) : s.raw_enc ? (uint32_t)(piece.len / (s.aiff_enc == SK_AIFF_U8 ? 1 : 3) / s.channels) : s.aiff ? (uint32_t)(piece.len / sk_pcm::aiff_group_bytes(s.aiff_enc, s.channels) * (s.aiff_enc == SK_AIFF_IMA4 ? 64 : 1) /
                                                    (s.aiff_enc == SK_AIFF_IMA4 ? 1 : s.channels))
                                       : (uint32_t)(piece.len / frame_bytes);
        // the decoder emits every complete SAMPLE of an add: a piece may end inside a frame.  Delivered as it is that is what the
        // reference delivers; its conversions refuse it (audio_data_to_f32_channels, lib.rs:3569-3574)
        if (s.aiff && !s.aiff_plain && s.pcm_route == kPcmAiffTick && s.aiff_enc != SK_AIFF_IMA4 &&
            piece.len / sk_pcm::aiff_group_bytes(s.aiff_enc, s.channels) % s.channels != 0) {
            r.fail(SK_PCM_ERR_STREAM, "Decoding failed: Output conversion failed: PCM data is unsupported or contains a partial frame");
            return false;
        }
        if (s.pcm_route == kPcmFast) {
            Output o;
            o.rate = s.rate, o.frames = frames, o.bits = s.pcm_bits, o.channels = s.channels, o.flags = s.pcm_flags;
            o.data.assign(piece.data, piece.data + piece.len);
            r.pre.push_back(std::move(o));
            outputs += 1;
            return true;
        }
        stage_unit(r, s, piece.data, piece.len, frames, outputs);
        return true;
    };
    if ((s.codec == kCodecWav || s.codec == kCodecAiff) && !s.pcm_detected) {
        while (s.pending.size() - s.pending_pos < kMinDetectionBytes && !s.saw_eof)
            if (pull_input(s) == 0) return;  // needs more input
        if (s.codec == kCodecAiff) s.aiff.reset(new sk_pcm::AiffStream());
        else s.wav.reset(new sk_pcm::WavStream(true));  // the coded mode: tags 1 and 3 walk as before
        s.pcm_detected = true;
        const uint8_t *d = s.pending.data() + s.pending_pos;
        const size_t n = s.pending.size() - s.pending_pos, first = std::min(n, kMaxDetectionBytes);
        bool ok = process(d, first);
        if (ok && n > first) ok = process(d + first, n - first);
        s.pending.clear();
        s.pending.shrink_to_fit();
        s.pending_pos = 0;
        if (!ok) return;
    }
    // the pass's limits: the output queue's room, the units of one stream in a tick, the bytes one tick takes
    auto full = [&](size_t next) {
        return outputs >= room || r.pcm_units.size() + r.pre.size() >= p->cfg.max_stream_frames_per_tick ||
               (!r.pcm_units.empty() && r.pcm_bytes.size() + next + 4096 > kPcmTickBytes);
    };
    while (!r.failed) {
        if (s.ts && (!s.ts->packets.empty() || !s.saw_eof)) {  // Blu-ray LPCM out of a transport stream: every PES payload is one piece
            if (s.ts->packets.empty()) {
                if (ts_pull(s) == 0) break;
                continue;
            }
            if (full(s.ts->packets.front().data.size())) {
                r.more = true;
                break;
            }
            const sk_ts::Packet pk = s.ts->take_packet();
            if (!process(pk.data.data(), pk.data.size())) break;
            continue;
        }
        // an AVI's `##wb` chunks, a program stream's whole blocks: one piece each (a chunk above 1 MiB goes in slices of that size)
        if ((s.avi || s.ps) && (s.cont_piece_pos < s.cont_piece.size() || cont_has_packets(s) || !s.saw_eof)) {
            if (s.cont_piece_pos >= s.cont_piece.size()) {
                if (!cont_has_packets(s)) {
                    if (cont_pull(s) == 0) break;
                    continue;
                }
                cont_take(s, s.cont_piece);
                s.cont_piece_pos = 0;
                continue;
            }
            const size_t n = std::min<size_t>(1u << 20, s.cont_piece.size() - s.cont_piece_pos);
            if (full(n)) {
                r.more = true;
                break;
            }
            const uint8_t *data = s.cont_piece.data() + s.cont_piece_pos;
            s.cont_piece_pos += n;
            if (!process(data, n)) break;
            continue;
        }
        if (s.mp4) {  // a PCM track of an MP4 stream: every run of frames the demuxer hands out is one piece
            if (!s.mp4->packets.empty()) {
                if (full(s.mp4->packets.front().data.size())) {
                    r.more = true;
                    break;
                }
                const sk_mp4::Packet pk = std::move(s.mp4->packets.front());
                s.mp4->packets.pop_front();
                if (!process(pk.data.data(), pk.data.size())) break;
                continue;
            }
            if (!s.mp4_error.empty()) {  // every complete run has gone: what the demuxer refused
                r.fail(SK_MP4_ERR_STREAM, "Decoding failed: " + s.mp4_error);
                break;
            }
            if (!s.saw_eof) {
                if (pull_mp4(s) == 0) break;
                continue;
            }
        }
        if (s.saw_eof) {  // flush_decoder (lib.rs:3139-3169): the framer's partial frame is an error, the resampler is flushed by the tick
            std::string err;
            if (s.raw && !s.raw->flush(err)) r.fail(SK_PCM_ERR_STREAM, "Decoding failed: " + err);
            else if (s.aiff && !process(nullptr, 0)) {}  // the finalising empty add (lib.rs:2426): a truncated stream ends with its text
            else r.eof = true;
            break;
        }
        std::vector<uint8_t> chunk;
        {
            std::lock_guard<std::mutex> lk(s.mu);
            if (s.in.empty()) break;
            const size_t next = s.in.front().size();
            if (next && full(next)) {
                r.more = true;
                break;
            }
            chunk = std::move(s.in.front());
            s.in.pop_front();
        }
        if (chunk.empty()) {
            s.saw_eof = true;
            continue;
        }
        s.queued_bytes.fetch_sub(chunk.size());
        if (!process(chunk.data(), chunk.size())) break;
    }
    r.pcm_bytes.resize((r.pcm_bytes.size() + 15) & ~(size_t)15);
}

// Pulls ADTS frames out of the stream's byte queue and runs the front-end on them, at most `limit` frames.
void parse_some(sk_lane *p, PStream &s, uint32_t limit, float *coeffs, sk_aac_frame_desc *descs, std::vector<uint8_t> &au_stage,
                sk_au_item *au_items, uint32_t room, Parsed &r) {
    const bool gpu_entropy = p->cfg.gpu_entropy == 1;
    const bool quant = p->cfg.gpu_entropy == 2;  // host Huffman decode, the rest of the front-end on the device (sk_tick_run_q)
    while (s.codec == 0) {  // the worker's detect_and_init_decoder: the stream's first bytes choose the decoder
        s.codec = sniff_codec(s.pending.data() + s.pending_pos, s.pending.size() - s.pending_pos, s.saw_eof);
        if (s.codec) break;
        if (s.saw_eof) {
            s.codec = kCodecAac;  // too short to tell: the ADTS path ends it
            break;
        }
        if (pull_input(s) == 0) return;  // needs more input
    }
    if (s.codec == kCodecWebm && !webm_open(s, r)) return;  // taken by its EBML magic: from its first Cluster on it is one of the streams below
    if (s.codec == kCodecTs && !ts_open(s, r)) return;      // a transport stream: from its track's first packet on it is one of the streams below
    if (s.codec == kCodecAvi && !avi_open(s, r)) return;    // an AVI, a program stream: the same from the config event on
    if (s.codec == kCodecPs && !ps_open(s, r)) return;
    if (s.codec == kCodecMp3) {
        // MPEG audio of which layer: that of the stream's first confirmed frame (two consistent headers one frame length apart)
        const sk_mp3_internal::PipelineGpuHooks &hooks = sk_mp3_internal::pipeline_gpu_hooks();
        if (s.mpa_layer == 0 && (s.engine_stream != kNoStream || !hooks.mpa_find_layer)) s.mpa_layer = 3;  // Layer III frames have decoded
        while (s.mpa_layer == 0) {
            const int layer = hooks.mpa_find_layer(s.pending.data() + s.pending_pos, s.pending.size() - s.pending_pos);
            if (layer > 0) {
                s.mpa_layer = (uint8_t)layer;
                break;
            }
            // 0: no header in sight; -3: a Layer III candidate waits for its follower -- the Layer III pass's business, which settles
            // nothing: the question is asked again at the next pass (Mp3Decoder does the same, mp12_decoder.cpp)
            if (layer != -1) break;
            if (s.saw_eof) break;                    // a lone unconfirmed frame: no frame, as the Layer III scan will find
            if (pull_input(s) == 0) return;          // a Layer I / II candidate waits for the header behind it: needs more input
        }
        if (s.mpa_layer == 1 || s.mpa_layer == 2) {
            // room counts AudioData: a Layer II frame gives two (never split: the last frame of a pass may overshoot by one)
            parse_some_mpa(p, s, s.mpa_layer == 2 ? std::max(1u, limit / 2) : limit, r);
            return;
        }
        parse_some_mp3(p, s, limit, r);
        return;
    }
    if (s.codec == kCodecFlac) {
        parse_some_flac(p, s, room, r);
        return;
    }
    if (s.codec == kCodecAlac) {
        parse_some_alac(p, s, room, r);
        return;
    }
    if (s.codec == kCodecVorbis) {
        if (!s.vorbis) {  // taken by its first page: the Ogg walk starts here, with the bytes of the detection
            s.vorbis = s.vorbis_ogg = true;
            s.ogg.reset(new sk_ogg::Parser());
            s.pcm_detected = true;
        }
        parse_some_vorbis(p, s, room, r);
        return;
    }
    if (s.codec == kCodecG72x) {
        parse_some_g72x(p, s, room, r);
        return;
    }
    if (s.codec == kCodecGsm) {
        parse_some_gsm(p, s, room, r);
        return;
    }
    if (s.codec == kCodecWav || s.codec == kCodecRawPcm || s.codec == kCodecAiff) {
        parse_some_pcm(p, s, room, r);
        return;
    }
    if (s.codec == kCodecMp4 && !s.mp4) {  // taken by its ftyp: the box walk starts here, with the bytes of the detection
        s.mp4.reset(new sk_mp4::Demuxer());
        const std::vector<uint8_t> head(s.pending.begin() + (ptrdiff_t)s.pending_pos, s.pending.end());
        s.pending.clear();
        s.pending_pos = 0;
        for (size_t at = 0; at < head.size(); at += 1u << 20) (void)s.mp4->add(head.data() + at, std::min<size_t>(1u << 20, head.size() - at));
        if (s.saw_eof) {
            s.mp4_done = true;
            (void)s.mp4->finish();
        }
        mp4_drain(s);
    }
    if (s.mp4 && s.codec != kCodecMp4) {  // the config event made it a FLAC or a raw PCM stream: that stream's pass, from here on
        parse_some(p, s, limit, coeffs, descs, au_stage, au_items, room, r);
        return;
    }
    while (r.n_frames < limit && !r.failed) {
        // make sure a whole frame is in `pending`
        size_t avail = s.pending.size() - s.pending_pos;
        size_t frame_len = 0, pay_off = 0, pay_len = 0;
        uint8_t asc[2];
        bool have = false;
        while (avail >= 7) {
            const uint8_t *d = s.pending.data() + s.pending_pos;
            if (sk_adts_parse(d, avail, &frame_len, &pay_off, &pay_len, asc) != SK_OK) {  // resynchronise
                s.pending_pos += 1;
                avail -= 1;
                continue;
            }
            have = avail >= frame_len;
            break;
        }
        if (!have) {
            if (s.mp4 && !s.mp4_done) {  // an MP4 stream: more frames come out of the demuxer
                if (pull_mp4(s) == 0) break;
                if (s.codec != kCodecMp4) {  // moov has arrived and the track is FLAC or PCM (nothing has been staged before the config)
                    parse_some(p, s, limit, coeffs, descs, au_stage, au_items, room, r);
                    return;
                }
                continue;
            }
            if (s.webm && !s.webm_done) {  // a WebM stream's A_AAC track: more frames come out of the demuxer
                if (webm_pull(s) == 0) break;
                webm_drain_aac(s);
                continue;
            }
            if (s.webm && !s.webm_error.empty()) {
                r.fail(SK_WEBM_ERR_STREAM, "Decoding failed: " + s.webm_error);
                break;
            }
            if (s.mp4 && !s.mp4_error.empty()) {  // every complete unit has gone: what the demuxer or the config check refused
                r.fail(SK_MP4_ERR_STREAM, "Decoding failed: " + s.mp4_error);
                break;
            }
            if (s.saw_eof) {  // whatever is left is not a frame: flush_decoder has nothing more to give
                r.eof = true;
                break;
            }
            if (pull_input(s) == 0) break;  // needs more input
            continue;
        }
        const uint8_t *frame = s.pending.data() + s.pending_pos;
        if (!s.fe) {  // first header: AacLcDecoder::from_audio_specific_config (lib.rs:1007-1027, decoder.rs:80)
            int rc = sk_aac_decoder_create(asc, 2, &s.fe);
            if (rc != SK_OK) {
                r.fail(rc, std::string("Decoding failed: AAC-LC decoder init: ") + sk_strerror(rc));
                break;
            }
            s.asc[0] = asc[0];
            s.asc[1] = asc[1];
            (void)sk_aac_decoder_info(s.fe, &s.rate, &s.channels);
            rc = sk_stream_open(p->engine, s.rate, s.channels, &s.engine_stream);
            if (rc != SK_OK) {
                r.fail(rc, std::string("Decoding failed: engine stream: ") + sk_strerror(rc));
                break;
            }
            const uint32_t target = s.opt.output_sample_rate ? s.opt.output_sample_rate : s.rate;
            s.resample = target != s.rate;
            if (s.resample) {
                rc = sk_resampler_open(p->engine, s.engine_stream, s.rate, target);
                if (rc != SK_OK) {  // StreamingResampler::new failing, lib.rs:3405-3417
                    s.resample = false;  // no resampler: the failed pass's row in the tick must not ask for one (the tick would refuse every stream in it)
                    r.fail(rc, "Decoding failed: Failed to create resampler: unsupported rate pair");
                    break;
                }
            }
        } else if (asc[0] != s.asc[0] || asc[1] != s.asc[1]) {
            r.fail(SK_AAC_ERR_UNSUPPORTED_FEATURE, "Decoding failed: AAC configuration changed mid-stream");
            break;
        }
        if (gpu_entropy) {  // framing only: the access unit itself goes to the device
            const size_t padded = (pay_len + 8 + 3) & ~(size_t)3;
            // one pass never stages more than an empty batch holds (a stream of maximum-length ADTS frames would otherwise
            // wait for room that cannot come); the rest of the stream's frames go into the next tick
            if (r.n_frames > 0 && r.n_au_bytes + padded > p->au_pass_budget) {
                r.budget_stop = true;
                break;
            }
            if (au_stage.size() < r.n_au_bytes + padded) au_stage.resize(r.n_au_bytes + padded + 4096);
            std::memcpy(au_stage.data() + r.n_au_bytes, frame + pay_off, pay_len);
            std::memset(au_stage.data() + r.n_au_bytes + pay_len, 0, padded - pay_len);
            au_items[r.n_frames] = sk_au_item{(uint32_t)r.n_au_bytes, (uint32_t)pay_len};
            r.n_au_bytes += padded;
        } else if (quant) {  // i16 values where the f32 spectra would go, side records staged like access units
            sk_aac_frame_desc &d = descs[r.n_frames];
            if (au_stage.size() < r.n_au_bytes + SK_AAC_UNIT_SIDE_BYTES) au_stage.resize(r.n_au_bytes + SK_AAC_UNIT_SIDE_BYTES + 8192);
            const int rc = sk_aac_decoder_parse_q(s.fe, frame + pay_off, pay_len, reinterpret_cast<int16_t *>(coeffs) + r.n_floats,
                                                  au_stage.data() + r.n_au_bytes, &d);
            if (rc != SK_OK) {
                r.fail(rc, std::string("Decoding failed: ") + sk_aac_decoder_last_error(s.fe));
                break;
            }
            d.stream = s.engine_stream;
            r.n_au_bytes += SK_AAC_UNIT_SIDE_BYTES;
            r.raw.insert(r.raw.end(), frame + pay_off, frame + pay_off + pay_len);
            r.raw_len.push_back((uint32_t)pay_len);
        } else {
            sk_aac_frame_desc &d = descs[r.n_frames];
            const int rc = sk_aac_decoder_parse(s.fe, frame + pay_off, pay_len, coeffs + r.n_floats, &d);
            if (rc != SK_OK) {
                r.fail(rc, std::string("Decoding failed: ") + sk_aac_decoder_last_error(s.fe));
                break;
            }
            d.stream = s.engine_stream;
        }
        s.pending_pos += frame_len;
        r.n_frames += 1;
        r.n_floats += (size_t)s.channels * 1024;
    }
}

int ensure_mp3(sk_lane *p) {
    if (p->mp3_ready.load(std::memory_order_acquire)) return SK_OK;
    std::lock_guard<std::mutex> lk(p->mp3_mu);
    if (p->mp3_ready.load(std::memory_order_relaxed)) return SK_OK;
    sk_mp3_tables t;
    int rc = sk_mp3_iso_tables(&t);
    if (rc != SK_OK) return rc;
    static const uint32_t rates[9] = {44100, 48000, 32000, 22050, 24000, 16000, 11025, 12000, 8000};
    for (int row = 0; row < 9 && rc == SK_OK; ++row) rc = sk_mp3_set_band_tables(p->engine, rates[row], t.long_offsets[row], t.short_offsets[row], t.pretab);
    if (rc == SK_OK) rc = sk_mp3_set_synthesis_window(p->engine, t.window);
    if (rc != SK_OK) return rc;
    if (!p->mp3_cb) {
        rc = sk_mp3_codebook_create(&t, &p->mp3_cb);
        if (rc != SK_OK) return rc;
    }
    if (p->mp3_gpu && p->mp3_blob.empty()) {
        size_t words = 0;
        rc = sk_mp3_codebook_flatten(p->mp3_cb, nullptr, 0, &words);
        if (rc != SK_OK && rc != SK_ERR_CAPACITY) return rc;
        std::vector<uint32_t> blob(words);
        rc = sk_mp3_codebook_flatten(p->mp3_cb, blob.data(), blob.size(), &words);
        if (rc == SK_OK) rc = sk_mp3_internal::pipeline_gpu_hooks().install_codebook(p->engine, blob.data(), blob.size());
        if (rc != SK_OK) return rc;
        p->mp3_blob.swap(blob);
    }
    {
        // the batches' granule arrays: workers copy into disjoint ranges without the lock, so they are sized once, here, while
        // no MP3 claim can exist yet (an MP3 pass reaches the batches only behind this function)
        std::lock_guard<std::mutex> bl(p->batch_mu);
        for (Batch &b : p->batches) {
            if (b.mp3_is || !b.mp3_frames.empty()) continue;
            const size_t cap = p->cfg.max_frames_per_tick;
            if (p->mp3_gpu) {  // frames instead of granules and integers (a frame has at least one granule)
                b.mp3_frames.resize(cap);
                continue;
            }
            if (hipHostMalloc((void **)&b.mp3_is, cap * 2 * 576 * sizeof(int16_t) + 64, hipHostMallocPortable) != hipSuccess) {
                b.mp3_is = nullptr;
                return SK_ERR_OOM;
            }
            b.mp3_gr.resize(cap);
            b.mp3_desc.resize(cap);
        }
    }
    p->mp3_ready.store(true, std::memory_order_release);
    return SK_OK;
}

// test hook (sk_debug_throw_in_thread): the n-th passage of point `where` throws std::bad_alloc
std::atomic<int> g_thread_throw_after{-1}, g_thread_throw_where{-1};
void thread_debug_point(int where) {
    if (g_thread_throw_after.load(std::memory_order_relaxed) < 0 || g_thread_throw_where.load(std::memory_order_relaxed) != where) return;
    if (g_thread_throw_after.fetch_sub(1) == 0) throw std::bad_alloc();
}

inline void shift_unit(sk_pcm_unit &u, size_t by) { u.byte_offset += by; }
inline void shift_unit(sk_flac_frame_info &f, size_t by) { f.offset += (uint32_t)by; }
inline void shift_unit(sk_alac_tick_packet &k, size_t by) { k.offset += (uint32_t)by; }
inline void shift_unit(sk_vorbis_tick_packet &k, size_t by) { k.offset += (uint32_t)by; }

// A PCM-family pass joins the table of its tick (batch_mu held): nothing when it neither brings units nor ends a resampler; else it
// takes its place in the batch's staged bytes (pcm_at) and a row with what the three ticks' rows share, and its units follow with
// their offsets moved to that place.  The row comes back for the fields that are its kind's own.
template <class Row, class Unit>
Row *claim_tick_row(Batch *b, TickTable<Row, Unit> &t, const PStream &s, const Parsed &r, const std::vector<Unit> &units, BatchEntry &be, size_t &pcm_at) {
    if (units.empty() && !(r.eof && s.resample)) return nullptr;
    pcm_at = b->pcm_used;
    b->pcm_used += r.pcm_bytes.size();
    Row row{};
    row.stream = s.engine_stream == kNoStream ? 0 : s.engine_stream;
    row.n_units = (uint32_t)units.size();
    row.channels = s.channels;
    row.out_bits = s.opt.output_bits_per_sample ? s.opt.output_bits_per_sample : s.pcm_bits;
    row.out_channels = s.opt.output_channels ? s.opt.output_channels : s.channels;
    row.resample = s.resample ? 1 : 0;
    row.flush = (r.eof && s.resample) ? 1 : 0;
    t.rows.push_back(row);
    be.pcm_row = true;
    t.entry.push_back((uint32_t)b->entries.size());
    for (Unit u : units) {
        shift_unit(u, pcm_at);
        t.units.push_back(u);
    }
    return &t.rows.back();
}

void worker_body(sk_lane *p) {
    const uint32_t per_stream = p->cfg.max_stream_frames_per_tick;
    const bool gpu_entropy = p->cfg.gpu_entropy == 1, quant = p->cfg.gpu_entropy == 2;
    std::vector<float> coeffs(gpu_entropy ? 0 : (size_t)per_stream * 2 * 1024);  // quant: the same storage holds i16 (half of it)
    std::vector<sk_aac_frame_desc> descs(per_stream);
    std::vector<uint8_t> au_stage;
    std::vector<sk_au_item> au_items(per_stream);
    for (;;) {
        uint32_t handle;
        {
            std::unique_lock<std::mutex> lk(p->rq_mu);
            p->workers_waiting_ready.fetch_add(1);
            p->rq_cv.wait(lk, [&] { return p->stop || !p->ready.empty(); });
            p->workers_waiting_ready.fetch_sub(1);
            if (p->stop) return;
            handle = p->ready.front();
            p->ready.pop_front();
        }
        thread_debug_point(1);
        PStream &s = *p->streams[handle];
        uint32_t room;
        {
            std::lock_guard<std::mutex> lk(s.mu);
            s.queued = false;
            if (!s.open || s.busy || s.finished || s.cancelled) continue;
            room = s.out.size() < p->cfg.output_buffer ? p->cfg.output_buffer - (uint32_t)s.out.size() : 0;
            if (room == 0) continue;
            s.busy = true;
        }
        Parsed r;
        p->workers_parsing.fetch_add(1);
        const Clock::time_point t0 = Clock::now();
        // room in the output queue bounds the access units of this pass: one AudioData per unit, or -- through the
        // streaming resampler -- one per completed chunk of 4096 source frames = 4 units (lib.rs:1970-2003)
        const uint32_t limit = std::min(per_stream, s.resample ? (room > per_stream / 4 ? per_stream : 4 * room) : room);
        try {
            thread_debug_point(0);
            parse_some(p, s, limit, coeffs.data(), descs.data(), au_stage, au_items.data(), room, r);
            // a transport stream the demuxer refused: its pass has come to the end of the units in front of the refusal
            if (s.ts && r.eof && !r.failed && !s.ts_error.empty()) {
                r.eof = false;
                r.fail(SK_TS_ERR_STREAM, "Invalid input format: " + s.ts_error);
            }
            if ((s.avi || s.ps) && r.eof && !r.failed && !s.cont_error.empty()) {  // the same for an AVI or a program stream
                r.eof = false;
                r.fail(s.avi ? SK_AVI_ERR_STREAM : SK_PS_ERR_STREAM, "Invalid input format: " + s.cont_error);
            }
        } catch (...) {
            // whatever was thrown while this stream's input was parsed is this stream's error and nobody else's
            // (soundkit-decoder/src/lib.rs:3131-3134); the frames of this pass are dropped with it
            r = Parsed{};
            r.failed = true;
            r.fail_status = sk::abi_caught("entropy thread");
            try {
                r.fail_msg = std::string("Decoding failed: ") + sk_strerror(r.fail_status) + ": " + sk::abi_message();
            } catch (...) {
            }
        }
        {
            std::lock_guard<std::mutex> lk(s.mu);  // read by mark_schedulable and the state dump
            s.more = (r.pcm ? r.more : (r.n_frames == limit || r.budget_stop)) && !r.eof && !r.failed;  // (a Layer I / II pass that met its frame limit: budget_stop)
        }
        p->parse_ns.fetch_add(ns_since(t0));
        p->workers_parsing.fetch_sub(1);
        if (r.n_frames == 0 && r.pcm_units.empty() && r.pre.empty() && !r.eof && !r.failed) {  // nothing complete yet
            bool dropped;
            {
                std::lock_guard<std::mutex> lk(s.mu);
                s.busy = false;
                dropped = s.cancelled;
                if (dropped) s.open = false;
                maybe_schedule(p, s, handle);
            }
            if (dropped) {  // the handle was dropped while this worker held the stream
                release_device_side(p, s);
                std::lock_guard<std::mutex> lk(p->handles_mu);
                p->free_handles.push_back(handle);
            }
            continue;
        }
        // claim room in the batch being filled
        Batch *b;
        size_t desc_at, float_at, au_at, mp3_at = 0, mp3_row_at = 0, mp3_frame_at = 0, pcm_at = 0;
        {
            std::unique_lock<std::mutex> lk(p->batch_mu);
            p->workers_waiting_room.fetch_add(1);
            p->room_cv.wait(lk, [&] {
                const Batch &f = p->batches[p->filling];
                return p->stop || (f.n_descs + f.n_mp3 + f.mpa_recs.size() + r.n_frames <= p->cfg.max_frames_per_tick &&
                                   (gpu_entropy ? f.au_used + r.n_au_bytes <= f.au_cap : f.n_floats + r.n_floats <= f.coeff_cap) &&
                                   (!quant || f.au_used + r.n_au_bytes <= f.au_cap) &&
                                   (r.pcm_units.empty() || f.pcm_used + r.pcm_bytes.size() <= f.pcm_cap));
            });
            p->workers_waiting_room.fetch_sub(1);
            if (p->stop) return;
            b = &p->batches[p->filling];
            desc_at = b->n_descs;
            float_at = b->n_floats;
            au_at = b->au_used;
            mp3_at = b->n_mp3;
            mp3_row_at = b->mp3_rows;
            mp3_frame_at = b->n_mp3_frames;
            b->mp3_frames_of.push_back((uint32_t)r.mp3_frames.size());
            if (r.mpa) {  // whole frames, in claim order = the order of their streams in ts
                const size_t at = (b->mpa_bytes.size() + 3) & ~(size_t)3;
                b->mpa_bytes.resize(at);
                b->mpa_bytes.insert(b->mpa_bytes.end(), r.mpa_bytes.begin(), r.mpa_bytes.end());
                for (sk_mpa_frame_record rec : r.mpa_recs) {
                    rec.byte_offset += (uint32_t)at;
                    b->mpa_recs.push_back(rec);
                }
            } else if (r.mp3) {
                b->n_mp3 += r.n_frames;
                b->mp3_rows += r.mp3_is.size() / 576;
                b->n_mp3_frames += r.mp3_frames.size();
            } else {
                b->n_descs += r.n_frames;
            }
            b->n_floats += r.n_floats;
            b->au_used += r.n_au_bytes;
            sk_tick_stream t{};
            t.codec = r.mpa ? SK_TICK_MPA : (r.mp3 ? SK_TICK_MP3 : SK_TICK_AAC);
            t.stream = s.engine_stream == kNoStream ? 0 : s.engine_stream;
            t.n_frames = r.n_frames;
            t.out_bits = s.opt.output_bits_per_sample ? s.opt.output_bits_per_sample : 16;
            t.out_channels = s.opt.output_channels ? s.opt.output_channels : s.channels;
            t.resample = s.resample ? 1 : 0;
            t.flush = (r.eof && s.resample) ? 1 : 0;
            BatchEntry be;
            be.handle = handle;
            be.eof = r.eof;
            be.failed = r.failed;
            be.fail_status = r.fail_status;
            be.fail_msg = std::move(r.fail_msg);
            be.raw = std::move(r.raw);
            be.raw_len = std::move(r.raw_len);
            if (r.pcm) {  // no row in the AAC / MP3 tick; a row of the PCM tick when it brings units or ends a resampler
                be.pcm = true;
                be.pre = std::move(r.pre);
                t.n_frames = 0;
                t.flush = 0;
                if (s.pcm_route == kPcmAiffTick) {
                    if (sk_aiff_tick_stream *row = claim_tick_row(b, b->aiff_ts, s, r, r.pcm_units, be, pcm_at)) row->encoding = s.aiff_enc;
                } else if (s.pcm_route == kPcmWavAdpcmTick) {
                    if (sk_wav_adpcm_tick_stream *row = claim_tick_row(b, b->wav_ts, s, r, r.pcm_units, be, pcm_at)) {
                        row->tag = (uint16_t)s.wav->tag(), row->block_align = s.wav->block_align(), row->n_coef = (uint8_t)s.wav->n_coef();
                        std::memcpy(row->coef, s.wav->coef(), sizeof row->coef);  // (the cap joins the row on the submission thread)
                    }
                } else if (s.pcm_route == kPcmFlacTick) {
                    if (sk_flac_tick_stream *row = claim_tick_row(b, b->flac_ts, s, r, r.flac_frames, be, pcm_at)) {
                        const uint8_t depth = s.flac->info().bits_per_sample;
                        row->bits_per_sample = depth;
                        // as decoded: the contract's width (the record's depth is put back at delivery); else what the options ask for
                        if (s.flac_plain) row->out_bits = depth <= 8 ? 8 : (depth <= 16 ? 16 : (depth <= 24 ? 24 : 32));
                    }
                } else if (s.pcm_route == kPcmAlacTick) {
                    if (sk_alac_tick_stream *row = claim_tick_row(b, b->alac_ts, s, r, r.alac_packets, be, pcm_at)) {
                        const sk_alac_config &c = s.alac_cfg;
                        row->frame_length = c.frame_length, row->bit_depth = c.bit_depth, row->pb = c.pb, row->mb = c.mb, row->kb = c.kb;
                    }
                } else if (s.pcm_route == kPcmVorbisTick) {
                    (void)claim_tick_row(b, b->vorbis_ts, s, r, r.vorbis_packets, be, pcm_at);  // the carry joins the row on the submission thread
                } else if (s.pcm_route == kPcmG72xTick) {
                    if (sk_g72x_tick_stream *row = claim_tick_row(b, b->g72x_ts, s, r, r.pcm_units, be, pcm_at))
                        row->codec = s.g72x_codec, row->g726_rate = s.g726_rate, row->g726_packing = s.g726_packing;
                } else if (s.pcm_route == kPcmGsmTick) {
                    if (sk_gsm_tick_stream *row = claim_tick_row(b, b->gsm_ts, s, r, r.pcm_units, be, pcm_at)) row->variant = s.gsm_variant;
                } else if (s.pcm_route == kPcmTick) {
                    if (sk_pcm_tick_stream *row = claim_tick_row(b, b->pcm_ts, s, r, r.pcm_units, be, pcm_at)) row->format = s.pcm_fmt;
                }
            }
            if (s.engine_stream == kNoStream) {  // ended before a single header was seen: nothing for the device
                t.n_frames = 0;
                t.flush = 0;
            }
            b->ts.push_back(t);
            b->entries.push_back(std::move(be));
            b->writers += 1;
        }
        if (r.pcm) {
            if (!r.pcm_units.empty()) std::memcpy(b->pcm_bytes + pcm_at, r.pcm_bytes.data(), r.pcm_bytes.size());
        } else if (r.mpa) {  // staged under the lock above
        } else if (r.n_frames && r.mp3 && p->mp3_gpu) {
            std::memcpy(b->au_bytes + au_at, r.mp3_bytes.data(), r.n_au_bytes);
            for (size_t k = 0; k < r.mp3_frames.size(); ++k) {
                b->mp3_frames[mp3_frame_at + k] = r.mp3_frames[k];
                b->mp3_frames[mp3_frame_at + k].byte_offset += (uint32_t)au_at;
            }
        } else if (r.n_frames && r.mp3) {
            std::memcpy(b->mp3_gr.data() + mp3_at, r.mp3_gr.data(), r.n_frames * sizeof(sk_mp3_requant_granule));
            std::memcpy(b->mp3_desc.data() + mp3_at, r.mp3_desc.data(), r.n_frames * sizeof(sk_mp3_granule_desc));
            std::memcpy(b->mp3_is + mp3_row_at * 576, r.mp3_is.data(), r.mp3_is.size() * sizeof(int16_t));
        } else if (r.n_frames && gpu_entropy) {
            std::memcpy(b->au_bytes + au_at, au_stage.data(), r.n_au_bytes);
            for (uint32_t k = 0; k < r.n_frames; ++k)
                b->units[desc_at + k] = sk_au_item{(uint32_t)(au_at + au_items[k].byte_offset), au_items[k].byte_len};
        } else if (r.n_frames && quant) {
            std::memcpy(b->descs.data() + desc_at, descs.data(), r.n_frames * sizeof(sk_aac_frame_desc));
            std::memcpy(reinterpret_cast<int16_t *>(b->coeffs) + float_at, coeffs.data(), r.n_floats * sizeof(int16_t));
            std::memcpy(b->au_bytes + au_at, au_stage.data(), r.n_au_bytes);
        } else if (r.n_frames) {
            std::memcpy(b->descs.data() + desc_at, descs.data(), r.n_frames * sizeof(sk_aac_frame_desc));
            std::memcpy(b->coeffs + float_at, coeffs.data(), r.n_floats * sizeof(float));
        }
        {
            std::lock_guard<std::mutex> lk(p->batch_mu);
            b->writers -= 1;
        }
        p->batch_cv.notify_one();  // only the submission thread waits on it
    }
}

void push_error(PStream &s, int32_t status, const std::string &msg) {
    Output o;
    o.is_error = true;
    o.status = status;
    o.data.assign(msg.begin(), msg.end());
    s.out.push_back(std::move(o));
}

// What the main tick's mixed forms take beside the table: the AAC units in the lane's form (all null without units), the MP3 streams'
// granules from the host's Huffman stage -- or, with that stage in the tick (with_md), the bytes their frames point into
sk_tick_input tick_input(const sk_lane *p, const Batch *b, uint32_t n_frames, bool with_md) {
    sk_tick_input in{};
    in.n_aac_units = n_frames;
    if (p->cfg.gpu_entropy == 2) in.descs = b->descs.data(), in.q_sides = b->au_bytes, in.q_quant = reinterpret_cast<const int16_t *>(b->coeffs);
    else if (p->cfg.gpu_entropy) in.units = b->units.data(), in.au_bytes = b->au_bytes, in.au_bytes_len = b->au_used + 8;
    else in.descs = b->descs.data(), in.coeffs = b->coeffs;
    if (n_frames == 0) in.descs = nullptr, in.coeffs = nullptr, in.units = nullptr, in.q_sides = nullptr;
    if (with_md) {
        in.au_bytes = b->au_bytes, in.au_bytes_len = b->au_used + 8;
    } else if (b->n_mp3) {
        in.n_mp3_granules = (uint32_t)b->n_mp3;
        in.mp3_granules = b->mp3_gr.data(), in.mp3_descs = b->mp3_desc.data(), in.mp3_is = b->mp3_is;
    }
    return in;
}

// The main tick's table with the Huffman stage in the tick: an MP3 stream's units are frames there (ts keeps counting granules: the
// budget and the output bound are in granules)
void frames_form(const Batch *b, const std::vector<sk_tick_stream> &ts, std::vector<sk_tick_stream> &ts_md) {
    ts_md = ts;
    for (size_t row = 0; row < ts_md.size(); ++row)
        if (ts_md[row].codec == SK_TICK_MP3) ts_md[row].n_frames = b->mp3_frames_of[b->row_of[row]];
}

// A PCM-family tick's share of the output buffer: 16 bytes for the alignment of its base plus the tick's own bound; the records it may
// write stay with the table
template <class Table, class Bound>
size_t follow_on_bound(sk_lane *p, Table &t, Bound out_bound) {
    if (t.rows.empty()) return 0;
    return 16 + out_bound(p->engine, t.rows.data(), (uint32_t)t.rows.size(), t.units.data(), (uint32_t)t.units.size(), &t.max_out);
}

// One PCM-family tick of a round, behind whatever ran before it: its outputs follow the others' in the same buffer from the next
// 16-byte aligned offset, its records in the same array, and its rows number on from theirs.  `run` calls the hook with the place
// for both; a failure (this tick's or an earlier one's) leaves the batch as it is, with the status in b->rc.
template <class Table, class Run>
void follow_on_tick(Batch *b, const Table &t, size_t &used, Run run) {
    if (b->rc != SK_OK || t.rows.empty()) return;
    const uint32_t first_row = (uint32_t)b->row_of.size();
    const size_t base = (used + 15) & ~(size_t)15;
    uint32_t n_out = 0;
    size_t tick_used = 0;
    b->rc = run(b->out_pinned + base, b->out_pinned_cap - base, b->recs.data() + b->n_out, t.max_out, &n_out, &tick_used);
    if (b->rc != SK_OK) return;
    for (uint32_t k = 0; k < n_out; ++k) {
        b->recs[b->n_out + k].stream_index += first_row;
        b->recs[b->n_out + k].byte_offset += base;
    }
    b->n_out += n_out;
    for (uint32_t row = 0; row < t.entry.size(); ++row) {
        b->entry_row[t.entry[row]] = first_row + row;
        b->row_of.push_back(t.entry[row]);
    }
    used = base + tick_used;
}

void submit_body(sk_lane *p) {
    const sk_mp3_internal::PipelineGpuHooks &hooks = sk_mp3_internal::pipeline_gpu_hooks();
    std::vector<sk_tick_stream> ts, ts_md;
    for (;;) {
        Batch *b;
        int index;
        {
            std::unique_lock<std::mutex> lk(p->batch_mu);
            const Clock::time_point t_idle = Clock::now();
            p->submit_where = 0;
            p->batch_cv.wait(lk, [&] { return p->stop || !p->batches[p->filling].ts.empty(); });
            if (p->stop) return;
            p->submit_where = 1;
            // let the batch fill for a moment unless it is already full
            // (system_clock deadline: pthread_cond_timedwait, which every sanitizer runtime understands)
            const auto deadline = std::chrono::system_clock::now() + std::chrono::microseconds(p->cfg.tick_wait_us);
            p->batch_cv.wait_until(lk, deadline, [&] {
                return p->stop || p->batches[p->filling].n_descs + p->cfg.max_stream_frames_per_tick > p->cfg.max_frames_per_tick;
            });
            // the workers move on to a free batch while this one runs
            p->submit_where = 2;
            p->batch_cv.wait(lk, [&] { return p->stop || (p->batches[p->filling].writers == 0 && !p->free_batches.empty()); });
            if (p->stop) return;
            p->submit_where = 3;
            p->idle_ns.fetch_add(ns_since(t_idle));
            index = p->filling;
            b = &p->batches[index];
            p->filling = p->free_batches.front();
            p->free_batches.pop_front();
        }
        p->room_cv.notify_all();  // room again
        thread_debug_point(2);

        const Clock::time_point t0 = Clock::now();
        const uint32_t n_streams = (uint32_t)b->ts.size(), n_frames = (uint32_t)b->n_descs;
        // a stream may have ended without ever reaching the device: it gets no row in the tick's table
        ts.clear();
        b->row_of.clear();
        b->entry_row.assign(n_streams, kNoStream);
        for (uint32_t i = 0; i < n_streams; ++i) {
            PStream &s = *p->streams[b->entries[i].handle];
            if (s.engine_stream == kNoStream || b->entries[i].pcm) continue;
            ts.push_back(b->ts[i]);
            b->entry_row[i] = (uint32_t)b->row_of.size();
            b->row_of.push_back(i);
        }
        uint32_t max_out = 0;
        size_t used = 0;
        b->rc = SK_OK;
        b->n_out = 0;
        if (!ts.empty() || !b->pcm_ts.rows.empty() || !b->aiff_ts.rows.empty() || !b->wav_ts.rows.empty() || !b->flac_ts.rows.empty() || !b->alac_ts.rows.empty() ||
            !b->g72x_ts.rows.empty() || !b->gsm_ts.rows.empty() || !b->vorbis_ts.rows.empty()) {
            // the Vorbis streams' carry as the ticks before this one left it (this thread alone reads and writes it): the bound needs it too
            for (uint32_t row = 0; row < b->vorbis_ts.rows.size(); ++row) {
                PStream &s = *p->streams[b->entries[b->vorbis_ts.entry[row]].handle];
                sk_vorbis_tick_stream &v = b->vorbis_ts.rows[row];
                v.setup = s.vorbis_setup.get(), v.overlap = s.vorbis_overlap.data(), v.prev_blocksize = s.vorbis_prev;
            }
            // the WAV ADPCM streams' fact cap likewise: a unit it cuts is that much shorter
            for (uint32_t row = 0; row < b->wav_ts.rows.size(); ++row)
                b->wav_ts.rows[row].frames_left = p->streams[b->entries[b->wav_ts.entry[row]].handle]->wav_tick_left;
            // the main tick's outputs, the AIFF tick's behind those, then the FLAC tick's, the ALAC tick's, then the PCM tick's: one buffer
            const size_t bound = (ts.empty() ? 0 : sk_tick_out_bound_on(p->engine, ts.data(), (uint32_t)ts.size(), &max_out)) +
                                 follow_on_bound(p, b->aiff_ts, hooks.tick_aiff_out_bound) + follow_on_bound(p, b->wav_ts, hooks.tick_wav_adpcm_out_bound) +
                                 follow_on_bound(p, b->flac_ts, hooks.tick_flac_out_bound) +
                                 follow_on_bound(p, b->alac_ts, hooks.tick_alac_out_bound) +
                                 follow_on_bound(p, b->g72x_ts, hooks.tick_g72x_out_bound) + follow_on_bound(p, b->gsm_ts, hooks.tick_gsm_out_bound) +
                                 follow_on_bound(p, b->vorbis_ts,
                                                 [&](sk_engine *e, const sk_vorbis_tick_stream *rows, uint32_t n, const sk_vorbis_tick_packet *units, uint32_t n_units,
                                                     uint32_t *most) { return hooks.tick_vorbis_out_bound(e, rows, n, units, n_units, b->pcm_bytes, b->pcm_used, most); }) +
                                 follow_on_bound(p, b->pcm_ts, hooks.tick_pcm_out_bound);
            if (bound > b->out_pinned_cap) {
                // Pinned memory is slow to get (10 ms per 64 MB on an idle device, many times that beside a running lane): the
                // bound is the engine's own (the streams' real ratios and widths, not the 8 -> 48 kHz stereo 32-bit case), with room
                // to grow into, and what one batch of the lane has needed the others ask for at once.
                const Clock::time_point t_alloc = Clock::now();
                const size_t want = std::max(bound + bound / 2, p->out_cap_seen.load());
                if (b->out_pinned) (void)hipHostFree(b->out_pinned);
                b->out_pinned = nullptr;
                b->out_pinned_cap = 0;
                if (hipHostMalloc((void **)&b->out_pinned, want, hipHostMallocPortable) == hipSuccess) {
                    b->out_pinned_cap = want;
                    p->out_cap_seen.store(want);
                } else {
                    b->rc = SK_ERR_OOM;
                }
                static const bool trace = std::getenv("SK_TICK_TRACE") != nullptr;
                if (trace) std::fprintf(stderr, "sk_pipeline: output buffer of batch %d regrown to %zu bytes in %.2f ms\n", index, b->out_pinned_cap, ns_since(t_alloc) * 1e-6);
            }
            const size_t n_recs = (size_t)max_out + b->aiff_ts.max_out + b->wav_ts.max_out + b->flac_ts.max_out + b->alac_ts.max_out + b->g72x_ts.max_out + b->gsm_ts.max_out + b->vorbis_ts.max_out + b->pcm_ts.max_out;
            if (b->recs.size() < n_recs) b->recs.resize(n_recs);
        }
        const bool with_md = b->n_mp3 && p->mp3_gpu;  // the MP3 streams' Huffman stage is the tick's as well
        if (ts.empty() || b->rc != SK_OK) {  // no row for the main tick, or no buffer for its outputs
        } else if (with_md || !b->mpa_recs.empty()) {
            // frames with main data or Layer I / II frames in this tick: the tick that takes them, with everything else in the lane's form
            const sk_tick_input in = tick_input(p, b, n_frames, with_md);
            const sk_tick_mp3_frames md{b->mp3_frames.data(), (uint32_t)b->n_mp3_frames, b->au_bytes, b->au_used + 8};
            if (with_md) {
                frames_form(b, ts, ts_md);
                // (the lane's first engine is the caller's: something else may have put its own code book there since)
                b->rc = hooks.install_codebook(p->engine, p->mp3_blob.data(), p->mp3_blob.size());
            }
            const bool with_mpa = !b->mpa_recs.empty();
            if (with_mpa) b->mpa_bytes.resize(b->mpa_bytes.size() + 8, 0);
            const sk_tick_mpa_frames mpa{b->mpa_recs.data(), (uint32_t)b->mpa_recs.size(), b->mpa_bytes.data(), b->mpa_bytes.size()};
            if (b->rc == SK_OK)
                b->rc = hooks.tick_mpa(p->engine, with_md ? ts_md.data() : ts.data(), (uint32_t)ts.size(), &in, with_md ? &md : nullptr,
                                       with_mpa ? &mpa : nullptr, b->out_pinned, b->out_pinned_cap, b->recs.data(), max_out, &b->n_out, &used);
        } else if (b->n_mp3) {  // streams of both codecs: the AAC units in the lane's form, the MP3 granules beside them
            const sk_tick_input in = tick_input(p, b, n_frames, false);
            b->rc = sk_tick_run_mixed(p->engine, ts.data(), (uint32_t)ts.size(), &in, b->out_pinned, b->out_pinned_cap, b->recs.data(), max_out, &b->n_out,
                                      &used);
        } else if (p->cfg.gpu_entropy == 2) {
            b->rc = sk_tick_run_q(p->engine, ts.data(), (uint32_t)ts.size(), b->descs.data(), b->au_bytes, reinterpret_cast<const int16_t *>(b->coeffs),
                                  n_frames, b->out_pinned, b->out_pinned_cap, b->recs.data(), max_out, &b->n_out, &used);
        } else if (p->cfg.gpu_entropy) {
            b->rc = sk_tick_run_au(p->engine, ts.data(), (uint32_t)ts.size(), b->units.data(), n_frames, b->au_bytes, b->au_used + 8, b->out_pinned,
                                   b->out_pinned_cap, b->recs.data(), max_out, &b->n_out, &used);
        } else {
            b->rc = sk_tick_run(p->engine, ts.data(), (uint32_t)ts.size(), b->descs.data(), b->coeffs, n_frames, b->out_pinned, b->out_pinned_cap,
                                b->recs.data(), max_out, &b->n_out, &used);
        }
        // the PCM-family ticks of this round, behind it: AIFF, FLAC, PCM
        follow_on_tick(b, b->aiff_ts, used, [&](uint8_t *out, size_t out_cap, sk_tick_output *recs, uint32_t recs_cap, uint32_t *n_out, size_t *out_used) {
            // the IMA4 carry of each stream as the ticks before this one left it (this thread alone reads and writes it)
            for (uint32_t row = 0; row < b->aiff_ts.rows.size(); ++row) {
                const PStream &s = *p->streams[b->entries[b->aiff_ts.entry[row]].handle];
                b->aiff_ts.rows[row].ima_state[0] = s.aiff_ima[0], b->aiff_ts.rows[row].ima_state[1] = s.aiff_ima[1];
            }
            return hooks.tick_aiff(p->engine, b->aiff_ts.rows.data(), (uint32_t)b->aiff_ts.rows.size(), b->aiff_ts.units.data(),
                                   (uint32_t)b->aiff_ts.units.size(), b->pcm_bytes, b->pcm_used, out, out_cap, recs, recs_cap, n_out, out_used);
        });
        for (uint32_t row = 0; b->rc == SK_OK && row < b->aiff_ts.rows.size(); ++row) {  // ... and as this one leaves it
            PStream &s = *p->streams[b->entries[b->aiff_ts.entry[row]].handle];
            s.aiff_ima[0] = b->aiff_ts.rows[row].ima_state[0], s.aiff_ima[1] = b->aiff_ts.rows[row].ima_state[1];
        }
        follow_on_tick(b, b->wav_ts, used, [&](uint8_t *out, size_t out_cap, sk_tick_output *recs, uint32_t recs_cap, uint32_t *n_out, size_t *out_used) {
            b->wav_status.assign(b->wav_ts.units.size() + 1, 0);  // (the worker has looked at every block header: no unit holds a bad one)
            return hooks.tick_wav_adpcm(p->engine, b->wav_ts.rows.data(), (uint32_t)b->wav_ts.rows.size(), b->wav_ts.units.data(),
                                        (uint32_t)b->wav_ts.units.size(), b->pcm_bytes, b->pcm_used, out, out_cap, recs, recs_cap, n_out, out_used,
                                        b->wav_status.data());
        });
        for (uint32_t row = 0; b->rc == SK_OK && row < b->wav_ts.rows.size(); ++row)  // the cap as this tick leaves it
            p->streams[b->entries[b->wav_ts.entry[row]].handle]->wav_tick_left = b->wav_ts.rows[row].frames_left;
        follow_on_tick(b, b->flac_ts, used, [&](uint8_t *out, size_t out_cap, sk_tick_output *recs, uint32_t recs_cap, uint32_t *n_out, size_t *out_used) {
            b->flac_status.assign(b->flac_ts.units.size() + 1, 0);
            return hooks.tick_flac(p->engine, b->flac_ts.rows.data(), (uint32_t)b->flac_ts.rows.size(), b->flac_ts.units.data(),
                                   (uint32_t)b->flac_ts.units.size(), b->pcm_bytes, b->pcm_used, out, out_cap, recs, recs_cap, n_out, out_used,
                                   b->flac_status.data());
        });
        follow_on_tick(b, b->alac_ts, used, [&](uint8_t *out, size_t out_cap, sk_tick_output *recs, uint32_t recs_cap, uint32_t *n_out, size_t *out_used) {
            b->alac_status.assign(b->alac_ts.units.size() + 1, 0);
            return hooks.tick_alac(p->engine, b->alac_ts.rows.data(), (uint32_t)b->alac_ts.rows.size(), b->alac_ts.units.data(),
                                   (uint32_t)b->alac_ts.units.size(), b->pcm_bytes, b->pcm_used, out, out_cap, recs, recs_cap, n_out, out_used,
                                   b->alac_status.data());
        });
        follow_on_tick(b, b->g72x_ts, used, [&](uint8_t *out, size_t out_cap, sk_tick_output *recs, uint32_t recs_cap, uint32_t *n_out, size_t *out_used) {
            // the codec's carry of each stream as the ticks before this one left it (this thread alone reads and writes it): row k names record k
            const uint32_t rows = (uint32_t)b->g72x_ts.rows.size();
            b->g726_states.resize(rows);
            b->g722_states.resize(rows);
            for (uint32_t row = 0; row < rows; ++row) {
                const PStream &s = *p->streams[b->entries[b->g72x_ts.entry[row]].handle];
                b->g72x_ts.rows[row].state = row;
                b->g726_states[row] = s.g726_state, b->g722_states[row] = s.g722_state;
            }
            return hooks.tick_g72x(p->engine, b->g72x_ts.rows.data(), rows, b->g72x_ts.units.data(), (uint32_t)b->g72x_ts.units.size(), b->pcm_bytes, b->pcm_used,
                                   out, out_cap, recs, recs_cap, n_out, out_used, b->g726_states.data(), rows, b->g722_states.data(), rows);
        });
        for (uint32_t row = 0; b->rc == SK_OK && row < b->g72x_ts.rows.size(); ++row) {  // ... and as this one leaves it
            PStream &s = *p->streams[b->entries[b->g72x_ts.entry[row]].handle];
            if (s.g72x_codec == SK_G726) s.g726_state = b->g726_states[row];
            if (s.g72x_codec == SK_G722) s.g722_state = b->g722_states[row];
        }
        follow_on_tick(b, b->gsm_ts, used, [&](uint8_t *out, size_t out_cap, sk_tick_output *recs, uint32_t recs_cap, uint32_t *n_out, size_t *out_used) {
            const uint32_t rows = (uint32_t)b->gsm_ts.rows.size();  // row k names record k, as above
            b->gsm_states.resize(rows);
            for (uint32_t row = 0; row < rows; ++row) {
                b->gsm_ts.rows[row].state = row;
                b->gsm_states[row] = p->streams[b->entries[b->gsm_ts.entry[row]].handle]->gsm_state;
            }
            return hooks.tick_gsm(p->engine, b->gsm_ts.rows.data(), rows, b->gsm_ts.units.data(), (uint32_t)b->gsm_ts.units.size(), b->pcm_bytes, b->pcm_used, out,
                                  out_cap, recs, recs_cap, n_out, out_used, b->gsm_states.data(), rows);
        });
        for (uint32_t row = 0; b->rc == SK_OK && row < b->gsm_ts.rows.size(); ++row)
            p->streams[b->entries[b->gsm_ts.entry[row]].handle]->gsm_state = b->gsm_states[row];
        follow_on_tick(b, b->vorbis_ts, used, [&](uint8_t *out, size_t out_cap, sk_tick_output *recs, uint32_t recs_cap, uint32_t *n_out, size_t *out_used) {
            b->vorbis_status.assign(b->vorbis_ts.units.size() + 1, 0);
            return hooks.tick_vorbis(p->engine, b->vorbis_ts.rows.data(), (uint32_t)b->vorbis_ts.rows.size(), b->vorbis_ts.units.data(),
                                     (uint32_t)b->vorbis_ts.units.size(), b->pcm_bytes, b->pcm_used, out, out_cap, recs, recs_cap, n_out, out_used,
                                     b->vorbis_status.data());
        });
        for (uint32_t row = 0; b->rc == SK_OK && row < b->vorbis_ts.rows.size(); ++row)  // the overlap half was written in place; the block size comes back
            p->streams[b->entries[b->vorbis_ts.entry[row]].handle]->vorbis_prev = b->vorbis_ts.rows[row].prev_blocksize;
        follow_on_tick(b, b->pcm_ts, used, [&](uint8_t *out, size_t out_cap, sk_tick_output *recs, uint32_t recs_cap, uint32_t *n_out, size_t *out_used) {
            return hooks.tick_pcm(p->engine, b->pcm_ts.rows.data(), (uint32_t)b->pcm_ts.rows.size(), b->pcm_ts.units.data(),
                                  (uint32_t)b->pcm_ts.units.size(), b->pcm_bytes, b->pcm_used, out, out_cap, recs, recs_cap, n_out, out_used);
        });
        p->submit_where = 4;
        p->tick_ns.fetch_add(ns_since(t0));
        p->n_ticks.fetch_add(1);
        p->n_frames.fetch_add(n_frames + (uint32_t)b->n_mp3 + (uint32_t)b->mpa_recs.size() + (uint32_t)b->pcm_ts.units.size() +
                              (uint32_t)b->aiff_ts.units.size() + (uint32_t)b->wav_ts.units.size() + (uint32_t)b->flac_ts.units.size() + (uint32_t)b->alac_ts.units.size() + (uint32_t)b->g72x_ts.units.size() + (uint32_t)b->gsm_ts.units.size() + (uint32_t)b->vorbis_ts.units.size());
        b->rec_begin.assign(b->row_of.size() + 1, b->n_out);
        {
            uint32_t k = 0;
            for (uint32_t row = 0; row < b->row_of.size(); ++row) {
                b->rec_begin[row] = k;
                while (b->rc == SK_OK && k < b->n_out && b->recs[k].stream_index == row) ++k;
            }
        }
        {
            std::lock_guard<std::mutex> lk(p->batch_mu);
            for (uint32_t d = 0; d < p->n_deliver; ++d) p->to_deliver.push_back(index);  // one slice per delivery thread
        }
        p->deliver_cv.notify_all();
    }
}

// The message behind a status the device reported for a unit of this entry.  The device reports codes; the reference's
// text comes from parsing the entry's access units of this tick once more on the host (errors are rare, and an entry holds
// at most max_stream_frames_per_tick units).
std::string device_error_text(sk_lane *p, const Batch *b, uint32_t entry, const PStream &s, int32_t status) {
    if (s.codec == kCodecAlac)
        return status == SK_ERR_UNSUPPORTED ? "Decoding failed: ALAC packet rejected: a channel pair at 32 bits without extra bytes is not supported"
               : status == SK_ALAC_UNSUPPORTED ? "Decoding failed: ALAC packet rejected: a CCE or PCE element is not supported"
                                               : "Decoding failed: ALAC packet rejected: the elements break the syntax or miss the packet's end";
    if (s.codec == kCodecVorbis) return std::string("Decoding failed: Vorbis packet rejected: ") + sk_strerror(status);
    if (s.codec == kCodecFlac)
        return status == SK_ERR_UNSUPPORTED ? "Decoding failed: FLAC frame rejected: 32-bit samples with a side channel are not supported"
                                            : "Decoding failed: FLAC frame rejected: the subframes break the syntax or miss the frame's end";
    std::string msg = "Decoding failed: invalid AAC config: frame rejected by the synthesis engine";
    if (!(p->cfg.gpu_entropy && status <= -101 && status >= -108)) return msg;
    msg = std::string("Decoding failed: ") + sk_strerror(status);  // found on the device (stereo tools, TNS) or in the unit's tail
    sk_aac_decoder *probe = nullptr;
    if (sk_aac_decoder_create(s.asc, 2, &probe) != SK_OK) return msg;
    std::vector<float> sink(2048);
    sk_aac_frame_desc d;
    if (p->cfg.gpu_entropy == 1) {
        size_t first = 0;
        for (uint32_t q = 0; q < entry; ++q) first += b->ts[q].n_frames;
        for (uint32_t u = 0; u < b->ts[entry].n_frames; ++u) {
            const sk_au_item &it = b->units[first + u];
            if (sk_aac_decoder_parse(probe, b->au_bytes + it.byte_offset, it.byte_len, sink.data(), &d) != SK_OK) {
                msg = std::string("Decoding failed: ") + sk_aac_decoder_last_error(probe);
                break;
            }
        }
    } else {  // quantised hand-over: the worker kept the pass's access units beside the entry for exactly this
        const BatchEntry &be = b->entries[entry];
        size_t at = 0;
        for (uint32_t len : be.raw_len) {
            if (sk_aac_decoder_parse(probe, be.raw.data() + at, len, sink.data(), &d) != SK_OK) {
                msg = std::string("Decoding failed: ") + sk_aac_decoder_last_error(probe);
                break;
            }
            at += len;
        }
    }
    sk_aac_decoder_destroy(probe);
    return msg;
}

void watchdog_main(sk_lane *p, int secs);

// Hands a finished tick's outputs to the streams' queues: outputs first (in order), then the end-of-stream /
// error notes, then the stream is free to be parsed again.
void deliver_body(sk_lane *p) {
    std::vector<uint32_t> wake;  // streams that can be parsed again: queued in one go, one wake-up
    std::vector<uint32_t> listed;  // handles that now have something to receive
    for (;;) {
        Batch *b;
        int index;
        uint32_t slice;
        {
            std::unique_lock<std::mutex> lk(p->batch_mu);
            p->deliverers_waiting.fetch_add(1);
            p->deliver_cv.wait(lk, [&] { return p->stop || !p->to_deliver.empty(); });
            p->deliverers_waiting.fetch_sub(1);
            if (p->stop) return;
            index = p->to_deliver.front();
            p->to_deliver.pop_front();
            b = &p->batches[index];
            slice = b->next_slice++;  // this thread serves the rows / entries congruent to `slice`
        }
        thread_debug_point(3);
        const uint32_t n_slices = p->n_deliver;
        const Clock::time_point t_deliver = Clock::now();
        const uint32_t n_streams = (uint32_t)b->ts.size();
        const int rc = b->rc;
        wake.clear();
        listed.clear();
        // One delivery thread serves an entry completely -- its outputs (the records of its tick row are contiguous), then
        // the end-of-stream / error note, then the stream is free again -- under one hold of the stream's lock.  (Rows and
        // entries used to be sliced separately: with several delivery threads a stream without a tick row in front of
        // another shifted the two numberings against each other, and that stream's end could be announced by one thread
        // before another had queued its last outputs.)
        for (uint32_t i = slice; i < n_streams; i += n_slices) {
            BatchEntry &be = b->entries[i];
            PStream &s = *p->streams[be.handle];
            const uint32_t row = b->entry_row[i];
            bool release = false, was_cancelled = false;  // was_cancelled: as seen under the lock that cleared `busy` -- a cancel that
                                                          // arrives later finds the stream idle and frees the slot itself
            {
                std::lock_guard<std::mutex> lk(s.mu);
                for (Output &o : be.pre) {  // a fast-path PCM stream's pieces, as they are
                    if (s.cancelled || s.finished) break;
                    s.out.push_back(std::move(o));
                    p->n_outputs.fetch_add(1);
                }
                be.pre.clear();
                for (uint32_t k = row == kNoStream ? 0 : b->rec_begin[row]; row != kNoStream && rc == SK_OK && k < b->rec_begin[row + 1]; ++k) {
                    const sk_tick_output &r = b->recs[k];
                    if (s.cancelled || s.finished) continue;
                    if (r.status != 0) {
                        push_error(s, r.status, device_error_text(p, b, i, s, r.status));
                        s.finished = true;
                        p->n_errors.fetch_add(1);
                        continue;
                    }
                    Output o;
                    o.rate = s.opt.output_sample_rate ? s.opt.output_sample_rate : s.rate;
                    o.frames = r.frames;
                    o.bits = s.flac_plain ? s.pcm_bits : r.bits;  // a FLAC frame as decoded: the stream's depth, in the contract's width
                    o.channels = r.channels;
                    o.flags = (r.reserved & SK_TICK_OUT_FLOAT) ? SK_AUDIO_FLOAT : 0;
                    o.data.assign(b->out_pinned + r.byte_offset, b->out_pinned + r.byte_offset + r.bytes);
                    s.out.push_back(std::move(o));
                    p->n_outputs.fetch_add(1);
                }
                if (rc != SK_OK && !s.finished && !(be.pcm && !be.pcm_row)) {
                    push_error(s, rc, std::string("Decoding failed: engine tick: ") + sk_strerror(rc));
                    s.finished = true;
                    p->n_errors.fetch_add(1);
                } else if (be.failed && !s.finished) {
                    push_error(s, be.fail_status, be.fail_msg);
                    s.finished = true;
                    p->n_errors.fetch_add(1);
                } else if (be.eof) {
                    s.finished = true;
                }
                s.busy = false;
                was_cancelled = s.cancelled;
                release = s.finished || was_cancelled;
                if (s.cancelled) {
                    s.out.clear();
                    s.in.clear();
                }
                if (!release && mark_schedulable(p, s)) wake.push_back(be.handle);
                if (!s.cancelled && !s.out_listed && (!s.out.empty() || s.finished)) {
                    s.out_listed = true;
                    listed.push_back(be.handle);
                }
                s.cv_out.notify_all();
            }
            if (release) {
                release_device_side(p, s);
                if (was_cancelled) {  // the handle was dropped while its frames were in flight: free the slot now
                    {
                        std::lock_guard<std::mutex> lk(s.mu);
                        s.open = false;
                    }
                    std::lock_guard<std::mutex> lk(p->handles_mu);
                    p->free_handles.push_back(be.handle);
                }
            }
        }
        if (!wake.empty()) {
            {
                std::lock_guard<std::mutex> lk(p->rq_mu);
                p->ready.insert(p->ready.end(), wake.begin(), wake.end());
            }
            p->rq_cv.notify_all();
        }
        if (!listed.empty()) {
            {
                std::lock_guard<std::mutex> lk(p->oq->mu);
                for (uint32_t h : listed) p->oq->ready.push_back(h * p->n_lanes + p->lane_index);
            }
            p->oq->cv.notify_all();
        }
        bool last;
        {
            std::lock_guard<std::mutex> lk(p->batch_mu);
            last = ++b->slices_done == n_slices;
            if (last) {
                b->clear();
                p->free_batches.push_back(index);
            }
        }
        if (last) p->batch_cv.notify_one();  // the submission thread may be waiting for a free batch
        p->deliver_ns.fetch_add(ns_since(t_deliver));
    }
}

// A thread of the lane that dies of an exception outside the per-stream guard (an allocation while it held a batch, say)
// cannot know which invariants it left broken, so the lane stops as a whole -- but it stops as an ERROR, not as
// std::terminate: every open stream gets the status as its last output (the reference's "an error ends the stream",
// soundkit-decoder/src/lib.rs:3131-3134, for all of the lane's streams at once), later calls on the lane return it, and the
// process lives.  Never throws.
void lane_fatal(sk_lane *p, int status) noexcept {
    int expected = 0;
    if (!p->fatal.compare_exchange_strong(expected, status)) return;  // once
    char text[320];
    std::snprintf(text, sizeof text, "Decoding failed: %s: %s", sk_strerror(status), sk::abi_message());
    for (uint32_t h = 0; h < p->streams.size(); ++h) {
        PStream &s = *p->streams[h];
        bool list = false;
        try {
            std::lock_guard<std::mutex> lk(s.mu);
            if (!s.open || s.cancelled) continue;
            if (!s.finished) {
                try {
                    push_error(s, status, text);
                } catch (...) {
                }
                s.finished = true;
                p->n_errors.fetch_add(1);
            }
            // s.busy stays: a thread that has not noticed the stop yet may still hold the stream; a cancel of such a handle
            // defers the release, and the lane's teardown (lane_destroy, after joining the threads) releases what is left
            if (!s.out_listed) s.out_listed = list = true;
            s.cv_out.notify_all();
        } catch (...) {
        }
        if (list) {
            try {
                std::lock_guard<std::mutex> lk(p->oq->mu);
                p->oq->ready.push_back(h * p->n_lanes + p->lane_index);
            } catch (...) {
            }
            p->oq->cv.notify_all();
        }
    }
    {
        std::lock_guard<std::mutex> a(p->rq_mu);  // lane_destroy's order
        std::lock_guard<std::mutex> b(p->batch_mu);
        p->stop = true;
    }
    p->rq_cv.notify_all();
    p->batch_cv.notify_all();
    p->room_cv.notify_all();
    p->deliver_cv.notify_all();
}

template <void (*Body)(sk_lane *)>
void guarded_main(sk_lane *p, const char *what) noexcept {
    try {
        Body(p);
    } catch (...) {
        lane_fatal(p, sk::abi_caught(what));
    }
}
void worker_main(sk_lane *p) { guarded_main<worker_body>(p, "entropy thread"); }
void submit_main(sk_lane *p) { guarded_main<submit_body>(p, "submission thread"); }
void deliver_main(sk_lane *p) { guarded_main<deliver_body>(p, "delivery thread"); }

// CPUs this process may actually use: the affinity mask, cut down by a cgroup v2 / v1 CPU quota when there is one
unsigned usable_cpus() {
    unsigned n = std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = (unsigned)CPU_COUNT(&set);
    double quota = 0.0;
    if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32];
        long period = 0;
        if (std::fscanf(f, "%31s %ld", q, &period) == 2 && period > 0 && std::strcmp(q, "max") != 0) quota = std::atof(q) / (double)period;
        std::fclose(f);
    } else if (FILE *g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
        long q = 0, period = 100000;
        if (std::fscanf(g, "%ld", &q) != 1) q = 0;
        std::fclose(g);
        if (FILE *h = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
            if (std::fscanf(h, "%ld", &period) != 1) period = 100000;
            std::fclose(h);
        }
        if (q > 0 && period > 0) quota = (double)q / (double)period;
    }
    if (quota >= 1.0 && quota < (double)n) n = (unsigned)quota;
    return n ? n : 1;
}

PStream *stream_of(sk_lane *p, uint32_t handle) {
    if (!p || handle >= p->streams.size()) return nullptr;
    return p->streams[handle].get();
}

}  // namespace

namespace {

int lane_create(sk_engine *e, const sk_pipeline_config *cfg, bool mp3_gpu, OutQueue *oq, uint32_t lane_index, uint32_t n_lanes, sk_lane **out) {
    if (!e || !out) return SK_ERR_INVALID_ARG;
    *out = nullptr;
    sk_lane *p = new (std::nothrow) sk_lane();
    if (!p) return SK_ERR_OOM;
    p->engine = e;
    p->oq = oq;
    p->lane_index = lane_index;
    p->n_lanes = n_lanes;
    if (cfg) p->cfg = *cfg;
    p->mp3_gpu = mp3_gpu;
    if (!p->cfg.entropy_threads) {
        const unsigned cpus = usable_cpus();  // leave room for the submission + delivery threads and the callers' own
        p->cfg.entropy_threads = cpus > 5 ? std::min(cpus - 5, 64u) : 1;
    }
    if (!p->cfg.max_streams) p->cfg.max_streams = 1024;
    // With the front-end on the GPU every access unit is a lane of its own and a tick costs about the same whatever its
    // size (the time of one unit), so ticks should be big; with the host front-end the tick is PCIe-bound and the host
    // threads want their results back soon.
    if (!p->cfg.max_frames_per_tick) p->cfg.max_frames_per_tick = p->cfg.gpu_entropy == 1 ? 65536 : 16384;
    if (!p->cfg.max_stream_frames_per_tick) p->cfg.max_stream_frames_per_tick = p->cfg.gpu_entropy == 1 ? 32 : 8;
    if (p->cfg.max_stream_frames_per_tick > p->cfg.max_frames_per_tick) p->cfg.max_stream_frames_per_tick = p->cfg.max_frames_per_tick;
    if (!p->cfg.input_buffer) p->cfg.input_buffer = 128;   // DEFAULT_INPUT_BUFFER, lib.rs:77
    if (!p->cfg.output_buffer) p->cfg.output_buffer = 16;  // DEFAULT_OUTPUT_BUFFER, lib.rs:78
    if (!p->cfg.tick_wait_us) p->cfg.tick_wait_us = p->cfg.gpu_entropy == 1 ? 2000 : 200;
    if (hipSetDevice(sk_engine_device(e)) != hipSuccess) {
        delete p;
        return SK_ERR_NO_DEVICE;
    }
    for (Batch &b : p->batches) {
        b.descs.resize(p->cfg.max_frames_per_tick);
        b.units.resize(p->cfg.max_frames_per_tick);
        hipError_t he;
        if (p->cfg.gpu_entropy == 2) {  // quantised hand-over: i16 values in the spectra's place (half of it) + one side record per unit
            b.coeff_cap = (size_t)p->cfg.max_frames_per_tick * 2 * 1024;
            b.au_cap = (size_t)p->cfg.max_frames_per_tick * SK_AAC_UNIT_SIDE_BYTES + 64;
            he = hipHostMalloc((void **)&b.coeffs, b.coeff_cap * sizeof(int16_t), hipHostMallocPortable);
            if (he == hipSuccess) he = hipHostMalloc((void **)&b.au_bytes, b.au_cap + 64, hipHostMallocPortable);
        } else if (p->cfg.gpu_entropy) {  // access units are ~0.4-0.8 KiB; 2 KiB each on average leaves room for any legal mix
            // ... and never less than one maximum-length ADTS frame (8191 bytes, padded) so that any single unit fits
            b.au_cap = std::max<size_t>((size_t)p->cfg.max_frames_per_tick * 2048, 8192 + 16) + 16384;
            p->au_pass_budget = b.au_cap;
            he = hipHostMalloc((void **)&b.au_bytes, b.au_cap + 64, hipHostMallocPortable);
        } else {
            b.coeff_cap = (size_t)p->cfg.max_frames_per_tick * 2 * 1024;
            he = hipHostMalloc((void **)&b.coeffs, b.coeff_cap * sizeof(float), hipHostMallocPortable);
        }
        if (he != hipSuccess) {
            for (Batch &x : p->batches) {
                if (x.coeffs) (void)hipHostFree(x.coeffs);
                if (x.au_bytes) (void)hipHostFree(x.au_bytes);
            }
            delete p;
            return SK_ERR_OOM;
        }
        if (b.au_bytes) std::memset(b.au_bytes, 0, b.au_cap + 64);
    }
    p->streams.resize(p->cfg.max_streams);
    for (uint32_t i = 0; i < p->cfg.max_streams; ++i) {
        p->streams[i].reset(new PStream());
        p->free_handles.push_back(p->cfg.max_streams - 1 - i);
    }
    for (int i = 1; i < sk_lane::kBatches; ++i) p->free_batches.push_back(i);
    for (uint32_t i = 0; i < p->cfg.entropy_threads; ++i) p->workers.emplace_back(worker_main, p);
    p->submitter = std::thread(submit_main, p);
    // With the front-end on the GPU the entropy threads have little to do and delivery is the busiest host stage -- and on the streams'
    // way back into the next tick: a stream is schedulable again when its outputs have been handed over.  As many delivery threads as
    // the lane has entropy threads, four at most (whole decode, 4096 streams on two lanes of four entropy threads each: 6.4 / 10.2 /
    // 10.7 / 11.3 / 11.7 M access units/s with 1 / 2 / 3 / 4 / 6 delivery threads per lane, gpurun_out/r4_ab_deliver.log).
    // With the front-end on host threads one delivery thread per three of them, three at most: MP3 (576-sample granules: many small
    // AudioData) is bound by a single delivery thread -- 2048 streams, nine entropy threads: 1.1-1.5 / 1.7-1.8 / 2.2-2.3 M granules/s
    // with 1 / 2 / 3, the single thread 0.8-0.99 busy and the run anywhere between 0.8 and 2.3 M from box to box; AAC with the host
    // front-end does not care (2.6-2.8 M access units/s with any of them; gpurun_ab/ab_mp3_deliver.sh, profiles/r04_tick_sections.md).
    p->n_deliver = p->cfg.gpu_entropy == 1 ? std::max(1u, std::min(4u, p->cfg.entropy_threads)) : std::max(1u, std::min(3u, p->cfg.entropy_threads / 3));
    if (const char *env = std::getenv("SK_PIPELINE_DELIVER_THREADS")) {  // tuning / test override
        const int n = std::atoi(env);
        if (n >= 1 && n <= 16) p->n_deliver = (uint32_t)n;
    }
    for (uint32_t d = 0; d < p->n_deliver; ++d) p->deliverers.emplace_back(deliver_main, p);
    if (const char *env = std::getenv("SK_PIPELINE_WATCHDOG")) {
        const int secs = std::atoi(env);
        if (secs > 0) p->watchdog = std::thread(watchdog_main, p, secs);
    }
    *out = p;
    return SK_OK;
}

// Where every thread of a lane stands and what the stream table looks like, as text.  Takes no lock it could wait for: the
// stream records and the queues are read under try_lock (a dump of a stuck pipeline must not get stuck itself, and the
// deques must not be read while a worker pushes to them); what could not be locked is counted as "held".
size_t lane_dump(sk_lane *p, char *buf, size_t cap) {
    size_t at = 0;
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wformat-security"  // every format below is a literal of this function
    auto put = [&](const char *fmt, auto... args) {
        if (at >= cap) return;
        const int n = std::snprintf(buf + at, cap - at, fmt, args...);
        if (n > 0) at += std::min<size_t>((size_t)n, cap - at - 1);
    };
#pragma GCC diagnostic pop
    size_t with_input = 0, busy = 0, queued = 0, out_full = 0, open = 0, more = 0, finished = 0, held = 0, with_output = 0, listed = 0,
           schedulable = 0;
    for (auto &sp : p->streams) {
        PStream &s = *sp;
        if (!s.mu.try_lock()) {
            ++held;
            continue;
        }
        if (s.open) {
            ++open;
            with_input += !s.in.empty();
            busy += s.busy;
            queued += s.queued;
            more += s.more && !s.busy;
            finished += s.finished;
            out_full += s.out.size() >= p->cfg.output_buffer;
            with_output += !s.out.empty();
            listed += s.out_listed;
            // would be scheduled if anybody asked: a non-zero count on a quiet pipeline is a lost wake-up
            schedulable += !s.busy && !s.queued && !s.finished && !s.cancelled && (!s.in.empty() || s.more) && s.out.size() < p->cfg.output_buffer;
        }
        s.mu.unlock();
    }
    put("[sk_pipeline] lane %u mode %u: ticks %llu frames %llu outputs %llu errors %llu | submitter at %d "
        "(0 idle, 1 filling, 2 waits for writers / a free batch, 3 in the tick, 4 hand-over) | workers: waiting for a stream %u, "
        "parsing %u, waiting for batch room %u of %zu | deliverers waiting %u of %u\n",
        p->lane_index, p->cfg.gpu_entropy, (unsigned long long)p->n_ticks.load(), (unsigned long long)p->n_frames.load(),
        (unsigned long long)p->n_outputs.load(), (unsigned long long)p->n_errors.load(), p->submit_where.load(),
        p->workers_waiting_ready.load(), p->workers_parsing.load(), p->workers_waiting_room.load(), p->workers.size(),
        p->deliverers_waiting.load(), p->n_deliver);
    put("    streams: open %zu (locked by others %zu) | input queued %zu | held by a worker or a tick %zu | in the ready queue %zu | "
        "stopped at the frame limit %zu | finished %zu | outputs waiting %zu, at the bound %zu, listed for wait_outputs %zu | "
        "schedulable but not queued %zu\n",
        open, held, with_input, busy, queued, more, finished, with_output, out_full, listed, schedulable);
    if (p->batch_mu.try_lock()) {
        put("    batches: filling %d, free %zu, to deliver %zu |", p->filling, p->free_batches.size(), p->to_deliver.size());
        for (int i = 0; i < sk_lane::kBatches; ++i)
            put(" [%d] streams %zu units %zu writers %u slices %u/%u |", i, p->batches[i].ts.size(), p->batches[i].n_descs, p->batches[i].writers,
                p->batches[i].slices_done, p->batches[i].next_slice);
        put("%s", "\n");
        p->batch_mu.unlock();
    } else {
        put("    batch_mu is held\n");
    }
    if (p->rq_mu.try_lock()) {
        put("    ready queue %zu\n", p->ready.size());
        p->rq_mu.unlock();
    } else {
        put("    rq_mu is held\n");
    }
    if (p->oq->mu.try_lock()) {
        put("    completion queue %zu\n", p->oq->ready.size());
        p->oq->mu.unlock();
    } else {
        put("    completion queue mutex is held\n");
    }
    const char *where = sk_engine_where(p->engine);
    put("    engine: %s\n", where ? where : "?");
    return at;
}

// SK_PIPELINE_WATCHDOG=<seconds>: prints lane_dump when no tick has finished for that long
void watchdog_main(sk_lane *p, int secs) {
    uint64_t last = p->n_ticks.load();
    int quiet = 0;
    std::vector<char> text(8192);
    for (;;) {
        for (int i = 0; i < 10; ++i) {
            std::this_thread::sleep_for(std::chrono::milliseconds(100));
            if (p->stop) return;
        }
        const uint64_t now = p->n_ticks.load();
        quiet = now == last ? quiet + 1 : 0;
        last = now;
        if (quiet < secs || quiet % secs) continue;
        lane_dump(p, text.data(), text.size());
        std::fprintf(stderr, "[sk_pipeline watchdog] no tick for %d s\n%s", quiet, text.data());
    }
}

void lane_destroy(sk_lane *p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> a(p->rq_mu);
        std::lock_guard<std::mutex> b(p->batch_mu);
        p->stop = true;
    }
    p->rq_cv.notify_all();
    p->batch_cv.notify_all();
    p->room_cv.notify_all();
    p->deliver_cv.notify_all();
    for (std::thread &t : p->workers) t.join();
    if (p->submitter.joinable()) p->submitter.join();
    for (std::thread &t : p->deliverers) t.join();
    if (p->watchdog.joinable()) p->watchdog.join();
    for (auto &s : p->streams) release_device_side(p, *s);
    for (Batch &b : p->batches) {
        if (b.coeffs) (void)hipHostFree(b.coeffs);
        if (b.au_bytes) (void)hipHostFree(b.au_bytes);
        if (b.out_pinned) (void)hipHostFree(b.out_pinned);
        if (b.mp3_is) (void)hipHostFree(b.mp3_is);
        if (b.pcm_bytes) (void)hipHostFree(b.pcm_bytes);
    }
    if (p->mp3_cb) sk_mp3_codebook_destroy(p->mp3_cb);
    delete p;
}

struct VorbisSpawn {  // sk_pipeline_spawn_vorbis_packets: the headers, parsed
    sk_vorbis::Ident ident;
    std::shared_ptr<sk_vorbis_setup> setup;
};
struct G72xSpawn {  // sk_pipeline_spawn_g711 / _g722 / _g726
    int codec;
    uint32_t sample_rate, channels, g726_rate;
    int g726_packing;
    int gsm_variant = -1;  // sk_pipeline_spawn_gsm: 0 / 1, nothing else of this record is read then
};

int lane_spawn(sk_lane *p, const sk_decode_options *opt, const sk_raw_pcm_format *raw, uint32_t *handle, bool aiff = false,
               const sk_alac_config *alac = nullptr, const G72xSpawn *g72x = nullptr, const VorbisSpawn *vorbis = nullptr, bool ts = false) {
    if (!p || !handle) return SK_ERR_INVALID_ARG;
    // RawPcmFormat::validate (raw_pcm.rs:117-125), and the sample formats there are
    if (raw && (raw->sample_rate == 0 || raw->channels == 0 || raw->format > SK_FMT_F32BE)) return SK_ERR_INVALID_ARG;
    if (const int dead = p->fatal.load()) return dead;
    sk_decode_options o{};
    if (opt) o = *opt;
    // apply_output_options' argument checks (lib.rs:3360-3376), made when the pipeline is created
    if (o.output_bits_per_sample && o.output_bits_per_sample != 16 && o.output_bits_per_sample != 24 && o.output_bits_per_sample != 32)
        return SK_ERR_UNSUPPORTED;
    uint32_t h;
    {
        std::lock_guard<std::mutex> lk(p->handles_mu);
        if (p->free_handles.empty()) return SK_ERR_CAPACITY;
        h = p->free_handles.back();
        p->free_handles.pop_back();
    }
    PStream &s = *p->streams[h];
    std::lock_guard<std::mutex> lk(s.mu);
    s.open = true;
    s.busy = s.queued = s.finished = s.cancelled = false;
    s.out_listed = false;
    s.in.clear();
    s.out.clear();
    s.opt = o;
    s.queued_bytes.store(0);
    s.pending.clear();
    s.pending_pos = 0;
    s.saw_eof = false;
    s.more = false;
    s.rate = 0;
    s.channels = 0;
    s.resample = false;
    s.codec = 0;
    s.mp3_reservoir.clear();
    s.mp3_free_format = 0;
    s.mpa_layer = 0;
    s.wav.reset();
    s.raw.reset();
    s.aiff.reset();
    s.aiff_enc = 0;
    s.wav_g711 = s.wav_adpcm = false;
    s.wav_parse_left = s.wav_tick_left = 0;
    s.flac.reset();
    s.flac_plain = false;
    s.alac = s.alac_plain = false;
    s.alac_cfg = sk_alac_config{};
    s.mp4.reset();
    s.mp4_checked = s.mp4_done = s.mp4_flac_head = false;
    s.mp4_error.clear();
    s.webm.reset();
    s.webm_routed = s.webm_done = s.webm_flac_head = false;
    s.webm_rate = s.webm_channels = 0;
    s.webm_error.clear();
    s.ts.reset();
    s.ts_routed = s.ts_done = false;
    s.ts_error.clear();
    s.avi.reset();
    s.ps.reset();
    s.cont_routed = s.cont_done = s.raw_enc = false;
    s.cont_error.clear();
    s.cont_piece.clear();
    s.cont_piece_pos = 0;
    s.aiff_plain = false;
    s.aiff_ima[0] = s.aiff_ima[1] = sk_aiff_ima_state{};
    s.raw_format = sk_raw_pcm_format{};
    s.g72x = false;
    s.g72x_codec = 0, s.g726_packing = 0, s.g72x_rate = 0, s.g726_rate = 0, s.g72x_channels = 1;
    s.g726_framer = sk_g72x::G726Framer();
    sk_g72x::init_state(&s.g726_state);
    sk_g72x::init_state(&s.g722_state);
    s.gsm = false;
    s.gsm_variant = 0;
    s.gsm_framer = sk_gsm::Framer();
    sk_gsm::init_state(&s.gsm_state);
    s.vorbis = s.vorbis_ogg = s.ogg_finished = s.vorbis_have_absgp = false;
    s.vorbis_headers = 0;
    s.ogg.reset();
    s.vorbis_ident = sk_vorbis::Ident();
    s.vorbis_setup.reset();
    s.vorbis_overlap.clear();
    s.vorbis_prev = s.vorbis_parse_prev = s.ogg_serial = 0;
    s.vorbis_absgp = 0;
    s.pcm_detected = false;
    s.pcm_route = 0, s.pcm_fmt = 0, s.pcm_flags = 0, s.pcm_bits = 0;
    s.pcm_fill = 0;
    if (raw) {  // spawn_raw_pcm_with_options (lib.rs:2475-2486): the stream has its decoder from the start and does not detect
        s.codec = kCodecRawPcm;
        s.raw_format = *raw;
        const size_t width = raw->format <= SK_FMT_S16BE ? 2 : (raw->format <= SK_FMT_S24BE ? 3 : 4);
        s.raw.reset(new sk_pcm::RawPcmStream(width * raw->channels));
    }
    if (aiff) {  // spawn_aiff_with_options (lib.rs:2714-2724): the decoder is there from the start, nothing is detected or gathered
        s.codec = kCodecAiff;
        s.aiff.reset(new sk_pcm::AiffStream());
        s.pcm_detected = true;
    }
    if (alac) {  // sk_pipeline_spawn_alac_packets: the cookie is the decoder, nothing is detected or gathered
        s.codec = kCodecAlac;
        s.alac = true;
        s.alac_cfg = *alac;
        s.pcm_detected = true;
    }
    if (vorbis) {  // sk_pipeline_spawn_vorbis_packets: the headers are the decoder, nothing is detected or gathered
        s.codec = kCodecVorbis;
        s.vorbis = true;
        s.vorbis_headers = 3;
        s.vorbis_ident = vorbis->ident;
        s.vorbis_setup = vorbis->setup;
        s.vorbis_overlap.assign((size_t)vorbis->ident.channels * (vorbis->ident.blocksize_1 / 2), 0.0f);
        s.pcm_detected = true;
    }
    if (g72x && g72x->gsm_variant >= 0) {  // spawn_gsm: the same, with GsmDecoder
        s.codec = kCodecGsm;
        s.gsm = true;
        s.gsm_variant = (uint8_t)g72x->gsm_variant;
        s.gsm_framer = sk_gsm::Framer(g72x->gsm_variant);
        s.pcm_detected = true;
    } else if (g72x) {  // spawn_g711 / spawn_g722 / spawn_g726*: the decoder is there from the start, nothing is detected or gathered
        s.codec = kCodecG72x;
        s.g72x = true;
        s.g72x_codec = (uint8_t)g72x->codec, s.g72x_rate = g72x->sample_rate, s.g72x_channels = (uint8_t)g72x->channels;
        s.g726_rate = g72x->g726_rate, s.g726_packing = (uint8_t)g72x->g726_packing;
        s.g726_framer = sk_g72x::G726Framer(sk_g72x::g726_bits(g72x->g726_rate));
        s.pcm_detected = true;
    }
    if (ts) s.codec = kCodecTs;  // sk_pipeline_spawn_mpeg_ts: nothing is detected, the demuxer finds the first sync itself
    *handle = h;
    return SK_OK;
}

int lane_send(sk_lane *p, uint32_t handle, const uint8_t *data, size_t len) {
    PStream *s = stream_of(p, handle);
    if (!s || (len && !data)) return SK_ERR_INVALID_ARG;
    if (len > kMaxInputChunkBytes) return SK_PIPE_CHUNK_TOO_LARGE;  // lib.rs:2796-2798
    if (p->fatal.load()) return SK_PIPE_CLOSED;  // the lane's threads are gone: Disconnected
    std::lock_guard<std::mutex> lk(s->mu);
    if (!s->open || s->cancelled) return SK_PIPE_CLOSED;
    if (s->finished) return SK_PIPE_CLOSED;  // the worker has ended: TrySendError::Disconnected, lib.rs:2827-2833
    if (len && s->queued_bytes.load() + len > kMaxQueuedInputBytes) return SK_PIPE_INPUT_FULL;  // lib.rs:2800-2811
    if (s->in.size() >= p->cfg.input_buffer) return SK_PIPE_INPUT_FULL;                         // lib.rs:2820-2826
    s->in.emplace_back(data, data + len);
    s->queued_bytes.fetch_add(len);
    maybe_schedule(p, *s, handle);
    return SK_OK;
}

int take_output(sk_lane *p, PStream &s, uint32_t handle, uint8_t *data, size_t cap, sk_audio_info *info) {
    // s.mu held
    if (s.out.empty()) return s.finished ? SK_PIPE_CLOSED : 0;
    Output &o = s.out.front();
    info->sampling_rate = o.rate;
    info->frames = o.frames;
    info->bytes = (uint32_t)o.data.size();
    info->bits_per_sample = o.bits;
    info->channel_count = o.channels;
    info->is_error = o.is_error ? 1 : 0;
    info->reserved = o.flags;
    info->status = o.status;
    if (o.data.size() > cap) return SK_ERR_CAPACITY;
    if (!o.data.empty()) std::memcpy(data, o.data.data(), o.data.size());
    s.out.pop_front();
    maybe_schedule(p, s, handle);
    if (!s.out_listed && (!s.out.empty() || s.finished)) {  // a waiter that stops early hears about the rest again
        s.out_listed = true;
        {
            std::lock_guard<std::mutex> lk(p->oq->mu);
            p->oq->ready.push_back(handle * p->n_lanes + p->lane_index);
        }
        p->oq->cv.notify_one();
    }
    return 1;
}

int lane_try_recv(sk_lane *p, uint32_t handle, uint8_t *data, size_t cap, sk_audio_info *info) {
    PStream *s = stream_of(p, handle);
    if (!s || !info || (cap && !data)) return SK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(s->mu);
    if (!s->open || s->cancelled) return SK_PIPE_CLOSED;
    return take_output(p, *s, handle, data, cap, info);
}

int lane_recv(sk_lane *p, uint32_t handle, uint8_t *data, size_t cap, sk_audio_info *info, uint32_t timeout_ms) {
    PStream *s = stream_of(p, handle);
    if (!s || !info || (cap && !data)) return SK_ERR_INVALID_ARG;
    std::unique_lock<std::mutex> lk(s->mu);
    if (!s->open || s->cancelled) return SK_PIPE_CLOSED;
    s->cv_out.wait_until(lk, std::chrono::system_clock::now() + std::chrono::milliseconds(timeout_ms),
                         [&] { return !s->out.empty() || s->finished || s->cancelled; });
    if (s->cancelled) return SK_PIPE_CLOSED;
    return take_output(p, *s, handle, data, cap, info);
}

int lane_cancel(sk_lane *p, uint32_t handle) {  // shutdown(), lib.rs:2868-2881: also what Drop does
    PStream *s = stream_of(p, handle);
    if (!s) return SK_ERR_INVALID_ARG;
    bool release_now = false;
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (!s->open || s->cancelled) return SK_PIPE_CLOSED;
        s->cancelled = true;
        s->in.clear();
        s->out.clear();
        s->queued_bytes.store(0);
        release_now = !s->busy;  // otherwise the submission thread frees it when its batch has been delivered
        if (release_now) s->open = false;
        s->cv_out.notify_all();
    }
    if (release_now) {
        release_device_side(p, *s);
        std::lock_guard<std::mutex> lk(p->handles_mu);
        p->free_handles.push_back(handle);
    }
    return SK_OK;
}

size_t lane_queued_input_bytes(sk_lane *p, uint32_t handle) {  // lib.rs:2863-2866
    PStream *s = stream_of(p, handle);
    return s ? s->queued_bytes.load() : 0;
}

int lane_get_stats(sk_lane *p, sk_pipeline_stats *out) {
    if (!p || !out) return SK_ERR_INVALID_ARG;
    out->ticks = p->n_ticks.load();
    out->frames = p->n_frames.load();
    out->outputs = p->n_outputs.load();
    out->errors = p->n_errors.load();
    out->parse_ns = p->parse_ns.load();
    out->tick_ns = p->tick_ns.load();
    out->idle_ns = p->idle_ns.load();
    out->deliver_ns = p->deliver_ns.load();
    out->entropy_threads = p->cfg.entropy_threads;
    out->lanes = 1;
    return SK_OK;
}

}  // namespace

struct sk_wav_reader {
    sk_pcm::WavStream stream;
    std::string error;
};
struct sk_wav_coded_reader {
    sk_pcm::WavStream stream{true};
    std::string error;
};
struct sk_aiff_reader {
    sk_pcm::AiffStream stream;
    std::string error;
};
struct sk_raw_pcm_framer {
    explicit sk_raw_pcm_framer(uint32_t bytes_per_frame) : stream(bytes_per_frame) {}
    sk_pcm::RawPcmStream stream;
    std::string error;
};

// ---- the pipeline: lanes behind one handle space ---------------------------------------------------------------
struct sk_pipeline {
    std::vector<sk_lane *> lanes;
    std::vector<sk_engine *> owned_engines;  // lanes 1.. run on engines of their own, on the device of the caller's engine
    // one completion queue per lane: a thread in sk_pipeline_wait_outputs waits on "its" lane's queue (threads are dealt
    // out over the lanes as they first call) and sweeps the others, so consumer threads do not meet on one mutex; one
    // consumer alone still serves every lane, at worst a millisecond late
    std::vector<std::unique_ptr<OutQueue>> oqs;
    std::atomic<uint32_t> next_lane{0}, next_waiter{0};
};

namespace {
inline sk_lane *lane_of(sk_pipeline *p, uint32_t handle, uint32_t *inner) {
    if (!p || p->lanes.empty()) return nullptr;
    const uint32_t n = (uint32_t)p->lanes.size();
    *inner = handle / n;
    return p->lanes[handle % n];
}

int pipeline_spawn(sk_pipeline *p, const sk_decode_options *opt, const sk_raw_pcm_format *raw, uint32_t *handle, bool aiff = false,
                   const sk_alac_config *alac = nullptr, const G72xSpawn *g72x = nullptr, const VorbisSpawn *vorbis = nullptr, bool ts = false) {
    if (!p || !handle || p->lanes.empty()) return SK_ERR_INVALID_ARG;
    const uint32_t n = (uint32_t)p->lanes.size();
    const uint32_t first = p->next_lane.fetch_add(1) % n;
    int rc = SK_ERR_CAPACITY;
    for (uint32_t k = 0; k < n; ++k) {  // round robin; a full lane passes the stream on
        const uint32_t li = (first + k) % n;
        uint32_t inner = 0;
        rc = lane_spawn(p->lanes[li], opt, raw, &inner, aiff, alac, g72x, vorbis, ts);
        if (rc == SK_OK) {
            *handle = inner * n + li;
            return SK_OK;
        }
        if (rc != SK_ERR_CAPACITY) return rc;
    }
    return rc;
}
}  // namespace

extern "C" {

int sk_pipeline_create(sk_engine *e, const sk_pipeline_config *cfg, sk_pipeline **out) try {
    sk::abi_enter();
    if (!e || !out) return SK_ERR_INVALID_ARG;
    *out = nullptr;
    sk_pipeline_config c{};
    if (cfg) c = *cfg;
    // gpu_entropy = 3 is 1 for the AAC streams, plus the MP3 streams' Huffman stage in the tick; SK_PIPELINE_MP3_GPU_ENTROPY=1 makes a
    // pipeline created with 1 one of those (read once)
    static const bool mp3_gpu_env = [] {
        const char *v = std::getenv("SK_PIPELINE_MP3_GPU_ENTROPY");
        return v && v[0] == '1';
    }();
    const bool mp3_gpu = c.gpu_entropy == 3 || (c.gpu_entropy == 1 && mp3_gpu_env);
    if (mp3_gpu) {
        const sk_mp3_internal::PipelineGpuHooks &hooks = sk_mp3_internal::pipeline_gpu_hooks();
        if (!hooks.tick_mpa || !hooks.install_codebook) return SK_ERR_UNSUPPORTED;  // built without the device stage
        c.gpu_entropy = 1;
    }
    // A stream hands a tick at most `max_stream_frames_per_tick` units and is not scheduled again until that tick has been delivered, so
    // with N streams a tick carries well under N times that: the quota decides how full the ticks are, and a tick costs ~2 ms of waits
    // and launches whatever its size.  With the GPU front-end (where the host threads only frame) the default is 32 units -- two
    // resampler rounds of four chunks; the output queue of a resampling stream has room for 64.  Whole decode, 4096 streams, one
    // lane (gpurun_out/r4_ab_quota*.log): quota 16: 5.6-5.9 M access units/s; 24: 7.3-7.7 M; 32: 7.5-8.3 M; 48: 8.5-9.5 M.
    // TWO lanes (engines) when every lane can still fill a whole tick from its own streams: one lane plans, uploads and delivers
    // while the other's tick has the device (8.2 M on one lane, 11.3 M on two, quota 32).  The engines of a device take TURNS with
    // their ticks' device work (engine.cpp, g_device_turn): two ticks on the device at the same time measured no faster (9.6-10.2 M)
    // and delivered short bursts of slightly wrong samples in a third of the streams (profiles/r04_lanes_corruption.md).  With the
    // host front-end the host threads are the limit and a second lane only splits them.
    if (!c.max_streams) c.max_streams = 1024;
    const uint32_t tick_frames = c.max_frames_per_tick ? c.max_frames_per_tick : (c.gpu_entropy == 1 ? 65536u : 16384u);
    const uint32_t stream_frames = c.max_stream_frames_per_tick ? c.max_stream_frames_per_tick : (c.gpu_entropy == 1 ? 32u : 8u);
    const uint32_t streams_per_tick = std::max(1u, tick_frames / std::max(1u, stream_frames));
    uint32_t n_lanes = c.lanes ? c.lanes : ((c.gpu_entropy == 1 && c.max_streams >= 2 * streams_per_tick) ? 2u : 1u);
    if (n_lanes > 8) return SK_ERR_INVALID_ARG;
    if (n_lanes > c.max_streams) n_lanes = c.max_streams;
    if (!c.entropy_threads) {
        const unsigned cpus = usable_cpus();  // leave room for the submission + delivery threads and the callers' own
        c.entropy_threads = cpus > 5 ? std::min(cpus - 5, 64u) : 1;
    }
    sk_pipeline *p = new (std::nothrow) sk_pipeline();
    if (!p) return SK_ERR_OOM;
    sk_pipeline_config lane_cfg = c;
    lane_cfg.lanes = 1;
    lane_cfg.max_streams = (c.max_streams + n_lanes - 1) / n_lanes;
    lane_cfg.entropy_threads = std::max(1u, c.entropy_threads / n_lanes);
    int rc = SK_OK;
    for (uint32_t i = 0; i < n_lanes && rc == SK_OK; ++i) {
        sk_engine *le = e;
        if (i > 0) {
            rc = sk_engine_create(sk_engine_device(e), std::max(lane_cfg.max_streams, 16u), &le);
            if (rc != SK_OK) break;
            p->owned_engines.push_back(le);
            // the lanes' own engines inherit the caller's pool of wide PCM streams
            const sk_mp3_internal::PipelineGpuHooks &hooks = sk_mp3_internal::pipeline_gpu_hooks();
            if (const uint32_t wide = hooks.wide_pcm_streams && hooks.enable_wide_pcm ? hooks.wide_pcm_streams(e) : 0) {
                rc = hooks.enable_wide_pcm(le, std::min(wide, sk_engine_max_streams(le)));
                if (rc != SK_OK) break;
            }
        }
        sk_lane *lane = nullptr;
        p->oqs.emplace_back(new OutQueue());
        rc = lane_create(le, &lane_cfg, mp3_gpu, p->oqs.back().get(), i, n_lanes, &lane);
        if (rc == SK_OK) p->lanes.push_back(lane);
    }
    if (rc != SK_OK) {
        sk_pipeline_destroy(p);
        return rc;
    }
    *out = p;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_pipeline_create");
}

void sk_pipeline_destroy(sk_pipeline *p) try {
    sk::abi_enter();
    if (!p) return;
    for (auto &q : p->oqs) {
        {
            std::lock_guard<std::mutex> lk(q->mu);
            q->stop = true;
        }
        q->cv.notify_all();
    }
    if (std::getenv("SK_PIPELINE_TRACE"))
        for (sk_lane *l : p->lanes)
            std::fprintf(stderr, "[sk_pipeline] lane %u: ticks %llu frames %llu tick_ms %.1f idle_ms %.1f deliver_ms %.1f parse_ms %.1f\n", l->lane_index,
                         (unsigned long long)l->n_ticks.load(), (unsigned long long)l->n_frames.load(), l->tick_ns.load() / 1e6,
                         l->idle_ns.load() / 1e6, l->deliver_ns.load() / 1e6, l->parse_ns.load() / 1e6);
    for (sk_lane *l : p->lanes) lane_destroy(l);
    for (sk_engine *e : p->owned_engines) sk_engine_destroy(e);
    delete p;
} catch (...) {
    (void)sk::abi_caught("sk_pipeline_destroy");
}

int sk_pipeline_spawn(sk_pipeline *p, const sk_decode_options *opt, uint32_t *handle) try {
    sk::abi_enter();
    return pipeline_spawn(p, opt, nullptr, handle);
} catch (...) {
    return sk::abi_caught("sk_pipeline_spawn");
}

int sk_pipeline_spawn_raw_pcm(sk_pipeline *p, const sk_raw_pcm_format *format, const sk_decode_options *opt, uint32_t *handle) try {
    sk::abi_enter();
    if (!format) return SK_ERR_INVALID_ARG;
    return pipeline_spawn(p, opt, format, handle);
} catch (...) {
    return sk::abi_caught("sk_pipeline_spawn_raw_pcm");
}

int sk_pipeline_spawn_mpeg_ts(sk_pipeline *p, const sk_decode_options *opt, uint32_t *handle) try {
    sk::abi_enter();
    return pipeline_spawn(p, opt, nullptr, handle, false, nullptr, nullptr, nullptr, true);
} catch (...) {
    return sk::abi_caught("sk_pipeline_spawn_mpeg_ts");
}

int sk_pipeline_spawn_aiff(sk_pipeline *p, const sk_decode_options *opt, uint32_t *handle) try {
    sk::abi_enter();
    return pipeline_spawn(p, opt, nullptr, handle, true);
} catch (...) {
    return sk::abi_caught("sk_pipeline_spawn_aiff");
}

int sk_pipeline_spawn_alac_packets(sk_pipeline *p, const uint8_t *cookie, size_t cookie_len, const sk_decode_options *opt, uint32_t *handle) try {
    sk::abi_enter();
    if (cookie_len && !cookie) return SK_ERR_INVALID_ARG;
    sk_alac_config cfg{};
    std::string text;
    if (!sk_alac::parse_cookie(cookie, cookie_len, &cfg, &text)) return SK_ALAC_ERR_STREAM;
    return pipeline_spawn(p, opt, nullptr, handle, false, &cfg);
} catch (...) {
    return sk::abi_caught("sk_pipeline_spawn_alac_packets");
}

int sk_pipeline_spawn_vorbis_packets(sk_pipeline *p, const uint8_t *ident, size_t ident_len, const uint8_t *comment, size_t comment_len, const uint8_t *setup,
                                     size_t setup_len, const sk_decode_options *opt, uint32_t *handle, char *error, size_t error_cap) try {
    sk::abi_enter();
    if ((ident_len && !ident) || (comment_len && !comment) || (setup_len && !setup)) return SK_ERR_INVALID_ARG;
    if (error && error_cap) error[0] = 0;
    VorbisSpawn v;
    v.setup = std::make_shared<sk_vorbis_setup>();
    std::string text;
    int rc = sk_vorbis::parse_ident(ident, ident_len, &v.ident, &text);
    if (rc == SK_OK) rc = sk_vorbis::parse_comment(comment, comment_len, &text);
    if (rc == SK_OK) rc = sk_vorbis::parse_setup(setup, setup_len, v.ident, &v.setup->setup, &text);
    if (rc != SK_OK) {
        if (error && error_cap) {
            const size_t n = std::min(error_cap - 1, text.size());
            std::memcpy(error, text.data(), n);
            error[n] = 0;
        }
        return rc;
    }
    return pipeline_spawn(p, opt, nullptr, handle, false, nullptr, nullptr, &v);
} catch (...) {
    return sk::abi_caught("sk_pipeline_spawn_vorbis_packets");
}

int sk_pipeline_spawn_g711(sk_pipeline *p, int law, uint32_t sample_rate, uint32_t channels, const sk_decode_options *opt, uint32_t *handle, char *error,
                           size_t error_cap) try {
    sk::abi_enter();
    if (error && error_cap) error[0] = 0;
    if (law != SK_G711_ULAW && law != SK_G711_ALAW) return SK_ERR_INVALID_ARG;
    std::string text;
    if (!sk_g72x::check_g711(sample_rate, channels, &text)) {  // DecodeError::InvalidInputFormat
        if (error && error_cap) {
            const size_t n = std::min(error_cap - 1, text.size());
            std::memcpy(error, text.data(), n);
            error[n] = 0;
        }
        return SK_G72X_ERR_STREAM;
    }
    if (channels > 255) return SK_ERR_INVALID_ARG;  // the reference's channel count is a u8
    const G72xSpawn g{law, sample_rate, channels, 0, 0};
    return pipeline_spawn(p, opt, nullptr, handle, false, nullptr, &g);
} catch (...) {
    return sk::abi_caught("sk_pipeline_spawn_g711");
}

int sk_pipeline_spawn_g722(sk_pipeline *p, const sk_decode_options *opt, uint32_t *handle) try {
    sk::abi_enter();
    const G72xSpawn g{SK_G722, 16000, 1, 0, 0};
    return pipeline_spawn(p, opt, nullptr, handle, false, nullptr, &g);
} catch (...) {
    return sk::abi_caught("sk_pipeline_spawn_g722");
}

int sk_pipeline_spawn_g726(sk_pipeline *p, uint32_t g726_rate, int g726_packing, const sk_decode_options *opt, uint32_t *handle) try {
    sk::abi_enter();
    if (!sk_g72x::g726_bits(g726_rate) || (g726_packing != SK_G726_LEFT && g726_packing != SK_G726_RIGHT)) return SK_ERR_INVALID_ARG;
    const G72xSpawn g{SK_G726, 8000, 1, g726_rate, g726_packing};
    return pipeline_spawn(p, opt, nullptr, handle, false, nullptr, &g);
} catch (...) {
    return sk::abi_caught("sk_pipeline_spawn_g726");
}

int sk_pipeline_spawn_gsm(sk_pipeline *p, int variant, const sk_decode_options *opt, uint32_t *handle) try {
    sk::abi_enter();
    if (!sk_gsm::variant_ok(variant)) return SK_ERR_INVALID_ARG;
    const G72xSpawn g{0, 8000, 1, 0, 0, variant};
    return pipeline_spawn(p, opt, nullptr, handle, false, nullptr, &g);
} catch (...) {
    return sk::abi_caught("sk_pipeline_spawn_gsm");
}

int sk_pipeline_send(sk_pipeline *p, uint32_t handle, const uint8_t *data, size_t len) try {
    sk::abi_enter();
    uint32_t inner;
    sk_lane *l = lane_of(p, handle, &inner);
    return l ? lane_send(l, inner, data, len) : SK_ERR_INVALID_ARG;
} catch (...) {
    return sk::abi_caught("sk_pipeline_send");
}

int sk_pipeline_finish(sk_pipeline *p, uint32_t handle) try {
    sk::abi_enter();
    return sk_pipeline_send(p, handle, nullptr, 0);
} catch (...) {
    return sk::abi_caught("sk_pipeline_finish");
}  // lib.rs:2838-2840

int sk_pipeline_try_recv(sk_pipeline *p, uint32_t handle, uint8_t *data, size_t cap, sk_audio_info *info) try {
    sk::abi_enter();
    uint32_t inner;
    sk_lane *l = lane_of(p, handle, &inner);
    return l ? lane_try_recv(l, inner, data, cap, info) : SK_ERR_INVALID_ARG;
} catch (...) {
    return sk::abi_caught("sk_pipeline_try_recv");
}

int sk_pipeline_recv(sk_pipeline *p, uint32_t handle, uint8_t *data, size_t cap, sk_audio_info *info, uint32_t timeout_ms) try {
    sk::abi_enter();
    uint32_t inner;
    sk_lane *l = lane_of(p, handle, &inner);
    return l ? lane_recv(l, inner, data, cap, info, timeout_ms) : SK_ERR_INVALID_ARG;
} catch (...) {
    return sk::abi_caught("sk_pipeline_recv");
}

int sk_pipeline_cancel(sk_pipeline *p, uint32_t handle) try {
    sk::abi_enter();
    uint32_t inner;
    sk_lane *l = lane_of(p, handle, &inner);
    return l ? lane_cancel(l, inner) : SK_ERR_INVALID_ARG;
} catch (...) {
    return sk::abi_caught("sk_pipeline_cancel");
}

int sk_pipeline_wait_outputs(sk_pipeline *p, uint32_t *handles, uint32_t cap, uint32_t timeout_ms) try {
    sk::abi_enter();
    if (!p || !handles || !cap || p->oqs.empty()) return SK_ERR_INVALID_ARG;
    const uint32_t n_q = (uint32_t)p->oqs.size();
    thread_local uint32_t waiter_id = 0xffffffffu;
    if (waiter_id == 0xffffffffu) waiter_id = p->next_waiter.fetch_add(1);
    const uint32_t home = waiter_id % n_q;
    const auto deadline = std::chrono::system_clock::now() + std::chrono::milliseconds(timeout_ms);
    uint32_t n = 0;
    for (;;) {
        bool stopped = false;
        for (uint32_t k = 0; k < n_q && n < cap; ++k) {  // the home queue first, then whatever the others hold
            OutQueue &q = *p->oqs[(home + k) % n_q];
            std::unique_lock<std::mutex> lk(q.mu, std::defer_lock);
            if (k == 0) lk.lock();
            else if (!lk.try_lock()) continue;
            stopped = stopped || q.stop;
            while (n < cap && !q.ready.empty()) {
                handles[n++] = q.ready.front();
                q.ready.pop_front();
            }
        }
        if (n || stopped) break;
        const auto now = std::chrono::system_clock::now();
        if (now >= deadline) break;
        OutQueue &q = *p->oqs[home];
        std::unique_lock<std::mutex> lk(q.mu);
        // with several lanes the wait is cut into millisecond slices so that a lone consumer also sees the other lanes
        const auto until = n_q > 1 ? std::min(deadline, now + std::chrono::milliseconds(1)) : deadline;
        q.cv.wait_until(lk, until, [&] { return q.stop || !q.ready.empty(); });
    }
    for (uint32_t i = 0; i < n; ++i) {  // handed out: the next delivery (or a partial drain) lists the handle again
        uint32_t inner;
        sk_lane *l = lane_of(p, handles[i], &inner);
        PStream *s = stream_of(l, inner);
        if (!s) continue;
        std::lock_guard<std::mutex> lk(s->mu);
        s->out_listed = false;
    }
    return (int)n;
} catch (...) {
    return sk::abi_caught("sk_pipeline_wait_outputs");
}

size_t sk_pipeline_debug_dump(sk_pipeline *p, char *buf, size_t cap) try {
    sk::abi_enter();
    if (!p || !buf || !cap) return 0;
    size_t at = 0;
    buf[0] = 0;
    for (sk_lane *l : p->lanes)
        if (at + 1 < cap) at += lane_dump(l, buf + at, cap - at);
    return at;
} catch (...) {
    (void)sk::abi_caught("sk_pipeline_debug_dump");
    return 0;
}

size_t sk_pipeline_queued_input_bytes(sk_pipeline *p, uint32_t handle) try {
    sk::abi_enter();  // lib.rs:2863-2866
    uint32_t inner;
    sk_lane *l = lane_of(p, handle, &inner);
    return l ? lane_queued_input_bytes(l, inner) : 0;
} catch (...) {
    (void)sk::abi_caught("sk_pipeline_queued_input_bytes");
    return 0;
}

int sk_pipeline_get_stats(sk_pipeline *p, sk_pipeline_stats *out) try {
    sk::abi_enter();
    if (!p || !out) return SK_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof(*out));
    for (sk_lane *l : p->lanes) {
        sk_pipeline_stats s{};
        (void)lane_get_stats(l, &s);
        out->ticks += s.ticks;
        out->frames += s.frames;
        out->outputs += s.outputs;
        out->errors += s.errors;
        out->parse_ns += s.parse_ns;
        out->tick_ns += s.tick_ns;
        out->idle_ns += s.idle_ns;
        out->deliver_ns += s.deliver_ns;
        out->entropy_threads += s.entropy_threads;
    }
    out->lanes = (uint32_t)p->lanes.size();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_pipeline_get_stats");
}

// ---- the two stream processors by themselves (pcm_stream.h), for callers and tests without a GPU ----

int sk_wav_reader_create(sk_wav_reader **out) try {
    sk::abi_enter();
    if (!out) return SK_ERR_INVALID_ARG;
    *out = new sk_wav_reader();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_wav_reader_create");
}

void sk_wav_reader_destroy(sk_wav_reader *r) try {
    sk::abi_enter();
    delete r;
} catch (...) {
    (void)sk::abi_caught("sk_wav_reader_destroy");
}

int sk_wav_reader_add(sk_wav_reader *r, const uint8_t *bytes, size_t len, uint64_t *piece_offset, size_t *piece_len, const uint8_t **piece) try {
    sk::abi_enter();
    if (!r || (len && !bytes) || !piece_offset || !piece_len) return SK_ERR_INVALID_ARG;
    sk_pcm::Piece got;
    *piece_offset = 0, *piece_len = 0;
    if (piece) *piece = nullptr;
    if (!r->stream.add(bytes, len, got, r->error)) return SK_PCM_ERR_STREAM;
    *piece_offset = got.stream_offset, *piece_len = got.len;
    if (piece) *piece = got.data;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_wav_reader_add");
}

int sk_wav_reader_info(const sk_wav_reader *r, uint32_t *sample_rate, uint32_t *channels, uint32_t *bits, int *is_float, uint64_t *total_frames) try {
    sk::abi_enter();
    if (!r) return SK_ERR_INVALID_ARG;
    if (sample_rate) *sample_rate = r->stream.sample_rate();
    if (channels) *channels = r->stream.channels();
    if (bits) *bits = r->stream.bits();
    if (is_float) *is_float = r->stream.is_float() ? 1 : 0;
    if (total_frames) *total_frames = r->stream.total_frames();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_wav_reader_info");
}

const char *sk_wav_reader_last_error(const sk_wav_reader *r) try {
    sk::abi_enter();
    return r ? r->error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_wav_reader_last_error");
    return "";
}

// the walker in its coded mode (A-law, mu-law, IMA and Microsoft ADPCM besides PCM and float): this project's own
int sk_wav_coded_reader_create(sk_wav_coded_reader **out) try {
    sk::abi_enter();
    if (!out) return SK_ERR_INVALID_ARG;
    *out = new sk_wav_coded_reader();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_wav_coded_reader_create");
}

void sk_wav_coded_reader_destroy(sk_wav_coded_reader *r) try {
    sk::abi_enter();
    delete r;
} catch (...) {
    (void)sk::abi_caught("sk_wav_coded_reader_destroy");
}

int sk_wav_coded_reader_add(sk_wav_coded_reader *r, const uint8_t *bytes, size_t len, uint64_t *piece_offset, size_t *piece_len, const uint8_t **piece) try {
    sk::abi_enter();
    if (!r || (len && !bytes) || !piece_offset || !piece_len) return SK_ERR_INVALID_ARG;
    sk_pcm::Piece got;
    *piece_offset = 0, *piece_len = 0;
    if (piece) *piece = nullptr;
    if (!r->stream.add(bytes, len, got, r->error)) return SK_PCM_ERR_STREAM;
    *piece_offset = got.stream_offset, *piece_len = got.len;
    if (piece) *piece = got.data;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_wav_coded_reader_add");
}

int sk_wav_coded_reader_info(const sk_wav_coded_reader *r, sk_wav_coded_info *info) try {
    sk::abi_enter();
    if (!r || !info) return SK_ERR_INVALID_ARG;
    std::memset(info, 0, sizeof *info);
    const sk_pcm::WavStream &s = r->stream;
    if (s.tag() == 0 || s.bits() == 0) return SK_OK;
    info->tag = s.tag(), info->sample_rate = s.sample_rate(), info->channels = s.channels(), info->bits = s.bits();
    info->is_float = s.is_float() ? 1 : 0;
    info->block_align = s.block_align(), info->frames_per_block = s.frames_per_block(), info->n_coef = s.n_coef();
    std::memcpy(info->coef, s.coef(), sizeof info->coef);
    info->fact_frames = s.fact_frames();
    info->total_frames = s.total_frames();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_wav_coded_reader_info");
}

const char *sk_wav_coded_reader_last_error(const sk_wav_coded_reader *r) try {
    sk::abi_enter();
    return r ? r->error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_wav_coded_reader_last_error");
    return "";
}

int sk_raw_pcm_framer_create(uint32_t bytes_per_frame, sk_raw_pcm_framer **out) try {
    sk::abi_enter();
    if (!out) return SK_ERR_INVALID_ARG;
    *out = new sk_raw_pcm_framer(bytes_per_frame);
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_raw_pcm_framer_create");
}

void sk_raw_pcm_framer_destroy(sk_raw_pcm_framer *f) try {
    sk::abi_enter();
    delete f;
} catch (...) {
    (void)sk::abi_caught("sk_raw_pcm_framer_destroy");
}

int sk_raw_pcm_framer_add(sk_raw_pcm_framer *f, const uint8_t *bytes, size_t len, uint64_t *piece_offset, size_t *piece_len, const uint8_t **piece) try {
    sk::abi_enter();
    if (!f || (len && !bytes) || !piece_offset || !piece_len) return SK_ERR_INVALID_ARG;
    sk_pcm::Piece got;
    *piece_offset = 0, *piece_len = 0;
    if (piece) *piece = nullptr;
    if (!f->stream.add(bytes, len, got, f->error)) return SK_PCM_ERR_STREAM;
    *piece_offset = got.stream_offset, *piece_len = got.len;
    if (piece) *piece = got.data;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_raw_pcm_framer_add");
}

int sk_raw_pcm_framer_flush(sk_raw_pcm_framer *f) try {
    sk::abi_enter();
    if (!f) return SK_ERR_INVALID_ARG;
    return f->stream.flush(f->error) ? SK_OK : SK_PCM_ERR_STREAM;
} catch (...) {
    return sk::abi_caught("sk_raw_pcm_framer_flush");
}

const char *sk_raw_pcm_framer_last_error(const sk_raw_pcm_framer *f) try {
    sk::abi_enter();
    return f ? f->error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_raw_pcm_framer_last_error");
    return "";
}

int sk_aiff_reader_create(sk_aiff_reader **out) try {
    sk::abi_enter();
    if (!out) return SK_ERR_INVALID_ARG;
    *out = new sk_aiff_reader();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_aiff_reader_create");
}

void sk_aiff_reader_destroy(sk_aiff_reader *r) try {
    sk::abi_enter();
    delete r;
} catch (...) {
    (void)sk::abi_caught("sk_aiff_reader_destroy");
}

int sk_aiff_reader_add(sk_aiff_reader *r, const uint8_t *bytes, size_t len, uint64_t *piece_offset, size_t *piece_len, const uint8_t **piece) try {
    sk::abi_enter();
    if (!r || (len && !bytes) || !piece_offset || !piece_len) return SK_ERR_INVALID_ARG;
    sk_pcm::Piece got;
    *piece_offset = 0, *piece_len = 0;
    if (piece) *piece = nullptr;
    if (!r->stream.add(bytes, len, got, r->error)) return SK_PCM_ERR_STREAM;
    *piece_offset = got.stream_offset, *piece_len = got.len;
    if (piece) *piece = got.data;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_aiff_reader_add");
}

int sk_aiff_reader_info(const sk_aiff_reader *r, sk_aiff_info *info) try {
    sk::abi_enter();
    if (!r || !info) return SK_ERR_INVALID_ARG;
    std::memset(info, 0, sizeof *info);
    info->buffered_bytes = (uint32_t)r->stream.buffered_bytes();
    if (!r->stream.have_info()) return SK_OK;
    info->sample_rate = r->stream.sample_rate();
    info->channels = (uint8_t)r->stream.channels();
    info->encoding = (uint8_t)r->stream.encoding();
    info->bits = (uint8_t)r->stream.bits();
    info->is_float = r->stream.is_float() ? 1 : 0;
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_aiff_reader_info");
}

const char *sk_aiff_reader_last_error(const sk_aiff_reader *r) try {
    sk::abi_enter();
    return r ? r->error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_aiff_reader_last_error");
    return "";
}

}  // extern "C"

// ---- MP4 / M4A (mp4_stream.h) -----------------------------------------------------------------------------------------------------

struct sk_mp4_demuxer {
    sk_mp4::Demuxer demuxer;
};

struct sk_mp4_index {
    sk_mp4::Track track;
};

struct sk_caf_index {
    sk_caf::Index index;
};

namespace {

void mp4_text(char *error, size_t cap, const std::string &text) {
    if (!error || cap == 0) return;
    const size_t n = std::min(cap - 1, text.size());
    std::memcpy(error, text.data(), n);
    error[n] = 0;
}

int mp4_track_info(const sk_mp4::Track &t, bool have, sk_mp4_track_info *info, uint8_t *codec_private, size_t private_cap) {
    std::memset(info, 0, sizeof *info);
    if (!have) return SK_OK;
    info->codec = t.codec, info->sample_rate = t.sample_rate, info->channels = t.channels, info->bits_per_sample = t.bits;
    info->track_id = t.id, info->timescale = t.timescale, info->sample_count = (uint32_t)t.samples.size();
    info->fragmented = t.fragmented ? 1 : 0, info->has_edit = t.has_edit ? 1 : 0;
    info->private_len = (uint32_t)t.codec_private.size();
    info->edit_presentation_start = t.edit_presentation_start, info->edit_media_start = t.edit_media_start, info->edit_duration = t.edit_duration;
    if (private_cap < t.codec_private.size()) return SK_ERR_CAPACITY;
    if (!t.codec_private.empty()) std::memcpy(codec_private, t.codec_private.data(), t.codec_private.size());
    return SK_OK;
}

int mp4_pcm_info(const sk_mp4::Track &t, bool have, sk_mp4_pcm_info *info) {
    std::memset(info, 0, sizeof *info);
    if (!have || t.codec != sk_mp4::kCodecPcm) return SK_OK;
    std::memcpy(info->codec_id, t.pcm.name, 4);
    info->big_endian = t.pcm.big_endian ? 1 : 0, info->is_float = t.pcm.is_float ? 1 : 0, info->bits_per_sample = t.bits;
    info->bytes_per_frame = t.pcm.bytes_per_frame, info->frames_per_packet = t.pcm.frames_per_packet;
    return SK_OK;
}

}  // namespace

extern "C" {

// ---- CAF (caf_stream.h) -------------------------------------------------------------------------------------------------------------------

int sk_caf_index_from_file(const uint8_t *file, size_t len, sk_caf_index **out, char *error, size_t error_cap) try {
    sk::abi_enter();
    if ((len && !file) || !out) return SK_ERR_INVALID_ARG;
    *out = nullptr;
    mp4_text(error, error_cap, "");
    std::unique_ptr<sk_caf_index> ix(new sk_caf_index());
    std::string text;
    static const uint8_t none[1] = {0};
    if (!sk_caf::index_from_file(len ? file : none, len, &ix->index, &text)) {
        mp4_text(error, error_cap, text);
        return SK_CAF_ERR_STREAM;
    }
    *out = ix.release();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_caf_index_from_file");
}

int sk_caf_index_create(const uint8_t *desc, size_t desc_len, const uint8_t *cookie, size_t cookie_len, const uint8_t *pakt, size_t pakt_len,
                        uint64_t data_offset, uint64_t data_size, sk_caf_index **out, char *error, size_t error_cap) try {
    sk::abi_enter();
    if ((desc_len && !desc) || (cookie_len && !cookie) || !out) return SK_ERR_INVALID_ARG;
    *out = nullptr;
    mp4_text(error, error_cap, "");
    std::unique_ptr<sk_caf_index> ix(new sk_caf_index());
    std::string text;
    static const uint8_t none[1] = {0};
    if (!sk_caf::index_from_metadata(desc ? desc : none, desc_len, cookie ? cookie : none, cookie_len, pakt, pakt_len, data_offset, data_size, &ix->index,
                                     &text)) {
        mp4_text(error, error_cap, text);
        return SK_CAF_ERR_STREAM;
    }
    *out = ix.release();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_caf_index_create");
}

void sk_caf_index_destroy(sk_caf_index *ix) try {
    sk::abi_enter();
    delete ix;
} catch (...) {
    (void)sk::abi_caught("sk_caf_index_destroy");
}

int sk_caf_index_info(const sk_caf_index *ix, sk_caf_info *info, uint8_t *cookie, size_t cookie_cap) try {
    sk::abi_enter();
    if (!ix || !info || (cookie_cap && !cookie)) return SK_ERR_INVALID_ARG;
    const sk_caf::Index &x = ix->index;
    std::memset(info, 0, sizeof *info);
    info->codec = x.codec;
    std::memcpy(info->format_id, x.format_id, 4);
    info->sample_rate = x.sample_rate, info->channels = x.channels, info->bits_per_sample = x.bits, info->format_flags = x.format_flags;
    info->big_endian = x.big_endian ? 1 : 0, info->is_float = x.is_float ? 1 : 0, info->bytes_per_frame = x.bytes_per_frame;
    info->frames_per_packet = x.frames_per_packet, info->priming_frames = x.priming_frames, info->remainder_frames = x.remainder_frames;
    info->n_packets = (uint32_t)x.packets.size(), info->cookie_len = (uint32_t)x.cookie.size(), info->valid_frames = x.valid_frames;
    if (cookie_cap < x.cookie.size()) return SK_ERR_CAPACITY;
    if (!x.cookie.empty()) std::memcpy(cookie, x.cookie.data(), x.cookie.size());
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_caf_index_info");
}

int sk_caf_index_packets(const sk_caf_index *ix, uint64_t *offsets, uint32_t *sizes, uint32_t *frames, uint64_t *start_frames, uint32_t cap) try {
    sk::abi_enter();
    if (!ix) return SK_ERR_INVALID_ARG;
    const std::vector<sk_caf::Packet> &p = ix->index.packets;
    if (cap < p.size()) return SK_ERR_CAPACITY;
    for (size_t i = 0; i < p.size(); ++i) {
        if (offsets) offsets[i] = p[i].offset;
        if (sizes) sizes[i] = p[i].size;
        if (frames) frames[i] = p[i].frames;
        if (start_frames) start_frames[i] = p[i].start;
    }
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_caf_index_packets");
}

// ---- MP4: the PCM description and the FLAC configuration ------------------------------------------------------------------------------

int sk_mp4_demuxer_pcm_info(const sk_mp4_demuxer *d, sk_mp4_pcm_info *info) try {
    sk::abi_enter();
    if (!d || !info) return SK_ERR_INVALID_ARG;
    return mp4_pcm_info(d->demuxer.track, d->demuxer.have_track, info);
} catch (...) {
    return sk::abi_caught("sk_mp4_demuxer_pcm_info");
}

int sk_mp4_index_pcm_info(const sk_mp4_index *ix, sk_mp4_pcm_info *info) try {
    sk::abi_enter();
    if (!ix || !info) return SK_ERR_INVALID_ARG;
    return mp4_pcm_info(ix->track, true, info);
} catch (...) {
    return sk::abi_caught("sk_mp4_index_pcm_info");
}

int sk_mp4_flac_config(const uint8_t *data, size_t len, uint8_t *out, size_t out_cap, size_t *out_len, char *error, size_t error_cap) try {
    sk::abi_enter();
    if ((len && !data) || !out_len) return SK_ERR_INVALID_ARG;
    mp4_text(error, error_cap, "");
    std::vector<uint8_t> got;
    std::string text;
    if (!sk_mp4::normalize_flac_config(data, len, &got, &text)) {
        mp4_text(error, error_cap, text);
        return SK_MP4_ERR_STREAM;
    }
    *out_len = got.size();
    if (out_cap < got.size() || !out) return SK_ERR_CAPACITY;
    std::memcpy(out, got.data(), got.size());
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_mp4_flac_config");
}

int sk_mp4_demuxer_create(sk_mp4_demuxer **out) try {
    sk::abi_enter();
    if (!out) return SK_ERR_INVALID_ARG;
    *out = new sk_mp4_demuxer();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_mp4_demuxer_create");
}

void sk_mp4_demuxer_destroy(sk_mp4_demuxer *d) try {
    sk::abi_enter();
    delete d;
} catch (...) {
    (void)sk::abi_caught("sk_mp4_demuxer_destroy");
}

int sk_mp4_demuxer_add(sk_mp4_demuxer *d, const uint8_t *bytes, size_t len) try {
    sk::abi_enter();
    if (!d || (len && !bytes)) return SK_ERR_INVALID_ARG;
    return d->demuxer.add(bytes, len) ? SK_OK : SK_MP4_ERR_STREAM;
} catch (...) {
    return sk::abi_caught("sk_mp4_demuxer_add");
}

int sk_mp4_demuxer_finish(sk_mp4_demuxer *d) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    return d->demuxer.finish() ? SK_OK : SK_MP4_ERR_STREAM;
} catch (...) {
    return sk::abi_caught("sk_mp4_demuxer_finish");
}

const char *sk_mp4_demuxer_last_error(const sk_mp4_demuxer *d) try {
    sk::abi_enter();
    return d ? d->demuxer.error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_mp4_demuxer_last_error");
    return "";
}

int sk_mp4_demuxer_config(const sk_mp4_demuxer *d, sk_mp4_track_info *info, uint8_t *codec_private, size_t private_cap) try {
    sk::abi_enter();
    if (!d || !info || (private_cap && !codec_private)) return SK_ERR_INVALID_ARG;
    return mp4_track_info(d->demuxer.track, d->demuxer.have_track, info, codec_private, private_cap);
} catch (...) {
    return sk::abi_caught("sk_mp4_demuxer_config");
}

int sk_mp4_demuxer_pending(const sk_mp4_demuxer *d, uint32_t *n_packets, size_t *front_bytes, size_t *buffered_bytes) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    if (n_packets) *n_packets = (uint32_t)d->demuxer.packets.size();
    if (front_bytes) *front_bytes = d->demuxer.packets.empty() ? 0 : d->demuxer.packets.front().data.size();
    if (buffered_bytes) *buffered_bytes = d->demuxer.buffered();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_mp4_demuxer_pending");
}

int sk_mp4_demuxer_take(sk_mp4_demuxer *d, uint8_t *out, size_t cap, size_t *len, uint64_t *start_time, uint32_t *duration) try {
    sk::abi_enter();
    if (!d || !len || (cap && !out)) return SK_ERR_INVALID_ARG;
    if (d->demuxer.packets.empty()) return SK_ERR_BAD_STREAM;
    const sk_mp4::Packet &p = d->demuxer.packets.front();
    *len = p.data.size();
    if (cap < p.data.size()) return SK_ERR_CAPACITY;
    if (!p.data.empty()) std::memcpy(out, p.data.data(), p.data.size());
    if (start_time) *start_time = p.start;
    if (duration) *duration = p.duration;
    d->demuxer.packets.pop_front();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_mp4_demuxer_take");
}

int sk_mp4_demuxer_trim(const sk_mp4_demuxer *d, uint64_t start_time, uint32_t duration, uint32_t decoded_frames, uint32_t decoded_rate, uint32_t *first,
                        uint32_t *count, char *error, size_t error_cap) try {
    sk::abi_enter();
    if (!d || !first || !count) return SK_ERR_INVALID_ARG;
    mp4_text(error, error_cap, "");
    std::string text = "MP4 demuxer has no track yet";
    sk_mp4::Sample s;
    s.start = start_time, s.duration = duration;
    if (!d->demuxer.have_track || !sk_mp4::trim(d->demuxer.track, s, decoded_frames, decoded_rate, first, count, &text)) {
        mp4_text(error, error_cap, text);
        return SK_MP4_ERR_STREAM;
    }
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_mp4_demuxer_trim");
}

int sk_mp4_index_from_file(const uint8_t *file, size_t len, sk_mp4_index **out, char *error, size_t error_cap) try {
    sk::abi_enter();
    if ((len && !file) || !out) return SK_ERR_INVALID_ARG;
    *out = nullptr;
    mp4_text(error, error_cap, "");
    std::unique_ptr<sk_mp4_index> ix(new sk_mp4_index());
    std::string text;
    static const uint8_t none[1] = {0};
    if (!sk_mp4::index_from_file(len ? file : none, len, &ix->track, &text)) {
        mp4_text(error, error_cap, text);
        return SK_MP4_ERR_STREAM;
    }
    *out = ix.release();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_mp4_index_from_file");
}

void sk_mp4_index_destroy(sk_mp4_index *ix) try {
    sk::abi_enter();
    delete ix;
} catch (...) {
    (void)sk::abi_caught("sk_mp4_index_destroy");
}

int sk_mp4_index_info(const sk_mp4_index *ix, sk_mp4_track_info *info, uint8_t *codec_private, size_t private_cap) try {
    sk::abi_enter();
    if (!ix || !info || (private_cap && !codec_private)) return SK_ERR_INVALID_ARG;
    return mp4_track_info(ix->track, true, info, codec_private, private_cap);
} catch (...) {
    return sk::abi_caught("sk_mp4_index_info");
}

int sk_mp4_index_samples(const sk_mp4_index *ix, uint64_t *offsets, uint32_t *sizes, uint32_t *durations, uint64_t *start_times, uint32_t cap) try {
    sk::abi_enter();
    if (!ix) return SK_ERR_INVALID_ARG;
    const std::vector<sk_mp4::Sample> &s = ix->track.samples;
    if (cap < s.size()) return SK_ERR_CAPACITY;
    for (size_t i = 0; i < s.size(); ++i) {
        if (offsets) offsets[i] = s[i].offset;
        if (sizes) sizes[i] = s[i].size;
        if (durations) durations[i] = s[i].duration;
        if (start_times) start_times[i] = s[i].start;
    }
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_mp4_index_samples");
}

int sk_mp4_index_trim(const sk_mp4_index *ix, uint32_t sample, uint32_t decoded_frames, uint32_t decoded_rate, uint32_t *first, uint32_t *count,
                      char *error, size_t error_cap) try {
    sk::abi_enter();
    if (!ix || !first || !count) return SK_ERR_INVALID_ARG;
    mp4_text(error, error_cap, "");
    std::string text;
    if (sample >= ix->track.samples.size()) {
        mp4_text(error, error_cap, "MP4 sample index " + std::to_string(sample) + " is out of range");
        return SK_MP4_ERR_STREAM;
    }
    if (!sk_mp4::trim(ix->track, ix->track.samples[sample], decoded_frames, decoded_rate, first, count, &text)) {
        mp4_text(error, error_cap, text);
        return SK_MP4_ERR_STREAM;
    }
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_mp4_index_trim");
}

int sk_mp4_adts_header(const uint8_t *asc, size_t asc_len, uint32_t sample_rate, uint32_t channels, size_t raw_len, uint8_t out[7]) try {
    sk::abi_enter();
    if ((asc_len && !asc) || !out) return SK_ERR_INVALID_ARG;
    sk_mp4::adts_header(asc, asc_len, sample_rate, channels, raw_len, out);
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_mp4_adts_header");
}

}  // extern "C"

// ---- WebM / Matroska (webm_stream.h) ------------------------------------------------------------------------------------------------

struct sk_webm_demuxer {
    sk_webm::Demuxer demuxer;
};

extern "C" {

int sk_webm_demuxer_create(sk_webm_demuxer **out) try {
    sk::abi_enter();
    if (!out) return SK_ERR_INVALID_ARG;
    *out = new sk_webm_demuxer();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_webm_demuxer_create");
}

void sk_webm_demuxer_destroy(sk_webm_demuxer *d) try {
    sk::abi_enter();
    delete d;
} catch (...) {
    (void)sk::abi_caught("sk_webm_demuxer_destroy");
}

int sk_webm_demuxer_add(sk_webm_demuxer *d, const uint8_t *bytes, size_t len) try {
    sk::abi_enter();
    if (!d || (len && !bytes)) return SK_ERR_INVALID_ARG;
    return d->demuxer.add(bytes, len) ? SK_OK : SK_WEBM_ERR_STREAM;
} catch (...) {
    return sk::abi_caught("sk_webm_demuxer_add");
}

int sk_webm_demuxer_finish(sk_webm_demuxer *d) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    return d->demuxer.finish() ? SK_OK : SK_WEBM_ERR_STREAM;
} catch (...) {
    return sk::abi_caught("sk_webm_demuxer_finish");
}

const char *sk_webm_demuxer_last_error(const sk_webm_demuxer *d) try {
    sk::abi_enter();
    return d ? d->demuxer.error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_webm_demuxer_last_error");
    return "";
}

uint32_t sk_webm_demuxer_n_tracks(const sk_webm_demuxer *d) try {
    sk::abi_enter();
    return d && d->demuxer.configured ? (uint32_t)d->demuxer.audio.size() : 0;
} catch (...) {
    (void)sk::abi_caught("sk_webm_demuxer_n_tracks");
    return 0;
}

int sk_webm_demuxer_config(const sk_webm_demuxer *d, uint32_t index, sk_webm_track_info *info, uint8_t *codec_private, size_t private_cap, uint8_t *prefix,
                           size_t prefix_cap) try {
    sk::abi_enter();
    if (!d || !info || (private_cap && !codec_private) || (prefix_cap && !prefix)) return SK_ERR_INVALID_ARG;
    if (!d->demuxer.configured || index >= d->demuxer.audio.size()) return SK_ERR_INVALID_ARG;
    const sk_webm::Track &t = d->demuxer.audio[index];
    std::memset(info, 0, sizeof *info);
    info->track_number = t.number, info->codec_delay_ns = t.codec_delay_ns, info->seek_pre_roll_ns = t.seek_pre_roll_ns;
    info->default_duration_ns = t.has_default_duration ? t.default_duration_ns : 0, info->timecode_scale_ns = d->demuxer.timecode_scale_ns;
    info->track_timestamp_scale = t.timestamp_scale, info->codec = t.codec;
    info->sample_rate = t.has_rate ? t.sample_rate : 48000, info->channels = t.has_channels ? t.channels : 2;
    info->private_len = (uint32_t)t.codec_private.size(), info->prefix_len = (uint32_t)t.prefix.size();
    if (private_cap < t.codec_private.size() || prefix_cap < t.prefix.size()) return SK_ERR_CAPACITY;
    if (!t.codec_private.empty()) std::memcpy(codec_private, t.codec_private.data(), t.codec_private.size());
    if (!t.prefix.empty()) std::memcpy(prefix, t.prefix.data(), t.prefix.size());
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_webm_demuxer_config");
}

int sk_webm_demuxer_pending(const sk_webm_demuxer *d, uint32_t *n_packets, size_t *front_bytes, size_t *buffered_bytes) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    if (n_packets) *n_packets = (uint32_t)d->demuxer.packets.size();
    if (front_bytes) *front_bytes = d->demuxer.packets.empty() ? 0 : d->demuxer.packets.front().data.size();
    if (buffered_bytes) *buffered_bytes = d->demuxer.buffered();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_webm_demuxer_pending");
}

int sk_webm_demuxer_take(sk_webm_demuxer *d, uint8_t *out, size_t cap, size_t *len, sk_webm_packet_info *info) try {
    sk::abi_enter();
    if (!d || !len || (cap && !out)) return SK_ERR_INVALID_ARG;
    if (d->demuxer.packets.empty()) return SK_ERR_BAD_STREAM;
    const sk_webm::Packet &p = d->demuxer.packets.front();
    *len = p.data.size();
    if (cap < p.data.size()) return SK_ERR_CAPACITY;
    if (!p.data.empty()) std::memcpy(out, p.data.data(), p.data.size());
    if (info) {
        std::memset(info, 0, sizeof *info);
        info->track_number = p.track, info->timestamp_ns = p.timestamp_ns, info->duration_ns = p.duration_ns, info->discard_padding_ns = p.discard_ns;
        info->codec = p.codec, info->has_duration = p.has_duration, info->has_discard_padding = p.has_discard;
    }
    d->demuxer.pop_packet();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_webm_demuxer_take");
}

int sk_webm_vorbis_headers(const uint8_t *codec_private, size_t len, size_t offsets[3], size_t sizes[3], char *error, size_t error_cap) try {
    sk::abi_enter();
    if ((len && !codec_private) || !offsets || !sizes) return SK_ERR_INVALID_ARG;
    mp4_text(error, error_cap, "");
    std::string text;
    if (!sk_webm::vorbis_headers(codec_private, len, offsets, sizes, &text)) {
        mp4_text(error, error_cap, text);
        return SK_WEBM_ERR_STREAM;
    }
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_webm_vorbis_headers");
}

int sk_webm_discard_frames(int64_t padding_ns, uint32_t sample_rate, uint32_t decoded_frames, uint32_t *front, uint32_t *back, char *error,
                           size_t error_cap) try {
    sk::abi_enter();
    if (!front || !back) return SK_ERR_INVALID_ARG;
    mp4_text(error, error_cap, "");
    std::string text;
    if (!sk_webm::discard_frames(padding_ns, sample_rate, decoded_frames, front, back, &text)) {
        mp4_text(error, error_cap, text);
        return SK_WEBM_ERR_STREAM;
    }
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_webm_discard_frames");
}

}  // extern "C"

// ---- MPEG transport stream (ts_stream.h) --------------------------------------------------------------------------------------------

struct sk_ts_demuxer {
    sk_ts::Demuxer demuxer;
};

extern "C" {

int sk_ts_demuxer_create(sk_ts_demuxer **out) try {
    sk::abi_enter();
    if (!out) return SK_ERR_INVALID_ARG;
    *out = new sk_ts_demuxer();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_ts_demuxer_create");
}

void sk_ts_demuxer_destroy(sk_ts_demuxer *d) try {
    sk::abi_enter();
    delete d;
} catch (...) {
    (void)sk::abi_caught("sk_ts_demuxer_destroy");
}

int sk_ts_demuxer_add(sk_ts_demuxer *d, const uint8_t *bytes, size_t len) try {
    sk::abi_enter();
    if (!d || (len && !bytes)) return SK_ERR_INVALID_ARG;
    return d->demuxer.add(bytes, len) ? SK_OK : SK_TS_ERR_STREAM;
} catch (...) {
    return sk::abi_caught("sk_ts_demuxer_add");
}

int sk_ts_demuxer_finish(sk_ts_demuxer *d) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    return d->demuxer.finish() ? SK_OK : SK_TS_ERR_STREAM;
} catch (...) {
    return sk::abi_caught("sk_ts_demuxer_finish");
}

const char *sk_ts_demuxer_last_error(const sk_ts_demuxer *d) try {
    sk::abi_enter();
    return d ? d->demuxer.error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_ts_demuxer_last_error");
    return "";
}

int sk_ts_demuxer_config(const sk_ts_demuxer *d, sk_ts_track_info *info) try {
    sk::abi_enter();
    if (!d || !info) return SK_ERR_INVALID_ARG;
    if (!d->demuxer.configured) return SK_ERR_BAD_STREAM;
    const sk_ts::Config &c = d->demuxer.config;
    std::memset(info, 0, sizeof *info);
    info->codec = c.codec, info->packet_format = c.format, info->stream_type = c.stream_type, info->pid = c.pid, info->program_number = c.program;
    info->packet_stride = c.stride, info->packet_prefix = c.prefix;
    info->has_rate = c.has_rate, info->has_channels = c.has_channels;
    info->sample_rate = c.has_rate ? c.sample_rate : 0, info->channels = c.has_channels ? c.channels : 0;
    info->bits_per_sample = c.bits, info->bytes_per_frame = c.bytes_per_frame, info->frames_per_packet = c.frames_per_packet;
    std::memcpy(info->lpcm_header, c.lpcm_header, 4);
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_ts_demuxer_config");
}

int sk_ts_demuxer_pending(const sk_ts_demuxer *d, uint32_t *n_packets, size_t *front_bytes, size_t *buffered_bytes) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    if (n_packets) *n_packets = (uint32_t)d->demuxer.packets.size();
    if (front_bytes) *front_bytes = d->demuxer.packets.empty() ? 0 : d->demuxer.packets.front().data.size();
    if (buffered_bytes) *buffered_bytes = d->demuxer.buffered();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_ts_demuxer_pending");
}

int sk_ts_demuxer_take(sk_ts_demuxer *d, uint8_t *out, size_t cap, size_t *len, sk_ts_packet_info *info) try {
    sk::abi_enter();
    if (!d || !len || (cap && !out)) return SK_ERR_INVALID_ARG;
    if (d->demuxer.packets.empty()) return SK_ERR_BAD_STREAM;
    const sk_ts::Packet &p = d->demuxer.packets.front();
    *len = p.data.size();
    if (cap < p.data.size()) return SK_ERR_CAPACITY;
    if (!p.data.empty()) std::memcpy(out, p.data.data(), p.data.size());
    if (info) {
        std::memset(info, 0, sizeof *info);
        info->pts = p.has_pts ? p.pts : 0, info->dts = p.has_dts ? p.dts : 0, info->duration = p.has_duration ? p.duration : 0;
        info->has_pts = p.has_pts, info->has_dts = p.has_dts, info->has_duration = p.has_duration;
        info->continuity_counter = p.continuity, info->discontinuity = p.discontinuity;
    }
    (void)d->demuxer.take_packet();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_ts_demuxer_take");
}

int sk_ts_sniff(const uint8_t *bytes, size_t len) try {
    sk::abi_enter();
    return bytes && sk_ts::sniff(bytes, len) ? 1 : 0;
} catch (...) {
    (void)sk::abi_caught("sk_ts_sniff");
    return 0;
}

}  // extern "C"

// ---- AVI and MPEG program stream (avi_stream.h, ps_stream.h) --------------------------------------------------------------------------

struct sk_avi_demuxer {
    sk_avi::Demuxer demuxer;
    bool config_taken = false;
};
struct sk_ps_demuxer {
    explicit sk_ps_demuxer(uint8_t mode) : demuxer(mode) {}
    sk_ps::Demuxer demuxer;
    bool config_taken = false;
};

namespace {
void demux_info(const sk_avi::Config &c, sk_avi_track_info *info) {
    info->stream_index = c.stream_index, info->sample_rate = c.sample_rate, info->format_tag = c.format_tag, info->channels = c.channels, info->bits = c.bits;
}
void demux_info(const sk_ps::Config &c, sk_ps_track_info *info) {
    info->sample_rate = c.sample_rate, info->block_bytes = c.block_bytes, info->kind = c.kind, info->stream_id = c.stream_id;
    info->substream_id = c.substream_id, info->channels = c.channels, info->bits = c.bits;
}
// sk_avi_demuxer_next / sk_ps_demuxer_next: the config in front of the first packet, then the packets in order
template <class Handle, class Info>
int demux_next(Handle *d, int *event, Info *info, uint8_t *out, size_t cap, size_t *len) {
    if (!d || !event || !len || (cap && !out)) return SK_ERR_INVALID_ARG;
    *event = SK_DEMUX_NONE, *len = 0;
    if (d->demuxer.configured && !d->config_taken) {
        if (!info) return SK_ERR_INVALID_ARG;
        std::memset(info, 0, sizeof *info);
        demux_info(d->demuxer.config, info);
        d->config_taken = true;
        *event = SK_DEMUX_CONFIG;
        return SK_OK;
    }
    if (d->demuxer.packets.empty()) return SK_OK;
    const std::vector<uint8_t> &data = d->demuxer.packets.front().data;
    *len = data.size();
    if (cap < data.size()) return SK_ERR_CAPACITY;
    if (!data.empty()) std::memcpy(out, data.data(), data.size());
    (void)d->demuxer.take_packet();
    *event = SK_DEMUX_PACKET;
    return SK_OK;
}
}  // namespace

extern "C" {

int sk_avi_demuxer_create(sk_avi_demuxer **out) try {
    sk::abi_enter();
    if (!out) return SK_ERR_INVALID_ARG;
    *out = new sk_avi_demuxer();
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_avi_demuxer_create");
}

void sk_avi_demuxer_destroy(sk_avi_demuxer *d) try {
    sk::abi_enter();
    delete d;
} catch (...) {
    (void)sk::abi_caught("sk_avi_demuxer_destroy");
}

int sk_avi_demuxer_add(sk_avi_demuxer *d, const uint8_t *bytes, size_t len) try {
    sk::abi_enter();
    if (!d || (len && !bytes)) return SK_ERR_INVALID_ARG;
    return d->demuxer.add(bytes, len) ? SK_OK : SK_AVI_ERR_STREAM;
} catch (...) {
    return sk::abi_caught("sk_avi_demuxer_add");
}

int sk_avi_demuxer_finish(sk_avi_demuxer *d) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    return d->demuxer.finish() ? SK_OK : SK_AVI_ERR_STREAM;
} catch (...) {
    return sk::abi_caught("sk_avi_demuxer_finish");
}

int sk_avi_demuxer_next(sk_avi_demuxer *d, int *event, sk_avi_track_info *info, uint8_t *out, size_t cap, size_t *len) try {
    sk::abi_enter();
    return demux_next(d, event, info, out, cap, len);
} catch (...) {
    return sk::abi_caught("sk_avi_demuxer_next");
}

const char *sk_avi_demuxer_last_error(const sk_avi_demuxer *d) try {
    sk::abi_enter();
    return d ? d->demuxer.error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_avi_demuxer_last_error");
    return "";
}

int sk_ps_demuxer_create(int track_mode, sk_ps_demuxer **out) try {
    sk::abi_enter();
    if (!out || track_mode < SK_PS_TRACK_FIRST || track_mode > SK_PS_TRACK_MPEG_AUDIO) return SK_ERR_INVALID_ARG;
    *out = new sk_ps_demuxer((uint8_t)track_mode);
    return SK_OK;
} catch (...) {
    return sk::abi_caught("sk_ps_demuxer_create");
}

void sk_ps_demuxer_destroy(sk_ps_demuxer *d) try {
    sk::abi_enter();
    delete d;
} catch (...) {
    (void)sk::abi_caught("sk_ps_demuxer_destroy");
}

int sk_ps_demuxer_add(sk_ps_demuxer *d, const uint8_t *bytes, size_t len) try {
    sk::abi_enter();
    if (!d || (len && !bytes)) return SK_ERR_INVALID_ARG;
    return d->demuxer.add(bytes, len) ? SK_OK : SK_PS_ERR_STREAM;
} catch (...) {
    return sk::abi_caught("sk_ps_demuxer_add");
}

int sk_ps_demuxer_finish(sk_ps_demuxer *d) try {
    sk::abi_enter();
    if (!d) return SK_ERR_INVALID_ARG;
    return d->demuxer.finish() ? SK_OK : SK_PS_ERR_STREAM;
} catch (...) {
    return sk::abi_caught("sk_ps_demuxer_finish");
}

int sk_ps_demuxer_next(sk_ps_demuxer *d, int *event, sk_ps_track_info *info, uint8_t *out, size_t cap, size_t *len) try {
    sk::abi_enter();
    return demux_next(d, event, info, out, cap, len);
} catch (...) {
    return sk::abi_caught("sk_ps_demuxer_next");
}

const char *sk_ps_demuxer_last_error(const sk_ps_demuxer *d) try {
    sk::abi_enter();
    return d ? d->demuxer.error.c_str() : "";
} catch (...) {
    (void)sk::abi_caught("sk_ps_demuxer_last_error");
    return "";
}

int sk_debug_throw_in_thread(int n, int where) {
    g_thread_throw_where.store(where, std::memory_order_relaxed);
    return g_thread_throw_after.exchange(n < 0 ? -1 : n, std::memory_order_relaxed);
}

}  // extern "C"

// mp3_decoder_gpu.cpp -- sk_mp3_decoder_decode_* with parts 2 + 3 on the device (sk_mp3_decoder_set_gpu_entropy).
//
// Framing, side information and the bit reservoir as in mp3_decoder.cpp's decode(); the frames and their assembled main data
// are collected and go through sk_mp3_decode_frames_* -- Huffman stage, requantisation and hybrid synthesis on the GPU, the
// integers never visiting the host.  Whether a frame decodes is known only after the device has seen it, while decode()'s
// rules (the output room, the stop once less than a frame's worth of room is left, the change of channel count) ask frame by
// frame.  So a call works in runs: frames are taken on the assumption that all of them decode -- then every rule comes out as in
// decode(), because a frame that fits after more samples fits after fewer -- and where the device reports a frame as
// dropped, the next run starts behind the last one with the true sample count.  A frame that stands AT a rule (it does not
// fit; it needs another stream) is asked about alone first (sk_mp3_entropy_decode of one frame).  A stream without damage
// costs one engine call per decode call, plus one single-frame question when its first frame opens the stream.
// "A failed call leaves the decoder as it was" holds for the host side (buffer, reservoir, counters); where a call needed several
// runs and a LATER one fails with a device error, the synthesis state the earlier runs advanced stays advanced.
//
// This file is what refers to the engine's device stage; mp3_decoder.cpp reaches it through sk_mp3_internal::gpu_hooks(),
// which the initialiser at the end fills in (mp3_internal.h says why).
#include "mp3_internal.h"

#include <cstring>

namespace {

using namespace sk_mp3_internal;

struct Assembled {
    bool host_ok = false;  // side information and main data are there
    sk_mp3_frame_item item;
};

// one frame's side information and main data (reservoir + its own bytes), appended to `bytes` as sk_mp3_decode_frames_* wants it
Assembled assemble(sk_mp3_decoder *d, const sk_mp3_frame_info &h, const std::vector<uint8_t> &reservoir, std::vector<uint8_t> &bytes) {
    Assembled a;
    const uint8_t *frame = d->buffer.data() + h.offset;
    a.item.header = h;
    if (sk_mp3_parse_side_info(frame, h.frame_bytes, &h, &a.item.side) != SK_OK) return a;
    d->main.resize(reservoir.size() + h.frame_bytes);
    size_t main_len = 0;
    if (sk_mp3_main_data(frame, h.frame_bytes, &h, &a.item.side, reservoir.data(), reservoir.size(), d->main.data(), d->main.size(), &main_len) != SK_OK) return a;
    const size_t at = (bytes.size() + 3) & ~(size_t)3;
    bytes.resize(at + main_len + 8, 0);  // 8 zero bytes behind every frame's data
    std::memcpy(bytes.data() + at, d->main.data(), main_len);
    a.item.byte_offset = (uint32_t)at;
    a.item.byte_len = (uint32_t)main_len;
    a.host_ok = true;
    return a;
}

int decode_gpu(sk_mp3_decoder *d, const uint8_t *input, size_t len, void *out, size_t out_cap, size_t *written, Out kind) {
    *written = 0;
    if (d->buffer.size() + len > kMaxBuffered) return SK_PIPE_CHUNK_TOO_LARGE;
    d->buffer.insert(d->buffer.end(), input, input + len);
    if (d->buffer.empty()) return SK_OK;
    auto fail = [&](int rc) {  // a failed call leaves the decoder as it was
        d->buffer.resize(d->buffer.size() - len);
        return rc;
    };

    d->found.resize(d->buffer.size() / 24 + 2);
    uint32_t n_found = 0;
    size_t scanned = 0;
    uint32_t free_format_bytes = d->free_format_bytes;
    uint32_t free_format_run = d->free_format_bytes;
    int rc = sk_mp3_scan_free(d->buffer.data(), d->buffer.size(), d->found.data(), (uint32_t)d->found.size(), &n_found, &scanned, &free_format_bytes);
    if (rc != SK_OK) return fail(rc);
    if (n_found > d->found.size()) n_found = (uint32_t)d->found.size();
    rc = gpu_hooks().install_codebook(d->engine, d->gpu_blob.data(), d->gpu_blob.size());  // another decoder of the engine may have brought its own
    if (rc != SK_OK) return fail(rc);

    d->staged_reservoir = d->reservoir;
    std::vector<uint8_t> &reservoir = d->staged_reservoir;
    uint32_t sample_rate = d->sample_rate;
    uint8_t channels = d->channels;
    uint64_t frames = d->frames;
    d->queued.clear();

    size_t samples = 0, consumed = 0;
    int result = SK_OK;
    bool stopped = false, any_queued = false;
    // what decode() does behind every frame it is done with, whatever became of it
    auto consume = [&](uint32_t k) {
        const sk_mp3_frame_info &h = d->found[k];
        const uint8_t *frame = d->buffer.data() + h.offset;
        const size_t head = 4u + (h.has_crc ? 2u : 0u) + h.side_info_bytes;
        if (h.frame_bytes > head) reservoir.insert(reservoir.end(), frame + head, frame + h.frame_bytes);
        if (reservoir.size() > 4 * kReservoirKept) reservoir.erase(reservoir.begin(), reservoir.end() - kReservoirKept);
        consumed = h.offset + h.frame_bytes;
        if ((frame[2] >> 4) == 0) free_format_run = h.frame_bytes - h.padding;
        if (k + 1 == n_found) consumed = scanned, free_format_run = free_format_bytes;
    };
    const size_t width = kind == Out::I16 ? 2 : 4;
    auto pcm_base = [&]() { return kind == Out::I32 ? (uint8_t *)d->pcm.data() : (uint8_t *)out; };  // i32: converted from f32 at the end

    uint32_t k = 0;
    while (k < n_found && !stopped) {
        const sk_mp3_frame_info &h = d->found[k];
        const size_t frame_samples = (size_t)h.samples_per_channel * h.channels;
        d->gpu_bytes.clear();
        Assembled first = assemble(d, h, reservoir, d->gpu_bytes);
        if (!first.host_ok) {
            consume(k++);
            continue;
        }
        const bool fits = samples + frame_samples <= out_cap;
        const bool other_stream = !d->stream_open || d->stream_channels != h.channels;
        if (!fits || other_stream) {  // the frame stands at one of decode()'s rules, which ask whether it decodes
            sk_mp3_granule_data cells[2][2];
            rc = sk_mp3_entropy_decode(d->engine, &first.item, 1, d->gpu_bytes.data(), d->gpu_bytes.size(), &cells[0][0]);
            if (rc != SK_OK) return fail(rc);
            bool decodable = true;
            for (int gr = 0; gr < first.item.side.granules; ++gr)
                for (int ch = 0; ch < first.item.side.channels; ++ch) decodable = decodable && cells[gr][ch].status == SK_OK;
            if (!decodable) {
                consume(k++);
                continue;
            }
            if (!fits) {  // write_frame_*: "Output buffer too small for decoded frame"
                result = SK_ERR_CAPACITY;
                break;
            }
            if (any_queued) break;  // frames queued for the old stream go first; this frame waits for the next call
            if (d->stream_open) (void)sk_stream_close(d->engine, d->stream);
            d->stream_open = false;
            rc = sk_stream_open(d->engine, h.sample_rate, h.channels, &d->stream);
            if (rc != SK_OK) return fail(rc);
            d->stream_open = true;
            d->stream_channels = h.channels;
        }
        // a run: frame k and what follows it, as long as no rule is met if all of them decode
        d->gpu_frames.clear();
        d->gpu_frames.push_back(first.item);
        size_t hoped = samples + frame_samples;
        bool hoped_stop = out_cap - hoped < SK_MP3_MAX_SAMPLES_PER_FRAME;  // lib.rs:300-302
        consume(k);
        uint32_t j = k + 1;
        while (!hoped_stop && j < n_found) {
            const sk_mp3_frame_info &hj = d->found[j];
            const size_t bytes_before = d->gpu_bytes.size();
            Assembled next = assemble(d, hj, reservoir, d->gpu_bytes);
            if (!next.host_ok) {
                consume(j++);
                continue;
            }
            const size_t more = (size_t)hj.samples_per_channel * hj.channels;
            if (hj.channels != d->stream_channels || hoped + more > out_cap) {  // at a rule: the outer loop's business
                d->gpu_bytes.resize(bytes_before);
                break;
            }
            d->gpu_frames.push_back(next.item);
            hoped += more;
            hoped_stop = out_cap - hoped < SK_MP3_MAX_SAMPLES_PER_FRAME;
            consume(j++);
        }
        const uint32_t n = (uint32_t)d->gpu_frames.size();
        d->gpu_streams.assign(n, d->stream);
        d->gpu_entropy_status.assign(n, 0);
        d->gpu_stage_status.assign(n, 0);
        size_t got = 0;
        if (kind == Out::I32 && d->pcm.size() < hoped) d->pcm.resize(hoped);
        uint8_t *dst = pcm_base() + samples * width;
        if (kind == Out::I16)
            rc = sk_mp3_decode_frames_s16(d->engine, d->gpu_frames.data(), d->gpu_streams.data(), n, d->gpu_bytes.data(), d->gpu_bytes.size(), (int16_t *)dst,
                                          out_cap - samples, d->gpu_entropy_status.data(), d->gpu_stage_status.data(), &got);
        else
            rc = sk_mp3_decode_frames_f32(d->engine, d->gpu_frames.data(), d->gpu_streams.data(), n, d->gpu_bytes.data(), d->gpu_bytes.size(), (float *)dst,
                                          out_cap - samples, d->gpu_entropy_status.data(), d->gpu_stage_status.data(), &got);
        if (rc != SK_OK) return fail(rc);
        bool last_decoded = false;
        for (uint32_t i = 0; i < n; ++i) {
            last_decoded = d->gpu_entropy_status[i] == SK_OK;
            if (!last_decoded) continue;
            const sk_mp3_frame_info &hi = d->gpu_frames[i].header;
            const size_t fs = (size_t)hi.samples_per_channel * hi.channels;
            if (!sample_rate) sample_rate = hi.sample_rate;
            if (!channels) channels = hi.channels;
            d->queued.push_back({0u, hi.granules, samples, fs, d->gpu_stage_status[i] != SK_OK});
            samples += fs;
            frames += 1;
            any_queued = true;
        }
        // the stop rule looks at the room behind a DECODED frame; within the run only its last frame can have met it
        if (hoped_stop && last_decoded && out_cap - samples < SK_MP3_MAX_SAMPLES_PER_FRAME) stopped = true;
        k = j;
    }

    if (any_queued) {
        // a frame one of whose granules a later GPU stage rejected is consumed without output: its samples are taken out
        size_t kept = 0;
        for (const auto &q : d->queued) {
            if (q.rejected) {
                frames -= 1;
                continue;
            }
            if (kept != q.first_sample) std::memmove(pcm_base() + kept * width, pcm_base() + q.first_sample * width, q.samples * width);
            kept += q.samples;
        }
        samples = kept;
        if (kind == Out::I32)
            for (size_t i = 0; i < samples; ++i) ((int32_t *)out)[i] = mp3_f32_to_i32(d->pcm[i]);
    } else if (n_found == 0) {
        consumed = scanned;
        free_format_run = free_format_bytes;
    }
    d->reservoir.swap(d->staged_reservoir);
    d->sample_rate = sample_rate, d->channels = channels, d->frames = frames;
    d->free_format_bytes = free_format_run;
    d->buffer.erase(d->buffer.begin(), d->buffer.begin() + (ptrdiff_t)consumed);
    *written = samples;
    return result;
}

const bool g_hooked = [] {
    GpuHooks &hooks = gpu_hooks();
    hooks.install_codebook = sk::mp3_install_codebook;
    hooks.decode = decode_gpu;
    return true;
}();

}  // namespace

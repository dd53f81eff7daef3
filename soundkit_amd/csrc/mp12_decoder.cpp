// mp12_decoder.cpp -- sk_mp3_decoder_decode_* on a Layer I / II stream.
//
// Mp3Decoder hands every MPEG-audio frame to one decoder of all three layers (soundkit-mp3/src/lib.rs:284), so the handle needs no
// switch: a stream's layer is that of its first confirmed frame (sk_mpa_scan with *layer = 0).  Until that frame and the header
// behind it are in the buffer a call only buffers; a stream that turns out to be Layer III is handed to mp3_decoder.cpp's decode()
// with nothing touched -- it sees the bytes it would have seen.  A Layer I / II stream is framed by sk_mpa_scan, each frame's serial
// front read by sk_mpa_parse_frame, and all frames of the call go through ONE sk_mpa_decode_frames_* launch; decode()'s output rules
// (the room, the stop once less than a frame's worth of room is left, the change of channel count, "a failed call leaves the decoder
// as it was") hold as there.  A frame the parse rejects is consumed without output.
//
// Like mp3_decoder_gpu.cpp this file refers to the engine's stage call; mp3_decoder.cpp reaches it through gpu_hooks().
#include "mp3_internal.h"
#include "mp12_internal.h"

#include <cstring>

namespace {

using namespace sk_mp3_internal;

int decode_mpa(sk_mp3_decoder *d, const uint8_t *input, size_t len, void *out, size_t out_cap, size_t *written, Out kind, bool *handled) {
    *handled = false;
    if (d->buffer.size() + len > kMaxBuffered) return SK_OK;  // decode() reports it (a Layer I / II stream: below)
    d->buffer.insert(d->buffer.end(), input, input + len);  // scanned in place; taken back where the call turns out to be decode()'s
    auto not_mine = [&]() {
        d->buffer.resize(d->buffer.size() - len);
        return SK_OK;
    };
    if (d->mpa_layer == 0) {
        if (d->sample_rate) {  // decode() has delivered frames: a Layer III stream (a free-format one, whose headers the scan here skips)
            d->mpa_layer = 3;
            return not_mine();
        }
        const int layer = sk_mp12::find_layer(d->buffer.data(), d->buffer.size());
        if (layer == -1) {  // a Layer I / II candidate waits for the header behind it: the bytes stay, nothing comes out yet
            *written = 0;
            *handled = true;
            return SK_OK;
        }
        // 0: no header in sight.  -3: a Layer III candidate waits; decode() takes a last frame without a header behind it, as it always
        // has, so the call is its own -- but that settles nothing: should the candidate be stray bytes in front of a Layer I / II stream,
        // the next call looks again, and the layer is that of the first CONFIRMED frame (or of the first frame decode() delivers).
        if (layer <= 0) return not_mine();
        d->mpa_layer = (uint8_t)layer;
        if (layer == 3) return not_mine();
    }
    *handled = true;
    *written = 0;
    if (d->buffer.empty()) return SK_OK;
    auto fail = [&](int rc) {  // a failed call leaves the decoder as it was
        d->buffer.resize(d->buffer.size() - len);
        return rc;
    };

    d->mpa_found.resize(d->buffer.size() / 24 + 2);
    uint32_t n_found = 0, layer = d->mpa_layer;
    size_t scanned = 0;
    int rc = sk_mp12::scan(d->buffer.data(), d->buffer.size(), &layer, d->mpa_found.data(), (uint32_t)d->mpa_found.size(), &n_found, &scanned);
    if (rc != SK_OK) return fail(rc);
    if (n_found > d->mpa_found.size()) n_found = (uint32_t)d->mpa_found.size();

    uint32_t sample_rate = d->sample_rate;
    uint8_t channels = d->channels;
    uint64_t frames = d->frames;
    d->mpa_records.clear(), d->gpu_bytes.clear();
    size_t samples = 0, consumed = 0;
    int result = SK_OK;
    bool stopped = false;
    for (uint32_t k = 0; k < n_found && !stopped; ++k) {
        const sk_mpa_frame_info &h = d->mpa_found[k];
        const uint8_t *frame = d->buffer.data() + h.offset;
        const size_t frame_samples = (size_t)h.samples_per_channel * h.channels;
        sk_mpa_frame_record rec;
        const bool decodable = sk_mp12::parse_frame(frame, h.frame_bytes, &h, &rec) == SK_OK;
        if (decodable) {
            if (samples + frame_samples > out_cap) {  // write_frame_*: "Output buffer too small for decoded frame"
                result = SK_ERR_CAPACITY;
                break;
            }
            if (!d->stream_open || d->stream_channels != h.channels) {  // the carried synthesis state belongs to a channel count
                if (!d->mpa_records.empty()) break;  // frames queued for the old stream go first; this frame waits for the next call
                uint32_t fresh = 0;  // opened before the old one goes: a failed call leaves the decoder as it was
                rc = sk_stream_open(d->engine, h.sample_rate, h.channels, &fresh);
                if (rc != SK_OK) return fail(rc);
                if (d->stream_open) (void)sk_stream_close(d->engine, d->stream);
                d->stream = fresh;
                d->stream_open = true;
                d->stream_channels = h.channels;
            }
            if (!sample_rate) sample_rate = h.sample_rate;
            if (!channels) channels = h.channels;
            const size_t at = (d->gpu_bytes.size() + 3) & ~(size_t)3;
            d->gpu_bytes.resize(at + h.frame_bytes + 8, 0);  // 8 zero bytes behind every frame
            std::memcpy(d->gpu_bytes.data() + at, frame, h.frame_bytes);
            rec.byte_offset = (uint32_t)at;
            d->mpa_records.push_back(rec);
            samples += frame_samples;
            frames += 1;
        }
        consumed = h.offset + h.frame_bytes;
        if (decodable && out_cap - samples < SK_MP3_MAX_SAMPLES_PER_FRAME) stopped = true;  // lib.rs:300-302
        if (k + 1 == n_found) consumed = scanned;  // every frame taken: garbage in front of an incomplete frame goes too
    }

    const uint32_t n = (uint32_t)d->mpa_records.size();
    if (n) {
        d->gpu_streams.assign(n, d->stream);
        d->gpu_stage_status.assign(n, 0);
        size_t got = 0;
        if (kind == Out::I16) {
            rc = sk_mpa_decode_frames_s16(d->engine, d->mpa_records.data(), d->gpu_streams.data(), n, d->gpu_bytes.data(), d->gpu_bytes.size(), (int16_t *)out,
                                          out_cap, d->gpu_stage_status.data(), &got);
        } else if (kind == Out::F32) {
            rc = sk_mpa_decode_frames_f32(d->engine, d->mpa_records.data(), d->gpu_streams.data(), n, d->gpu_bytes.data(), d->gpu_bytes.size(), (float *)out,
                                          out_cap, d->gpu_stage_status.data(), &got);
        } else {
            if (d->pcm.size() < samples) d->pcm.resize(samples);
            rc = sk_mpa_decode_frames_f32(d->engine, d->mpa_records.data(), d->gpu_streams.data(), n, d->gpu_bytes.data(), d->gpu_bytes.size(), d->pcm.data(),
                                          samples, d->gpu_stage_status.data(), &got);
            for (size_t i = 0; rc == SK_OK && i < got; ++i) ((int32_t *)out)[i] = mp3_f32_to_i32(d->pcm[i]);
        }
        if (rc != SK_OK) return fail(rc);
        // a frame the stage call rejected took no room in its output and counts for nothing
        for (uint32_t i = 0; i < n; ++i)
            if (d->gpu_stage_status[i] != SK_OK) frames -= 1;
        samples = got;
    } else if (n_found == 0) {
        consumed = scanned;
    }
    d->sample_rate = sample_rate, d->channels = channels, d->frames = frames;
    d->buffer.erase(d->buffer.begin(), d->buffer.begin() + (ptrdiff_t)consumed);
    *written = samples;
    return result;
}

const bool g_hooked = [] {
    gpu_hooks().decode_mpa = decode_mpa;
    return true;
}();

}  // namespace

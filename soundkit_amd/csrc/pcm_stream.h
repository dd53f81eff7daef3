// pcm_stream.h -- the two stream processors in front of the PCM tick: host code, no GPU.
//
//   WavStream     = WavStreamProcessor::add with install_fmt / install_ds64 (soundkit/src/wav.rs:95-324)
//   RawPcmStream  = RawPcmStreamProcessor::add / flush (soundkit/src/raw_pcm.rs:150-190)
//
// Both take a stream's bytes in whatever chunks they arrive and give back, per call, at most one PIECE: the whole PCM frames
// available now.  A piece is a contiguous range of the stream (the bytes buffered since the last piece plus part of this chunk), so
// it is described by its offset in the stream, its length and a pointer into the processor's buffer that stays valid until the next
// call.  Error texts are the reference's.  Header-only: pipeline.cpp includes it (the scheduler's link line does not change), and
// the C ABI (sk_wav_reader_*, sk_raw_pcm_framer_*) exports it so that it can be tested without a GPU.
//
// Limits: a chunk of at most 4 MiB (MAX_WAV_INPUT_CHUNK_BYTES, wav.rs:19; MAX_INPUT_CHUNK_BYTES, raw_pcm.rs), `fmt ` / `ds64`
// chunks of at most 4096 bytes (MAX_WAV_FMT_BYTES, wav.rs:20).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace sk_pcm {

constexpr size_t kMaxInputChunkBytes = 4u * 1024 * 1024;
constexpr size_t kMaxWavFmtBytes = 4096;

struct Piece {
    const uint8_t *data = nullptr;  // valid until the next add()
    size_t len = 0;                 // 0: nothing complete yet
    uint64_t stream_offset = 0;     // where the piece starts, counted over every byte ever passed to add()
};

class WavStream {
public:
    // false = error (text in `err`); the processor is finished then, as the reference's is (state left at Finished)
    bool add(const uint8_t *chunk, size_t len, Piece &piece, std::string &err) {
        piece = Piece{};
        if (len > kMaxInputChunkBytes) {
            err = "WAV input chunk exceeds the " + std::to_string(kMaxInputChunkBytes) + " byte streaming budget";
            return false;
        }
        if (pos_ > 0) {  // what earlier calls consumed goes now: the last piece's pointer was valid until here
            buf_.erase(buf_.begin(), buf_.begin() + (std::ptrdiff_t)pos_);
            base_ += pos_;
            pos_ = 0;
        }
        if (len) buf_.insert(buf_.end(), chunk, chunk + len);
        for (;;) {
            const State state = state_;
            state_ = Finished;  // std::mem::replace(&mut self.state, Finished): an error return leaves it there
            const size_t avail = buf_.size() - pos_;
            const uint8_t *b = buf_.data() + pos_;
            switch (state) {
            case Initial:
                if (avail < 12) {
                    state_ = Initial;
                    return true;
                }
                rf64_ = std::memcmp(b, "RF64", 4) == 0;
                if ((!rf64_ && std::memcmp(b, "RIFF", 4) != 0) || std::memcmp(b + 8, "WAVE", 4) != 0) {
                    err = "Not a WAV file";
                    return false;
                }
                pos_ += 12;
                state_ = ChunkHeader;
                break;
            case ChunkHeader: {
                if (avail < 8) {
                    state_ = ChunkHeader;
                    return true;
                }
                std::memcpy(kind_, b, 4);
                const uint32_t size = le32(b + 4);
                pos_ += 8;
                if (std::memcmp(kind_, "data", 4) == 0) {
                    if (bits_ == 0 || channels_ == 0 || rate_ == 0) {
                        err = "WAV data appears before a valid fmt chunk";
                        return false;
                    }
                    uint64_t data_size = size;
                    if (rf64_ && size == 0xffffffffu) {
                        if (!have_ds64_) {
                            err = "RF64 data chunk appears before a valid ds64 chunk";
                            return false;
                        }
                        data_size = rf64_data_size_;
                    }
                    data_chunk_size_ = data_size;
                    remaining_ = data_size;
                    state_ = data_size == 0 ? Finished : ReadingData;
                } else {
                    const bool meta = is_meta();
                    if (meta && size > kMaxWavFmtBytes) {
                        err = "WAV fmt chunk exceeds the " + std::to_string(kMaxWavFmtBytes) + " byte metadata budget";
                        return false;
                    }
                    remaining_ = size;
                    padding_ = (size & 1) != 0;
                    payload_.clear();
                    state_ = ChunkPayload;
                }
                break;
            }
            case ChunkPayload: {
                const size_t consumed = (size_t)(remaining_ < avail ? remaining_ : avail);
                const bool meta = is_meta();
                if (meta) payload_.insert(payload_.end(), b, b + consumed);
                pos_ += consumed;
                remaining_ -= consumed;
                if (remaining_ > 0) {
                    state_ = ChunkPayload;
                    return true;
                }
                if (padding_) {
                    if (buf_.size() == pos_) {
                        state_ = ChunkPayload;
                        return true;
                    }
                    pos_ += 1;
                    padding_ = false;
                }
                if (std::memcmp(kind_, "fmt ", 4) == 0) {
                    if (!install_fmt(err)) return false;
                } else if (std::memcmp(kind_, "ds64", 4) == 0) {
                    if (!install_ds64(err)) return false;
                }
                state_ = ChunkHeader;
                break;
            }
            case ReadingData: {
                const size_t frame = (size_t)(bits_ / 8) * channels_;
                if (frame == 0) {
                    err = "WAV fmt has zero bytes per frame";
                    return false;
                }
                const size_t available = (size_t)(remaining_ < avail ? remaining_ : avail);
                const size_t n = available / frame * frame;
                if (n == 0) {
                    if ((uint64_t)avail >= remaining_ && remaining_ > 0) {
                        err = "WAV data chunk is not frame-aligned";
                        return false;
                    }
                    state_ = ReadingData;
                    return true;  // wait for more data
                }
                piece.data = b;
                piece.len = n;
                piece.stream_offset = base_ + pos_;
                pos_ += n;
                remaining_ -= n;
                state_ = remaining_ == 0 ? Finished : ReadingData;
                return true;
            }
            case Finished:  // whatever follows the data chunk is ignored
                state_ = Finished;
                return true;
            }
        }
    }

    uint32_t sample_rate() const { return rate_; }
    uint32_t channels() const { return channels_; }
    uint32_t bits() const { return bits_; }
    bool is_float() const { return float_; }
    // total_frames (wav.rs:86-93): 0 = not known (no data chunk header yet, or an empty one)
    uint64_t total_frames() const {
        const uint64_t frame = (uint64_t)(bits_ / 8) * channels_;
        return frame == 0 || data_chunk_size_ == 0 ? 0 : data_chunk_size_ / frame;
    }

private:
    enum State { Initial, ChunkHeader, ChunkPayload, ReadingData, Finished };
    static uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
    static uint32_t le32(const uint8_t *p) { return le16(p) | (le16(p + 2) << 16); }
    static uint64_t le64(const uint8_t *p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }
    bool is_meta() const { return std::memcmp(kind_, "fmt ", 4) == 0 || std::memcmp(kind_, "ds64", 4) == 0; }

    bool install_fmt(std::string &err) {
        const std::vector<uint8_t> &p = payload_;
        if (p.size() < 16) {
            err = "WAV fmt chunk must contain at least 16 bytes";
            return false;
        }
        uint32_t format = le16(p.data());
        if (format == 0xfffe) {
            if (p.size() < 40) {
                err = "WAVE_FORMAT_EXTENSIBLE fmt chunk is truncated";
                return false;
            }
            format = le16(p.data() + 24);
        }
        channels_ = le16(p.data() + 2);
        rate_ = le32(p.data() + 4);
        bits_ = le16(p.data() + 14);
        if (format == 1) {
            float_ = false;
        } else if (format == 3) {
            float_ = true;
        } else {
            err = "unsupported WAV format tag " + std::to_string(format);
            return false;
        }
        if (channels_ == 0 || rate_ == 0 || bits_ == 0) {
            err = "WAV fmt contains invalid audio geometry";
            return false;
        }
        if (bits_ % 8 != 0) {
            err = "WAV sample width must be byte-aligned";
            return false;
        }
        return true;
    }

    bool install_ds64(std::string &err) {
        const std::vector<uint8_t> &p = payload_;
        if (!rf64_) {
            err = "ds64 chunk requires an RF64 header";
            return false;
        }
        if (p.size() < 28) {
            err = "RF64 ds64 chunk is truncated";
            return false;
        }
        const uint64_t data_size = le64(p.data() + 8);
        const uint64_t table_length = le32(p.data() + 24);
        if ((uint64_t)p.size() < 28 + table_length * 12) {  // (no overflow in 64 bits: table_length < 2^32)
            err = "RF64 ds64 table is truncated";
            return false;
        }
        rf64_data_size_ = data_size;
        have_ds64_ = true;
        return true;
    }

    State state_ = Initial;
    std::vector<uint8_t> buf_, payload_;
    size_t pos_ = 0;     // consumed prefix of buf_
    uint64_t base_ = 0;  // stream offset of buf_[0]
    uint8_t kind_[4] = {0, 0, 0, 0};
    uint64_t remaining_ = 0;
    bool padding_ = false;
    uint32_t bits_ = 0, channels_ = 0, rate_ = 0;
    bool float_ = false, rf64_ = false, have_ds64_ = false;
    uint64_t rf64_data_size_ = 0, data_chunk_size_ = 0;
};

class RawPcmStream {
public:
    explicit RawPcmStream(size_t bytes_per_frame) : frame_(bytes_per_frame) {}

    bool add(const uint8_t *chunk, size_t len, Piece &piece, std::string &err) {
        piece = Piece{};
        if (len > kMaxInputChunkBytes) {
            err = "raw PCM input chunk exceeds the " + std::to_string(kMaxInputChunkBytes) + " byte streaming budget";
            return false;
        }
        if (pos_ > 0) {
            buf_.erase(buf_.begin(), buf_.begin() + (std::ptrdiff_t)pos_);
            base_ += pos_;
            pos_ = 0;
        }
        if (len) buf_.insert(buf_.end(), chunk, chunk + len);
        if (frame_ == 0) {
            err = "Raw PCM bytes per frame must be > 0";
            return false;
        }
        const size_t n = buf_.size() / frame_ * frame_;
        if (n == 0) return true;
        piece.data = buf_.data();
        piece.len = n;
        piece.stream_offset = base_;
        pos_ = n;
        return true;
    }

    // end of stream: false (and the reference's text) when a partial frame is left
    bool flush(std::string &err) const {
        const size_t left = buf_.size() - pos_;
        if (left == 0) return true;
        err = "Raw PCM stream ended with " + std::to_string(left) + " trailing partial-frame byte(s)";
        return false;
    }

    size_t buffered() const { return buf_.size() - pos_; }

private:
    size_t frame_;
    std::vector<uint8_t> buf_;
    size_t pos_ = 0;
    uint64_t base_ = 0;
};

}  // namespace sk_pcm

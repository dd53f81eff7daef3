// pcm_stream.h -- the two stream processors in front of the PCM tick: host code, no GPU.
//
//   WavStream     = WavStreamProcessor::add with install_fmt / install_ds64 (soundkit/src/wav.rs:95-324); WavStream(true), the coded
//                   mode, is this project's own: the same walk, and four more format tags (see the class)
//   RawPcmStream  = RawPcmStreamProcessor::add / flush (soundkit/src/raw_pcm.rs:150-190)
//   AiffStream    = AiffDecoder::add without its per-sample work (soundkit-aiff/src/lib.rs:93-475); see the class
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
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

// The coded mode (WavStream(true); sk_wav_coded_reader_*): a decision beyond the reference, whose WavStreamProcessor is the default
// mode bit for bit.  The chunk walk, the budgets and every text of the default mode stay; the fmt installer additionally takes
//   6 / 7   A-law / mu-law: 8 bits per sample, a frame is `channels` bytes, pieces are whole frames
//   0x11    IMA / DVI ADPCM, 2 Microsoft ADPCM: 4 bits per sample, 1 or 2 channels, pieces are whole blocks of nBlockAlign bytes
// and a `fact` chunk in front of `data` is kept (the metadata budget bounds it): its dwSampleLength caps total_frames() of the two
// ADPCM tags, so the padding samples of a last block can be cut; absent, zero or larger than what the blocks hold it is ignored.
// Not taken: the coded tags inside WAVE_FORMAT_EXTENSIBLE, ADPCM with more than two channels, every other tag.
constexpr uint32_t kWavTagPcm = 1, kWavTagMsAdpcm = 2, kWavTagFloat = 3, kWavTagAlaw = 6, kWavTagUlaw = 7, kWavTagImaAdpcm = 0x11;
constexpr uint32_t kMaxWavAdpcmBlockFrames = 65536;
constexpr uint32_t kMaxWavAdpcmCoefs = 32;

// frames of one ADPCM block; 0 where the block size is no block of the tag (the walker's rules, shared with the decode stage)
inline uint32_t wav_adpcm_block_frames(uint32_t tag, uint32_t channels, uint32_t block_align) {
    if (channels < 1 || channels > 2) return 0;
    if (tag == kWavTagImaAdpcm) return block_align < 4 * channels || block_align % (4 * channels) ? 0 : (block_align - 4 * channels) * 2 / channels + 1;
    if (tag == kWavTagMsAdpcm) return block_align < 7 * channels ? 0 : (block_align - 7 * channels) * 2 / channels + 2;
    return 0;
}

class WavStream {
public:
    explicit WavStream(bool coded = false) : coded_(coded) {}

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
                } else if (std::memcmp(kind_, "fact", 4) == 0) {
                    if (coded_ && payload_.size() >= 4) fact_frames_ = le32(payload_.data());
                } else if (std::memcmp(kind_, "ds64", 4) == 0) {
                    if (!install_ds64(err)) return false;
                }
                state_ = ChunkHeader;
                break;
            }
            case ReadingData: {
                const size_t frame = (size_t)frame_bytes();
                if (frame == 0) {
                    err = "WAV fmt has zero bytes per frame";
                    return false;
                }
                const size_t available = (size_t)(remaining_ < avail ? remaining_ : avail);
                const size_t n = available / frame * frame;
                if (n == 0) {
                    if ((uint64_t)avail >= remaining_ && remaining_ > 0) {
                        err = is_adpcm() ? "WAV data chunk is not block-aligned" : "WAV data chunk is not frame-aligned";
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
        const uint64_t frame = frame_bytes();
        if (frame == 0 || data_chunk_size_ == 0) return 0;
        if (!is_adpcm()) return data_chunk_size_ / frame;
        const uint64_t held = data_chunk_size_ / frame * frames_per_block_;  // the fact chunk's count where it cuts, else what the blocks hold
        return fact_frames_ != 0 && fact_frames_ <= held ? fact_frames_ : held;
    }
    // the coded mode's description (the default mode: tag 1 or 3, the rest zero)
    uint32_t tag() const { return tag_; }
    uint32_t block_align() const { return is_adpcm() ? block_align_ : (uint32_t)frame_bytes(); }
    uint32_t frames_per_block() const { return is_adpcm() ? frames_per_block_ : (frame_bytes() ? 1 : 0); }
    uint32_t n_coef() const { return n_coef_; }
    const int16_t (*coef() const)[2] { return coef_; }
    uint32_t fact_frames() const { return fact_frames_; }
    bool is_adpcm() const { return tag_ == kWavTagMsAdpcm || tag_ == kWavTagImaAdpcm; }

private:
    enum State { Initial, ChunkHeader, ChunkPayload, ReadingData, Finished };
    static uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
    static uint32_t le32(const uint8_t *p) { return le16(p) | (le16(p + 2) << 16); }
    static uint64_t le64(const uint8_t *p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }
    bool is_meta() const {
        return std::memcmp(kind_, "fmt ", 4) == 0 || std::memcmp(kind_, "ds64", 4) == 0 || (coded_ && std::memcmp(kind_, "fact", 4) == 0);
    }
    uint64_t frame_bytes() const { return is_adpcm() ? block_align_ : (uint64_t)(bits_ / 8) * channels_; }

    bool install_fmt(std::string &err) {
        const std::vector<uint8_t> &p = payload_;
        if (p.size() < 16) {
            err = "WAV fmt chunk must contain at least 16 bytes";
            return false;
        }
        uint32_t format = le16(p.data());
        const bool coded_tag = coded_ && (format == kWavTagMsAdpcm || format == kWavTagAlaw || format == kWavTagUlaw || format == kWavTagImaAdpcm);
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
        } else if (coded_tag) {
            float_ = false;
        } else {
            err = "unsupported WAV format tag " + std::to_string(format);
            return false;
        }
        if (channels_ == 0 || rate_ == 0 || bits_ == 0) {
            err = "WAV fmt contains invalid audio geometry";
            return false;
        }
        tag_ = format, block_align_ = frames_per_block_ = n_coef_ = 0;
        if (coded_tag) return install_coded(err);
        if (bits_ % 8 != 0) {
            err = "WAV sample width must be byte-aligned";
            return false;
        }
        return true;
    }

    // the four tags of the coded mode (an error finishes the walker, as every other does)
    bool install_coded(std::string &err) {
        const std::vector<uint8_t> &p = payload_;
        const uint32_t bits = bits_, channels = channels_;
        if (tag_ == kWavTagAlaw || tag_ == kWavTagUlaw) {
            if (bits != 8) {
                err = "WAV G.711 requires 8 bits per sample, found " + std::to_string(bits);
                return false;
            }
            return true;
        }
        const bool ima = tag_ == kWavTagImaAdpcm;
        if (bits != 4) {
            err = "WAV ADPCM requires 4 bits per sample, found " + std::to_string(bits);
            return false;
        }
        if (channels > 2) {
            err = "WAV ADPCM with " + std::to_string(channels) + " channels is not built: mono and stereo are";
            return false;
        }
        const uint32_t align = le16(p.data() + 12);
        const uint32_t frames = wav_adpcm_block_frames(tag_, channels, align);
        if (frames == 0) {
            err = std::string(ima ? "WAV IMA ADPCM" : "WAV MS ADPCM") + " block size " + std::to_string(align) + " is invalid for " + std::to_string(channels) + " channels";
            return false;
        }
        if (frames > kMaxWavAdpcmBlockFrames) {
            err = "WAV ADPCM block of " + std::to_string(frames) + " samples exceeds the " + std::to_string(kMaxWavAdpcmBlockFrames) + " sample budget";
            return false;
        }
        const uint32_t cb = p.size() >= 18 ? le16(p.data() + 16) : 0;
        if (!ima && (p.size() < 22 || cb < 4)) {  // wSamplesPerBlock and wNumCoef are not optional here
            err = "WAV MS ADPCM fmt chunk is truncated";
            return false;
        }
        if (cb >= 2) {
            if (p.size() < 20) {
                err = "WAV IMA ADPCM fmt chunk is truncated";
                return false;
            }
            const uint32_t declared = le16(p.data() + 18);
            if (declared != frames) {
                err = "WAV ADPCM fmt declares " + std::to_string(declared) + " samples per block, the block holds " + std::to_string(frames);
                return false;
            }
        }
        if (!ima) {
            const uint32_t n = le16(p.data() + 20);
            if (n < 1 || n > kMaxWavAdpcmCoefs) {
                err = "WAV MS ADPCM fmt declares " + std::to_string(n) + " coefficient sets: 1 to " + std::to_string(kMaxWavAdpcmCoefs) + " are read";
                return false;
            }
            if (p.size() < 22 + (size_t)4 * n || cb < 4 + 4 * n) {
                err = "WAV MS ADPCM fmt chunk is truncated";
                return false;
            }
            for (uint32_t i = 0; i < n; ++i)
                for (int k = 0; k < 2; ++k) coef_[i][k] = (int16_t)le16(p.data() + 22 + 4 * i + 2 * k);
            n_coef_ = n;
        }
        block_align_ = align, frames_per_block_ = frames;
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
    // the coded mode
    const bool coded_;
    uint32_t tag_ = 0, block_align_ = 0, frames_per_block_ = 0, n_coef_ = 0, fact_frames_ = 0;
    int16_t coef_[kMaxWavAdpcmCoefs][2] = {};
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

// AiffStream = AiffDecoder::add / parse_available / parse_stream_info / parse_extended_sample_rate (soundkit-aiff/src/lib.rs:93-475)
// up to, and without, decode_stream_bytes: one add gives at most one piece of whole SOURCE-ENCODED sample groups (a sample; for IMA4
// 34 bytes per channel) and the stream's description; the per-sample work is the tick's (aiff_decode.hip).  A piece may join the
// retained incomplete group with this chunk's bytes, so it lives in a buffer of its own; its stream_offset counts sound bytes.
// An empty add is the finalising one.  After an error every further add repeats it.
enum AiffEncoding : uint8_t {  // = enum sk_aiff_encoding
    kAiffU8, kAiffS8, kAiffS16BE, kAiffS16LE, kAiffS24BE, kAiffS32BE, kAiffS32LE, kAiffF32BE, kAiffF64BE, kAiffUlaw, kAiffAlaw, kAiffIma4,
    kAiffUnassigned12,  // refused, as every unknown value is (aiff_encoding_known)
    kAiffF64LE,  // = 13; container PCM (QuickTime `fl64` with enda = 1, CAF lpcm flags 3); no AIFF-C compression type names it
    kAiffDvdS24,  // = 14; DVD LPCM at 24 bits (MPEG program streams): 12-byte groups of four samples, high parts first
    kAiffEncodings
};
constexpr size_t kMaxAiffCommBytes = 4096;
constexpr uint32_t kMaxAiffChannels = 32;

inline bool aiff_encoding_known(int enc) { return enc >= 0 && enc < kAiffEncodings && enc != kAiffUnassigned12; }

// bytes of one encoded sample group, and of what it decodes to (the output contract, lib.rs:41-54)
inline size_t aiff_group_bytes(int enc, uint32_t channels) {
    switch (enc) {
    case kAiffU8: case kAiffS8: case kAiffUlaw: case kAiffAlaw: return 1;
    case kAiffS16BE: case kAiffS16LE: return 2;
    case kAiffS24BE: return 3;
    case kAiffS32BE: case kAiffS32LE: case kAiffF32BE: return 4;
    case kAiffF64BE: case kAiffF64LE: return 8;
    case kAiffDvdS24: return 12;  // four samples
    default: return (size_t)34 * channels;
    }
}
inline uint32_t aiff_contract_bits(int enc) { return enc == kAiffS24BE || enc == kAiffDvdS24 ? 24 : ((enc >= kAiffS32BE && enc <= kAiffF64BE) || enc == kAiffF64LE ? 32 : 16); }
inline bool aiff_contract_float(int enc) { return enc == kAiffF32BE || enc == kAiffF64BE || enc == kAiffF64LE; }
inline size_t aiff_group_out_bytes(int enc, uint32_t channels) {
    return enc == kAiffIma4 ? (size_t)128 * channels : (enc == kAiffDvdS24 ? 12 : aiff_contract_bits(enc) / 8);
}
inline uint32_t aiff_group_samples(int enc) { return enc == kAiffDvdS24 ? 4 : 1; }  // samples the elementwise kernel counts per group

class AiffStream {
public:
    bool add(const uint8_t *chunk, size_t len, Piece &piece, std::string &err) {
        piece = Piece{};
        if (failed_) {
            err = error_;
            return false;
        }
        if (finished_) return true;
        if (len > kMaxInputChunkBytes) {  // (the reference's decoder stays usable after this one; so does this)
            err = "AIFF input chunk exceeds the " + std::to_string(kMaxInputChunkBytes) + " byte streaming budget";
            return false;
        }
        audio_base_ += out_.size();
        out_.clear();
        if (len) buf_.insert(buf_.end(), chunk, chunk + len);
        if (!parse_available(err)) return fail(err);
        if (len == 0) {
            if (state_ != Done) return fail(err = "truncated AIFF stream in state " + debug_state());
            if (!pending_.empty()) return fail(err = "AIFF sound data ends inside an encoded sample group");
            finished_ = true;
        }
        if (out_.empty()) return true;
        if (!have_info_) return fail(err = "AIFF PCM arrived before COMM metadata");
        piece.data = out_.data();
        piece.len = out_.size();
        piece.stream_offset = audio_base_;
        return true;
    }

    size_t buffered_bytes() const { return buf_.size() + pending_.size(); }
    bool have_info() const { return have_info_; }
    uint32_t sample_rate() const { return rate_; }
    uint32_t channels() const { return channels_; }
    int encoding() const { return enc_; }
    uint32_t bits() const { return have_info_ ? aiff_contract_bits(enc_) : 0; }
    bool is_float() const { return have_info_ && aiff_contract_float(enc_); }

private:
    enum State { FormHeader, ChunkHeader, Comm, SsndHeader, SsndOffset, Audio, Skip, Padding, Done };
    static uint32_t be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
    static uint32_t be32(const uint8_t *p) { return (be16(p) << 16) | be16(p + 2); }
    static std::string lossy4(const uint8_t *p) {  // String::from_utf8_lossy of four bytes
        std::string s;
        for (int i = 0; i < 4;) {
            const uint8_t c = p[i];
            int n = c < 0x80 ? 1 : (c >= 0xc2 && c <= 0xdf ? 2 : (c >= 0xe0 && c <= 0xef ? 3 : (c >= 0xf0 && c <= 0xf4 ? 4 : 0)));
            bool ok = n > 0;
            int have = 1;  // bytes of the maximal valid prefix of this sequence (one U+FFFD replaces it)
            if (n > 1) {
                for (int k = 1; k < n; ++k) {
                    if (i + k >= 4) { ok = false; break; }
                    const uint8_t d = p[i + k];
                    uint8_t lo = 0x80, hi = 0xbf;
                    if (k == 1) {
                        if (c == 0xe0) lo = 0xa0;
                        if (c == 0xed) hi = 0x9f;
                        if (c == 0xf0) lo = 0x90;
                        if (c == 0xf4) hi = 0x8f;
                    }
                    if (d < lo || d > hi) { ok = false; break; }
                    have += 1;
                }
            }
            if (ok) {
                s.append((const char *)p + i, (size_t)n);
                i += n;
            } else {
                s += "\xef\xbf\xbd";
                i += have;
            }
        }
        return s;
    }
    bool fail(const std::string &text) {
        failed_ = true;
        error_ = text;
        return false;
    }
    static const char *tf(bool b) { return b ? "true" : "false"; }
    std::string debug_state() const {  // {:?} of ParseState
        const std::string pad = std::string(", padded: ") + tf(padded_) + " }";
        switch (state_) {
        case FormHeader: return "FormHeader";
        case ChunkHeader: return "ChunkHeader";
        case Comm: return "Comm { size: " + std::to_string(remaining_) + pad;
        case SsndHeader: return "SsndHeader { remaining: " + std::to_string(remaining_) + pad;
        case SsndOffset: return "SsndOffset { skip: " + std::to_string(skip_) + ", remaining_audio: " + std::to_string(remaining_) + pad;
        case Audio: return "Audio { remaining: " + std::to_string(remaining_) + pad;
        case Skip: return "Skip { remaining: " + std::to_string(remaining_) + pad;
        case Padding: return "Padding";
        default: return "Done";
        }
    }
    bool consume_form(uint64_t n, std::string &err) {
        if (n > form_remaining_) {
            err = "AIFF parser crossed the FORM boundary";
            return false;
        }
        form_remaining_ -= n;
        return true;
    }
    State next_chunk_state() const { return form_remaining_ == 0 ? Done : ChunkHeader; }
    void finish_chunk(bool padded) {
        const State next = next_chunk_state();
        if (padded) padding_next_ = next, state_ = Padding;
        else state_ = next;
    }

    // {value} of an f64 as Rust's Display prints it: the shortest digits that read back, never an exponent
    static std::string display_f64(double v) {
        if (v != v) return "NaN";
        if (v == HUGE_VAL) return "inf";
        if (v == 0) return "0";
        char text[40];
        int prec = 0;
        for (; prec < 17; ++prec) {
            std::snprintf(text, sizeof text, "%.*e", prec, v);
            if (std::strtod(text, nullptr) == v) break;
        }
        std::string digits;
        const char *e = std::strchr(text, 'e');
        for (const char *p = text; p < e; ++p)
            if (*p != '.') digits += *p;
        const int exp10 = std::atoi(e + 1);  // value = d.ddd * 10^exp10
        while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
        std::string s;
        if (exp10 < 0) {
            s = "0." + std::string((size_t)(-exp10 - 1), '0') + digits;
        } else if ((size_t)exp10 + 1 >= digits.size()) {
            s = digits + std::string((size_t)exp10 + 1 - digits.size(), '0');
        } else {
            s = digits.substr(0, (size_t)exp10 + 1) + "." + digits.substr((size_t)exp10 + 1);
        }
        return s;
    }

    bool parse_rate(const uint8_t *d, std::string &err) {  // parse_extended_sample_rate + parse_sample_rate
        const uint32_t exponent_word = be16(d);
        if (exponent_word & 0x8000) {
            err = "AIFF sample rate is negative";
            return false;
        }
        const uint32_t exponent = exponent_word & 0x7fff;
        const uint64_t mantissa = ((uint64_t)be32(d + 2) << 32) | be32(d + 6);
        if (exponent == 0 && mantissa == 0) {
            err = "AIFF sample rate is zero";
            return false;
        }
        if (exponent == 0x7fff) {
            err = "AIFF sample rate is not finite";
            return false;
        }
        // 2f64.powi(n): exact powers of two by repeated multiplication, and 1 / 2^-n for n < 0 -- inf beyond 2^1023, so 0 below 2^-1023
        const int n = (int)exponent - 16383 - 63;
        const double scale = n > 1023 ? HUGE_VAL : (n < -1023 ? 0.0 : std::ldexp(1.0, n));
        const double value = (double)mantissa * scale;
        if (!(value == value) || value == HUGE_VAL || value <= 0.0 || value > 4294967295.0) {
            err = "Invalid AIFF sample rate: " + display_f64(value);
            return false;
        }
        rate_ = (uint32_t)std::round(value);
        return true;
    }

    bool parse_stream_info(const uint8_t *d, size_t n, std::string &err) {
        if (n < 18) {
            err = "AIFF COMM is shorter than 18 bytes";
            return false;
        }
        const uint32_t channels = be16(d);
        if (channels < 1 || channels > kMaxAiffChannels) {
            err = "invalid AIFF channel count: " + std::to_string(channels);
            return false;
        }
        const uint32_t sample_size = be16(d + 6);
        if (!parse_rate(d + 8, err)) return false;
        int enc = -1;
        auto signed_be = [&]() {
            if (sample_size >= 1 && sample_size <= 8) enc = kAiffS8;
            else if (sample_size <= 16 && sample_size >= 9) enc = kAiffS16BE;
            else if (sample_size <= 24 && sample_size >= 17) enc = kAiffS24BE;
            else if (sample_size <= 32 && sample_size >= 25) enc = kAiffS32BE;
            else err = "unsupported AIFF sample size: " + std::to_string(sample_size);
            return enc >= 0;
        };
        if (!aifc_) {
            if (!signed_be()) return false;
        } else {
            if (n < 22) {
                err = "AIFF-C COMM has no compression type";
                return false;
            }
            static const struct { const char *tag; int enc; } tags[] = {
                {"raw ", kAiffU8}, {"twos", kAiffS16BE}, {"sowt", kAiffS16LE}, {"in24", kAiffS24BE}, {"in32", kAiffS32BE}, {"23ni", kAiffS32LE},
                {"FL32", kAiffF32BE}, {"fl32", kAiffF32BE}, {"FL64", kAiffF64BE}, {"fl64", kAiffF64BE}, {"ULAW", kAiffUlaw}, {"ulaw", kAiffUlaw},
                {"ALAW", kAiffAlaw}, {"alaw", kAiffAlaw}, {"ima4", kAiffIma4}};
            if (std::memcmp(d + 18, "NONE", 4) == 0) {
                if (!signed_be()) return false;
            } else {
                for (const auto &t : tags)
                    if (std::memcmp(d + 18, t.tag, 4) == 0) enc = t.enc;
                if (enc < 0) {
                    err = "unsupported AIFF-C compression type: " + lossy4(d + 18);
                    return false;
                }
            }
        }
        if (enc == kAiffIma4 && channels > 2) {
            err = "AIFF-C IMA4 supports at most two channels";
            return false;
        }
        channels_ = channels, enc_ = enc, have_info_ = true;
        return true;
    }

    // the sound bytes of one Audio step: whole groups go to the piece, the incomplete last one is retained
    void take_audio(const uint8_t *p, size_t n) {
        const size_t group = aiff_group_bytes(enc_, channels_);
        if (!pending_.empty()) {
            const size_t need = group - pending_.size();
            const size_t k = n < need ? n : need;
            pending_.insert(pending_.end(), p, p + k);
            p += k, n -= k;
            if (pending_.size() < group) return;
            out_.insert(out_.end(), pending_.begin(), pending_.end());
            pending_.clear();
        }
        const size_t whole = n / group * group;
        out_.insert(out_.end(), p, p + whole);
        pending_.assign(p + whole, p + n);
    }

    bool parse_available(std::string &err) {
        size_t position = 0;
        for (;;) {
            const size_t available = buf_.size() - position;
            const uint8_t *b = buf_.data() + position;
            bool stop = false;
            switch (state_) {
            case FormHeader: {
                if (available < 12) { stop = true; break; }
                if (std::memcmp(b, "FORM", 4) != 0) {
                    err = "AIFF stream does not start with FORM";
                    return false;
                }
                const uint32_t form_size = be32(b + 4);
                if (form_size < 4) {
                    err = "AIFF FORM is shorter than its type field";
                    return false;
                }
                if (std::memcmp(b + 8, "AIFF", 4) == 0) aifc_ = false;
                else if (std::memcmp(b + 8, "AIFC", 4) == 0) aifc_ = true;
                else {
                    err = "unsupported FORM type " + lossy4(b + 8);
                    return false;
                }
                form_remaining_ = form_size - 4;
                position += 12;
                state_ = next_chunk_state();
                break;
            }
            case ChunkHeader: {
                if (form_remaining_ == 0) { state_ = Done; break; }
                if (form_remaining_ < 8) {
                    err = "AIFF FORM ends inside a chunk header";
                    return false;
                }
                if (available < 8) { stop = true; break; }
                const uint32_t size = be32(b + 4);
                if (!consume_form(8, err)) return false;
                position += 8;
                const bool padded = (size & 1) != 0;
                if ((uint64_t)size + (padded ? 1 : 0) > form_remaining_) {
                    err = "AIFF chunk " + lossy4(b) + " exceeds the FORM boundary";
                    return false;
                }
                padded_ = padded;
                remaining_ = size;
                if (std::memcmp(b, "COMM", 4) == 0) {
                    if (size > kMaxAiffCommBytes) {
                        err = "AIFF COMM exceeds the " + std::to_string(kMaxAiffCommBytes) + " byte budget";
                        return false;
                    }
                    state_ = Comm;
                } else if (std::memcmp(b, "SSND", 4) == 0) {
                    if (size < 8) {
                        err = "AIFF SSND is shorter than its header";
                        return false;
                    }
                    if (!have_info_) {
                        err = "AIFF SSND appears before COMM";
                        return false;
                    }
                    state_ = SsndHeader;
                } else {
                    state_ = Skip;
                }
                break;
            }
            case Comm: {
                const size_t size = (size_t)remaining_;
                if (available < size) { stop = true; break; }
                if (!parse_stream_info(b, size, err)) return false;
                if (!consume_form(size, err)) return false;
                position += size;
                finish_chunk(padded_);
                break;
            }
            case SsndHeader: {
                if (available < 8) { stop = true; break; }
                const uint64_t offset = be32(b);
                const uint64_t audio_and_offset = remaining_ - 8;
                if (offset > audio_and_offset) {
                    err = "AIFF SSND offset exceeds its chunk";
                    return false;
                }
                if (!consume_form(8, err)) return false;
                position += 8;
                skip_ = offset;
                remaining_ = audio_and_offset - offset;
                state_ = SsndOffset;
                break;
            }
            case SsndOffset: {
                const size_t take = (size_t)((uint64_t)available < skip_ ? available : skip_);
                position += take;
                if (!consume_form(take, err)) return false;
                skip_ -= take;
                if (skip_ == 0) state_ = Audio;
                else stop = true;
                break;
            }
            case Audio: {
                const size_t take = (size_t)((uint64_t)available < remaining_ ? available : remaining_);
                take_audio(b, take);
                position += take;
                if (!consume_form(take, err)) return false;
                remaining_ -= take;
                if (remaining_ == 0) {
                    if (!pending_.empty()) {
                        err = "AIFF SSND ends inside an encoded sample group";
                        return false;
                    }
                    finish_chunk(padded_);
                } else {
                    stop = true;
                }
                break;
            }
            case Skip: {
                const size_t take = (size_t)((uint64_t)available < remaining_ ? available : remaining_);
                position += take;
                if (!consume_form(take, err)) return false;
                remaining_ -= take;
                if (remaining_ == 0) finish_chunk(padded_);
                else stop = true;
                break;
            }
            case Padding:
                if (available == 0) { stop = true; break; }
                position += 1;
                if (!consume_form(1, err)) return false;
                state_ = padding_next_;
                break;
            case Done:
                if (available != 0) {
                    err = "AIFF stream has bytes after the FORM boundary";
                    return false;
                }
                stop = true;
                break;
            }
            if (stop) break;
        }
        buf_.erase(buf_.begin(), buf_.begin() + (std::ptrdiff_t)position);
        return true;
    }

    State state_ = FormHeader, padding_next_ = ChunkHeader;
    std::vector<uint8_t> buf_, pending_, out_;
    uint64_t form_remaining_ = 0, remaining_ = 0, skip_ = 0, audio_base_ = 0;
    bool padded_ = false, aifc_ = false, have_info_ = false, finished_ = false, failed_ = false;
    uint32_t rate_ = 0, channels_ = 0;
    int enc_ = 0;
    std::string error_;
};

}  // namespace sk_pcm

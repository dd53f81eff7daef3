"""Writes AVI files for the tests: RIFF chunks, LISTs, forms, `hdrl` with `strl` lists, `movi` with interleaved `##dc` / `##wb` chunks,
`LIST rec `, OpenDML `AVIX` forms, and the files tests/test_avi_*.py demux and decode.  The audio comes from tests/golden/."""
import os
import struct

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(*path):
    with open(os.path.join(GOLDEN, *path), "rb") as f:
        return f.read()


def chunk(fourcc, payload, size=None):
    """id, little-endian size (`size` lies), payload, the pad byte behind an odd payload"""
    return fourcc + struct.pack("<I", len(payload) if size is None else size) + payload + (b"\x00" if len(payload) & 1 else b"")


def lst(kind, *children, size=None):
    return chunk(b"LIST", kind + b"".join(children), size)


def riff(form, *children, size=None):
    body = form + b"".join(children)
    return b"RIFF" + struct.pack("<I", len(body) if size is None else size) + body + (b"\x00" if len(body) & 1 else b"")


def waveformat(tag, channels, rate, bits, extra=b""):
    align = channels * ((bits + 7) // 8)
    return struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, bits) + extra


def strl(fcc, strf, with_strf=True):
    return lst(b"strl", chunk(b"strh", fcc + bytes(52)), *([chunk(b"strf", strf)] if with_strf else []))


def video_strl():
    return strl(b"vids", struct.pack("<IiiHHIIiiII", 40, 16, 16, 1, 24, 0, 768, 0, 0, 0, 0))


def hdrl(*strls):
    return lst(b"hdrl", chunk(b"avih", bytes(56)), *strls)


def wb(index, payload):
    return chunk(b"%02dwb" % index, payload)


def dc(index, n=50, fill=0xE5):
    return chunk(b"%02ddc" % index, bytes([fill]) * n)


def split(data, sizes):
    """data cut into pieces of the sizes in turn (cycled)"""
    out, at, k = [], 0, 0
    while at < len(data):
        out.append(data[at:at + sizes[k % len(sizes)]])
        at += len(out[-1])
        k += 1
    return out


def interleaved(pieces, audio_index, video_index=None):
    """the `movi` children: a video chunk in front of every audio chunk where there is a video stream"""
    out = []
    for k, p in enumerate(pieces):
        if video_index is not None:
            out.append(dc(video_index, 30 + (k % 5)))
        out.append(wb(audio_index, p))
    return out


def avi(fmt, pieces, audio_index=1, extra_forms=(), movi=None, index=True):
    """a whole file: `hdrl` with a video stream and the audio stream (audio_index 0: audio first), `movi`, an `idx1`"""
    strls = [strl(b"auds", fmt), video_strl()] if audio_index == 0 else [video_strl(), strl(b"auds", fmt)]
    children = movi if movi is not None else interleaved(pieces, audio_index, 1 - audio_index)
    return riff(b"AVI ", hdrl(*strls), chunk(b"JUNK", bytes(13)), lst(b"movi", *children), *([chunk(b"idx1", bytes(32))] if index else [])) + b"".join(extra_forms)


# ---- what the golden files hold ----------------------------------------------------------------------------------------------------------

def wav_data(name):
    """the `data` chunk of a golden WAV file"""
    d = golden(name)
    at = 12
    while at + 8 <= len(d):
        size = struct.unpack_from("<I", d, at + 4)[0]
        if d[at:at + 4] == b"data":
            return d[at + 8:at + 8 + size]
        at += 8 + size + (size & 1)
    raise ValueError(name)


FRAMES = 6000  # of every PCM source: more than one run of 4096 frames, more than one resampler chunk
S16 = golden("linear16_A_Tusk.s16le")[:FRAMES * 2]            # mono, 16 kHz
S16_STEREO = wav_data("wav_stereo_A_Tusk.wav")[:FRAMES * 4]    # stereo, 16 kHz
S24 = wav_data("wav_24_A_Tusk.wav")[:FRAMES * 3]               # mono, 16 kHz
F32 = wav_data("wav_32f_A_Tusk.wav")[:FRAMES * 4]              # mono, 16 kHz
S16_48K = golden("linear16_48k_A_Tusk.s16le")[:3 * FRAMES * 2]  # mono, 48 kHz
U8 = bytes(((s >> 8) + 128) & 0xFF for (s,) in struct.iter_unpack("<h", S16))  # the 16-bit source's high bytes, offset binary
MP3 = golden("mp3", "mono16k_A_Tusk.mp3")


def cases():
    """name -> (file, format tag, channels, rate, bits, stream index, the track's bytes)"""
    out = {}

    def add(name, data, tag, channels, rate, bits, index, track):
        out[name] = (data, tag, channels, rate, bits, index, track)

    add("pcm16_stereo", avi(waveformat(1, 2, 16000, 16), split(S16_STEREO, [4000, 1600])), 1, 2, 16000, 16, 1, S16_STEREO)
    add("pcm16_audio_first", avi(waveformat(1, 1, 16000, 16), split(S16, [2048]), audio_index=0), 1, 1, 16000, 16, 0, S16)
    add("pcm16_48k", avi(waveformat(1, 1, 48000, 16), split(S16_48K, [9600])), 1, 1, 48000, 16, 1, S16_48K)
    add("pcm24", avi(waveformat(1, 1, 16000, 24), split(S24, [3000, 3003])), 1, 1, 16000, 24, 1, S24)
    add("f32", avi(waveformat(3, 1, 16000, 32), split(F32, [4096])), 3, 1, 16000, 32, 1, F32)
    add("u8_odd_chunks", avi(waveformat(1, 1, 16000, 8), split(U8, [999, 1, 1001])), 1, 1, 16000, 8, 1, U8)
    # a frame straddles every chunk boundary: 4-byte frames in chunks of 4001 bytes
    add("pcm16_split_frames", avi(waveformat(1, 2, 16000, 16), split(S16_STEREO, [4001])), 1, 2, 16000, 16, 1, S16_STEREO)
    # records: every two chunk pairs in a `LIST rec `, one of them nested a level deeper
    pieces = split(S16, [1500])
    recs = []
    for k in range(0, len(pieces), 2):
        inner = interleaved(pieces[k:k + 2], 1, 0)
        recs.append(lst(b"rec ", *inner) if k % 4 else lst(b"rec ", lst(b"rec ", *inner[:2]), *inner[2:]))
    add("pcm16_records", avi(waveformat(1, 1, 16000, 16), None, movi=recs), 1, 1, 16000, 16, 1, S16)
    # OpenDML: the second half of the track in an AVIX form, with the index chunks that are stepped over
    half = len(pieces) // 2
    first = interleaved(pieces[:half], 1, 0) + [chunk(b"ix01", bytes(40))]
    second = riff(b"AVIX", lst(b"movi", chunk(b"ix00", bytes(24)), *interleaved(pieces[half:], 1, 0)))
    add("pcm16_avix", avi(waveformat(1, 1, 16000, 16), None, movi=first, extra_forms=[second]), 1, 1, 16000, 16, 1, S16)
    add("mp3", avi(waveformat(0x55, 1, 16000, 0, struct.pack("<HHIHHH", 12, 1, 2, 576, 1, 0)), split(MP3, [1000, 417])), 0x55, 1, 16000, 0, 1, MP3)
    return out


def big_chunk():
    """24-bit mono PCM in one `##wb` chunk above 1 MiB (1 136 640 bytes: 3-byte frames do not divide 2^20, so the scheduler's 1 MiB slices
    cut through frames) and a small one behind it -> the same tuple as a case of cases().  Kept out of cases(): it is fed in large pieces"""
    track = wav_data("wav_24_A_Tusk.wav") * 8
    assert len(track) > (1 << 20) + 3000 and len(track) % 3 == 0
    data = avi(waveformat(1, 1, 16000, 24), [track[:-3000], track[-3000:]])
    return data, 1, 1, 16000, 24, 1, track


def cut_inside_a_chunk():
    """pcm16_stereo cut in the middle of its fifth audio chunk -> (file, the bytes of the four chunks in front)"""
    pieces = split(S16_STEREO, [4000, 1600])
    children = interleaved(pieces, 1, 0)  # [dc, wb, dc, wb, ...]
    whole = avi(waveformat(1, 2, 16000, 16), None, movi=children)
    at = whole.index(b"movi") + 4 + sum(len(c) for c in children[:9])
    assert whole[at:at + 4] == b"01wb"
    return whole[:at + 8 + 700], b"".join(pieces[:4])

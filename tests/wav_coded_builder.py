"""WAV files for the coded walker's tests: RIFF / RF64 writers with any `fmt ` extension, a `fact` chunk, odd chunks and padding.
Run as a program it writes the fixtures of tests/golden/wav_coded/ (see the README there) from files already in tests/golden/."""
import os
import struct

import numpy as np

import wav_adpcm_model as M

TAG_ALAW, TAG_ULAW = 6, 7


def chunk(kind, payload):
    return kind + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def fmt_payload(tag, channels, rate, block_align, bits, ext=None, avg_bytes=None):
    """ext: the bytes behind cbSize (None: a 16-byte fmt without cbSize)"""
    avg = rate * block_align if avg_bytes is None else avg_bytes
    p = struct.pack("<HHIIHH", tag, channels, rate, avg & 0xffffffff, block_align, bits)
    return p if ext is None else p + struct.pack("<H", len(ext)) + ext


def ima_ext(channels, block_align):
    return struct.pack("<H", M.block_frames(M.TAG_IMA, channels, block_align))


def ms_ext(channels, block_align, coef=M.MS_COEF, samples_per_block=None):
    n = M.block_frames(M.TAG_MS, channels, block_align) if samples_per_block is None else samples_per_block
    return struct.pack("<HH", n, len(coef)) + b"".join(struct.pack("<hh", a, b) for a, b in coef)


def wav(fmt, data, fact=None, before_fmt=(), before_data=(), after_data=(), rf64=False, data_size=None):
    """fmt: the fmt chunk's payload; fact: dwSampleLength or None; before_* / after_data: [(kind, payload)] put there; rf64: an RF64
    header with a ds64 chunk and 0xFFFFFFFF sizes; data_size: a declared size other than len(data)"""
    size = len(data) if data_size is None else data_size
    body = b"".join(chunk(k, p) for k, p in before_fmt) + chunk(b"fmt ", fmt)
    if fact is not None:
        body += chunk(b"fact", struct.pack("<I", fact))
    body += b"".join(chunk(k, p) for k, p in before_data)
    tail = data + (b"\0" if len(data) & 1 else b"") + b"".join(chunk(k, p) for k, p in after_data)
    if rf64:
        ds64 = chunk(b"ds64", struct.pack("<QQQI", 0, size, 0, 0))
        total = 4 + len(ds64) + len(body) + 8 + len(tail)
        ds64 = chunk(b"ds64", struct.pack("<QQQI", total, size, 0, 0))
        return b"RF64" + struct.pack("<I", 0xffffffff) + b"WAVE" + ds64 + body + b"data" + struct.pack("<I", 0xffffffff) + tail
    rest = body + b"data" + struct.pack("<I", size) + tail
    return b"RIFF" + struct.pack("<I", 4 + len(rest)) + b"WAVE" + rest


def g711_wav(tag, payload, channels=1, rate=8000, **kw):
    return wav(fmt_payload(tag, channels, rate, channels, 8, b""), payload, **kw)


def ima_wav(pcm, block_align, rate=8000, fact=True, **kw):
    """pcm: int16 [frames, channels]"""
    ch = pcm.shape[1]
    return wav(fmt_payload(M.TAG_IMA, ch, rate, block_align, 4, ima_ext(ch, block_align)), M.ima_encode(pcm, block_align),
               fact=len(pcm) if fact else None, **kw)


def ms_wav(pcm, block_align, rate=8000, coef=M.MS_COEF, fact=True, **kw):
    ch = pcm.shape[1]
    return wav(fmt_payload(M.TAG_MS, ch, rate, block_align, 4, ms_ext(ch, block_align, coef)), M.ms_encode(pcm, block_align, coef),
               fact=len(pcm) if fact else None, **kw)


def model_decode_file(data):
    """What a coded file decodes to, from the builder's own layout (fmt first or after odd chunks; RIFF only): interleaved int16 cut
    to the fact count.  The fixtures' recordings come from here."""
    at, fmt, fact = 12, None, 0
    while True:
        kind, size = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
        body = data[at + 8:at + 8 + size]
        if kind == b"fmt ":
            fmt = body
        elif kind == b"fact":
            fact = struct.unpack("<I", body[:4])[0]
        elif kind == b"data":
            break
        at += 8 + size + (size & 1)
    tag, ch, _, _, align, _ = struct.unpack("<HHIIHH", fmt[:16])
    coef = None
    if tag == M.TAG_MS:
        n = struct.unpack("<H", fmt[20:22])[0]
        coef = [struct.unpack("<hh", fmt[22 + 4 * i:26 + 4 * i]) for i in range(n)]
    pcm, status = M.decode(tag, ch, align, body, coef)
    assert not any(status)
    frames = pcm.size // ch
    return pcm[:(fact if 0 < fact <= frames else frames) * ch]


def audioop_ima_mono_block(block):
    """A mono IMA block's body through Python's audioop.adpcm2lin (an IMA decoder nobody here wrote): it takes the high nibble first,
    so every byte's nibbles are swapped, and its state is seeded from the block header.  -> int16 [frames - 1]"""
    import audioop
    state = (int.from_bytes(block[:2], "little", signed=True), block[2])
    pcm, _ = audioop.adpcm2lin(bytes(((b & 15) << 4) | (b >> 4) for b in block[4:]), 2, state)
    return np.frombuffer(pcm, "<i2")


AUDIOOP_BLOCKS = 4  # of ima_mono_8k.wav, recorded in ima_mono_8k.audioop.s16le


def data_of(file):
    return file[file.index(b"data") + 8:]


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------

def fixtures(golden):
    """{name: bytes} of tests/golden/wav_coded/: the files, and the recordings the model makes of the four ADPCM ones"""
    clip = "A_Tusk_is_used_to_make_costly_gifts"
    speech = np.frombuffer(open(os.path.join(golden, "linear16_8k_A_Tusk.s16le"), "rb").read(), "<i2")
    mono = speech[4000:4000 + 3000].reshape(-1, 1)  # 3000 frames: the fact chunk cuts the last block of every file below
    stereo = np.stack([speech[4000:6500], speech[9000:11500]], 1)
    out = {"ulaw_A_Tusk.wav": g711_wav(TAG_ULAW, open(os.path.join(golden, "g711", clip + ".ulaw"), "rb").read()),
           "alaw_A_Tusk.wav": g711_wav(TAG_ALAW, open(os.path.join(golden, "g711", clip + ".alaw"), "rb").read()),
           "ima_mono_8k.wav": ima_wav(mono, 256), "ima_stereo.wav": ima_wav(stereo, 1024),
           "ms_mono_8k.wav": ms_wav(mono, 256), "ms_stereo.wav": ms_wav(stereo, 1024)}
    for name in [n for n in out if n[0] in "im"]:
        out[name[:-4] + ".decoded.s16le"] = model_decode_file(out[name]).astype("<i2").tobytes()
    return out


if __name__ == "__main__":
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    os.makedirs(os.path.join(golden, "wav_coded"), exist_ok=True)
    files = fixtures(golden)
    blocks = data_of(files["ima_mono_8k.wav"])
    files["ima_mono_8k.audioop.s16le"] = b"".join(audioop_ima_mono_block(blocks[256 * k:256 * k + 256]).astype("<i2").tobytes() for k in range(AUDIOOP_BLOCKS))
    for name, data in files.items():
        with open(os.path.join(golden, "wav_coded", name), "wb") as f:
            f.write(data)
        print(name, len(data))

"""WAV's two ADPCM block forms in numpy: decoders (every block of a stream at once, one step of the recurrence per loop pass; and a
plain block-at-a-time form of each, which the tests pin the vectorised ones and the outside world to) and simple encoders, so that
streams can be written.  The rules are the ones include/soundkit_amd.h states for sk_wav_adpcm_decode.

  IMA (tag 0x11): per channel {predictor s16le, step index, reserved}; then groups of 4 bytes per channel, low nibble first.
  MS  (tag 2):    bPredictor x ch, iDelta x ch, iSamp1 x ch, iSamp2 x ch; output iSamp2, iSamp1, then high nibble, low nibble
                  (stereo: left, right).  pred = (samp1 * c1 + samp2 * c2) / 256, the 32-bit wrapping sum DIVIDED (toward zero)."""
import numpy as np

TAG_MS, TAG_IMA = 2, 0x11
BAD_BLOCK = -1201
IMA_STEP = np.array([
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
    157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552,
    1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487,
    12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767], np.int64)
IMA_INDEX = np.array([-1, -1, -1, -1, 2, 4, 6, 8] * 2, np.int64)
MS_ADAPT = np.array([230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230], np.int64)
MS_COEF = [(256, 0), (512, -256), (0, 0), (192, 64), (240, 0), (460, -208), (392, -232)]  # the standard seven
MS_DELTA_MAX = 0x7fffffff // 768


def block_frames(tag, ch, align):
    if tag == TAG_IMA:
        return 0 if align < 4 * ch or align % (4 * ch) else (align - 4 * ch) * 2 // ch + 1
    return 0 if align < 7 * ch else (align - 7 * ch) * 2 // ch + 2


def _wrap32(x):
    return ((x + 2 ** 31) % 2 ** 32) - 2 ** 31


def _div256(x):  # C's division: toward zero
    return np.sign(x) * (np.abs(x) // 256)


def _s16(lo, hi):
    return (lo.astype(np.int64) | (hi.astype(np.int64) << 8)).astype(np.uint16).view(np.int16).astype(np.int64)


# ---- every block at once --------------------------------------------------------------------------------------------------------

def ima_decode(data, ch, align):
    """-> (int16 [blocks, frames, ch], status [blocks])"""
    b = np.frombuffer(bytes(data), np.uint8).reshape(-1, align)
    n, groups = b.shape[0], (align - 4 * ch) // (4 * ch)
    hdr = b[:, :4 * ch].reshape(n, ch, 4)
    p, idx = _s16(hdr[:, :, 0], hdr[:, :, 1]), hdr[:, :, 2].astype(np.int64)
    bad = (idx > 88).any(axis=1)
    idx = np.minimum(idx, 88)
    body = b[:, 4 * ch:].reshape(n, groups, ch, 4)
    nib = np.stack([body & 15, body >> 4], -1).reshape(n, groups, ch, 8).transpose(0, 1, 3, 2).reshape(n, groups * 8, ch).astype(np.int64)
    out = np.zeros((n, groups * 8 + 1, ch), np.int64)
    out[:, 0] = p
    for f in range(groups * 8):
        c, step = nib[:, f], IMA_STEP[idx]
        d = (step >> 3) + np.where(c & 4, step, 0) + np.where(c & 2, step >> 1, 0) + np.where(c & 1, step >> 2, 0)
        p = np.clip(p + np.where(c & 8, -d, d), -32768, 32767)
        idx = np.clip(idx + IMA_INDEX[c], 0, 88)
        out[:, f + 1] = p
    out[bad] = 0
    return out.astype(np.int16), np.where(bad, BAD_BLOCK, 0).tolist()


def ms_decode(data, ch, align, coef):
    b = np.frombuffer(bytes(data), np.uint8).reshape(-1, align)
    n = b.shape[0]
    coef = np.asarray(coef, np.int64).reshape(-1, 2)
    pred = b[:, :ch].astype(np.int64)
    bad = (pred >= len(coef)).any(axis=1)
    pred = np.minimum(pred, len(coef) - 1)
    c1, c2 = coef[pred, 0], coef[pred, 1]
    w = b[:, ch:7 * ch].reshape(n, 3, ch, 2)
    delta, s1, s2 = (_s16(w[:, k, :, 0], w[:, k, :, 1]) for k in range(3))
    body = b[:, 7 * ch:]
    nib = np.stack([body >> 4, body & 15], -1).reshape(n, -1, ch).astype(np.int64)
    out = np.zeros((n, nib.shape[1] + 2, ch), np.int64)
    out[:, 0], out[:, 1] = s2, s1
    for f in range(nib.shape[1]):
        c = nib[:, f]
        v = np.clip(_div256(_wrap32(s1 * c1 + s2 * c2)) + ((c ^ 8) - 8) * delta, -32768, 32767)
        s2, s1 = s1, v
        delta = np.clip(_div256(MS_ADAPT[c] * delta), 16, MS_DELTA_MAX)
        out[:, f + 2] = v
    out[bad] = 0
    return out.astype(np.int16), np.where(bad, BAD_BLOCK, 0).tolist()


def decode(tag, ch, align, data, coef=None):
    """-> (interleaved int16 of every block, one after the other; status per block)"""
    if len(data) == 0:
        return np.zeros(0, np.int16), []
    out, status = ima_decode(data, ch, align) if tag == TAG_IMA else ms_decode(data, ch, align, coef)
    return out.reshape(-1), status


# ---- one block, plainly (what the known-answer tests and the audioop pin run against) ---------------------------------------------

def ima_decode_block(block, ch):
    """-> [frames][ch] ints, or None for a block its header rules out"""
    if any(block[4 * c + 2] > 88 for c in range(ch)):
        return None
    frames = block_frames(TAG_IMA, ch, len(block))
    out = [[0] * ch for _ in range(frames)]
    for c in range(ch):
        p = int.from_bytes(block[4 * c:4 * c + 2], "little", signed=True)
        idx = block[4 * c + 2]
        out[0][c] = p
        for g in range((len(block) - 4 * ch) // (4 * ch)):
            for k in range(8):
                byte = block[4 * ch + 4 * ch * g + 4 * c + k // 2]
                n = byte >> 4 if k & 1 else byte & 15
                step = int(IMA_STEP[idx])
                d = (step >> 3) + (step if n & 4 else 0) + (step >> 1 if n & 2 else 0) + (step >> 2 if n & 1 else 0)
                p = max(-32768, min(32767, p - d if n & 8 else p + d))
                idx = max(0, min(88, idx + int(IMA_INDEX[n])))
                out[1 + 8 * g + k][c] = p
    return out


def _cdiv(a, b):
    q = abs(a) // b
    return -q if a < 0 else q


def ms_decode_block(block, ch, coef):
    if any(block[c] >= len(coef) for c in range(ch)):
        return None
    frames = block_frames(TAG_MS, ch, len(block))
    out = [[0] * ch for _ in range(frames)]
    rd = lambda at: int.from_bytes(block[at:at + 2], "little", signed=True)  # noqa: E731
    for c in range(ch):
        c1, c2 = coef[block[c]]
        delta, s1, s2 = rd(ch + 2 * c), rd(3 * ch + 2 * c), rd(5 * ch + 2 * c)
        out[0][c], out[1][c] = s2, s1
        for f in range(2, frames):
            k = (f - 2) * ch + c  # nibble number in the body, high nibble first
            byte = block[7 * ch + k // 2]
            n = byte & 15 if k & 1 else byte >> 4
            v = max(-32768, min(32767, _cdiv(int(_wrap32(s1 * c1 + s2 * c2)), 256) + ((n ^ 8) - 8) * delta))
            s2, s1 = s1, v
            delta = max(16, min(MS_DELTA_MAX, _cdiv(int(MS_ADAPT[n]) * delta, 256)))
            out[f][c] = v
    return out


# ---- encoders: plain ones, good enough to write speech into blocks ----------------------------------------------------------------

def _pad_blocks(pcm, frames):
    pcm = np.asarray(pcm, np.int64)
    short = -len(pcm) % frames
    return np.concatenate([pcm, np.repeat(pcm[-1:], short, axis=0)]) if short else pcm


def ima_encode(pcm, align):
    """pcm: int16 [frames, ch] -> whole blocks; the last one is padded with its last frame.  The step index runs on from block to
    block in the encoder (the decoder takes it from each header)."""
    ch = pcm.shape[1]
    frames = block_frames(TAG_IMA, ch, align)
    pcm = _pad_blocks(pcm, frames)
    idx, out = [0] * ch, bytearray()
    for at in range(0, len(pcm), frames):
        blk, body = pcm[at:at + frames], bytearray(align - 4 * ch)
        for c in range(ch):
            p = int(blk[0, c])
            out += p.to_bytes(2, "little", signed=True) + bytes([idx[c], 0])
            i = idx[c]
            for f in range(1, frames):
                step, diff, n = int(IMA_STEP[i]), int(blk[f, c]) - p, 0
                if diff < 0:
                    n, diff = 8, -diff
                d = step >> 3
                for bit, s in ((4, step), (2, step >> 1), (1, step >> 2)):
                    if diff >= s:
                        n, diff, d = n | bit, diff - s, d + s
                p = max(-32768, min(32767, p - d if n & 8 else p + d))
                i = max(0, min(88, i + int(IMA_INDEX[n])))
                k = f - 1
                body[(k // 8) * 4 * ch + 4 * c + (k % 8) // 2] |= n << (4 * (k & 1))
            idx[c] = i
        out += body
    return bytes(out)


def ms_encode(pcm, align, coef=MS_COEF):
    """pcm: int16 [frames, ch] -> whole blocks, each with the coefficient set that predicts it best and a delta taken from its first
    prediction errors"""
    ch = pcm.shape[1]
    frames = block_frames(TAG_MS, ch, align)
    pcm = _pad_blocks(pcm, frames)
    out = bytearray()
    for at in range(0, len(pcm), frames):
        blk = pcm[at:at + frames]
        hdr = [bytearray() for _ in range(4)]
        nibbles = np.zeros((frames - 2, ch), np.uint8)
        for c in range(ch):
            x = blk[:, c]
            errs = [np.abs(x[2:] - (x[1:-1] * c1 + x[:-2] * c2) // 256).sum() if frames > 2 else 0 for c1, c2 in coef]
            best = int(np.argmin(errs))
            c1, c2 = coef[best]
            s2, s1 = int(x[0]), int(x[1])
            delta = max(16, int(np.abs(x[2:6] - (x[1:5] * c1 + x[:4] * c2) // 256).max()) // 4 if frames > 5 else 16)
            delta = min(delta, 32767)
            for k, v in enumerate((best, delta, s1, s2)):
                hdr[k] += bytes([v]) if k == 0 else int(v).to_bytes(2, "little", signed=True)
            for f in range(2, frames):
                pred = _cdiv(int(_wrap32(s1 * c1 + s2 * c2)), 256)
                err = int(x[f]) - pred
                sn = max(-8, min(7, int(round(err / delta))))
                n = sn & 15
                v = max(-32768, min(32767, pred + sn * delta))
                s2, s1 = s1, v
                delta = max(16, min(MS_DELTA_MAX, _cdiv(int(MS_ADAPT[n]) * delta, 256)))
                nibbles[f - 2, c] = n
        flat = nibbles.reshape(-1)
        out += b"".join(bytes(h) for h in hdr) + bytes(((flat[0::2] << 4) | flat[1::2]).astype(np.uint8))
    return bytes(out)

"""The stream processors in front of the scheduler's WAV / raw PCM / AIFF streams, by themselves (csrc/pcm_stream.h through the C ABI;
host code, no GPU): WavStreamProcessor.add (soundkit/src/wav.rs:95-324) and RawPcmStreamProcessor.add / flush
(soundkit/src/raw_pcm.rs:150-190).  `add` returns None or (stream_offset, bytes): the whole PCM frames available now and where
they start in the stream; a rejected stream raises ValueError with the reference's text.  AiffReader is the container walk of
AiffDecoder.add (soundkit-aiff/src/lib.rs:93-475): its pieces are whole sample groups in the FILE's encoding (info()["encoding"], an
AIFF_* of engine.py), which Engine.aiff_decode or the AIFF tick turn into the PCM of the output contract; add(b"") finalises.
WavCodedReader is the WAV walker in its coded mode, this project's own: besides PCM and float it takes A-law, mu-law, IMA and Microsoft
ADPCM files (pieces of whole frames or whole blocks, still encoded); decode_wav decodes such a file whole, outside the scheduler."""
import ctypes as C

from ._lib import SoundkitError, lib

SK_PCM_ERR_STREAM = -401


class _Processor:
    _add = _err = _destroy = None

    def add(self, chunk):
        chunk = bytes(chunk)
        off, n, ptr = C.c_uint64(), C.c_size_t(), C.c_void_p()
        rc = self._add(self._h, chunk if chunk else None, len(chunk), C.byref(off), C.byref(n), C.byref(ptr))
        if rc == SK_PCM_ERR_STREAM:
            raise ValueError(self._err(self._h).decode())
        if rc != 0:
            raise SoundkitError(rc, "add")
        if n.value == 0:
            return None
        return off.value, C.string_at(ptr.value, n.value)

    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WavStreamProcessor(_Processor):
    def __init__(self):
        self._add, self._err, self._destroy = lib.sk_wav_reader_add, lib.sk_wav_reader_last_error, lib.sk_wav_reader_destroy
        h = C.c_void_p()
        rc = lib.sk_wav_reader_create(C.byref(h))
        if rc != 0:
            raise SoundkitError(rc, "sk_wav_reader_create")
        self._h = h

    def info(self):
        """{sample_rate, channels, bits, is_float, total_frames}: zeros until the fmt chunk / the data chunk's header has been seen"""
        rate, ch, bits, fl, total = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int(), C.c_uint64()
        lib.sk_wav_reader_info(self._h, C.byref(rate), C.byref(ch), C.byref(bits), C.byref(fl), C.byref(total))
        return {"sample_rate": rate.value, "channels": ch.value, "bits": bits.value, "is_float": bool(fl.value), "total_frames": total.value}


class WavCodedReader(_Processor):
    """sk_wav_coded_reader: the WAV walker in its coded mode -- beyond the reference, it takes A-law (6), mu-law (7), IMA ADPCM (0x11)
    and Microsoft ADPCM (2) besides PCM and float.  Pieces are whole frames, for the two ADPCM tags whole blocks."""

    def __init__(self):
        self._add, self._err, self._destroy = lib.sk_wav_coded_reader_add, lib.sk_wav_coded_reader_last_error, lib.sk_wav_coded_reader_destroy
        h = C.c_void_p()
        rc = lib.sk_wav_coded_reader_create(C.byref(h))
        if rc != 0:
            raise SoundkitError(rc, "sk_wav_coded_reader_create")
        self._h = h

    def info(self):
        """{tag, sample_rate, channels, bits, is_float, block_align, frames_per_block, coef: [(iCoef1, iCoef2)], fact_frames,
        total_frames}: zeros until the fmt chunk has been read; total_frames once the data chunk's header has been"""
        from ._lib import WavCodedInfo
        i = WavCodedInfo()
        lib.sk_wav_coded_reader_info(self._h, C.byref(i))
        return {"tag": i.tag, "sample_rate": i.sample_rate, "channels": i.channels, "bits": i.bits, "is_float": bool(i.is_float),
                "block_align": i.block_align, "frames_per_block": i.frames_per_block, "coef": [(i.coef[k][0], i.coef[k][1]) for k in range(i.n_coef)],
                "fact_frames": i.fact_frames, "total_frames": i.total_frames}


def wav_bad_block_text(info, block):
    """The text a block has that sk_wav_adpcm_decode marked WAV_BAD_BLOCK: which header field rules it out"""
    from .engine import WAV_TAG_IMA_ADPCM
    for c in range(info["channels"]):
        if info["tag"] == WAV_TAG_IMA_ADPCM and block[4 * c + 2] > 88:
            return "WAV IMA ADPCM block step index %d exceeds 88" % block[4 * c + 2]
        if info["tag"] != WAV_TAG_IMA_ADPCM and block[c] >= len(info["coef"]):
            return "WAV MS ADPCM block predictor %d exceeds the %d coefficient sets" % (block[c], len(info["coef"]))
    return "WAV ADPCM block is invalid"


def decode_wav(data, options=None, engine=None, scheduler=None):
    """A whole WAV file of one of the four coded tags, outside the scheduler: WavCodedReader -> A-law / mu-law expanded by
    Engine.aiff_decode, ADPCM blocks decoded by Engine.wav_adpcm_decode and cut to the fact chunk's count -> the output options through
    alac.output_stage (the conversion stage every PCM-family input ends in), the resampler flushed.  -> (info, [AudioData]).  A block
    that its header rules out raises `Decoding failed: ` + its text; a walker error raises ValueError with the walker's text.  PCM and
    float files are the scheduler's (DecodePipeline.spawn): this refuses them."""
    from . import alac
    from .engine import AIFF_ALAW, AIFF_ULAW, WAV_TAG_ALAW, WAV_TAG_IMA_ADPCM, WAV_TAG_MS_ADPCM, WAV_TAG_ULAW, default_engine
    data = bytes(data)
    reader = WavCodedReader()
    try:
        pieces = []
        for at in range(0, len(data), 1 << 20):
            got = reader.add(data[at:at + (1 << 20)])
            if got is not None:
                pieces.append(got[1])
        info = reader.info()
    finally:
        reader.close()
    tag, ch = info["tag"], info["channels"]
    if tag not in (WAV_TAG_ALAW, WAV_TAG_ULAW, WAV_TAG_IMA_ADPCM, WAV_TAG_MS_ADPCM):
        raise ValueError("decode_wav reads WAV format tags 2, 6, 7 and 0x11; this file has tag %d" % tag)
    eng = engine or default_engine()
    pcm = []
    if tag in (WAV_TAG_ALAW, WAV_TAG_ULAW):
        pcm = [eng.aiff_decode(AIFF_ALAW if tag == WAV_TAG_ALAW else AIFF_ULAW, ch, p) for p in pieces]
    else:
        left = info["total_frames"]
        for p in pieces:
            got, status = eng.wav_adpcm_decode(tag, ch, info["block_align"], p, info["coef"])
            for k, st in enumerate(status):
                if st != 0:
                    raise SoundkitError(st, "decode_wav", "Decoding failed: " + wav_bad_block_text(info, p[k * info["block_align"]:(k + 1) * info["block_align"]]))
            got = got[:left * ch * 2]
            left -= len(got) // (ch * 2)
            if got:
                pcm.append(got)
    return info, alac.output_stage(pcm, info["sample_rate"], ch, 16, options, scheduler)


class RawPcmStreamProcessor(_Processor):
    def __init__(self, bytes_per_frame):
        self._add, self._err, self._destroy = lib.sk_raw_pcm_framer_add, lib.sk_raw_pcm_framer_last_error, lib.sk_raw_pcm_framer_destroy
        h = C.c_void_p()
        rc = lib.sk_raw_pcm_framer_create(bytes_per_frame, C.byref(h))
        if rc != 0:
            raise SoundkitError(rc, "sk_raw_pcm_framer_create")
        self._h = h

    def flush(self):
        rc = lib.sk_raw_pcm_framer_flush(self._h)
        if rc == SK_PCM_ERR_STREAM:
            raise ValueError(self._err(self._h).decode())
        if rc != 0:
            raise SoundkitError(rc, "sk_raw_pcm_framer_flush")


class AiffReader(_Processor):
    def __init__(self):
        self._add, self._err, self._destroy = lib.sk_aiff_reader_add, lib.sk_aiff_reader_last_error, lib.sk_aiff_reader_destroy
        h = C.c_void_p()
        rc = lib.sk_aiff_reader_create(C.byref(h))
        if rc != 0:
            raise SoundkitError(rc, "sk_aiff_reader_create")
        self._h = h

    def info(self):
        """{sample_rate, channels, encoding, bits, is_float, buffered_bytes}: zeros (but buffered_bytes) until COMM has been read;
        bits / is_float are the output contract's"""
        from ._lib import AiffInfo
        i = AiffInfo()
        lib.sk_aiff_reader_info(self._h, C.byref(i))
        return {"sample_rate": i.sample_rate, "channels": i.channels, "encoding": i.encoding, "bits": i.bits, "is_float": bool(i.is_float),
                "buffered_bytes": i.buffered_bytes}

    def buffered_bytes(self):
        return self.info()["buffered_bytes"]

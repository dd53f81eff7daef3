"""The stream processors in front of the scheduler's WAV / raw PCM / AIFF streams, by themselves (csrc/pcm_stream.h through the C ABI;
host code, no GPU): WavStreamProcessor.add (soundkit/src/wav.rs:95-324) and RawPcmStreamProcessor.add / flush
(soundkit/src/raw_pcm.rs:150-190).  `add` returns None or (stream_offset, bytes): the whole PCM frames available now and where
they start in the stream; a rejected stream raises ValueError with the reference's text.  AiffReader is the container walk of
AiffDecoder.add (soundkit-aiff/src/lib.rs:93-475): its pieces are whole sample groups in the FILE's encoding (info()["encoding"], an
AIFF_* of engine.py), which Engine.aiff_decode or the AIFF tick turn into the PCM of the output contract; add(b"") finalises."""
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

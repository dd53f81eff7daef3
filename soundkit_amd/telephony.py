"""Headerless telephony streams on the GPU: G.711 (mu-law / A-law), G.722 (64 kbit/s), G.726 (16 / 24 / 32 / 40 kbit/s) and GSM 06.10
full rate (13 kbit/s, in the standard 33-byte framing or the reference's Microsoft framing of 65-byte pairs).

The decoders have the shape of the reference's Decoder objects (soundkit-g711, soundkit-g722, soundkit-g726): `decode_i16`,
`decode_i32` (= the s16 sample << 16), `decode_f32` (= / 32768), `sample_rate`, `channels`, and for G.726 `flush`.  The carry from call
to call (sk_g726_state / sk_g722_state) lives in the decoder; Engine.g72x_decode, g72x_decode_batch and tick_run_g72x take it as a
record from `new_state`.  GsmDecoder is the reference's GsmDecoder (soundkit-gsm) in the same shape, with `flush`; its carry
(sk_gsm_state) is `new_state(GSM)` for Engine.gsm_decode, gsm_decode_batch and tick_run_gsm.  Not built: G.722 at 56 / 48 kbit/s, libgsm's
LSB-first WAV-49 layout, AMR-NB, G.729, Speex, and the encoders.
"""
import ctypes as C

import numpy as np

from ._lib import G722State, G726State, GsmState, SoundkitError, lib

ULAW, ALAW, G722, G726 = 0, 1, 2, 3  # enum sk_g72x_codec
LEFT, RIGHT = 0, 1  # enum sk_g726_packing: MSB first (`ffmpeg -f g726`), LSB first (`-f g726le`)
GSM = 16  # no sk_g72x_codec: GSM 06.10 has its own entry points (sk_gsm_*); here it names the carry for new_state
GSM_STANDARD, GSM_MICROSOFT = 0, 1  # enum sk_gsm_variant: 33 bytes -> 160 samples, 65 bytes -> 320 samples
_GSM_PACKET = {GSM_STANDARD: (33, 160), GSM_MICROSOFT: (65, 320)}  # variant -> (bytes, samples) of a packet
ERR_STREAM = -701
MAX_SEND_SAMPLES = 262144
G726_RATES = (16000, 24000, 32000, 40000)
_GROUP = {16000: (1, 4), 24000: (3, 8), 32000: (1, 2), 40000: (5, 8)}  # rate -> (bytes, samples) of a group


class TelephonyError(ValueError):
    """A send or a stream that was rejected with the reference's text."""


def _check_codec(codec, rate=32000, packing=LEFT):
    if codec not in (ULAW, ALAW, G722, G726):
        raise ValueError("codec must be telephony.ULAW, ALAW, G722 or G726, not %r" % (codec,))
    if codec == G726 and rate not in G726_RATES:
        raise ValueError("G.726 rate must be one of %s, not %r" % (G726_RATES, rate))
    if codec == G726 and packing not in (LEFT, RIGHT):
        raise ValueError("G.726 packing must be telephony.LEFT or telephony.RIGHT, not %r" % (packing,))


def new_state(codec):
    """The record a fresh stream starts from: G726Core::default() for G.726, all zeros for G.722, None for G.711; for GSM all zeros
    but nrp = 40."""
    if codec == GSM:
        st = GsmState()
        lib.sk_gsm_state_init(C.byref(st))
        return st
    _check_codec(codec)
    if codec == G726:
        st = G726State()
        lib.sk_g726_state_init(C.byref(st))
        return st
    if codec == G722:
        st = G722State()
        lib.sk_g722_state_init(C.byref(st))
        return st
    return None


def state_words(state):
    """A state record as a list of ints (24 for G.726, 66 for G.722, 138 for GSM), in the order of the C struct."""
    return np.frombuffer(bytes(state), np.int32).tolist()


def decoded_samples(codec, n_bytes, rate=32000):
    """Samples that n_bytes decode to (G.726: by whole groups)."""
    _check_codec(codec, rate)
    if codec == G726:
        gb, gs = _GROUP[rate]
        return n_bytes // gb * gs
    return n_bytes * 2 if codec == G722 else n_bytes


def _check_gsm_variant(variant):
    if variant not in (GSM_STANDARD, GSM_MICROSOFT):
        raise ValueError("variant must be telephony.GSM_STANDARD or telephony.GSM_MICROSOFT, not %r" % (variant,))


def gsm_decoded_samples(variant, n_bytes):
    """Samples that n_bytes of GSM decode to, by whole packets."""
    _check_gsm_variant(variant)
    pb, ps = _GSM_PACKET[variant]
    return n_bytes // pb * ps


class _Decoder:
    _family = "sk_g72x_decoder"  # the C handle's functions

    def __init__(self, engine, handle):
        self._engine, self._h = engine, handle  # the engine outlives the decoder

    def __del__(self):
        if getattr(self, "_h", None):
            getattr(lib, self._family + "_destroy")(self._h)
            self._h = None

    def _info(self):
        codec, rate, ch = C.c_int(), C.c_uint32(), C.c_uint32()
        getattr(lib, self._family + "_info")(self._h, C.byref(codec), C.byref(rate), C.byref(ch))
        return codec.value, rate.value, ch.value

    @property
    def sample_rate(self):
        return self._info()[1]

    @property
    def channels(self):
        return self._info()[2]

    def _last_error(self):
        return getattr(lib, self._family + "_last_error")(self._h).decode()

    def _decode(self, kind, dtype, data):
        fn = getattr(lib, self._family + "_decode_" + kind)
        data = np.frombuffer(bytes(data), np.uint8)
        out = np.zeros(max(self._capacity(data.size), 1), dtype)
        n = C.c_size_t()
        rc = fn(self._h, data.ctypes.data_as(C.c_void_p) if data.size else None, data.size, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n))
        if rc != 0:
            text = self._last_error()
            if rc in (ERR_STREAM, -6) and text:
                raise TelephonyError(text)
            raise SoundkitError(rc, fn.__name__)
        return out[:n.value].copy()

    def decode_i16(self, data):
        return self._decode("i16", np.int16, data)

    def decode_i32(self, data):
        return self._decode("i32", np.int32, data)

    def decode_f32(self, data):
        return self._decode("f32", np.float32, data)

    def reset(self):
        getattr(lib, self._family + "_reset")(self._h)


class G711Decoder(_Decoder):
    def __init__(self, engine, law, sample_rate=8000, channels=1):
        if law not in (ULAW, ALAW):
            raise ValueError("law must be telephony.ULAW or telephony.ALAW, not %r" % (law,))
        h, text = C.c_void_p(), C.create_string_buffer(128)
        rc = lib.sk_g711_decoder_create(engine._h, int(law), int(sample_rate), int(channels), C.byref(h), text, 128)
        if rc == ERR_STREAM:
            raise TelephonyError(text.value.decode())
        if rc != 0:
            raise SoundkitError(rc, "sk_g711_decoder_create")
        super().__init__(engine, h)

    def _capacity(self, n):
        return n


class G722Decoder(_Decoder):
    def __init__(self, engine):
        h = C.c_void_p()
        rc = lib.sk_g722_decoder_create(engine._h, C.byref(h))
        if rc != 0:
            raise SoundkitError(rc, "sk_g722_decoder_create")
        super().__init__(engine, h)

    def _capacity(self, n):
        return 2 * n


class G726Decoder(_Decoder):
    def __init__(self, engine, rate=32000, packing=LEFT):
        _check_codec(G726, rate, packing)
        h = C.c_void_p()
        rc = lib.sk_g726_decoder_create(engine._h, int(rate), int(packing), C.byref(h))
        if rc != 0:
            raise SoundkitError(rc, "sk_g726_decoder_create")
        super().__init__(engine, h)
        self.rate, self.packing = rate, packing

    def _capacity(self, n):
        gb, gs = _GROUP[self.rate]
        return (n + gb) // gb * gs  # + the group a pending partial one may complete

    def flush(self):
        """The end of the stream: raises TelephonyError(`G.726 stream ended with N trailing partial-packet byte(s)`) when a partial
        group is left."""
        rc = lib.sk_g726_decoder_flush(self._h)
        if rc == ERR_STREAM:
            raise TelephonyError(lib.sk_g72x_decoder_last_error(self._h).decode())
        if rc != 0:
            raise SoundkitError(rc, "sk_g726_decoder_flush")


class GsmDecoder(_Decoder):
    """The reference's GsmDecoder: whole packets decode, a partial packet waits for the next call."""
    _family = "sk_gsm_decoder"

    def __init__(self, engine, variant=GSM_STANDARD):
        _check_gsm_variant(variant)
        h = C.c_void_p()
        rc = lib.sk_gsm_decoder_create(engine._h, int(variant), C.byref(h))
        if rc != 0:
            raise SoundkitError(rc, "sk_gsm_decoder_create")
        super().__init__(engine, h)
        self.variant = variant

    def _capacity(self, n):
        pb, ps = _GSM_PACKET[self.variant]
        return (n + pb) // pb * ps  # + the packet a pending partial one may complete

    def flush(self):
        """The end of the stream: raises TelephonyError(`GSM stream ended with N trailing partial-frame byte(s)`) when a partial
        packet is left."""
        rc = lib.sk_gsm_decoder_flush(self._h)
        if rc == ERR_STREAM:
            raise TelephonyError(self._last_error())
        if rc != 0:
            raise SoundkitError(rc, "sk_gsm_decoder_flush")

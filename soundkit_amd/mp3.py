"""Host-side mirror of soundkit-mp3's decoder (soundkit-mp3/src/lib.rs:147-374): frame sync, header, side information,
the bit reservoir, scale factors and the Huffman stage on the host (csrc/mp3_bitstream.cpp, csrc/mp3_decoder.cpp) -- or the last
two on the GPU (csrc/mp3_entropy.hip: set_codebook / entropy_decode / decode_frames, Mp3Decoder(gpu_entropy=True));
requantisation, joint stereo and the short-block reorder (csrc/mp3_requant.hip) and the hybrid synthesis filterbank
(csrc/mp3_hybrid.hip) on the GPU; the reference's `f32_to_i16` tail.  The standard's data tables (ISO/IEC 11172-3 B.3 /
B.6 / B.7 / B.8, 13818-3 2.4.3.2) are csrc/mp3_iso_tables.h; `Mp3Decoder()` uses them unless given another Codebook."""
import ctypes as C

import numpy as np

from ._lib import (Mp3FrameInfo, Mp3FrameItem, Mp3GranuleData, Mp3GranuleDesc, Mp3RequantGranule, Mp3SideInfo, MpaFrameInfo,
                   MpaFrameRecord, SoundkitError, check, lib)
from .engine import _ptr, default_engine


def set_synthesis_window(d512, engine=None):
    """ISO/IEC 11172-3 Table B.3, 512 coefficients, once per engine"""
    engine = engine or default_engine()
    d = np.ascontiguousarray(d512, np.float32)
    assert d.shape == (512,)
    check(lib.sk_mp3_set_synthesis_window(engine._h, _ptr(d)), "sk_mp3_set_synthesis_window", engine._h)


def make_descs(granules):
    """granules: iterable of (stream, channels, (block_type...), (mixed_block_flag...))"""
    granules = list(granules)
    arr = (Mp3GranuleDesc * max(len(granules), 1))()
    for i, (stream, ch, block_types, mixed) in enumerate(granules):
        arr[i].stream, arr[i].channels = stream, ch
        for c in range(min(ch, 2)):  # a count outside 1..2 is the engine's to reject
            arr[i].block_type[c] = block_types[c]
            arr[i].mixed_block_flag[c] = mixed[c]
    return arr, len(granules)


def hybrid_synthesize(granules, xr, engine=None, s16=False):
    """xr [n][channels][576] f32 -> (pcm [n][576][channels] f32 in +-1.0, or s16 through f32_to_i16; status [n])"""
    engine = engine or default_engine()
    descs, n = make_descs(granules)
    xr = np.ascontiguousarray(xr, np.float32)
    ch = xr.shape[1] if xr.ndim == 3 else 1
    out = np.zeros((n, 576, ch), np.int16 if s16 else np.float32)
    status = np.zeros(max(n, 1), np.int32)
    fn = lib.sk_mp3_hybrid_synthesize_s16 if s16 else lib.sk_mp3_hybrid_synthesize_f32
    check(fn(engine._h, descs, _ptr(xr), _ptr(out), n, _ptr(status)), "sk_mp3_hybrid_synthesize", engine._h)
    return out, status[:n]


# ---- the fixed-syntax front (host) ----------------------------------------------------------------------------------------

def _as_dict(struct):
    out = {}
    for name, _ in struct._fields_:
        v = getattr(struct, name)
        out[name] = v if isinstance(v, int) else np.ctypeslib.as_array(v).tolist()
    return out


def _bytes(data):
    return np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)


def parse_header(data):
    """4 bytes -> (status, Mp3FrameInfo)"""
    info = Mp3FrameInfo()
    b = _bytes(data)
    return lib.sk_mp3_parse_header(_ptr(b), len(data), C.byref(info)), info


def parse_side_info(frame, info):
    side = Mp3SideInfo()
    b = _bytes(frame)
    return lib.sk_mp3_parse_side_info(_ptr(b), len(frame), C.byref(info), C.byref(side)), side


def scan(data, cap=1 << 16):
    """every frame of a byte string -> ([Mp3FrameInfo], bytes consumed)"""
    frames = (Mp3FrameInfo * cap)()
    n, used = C.c_uint32(0), C.c_size_t(0)
    b = _bytes(data)
    check(lib.sk_mp3_scan(_ptr(b), len(data), frames, cap, C.byref(n), C.byref(used)), "sk_mp3_scan")
    return [frames[i] for i in range(min(n.value, cap))], used.value


def scan_free(data, free_format_bytes=0, cap=1 << 16):
    """sk_mp3_scan_free -> ([Mp3FrameInfo], bytes consumed, free_format_bytes to hand to the next call)"""
    frames = (Mp3FrameInfo * cap)()
    n, used, ffb = C.c_uint32(0), C.c_size_t(0), C.c_uint32(free_format_bytes)
    b = _bytes(data)
    check(lib.sk_mp3_scan_free(_ptr(b), len(data), frames, cap, C.byref(n), C.byref(used), C.byref(ffb)), "sk_mp3_scan_free")
    return [frames[i] for i in range(min(n.value, cap))], used.value, ffb.value


def main_data(frame, info, side, reservoir):
    """(status, the bytes parts 2 + 3 of this frame are read from)"""
    out = np.zeros(len(reservoir) + len(frame) + 16, np.uint8)
    n = C.c_size_t(0)
    f, r = _bytes(frame), _bytes(reservoir)
    rc = lib.sk_mp3_main_data(_ptr(f), len(frame), C.byref(info), C.byref(side), _ptr(r), len(reservoir), _ptr(out), out.size, C.byref(n))
    return rc, out[:n.value].tobytes()


# ---- requantisation / joint stereo / reorder (GPU) -------------------------------------------------------------------------

def set_band_tables(sample_rate, long_offsets, short_offsets, pretab, engine=None):
    """ISO/IEC 11172-3 Table B.8 (23 long, 14 short offsets) and the pre-emphasis table (22), once per engine and rate"""
    engine = engine or default_engine()
    lo, so, pt = (np.ascontiguousarray(long_offsets, np.uint16), np.ascontiguousarray(short_offsets, np.uint16),
                  np.ascontiguousarray(pretab, np.uint8))
    assert lo.shape == (23,) and so.shape == (14,) and pt.shape == (22,)
    return lib.sk_mp3_set_band_tables(engine._h, sample_rate, _ptr(lo), _ptr(so), _ptr(pt))


def make_requant_granules(granules):
    """granules: dicts as oracle/mp3_bitstream.py requantize_granule takes them, plus sample_rate and lsf"""
    arr = (Mp3RequantGranule * max(len(granules), 1))()
    for i, g in enumerate(granules):
        a = arr[i]
        a.sample_rate, a.channels = g["sample_rate"], g["channels"]
        a.ms_stereo, a.intensity_stereo, a.lsf = g.get("ms_stereo", 0), g.get("intensity_stereo", 0), g.get("lsf", 0)
        for c in range(min(g["channels"], 2)):
            src, dst = g["ch"][c], a.ch[c]
            for name in ("global_gain", "scalefac_scale", "preflag", "block_type", "mixed_block_flag"):
                setattr(dst, name, src[name])
            for w in range(3):
                dst.subblock_gain[w] = src["subblock_gain"][w]
            for b in range(22):
                dst.scalefac_l[b] = src["scalefac_l"][b]
            for b in range(13):
                for w in range(3):
                    dst.scalefac_s[b][w] = src["scalefac_s"][b][w]
    return arr


def requantize(granules, quant, engine=None):
    """quant: int16, the granules' channels one after another, 576 lines each, bitstream order -> (xr f32 same shape, status)"""
    engine = engine or default_engine()
    arr = make_requant_granules(granules)
    n = len(granules)
    q = np.ascontiguousarray(quant, np.int16)
    xr = np.zeros(q.shape, np.float32)
    status = np.zeros(max(n, 1), np.int32)
    check(lib.sk_mp3_requantize(engine._h, arr, _ptr(q), _ptr(xr), n, _ptr(status)), "sk_mp3_requantize", engine._h)
    return xr, status[:n]


# ---- parts 2 + 3 over caller-supplied tables, and the decoder handle -----------------------------------------------------------

def iso_tables():
    """the standard's tables as the library holds them (sk_mp3_iso_tables) -> Mp3Tables"""
    from ._lib import Mp3Tables
    t = Mp3Tables()
    check(lib.sk_mp3_iso_tables(C.byref(t)), "sk_mp3_iso_tables")
    return t


class Codebook:
    """sk_mp3_codebook: host-side decoding structures built from an Mp3Tables; tables=None: the standard's (Table B.7 and
    friends, csrc/mp3_iso_tables.h)"""

    def __init__(self, tables=None):
        self._h = C.c_void_p()
        if tables is None:
            check(lib.sk_mp3_codebook_create_iso(C.byref(self._h)), "sk_mp3_codebook_create_iso")
        else:
            check(lib.sk_mp3_codebook_create(C.byref(tables), C.byref(self._h)), "sk_mp3_codebook_create")

    def close(self):
        if self._h:
            lib.sk_mp3_codebook_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        self.close()


def decode_main_data(codebook, info, side, main):
    """(status, [granule][channel] Mp3GranuleData) -- scale factors and the 576 integers of every granule of one frame"""
    out = ((Mp3GranuleData * 2) * 2)()
    b = _bytes(main)
    rc = lib.sk_mp3_decode_main_data(codebook._h, C.byref(info), C.byref(side), _ptr(b), len(main), out)
    return rc, out


# ---- parts 2 + 3 on the GPU (csrc/mp3_entropy.hip) -----------------------------------------------------------------------------

def codebook_flatten(codebook):
    """sk_mp3_codebook_flatten: the device form of a code book as uint32 words (layout: csrc/mp3_codebook_blob.h)"""
    n = C.c_size_t(0)
    rc = lib.sk_mp3_codebook_flatten(codebook._h, None, 0, C.byref(n))
    if rc not in (0, -7):  # SK_ERR_CAPACITY: the size was asked for
        check(rc, "sk_mp3_codebook_flatten")
    out = np.zeros(n.value, np.uint32)
    check(lib.sk_mp3_codebook_flatten(codebook._h, _ptr(out), out.size, C.byref(n)), "sk_mp3_codebook_flatten")
    return out


def set_codebook(codebook=None, engine=None):
    """the code book of the engine's device Huffman stage; None: the standard's tables"""
    engine = engine or default_engine()
    check(lib.sk_mp3_set_codebook(engine._h, codebook._h if codebook is not None else None), "sk_mp3_set_codebook", engine._h)


def pack_frames(frames):
    """frames: iterable of (Mp3FrameInfo, Mp3SideInfo, main data bytes) -> (Mp3FrameItem array, n, uint8 buffer) laid out as
    sk_mp3_entropy_decode / sk_mp3_decode_frames_* take them (offsets multiples of 4, 8 zero bytes behind each)"""
    frames = list(frames)
    items = (Mp3FrameItem * max(len(frames), 1))()
    at, chunks = 0, []
    for i, (info, side, main) in enumerate(frames):
        main = bytes(main)
        C.memmove(C.byref(items[i].header), C.byref(info), C.sizeof(Mp3FrameInfo))
        C.memmove(C.byref(items[i].side), C.byref(side), C.sizeof(Mp3SideInfo))
        items[i].byte_offset, items[i].byte_len = at, len(main)
        room = (len(main) + 8 + 3) & ~3
        chunks.append(main + bytes(room - len(main)))
        at += room
    buf = np.frombuffer(b"".join(chunks) or bytes(8), np.uint8)
    return items, len(frames), buf


def entropy_decode(items, n, buf, engine=None, out=None):
    """sk_mp3_entropy_decode -> (status, Mp3GranuleData[n][2][2]); only the cells a frame has are written"""
    engine = engine or default_engine()
    if out is None:
        out = (((Mp3GranuleData * 2) * 2) * max(n, 1))()
    return lib.sk_mp3_entropy_decode(engine._h, items, n, _ptr(buf), buf.size, out), out


def decode_frames(items, streams, n, buf, engine=None, s16=False, out_cap=None):
    """sk_mp3_decode_frames_* -> (status, pcm[:written], entropy_status[n], stage_status[n])"""
    engine = engine or default_engine()
    streams = np.ascontiguousarray(streams, np.uint32)
    cap = n * MAX_SAMPLES_PER_FRAME if out_cap is None else out_cap
    pcm = np.zeros(max(cap, 1), np.int16 if s16 else np.float32)
    es, ss = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    written = C.c_size_t(0)
    fn = lib.sk_mp3_decode_frames_s16 if s16 else lib.sk_mp3_decode_frames_f32
    rc = fn(engine._h, items, _ptr(streams), n, _ptr(buf), buf.size, _ptr(pcm), cap, _ptr(es), _ptr(ss), C.byref(written))
    return rc, pcm[:written.value], es[:n], ss[:n]


MAX_SAMPLES_PER_FRAME = 2304


# ---- Layer I / II: the host front (csrc/mp12_bitstream.cpp) and the stage call (csrc/mp12_synth.hip) ---------------------------

def mpa_parse_header(data):
    """4 bytes of any layer -> (status, MpaFrameInfo)"""
    info = MpaFrameInfo()
    b = _bytes(data)
    return lib.sk_mpa_parse_header(_ptr(b), len(data), C.byref(info)), info


def mpa_scan(data, layer=0, cap=1 << 16):
    """sk_mpa_scan: frames of one layer (0: that of the first confirmed frame) -> ([MpaFrameInfo], bytes consumed, layer)"""
    frames = (MpaFrameInfo * cap)()
    n, used, lay = C.c_uint32(0), C.c_size_t(0), C.c_uint32(layer)
    b = _bytes(data)
    check(lib.sk_mpa_scan(_ptr(b), len(data), C.byref(lay), frames, cap, C.byref(n), C.byref(used)), "sk_mpa_scan")
    return [frames[i] for i in range(min(n.value, cap))], used.value, lay.value


def mpa_parse_frame(frame, info):
    """one Layer I / II frame -> (status, MpaFrameRecord): classes, scale factors, where the samples stand"""
    rec = MpaFrameRecord()
    b = _bytes(frame)
    return lib.sk_mpa_parse_frame(_ptr(b), len(frame), C.byref(info), C.byref(rec)), rec


def mpa_pack_frames(frames):
    """frames: iterable of (MpaFrameRecord, frame bytes) -> (record array, n, uint8 buffer) laid out as sk_mpa_decode_frames_* take
    them (offsets multiples of 4, 8 zero bytes behind each)"""
    frames = list(frames)
    recs = (MpaFrameRecord * max(len(frames), 1))()
    at, chunks = 0, []
    for i, (rec, data) in enumerate(frames):
        data = bytes(data)
        C.memmove(C.byref(recs[i]), C.byref(rec), C.sizeof(MpaFrameRecord))
        recs[i].byte_offset = at
        room = (len(data) + 8 + 3) & ~3
        chunks.append(data + bytes(room - len(data)))
        at += room
    buf = np.frombuffer(b"".join(chunks) or bytes(8), np.uint8)
    return recs, len(frames), buf


def mpa_decode_frames(recs, streams, n, buf, engine=None, s16=False, out_cap=None, timed=False):
    """sk_mpa_decode_frames_* -> (status, pcm[:written], status[n]) and, with timed (s16 only), the launch's HIP-event milliseconds"""
    engine = engine or default_engine()
    streams = np.ascontiguousarray(streams, np.uint32)
    cap = n * MAX_SAMPLES_PER_FRAME if out_cap is None else out_cap
    pcm = np.zeros(max(cap, 1), np.int16 if (s16 or timed) else np.float32)
    st = np.zeros(max(n, 1), np.int32)
    written = C.c_size_t(0)
    if timed:
        ms = C.c_float(0.0)
        rc = lib.sk_mpa_decode_frames_timed(engine._h, recs, _ptr(streams), n, _ptr(buf), buf.size, _ptr(pcm), cap, _ptr(st), C.byref(written), C.byref(ms))
        return rc, pcm[:written.value], st[:n], ms.value
    fn = lib.sk_mpa_decode_frames_s16 if s16 else lib.sk_mpa_decode_frames_f32
    rc = fn(engine._h, recs, _ptr(streams), n, _ptr(buf), buf.size, _ptr(pcm), cap, _ptr(st), C.byref(written))
    return rc, pcm[:written.value], st[:n]


class Mp3Decoder:
    """soundkit-mp3's Mp3Decoder (soundkit-mp3/src/lib.rs:147-374): new / sample_rate / channels / buffer_len / reset /
    decode_i16 / decode_i32 / decode_f32, bytes in at any chunking, interleaved samples out; errors raise SoundkitError.
    All three layers, as nanomp3 behind the reference's: a stream whose first confirmed frame is Layer I or II is unpacked and
    synthesised by csrc/mp12_synth.hip (384 / 1152 samples per channel and frame), with no switch."""

    def __init__(self, codebook=None, engine=None, gpu_entropy=False):
        """gpu_entropy: scale factors and Huffman decode on the GPU as well (sk_mp3_decoder_set_gpu_entropy); same results"""
        self._engine = engine or default_engine()
        self._codebook = codebook  # None: Mp3Decoder::new() -- the standard's tables
        self._h = C.c_void_p()
        check(lib.sk_mp3_decoder_create(self._engine._h, codebook._h if codebook is not None else None, C.byref(self._h)),
              "sk_mp3_decoder_create", self._engine._h)
        if gpu_entropy:
            self.set_gpu_entropy(True)

    def set_gpu_entropy(self, on):
        check(lib.sk_mp3_decoder_set_gpu_entropy(self._h, 1 if on else 0), "sk_mp3_decoder_set_gpu_entropy", self._engine._h)

    def close(self):
        if self._h:
            lib.sk_mp3_decoder_destroy(self._h)
            self._h = C.c_void_p()

    def _info(self):
        rate, ch, n, frames = C.c_uint32(0), C.c_uint8(0), C.c_size_t(0), C.c_uint64(0)
        check(lib.sk_mp3_decoder_info(self._h, C.byref(rate), C.byref(ch), C.byref(n), C.byref(frames)), "sk_mp3_decoder_info")
        return rate.value, ch.value, n.value, frames.value

    def sample_rate(self):
        return self._info()[0] or None

    def channels(self):
        return self._info()[1] or None

    def buffer_len(self):
        return self._info()[2]

    def frames_decoded(self):
        return self._info()[3]

    def reset(self):
        check(lib.sk_mp3_decoder_reset(self._h), "sk_mp3_decoder_reset")

    def _decode(self, fn, data, out):
        b = _bytes(data)
        n = C.c_size_t(0)
        rc = fn(self._h, _ptr(b), len(data), _ptr(out), out.size, C.byref(n))
        if rc != 0:
            raise SoundkitError(rc, "sk_mp3_decoder_decode", lib.sk_engine_last_hip_error(self._engine._h).decode() if rc in (-3, -4, -8) else "")
        return n.value

    def decode_i16(self, data, out, fec=False):
        assert out.dtype == np.int16
        return self._decode(lib.sk_mp3_decoder_decode_i16, data, out)

    def decode_i32(self, data, out, fec=False):
        assert out.dtype == np.int32
        return self._decode(lib.sk_mp3_decoder_decode_i32, data, out)

    def decode_f32(self, data, out, fec=False):
        assert out.dtype == np.float32
        return self._decode(lib.sk_mp3_decoder_decode_f32, data, out)

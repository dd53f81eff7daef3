"""Core Audio Format, `lpcm` and `alac`: the host's chunk walk and packet index (csrc/caf_stream.h: CafAudioIndex,
soundkit-audio-demux/src/caf.rs) and decode_file: soundkit-decoder's decode_seekable_caf_audio (lib.rs:1029-1092).  An ALAC file goes
through the calls alac.decode_caf uses; a PCM file's bytes are the audio: they go to the output stage in the file's byte order, 64-bit
float rounded to f32 on the GPU first (beyond the reference, which refuses 64 bits).

An `lpcm` file's packets -- one frame each in what FFmpeg writes -- are handed out as runs of at most 4096 frames; the concatenated
output is what counts, and the streaming resampler works in 4096-frame blocks whatever the grouping."""
import ctypes as C

import numpy as np

from ._lib import CafInfo, SoundkitError, check, lib
from .engine import _ptr

ERR_STREAM = -1301
CODECS = {1: "alac", 2: "pcm"}


def _bytes(data):
    return np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)


class CafIndex:
    """CafAudioIndex: codec ("alac" / "pcm"), format_id, sample_rate, channels, bits_per_sample (0: none stated), format_flags,
    big_endian / is_float / bytes_per_frame (pcm), frames_per_packet (of a packet of the file), valid / priming / remainder frames,
    codec_private (the kuki chunk) and packets = [(absolute offset, size, frames, first frame on the file's timeline)]: the file's
    packets for alac, runs of them for pcm"""

    def __init__(self, handle):
        try:
            info = CafInfo()
            rc = lib.sk_caf_index_info(handle, C.byref(info), None, 0)
            if rc not in (0, -7):
                check(rc, "sk_caf_index_info")
            cookie = np.zeros(max(int(info.cookie_len), 1), np.uint8)
            check(lib.sk_caf_index_info(handle, C.byref(info), _ptr(cookie), cookie.size), "sk_caf_index_info")
            self.codec, self.format_id = CODECS[info.codec], bytes(info.format_id).decode("latin-1")
            for n in ("sample_rate", "channels", "bits_per_sample", "format_flags", "bytes_per_frame", "frames_per_packet", "priming_frames",
                      "remainder_frames", "valid_frames"):
                setattr(self, n, int(getattr(info, n)))
            self.big_endian, self.is_float = bool(info.big_endian), bool(info.is_float)
            self.codec_private = cookie[:info.cookie_len].tobytes()
            n = int(info.n_packets)
            offsets, starts = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
            sizes, frames = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
            check(lib.sk_caf_index_packets(handle, _ptr(offsets), _ptr(sizes), _ptr(frames), _ptr(starts), n), "sk_caf_index_packets")
            self.packets = [(int(offsets[i]), int(sizes[i]), int(frames[i]), int(starts[i])) for i in range(n)]
        finally:
            lib.sk_caf_index_destroy(handle)

    @classmethod
    def from_file(cls, data):
        b = _bytes(data)
        h, text = C.c_void_p(), C.create_string_buffer(256)
        rc = lib.sk_caf_index_from_file(_ptr(b), len(data), C.byref(h), text, len(text))
        if rc != 0:
            raise SoundkitError(rc, "sk_caf_index_from_file", text.value.decode())
        return cls(h)

    @classmethod
    def new(cls, description, magic_cookie, packet_table, data_payload_offset, data_payload_size):
        """CafAudioIndex::from_metadata; packet_table None: the file holds no pakt chunk"""
        d, k = _bytes(description), _bytes(magic_cookie)
        t = _bytes(packet_table) if packet_table is not None else None
        h, text = C.c_void_p(), C.create_string_buffer(256)
        rc = lib.sk_caf_index_create(_ptr(d), len(description), _ptr(k), len(magic_cookie), _ptr(t) if t is not None else None,
                                     len(packet_table) if packet_table is not None else 0, data_payload_offset, data_payload_size, C.byref(h), text,
                                     len(text))
        if rc != 0:
            raise SoundkitError(rc, "sk_caf_index_create", text.value.decode())
        return cls(h)

    def packet_bytes(self, data):
        """the packets (runs) of the file the index was made from"""
        return [bytes(data[o:o + s]) for o, s, _, _ in self.packets]

    def trim(self, index, decoded_frames):
        """pcm_packet_trim (caf.rs:365-393): the frames of packet `index` that lie in the programme -> (first frame, count) or None"""
        start = self.packets[index][3]
        lo, hi = max(start, self.priming_frames), min(start + decoded_frames, self.priming_frames + self.valid_frames)
        return (lo - start, hi - lo) if hi > lo else None


def decode_file(data, options=None, scheduler=None, engine=None):
    """decode_seekable_caf_audio: index -> every packet decoded -> each trimmed by priming / valid frames -> the output options ->
    the resampler's flush.  -> (the index, [AudioData]).  With no options a PCM file's AudioData keep its bytes and byte order."""
    from . import alac, mp4
    index = CafIndex.from_file(data)
    packets = index.packet_bytes(data)
    is_float = big_endian = False
    if index.codec == "alac":
        try:
            cfg = alac.parse_cookie(index.codec_private)
        except SoundkitError as e:
            raise SoundkitError(e.status, "decode_file", "Decoder initialization failed: %s" % e)
        pcm, status, frames = alac.decode_packets(cfg, packets, engine)
        for i, st in enumerate(status):
            if st != 0:
                raise SoundkitError(alac.ERR_STREAM, "decode_file", "Decoding failed: ALAC packet %d: %s" % (i, lib.sk_strerror(st).decode()))
        rate, channels, bits = cfg["sample_rate"], cfg["channels"], cfg["bit_depth"]
    else:
        rate, channels = index.sample_rate, index.channels
        frames = [f for _, _, f, _ in index.packets]
        pcm, bits, big_endian = mp4.container_pcm(b"".join(packets), rate, channels, index.bits_per_sample, index.is_float, index.big_endian, engine)
        is_float = index.is_float
    width = channels * (bits // 8)
    pieces, at = [], 0
    for i, n in enumerate(frames):
        t = index.trim(i, n)
        if t:
            pieces.append(pcm[at + t[0] * width:at + (t[0] + t[1]) * width])
        at += n * width
    if not pieces:
        raise SoundkitError(ERR_STREAM, "decode_file", "Decoding failed: CAF track emitted no audio frames")
    return index, alac.output_stage(pieces, rate, channels, bits, options, scheduler, is_float=is_float, big_endian=big_endian)

"""The generic CAF index on the host (csrc/caf_stream.h) through the C ABI: the five PCM fixtures against the hashes the reference's
tests record for them, every `lpcm` rejection with its text, the chunk walk's refusals, and an ALAC file indexed the same through the
generic index and through the ALAC-only one that came before it.  No GPU.  (The sanitizer fuzz of the CAF header: test_mp4_pcm_cpu.py.)"""
import hashlib
import json
import os
import struct

import numpy as np
import pytest

from soundkit_amd import SoundkitError, alac, caf

HERE = os.path.dirname(os.path.abspath(__file__))
CAF = os.path.join(HERE, "golden", "caf_pcm")
HASHES = json.load(open(os.path.join(HERE, "golden", "mov_pcm", "pcm_hashes.json")))["caf_pcm"]
ALAC_FILE = os.path.join(HERE, "golden", "alac", "A_Tusk_is_used_to_make_costly_gifts.caf")
FLOAT, LITTLE = 1, 2


def desc(format_id=b"lpcm", flags=LITTLE, bytes_per_packet=4, frames_per_packet=1, channels=2, bits=16, rate=48000.0):
    return struct.pack(">d4sIIIII", rate, format_id, flags, bytes_per_packet, frames_per_packet, channels, bits)


def chunk(name, payload, size=None):
    return name + struct.pack(">q", len(payload) if size is None else size) + payload


def caf_file(description, payload, more=b"", open_ended=False):
    return b"caff\0\1\0\0" + chunk(b"desc", description) + more + chunk(b"data", bytes(4) + payload, -1 if open_ended else None)


def refusal(data):
    with pytest.raises(SoundkitError) as e:
        caf.CafIndex.from_file(data)
    assert "CafStreamRejected" in str(e.value)
    return str(e.value)


@pytest.mark.parametrize("name", sorted(HASHES))
def test_pcm_fixture_is_described_and_its_payload_has_the_recorded_hash(name):
    want = HASHES[name]
    data = open(os.path.join(CAF, name), "rb").read()
    ix = caf.CafIndex.from_file(data)
    width = 2 * want["bits"] // 8
    assert (ix.codec, ix.format_id, ix.sample_rate, ix.channels, ix.bits_per_sample, ix.big_endian, ix.is_float, ix.bytes_per_frame) == \
        ("pcm", "lpcm", 48000, 2, want["bits"], want["big_endian"], want["float"], width)
    assert (ix.valid_frames, ix.priming_frames, ix.remainder_frames, ix.frames_per_packet, ix.codec_private) == (4800, 0, 0, 1, b"")
    # one frame per packet in the file: handed out as runs of at most 4096 frames
    assert [(size, frames, start) for _, size, frames, start in ix.packets] == [(4096 * width, 4096, 0), (704 * width, 704, 4096)]
    payload = b"".join(ix.packet_bytes(data))
    if want["big_endian"]:
        payload = np.frombuffer(payload, np.uint8).reshape(-1, want["bits"] // 8)[:, ::-1].tobytes()
    assert hashlib.sha256(payload).hexdigest() == want["sha256"]
    assert ix.trim(0, 4096) == (0, 4096) and ix.trim(1, 704) == (0, 704)


def test_runs_follow_the_packet_geometry():
    ix = caf.CafIndex.from_file(caf_file(desc(bytes_per_packet=4 * 1000, frames_per_packet=1000), bytes(4 * 9500 - 4 * 500)))
    assert [(s, f, t) for _, s, f, t in ix.packets] == [(16000, 4000, 0), (16000, 4000, 4000), (4000, 1000, 8000)]  # four whole packets a run
    ix = caf.CafIndex.from_file(caf_file(desc(bytes_per_packet=4 * 5000, frames_per_packet=5000), bytes(4 * 10000)))
    assert [(s, f) for _, s, f, _ in ix.packets] == [(20000, 5000)] * 2  # a packet larger than a run stays whole
    ix = caf.CafIndex.from_file(caf_file(desc(), bytes(4 * 10), open_ended=True))  # a data chunk of size -1 runs to the end of the file
    assert [(s, f) for _, s, f, _ in ix.packets] == [(40, 10)]
    # the reference counts a packet table's entries against its bytes even where no sizes follow: a table beside constant packets is refused
    pakt = chunk(b"pakt", struct.pack(">qqii", 10, 7, 2, 1))
    assert "CAF packet count exceeds its variable-length table" in refusal(caf_file(desc(), bytes(40), pakt))


def test_lpcm_rejections():
    assert "CAF LPCM bits per channel is zero" in refusal(caf_file(desc(bits=0), bytes(40)))
    assert "CAF float PCM must use 32-bit or 64-bit samples" in refusal(caf_file(desc(flags=FLOAT, bits=16), bytes(40)))
    assert "CAF float PCM must use 32-bit or 64-bit samples" in refusal(caf_file(desc(flags=FLOAT | LITTLE, bits=24, bytes_per_packet=6), bytes(36)))
    pakt = chunk(b"pakt", struct.pack(">qqii", 2, 2, 0, 0) + bytes([20, 20]))
    assert "CAF LPCM requires a constant packet size" in refusal(caf_file(desc(bytes_per_packet=0), bytes(40), pakt))
    assert "CAF LPCM packet geometry is not frame-aligned" in refusal(caf_file(desc(bytes_per_packet=10, frames_per_packet=4), bytes(40)))
    assert "CAF LPCM packet geometry is not frame-aligned" in refusal(caf_file(desc(bytes_per_packet=2, frames_per_packet=4), bytes(40)))
    assert "CAF LPCM bytes per frame cannot hold its channels" in refusal(caf_file(desc(bytes_per_packet=3), bytes(39)))
    assert "CAF LPCM frames padded beyond their channels are unsupported" in refusal(caf_file(desc(bits=24, bytes_per_packet=8), bytes(40)))
    assert "unsupported CAF audio format aac " in refusal(caf_file(desc(format_id=b"aac "), bytes(40)))
    assert "CAF frames per packet is zero" in refusal(caf_file(desc(frames_per_packet=0), bytes(40)))
    assert "CAF constant packet size does not divide the data chunk" in refusal(caf_file(desc(), bytes(41)))
    assert "CAF channel count is outside 1...255" in refusal(caf_file(desc(channels=0), bytes(40)))
    assert "CAF channel count is outside 1...255" in refusal(caf_file(desc(channels=256), bytes(40)))
    assert "CAF bits per channel exceeds 255" in refusal(caf_file(desc(bits=256), bytes(40)))
    assert "invalid CAF sample rate" in refusal(caf_file(desc(rate=44100.5), bytes(40)))
    assert "invalid CAF sample rate" in refusal(caf_file(desc(rate=float("nan")), bytes(40)))
    assert "CAF packet table count disagrees with constant packet data" in refusal(caf_file(desc(), bytes(40), chunk(b"pakt", struct.pack(">qqii", 0, 0, 0, 0))))


def test_chunk_walk_refusals():
    good = caf_file(desc(), bytes(40))
    assert "CAF source ends before its 8-byte file header" in refusal(b"caff\0\1")
    assert "CAF source does not start with caff" in refusal(b"caf!" + good[4:])
    assert "unsupported CAF header version=2 flags=0" in refusal(b"caff\0\2\0\0" + good[8:])
    assert "unsupported CAF header version=1 flags=5" in refusal(b"caff\0\1\0\5" + good[8:])
    assert "CAF source ends before a chunk header" in refusal(good + b"free")
    assert "CAF chunk desc cannot have an unknown size" in refusal(b"caff\0\1\0\0" + chunk(b"desc", desc(), -1))
    assert "CAF chunk has invalid negative size -2" in refusal(b"caff\0\1\0\0" + chunk(b"free", b"", -2))
    assert "CAF chunk data exceeds the source length" in refusal(good[:-1])
    assert "CAF chunk desc exceeds the 32 byte metadata budget" in refusal(b"caff\0\1\0\0" + chunk(b"desc", desc() + b"\0") + good[8 + 44:])
    assert "CAF source contains multiple desc chunks" in refusal(caf_file(desc(), bytes(40), chunk(b"desc", desc())))
    assert "CAF source contains multiple data chunks" in refusal(good + chunk(b"data", bytes(8)))
    assert "CAF source is missing its desc chunk" in refusal(b"caff\0\1\0\0" + chunk(b"data", bytes(8)))
    assert "CAF source is missing its data chunk" in refusal(b"caff\0\1\0\0" + chunk(b"desc", desc()))
    assert "CAF data chunk is shorter than its edit count" in refusal(b"caff\0\1\0\0" + chunk(b"desc", desc()) + chunk(b"data", bytes(3)))
    assert "CAF desc must contain 32 bytes, got 31" in refusal(b"caff\0\1\0\0" + chunk(b"desc", desc()[:31]) + chunk(b"data", bytes(8)))
    caf.CafIndex.from_file(caf_file(desc(), bytes(40), chunk(b"free", bytes(100)) + chunk(b"chan", bytes(12))))  # unknown chunks are stepped over


def test_an_alac_file_indexes_as_it_did():
    data = open(ALAC_FILE, "rb").read()
    new, old = caf.CafIndex.from_file(data), alac.CafAlacPacketIndex.from_file(data)
    assert new.codec == "alac" and new.format_id == "alac"
    assert [(o, s) for o, s, _, _ in new.packets] == old.packets and len(old.packets) > 1
    assert [f for _, _, f, _ in new.packets] == [old.frames_per_packet] * len(old.packets)
    assert [t for _, _, _, t in new.packets] == [i * old.frames_per_packet for i in range(len(old.packets))]
    assert (new.valid_frames, new.priming_frames, new.remainder_frames, new.frames_per_packet) == \
        (old.valid_frames, old.priming_frames, old.remainder_frames, old.frames_per_packet)
    assert alac.parse_cookie(new.codec_private) == old.config and (new.sample_rate, new.channels) == (old.sample_rate, old.channels)
    assert [new.trim(i, old.frames_per_packet) for i in range(len(old.packets))] == [old.trim(i, old.frames_per_packet) for i in range(len(old.packets))]
    # the ALAC-only index keeps its own text for a description that is not ALAC
    with pytest.raises(SoundkitError, match="CAF audio description is not ALAC"):
        alac.CafAlacPacketIndex.new(desc(), b"", b"", 0, 44)
    # from_metadata, the chunks handed over one by one
    at = data.find(b"desc") + 12
    d = data[at:at + 32]
    k_at = data.find(b"kuki")
    k = data[k_at + 12:k_at + 12 + struct.unpack(">q", data[k_at + 4:k_at + 12])[0]]
    p_at = data.find(b"pakt")
    p = data[p_at + 12:p_at + 12 + struct.unpack(">q", data[p_at + 4:p_at + 12])[0]]
    d_at = data.find(b"data")
    size = struct.unpack(">q", data[d_at + 4:d_at + 12])[0]
    size = len(data) - d_at - 12 if size < 0 else size
    pieces = caf.CafIndex.new(d, k, p, d_at + 12, size)
    assert pieces.packets == new.packets and pieces.valid_frames == new.valid_frames

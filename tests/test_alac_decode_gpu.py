"""The ALAC decode stage on the GPU (csrc/alac_decode.hip through sk_alac_decode_packets and AlacPacketDecoder) against
tests/alac_model.py, bit for bit, at the smallest shapes that can still go wrong: the predictor orders the kernels take another path for
(0, 31, and one in each register size), packets of 1, 2, order and order + 1 frames where the warm-up branches end, every quantiser
shift, prediction type 15, full-scale material that wraps the 32-bit sums and runs the coefficient walk to its end, k at the Rice limit,
escapes, a pinned history, zero runs of 1 and of 0xFFFF and one that ends at the last sample, pairs on odd sums, extra bytes, an
uncompressed element, DSE and FIL, 1 ... 8 channels, 130 packets of mixed length in one call, every rejection beside intact
neighbours, and the reference's fixture against its twin.

Every built packet (tests/alac_cases.py) is written by tests/alac_builder.py from the samples the decoder must return; test_alac_cpu.py
shows that the model decodes each back to those samples."""
import os

import pytest

import alac_builder as B
import alac_cases as CASES
import alac_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "alac")
FIXTURE = os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts.caf")
TWIN = os.path.join(GOLDEN, "A_Tusk_is_used_to_make_costly_gifts.decoded.wav")
OK, INVALID, ELEMENT, UNSUPPORTED = 0, -601, -603, -6
FILL = 0xA5


def split(pcm, cfg, frames):
    width = cfg["channels"] * (cfg["bit_depth"] // 8)
    out, at = [], 0
    for n in frames:
        out.append(pcm[at:at + n * width])
        at += n * width
    assert at == len(pcm)
    return out


def model_status(cfg, packet):
    try:
        chans, _ = M.decode_packet(cfg, packet)
        return OK, M.pcm_bytes(chans, cfg["bit_depth"])
    except M.AlacError as e:
        return {M.INVALID: INVALID, M.ELEMENT: ELEMENT, M.UNSUPPORTED: UNSUPPORTED}[e.kind], None


@pytest.fixture(scope="module")
def decoded():
    """every built case through the product, one call per cookie -> {name: [(status, frames, bytes)]}"""
    from soundkit_amd import alac
    groups = {}
    for name, cfg, packets in CASES.cases():
        groups.setdefault(tuple(sorted(cfg.items())), []).append((name, packets))
    out = {}
    for key, members in groups.items():
        cfg = dict(key)
        flat = [p for _, packets in members for p, _ in packets]
        pcm, status, frames = alac.decode_packets(cfg, flat, fill=FILL)
        pieces = split(pcm, cfg, frames)
        at = 0
        for name, packets in members:
            out[name] = list(zip(status[at:at + len(packets)], frames[at:at + len(packets)], pieces[at:at + len(packets)]))
            at += len(packets)
    return out


@pytest.mark.parametrize("case", CASES.cases(), ids=lambda c: c[0])
def test_built_packets_bit_for_bit(case, decoded):
    name, cfg, packets = case
    for (packet, chans), (status, frames, pcm) in zip(packets, decoded[name]):
        assert status == OK and frames == len(chans[0])
        assert pcm == M.pcm_bytes(chans, cfg["bit_depth"])


def test_fixture_against_its_twin():
    from soundkit_amd import alac
    data = open(FIXTURE, "rb").read()
    twin = open(TWIN, "rb").read()
    twin = twin[twin.index(b"data") + 8:]
    ix = alac.CafAlacPacketIndex.from_file(data)
    pcm, status, frames = alac.decode_packets(ix.config, ix.packet_bytes(data))
    assert status == [OK] * 6 and frames == [4096] * 5 + [3200]
    assert len(pcm) == 2 * 23680 and pcm == twin


def test_130_packets_of_mixed_lengths_map_back_to_packet_order():
    from soundkit_amd import alac
    cfg, packets = CASES.many()
    pcm, status, frames = alac.decode_packets(cfg, [p for p, _ in packets], fill=FILL)
    assert status == [OK] * 130 and frames == [len(ch[0]) for _, ch in packets]
    assert split(pcm, cfg, frames) == [M.pcm_bytes(ch, 16) for _, ch in packets]


def test_a_33_bit_pair_is_unsupported():
    from soundkit_amd import alac
    cfg = B.config(4096, 32, 2, 48000)
    good = CASES.signal("rand", 40, 32, 1, 2)
    packets = [B.packet(cfg, good, extra_bytes=1, order=2, shift=4), B.packet(cfg, good, order=2, shift=4), B.packet(cfg, good, raw=True),
               B.packet(cfg, good, extra_bytes=2, order=2, shift=4)]
    pcm, status, frames = alac.decode_packets(cfg, packets, fill=FILL)
    assert status == [OK, UNSUPPORTED, UNSUPPORTED, OK] == [model_status(cfg, p)[0] for p in packets]
    want = M.pcm_bytes(good, 32)
    assert split(pcm, cfg, frames) == [want, bytes([FILL]) * len(want), bytes([FILL]) * len(want), want]


def rejections():
    """(name, cfg, bad packet, its status)"""
    m16, s16 = B.config(4096, 16, 1, 44100), B.config(4096, 16, 2, 44100)
    mono, pair, silent = CASES.signal("tone", 100, 16), CASES.signal("tone", 100, 16, 0, 2), CASES.signal("silence", 100, 16)
    out = [(f"tag{tag}", m16, B.packet(m16, mono, before=lambda w, tag=tag: w.put(tag, 3)), ELEMENT) for tag in (2, 5)]
    two = B.BitWriter()
    B.write_element(two, s16, B.Element("sce", has_size=True), [pair[0]])
    two.put(2, 3)
    out.append(("tag2_behind_an_element", s16, two.bytes() + bytes(4), ELEMENT))
    out.append(("prediction_type_3", m16, B.packet(m16, mono, ptype=3), INVALID))
    out.append(("run_past_the_end", m16, B.packet(m16, silent, elements=[B.Element(order=0, n_override=50, has_size=True)]), INVALID))
    out.append(("count_above_frame_length", m16, B.packet(m16, mono, elements=[B.Element(n_override=4097, has_size=True)]), INVALID))
    out.append(("count_zero", m16, B.packet(m16, mono, elements=[B.Element(n_override=0, has_size=True)]), INVALID))
    differ = B.BitWriter()
    B.write_element(differ, s16, B.Element("sce", has_size=True), [pair[0]])
    B.write_element(differ, s16, B.Element("sce", has_size=True), [pair[1][:90]])
    differ.put(7, 3)
    out.append(("elements_with_different_counts", s16, differ.bytes(), INVALID))
    out.append(("one_channel_short", s16, B.packet(s16, pair[:1], elements=[B.Element("sce")]), INVALID))
    out.append(("one_channel_more", m16, B.packet(m16, pair, elements=[B.Element("cpe")]), INVALID))
    out.append(("no_end", m16, B.packet(m16, mono, end=False), INVALID))
    out.append(("a_byte_behind_end", m16, B.packet(m16, mono) + b"\0", INVALID))
    out.append(("dse_past_the_end", m16, B.packet(m16, mono, before=lambda w: [w.put(v, n) for v, n in ((4, 3), (0, 4), (0, 1), (255, 8), (255, 8))]),
                INVALID))
    out.append(("fil_behind_the_element_past_the_end", m16, B.packet(m16, mono, end=False) + bytes([0xDF, 0xFF]), INVALID))
    return out


@pytest.mark.parametrize("case", rejections(), ids=lambda c: c[0])
def test_each_rejection_gets_its_status_and_its_neighbours_stay_exact(case):
    from soundkit_amd import alac
    _, cfg, bad, want_status = case
    assert model_status(cfg, bad)[0] == want_status
    good = CASES.signal("tone", 120, 16, 3, cfg["channels"])
    before, after = B.packet(cfg, good, order=4, shift=6), B.packet(cfg, [c[:77] for c in good], order=8, shift=5)
    pcm, status, frames = alac.decode_packets(cfg, [before, bad, after], fill=FILL)
    assert status == [OK, want_status, OK] and frames[0] == 120 and frames[2] == 77
    pieces = split(pcm, cfg, frames)
    assert pieces[0] == M.pcm_bytes(good, 16) and pieces[2] == M.pcm_bytes([c[:77] for c in good], 16)
    assert pieces[1] == bytes([FILL]) * len(pieces[1])  # the rejected packet keeps its place and nothing is written there


def test_a_packet_cut_short_at_every_eighth_byte():
    from soundkit_amd import alac
    cfg = B.config(4096, 24, 2, 48000)
    good = CASES.signal("tone", 150, 24, 5, 2)
    whole = B.packet(cfg, good, order=4, shift=6, extra_bytes=1, mix_weight=1, mix_shift=2, dse=b"abcdef")
    cuts = [whole[:k] for k in range(1, len(whole), 8)]
    packets = [whole] + [p for cut in cuts for p in (cut, whole)]
    pcm, status, frames = alac.decode_packets(cfg, packets, fill=FILL)
    want = M.pcm_bytes(good, 24)
    pieces = split(pcm, cfg, frames)
    for i, packet in enumerate(packets):
        if i % 2 == 0:
            assert status[i] == OK and pieces[i] == want
        else:
            assert status[i] == INVALID == model_status(cfg, packet)[0], (i, len(packet))
            assert pieces[i] == bytes([FILL]) * len(pieces[i])


def test_damaged_packets_agree_with_the_model():
    """single bit flips anywhere in a packet: the product's status is the model's, and an accepted packet's samples are the model's"""
    import random
    from soundkit_amd import alac
    rng = random.Random(11)
    cfg = B.config(4096, 16, 2, 44100)
    good = CASES.signal("tone", 200, 16, 9, 2)
    whole = B.packet(cfg, good, order=4, shift=6, mix_weight=1, mix_shift=2)
    packets = []
    for _ in range(120):
        p = bytearray(whole)
        p[rng.randrange(len(p) if rng.random() < 0.5 else 12)] ^= 1 << rng.randrange(8)
        packets.append(bytes(p))
    pcm, status, frames = alac.decode_packets(cfg, packets, fill=FILL)
    pieces = split(pcm, cfg, frames)
    accepted = 0
    for packet, st, piece in zip(packets, status, pieces):
        want_status, want = model_status(cfg, packet)
        assert st == want_status
        if st == OK:
            accepted += 1
            assert piece == want
        else:
            assert piece == bytes([FILL]) * len(piece)
    assert 0 < accepted < 120


def test_bad_tables_are_refused_before_anything_runs():
    import ctypes as C
    import numpy as np
    from soundkit_amd import alac, default_engine
    from soundkit_amd._lib import AlacPacket, lib
    from soundkit_amd.engine import _ptr
    cfg = B.config(4096, 16, 1, 44100)
    packet = B.packet(cfg, CASES.signal("tone", 64, 16))
    e = default_engine()

    def call(cfg, table, n, src, out_cap=1 << 16):
        out = np.full(1 << 16, FILL, np.uint8)
        status, frames, used = np.full(4, 99, np.int32), np.zeros(4, np.uint32), C.c_size_t(7)
        rc = lib.sk_alac_decode_packets(e._h, C.byref(alac.config(cfg)), table, n, _ptr(src), _ptr(out), out_cap, C.byref(used), _ptr(status), _ptr(frames))
        assert (out == FILL).all() or rc == 0
        return rc, used.value

    src = np.frombuffer(bytes(16) + packet + bytes(16), np.uint8)
    table = (AlacPacket * 2)()
    table[0].offset, table[0].size = 16, len(packet)
    assert call(cfg, table, 1, src) == (0, 128)
    table[0].size = 0  # an empty packet
    assert call(cfg, table, 1, src) == (-1, 0)
    table[0].size = 16 * 1024 * 1024 + 1
    assert call(cfg, table, 1, src) == (-1, 0)
    table[0].offset, table[0].size = 8, len(packet)  # not a multiple of 16
    assert call(cfg, table, 1, src) == (-1, 0)
    table[0].offset = 16
    assert call(cfg, table, 1, src, out_cap=127) == (-1, 0)  # no room
    for change in (dict(channels=0), dict(channels=9), dict(bit_depth=20), dict(frame_length=0), dict(frame_length=65537), dict(sample_rate=0)):
        assert call(dict(cfg, **change), table, 1, src) == (-1, 0)
    assert call(cfg, table, 0, src) == (0, 0)


def test_packet_decoder_on_the_fixture_its_texts_and_the_empty_packet():
    from soundkit_amd import SoundkitError, alac
    data = open(FIXTURE, "rb").read()
    twin = open(TWIN, "rb").read()
    twin = twin[twin.index(b"data") + 8:]
    at, size = M.caf_chunks(data)["kuki"]
    cookie = data[at:at + size]
    ix = alac.CafAlacPacketIndex.from_file(data)
    d = alac.AlacPacketDecoder(cookie)
    assert (d.sample_rate(), d.channels(), d.bit_depth(), d.maximum_pcm_samples()) == (8000, 1, 16, 4096)
    packets = ix.packet_bytes(data)
    out = b""
    for i, p in enumerate(packets):
        if i == 2:  # errors in between do not disturb the packets that follow
            with pytest.raises(SoundkitError) as e:
                d.decode_packet(b"")
            assert e.value.status == alac.ERR_STREAM and "ALAC packet is empty" in str(e.value) and d.last_error() == "ALAC packet is empty"
            with pytest.raises(SoundkitError) as e:
                d.decode_packet(p[:len(p) // 2])
            assert "ALAC packet: invalid ALAC packet" in str(e.value)
            with pytest.raises(SoundkitError) as e:
                d.decode_packet(bytes([0x40]) + p)
            assert "ALAC packet: unsupported ALAC element" in str(e.value)
        a = d.decode_packet(p)
        assert (a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 8000)
        out += a.data.tobytes()
    assert out == twin
    d.close()
    # the MP4 form of the same cookie, and what a cookie is refused for
    assert alac.AlacPacketDecoder(bytes(4) + cookie[-24:]).decode_packet(packets[5]).data.tobytes() == twin[-6400:]
    with pytest.raises(SoundkitError) as e:
        alac.AlacPacketDecoder(cookie[-24:-1])
    assert "ALAC magic cookie is shorter than 24 bytes" in str(e.value)
    with pytest.raises(SoundkitError) as e:
        alac.AlacPacketDecoder(cookie[-24:-19] + bytes([20]) + cookie[-18:])
    assert "Unsupported ALAC bit depth: 20" in str(e.value)
    with pytest.raises(SoundkitError) as e:
        alac.AlacPacketDecoder(cookie).decode_packet(bytes(16 * 1024 * 1024 + 1))
    assert "ALAC packet exceeds the 16777216 byte budget" in str(e.value)

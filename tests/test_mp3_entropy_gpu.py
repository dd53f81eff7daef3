"""Parts 2 and 3 of the Layer III main data on the GPU (csrc/mp3_entropy.hip: sk_mp3_set_codebook, sk_mp3_entropy_decode,
sk_mp3_decode_frames_*, sk_mp3_decoder_set_gpu_entropy) against two references, neither of them the device path: what
tests/mp3_builder.py's writer encoded, and the host stage sk_mp3_decode_main_data.  Every comparison is exact (integers,
bytes, status codes)."""
import ctypes as C
import os

import numpy as np
import pytest

import mp3_builder as B
from oracle import mp3_iso
from soundkit_amd import mp3
from soundkit_amd._lib import SK_OK, Mp3FrameItem, Mp3GranuleData, Mp3GranuleDesc, Mp3RequantGranule, SoundkitError, lib
from soundkit_amd.engine import _ptr

pytestmark = pytest.mark.gpu
NEED_MORE, UNSUPPORTED, INVALID = -301, -303, -304
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mp3")
ISO = mp3_iso.tables()
FIELDS = ("is_", "scalefac_l", "scalefac_s", "preflag", "intensity_scale", "part2_bits", "part3_bits", "nonzero_lines", "status")
RATES = {1: (44100, 48000, 32000), 2: (22050, 24000, 16000), 25: (11025, 12000, 8000)}
MODES = [dict(channels=1), dict(channels=2, mode=0), dict(channels=2, mode=1, joint_modes=(0, 2)), dict(channels=2, mode=1, joint_modes=(1,)),
         dict(channels=2, mode=1, joint_modes=(1, 3)), dict(channels=2, mode=2)]


@pytest.fixture(scope="module")
def iso_codebook():
    cb = mp3.Codebook()
    yield cb
    cb.close()


def stream_params(version, rate, mode, crc):
    kw = dict(version=version, rate=rate, crc=crc, **mode)
    if version != 1:
        kw["bitrate_indices"] = (6, 9, 12) if mode["channels"] == 1 else (8, 10, 13)
    return kw


def split(data):
    """every frame of a stream whose side information and main data the host stages accept -> [(index, info, side, main)]"""
    found, _ = mp3.scan_free(data)[:2]
    kept, out = b"", []
    for i, f in enumerate(found):
        frame = data[f.offset:f.offset + f.frame_bytes]
        rc, side = mp3.parse_side_info(frame, f)
        if rc == SK_OK:
            rc, main = mp3.main_data(frame, f, side, kept)
            if rc == SK_OK:
                out.append((i, f, side, main))
        head = 4 + 2 * f.has_crc + f.side_info_bytes
        kept = (kept + frame[head:])[-2048:]
    return out


def assert_same_cell(dev, host, where):
    for k in FIELDS:
        a, b = getattr(dev, k), getattr(host, k)
        if isinstance(a, int):
            assert a == b, (where, k, a, b)
        else:
            assert bytes(a) == bytes(b), (where, k)


def device_equals_host(engine, codebook, frames, require_good=False):
    """frames: [(info, side, main)] -> (device cells, host cells, host statuses); asserts equality cell by cell"""
    items, n, buf = mp3.pack_frames(frames)
    rc, dev = mp3.entropy_decode(items, n, buf, engine)
    assert rc == SK_OK
    hosts, codes = [], []
    for k, (info, side, main) in enumerate(frames):
        rc, host = mp3.decode_main_data(codebook, info, side, main)
        hosts.append(host)
        codes.append(rc)
        worst = SK_OK
        for gr in range(side.granules):
            for ch in range(side.channels):
                h = host[gr][ch]
                if require_good:  # the inputs are known good before the device is asked
                    assert h.status == SK_OK and h.part2_bits + h.part3_bits == side.gr[gr][ch].part2_3_length, (k, gr, ch)
                assert_same_cell(dev[k][gr][ch], h, (k, gr, ch))
                if h.status != SK_OK:
                    assert not any(dev[k][gr][ch].is_), (k, gr, ch)
                    worst = worst or h.status
        assert rc == worst
    return dev, hosts, codes


def assert_is_what_was_written(dev, split_frames, built):
    for k, (index, info, side, _main) in enumerate(split_frames):
        for gr in range(side.granules):
            for ch in range(side.channels):
                g, w = dev[k][gr][ch], built[index]["granules"][gr][ch]
                assert list(g.is_) == w["is"], (index, gr, ch)
                assert list(g.scalefac_l) == w["scalefac_l"] and [list(r) for r in g.scalefac_s] == w["scalefac_s"], (index, gr, ch)
                assert g.preflag == w["preflag"], (index, gr, ch)


# ---- 1. stage parity over the standard's tables ---------------------------------------------------------------------------------

@pytest.mark.parametrize("version,column", [(v, c) for v in (1, 2, 25) for c in range(3)], ids=lambda v: str(v))
def test_stage_equals_writer_and_host_over_the_standards_tables(engine, iso_codebook, version, column):
    rate = RATES[version][column]
    mp3.set_codebook(None, engine)
    seen = {"short": 0, "mixed": 0, "scfsi": 0, "escape": 0, "quads": 0, "reservoir": 0, "marked": 0}
    for m, mode in enumerate(MODES):
        for crc in (False, True):
            data, built = B.build_stream(ISO, 1000 * version + 100 * column + 10 * m + crc, n_frames=10, **stream_params(version, rate, mode, crc))
            frames = split(data)
            assert len(frames) == len(built) == 10
            dev, _, _ = device_equals_host(engine, iso_codebook, [f[1:] for f in frames], require_good=True)
            assert_is_what_was_written(dev, frames, built)
            for k, (index, info, side, _main) in enumerate(frames):
                seen["reservoir"] += side.main_data_begin > 0
                for gr in range(side.granules):
                    for ch in range(side.channels):
                        s, g = side.gr[gr][ch], dev[k][gr][ch]
                        seen["short"] += s.window_switching and s.block_type == 2
                        seen["mixed"] += s.mixed_block_flag
                        seen["scfsi"] += gr == 1 and any(side.scfsi[ch])
                        seen["escape"] += int(np.abs(np.array(g.is_)).max()) > 15
                        seen["quads"] += g.nonzero_lines > 2 * s.big_values
                        seen["marked"] += any(v & 0x80 for v in g.scalefac_l) or any(v & 0x80 for r in g.scalefac_s for v in r)
    assert seen["short"] and seen["mixed"] and seen["escape"] and seen["quads"] and seen["reservoir"], seen
    assert seen["scfsi"] if version == 1 else seen["marked"], seen


# ---- 2. every table, long escapes, random code sets -------------------------------------------------------------------------------

def every_table_frames(tables):
    """tests/test_mp3_decoder.py::test_every_table_and_long_escapes: one granule per big-value table, values up to its maximum"""
    from oracle import mp3_bitstream as ref
    rng = np.random.default_rng(9)
    hb = B.header_bytes(1, 44100, 14, 1, 3, 0, False)
    h = ref.parse_header(hb)
    rc, info = mp3.parse_header(hb)
    assert rc == SK_OK
    out = []
    for t in range(32):
        table = tables["big_values"][t]
        if not table:
            continue
        top = min(8206, table["xlen"] - 1 + ((1 << table["linbits"]) - 1 if table["linbits"] else 0))
        w = B.BitWriter()
        values = [0] * 576
        for line in range(0, 120, 2):
            x, y = (int(rng.integers(-top, top + 1)) for _ in range(2))
            if line == 0:
                x, y = top, -top
            B.put_pair(w, table, x, y)
            values[line], values[line + 1] = x, y
        if len(w) > 4095:
            continue
        s = {"part2_3_length": len(w), "big_values": 60, "global_gain": 100, "scalefac_compress": 0, "window_switching": 0, "block_type": 0,
             "mixed_block_flag": 0, "table_select": [t, t, t], "subblock_gain": [0, 0, 0], "region0_count": 3, "region1_count": 2, "preflag": 0,
             "scalefac_scale": 0, "count1table_select": 0}
        empty = dict(s, part2_3_length=0, big_values=0)
        side_bytes = B.pack_side_info(h, {"main_data_begin": 0, "scfsi": [[0] * 4] * 2, "gr": [[s], [empty]]})
        rc, side = mp3.parse_side_info(hb + side_bytes, info)
        assert rc == SK_OK
        out.append((info, side, w.tobytes(), values))
        if len(w) % 8 == 1:  # one bit short: the bytes do not hold what part2_3_length promises
            out.append((info, side, w.tobytes()[:-1], None))
    return out


@pytest.mark.parametrize("seed", [None, 3, 11, 29], ids=["iso", "random3", "random11", "random29"])
def test_every_table_long_escapes_and_random_code_sets(engine, seed):
    tables = ISO if seed is None else B.make_tables(seed)
    ct, _keep = B.to_ctypes(tables)
    cb = mp3.Codebook(ct)
    try:
        mp3.set_codebook(cb, engine)
        cases = every_table_frames(tables)
        assert len(cases) > 20
        dev, _, codes = device_equals_host(engine, cb, [c[:3] for c in cases])
        cut = 0
        for k, (info, side, main, values) in enumerate(cases):
            if values is None:
                cut += 1
                assert codes[k] == NEED_MORE and dev[k][0][0].status == NEED_MORE and not any(dev[k][0][0].is_)
            else:
                assert codes[k] == SK_OK and list(dev[k][0][0].is_) == values and dev[k][0][0].nonzero_lines == 120
                assert not any(dev[k][1][0].is_)
        assert cut or seed is not None
        for k, kw in enumerate([dict(version=1, rate=44100, channels=2, mode=1, joint_modes=(0, 1, 2, 3)), dict(version=1, rate=32000, channels=1, crc=True),
                                dict(version=2, rate=24000, channels=2, mode=1, joint_modes=(1, 3), bitrate_indices=(8, 10, 13)),
                                dict(version=25, rate=8000, channels=2, mode=2, bitrate_indices=(8, 11))]):
            data, built = B.build_stream(tables, 40 * (seed or 1) + k, n_frames=12, **kw)
            frames = split(data)
            assert len(frames) == 12
            dev, _, _ = device_equals_host(engine, cb, [f[1:] for f in frames], require_good=True)
            assert_is_what_was_written(dev, frames, built)
    finally:
        mp3.set_codebook(None, engine)
        cb.close()


def test_a_rate_the_code_book_lacks_is_unsupported(engine):
    tables = B.make_tables(5, rates=(44100,))
    ct, _keep = B.to_ctypes(tables)
    cb = mp3.Codebook(ct)
    try:
        mp3.set_codebook(cb, engine)
        full = B.make_tables(5)  # the same code sets (one seed), every band table: a stream at a rate `cb` has no bands for
        data, _ = B.build_stream(full, 77, version=1, rate=48000, channels=2, mode=0, n_frames=4)
        frames = split(data)
        dev, _, codes = device_equals_host(engine, cb, [f[1:] for f in frames])
        assert all(c == UNSUPPORTED for c in codes) and dev[0][0][0].status == UNSUPPORTED
    finally:
        mp3.set_codebook(None, engine)
        cb.close()


# ---- 3. damage ------------------------------------------------------------------------------------------------------------------

def copy_side(side):
    fresh = type(side)()
    C.memmove(C.byref(fresh), C.byref(side), C.sizeof(side))
    return fresh


def damaged_frames(data, rng, trials):
    """the mutations of test_damaged_main_data_is_reported_not_followed, plus bit flips and truncations -> [(info, side, main)]"""
    out = []
    for _index, info, side, main in split(data):
        for trial in range(trials):
            bad, hurt = bytearray(main), copy_side(side)
            gr, ch = int(rng.integers(0, side.granules)), int(rng.integers(0, side.channels))
            kind = trial % 6
            if kind == 0:
                for _flip in range(int(rng.integers(1, 6))):
                    bad[int(rng.integers(0, len(bad)))] ^= 1 << int(rng.integers(0, 8))
            elif kind == 1:  # part2_3_length cut short: the big values run past it
                hurt.gr[gr][ch].part2_3_length = max(0, hurt.gr[gr][ch].part2_3_length - int(rng.integers(1, 300)))
            elif kind == 2:  # a region names a table that has no codes
                hurt.gr[gr][ch].table_select[int(rng.integers(0, 2))] = int(rng.choice([4, 14]))
            elif kind == 3:  # the main data ends early
                bad = bad[:int(rng.integers(0, len(bad)))]
            elif kind == 4:  # more big values than lines, or a part2_3_length beyond the data
                if trial % 12 == 4:
                    hurt.gr[gr][ch].big_values = int(rng.integers(289, 512))
                else:
                    hurt.gr[gr][ch].part2_3_length = min(4095, hurt.gr[gr][ch].part2_3_length + int(rng.integers(1, 3000)))
            else:            # scale factors alone longer than part2_3_length; random bytes
                if trial % 12 == 5:
                    hurt.gr[gr][ch].part2_3_length = int(rng.integers(0, 12))
                else:
                    bad = bytearray(rng.integers(0, 256, len(bad), dtype=np.uint8).tobytes())
            out.append((info, hurt, bytes(bad)))
    return out


def test_damaged_main_data_device_equals_host(engine, iso_codebook):
    mp3.set_codebook(None, engine)
    rng = np.random.default_rng(17)
    frames = []
    for k, kw in enumerate([dict(version=1, rate=44100, channels=2, mode=0, bitrate_indices=(9,)), dict(version=1, rate=48000, channels=2, mode=1, joint_modes=(0, 1, 2, 3)),
                            dict(version=2, rate=22050, channels=2, mode=1, joint_modes=(1, 3), bitrate_indices=(8, 10)), dict(version=25, rate=11025, channels=1, bitrate_indices=(6, 9))]):
        data, _ = B.build_stream(ISO, 55 + k, n_frames=6, **kw)
        frames += damaged_frames(data, rng, 24)
    assert len(frames) > 500
    items, n, buf = mp3.pack_frames(frames)
    # guard cells before and behind the output, and the cells a frame does not have, keep their fill pattern
    guard = 3
    raw = np.full((n + 2 * guard) * 4 * C.sizeof(Mp3GranuleData), 0xA5, np.uint8)
    out = (((Mp3GranuleData * 2) * 2) * n).from_buffer(raw, guard * 4 * C.sizeof(Mp3GranuleData))
    rc, dev = mp3.entropy_decode(items, n, buf, engine, out)
    assert rc == SK_OK
    cell = C.sizeof(Mp3GranuleData)
    assert (raw[:guard * 4 * cell] == 0xA5).all() and (raw[(guard + n) * 4 * cell:] == 0xA5).all()
    statuses = {SK_OK: 0, NEED_MORE: 0, INVALID: 0}
    for k, (info, side, main) in enumerate(frames):
        rc, host = mp3.decode_main_data(iso_codebook, info, side, main)
        for gr in range(2):
            for ch in range(2):
                at = ((guard + k) * 4 + gr * 2 + ch) * cell
                if gr >= side.granules or ch >= side.channels:
                    assert (raw[at:at + cell] == 0xA5).all(), (k, gr, ch)
                    continue
                assert_same_cell(dev[k][gr][ch], host[gr][ch], (k, gr, ch))
                statuses[host[gr][ch].status] += 1
                if host[gr][ch].status != SK_OK:
                    assert not any(dev[k][gr][ch].is_)
    assert statuses[SK_OK] > 200 and statuses[NEED_MORE] > 50 and statuses[INVALID] > 100, statuses


# ---- 4. the stage at bench size ------------------------------------------------------------------------------------------------

def test_full_device_batch_equals_host_and_repeats(engine, iso_codebook):
    """2048 stereo streams x 16 MPEG-1 frames = 131 072 granule-channels in one call (64 distinct built streams tiled 32 times)"""
    mp3.set_codebook(None, engine)
    base = []
    for k in range(64):
        data, _ = B.build_stream(ISO, 5000 + k, version=1, rate=(44100, 48000, 32000)[k % 3], channels=2, mode=k % 3, joint_modes=(0, 1, 2, 3), n_frames=16)
        frames = split(data)
        assert len(frames) == 16
        base += [f[1:] for f in frames]
    items, n, buf = mp3.pack_frames(base)
    assert n == 1024
    cell = C.sizeof(Mp3GranuleData)
    want = np.zeros((n, 4 * cell), np.uint8)
    for k, (info, side, main) in enumerate(base):
        rc, host = mp3.decode_main_data(iso_codebook, info, side, main)
        assert rc == SK_OK
        want[k] = np.frombuffer(bytes(host), np.uint8)
    tiles = 32
    words = np.frombuffer(bytes(items), np.uint32).reshape(n, C.sizeof(Mp3FrameItem) // 4)
    tiled = np.tile(words, (tiles, 1))
    tiled[:, Mp3FrameItem.byte_offset.offset // 4] += np.repeat(np.arange(tiles, dtype=np.uint32) * np.uint32(buf.size), n)
    big_buf = np.tile(buf, tiles)
    big_items = (Mp3FrameItem * (n * tiles)).from_buffer(tiled)
    first = np.zeros((n * tiles, 4 * cell), np.uint8)
    rc = lib.sk_mp3_entropy_decode(engine._h, big_items, n * tiles, _ptr(big_buf), big_buf.size, _ptr(first))
    assert rc == SK_OK
    assert np.array_equal(first.reshape(tiles, n, 4 * cell), np.broadcast_to(want, (tiles, n, 4 * cell)))
    second = np.zeros_like(first)
    rc = lib.sk_mp3_entropy_decode(engine._h, big_items, n * tiles, _ptr(big_buf), big_buf.size, _ptr(second))
    assert rc == SK_OK and np.array_equal(first, second)


# ---- 5. the fused chain ----------------------------------------------------------------------------------------------------------

def host_chain(engine, codebook, stream, frames, s16):
    """host Huffman stage + sk_mp3_decode_granules_* over the frames that decode -> (pcm, per frame: decoded?, per frame: stage status)"""
    granules, descs, ints, ok = [], [], [], []
    for info, side, main in frames:
        rc, data = mp3.decode_main_data(codebook, info, side, main)
        ok.append(rc == SK_OK)
        if rc != SK_OK:
            continue
        joint = info.mode == 1
        for gr in range(info.granules):
            g = Mp3RequantGranule()
            g.sample_rate, g.channels, g.lsf = info.sample_rate, info.channels, int(info.version != 1)
            g.ms_stereo, g.intensity_stereo = int(joint and bool(info.mode_ext & 2)), int(joint and bool(info.mode_ext & 1))
            if g.lsf and g.intensity_stereo and info.channels == 2 and data[gr][1].intensity_scale:
                g.intensity_stereo |= 2
            d = Mp3GranuleDesc()
            d.stream, d.channels = stream, info.channels
            for ch in range(info.channels):
                s, src, c = side.gr[gr][ch], data[gr][ch], g.ch[ch]
                c.global_gain, c.scalefac_scale, c.preflag = s.global_gain, s.scalefac_scale, src.preflag
                c.block_type, c.mixed_block_flag = s.block_type, s.mixed_block_flag
                C.memmove(c.subblock_gain, s.subblock_gain, 3)
                C.memmove(c.scalefac_l, src.scalefac_l, 22)
                C.memmove(c.scalefac_s, src.scalefac_s, 39)
                d.block_type[ch], d.mixed_block_flag[ch] = s.block_type, s.mixed_block_flag
                ints.append(np.array(src.is_, np.int16))
            granules.append(g)
            descs.append(d)
    n = len(granules)
    ga, da = (Mp3RequantGranule * max(n, 1))(*granules), (Mp3GranuleDesc * max(n, 1))(*descs)
    q = np.concatenate(ints) if ints else np.zeros(1, np.int16)
    pcm = np.zeros(max(q.size, 1), np.int16 if s16 else np.float32)
    status = np.zeros(max(n, 1), np.int32)
    fn = lib.sk_mp3_decode_granules_s16 if s16 else lib.sk_mp3_decode_granules_f32
    assert fn(engine._h, ga, da, _ptr(q), _ptr(pcm), n, _ptr(status)) == SK_OK
    # what the two later stages said of each decoded frame (a mixed block at a rate whose band table has no long / short seam at
    # line 36 is SK_MP3_UNSUPPORTED there): the first non-zero status of its granules
    stage, at = [], 0
    for (info, _side, _main), good in zip(frames, ok):
        mine = [int(v) for v in status[at:at + info.granules]] if good else []
        stage.append(next((v for v in mine if v), 0))
        at += len(mine)
    return pcm[:q.size if ints else 0], ok, stage


@pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])
def test_fused_chain_equals_host_huffman_plus_granule_decode(engine, iso_codebook, s16):
    dec = mp3.Mp3Decoder(engine=engine)  # installs the standard's band tables and synthesis window
    dec.close()
    mp3.set_codebook(None, engine)
    rng = np.random.default_rng(23)
    dropped = 0
    for k, (version, rate, mode) in enumerate([(1, 44100, MODES[2]), (1, 48000, MODES[0]), (1, 32000, MODES[4]), (2, 22050, MODES[4]), (2, 16000, MODES[1]),
                                               (25, 11025, MODES[5]), (25, 8000, MODES[0]), (2, 24000, MODES[3])]):
        data, _ = B.build_stream(ISO, 8000 + k, n_frames=14, **stream_params(version, rate, mode, bool(k & 1)))
        frames = [f[1:] for f in split(data)]
        assert len(frames) == 14
        hurt = damaged_frames(data, rng, 6)
        for at in (3, 4, 9):  # damaged frames among the good ones: the frames behind them must come out as without them
            frames[at] = hurt[int(rng.integers(0, len(hurt)))]
        a, b = engine.open_stream(rate, frames[0][0].channels), engine.open_stream(rate, frames[0][0].channels)
        try:
            want, ok, stage = host_chain(engine, iso_codebook, a, frames, s16)
            items, n, buf = mp3.pack_frames(frames)
            rc, got, es, ss = mp3.decode_frames(items, [b] * n, n, buf, engine, s16)
            assert rc == SK_OK and [int(v) for v in ss] == stage
            assert [int(e) == SK_OK for e in es] == ok
            for e, (info, side, main) in zip(es, frames):
                assert int(e) == mp3.decode_main_data(iso_codebook, info, side, main)[0]
            assert got.size == want.size and got.tobytes() == want.tobytes(), k
            assert np.abs(got.astype(np.float64)).max() > 0
            dropped += ok.count(False)
            # not enough room: nothing is synthesised, and the same call with room gives the same stream of samples going on
            rc, none, es2, _ = mp3.decode_frames(items, [b] * n, n, buf, engine, s16, out_cap=want.size - 1)
            assert rc == -7 and none.size == 0 and list(es2) == list(es)
        finally:
            engine.close_stream(a), engine.close_stream(b)
    assert dropped > 5


def test_fused_chain_argument_errors(engine):
    mp3.set_codebook(None, engine)
    data, _ = B.build_stream(ISO, 1, version=1, rate=44100, channels=2, mode=0, n_frames=2)
    frames = [f[1:] for f in split(data)]
    items, n, buf = mp3.pack_frames(frames)
    items[1].byte_offset += 2  # not a multiple of 4
    assert mp3.entropy_decode(items, n, buf, engine)[0] == -1
    items[1].byte_offset -= 2
    items[1].byte_len = buf.size  # no room behind it
    assert mp3.entropy_decode(items, n, buf, engine)[0] == -1
    assert mp3.decode_frames(items, [0, 0], n, buf, engine)[0] == -1


# ---- 6. the decoder handle -------------------------------------------------------------------------------------------------------

def run_decoder(engine, codebook, gpu, data, chunk, kind, room):
    """every call's (return code, written, samples, info) until the input is used up and an empty call returns nothing"""
    dtype = {"f32": np.float32, "i16": np.int16, "i32": np.int32}[kind]
    dec = mp3.Mp3Decoder(codebook, engine, gpu_entropy=gpu)
    trace, out = [], np.zeros(room, dtype)
    try:
        fn = getattr(dec, "decode_" + kind)
        at, idle = 0, 0
        while idle < 2 and len(trace) < 200000:
            piece = data[at:at + chunk]
            at += len(piece)
            try:
                n, rc = fn(piece, out), 0
            except SoundkitError as exc:
                n, rc = 0, exc.status
            trace.append((rc, n, out[:n].tobytes(), dec._info()))
            if rc != 0:
                break
            idle = idle + 1 if (not piece and n == 0) else 0
    finally:
        dec.close()
    return trace


def assert_same_trace(engine, codebook, data, chunk, kind, room=1 << 16):
    host = run_decoder(engine, codebook, False, data, chunk, kind, room)
    dev = run_decoder(engine, codebook, True, data, chunk, kind, room)
    assert len(host) == len(dev), (len(host), len(dev))
    for i, (h, d) in enumerate(zip(host, dev)):
        assert h[:2] == d[:2] and h[3] == d[3], (i, h[:2], d[:2], h[3], d[3])
        assert h[2] == d[2], i
    return host


@pytest.mark.parametrize("name", sorted(os.listdir(GOLD)))
@pytest.mark.parametrize("chunk", [1 << 20, 1, 417, 1200], ids=["whole", "1", "417", "1200"])
def test_decoder_handle_gpu_mode_equals_host_mode_on_the_fixtures(engine, name, chunk):
    with open(os.path.join(GOLD, name), "rb") as fh:
        data = fh.read()
    for kind in ("i16", "i32", "f32"):
        trace = assert_same_trace(engine, None, data, chunk, kind, room=1 << 20 if chunk > 5000 else 1 << 15)
        assert sum(t[1] for t in trace) > 40000 and trace[-1][3][3] > 80


def test_decoder_handle_gpu_mode_equals_host_mode_on_built_streams(engine):
    tables = B.make_tables(3)
    ct, _keep = B.to_ctypes(tables)
    cb = mp3.Codebook(ct)
    try:
        for k, kw in enumerate([dict(version=1, rate=44100, channels=2, mode=1, joint_modes=(0, 1, 2, 3)), dict(version=2, rate=16000, channels=1, bitrate_indices=(6, 9, 12)),
                                dict(version=25, rate=12000, channels=2, mode=1, joint_modes=(1, 2, 3), bitrate_indices=(6, 8), crc=True),
                                dict(version=1, rate=48000, channels=2, mode=0, free_format_bytes=640)]):
            data, _ = B.build_stream(tables, 600 + k, n_frames=14, **kw)
            rng = np.random.default_rng(k)
            hurt = bytearray(data)
            for _ in range(12):  # damage anywhere: headers, side information, main data
                hurt[int(rng.integers(len(data) // 4, len(data)))] ^= 1 << int(rng.integers(0, 8))
            for chunk in (1 << 20, 1, 417, 1200):
                for kind in ("i16", "i32", "f32"):
                    trace = assert_same_trace(engine, cb, data, chunk, kind)
                    assert sum(t[1] for t in trace) == 14 * 1152 * (2 if kw["channels"] == 2 else 1) * (1 if kw["version"] == 1 else 0.5)
                    assert_same_trace(engine, cb, bytes(hurt), chunk, kind)
        # the output-room rule: a buffer of one frame and a bit hands back one frame per call; one that cannot take a frame fails
        data, _ = B.build_stream(tables, 300, version=1, rate=44100, channels=2, mode=0, n_frames=9)
        trace = assert_same_trace(engine, cb, data, 1 << 20, "f32", room=2304 + 100)
        assert [t[1] for t in trace[:9]] == [2304] * 9
        trace = assert_same_trace(engine, cb, data, 1 << 20, "i16", room=1000)
        assert trace[-1][0] == -7 and trace[-1][3][2] == len(data)
        trace = assert_same_trace(engine, cb, data, 700, "i16", room=2 * 2304 + 5)
        assert sum(t[1] for t in trace) == 9 * 2304
        # a mono stream spliced to a stereo one, and back: the synthesis state belongs to a channel count
        mono, _ = B.build_stream(tables, 501, version=2, rate=22050, channels=1, n_frames=8, bitrate_indices=(8, 12))
        stereo, _ = B.build_stream(tables, 500, version=1, rate=44100, channels=2, mode=1, n_frames=8)
        for chunk in (1 << 20, 417):
            trace = assert_same_trace(engine, cb, mono + stereo + mono, chunk, "f32")
            assert sum(t[1] for t in trace) > 8 * 576 + 8 * 2304  # (what a seam costs is the framing's business: equal in both modes)
    finally:
        cb.close()


def test_two_gpu_mode_decoders_with_different_code_books_share_an_engine(engine):
    """each call installs its decoder's own code book first: interleaved calls of two handles give what each gives alone.  (Band
    tables and synthesis window are the engine's, one set per engine: the two code books differ in their codes only.)"""
    tables = dict(B.make_tables(11), bands=ISO["bands"], pretab=ISO["pretab"], window=ISO["window"])
    ct, _keep = B.to_ctypes(tables)
    cb = mp3.Codebook(ct)
    built, _ = B.build_stream(tables, 650, version=1, rate=32000, channels=2, mode=1, joint_modes=(0, 1, 2, 3), n_frames=12)
    with open(os.path.join(GOLD, "stereo16k_A_Tusk_encoded.mp3"), "rb") as fh:
        real = fh.read()[:576 * 30]
    try:
        alone = [[t[2] for t in run_decoder(engine, book, False, data, 700, "i16", 1 << 16)] for book, data in ((cb, built), (None, real))]
        a, b = mp3.Mp3Decoder(cb, engine, gpu_entropy=True), mp3.Mp3Decoder(None, engine, gpu_entropy=True)
        try:
            got, room = [[], []], np.zeros(1 << 16, np.int16)
            for at in range(0, max(len(built), len(real)) + 1400, 700):
                for k, (dec, data) in enumerate(((a, built), (b, real))):
                    n = dec.decode_i16(data[at:at + 700], room)
                    got[k].append(room[:n].tobytes())
        finally:
            a.close(), b.close()
        for k in range(2):
            assert b"".join(got[k]) == b"".join(alone[k]) and len(b"".join(got[k])) > 20000, k
    finally:
        mp3.set_codebook(None, engine)
        cb.close()


# ---- 7. the scheduler ------------------------------------------------------------------------------------------------------------

AAC_FILES = ["aac/aac-stereo-48k.adts", "aac/A_Tusk_is_used_to_make_costly_gifts_encoded.aac", "aac/mono16k_A_Tusk.aac", "aac/stereo-music-44100-192k.aac"]
MP3_FILES = ["mp3/stereo16k_A_Tusk_encoded.mp3", "mp3/mono16k_A_Tusk.mp3"]


def read_golden(name):
    with open(os.path.join(os.path.dirname(GOLD), name), "rb") as fh:
        return fh.read()


def through_scheduler(engine, datas, chunks, **config):
    """every stream's s16 samples (errors left out) and whether it met one"""
    import threading

    from soundkit_amd import pipeline
    from test_scheduler_gpu import drain, feed_all
    sched = pipeline.BatchScheduler(engine, **config)
    try:
        handles = [sched.spawn() for _ in datas]
        feeder = threading.Thread(target=feed_all, args=(handles, datas, chunks))
        feeder.start()
        outs = drain(handles, 120)
        feeder.join()
        for h in handles:
            h.cancel()
    finally:
        sched.close()
    pcm = [np.concatenate([np.frombuffer(a.data.tobytes(), "<i2") for a in got if not isinstance(a, Exception)] or [np.zeros(0, "<i2")]) for got in outs]
    return pcm, [[str(a) for a in got if isinstance(a, Exception)] for got in outs]


def damaged_fixture():
    bad = bytearray(read_golden(MP3_FILES[0]))
    for at in range(20000, 20000 + 576 * 3, 7):  # three frames' worth of side information and main data overwritten
        bad[at] = (at * 131) & 0xff
    for at in range(30000, 30400, 3):            # and Huffman data alone, further on
        bad[at + 40] ^= 0x5a
    return bytes(bad)


def test_scheduler_with_the_huffman_stage_in_the_tick_equals_the_single_decoders(engine):
    from test_scheduler_mp3_gpu import single_decoder
    names = [n for pair in zip(AAC_FILES * 2, MP3_FILES * 4) for n in pair]  # 16 streams, half of each codec
    datas = [read_golden(n) for n in names]
    want = {n: single_decoder(engine, n, read_golden(n)) for n in set(names)}
    rng = np.random.default_rng(3)
    chunks = [int(c) for c in rng.integers(200, 6000, len(names))]
    chunks[1], chunks[3] = 61, 100000
    got, errors = through_scheduler(engine, datas, chunks, entropy_threads=4, max_streams=32, max_frames_per_tick=96, max_stream_frames_per_tick=5,
                                    gpu_entropy=3)
    for name, mine, errs in zip(names, got, errors):
        assert not errs, (name, errs[:1])
        assert mine.size == want[name][2].size and np.array_equal(mine, want[name][2]), name


def test_a_damaged_mp3_stream_fares_as_with_the_host_stage(engine):
    datas = [read_golden(MP3_FILES[0]), damaged_fixture(), read_golden(AAC_FILES[0]), read_golden(MP3_FILES[1]), damaged_fixture()]
    chunks = [1500, 1500, 1500, 333, 97]
    config = dict(entropy_threads=3, max_streams=8, max_stream_frames_per_tick=4)
    host, host_errors = through_scheduler(engine, datas, chunks, gpu_entropy=1, **config)
    dev, dev_errors = through_scheduler(engine, datas, chunks, gpu_entropy=3, **config)
    assert host_errors == dev_errors
    for k in range(len(datas)):
        assert host[k].size == dev[k].size and np.array_equal(host[k], dev[k]), k
    assert 0 < host[1].size < host[0].size


CHILD = r"""
import hashlib, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import soundkit_amd
import soundkit_amd.engine as E
import test_mp3_entropy_gpu as T
eng = soundkit_amd.Engine(0, 64)
E._default = eng
datas = [T.read_golden(T.MP3_FILES[0]), T.damaged_fixture(), T.read_golden(T.AAC_FILES[0]), T.read_golden(T.MP3_FILES[1])]
pcm, errors = T.through_scheduler(eng, datas, [1500, 700, 1500, 333], entropy_threads=3, max_streams=8, max_stream_frames_per_tick=4, gpu_entropy=int(sys.argv[2]))
print("RESULT", " ".join(hashlib.sha256(p.tobytes()).hexdigest() for p in pcm), sum(len(e) for e in errors))
eng.close()
"""


def test_the_environment_switch_turns_mode_1_into_mode_3():
    """a child process each (the switch is read once): 1 without it, 1 with it, 3 -- the same bytes; with it the stage did run on the device"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = []
    for mode, switch in ((1, None), (1, "1"), (3, None)):
        env = dict(os.environ, SK_TICK_TRACE="1")
        env.pop("SK_PIPELINE_MP3_GPU_ENTROPY", None)
        if switch:
            env["SK_PIPELINE_MP3_GPU_ENTROPY"] = switch
        out = subprocess.run([sys.executable, "-c", CHILD, root, str(mode)], capture_output=True, text=True, env=env, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        lines.append(([l for l in out.stdout.splitlines() if l.startswith("RESULT")][0], "mp3 huffman stage in the tick" in out.stderr))
    assert lines[0][0] == lines[1][0] == lines[2][0]
    assert [seen for _, seen in lines] == [False, True, True]


def test_2048_mp3_streams_through_two_lanes_hash_as_with_the_host_stage(engine):
    from soundkit_amd import pipeline
    from soundkit_amd._lib import DecodeOptionsC
    from test_scale_gpu import Check, Result
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    clip = read_golden(MP3_FILES[0])
    found, used = mp3.scan(clip)
    clip = clip[:used]
    units = sum(f.granules for f in found)
    streams, loops = 2048, 6
    lg = C.CDLL(os.path.join(root, "soundkit_amd", "libsk_loadgen.so"))
    lg.sk_loadgen_run_checked.restype = C.c_int
    lg.sk_loadgen_run_checked.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    seen = {}
    for mode in (1, 3):
        hashes, outputs = np.zeros(streams, np.uint64), np.zeros(streams, np.uint32)
        nbytes, errors = np.zeros(streams, np.uint64), np.zeros(streams, np.uint32)
        capture = np.array([0], np.uint32)
        buf, lens = np.zeros((1, 1 << 22), np.uint8), np.zeros(1, np.uint64)
        chk = Check(hashes.ctypes.data, outputs.ctypes.data, nbytes.ctypes.data, errors.ctypes.data, capture.ctypes.data, 1, buf.ctypes.data,
                    buf.shape[1], lens.ctypes.data)
        sched = pipeline.BatchScheduler(engine, max_streams=streams, gpu_entropy=mode, lanes=2, max_stream_frames_per_tick=32)
        try:
            res = Result()
            opt = DecodeOptionsC(0, 16, 0, 0)
            rc = lg.sk_loadgen_run_checked(sched._h, clip, len(clip), units, streams, loops, C.byref(opt), 4, 0, C.byref(res), C.byref(chk))
            assert rc == 0
        finally:
            sched.close()
        assert res.errors == 0 and not errors.any()
        assert np.unique(outputs).size == 1 and np.unique(nbytes).size == 1 and nbytes[0] > 0
        assert (hashes == hashes[0]).all(), "%d streams delivered other bytes than stream 0" % int((hashes != hashes[0]).sum())
        seen[mode] = (int(hashes[0]), int(outputs[0]), int(nbytes[0]))
    assert seen[1] == seen[3]

"""The device Huffman stage's host side (no GPU): the new entry points are declared and exported, the new record has the
layout of its ctypes mirror, no existing record changed size, argument errors are reported before any device is touched, and
the flattened code book (sk_mp3_codebook_flatten, csrc/mp3_codebook_blob.h) decodes every code of the standard's tables and
of three random code sets to the symbol and length the tables give it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mp3_builder as B
import soundkit_amd
from oracle import mp3_iso
from soundkit_amd import _lib, mp3
from soundkit_amd._lib import lib

NEW = ["sk_mp3_codebook_flatten", "sk_mp3_set_codebook", "sk_mp3_entropy_decode", "sk_mp3_decode_frames_f32", "sk_mp3_decode_frames_s16",
       "sk_mp3_decoder_set_gpu_entropy", "sk_tick_run_mixed_md"]
HEADER_WORDS, L1_BITS, REGION_COUNTS = 608, 8, 40


def test_new_entry_points_are_declared_and_exported():
    declared = soundkit_amd.declared_symbols()
    for name in NEW:
        assert name in declared and hasattr(lib, name), name


def test_record_layouts(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "soundkit_amd.h"\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(sk_mp3_frame_item), offsetof(sk_mp3_frame_item, header), offsetof(sk_mp3_frame_item, side),\n'
                   '         offsetof(sk_mp3_frame_item, byte_offset), offsetof(sk_mp3_frame_item, byte_len));\n'
                   '  printf("%zu %zu %zu\\n", sizeof(sk_tick_input), sizeof(sk_pipeline_config), sizeof(sk_mp3_granule_data));\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.dirname(_lib.HEADER_PATH), "-o", exe, str(src)])
    lines = subprocess.check_output([exe], text=True).split("\n")
    item = _lib.Mp3FrameItem
    assert [int(v) for v in lines[0].split()] == [C.sizeof(item), item.header.offset, item.side.offset, item.byte_offset.offset, item.byte_len.offset]
    # what these were before the device stage was added: no existing record changed its layout
    assert [int(v) for v in lines[1].split()] == [88, 36, 1228]
    assert C.sizeof(_lib.Mp3GranuleData) == 1228


def test_argument_errors_need_no_device():
    cb = mp3.Codebook()
    try:
        n = C.c_size_t(0)
        assert lib.sk_mp3_set_codebook(None, cb._h) == -1 and lib.sk_mp3_set_codebook(None, None) == -1
        assert lib.sk_mp3_codebook_flatten(None, None, 0, C.byref(n)) == -1
        assert lib.sk_mp3_codebook_flatten(cb._h, None, 0, None) == -1
        assert lib.sk_mp3_codebook_flatten(cb._h, None, 0, C.byref(n)) == -7 and n.value > HEADER_WORDS
        small = np.zeros(16, np.uint32)
        assert lib.sk_mp3_codebook_flatten(cb._h, small.ctypes.data, small.size, C.byref(n)) == -7 and not small.any()
        item = _lib.Mp3FrameItem()
        out = ((_lib.Mp3GranuleData * 2) * 2)()
        buf = np.zeros(64, np.uint8)
        assert lib.sk_mp3_entropy_decode(None, C.byref(item), 1, buf.ctypes.data, buf.size, out) == -1
        w = C.c_size_t(0)
        st = np.zeros(1, np.int32)
        for fn in (lib.sk_mp3_decode_frames_f32, lib.sk_mp3_decode_frames_s16):
            assert fn(None, C.byref(item), st.ctypes.data, 1, buf.ctypes.data, buf.size, buf.ctypes.data, 16, st.ctypes.data, None, C.byref(w)) == -1
        assert lib.sk_mp3_decoder_set_gpu_entropy(None, 1) == -1
    finally:
        cb.close()


def walk(blob, first, bits):
    """decodes the code `bits` (a string of 0 / 1, long enough) starts with -> (entry, length), entry 0: no code"""
    e, width, used = int(blob[first + int(bits[:L1_BITS], 2)]), L1_BITS, 0
    while e & 0x80000000:
        used += width
        width = (e >> 26) & 31
        assert 1 <= width <= L1_BITS and used + width <= 32
        e = int(blob[(e & 0x03ffffff) + int(bits[used:used + width], 2)])
    return e, used + ((e >> 16) & 63)


@pytest.mark.parametrize("seed", [None, 3, 11, 29], ids=["iso", "random3", "random11", "random29"])
def test_flattened_code_book_decodes_every_code(seed):
    tables = mp3_iso.tables() if seed is None else B.make_tables(seed)
    ct, _keep = B.to_ctypes(tables)
    cb = mp3.Codebook(ct)
    try:
        blob = mp3.codebook_flatten(cb)
    finally:
        cb.close()
    assert blob[0] == blob.size and HEADER_WORDS <= blob[1] <= blob.size and (blob[1] - HEADER_WORDS) % (1 << L1_BITS) == 0
    rng = np.random.default_rng(seed or 0)
    big, count1 = blob[2:34], blob[34:36]
    checked = 0
    for t, table in enumerate(tables["big_values"]):
        if not table:
            assert big[t] == 0
            continue
        xlen, linbits, first = int(big[t]) & 0xff, (int(big[t]) >> 8) & 0xff, int(big[t]) >> 16
        assert (xlen, linbits) == (table["xlen"], table["linbits"]) and HEADER_WORDS <= first < blob[1]
        for symbol, (n, code) in enumerate(zip(table["hlen"], table["hcod"])):
            tail = "".join(str(int(b)) for b in rng.integers(0, 2, 40))
            e, length = walk(blob, first, format(code, "0%db" % n) + tail)
            assert e & 0x8000 and length == n and ((e >> 4) & 15) * xlen + (e & 15) == symbol, (t, symbol)
            checked += 1
    for k in range(2):
        for symbol in range(16):
            n, code = tables["count1"][k]["hlen"][symbol], tables["count1"][k]["hcod"][symbol]
            e, length = walk(blob, int(count1[k]), format(code, "0%db" % n) + "".join(str(int(b)) for b in rng.integers(0, 2, 40)))
            assert e & 0x8000 and length == n and (e & 15) == symbol
    assert checked > 1300
    if seed is None:
        # the standard's tables 16-23 share one code set, 24-31 another: 15 + 2 distinct first-level tables, 19.4 KiB of LDS
        assert blob[1] == HEADER_WORDS + 17 * (1 << L1_BITS) and blob.size * 4 < 32 * 1024
        assert len({int(big[t]) >> 16 for t in range(16, 24)}) == 1 and len({int(big[t]) >> 16 for t in range(24, 32)}) == 1
    # the rest of the header: slen, lsf_partitions, rates, and the region boundaries of every cut
    raw = blob[:HEADER_WORDS].tobytes()
    at = 4 * 36
    assert list(raw[at:at + 32]) == [v for row in tables["slen"] for v in row]
    assert list(raw[at + 32:at + 104]) == [v for row in tables["lsf_partitions"] for col in row for v in col]
    present = list(raw[at + 104:at + 113])
    region = np.frombuffer(raw[at + 116:at + 116 + 9 * 3 * REGION_COUNTS * 2], np.uint16).reshape(9, 3, REGION_COUNTS)
    for row, rate in enumerate(B.RATES):
        assert present[row] == (rate in tables["bands"])
        if not present[row]:
            continue
        lo, so = tables["bands"][rate]
        short = [so[b + 1] - so[b] for b in range(13) for _ in range(3)]
        first_short = next(b for b in range(14) if 3 * so[b] >= 36)
        cuts = [[lo[b + 1] - lo[b] for b in range(22)], short,
                [lo[b + 1] - lo[b] for b in range(22) if lo[b + 1] <= 36] + short[3 * first_short:]]
        for cut in range(3):
            for count in range(REGION_COUNTS):
                assert region[row][cut][count] == min(576, sum(cuts[cut][:count])), (rate, cut, count)


"""The library's kernel flavour is what it says it is.  The default build must not contain a single packed-f32 vector instruction
(v_pk_mul/add/fma_f32): on MI355X they deliver a wrong low half now and then while another wave of the CU executes a 16x16x32 matrix
instruction (profiles/r04_lanes_corruption.md), and the immunity of the default build rests on their absence from EVERY kernel --
a builtin or a line of inline assembly that brings one back would not fail any parity test.

Nobody has shown which other packed (v_pk_*) opcodes are safe beside matrix instructions, so the default build's set is an
allow-list: every v_pk_* mnemonic in every code object, equal to PACKED_ALLOWED below.  A new one fails here until it is added
on purpose, with the kernels that use it."""
import os
import re
import shutil
import subprocess

import pytest

from soundkit_amd import _lib

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

# every packed opcode of the default build -> the kernels that use it (16-bit integer arithmetic, no packed f32)
PACKED_ALLOWED = {
    "v_pk_add_u16": "k_frames_to_s16 (aac_synth.hip), k_convert<FLOAT_TO_I16_ROUND, false> (pcm.hip): the s16 narrowing",
    "v_pk_sub_i16": "k_frames_to_s16 (aac_synth.hip), k_convert<FLOAT_TO_I16_ROUND, false> (pcm.hip): the s16 narrowing",
}


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump of the ROCm toolchain not found")
def test_default_build_has_no_packed_f32_instructions(tmp_path):
    so = str(tmp_path / "libsoundkit_amd.so")
    shutil.copy(_lib.LIB_PATH, so)
    subprocess.check_call([OBJDUMP, "--offloading", so], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)  # writes the bundles beside its input
    objects = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert len(objects) >= 7, objects  # one code object per .hip file
    packed, total = 0, 0
    used = {}  # packed mnemonic -> kernels
    for f in objects:
        text = subprocess.run([OBJDUMP, "-d", str(tmp_path / f)], capture_output=True, text=True, check=True).stdout
        total += len(re.findall(r"^\s+v_", text, re.M))
        packed += len(re.findall(r"\bv_pk_(?:mul|add|fma)_f32\b", text))
        kernel = None
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
            if m:
                kernel = m.group(1)
            for op in re.findall(r"\bv_pk_[a-z0-9_]+", line):
                used.setdefault(op, set()).add(kernel)
    assert total > 50000, total  # the disassembly is really there
    if _lib.lib.sk_kernels_use_packed_f32() == 0:
        assert packed == 0, packed
        assert set(used) == set(PACKED_ALLOWED), {op: sorted(k)[:3] for op, k in used.items() if op not in PACKED_ALLOWED}
    else:
        assert packed > 0  # make PACKED_F32=1: the flavour that needs its GPU to itself

"""A guard on the interior loop of the 48 -> 16 kHz FIR on s16 rows (profiles/fir_interior.md).

The launch of the flagship line is k_fir_48k_16k_bf16<true, true, 2, true, true, true>: frame-packed s16 rows, f16 planes, interleaved
stereo s16 out, and -- the sixth argument -- 32-bit addressing through buffer descriptors, which the host takes whenever a group's
offsets fit.  Its interior body (four periods, eight tiles, 192 matrix instructions) used to hold eight exec-mask branches around
stores that only the even lanes made, 56 64-bit vector adds for load addresses and 13 spilled registers outside the loop.  Should a
later change, or a compiler, bring any of that back, nothing fails -- the launch just gets slower.  So the device assembly is built
with the Makefile's own flags, as test_synth_valu_count_asm.py builds it, and read:

  the innermost loop holding at least 190 matrix instructions
      has no conditional branch other than its back-edge and its exits,
      touches no scratch memory,
      holds at most 650 `v_` lines that are not matrix instructions (726 by this count before; 607 with the stores and the
      addressing changed, 463 with the split's remainder as one mixed-precision multiply-add per sample);
  metadata: vgpr_count <= 168 (three waves per SIMD), no more than the 13 spilled registers it had, 12 800 bytes of LDS.

The test counts lines and reads metadata; it looks for no particular instruction.
"""
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "soundkit_amd", "csrc")
TAG = "18k_fir_48k_16k_bf16ILb1ELb1ELi2ELb1ELb1ELb1EEE"
MATRIX = "v_mfma"        # the prefix every matrix instruction's mnemonic starts with
MIN_MATRIX = 190
MAX_VECTOR = 650
MAX_VGPRS = 168
PARENT_SPILLS = 13
LDS_BYTES = 12800


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    # the compile line make itself would run for fir_bf16.hip, turned into a device-only assembly build
    try:
        dry = subprocess.run(["make", "-C", CSRC, "-n", "-B", "build/fir_bf16.o"], capture_output=True, text=True, check=True).stdout
    except (OSError, subprocess.CalledProcessError) as e:
        pytest.skip("make is not usable here: %s" % e)
    line = next(l for l in dry.splitlines() if "fir_bf16.hip" in l and " -c " in l)
    argv = shlex.split(line)
    if not os.path.exists(argv[0]):
        pytest.skip("no hipcc at %s" % argv[0])
    out = str(tmp_path_factory.mktemp("asm") / "fir_bf16.s")
    cut = argv.index("-c")
    argv = argv[:cut] + ["--cuda-device-only", "-S", os.path.join(CSRC, "fir_bf16.hip"), "-o", out]
    subprocess.run(argv, cwd=CSRC, check=True, capture_output=True)
    return open(out).read()


def kernel_lines(asm, tag):
    m = re.search(r"^(_ZN\S*%s\S*):.*?\n(.*?)\n\.Lfunc_end" % tag, asm, re.S | re.M)
    assert m, tag
    return [l.strip() for l in m.group(2).split("\n")]


def interior_loop(lines):
    """(header, back-edge) line numbers of the innermost (shortest) loop that holds at least MIN_MATRIX matrix instructions"""
    label_at = {l.split(":")[0]: i for i, l in enumerate(lines) if re.match(r"\.LBB\d+_\d+:", l)}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", l)
        if m and label_at.get(m.group(1), i) < i:
            head = label_at[m.group(1)]
            if sum(x.startswith(MATRIX) for x in lines[head:i]) >= MIN_MATRIX:
                loops.append((i - head, head, i))
    assert loops, "no loop with %d matrix instructions" % MIN_MATRIX
    return min(loops)[1:], label_at


def kernel_metadata(asm, tag):
    """the scalar fields of the kernel's entry in amdhsa.kernels (entries start at `- .agpr_count`)"""
    entries = [e for e in re.split(r"\n  - (?=\.agpr_count)", asm) if re.search(r"\.name:\s+_ZN\S*%s" % tag, e)]
    assert len(entries) == 1, tag
    return dict(re.findall(r"^    \.(\w+):\s+(\S+)", entries[0], re.M))


def test_interior_loop_is_branch_free_without_scratch_and_lean(assembly):
    lines = kernel_lines(assembly, TAG)
    (head, back), label_at = interior_loop(lines)
    body = lines[head:back + 1]
    matrix = sum(l.startswith(MATRIX) for l in body)
    vector = sum(l.startswith("v_") and not l.startswith(MATRIX) for l in body)
    inner = []   # conditional branches that stay inside the loop without being its back-edge
    for i, l in enumerate(body):
        m = re.match(r"s_cbranch\S*\s+(\.LBB\d+_\d+)", l)
        if m and head < label_at.get(m.group(1), -1) <= back:
            inner.append(l)
    scratch = [l for l in body if l.startswith("scratch_") or "Spill" in l or "Reload" in l]
    print("interior loop: %d lines, %d matrix instructions, %d other v_ lines (limit %d), %d inner branches, %d scratch accesses"
          % (len(body), matrix, vector, MAX_VECTOR, len(inner), len(scratch)))
    assert not inner, inner
    assert not scratch, scratch[:4]
    assert vector <= MAX_VECTOR, vector


def test_registers_spills_and_lds(assembly):
    meta = kernel_metadata(assembly, TAG)
    print("vgpr_count %s, vgpr_spill_count %s, sgpr_spill_count %s, private segment %s B, LDS %s B"
          % (meta["vgpr_count"], meta["vgpr_spill_count"], meta["sgpr_spill_count"], meta["private_segment_fixed_size"],
             meta["group_segment_fixed_size"]))
    assert int(meta["vgpr_count"]) <= MAX_VGPRS, meta
    assert int(meta["vgpr_spill_count"]) + int(meta["sgpr_spill_count"]) <= PARENT_SPILLS, meta
    assert int(meta["group_segment_fixed_size"]) == LDS_BYTES, meta

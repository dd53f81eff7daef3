"""A guard on the vector-instruction count of the synthesis kernels (profiles/synth_valu_diet.md).

Built without the packed-f32 instructions, the long-only pair kernel is bound by vector issue: the counters put its vector
pipe at 79 % busy and 989 vector instructions per pair-frame, and the listing of its frame loop held 992 lines starting
with `v_`.  Four source-level changes (one stage-1 twiddle instead of two, pre-twiddle and window + overlap-add as fused
multiply-adds, `h` folded into dft8's last butterfly) take 152 of them out.  Should a later change, or a compiler, bring them
back, nothing fails -- the launch just gets slower.  So the device assembly is built with the Makefile's own flags, as
test_synth_store_order_asm.py builds it, and counted:

  k_aac_synth_pair<true, false>    frame loop: 992 `v_` lines at the parent commit, 840 the target, at most 850 allowed
  k_aac_synth_pair<false, false>   frame loop: 782 `v_` lines at the parent commit, at most 782 - 140 = 642 allowed

and every k_aac_synth* kernel and k_aac_tail reports no spill, no private segment and a vgpr_count inside the occupancy its
__launch_bounds__ asks for: 256 for the pair kernels and for k_aac_tail (two waves per SIMD; the tail holds 68 registers of FIR
taps and stood at 211), 128 for k_aac_synth<., true> (four waves), 168 for k_aac_synth<., false> (three); the pair kernels' LDS
leaves room for two workgroups per CU.  The test counts lines and reads metadata; it looks for no particular instruction.
"""
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "soundkit_amd", "csrc")
PARENT_F32_LOOP = 782  # `v_` lines in the frame loop of k_aac_synth_pair<false, false> at the parent commit
LOOP_LIMIT = {"16k_aac_synth_pairILb1ELb0EEE": 850, "16k_aac_synth_pairILb0ELb0EEE": PARENT_F32_LOOP - 140}
# vgpr_count each kernel may report: 512 registers per SIMD lane over the waves its __launch_bounds__ asks for
VGPR_LIMIT = {
    "16k_aac_synth_pairILb1ELb0EEE": 256, "16k_aac_synth_pairILb0ELb0EEE": 256,
    "16k_aac_synth_pairILb1ELb1EEE": 256, "16k_aac_synth_pairILb0ELb1EEE": 256,
    "11k_aac_synthILb1ELb1EEE": 128, "11k_aac_synthILb0ELb1EEE": 128,
    "11k_aac_synthILb1ELb0EEE": 168, "11k_aac_synthILb0ELb0EEE": 168,
    "10k_aac_tailE": 256,
}


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    # the compile line make itself would run for aac_synth.hip, turned into a device-only assembly build
    try:
        dry = subprocess.run(["make", "-C", CSRC, "-n", "-B", "build/aac_synth.o"], capture_output=True, text=True, check=True).stdout
    except (OSError, subprocess.CalledProcessError) as e:
        pytest.skip("make is not usable here: %s" % e)
    line = next(l for l in dry.splitlines() if "aac_synth.hip" in l and " -c " in l)
    argv = shlex.split(line)
    if not os.path.exists(argv[0]):
        pytest.skip("no hipcc at %s" % argv[0])
    out = str(tmp_path_factory.mktemp("asm") / "aac_synth.s")
    cut = argv.index("-c")
    argv = argv[:cut] + ["--cuda-device-only", "-S", os.path.join(CSRC, "aac_synth.hip"), "-o", out]
    subprocess.run(argv, cwd=CSRC, check=True, capture_output=True)
    return open(out).read()


def kernel_body(asm, tag):
    m = re.search(r"^(_ZN\S*%s\S*):.*?\n(.*?)\n\.Lfunc_end" % tag, asm, re.S | re.M)
    assert m, tag
    return m.group(1), [l.strip() for l in m.group(2).split("\n")]


def frame_loop(lines):
    """(header, back-edge) line numbers of the innermost loop that requests a pair-frame's sixteen spectrum rows"""
    label_at = {l[:-1].split(":")[0]: i for i, l in enumerate(lines) if re.match(r"\.LBB\d+_\d+:", l)}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", l)
        if m and label_at.get(m.group(1), i) < i:
            head = label_at[m.group(1)]
            if sum(x.startswith("global_load_dwordx2") for x in lines[head:i]) >= 16:
                loops.append((i - head, head, i))
    assert loops, "no frame loop found"
    return min(loops)[1:]


def vector_lines(asm, tag):
    _, lines = kernel_body(asm, tag)
    head, back = frame_loop(lines)
    return sum(l.startswith("v_") for l in lines[head:back])


def kernel_metadata(asm, tag):
    """the scalar fields of the kernel's entry in amdhsa.kernels (entries start at `- .agpr_count`)"""
    entries = [e for e in re.split(r"\n  - (?=\.agpr_count)", asm) if re.search(r"\.name:\s+_ZN\S*%s" % tag, e)]
    assert len(entries) == 1, tag
    return dict(re.findall(r"^    \.(\w+):\s+(\S+)", entries[0], re.M))


@pytest.mark.parametrize("tag", sorted(LOOP_LIMIT))
def test_frame_loop_vector_instructions(assembly, tag):
    n = vector_lines(assembly, tag)
    print("%s: %d v_ lines in the frame loop (limit %d)" % (tag, n, LOOP_LIMIT[tag]))
    assert n <= LOOP_LIMIT[tag], n


@pytest.mark.parametrize("tag", sorted(VGPR_LIMIT))
def test_no_spill_no_scratch_and_registers_in_class(assembly, tag):
    meta = kernel_metadata(assembly, tag)
    print("%s: %s VGPRs, %s B LDS" % (tag, meta["vgpr_count"], meta["group_segment_fixed_size"]))
    assert meta["vgpr_spill_count"] == "0" and meta["sgpr_spill_count"] == "0" and meta["private_segment_fixed_size"] == "0", meta
    assert int(meta["vgpr_count"]) <= VGPR_LIMIT[tag], meta
    if "synth_pair" in tag:  # two workgroups of a pair kernel on a CU: 160 KiB of LDS between them
        assert int(meta["group_segment_fixed_size"]) <= 81920, meta

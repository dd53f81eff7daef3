"""A guard on the generated code of the long-only pair synthesis kernels (profiles/synth_store_drain.md).

Loads and stores share one in-order counter on gfx950, and the frame loop's head waits for the spectra requested a frame
earlier.  That wait is a wait for loads alone only while no PCM store is issued between the spectrum requests and the
back-edge: the kernels hold a frame's PCM and store it in front of the next prefetch.  Should a compiler move the stores
back behind the loads, every frame drains the wave's store queue again -- nothing fails, the launch just gets slower.
So the device assembly is built with the Makefile's own flags and read: in the frame loop of k_aac_synth_pair<true, false>
and <false, false> no global_store lies between the last spectrum load and the back-edge, and nothing spills.
"""
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "soundkit_amd", "csrc")
KERNELS = {"s16": "16k_aac_synth_pairILb1ELb0EEE", "f32": "16k_aac_synth_pairILb0ELb0EEE"}


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


@pytest.mark.parametrize("out", sorted(KERNELS))
def test_no_pcm_store_between_the_spectrum_loads_and_the_back_edge(assembly, out):
    name, lines = kernel_body(assembly, KERNELS[out])
    head, back = frame_loop(lines)
    body = lines[head:back]
    loads = [i for i, l in enumerate(body) if l.startswith("global_load")]
    stores = [i for i, l in enumerate(body) if l.startswith("global_store")]
    assert len(stores) == 8, "the held frame's eight stores belong in the loop: %d" % len(stores)
    late = [body[i] for i in stores if i > loads[-1]]
    assert not late, "stores younger than the spectrum requests at the loop head:\n" + "\n".join(late)


@pytest.mark.parametrize("out", sorted(KERNELS))
def test_nothing_spills(assembly, out):
    m = re.search(r"\.name:\s+_ZN\S*%s\S*\n(.*?)\.wavefront_size" % KERNELS[out], assembly, re.S)
    assert m
    meta = dict(re.findall(r"\.(\w+):\s+(\S+)", m.group(1)))
    assert meta["vgpr_spill_count"] == "0" and meta["sgpr_spill_count"] == "0" and meta["private_segment_fixed_size"] == "0", meta
    assert int(meta["vgpr_count"]) <= 256  # two waves per SIMD, as __launch_bounds__ asks

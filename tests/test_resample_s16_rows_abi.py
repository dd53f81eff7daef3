"""The any-rate s16 frame-row resampler's two entry points are exported by the built library and bound in _lib.py with the
header's argument count (no GPU)."""
import re
import subprocess

import pytest

import soundkit_amd
from soundkit_amd import _lib

NAMES = ["sk_downsample_frames_s16_to_s16_dev", "sk_downsample_frames_s16_to_f32_dev"]


def header_arg_count(name):
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % re.escape(name), text, flags=re.S)
    assert m, "%s is not declared in include/soundkit_amd.h" % name
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_is_exported_and_bound(name):
    assert name in soundkit_amd.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", soundkit_amd.LIB_PATH], text=True)
    assert any(line.split()[-1] == name for line in out.splitlines() if " T " in line)
    fn = getattr(_lib.lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == header_arg_count(name) == 12
    # the 48 kHz pair's shape with the two rates added
    twin = getattr(_lib.lib, name.replace("sk_downsample_", "sk_downsample_48k_16k_"))
    assert len(twin.argtypes) == 10 and list(fn.argtypes[:7]) == list(twin.argtypes[:7]) and list(fn.argtypes[9:]) == list(twin.argtypes[7:])
    assert hasattr(soundkit_amd.Engine, name[len("sk_"):])

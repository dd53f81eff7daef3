"""AAC-LC at all 13 sampling-frequency indices, on the CPU: the band tables themselves, the way from index to rate to tables, the host
front end (csrc/aac_frontend.cpp) and the CPU build of the device core (csrc/aac_entropy_core.h) against the oracle on the units of
tests/aac_index_cases.py.  The other front-end tests run indices 0, 3, 4, 6, 8 and 11; the oracle reads the product's own
aac_tables.h, so a wrong offset would move both -- the table gates and the transcription check below are what holds the tables.
The same units on the GPU: tests/test_aac_sf_index_gpu.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import aac_index_cases as A
from au_builder import EIGHT_SHORT, ONLY_LONG, Writer, asc_for, directed_access_unit
from oracle import aac_frontend as OF
from soundkit_amd import aac_lc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# sfb.rs:52-71 as long_layout / short_layout (csrc/aac_frontend.cpp) declare it
LONG_BANDS = [41, 41, 47, 49, 49, 51, 47, 47, 43, 43, 43, 40, 40]
SHORT_BANDS = [12, 12, 12, 14, 14, 14, 15, 15, 15, 15, 15, 15, 15]


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- the tables ---------------------------------------------------------------------------------------------------------------------

def test_band_tables_are_well_formed():
    assert sorted(OF._SWB) == sorted("kSwb%s_%s" % (n, r) for n, rates in (("1024", (96, 64, 48, 32, 24, 16, 8)), ("128", (96, 48, 24, 16, 8)))
                                     for r in rates)
    for name, off in OF._SWB.items():
        end = 1024 if name.startswith("kSwb1024") else 128
        widths = np.diff(off)
        assert off[0] == 0 and off[-1] == end, name
        assert (widths > 0).all() and not (widths % 4).any(), (name, widths)


@pytest.mark.parametrize("sf_index", A.INDICES)
def test_band_counts_and_tns_limits(sf_index):
    assert A.band_counts(sf_index) == (LONG_BANDS[sf_index], SHORT_BANDS[sf_index])
    assert OF.tns_max_bands(sf_index, False) <= LONG_BANDS[sf_index]
    assert OF.tns_max_bands(sf_index, True) <= SHORT_BANDS[sf_index]
    assert len(OF._TNS_MAX[0]) == len(OF._TNS_MAX[1]) == 13


def test_tables_equal_a_fresh_transcription(tmp_path):
    """tools/transcribe_iso_tables.py run again on the reference tree writes aac_tables.h byte for byte"""
    tool = os.path.join(ROOT, "tools", "transcribe_iso_tables.py")
    src = os.environ.get("SOUNDKIT_REFERENCE_AAC_SRC") or re.search(r'else "([^"]+)"', open(tool).read()).group(1)
    if not all(os.access(os.path.join(src, f), os.R_OK) for f in ("spectral.rs", "scalefactor.rs", "sfb.rs", "tns.rs")):
        pytest.skip("the reference tree is not on this machine")
    os.makedirs(tmp_path / "soundkit_amd" / "csrc")
    subprocess.check_call([sys.executable, tool, src], cwd=tmp_path, stdout=subprocess.DEVNULL)
    fresh = open(tmp_path / "soundkit_amd" / "csrc" / "aac_tables.h", "rb").read()
    assert fresh == open(os.path.join(ROOT, "soundkit_amd", "csrc", "aac_tables.h"), "rb").read()


# ---- index -> rate -> tables ----------------------------------------------------------------------------------------------------------

def refusals(asc, unit):
    """the unit through a fresh host front end and a fresh oracle decoder -> (AacLcError, AacError)"""
    with pytest.raises(aac_lc.AacLcError) as host:
        aac_lc.AacLcFrontEnd(asc).parse(unit)
    with pytest.raises(OF.AacError) as want:
        OF.Decoder(asc).decode_access_unit(unit)
    return host.value, want.value


@pytest.mark.parametrize("sf_index", A.INDICES)
def test_index_to_rate_to_tables(sf_index):
    """the directed unit with max_sfb = the table's band count is accepted (bit for bit the oracle's), one band more is refused as the
    oracle refuses it: the product's layouts hold exactly LONG_BANDS / SHORT_BANDS bands at this index"""
    for channels, s in A.cases(sf_index).items():
        fe = aac_lc.AacLcFrontEnd(s.asc)
        assert (fe.sample_rate, fe.channels) == (OF.RATES[sf_index], channels)
        for name in ("only_long", "short_8_groups"):
            k = s.label.index(name)     # the stream's first unit, or the first short one on a generator that has run: use a fresh pair
            got, gseq, gshape = aac_lc.AacLcFrontEnd(s.asc).parse(s.units[k])
            want, seq, shape = OF.Decoder(s.asc).decode_access_unit(s.units[k])
            assert (gseq, gshape) == (seq, shape) and same_bits(got, want), (sf_index, channels, name)
        assert [o[0] for o in s.over] == (["only_long", "short_8_groups"] if SHORT_BANDS[sf_index] < 15 else ["only_long"])
        for name, first, first_want, over, err in s.over:
            fe = aac_lc.AacLcFrontEnd(s.asc)
            got, gseq, gshape = fe.parse(first)
            assert (gseq, gshape) == (first_want[1], first_want[2]) and same_bits(got, first_want[0])
            with pytest.raises(aac_lc.AacLcError) as exc:
                fe.parse(over)
            assert (err.kind, str(err)) == ("InvalidConfig", "missing scale-factor band offset")
            assert exc.value.kind == err.kind and str(exc.value) == "%s: %s" % (err.kind, err), (sf_index, channels, name, str(exc.value))


@pytest.mark.parametrize("sf_index", [13, 14])
@pytest.mark.parametrize("channels", [1, 2])
def test_reserved_indices_refuse_at_construction(sf_index, channels):
    with pytest.raises(OF.AacError) as want:
        OF.Decoder(asc_for(sf_index, channels))
    with pytest.raises(aac_lc.AacLcError) as host:
        aac_lc.AacLcFrontEnd(asc_for(sf_index, channels))
    assert want.value.kind == "UnsupportedSamplingFrequencyIndex" and host.value.kind == want.value.kind


@pytest.mark.parametrize("channels", [1, 2])
def test_an_explicit_rate_refuses_every_unit(channels):
    """index 15 and 24 bits of rate: the config is taken, but no band table belongs to it"""
    w = Writer()
    w.put(2, 5), w.put(15, 4), w.put(48000, 24), w.put(channels, 4), w.put(0, 3)
    asc = w.bytes()
    fe, dec = aac_lc.AacLcFrontEnd(asc), OF.Decoder(asc)
    assert (fe.sample_rate, fe.channels) == (dec.sample_rate, dec.channels) == (48000, channels)
    rng = np.random.default_rng(15)
    for seq in (ONLY_LONG, EIGHT_SHORT):
        unit = directed_access_unit(rng, 3, channels, seq)
        host, want = refusals(asc, unit)
        assert want.kind == "UnsupportedFeature" and host.kind == want.kind and str(want) in str(host), (str(host), str(want))


# ---- the shared units -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sf_index", A.INDICES)
def test_the_units_reach_what_they_are_for(sf_index):
    r = A.reach(sf_index)
    assert all(n >= 1 for n in r["top"].values()), r          # per window shape: a channel whose top band is non-zero
    assert r["tns_long"] >= 1 and r["tns_short"] >= 1, r      # a TNS filter stopped by the index's tns_max_bands
    assert r["noise"] >= 1, r                                 # a unit that draws PNS noise
    for s in A.cases(sf_index).values():
        assert len(s.units) == len(s.want) == A.ACCEPTED == 44
        assert max(len(u) for u in s.units) + 7 < 8192       # the ADTS length field, and the device's bound on a unit


@pytest.mark.parametrize("sf_index", A.INDICES)
def test_host_front_end_equals_oracle(sf_index):
    """one front end per (index, channels): the PNS generator is carried through all 44 units, as the oracle's was"""
    for channels, s in A.cases(sf_index).items():
        fe = aac_lc.AacLcFrontEnd(s.asc)
        compared = 0
        for k, (au, (want, seq, shape)) in enumerate(zip(s.units, s.want)):
            got, gseq, gshape = fe.parse(au)
            assert (gseq, gshape) == (seq, shape), (sf_index, channels, k, s.label[k])
            assert same_bits(got, want), (sf_index, channels, k, s.label[k])
            compared += 1
        assert compared == A.ACCEPTED


# ---- the device core, built for the CPU -----------------------------------------------------------------------------------------------

FORMS = [pytest.param([], id="nested"), pytest.param(["-DSK_EC_FLAT"], id="flat")]
MUTANTS = 100


@pytest.mark.parametrize("form", FORMS)
def test_entropy_core_equals_host_front_end_at_every_index(tmp_path, form):
    """tests/entropy_core_check.cpp as tests/test_entropy_core.py builds it (stand-alone, AddressSanitizer + UBSan), on one ADTS file
    per (index, channels): the 44 units, the units with max_sfb past the table behind them, and 100 mutants of each file"""
    exe = str(tmp_path / "entropy_core_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-ffp-contract=off", "-Wno-subobject-linkage"] + form + ["-o", exe, os.path.join(HERE, "entropy_core_check.cpp")],
                          cwd=HERE)
    files, units = [], 0
    for sf_index in A.INDICES:
        for channels, s in A.cases(sf_index).items():
            path = str(tmp_path / ("sf%d_ch%d.adts" % (sf_index, channels)))
            open(path, "wb").write(s.adts(over=True))
            files.append(path)
            units += len(s.units) + len(s.over) + MUTANTS
    assert len(files) == 26 and units == 26 * (44 + MUTANTS) + 2 * (6 * 2 + 7 * 1)
    out = subprocess.run([exe, str(MUTANTS)] + files, capture_output=True, text=True)
    assert out.returncode == 0 and "identical" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    assert "checked %d access units" % units in out.stdout
    accepted = int(re.search(r"(\d+) accepted", out.stdout).group(1))
    assert accepted >= 26 * 44, out.stdout[-200:]             # every unit of the accepted sets was accepted here too

"""The access units the sampling-frequency-index tests share (test_aac_sf_index_cpu.py, test_aac_sf_index_gpu.py), built and decoded
by the oracle once per process: for each of the 13 indices and each of mono / stereo one stream of

  24 directed units (au_builder.directed_access_unit: every band of the index's table coded, the top one non-zero, TNS longer than
     the table, a mid/side mask on the top band), four for each of the six window shapes of SHAPES, then
  20 units of au_builder.random_access_unit,

decoded in this order by one oracle decoder, so the PNS generator is carried from unit to unit; and beside it the units with max_sfb
one past the table (over = 1), each the last unit of a two-unit stream of its own, with the oracle's error.  The seeds are chosen so
that the oracle accepts all 44 units of every stream: build() asserts it, and that it refuses every over unit.

reach(sf_index) counts, on the oracle's parse, what the units are there for; test_aac_sf_index_cpu.py asserts the counts."""
import functools

import numpy as np

from au_builder import EIGHT_SHORT, LONG_START, LONG_STOP, ONLY_LONG, adts_frame, asc_for, directed_access_unit, random_access_unit
from oracle import aac_frontend as OF

INDICES = list(range(13))
SHAPES = [("only_long", ONLY_LONG, 0), ("long_start", LONG_START, 0), ("long_stop", LONG_STOP, 0),
          ("short_8_groups", EIGHT_SHORT, 0), ("short_1_group", EIGHT_SHORT, 127), ("short_4_groups", EIGHT_SHORT, 0b1010101)]
DIRECTED_PER_SHAPE, RANDOM_UNITS = 4, 20
ACCEPTED = len(SHAPES) * DIRECTED_PER_SHAPE + RANDOM_UNITS   # units per (index, channels) stream
SEED = 20260


def band_counts(sf_index):
    return len(OF.long_offsets(sf_index)) - 1, len(OF.short_offsets(sf_index)) - 1


class _Spy(OF.Decoder):
    """the oracle decoder, noting per unit what its parse met: the TNS data it applied and whether the unit drew noise"""

    def __init__(self, asc):
        super().__init__(asc)
        self.tns_seen = []

    def tns(self, ch, coef):
        self.tns_seen.append((ch.ics.sequence, ch.ics.max_sfb, ch.tns))
        super().tns(ch, coef)


class Stream:
    """units: the 44 access units; want: the oracle's (spectra, sequence, shape) of each; label: the window shape's name or 'random';
    tns: per unit the (sequence, max_sfb, tns data) of its channels that carry TNS; noise: per unit, whether it moved the PNS generator;
    over: [(label, accepted first unit, its oracle result, over unit, the oracle's AacError)]"""

    def __init__(self, sf_index, channels):
        self.sf_index, self.channels, self.asc = sf_index, channels, asc_for(sf_index, channels)
        self.units, self.want, self.label, self.tns, self.noise, self.over = [], [], [], [], [], []

    def adts(self, over=False):
        units = self.units + ([o[3] for o in self.over] if over else [])
        return b"".join(adts_frame(au, self.sf_index, self.channels) for au in units)


def _build(sf_index, channels):
    s = Stream(sf_index, channels)
    rng = np.random.default_rng([SEED, sf_index, channels, 0])
    for name, seq, grouping in SHAPES:
        for _ in range(DIRECTED_PER_SHAPE):
            s.units.append(directed_access_unit(rng, sf_index, channels, seq, grouping))
            s.label.append(name)
    rng = np.random.default_rng([SEED, sf_index, channels, 1])
    for _ in range(RANDOM_UNITS):
        s.units.append(random_access_unit(rng, sf_index, channels))
        s.label.append("random")
    dec = _Spy(s.asc)
    for k, au in enumerate(s.units):
        before, seen = dec.pns_state, len(dec.tns_seen)
        try:
            s.want.append(dec.decode_access_unit(au))
        except OF.AacError as e:
            raise AssertionError("the oracle refuses unit %d (%s) of index %d, %d ch: %s -- choose another SEED"
                                 % (k, s.label[k], sf_index, channels, e))
        s.tns.append(dec.tns_seen[seen:])
        s.noise.append(dec.pns_state != before)
    assert len(s.units) == len(s.want) == ACCEPTED
    n_long, n_short = band_counts(sf_index)
    rng = np.random.default_rng([SEED, sf_index, channels, 2])
    for name, seq, bands in (("only_long", ONLY_LONG, n_long), ("short_8_groups", EIGHT_SHORT, n_short)):
        if seq == EIGHT_SHORT and bands >= 15:
            continue                                   # the 4-bit field cannot name a band past a 15-band table
        first = s.units[s.label.index(name)]
        over = directed_access_unit(rng, sf_index, channels, seq, 0, over=1)
        dec = OF.Decoder(s.asc)
        first_want = dec.decode_access_unit(first)     # accepted above from the same generator state (a fresh decoder's)
        try:
            dec.decode_access_unit(over)
        except OF.AacError as e:
            s.over.append((name, first, first_want, over, e))
        else:
            raise AssertionError("the oracle accepts max_sfb one past the table at index %d (%s)" % (sf_index, name))
    return s


@functools.lru_cache(maxsize=None)
def cases(sf_index):
    """-> {1: Stream, 2: Stream}; treat as read-only"""
    return {channels: _build(sf_index, channels) for channels in (1, 2)}


def _top_band_nonzero(sf_index, coeffs, sequence):
    """per channel: does the last band of the table hold a non-zero value (in any window, for eight short)?"""
    out = []
    for c, seq in enumerate(sequence):
        if seq == EIGHT_SHORT:
            off = OF.short_offsets(sf_index)
            out.append(any(coeffs[c, w * 128 + off[-2]:w * 128 + off[-1]].any() for w in range(8)))
        else:
            off = OF.long_offsets(sf_index)
            out.append(bool(coeffs[c, off[-2]:off[-1]].any()))
    return out


def _cut_by_tns_limit(sf_index, sequence, max_sfb, tns):
    """Does a filter of this TNS data stop at the index's tns_max_bands?  tns.rs:103-174: a window's filters are stacked from the top
    of the table downwards and both ends of each go through min(., tns_max_bands, max_sfb).  A filter with an order whose top lies at
    or above tns_max_bands, in a unit whose max_sfb does too, ends at off[tns_max_bands] -- the index's table entry decides, not the
    unit.  (At index 5 long and at 3, 4, 5 short tns_max_bands equals the table's band count: the stop is the table's end as well.)"""
    short = sequence == EIGHT_SHORT
    limit = OF.tns_max_bands(sf_index, short)
    off = OF.short_offsets(sf_index) if short else OF.long_offsets(sf_index)
    bands = len(off) - 1
    if max_sfb < limit:
        return False
    for _res, filters in tns:
        bottom = bands
        for length, order, _direction, _bits, _coeffs in filters:
            top, bottom = bottom, max(bottom - length, 0)
            if order and top >= limit and min(bottom, limit) < limit:
                return True
    return False


@functools.lru_cache(maxsize=None)
def reach(sf_index):
    """-> {"top": {shape name: channels whose top band is non-zero}, "tns_long": units, "tns_short": units, "noise": units}"""
    out = {"top": {name: 0 for name, _, _ in SHAPES}, "tns_long": 0, "tns_short": 0, "noise": 0}
    for s in cases(sf_index).values():
        for k in range(ACCEPTED):
            coeffs, sequence, _ = s.want[k]
            if s.label[k] != "random":
                out["top"][s.label[k]] += sum(_top_band_nonzero(sf_index, coeffs, sequence))
            cut = [seq == EIGHT_SHORT for seq, max_sfb, tns in s.tns[k] if _cut_by_tns_limit(sf_index, seq, max_sfb, tns)]
            out["tns_long"] += False in cut
            out["tns_short"] += True in cut
            out["noise"] += s.noise[k]
    return out

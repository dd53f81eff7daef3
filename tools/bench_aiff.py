#!/usr/bin/env python
"""Times the AIFF streams' decode stage (csrc/aiff_decode.hip: k_aiff_ima4, k_aiff_elem) inside sk_tick_run_aiff at the size the
scheduler is built for.

Two encodings, 4096 stereo streams x 1 s at 44.1 kHz each, one unit per stream:
  ima4    690 groups of two 34-byte packets per stream (44 160 frames): 46 920 bytes in, 176 640 bytes of s16 out
  s24be   44 100 frames: 264 600 bytes in, the same out
  dvds24  (not in the default cases) DVD LPCM's 24-bit groups, SK_AIFF_DVD_S24: the same bytes in and out as s24be; --rate 48000 for a DVD's
each in two forms of the tick:
  plain   delivered as decoded (nothing further to change): the decode launch writes the output records
  to16k   -> 16 kHz mono s16: the decode launch fills the decoded buffer, then what sk_tick_run_pcm runs (k_pcm_ingest, the
          resampler rounds, k_pack_jobs)
For each the whole sk_tick_run_aiff call (host planning, the PCIe copy of the input up and of the output down, every launch, the
wait) as wall time over --steps calls after --warmup.  The kernels' own times are not taken here: run this script under
`rocprofv3 --kernel-trace --stats -- python tools/bench_aiff.py` and read k_aiff_ima4 / k_aiff_elem and the tick's other kernels from
the kernel statistics; the decode stage's share of the tick's device time is its time over the sum of all kernels of the case (run one
case per visit with --cases for that).  The script prints the decode launch's algorithmic bytes per call (bytes read + bytes written),
so that bytes / kernel time = rate and rate / 8 TB/s = the share of the HBM peak.
Prints one JSON line per case.  The input is seeded noise: the kernels' time does not depend on the samples, except that an IMA4
packet that saturates costs its wave one serial decode more -- noise saturates more often than speech or music do."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import soundkit_amd  # noqa: E402
from soundkit_amd._lib import AiffTickStream, PcmUnit, TickOutput, check, lib  # noqa: E402
from soundkit_amd.engine import AIFF_DVD_S24, AIFF_IMA4, AIFF_S24BE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--cases", default="ima4_plain,s24be_plain,ima4_to16k,s24be_to16k")
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    n, ch = args.streams, 2
    eng = soundkit_amd.Engine(0, max(n, 16))
    rng = np.random.default_rng(0)
    for case in [c for c in args.cases.split(",") if c]:
        name, form = case.split("_")
        if name == "ima4":
            enc, groups = AIFF_IMA4, (args.rate + 63) // 64
            frames, unit_bytes, decoded_bytes = groups * 64, groups * 34 * ch, groups * 128 * ch
        else:
            enc, frames = (AIFF_DVD_S24 if name == "dvds24" else AIFF_S24BE), args.rate // 2 * 2  # (whole 12-byte groups of four samples)
            unit_bytes = decoded_bytes = frames * 3 * ch
        stride = (unit_bytes + 15) & ~15
        blob = rng.integers(0, 256, n * stride, dtype=np.uint8)
        if name == "ima4":  # valid step indices in the headers
            view = blob.reshape(n, stride)[:, :unit_bytes].reshape(n, groups * ch, 34)
            view[:, :, 1] = (view[:, :, 1] & 0x80) | (view[:, :, 1] & 0x7f) % 89
        units = (PcmUnit * n)()
        ts = (AiffTickStream * n)()
        sids = []
        for s in range(n):
            units[s].byte_offset, units[s].byte_len = s * stride, unit_bytes
            ts[s].n_units, ts[s].encoding, ts[s].channels = 1, enc, ch
            if form == "to16k":
                sids.append(eng.open_stream(args.rate, ch))
                eng.resampler_open(sids[-1], args.rate, 16000)
                ts[s].stream, ts[s].resample, ts[s].out_bits, ts[s].out_channels = sids[-1], 1, 16, 1
            else:
                ts[s].out_bits, ts[s].out_channels = (16 if name == "ima4" else 24), ch
        max_out = C.c_uint32()
        cap = lib.sk_tick_aiff_out_bound_on(eng._h, ts, n, units, n, C.byref(max_out))
        assert cap, "the tick refuses this table"
        out = np.zeros(cap, np.uint8)
        recs = (TickOutput * max_out.value)()
        n_out, used = C.c_uint32(), C.c_size_t()
        times = []
        for step in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            check(lib.sk_tick_run_aiff(eng._h, ts, n, units, n, blob.ctypes.data, blob.size, out.ctypes.data, out.size, recs, max_out.value,
                                       C.byref(n_out), C.byref(used)), "sk_tick_run_aiff", eng._h)
            if step >= args.warmup:
                times.append(time.perf_counter() - t0)
        best = min(times)
        print(json.dumps({"case": case, "kernel": "k_aiff_ima4" if name == "ima4" else "k_aiff_elem", "streams": n, "channels": ch,
                          "frames_per_stream": frames, "input_bytes": n * unit_bytes, "decoded_bytes": n * decoded_bytes, "output_bytes": used.value,
                          "outputs": n_out.value, "decode_algorithmic_bytes_per_call": n * (unit_bytes + decoded_bytes),
                          "call_with_pcie_copies_ms_best": round(best * 1e3, 3), "call_with_pcie_copies_ms_all": [round(t * 1e3, 3) for t in times]}))
        for sid in sids:
            eng.close_stream(sid)
    eng.close()


if __name__ == "__main__":
    main()

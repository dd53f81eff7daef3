#!/usr/bin/env python
"""Times the PCM streams' tick (sk_tick_run_pcm: k_pcm_ingest, k_pcm_direct) at the size the scheduler is built for.

Two cases, 4096 streams x 1 s of 48 kHz stereo s16le each (786 MB of input in all):
  ingest   -> 16 kHz mono s16: k_pcm_ingest into the resampler rows, the resampler rounds, k_pack_jobs
  direct   -> 24-bit stereo, same rate: k_pcm_direct alone
and two on an engine of its own with the pool of wide streams, 1024 streams x 1 s of 48 kHz six-channel s16le each (590 MB):
  wide_ingest  -> 16 kHz mono s16: k_pcm_wide_ingest into six resampler rows per stream, the rounds, k_pcm_wide as the pack
  wide_direct  -> 24-bit stereo, same rate: k_pcm_wide twice (the peak pass, then the conversion)
For each: the whole sk_tick_run_pcm call (host planning, the PCIe copy of the input up and of the output down, every launch, the
wait) as wall time -- named "call, with PCIe copies" -- over --steps calls after --warmup.  The kernels' own times are not taken
here: run this script under `rocprofv3 --kernel-trace --stats -- python tools/bench_pcm_tick.py` and read k_pcm_ingest /
k_pcm_direct / k_pcm_wide_ingest / k_pcm_wide<true> (peak) / k_pcm_wide<false> from the kernel statistics (tools/profile_bench.sh
shows the form); the script prints the algorithmic bytes per call of either kernel (ingest: input bytes + 4 B per sample written;
direct: input + output bytes; the wide direct case's peak pass reads the input once more, printed separately), so that
    bytes / kernel time = rate, and rate / 8 TB/s = the share of the HBM peak.
Prints one JSON line per case.  The input is seeded noise: the kernels' time does not depend on the samples."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import soundkit_amd  # noqa: E402
from soundkit_amd._lib import PcmTickStream, PcmUnit, TickOutput, check, lib  # noqa: E402

FMT_S16LE = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--wide-streams", type=int, default=1024)
    ap.add_argument("--cases", default="ingest,direct,wide_ingest,wide_direct")
    ap.add_argument("--frames", type=int, default=48000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    cases = [c for c in args.cases.split(",") if c]
    for wide in (False, True):
        mine = [c for c in cases if c.startswith("wide_") == wide]
        if mine:
            run_cases(args, mine, wide)


def run_cases(args, cases, wide):
    n, frames, ch = (args.wide_streams, args.frames, 6) if wide else (args.streams, args.frames, 2)
    unit_bytes = frames * ch * 2
    stride = (unit_bytes + 15) & ~15
    eng = soundkit_amd.Engine(0, max(n, 16))
    if wide:
        eng.enable_wide_pcm(n)
    blob = np.random.default_rng(0).integers(0, 65536, n * stride // 2, dtype=np.uint16).view(np.uint8)
    units = (PcmUnit * n)()
    for s in range(n):
        units[s].byte_offset, units[s].byte_len = s * stride, unit_bytes
    for case in cases:
        ts = (PcmTickStream * n)()
        sids = []
        for s in range(n):
            ts[s].n_units, ts[s].format, ts[s].channels = 1, FMT_S16LE, ch
            if case.endswith("ingest"):
                sids.append(eng.open_stream(48000, ch))
                eng.resampler_open(sids[-1], 48000, 16000)
                ts[s].stream, ts[s].resample, ts[s].out_bits, ts[s].out_channels = sids[-1], 1, 16, 1
            else:
                ts[s].out_bits, ts[s].out_channels = 24, 2
        max_out = C.c_uint32()
        cap = lib.sk_tick_pcm_out_bound_on(eng._h, ts, n, units, n, C.byref(max_out))
        assert cap, "the tick refuses this table"
        out = np.zeros(cap, np.uint8)
        recs = (TickOutput * max_out.value)()
        n_out, used = C.c_uint32(), C.c_size_t()
        times = []
        for step in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            check(lib.sk_tick_run_pcm(eng._h, ts, n, units, n, blob.ctypes.data, blob.size, out.ctypes.data, out.size, recs, max_out.value,
                                      C.byref(n_out), C.byref(used)), "sk_tick_run_pcm", eng._h)
            if step >= args.warmup:
                times.append(time.perf_counter() - t0)
        samples = n * frames * ch
        in_bytes = n * unit_bytes
        algo = in_bytes + 4 * samples if case.endswith("ingest") else in_bytes + n * frames * 2 * 3
        best = min(times)
        extra = {"peak_pass_algorithmic_bytes_per_call": in_bytes} if case == "wide_direct" else {}
        kernel = {"wide_ingest": "k_pcm_wide_ingest", "wide_direct": "k_pcm_wide<false>"}.get(case, "k_pcm_" + case)
        print(json.dumps({**extra, "case": case, "kernel": kernel, "streams": n, "channels": ch, "frames_per_stream": frames, "input_bytes": in_bytes,
                          "output_bytes": used.value, "outputs": n_out.value, "kernel_algorithmic_bytes_per_call": algo,
                          "call_with_pcie_copies_ms_best": round(best * 1e3, 3), "call_with_pcie_copies_ms_all": [round(t * 1e3, 3) for t in times],
                          "call_input_GBps": round(in_bytes / best / 1e9, 2)}))
        for sid in sids:
            eng.close_stream(sid)
    eng.close()


if __name__ == "__main__":
    main()

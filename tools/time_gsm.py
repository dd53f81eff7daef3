#!/usr/bin/env python3
"""The GSM 06.10 decode stage (csrc/gsm_decode.hip) at a batch size, in the two shapes of tools/time_g72x.py:

  (a) 4096 streams x one 33-byte frame (20 ms, 160 samples), every stream in its own state after a first, untimed call over
      another frame;
  (b) 2048 streams x the whole fixture (4 884 bytes = 148 frames), every stream compared with the decoded twin after every call.

REPS sk_gsm_decode_batch calls per shape (after one that warms up the buffers and the code object).  Prints one JSON line per shape
with the host clock around the whole call (uploads, tables, the copy back included).  The kernels' own times come from a run of this
script under the profiler, in a run of its own:

    timeout -k 10 300 python tools/time_gsm.py [--reps 5] [--out FILE]
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_gsm.py --reps 3

profiles/gsm.md holds what was measured."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAME = "A_Tusk_is_used_to_make_costly_gifts"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--packet-streams", type=int, default=4096)
    ap.add_argument("--fixture-streams", type=int, default=2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import soundkit_amd
    from soundkit_amd import telephony
    from soundkit_amd._lib import G72xUnit, GsmState, GsmStream, check, lib

    golden = os.path.join(ROOT, "tests", "golden", "gsm")
    data = np.frombuffer(open(os.path.join(golden, NAME + ".gsm"), "rb").read(), np.uint8)
    wav = open(os.path.join(golden, NAME + ".decoded.wav"), "rb").read()
    twin = np.frombuffer(wav[wav.index(b"data") + 8:], np.uint8)
    eng = soundkit_amd.Engine(0, 8)
    lines = []
    try:
        for shape, streams, length in (("one 33-byte frame a stream", args.packet_streams, 33), ("the whole fixture a stream", args.fixture_streams, data.size)):
            whole = length == data.size
            decoded = length // 33 * 320  # bytes of s16 a unit gives
            stride = (length + 15) & ~15
            out_stride = (decoded + 15) & ~15
            ts = (GsmStream * streams)()
            units = (G72xUnit * streams)()
            for i in range(streams):
                ts[i].variant, ts[i].n_units, ts[i].state = telephony.GSM_STANDARD, 1, i
                units[i].offset, units[i].size = i * stride, length
            states = (GsmState * streams)()
            fresh = telephony.new_state(telephony.GSM)
            src = np.zeros(stride * streams, np.uint8)
            out = np.zeros(out_stride * streams, np.uint8)
            n = C.c_size_t(0)

            def call(first_byte):
                src.reshape(streams, stride)[:, :length] = data[first_byte:first_byte + length]
                t0 = time.perf_counter()
                check(lib.sk_gsm_decode_batch(eng._h, ts, streams, units, streams, src.ctypes.data_as(C.c_void_p), src.size, out.ctypes.data_as(C.c_void_p),
                                              out.size, C.byref(n), states, streams), "sk_gsm_decode_batch", eng._h)
                return (time.perf_counter() - t0) * 1e3

            times = []
            for rep in range(args.reps + 1):
                for i in range(streams):
                    states[i] = fresh
                if whole:
                    ms = call(0)
                    got = out.reshape(streams, out_stride)[:, :twin.size]
                    assert np.array_equal(got, np.broadcast_to(twin, got.shape))
                else:  # the stream's first frame brings the state off its initial value, the second one is timed
                    call(0)
                    ms = call(length)
                    got = out.reshape(streams, out_stride)[:, :decoded]
                    assert np.array_equal(got, np.broadcast_to(twin[decoded:2 * decoded], got.shape))
                if rep:  # the first call grows the buffers and loads the code object
                    times.append(ms)
            samples = streams * decoded // 2
            med = float(np.median(times))
            lines.append(json.dumps({"call": "sk_gsm_decode_batch", "codec": "GSM 06.10", "shape": shape, "streams": streams, "bytes_per_stream": int(length),
                                     "samples": int(samples), "call_ms_median": round(med, 3), "samples_per_second": round(samples / (med * 1e-3)),
                                     "call_ms_all": [round(t, 3) for t in times]}))
            print(lines[-1])
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The telephony decode stage (csrc/g72x_decode.hip) at a batch size, for G.726-32 and G.722 in two shapes each:

  (a) 4096 streams x one 20 ms packet (80 bytes of G.726-32 = 160 samples, 160 bytes of G.722 = 320 samples), every stream in its
      own state after a first call over another packet;
  (b) 2048 streams x the whole fixture (11 840 / 23 680 bytes), every stream compared with the decoded twin after every call.

REPS sk_g72x_decode_batch calls per shape (after one that warms up the buffers and the code object).  Prints one JSON line per shape
with the host clock around the whole call (uploads, tables, the copy back included).  The kernels' own times come from a run of this
script under the profiler, in a run of its own:

    timeout -k 10 300 python tools/time_g72x.py [--reps 5] [--out FILE]
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_g72x.py --reps 3

profiles/telephony.md holds what was measured."""
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
    from soundkit_amd._lib import G722State, G726State, G72xStream, G72xUnit, check, lib

    golden = os.path.join(ROOT, "tests", "golden")
    sources = {telephony.G726: ("g726/%s_32.g726" % NAME, "g726/%s_32.decoded.wav" % NAME), telephony.G722: ("g722/%s.g722" % NAME, "g722/%s.decoded.wav" % NAME)}
    eng = soundkit_amd.Engine(0, 8)
    lines = []
    try:
        for codec, (src_path, twin_path) in sources.items():
            data = np.frombuffer(open(os.path.join(golden, src_path), "rb").read(), np.uint8)
            wav = open(os.path.join(golden, twin_path), "rb").read()
            twin = np.frombuffer(wav[wav.index(b"data") + 8:], np.uint8)
            per_byte = 4  # bytes of s16 a source byte gives: two samples at 32 kbit/s and in G.722 alike
            packet = 80 if codec == telephony.G726 else 160
            for shape, streams, length in (("one 20 ms packet a stream", args.packet_streams, packet), ("the whole fixture a stream", args.fixture_streams, data.size)):
                whole = length == data.size
                stride = (length + 15) & ~15
                out_stride = (length * per_byte + 15) & ~15
                ts = (G72xStream * streams)()
                units = (G72xUnit * streams)()
                for i in range(streams):
                    ts[i].codec, ts[i].g726_rate, ts[i].g726_packing, ts[i].n_units, ts[i].state = codec, 32000, telephony.LEFT, 1, i
                    units[i].offset, units[i].size = i * stride, length
                s726, s722 = (G726State * streams)(), (G722State * streams)()
                fresh = telephony.new_state(codec)
                states = s726 if codec == telephony.G726 else s722
                src = np.zeros(stride * streams, np.uint8)
                out = np.zeros(out_stride * streams, np.uint8)
                n = C.c_size_t(0)

                def call(first_byte):
                    src.reshape(streams, stride)[:, :length] = data[first_byte:first_byte + length]
                    t0 = time.perf_counter()
                    check(lib.sk_g72x_decode_batch(eng._h, ts, streams, units, streams, src.ctypes.data_as(C.c_void_p), src.size, out.ctypes.data_as(C.c_void_p),
                                                   out.size, C.byref(n), s726, streams if codec == telephony.G726 else 0, s722,
                                                   streams if codec == telephony.G722 else 0), "sk_g72x_decode_batch", eng._h)
                    return (time.perf_counter() - t0) * 1e3

                times = []
                for rep in range(args.reps + 1):
                    for i in range(streams):
                        states[i] = fresh
                    if whole:
                        ms = call(0)
                        got = out.reshape(streams, out_stride)[:, :twin.size]
                        assert np.array_equal(got, np.broadcast_to(twin, got.shape))
                    else:  # the stream's first packet brings the state off its initial value, the second one is timed
                        call(0)
                        ms = call(length)
                        got = out.reshape(streams, out_stride)[:, :length * per_byte]
                        assert np.array_equal(got, np.broadcast_to(twin[length * per_byte:2 * length * per_byte], got.shape))
                    if rep:  # the first call grows the buffers and loads the code object
                        times.append(ms)
                samples = streams * length * per_byte // 2
                med = float(np.median(times))
                lines.append(json.dumps({"call": "sk_g72x_decode_batch", "codec": "G.726-32" if codec == telephony.G726 else "G.722", "shape": shape,
                                         "streams": streams, "bytes_per_stream": int(length), "samples": int(samples), "call_ms_median": round(med, 3),
                                         "samples_per_second": round(samples / (med * 1e-3)), "call_ms_all": [round(t, 3) for t in times]}))
                print(lines[-1])
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()

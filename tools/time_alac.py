#!/usr/bin/env python3
"""The ALAC decode stage (csrc/alac_decode.hip) at a batch size: the mono fixture tiled to STREAMS streams, every stream with its own
copy of the packets, REPS sk_alac_decode_packets calls over all of them (after one that warms up the buffers and the code object), each
checked against the fixture's decoded twin.  Prints one JSON line with the host clock around the whole call (uploads, the host's read of
every packet's frame count and the copy back included).  The three kernels' own times come from a run of this script under the
profiler, in a run of its own:

    timeout -k 10 300 python tools/time_alac.py [--streams 2048] [--reps 5] [--out FILE]
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_alac.py

profiles/alac.md holds what was measured."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clip", default=os.path.join(ROOT, "tests", "golden", "alac", "A_Tusk_is_used_to_make_costly_gifts.caf"))
    ap.add_argument("--twin", default=os.path.join(ROOT, "tests", "golden", "alac", "A_Tusk_is_used_to_make_costly_gifts.decoded.wav"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import soundkit_amd
    from soundkit_amd import alac
    from soundkit_amd._lib import AlacPacket, check, lib

    data = open(args.clip, "rb").read()
    index = alac.CafAlacPacketIndex.from_file(data)
    packets = index.packet_bytes(data)
    table1, blob1 = alac.pack_packets(packets)
    n1 = len(packets)
    stride = (len(blob1) + 255) & ~255
    one = np.frombuffer(bytes(table1), np.dtype(AlacPacket))[:n1]
    table = np.tile(one, args.streams)
    table["offset"] += np.repeat(np.arange(args.streams, dtype=np.uint32) * np.uint32(stride), n1)
    src = np.zeros(stride * args.streams, np.uint8)
    src.reshape(args.streams, stride)[:, :len(blob1)] = np.frombuffer(blob1, np.uint8)
    wav = open(args.twin, "rb").read()
    twin = np.frombuffer(wav[wav.index(b"data") + 8:], np.uint8)
    pcm_bytes = twin.size
    out = np.zeros(pcm_bytes * args.streams, np.uint8)
    status = np.zeros(n1 * args.streams, np.int32)
    frames = np.zeros(n1 * args.streams, np.uint32)
    cfg = alac.config(index.config)
    n = C.c_size_t(0)

    eng = soundkit_amd.Engine(0, 8)
    try:
        times = []
        for rep in range(args.reps + 1):
            out[:] = 0
            t0 = time.perf_counter()
            check(lib.sk_alac_decode_packets(eng._h, C.byref(cfg), table.ctypes.data_as(C.c_void_p), n1 * args.streams, src.ctypes.data_as(C.c_void_p),
                                             out.ctypes.data_as(C.c_void_p), out.size, C.byref(n), status.ctypes.data_as(C.c_void_p),
                                             frames.ctypes.data_as(C.c_void_p)), "sk_alac_decode_packets", eng._h)
            ms = (time.perf_counter() - t0) * 1e3
            assert n.value == out.size and not status.any()
            assert np.array_equal(out.reshape(args.streams, pcm_bytes), np.broadcast_to(twin, (args.streams, pcm_bytes)))
            if rep:  # the first call grows the buffers and loads the code object
                times.append(ms)
        result = {
            "call": "sk_alac_decode_packets", "streams": args.streams, "packets": n1 * args.streams, "packet_bytes_read": len(blob1) * args.streams,
            "pcm_bytes_written": int(out.size), "samples": int(out.size // 2), "call_ms_median": round(float(np.median(times)), 3),
            "call_ms_all": [round(t, 3) for t in times],
        }
        line = json.dumps(result)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()

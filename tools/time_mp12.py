#!/usr/bin/env python3
"""Kernel time of the Layer I / II stage call (csrc/mp12_synth.hip): the MP2 fixture tiled to STREAMS stereo streams x FRAMES frames,
every stream with its own copy of the bytes, one sk_mpa_decode_frames_timed launch per repetition (HIP events around the launch
alone).  Prints one JSON line; profiles/mp12.md holds a measured run.  Run it under a time limit:

    timeout -k 10 300 python tools/time_mp12.py [--streams 2048] [--frames 16] [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--clip", default=os.path.join(ROOT, "tests", "golden", "mp2", "stereo48k_A_Tusk_1s.mp2"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import soundkit_amd
    from soundkit_amd import mp3
    from soundkit_amd._lib import MpaFrameRecord

    data = open(args.clip, "rb").read()
    infos, _, layer = mp3.mpa_scan(data)
    infos = infos[:args.frames]
    assert len(infos) == args.frames and layer in (1, 2)
    one = []
    for f in infos:
        rc, rec = mp3.mpa_parse_frame(data[f.offset:f.offset + f.frame_bytes], f)
        assert rc == 0
        one.append((rec, data[f.offset:f.offset + f.frame_bytes]))
    recs1, n1, buf1 = mp3.mpa_pack_frames(one)
    stride = (buf1.size + 255) & ~255
    buf = np.zeros(stride * args.streams, np.uint8)
    recs = (MpaFrameRecord * (n1 * args.streams))()
    for s in range(args.streams):
        buf[s * stride:s * stride + buf1.size] = buf1
        for i in range(n1):
            recs[s * n1 + i] = recs1[i]
            recs[s * n1 + i].byte_offset = s * stride + recs1[i].byte_offset
    frame_bytes = sum(f.frame_bytes for f in infos) * args.streams
    samples = sum(f.samples_per_channel * f.channels for f in infos) * args.streams

    eng = soundkit_amd.Engine(0, args.streams + 8)
    try:
        mp3.set_synthesis_window(np.ctypeslib.as_array(mp3.iso_tables().window), eng)
        sids = [eng.open_stream(infos[0].sample_rate, infos[0].channels) for _ in range(args.streams)]
        ids = np.repeat(np.asarray(sids, np.uint32), n1)
        times = []
        for rep in range(args.reps + 1):
            rc, pcm, st, ms = mp3.mpa_decode_frames(recs, ids, n1 * args.streams, buf, eng, timed=True, out_cap=samples)
            assert rc == 0 and not st.any() and pcm.size == samples, (rc, pcm.size)
            if rep:  # the first launch pays for the code object
                times.append(ms)
        ms = float(np.median(times))
        result = {
            "kernel": "k_mp12_synth", "streams": args.streams, "frames_per_stream": args.frames, "layer": layer,
            "kernel_ms_median": round(ms, 4), "kernel_ms_all": [round(t, 4) for t in times],
            "frame_bytes_read": frame_bytes, "pcm_bytes_written_s16": samples * 2,
            "tb_per_s_on_its_own_bytes": round((frame_bytes + samples * 2) / (ms * 1e-3) / 1e12, 4),
            "units_of_576_per_s": round(samples / infos[0].channels / 576 / (ms * 1e-3)),
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

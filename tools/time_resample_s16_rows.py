#!/usr/bin/env python3
"""Times the any-rate decode tail's resample step on the device: sk_downsample_frames_s16_to_s16_dev (planar s16 frames in,
interleaved s16 out, one entry) against the route to the same bytes without it -- widen and repack the s16 frames to f32 rows,
sk_downsample_f32_dev, sk_pcm_f32_planar_to_bytes_batch_dev(SK_FMT_S16LE) -- and against sk_downsample_f32_dev alone on f32 rows
of the same shape.  Device events on the engine's stream around each call, after a warm-up; the three are alternated inside every
repetition so that they share whatever else the box is doing; median, minimum and the 10th / 90th percentiles per form.

    python tools/time_resample_s16_rows.py                       # 4096 streams x 2 ch x 43 frames of 44.1 -> 16 kHz, 30 repetitions
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_resample_s16_rows.py --reps 10
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE ... -d DIR -- python tools/time_resample_s16_rows.py --only new --reps 3

Prints one JSON line.  A run without a GPU fails: there is nothing to time on a CPU."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--ch", type=int, default=2)
    ap.add_argument("--frames", type=int, default=43)
    ap.add_argument("--in-hz", type=int, default=44100)
    ap.add_argument("--out-hz", type=int, default=16000)
    ap.add_argument("--layout", choices=["frame", "stream"], default="frame")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["new", "route", "f32"], default=None)
    args = ap.parse_args()

    import torch
    import soundkit_amd
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    dev = torch.device("cuda:0")
    streams, ch, frames = args.streams, args.ch, args.frames
    eng = soundkit_amd.Engine(0, 8)
    ext = torch.cuda.ExternalStream(eng.hip_stream, device=dev)
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randint(-32768, 32768, (streams, frames, ch, 1024), generator=g, device=dev, dtype=torch.int32).to(torch.int16)
    if args.layout == "frame":
        d_in = x.transpose(0, 1).contiguous()             # [frames][streams][ch][1024]
        as_rows = d_in.permute(1, 2, 0, 3)                # -> [streams][ch][frames][1024]
        strides = (ch * 1024, streams * ch * 1024)
    else:
        d_in = x
        as_rows = d_in.permute(0, 2, 1, 3)
        strides = (frames * ch * 1024, ch * 1024)
    del x
    samples = frames * 1024
    n_out = eng.downsample_out_frames(samples, args.in_hz, args.out_hz)
    o_stride = (n_out + 7) // 8 * 8
    rows = torch.zeros((streams * ch, samples), device=dev)
    f32_out = torch.zeros((streams * ch, o_stride), device=dev)
    out_new = torch.zeros((streams, o_stride, ch), dtype=torch.int16, device=dev)
    out_route = torch.zeros((streams, n_out, ch), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()

    def new():
        eng.downsample_frames_s16_to_s16_dev(d_in, strides[0], strides[1], ch, streams, frames, args.in_hz, args.out_hz, out_new, o_stride)

    def widen():
        with torch.cuda.stream(ext):
            torch.mul(as_rows, 1.0 / 32768.0, out=rows.view(streams, ch, frames, 1024))

    def f32():
        eng.downsample_dev(rows, samples, streams * ch, samples, args.in_hz, args.out_hz, f32_out, o_stride)

    def route():
        widen()
        f32()
        eng.f32_planar_to_bytes_batch_dev(0, f32_out, streams, o_stride, n_out, ch, out_route)

    forms = {"new": new, "route": route, "f32": f32}
    if args.only:
        forms = {args.only: forms[args.only]}
    widen()
    eng.synchronize()
    times = {k: [] for k in forms}
    for rep in range(args.warmup + args.reps):
        pairs = {}
        for name, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ext)
            fn()
            b.record(ext)
            pairs[name] = (a, b)
        eng.synchronize()
        torch.cuda.synchronize()
        if rep >= args.warmup:
            for name, (a, b) in pairs.items():
                times[name].append(a.elapsed_time(b))
    report = {"shape": {"streams": streams, "channels": ch, "frames": frames, "in_hz": args.in_hz, "out_hz": args.out_hz, "layout": args.layout,
                        "out_frames": n_out}, "reps": args.reps, "device": torch.cuda.get_device_name(0), "ms": {}}
    for name, t in times.items():
        t = np.array(t)
        report["ms"][name] = {"median": round(float(np.median(t)), 4), "min": round(float(t.min()), 4), "p10": round(float(np.percentile(t, 10)), 4),
                              "p90": round(float(np.percentile(t, 90)), 4), "max": round(float(t.max()), 4)}
    if "new" in forms and "route" in forms:
        d = (out_new[:, :n_out].to(torch.int32) - out_route.to(torch.int32)).abs()
        report["new_vs_route"] = {"max_abs_lsb": int(d.max()), "differing_fraction": float((d > 0).float().mean())}
    eng.close()
    print(json.dumps(report))


if __name__ == "__main__":
    main()

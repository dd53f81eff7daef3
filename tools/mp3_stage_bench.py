"""The two GPU stages of the MP3 path at scale, for rocprofv3 --kernel-trace --stats (profiles/r03_mp3_kernel_stats.csv):
STREAMS stereo streams x GRANULES granules of random integers through sk_mp3_decode_granules_s16 (requantisation +
mid/side + reorder, then the hybrid synthesis), band tables and window synthetic.  Host-buffer entry point: the wall time
printed includes the PCIe copies; the kernel times are what the profiler reports.
    python3 tools/mp3_stage_bench.py [streams] [granules_per_stream] [repeats]
--stage entropy [--clip FILE]: the stage in front of them instead (k_mp3_entropy through sk_mp3_entropy_decode) -- the frames of
a real MP3 file (default: the stereo fixture, the file tools/mp3_host_rate.cpp reads), framed on the host once and tiled to STREAMS x
GRANULES granules, the standard's tables.  Timed like the other leg: the wall time is the host-buffer call, the kernel time is the
profiler's."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import soundkit_amd  # noqa: E402
from soundkit_amd import mp3  # noqa: E402
from soundkit_amd._lib import Mp3GranuleDesc, check, lib  # noqa: E402
from soundkit_amd.engine import _ptr  # noqa: E402


def entropy_leg(streams, per, repeats, clip):
    from soundkit_amd._lib import Mp3FrameItem, Mp3GranuleData
    data = open(clip, "rb").read()
    found, _, _ = mp3.scan_free(data)
    frames, kept = [], b""
    for f in found:
        frame = data[f.offset:f.offset + f.frame_bytes]
        rc, side = mp3.parse_side_info(frame, f)
        if rc == 0:
            rc, main = mp3.main_data(frame, f, side, kept)
            if rc == 0:
                frames.append((f, side, main))
        kept = (kept + frame[4 + 2 * f.has_crc + f.side_info_bytes:])[-2048:]
    per_frame = frames[0][0].granules
    want = streams * per // per_frame  # frames
    items, n, buf = mp3.pack_frames(frames)
    tiles = -(-want // n)
    words = np.frombuffer(bytes(items), np.uint32).reshape(-1, C.sizeof(Mp3FrameItem) // 4)[:n]
    tiled = np.tile(words, (tiles, 1))
    tiled[:, Mp3FrameItem.byte_offset.offset // 4] += np.repeat(np.arange(tiles, dtype=np.uint32) * np.uint32(buf.size), n)
    tiled = np.ascontiguousarray(tiled[:want])
    big = np.tile(buf, tiles)
    cells = sum(f.granules * f.channels for f, _, _ in frames) * tiles  # an upper bound is enough for the output room
    engine = soundkit_amd.Engine(0, 16)
    mp3.set_codebook(None, engine)
    out = np.zeros((want, 4 * C.sizeof(Mp3GranuleData)), np.uint8)
    arr = (Mp3FrameItem * want).from_buffer(tiled)
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        check(lib.sk_mp3_entropy_decode(engine._h, arr, want, _ptr(big), big.size, _ptr(out)), "sk_mp3_entropy_decode", engine._h)
        times.append(time.perf_counter() - t0)
    status = out.view(np.int32).reshape(want, 4, -1)[:, :, -1]
    n_cells = want * per_frame * frames[0][0].channels
    assert not status.any() and out.any() and cells >= n_cells
    best = min(times)
    print(json.dumps({"workload": "mp3 entropy stage: %d frames of %s tiled (%d granule-channels), main data in host memory -> integers and scale factors in host memory"
                                  % (want, os.path.basename(clip), n_cells),
                      "granule_channels": n_cells, "main_data_bytes": int(big.size), "best_call_ms": best * 1e3, "granule_channels_per_s": n_cells / best,
                      "note": "wall time of the host-buffer call incl. PCIe (1152 B of integers per granule-channel come back); kernel time: rocprofv3 stats"}))
    engine.close()


def main():
    args = sys.argv[1:]
    stage, clip = "synthesis", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "mp3", "stereo16k_A_Tusk_encoded.mp3")
    while "--stage" in args or "--clip" in args:
        at = args.index("--stage") if "--stage" in args else args.index("--clip")
        if args[at] == "--stage":
            stage = args[at + 1]
        else:
            clip = args[at + 1]
        del args[at:at + 2]
    streams = int(args[0]) if len(args) > 0 else 2048
    per = int(args[1]) if len(args) > 1 else 32
    repeats = int(args[2]) if len(args) > 2 else 5
    if stage == "entropy":
        return entropy_leg(streams, per, repeats, clip)
    rng = np.random.default_rng(1)
    engine = soundkit_amd.Engine(0, streams)
    long_o = np.array([0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 52, 62, 74, 90, 110, 134, 162, 196, 238, 288, 342, 418, 576], np.uint16)
    short_o = np.array([0, 4, 8, 12, 16, 22, 30, 40, 52, 66, 84, 106, 136, 192], np.uint16)
    assert mp3.set_band_tables(44100, long_o, short_o, np.zeros(22, np.uint8), engine) == 0
    from oracle import mp3_hybrid
    mp3.set_synthesis_window(mp3_hybrid.synthetic_window(3), engine)
    sids = [engine.open_stream(44100, 2) for _ in range(streams)]
    n = streams * per
    granules = []
    for g in range(per):          # granule-major: the streams advance together
        for s in range(streams):
            bt = int(rng.integers(0, 4)) if (s % 8 == 0) else 0
            ch = {"global_gain": 130, "scalefac_scale": 0, "preflag": 0, "block_type": bt, "mixed_block_flag": 0, "subblock_gain": [0, 0, 0],
                  "scalefac_l": [1] * 21 + [0], "scalefac_s": [[1, 1, 1]] * 12 + [[0, 0, 0]]}
            granules.append((sids[s], {"sample_rate": 44100, "channels": 2, "ms_stereo": 1, "ch": [ch, ch]}, bt))
    req = mp3.make_requant_granules([g for _, g, _ in granules])
    descs = (Mp3GranuleDesc * n)()
    for i, (sid, _, bt) in enumerate(granules):
        descs[i].stream, descs[i].channels = sid, 2
        descs[i].block_type[0] = descs[i].block_type[1] = bt
    quant = rng.integers(-8, 9, (2 * n, 576)).astype(np.int16)
    pcm = np.zeros((n, 576, 2), np.int16)
    status = np.zeros(n, np.int32)
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        check(lib.sk_mp3_decode_granules_s16(engine._h, req, descs, _ptr(quant), _ptr(pcm), n, _ptr(status)), "sk_mp3_decode_granules_s16", engine._h)
        times.append(time.perf_counter() - t0)
    assert not status.any() and pcm.any()
    best = min(times)
    print(json.dumps({"workload": "mp3 stages: %d stereo streams x %d granules (44.1 kHz), integers in host memory -> s16 PCM in host memory" % (streams, per),
                      "granule_channels": 2 * n, "best_call_ms": best * 1e3, "granule_channels_per_s": 2 * n / best,
                      "x_realtime_stereo": n * 576 / 44100 / best, "note": "wall time of the host-buffer call incl. PCIe; kernel times: rocprofv3 stats"}))
    engine.close()


if __name__ == "__main__":
    main()

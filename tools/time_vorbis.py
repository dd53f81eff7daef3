"""Times the Vorbis decode stage (sk_vorbis_decode_packets) in two shapes on the reference's Ogg fixture (profiles/vorbis.md):

  (a) 4 096 streams x one audio packet each.  Every stream decodes its first packets in a call that is not timed, so that the timed one
      starts from a carried overlap and yields 256 samples a stream;
  (b) 2 048 streams x the whole fixture (94 audio packets, 23 808 samples before the granule cut).

Host clock around the C call, pageable buffers, uploads and the copy back included.  After every call every stream's samples are compared
with a yardstick's hash.  The yardstick is one stream decoded alone, which is first held to tests/vorbis_model.py (float64, narrowed by
truncation): within one step on every sample.

    timeout -k 10 300 python tools/time_vorbis.py --reps 5"""
import argparse
import ctypes as C
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--streams-a", type=int, default=4096)
    ap.add_argument("--streams-b", type=int, default=2048)
    ap.add_argument("--shape", choices=("a", "b", "both"), default="both")
    args = ap.parse_args()

    import soundkit_amd
    import vorbis_model as M
    from soundkit_amd import vorbis
    from soundkit_amd._lib import check, lib
    from soundkit_amd.engine import _ptr

    data = open(os.path.join(ROOT, "tests", "golden", "vorbis", "A_Tusk_is_used_to_make_costly_gifts.ogg"), "rb").read()
    pk = [p["data"] for p in M.ogg_packets(data)]
    ident = vorbis.parse_ident(pk[0])
    setup = vorbis.Setup(ident, pk[2])
    audio = pk[3:]
    eng = soundkit_amd.Engine(0, 64)

    # the yardstick: one stream alone, against the model
    one = vorbis.decode_packets([(vorbis.StreamState(setup), audio)], engine=eng)[0]
    assert all(s == 0 for s, _ in one)
    mset = M.parse_setup(pk[2], ident["channels"], ident["blocksize_0"], ident["blocksize_1"])
    st, want = M.Stream(mset, np.float64), []
    for p in audio:
        want.append(M.to_s16(st.decode(p)[1][0]))
    d = np.abs(np.concatenate([x.reshape(-1) for _, x in one]).astype(np.int32) - np.concatenate(want).astype(np.int32))
    assert d.max() <= 1, d.max()
    print("yardstick: %d samples, %d one step from the float64 model" % (d.size, int((d > 0).sum())))

    def run(name, n_streams, packets, warm):
        """n_streams identical streams, `warm` decoded first (not timed), then `packets` per stream in one timed call"""
        states = [vorbis.StreamState(setup) for _ in range(n_streams)]
        if warm:
            vorbis.decode_packets([(s, warm) for s in states], engine=eng)
        ref_state = vorbis.StreamState(setup)
        if warm:
            vorbis.decode_packets([(ref_state, warm)], engine=eng)
        ref = np.concatenate([x.reshape(-1) for _, x in vorbis.decode_packets([(ref_state.copy(), packets)], engine=eng)[0]])
        ref_hash = hashlib.sha256(ref.tobytes()).hexdigest()
        times = []
        for rep in range(args.reps + 1):
            work = [s.copy() for s in states]
            streams, table, blob, n = vorbis._pack([(s, packets) for s in work])
            src = np.frombuffer(blob, np.uint8)
            out = np.zeros(n_streams * ref.size, np.int16)
            status, frames, used = np.zeros(n, np.int32), np.zeros(n, np.uint32), C.c_size_t(0)
            t0 = time.perf_counter()
            check(lib.sk_vorbis_decode_packets(eng._h, streams, n_streams, table, n, _ptr(src), len(blob), 0, _ptr(out), out.nbytes, C.byref(used),
                                               _ptr(status), _ptr(frames)), "sk_vorbis_decode_packets", eng._h)
            dt = time.perf_counter() - t0
            assert not status.any() and used.value == out.nbytes
            rows = out.reshape(n_streams, ref.size)
            bad = [i for i in range(n_streams) if hashlib.sha256(rows[i].tobytes()).hexdigest() != ref_hash]
            assert not bad, "%s: %d streams differ from the yardstick, first %d" % (name, len(bad), bad[0])
            if rep:
                times.append(dt)
        med = statistics.median(times)
        print("%s: %d streams x %d packets, %d samples a call: median of %d %.3f ms (%.3f ... %.3f), %.3g samples / s" % (
            name, n_streams, len(packets), n_streams * ref.size, len(times), med * 1e3, min(times) * 1e3, max(times) * 1e3, n_streams * ref.size / med))

    if args.shape in ("a", "both"):
        run("(a)", args.streams_a, audio[40:41], audio[:40])
    if args.shape in ("b", "both"):
        run("(b)", args.streams_b, audio, [])
    eng.close()


if __name__ == "__main__":
    main()

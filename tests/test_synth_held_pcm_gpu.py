"""The synthesis kernels keep a frame's packed PCM in registers for one frame and store it at the top of the next one (after
the loop for a task's last frame; in front of an EightShort frame's own stores) -- profiles/synth_store_drain.md.  A delay of
the stores can go wrong in small ways: a frame never stored, stored twice, or stored at the offset of another frame.  So:
1, 2, 3 and 8 frames per launch, five stereo streams and one mono stream (pairs, and a partnerless channel in the
one-channel kernels), both batch layouts, both output types, OnlyLong / a LongStart-LongStop bracket / coinciding EightShort.

  (a) one launch of N frames = N launches of one frame, byte for byte: PCM, carried delay, prev_shape
  (b) the PCM buffer is poisoned first -- one frame past the end and the two slots of a refused frame at offset 0 included
      (a held offset starts as 0) -- and only the expected slots change
  (c) f32 against the oracle at test_aac_synth_gpu's bounds; s16 = the oracle's conversion of the f32 output, bit for bit,
      as in test_s16_chain_gpu
  (d) sk_aac_plan_run_tail_s16_dev still equals the two calls on the batch's stereo streams
"""
import numpy as np
import pytest

import soundkit_amd
from test_aac_synth_gpu import RMS_TOL, rel_rms

pytestmark = pytest.mark.gpu

CHANNELS = [2, 2, 2, 2, 2, 1]   # per stream; the mono stream's channel finds no partner
FRAME_SLOTS = sum(CHANNELS)     # 1024-sample slots one frame of all streams takes
DEAD_STREAM = 0xFFFF0000        # never opened: its frame is refused and its two slots at offset 0 stay as they were
POISON16 = 0x5A5B
POISON32 = 0x7FC5A5B7           # (a NaN: compared as bits)
FRAME_COUNTS = [1, 2, 3, 8]


def sequences(kind, n, s):
    """window sequence of each of stream s's n frames (both channels switch together)"""
    seq = [0] * n
    if kind == "bracket" and s % 2:
        if n == 1:
            seq = [1]
        else:
            a = (n - 2) // 2
            seq[a], seq[a + 1] = 1, 3
    elif kind == "short":
        if n == 1:
            seq = [2]
        elif n == 2:
            seq = [2, 3] if s % 3 == 0 else [1, 2]   # a long frame behind the short one / a held frame in front of a final short one
        elif n == 3:
            seq = [1, 2, 3]
        else:
            seq = [0, 1, 2, 2, 3, 0, 1, 2] if s % 2 else [0, 0, 1, 2, 3, 0, 0, 0]
    return seq


_batches = {}


def batch(oracle, kind, n):
    """spectra, windows and the oracle's PCM and final state of every stream: computed once per (kind, n), never changed"""
    key = (kind, n)
    if key not in _batches:
        per = []
        for s, ch in enumerate(CHANNELS):
            coeffs = np.empty((n, ch, 1024), np.float32)
            for f in range(n):
                for c in range(ch):
                    coeffs[f, c] = oracle.seeded_spectrum(1024, 0x51F15EED + 977 * s + 2 * f + c) * np.float32(9000.0)
            seq = sequences(kind, n, s)
            seqs = np.array([[q, q] for q in seq], np.uint8)
            shapes = np.array([[(f + s) & 1, (f // 2 + s) & 1] for f in range(n)], np.uint8)
            want, chans = oracle.synthesize_stream(coeffs, seqs, shapes)
            for a in (coeffs, seqs, shapes, want):
                a.setflags(write=False)
            per.append((coeffs, seqs, shapes, want, [(c.delay, c.prev_shape) for c in chans]))
        _batches[key] = per
    return _batches[key]


def frame_order(layout, n, streams):
    return [(s, f) for f in range(n) for s in streams] if layout == "frame" else [(s, f) for s in streams for f in range(n)]


def poisoned(torch, slots, dtype):
    if dtype == torch.int16:
        return torch.full((slots, 1024), POISON16, dtype=torch.int16, device="cuda")
    return torch.full((slots, 1024), POISON32, dtype=torch.int32, device="cuda").view(torch.float32)


def bits(t):
    """host copy as integers, so that NaN poison compares equal to itself"""
    a = t.cpu().numpy()
    return a.view(np.int32) if a.dtype == np.float32 else a


def run_plan(plan, out16, d_coeffs, d_pcm):
    if out16:
        plan.run_s16_planar(d_coeffs, d_pcm)
    else:
        plan.run_f32(d_coeffs, d_pcm)


@pytest.mark.parametrize("layout", ["frame", "stream"])
@pytest.mark.parametrize("kind", ["long", "bracket", "short"])
@pytest.mark.parametrize("n", FRAME_COUNTS)
def test_one_launch_equals_single_frame_launches_and_touches_only_its_slots(engine, oracle, n, kind, layout):
    import torch
    per = batch(oracle, kind, n)
    streams = list(range(len(CHANNELS)))
    sids = [engine.open_stream(48000, ch) for ch in CHANNELS]
    order = frame_order(layout, n, streams)
    # the whole batch behind one refused frame: slot of (s, f), channel c = at[(s, f)] + c
    at, slot = {}, 2
    frames = [(DEAD_STREAM, 2, (0, 0), (0, 0))]
    for s, f in order:
        at[(s, f)] = slot
        slot += CHANNELS[s]
        frames.append((sids[s], CHANNELS[s], per[s][1][f], per[s][2][f]))
    used = slot
    assert used == 2 + n * FRAME_SLOTS
    total = used + FRAME_SLOTS  # one frame of every stream past the end
    descs, nd = soundkit_amd.make_descs(frames)
    plan = engine.plan(descs, nd)
    assert plan.status.tolist() == [1] + [0] * (nd - 1)
    host = np.zeros((total, 1024), np.float32)
    for (s, f), a in at.items():
        host[a:a + CHANNELS[s]] = per[s][0][f]
    d_coeffs = torch.from_numpy(host).cuda()
    # single-frame plans: frame f of every stream, packed in stream order
    single_at = np.concatenate([[0], np.cumsum(CHANNELS)])
    singles = []
    for f in range(n):
        d1, n1 = soundkit_amd.make_descs([(sids[s], CHANNELS[s], per[s][1][f], per[s][2][f]) for s in streams])
        c1 = torch.from_numpy(np.concatenate([per[s][0][f] for s in streams])).cuda()
        singles.append((engine.plan(d1, n1), c1))
    torch.cuda.synchronize()

    f32_out = None
    for out16 in (False, True):
        dtype = torch.int16 if out16 else torch.float32
        # N launches of one frame
        for sid in sids:
            engine.reset_stream(sid)
        parts = []
        for p1, c1 in singles:
            o1 = poisoned(torch, FRAME_SLOTS + 1, dtype)
            torch.cuda.synchronize()
            run_plan(p1, out16, c1, o1)
            engine.synchronize()
            o1 = bits(o1)
            assert (o1[FRAME_SLOTS] == (POISON16 if out16 else POISON32)).all()
            parts.append(o1)
        state_parts = [engine.get_state(sids[s], CHANNELS[s]) for s in streams]
        # one launch of N frames
        for sid in sids:
            engine.reset_stream(sid)
        d_pcm = poisoned(torch, total, dtype)
        torch.cuda.synchronize()
        run_plan(plan, out16, d_coeffs, d_pcm)
        engine.synchronize()
        got = bits(d_pcm)
        state_got = [engine.get_state(sids[s], CHANNELS[s]) for s in streams]
        # (b) the refused frame's slots and the frame past the end are untouched, every expected slot is written
        poison = POISON16 if out16 else POISON32
        assert (got[:2] == poison).all(), "slots of the refused frame at offset 0 were written"
        assert (got[used:] == poison).all(), "slots past the end were written"
        for (s, f), a in at.items():
            for c in range(CHANNELS[s]):
                assert (got[a + c] != poison).mean() > 0.99, (s, f, c, "not stored")
        # (a) byte for byte the single-frame launches, and the carried state
        for (s, f), a in at.items():
            b = single_at[s]
            assert np.array_equal(got[a:a + CHANNELS[s]], parts[f][b:b + CHANNELS[s]]), (s, f, out16)
        for s in streams:
            assert np.array_equal(state_got[s][0].view(np.int32), state_parts[s][0].view(np.int32)), (s, "delay")
            assert np.array_equal(state_got[s][1], state_parts[s][1]), (s, "prev_shape")
        # (c) against the oracle
        if not out16:
            f32_out = got.view(np.float32)
            for s in streams:
                mine = np.stack([f32_out[at[(s, f)]:at[(s, f)] + CHANNELS[s]] for f in range(n)])
                want = per[s][3]
                assert rel_rms(mine, want) < RMS_TOL, s
                for c in range(CHANNELS[s]):
                    assert rel_rms(state_got[s][0][c], per[s][4][c][0]) < RMS_TOL, (s, c)
                    assert state_got[s][1][c] == per[s][4][c][1], (s, c)
        else:
            want16 = oracle.pcm_convert("FLOAT_TO_I16_ROUND", f32_out[2:used].ravel()).reshape(-1, 1024)
            assert np.array_equal(got[2:used], want16)
            assert np.abs(got[2:used].astype(np.int32)).max() > 1000   # far above the rounding step: a single frame has no overlap added yet

    plan.destroy()
    for p1, _ in singles:
        p1.destroy()
    for sid in sids:
        engine.close_stream(sid)


@pytest.mark.parametrize("layout", ["frame", "stream"])
@pytest.mark.parametrize("kind", ["long", "bracket"])
@pytest.mark.parametrize("n", FRAME_COUNTS)
def test_fused_tail_still_equals_the_two_calls(engine, oracle, n, kind, layout, monkeypatch):
    """(d) on the batch's stereo streams (the one-launch tail takes batches of one channel count, without EightShort frames)"""
    import torch
    monkeypatch.setenv("SK_AAC_TAIL_ONE_LAUNCH", "1")
    per = batch(oracle, kind, n)
    streams = [s for s, ch in enumerate(CHANNELS) if ch == 2]
    ns, ch = len(streams), 2
    sids = [engine.open_stream(48000, ch) for _ in streams]
    order = frame_order(layout, n, streams)
    strides = (ch * 1024, ns * ch * 1024) if layout == "frame" else (n * ch * 1024, ch * 1024)
    packed = np.stack([per[s][0][f] for s, f in order])
    descs, nd = soundkit_amd.descs_from_arrays([sids[streams.index(s)] for s, f in order], ch, [per[s][1][f] for s, f in order],
                                               [per[s][2][f] for s, f in order])
    plan = engine.plan(descs, nd)
    d_coeffs = torch.from_numpy(packed).cuda()
    n_out = engine.downsample_out_frames(n * 1024)
    stride = (n_out + 7) // 8 * 8
    pcm16 = torch.zeros(d_coeffs.shape, dtype=torch.int16, device="cuda")
    want = torch.zeros((ns, stride, ch), dtype=torch.int16, device="cuda")
    got = torch.zeros_like(want)
    torch.cuda.synchronize()
    plan.run_s16_planar(d_coeffs, pcm16)
    assert engine.downsample_48k_16k_frames_s16_to_s16_dev(pcm16, strides[0], strides[1], ch, ns, n, want, stride) == n_out
    engine.synchronize()
    state_want = [engine.get_state(sid, ch) for sid in sids]
    for sid in sids:
        engine.reset_stream(sid)
    assert plan.run_tail_s16(d_coeffs, strides[0], ch, n, got, stride) == n_out
    engine.synchronize()
    assert torch.equal(got, want), int((got != want).sum())
    assert int(want.abs().max()) > 1000
    for sid, (d, sh) in zip(sids, state_want):
        d2, sh2 = engine.get_state(sid, ch)
        assert np.array_equal(d, d2) and np.array_equal(sh, sh2)
    plan.destroy()
    for sid in sids:
        engine.close_stream(sid)

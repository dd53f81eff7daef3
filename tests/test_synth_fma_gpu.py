"""The synthesis arithmetic after the vector-instruction diet (profiles/synth_valu_diet.md): one stage-1 twiddle W512^(lane k)
instead of two, pre-twiddle and window + overlap-add as fused multiply-adds, dft8's 1/sqrt2 folded into its last butterfly.
Every change drops a rounding step, so results move in the last bits; what defines them is unchanged -- the oracle within the
bounds of test_aac_synth_gpu.py, and the s16 form as the exact conversion of the kernel's own f32 result.

One plan of one mono and two stereo streams x 5 frames, frame-major: the mono channel finds no partner (one-channel kernel,
with its eight-short arm), one stereo stream is OnlyLong throughout (long-only pair kernel), the other walks
LongStart - EightShort - EightShort - LongStop - OnlyLong on both channels (pair kernel with the eight-short arm).  Both window
shapes occur as previous and as current shape, and every channel starts from a non-zero overlap.
"""
import numpy as np
import pytest

import soundkit_amd
from soundkit_amd import aac_lc
from test_aac_synth_gpu import RMS_TOL, rel_rms

pytestmark = pytest.mark.gpu

CHANNELS = [1, 2, 2]
N_FRAMES = 5
SEQUENCES = [[0, 1, 2, 3, 0], [0, 0, 0, 0, 0], [1, 2, 2, 3, 0]]  # per stream; both channels of a stream switch together
PREV_SHAPES = [[1], [0, 1], [1, 0]]


def fixed_pattern_inputs(oracle):
    """the four inputs of test_reference_fixed_pattern_and_seeds (dsp.rs:653-723)"""
    pat = [0.0, 1.0, -2.0, 0.5, -0.25, 4.0, -8.0, 0.125, -0.75]
    return [np.array([pat[i % 9] for i in range(1024)], np.float32)] + [oracle.seeded_spectrum(1024, s) for s in (0x12345678, 0xA5A50101, 0xDEADBEEF)]


@pytest.fixture(scope="module")
def batch(oracle):
    """spectra, windows, initial state and the oracle's PCM and final state of every stream: computed once, never changed"""
    rng = np.random.default_rng(0x5EED)
    per = []
    for s, ch in enumerate(CHANNELS):
        coeffs = np.empty((N_FRAMES, ch, 1024), np.float32)
        for f in range(N_FRAMES):
            for c in range(ch):
                coeffs[f, c] = oracle.seeded_spectrum(1024, 0x0D1E7 + 977 * s + 2 * f + c) * np.float32(9000.0)
        seqs = np.array([[q] * ch for q in SEQUENCES[s]], np.uint8)
        shapes = np.array([[(f + s + c) & 1 for c in range(ch)] for f in range(N_FRAMES)], np.uint8)
        delay0 = rng.uniform(-0.25, 0.25, (ch, 1024)).astype(np.float32)
        chans = [oracle.Channel() for _ in range(ch)]
        for c in range(ch):
            chans[c].set_state(delay0[c], PREV_SHAPES[s][c])
        want, chans = oracle.synthesize_stream(coeffs, seqs, shapes, chans)
        final = np.stack([c.delay for c in chans])
        for a in (coeffs, seqs, shapes, delay0, want, final):
            a.setflags(write=False)
        per.append((coeffs, seqs, shapes, delay0, want, final, [c.prev_shape for c in chans]))
    assert {int(q) for s in SEQUENCES for q in s} == {0, 1, 2, 3}
    return per


def test_f32_within_the_oracle_bounds_and_s16_is_its_exact_conversion(engine, oracle, batch):
    import torch
    streams = range(len(CHANNELS))
    sids = [engine.open_stream(48000, ch) for ch in CHANNELS]
    at, slot, frames = {}, 0, []
    for f in range(N_FRAMES):
        for s in streams:
            at[(s, f)] = slot
            slot += CHANNELS[s]
            frames.append((sids[s], CHANNELS[s], batch[s][1][f], batch[s][2][f]))
    descs, nd = soundkit_amd.make_descs(frames)
    plan = engine.plan(descs, nd)
    assert not plan.status.any(), plan.status
    host = np.zeros((slot, 1024), np.float32)
    for (s, f), a in at.items():
        host[a:a + CHANNELS[s]] = batch[s][0][f]
    d_coeffs = torch.from_numpy(host).cuda()

    def run(out16):
        for s in streams:
            engine.set_state(sids[s], batch[s][3], PREV_SHAPES[s])
        d_pcm = torch.zeros((slot, 1024), dtype=torch.int16 if out16 else torch.float32, device="cuda")
        torch.cuda.synchronize()
        if out16:
            plan.run_s16_planar(d_coeffs, d_pcm)
        else:
            plan.run_f32(d_coeffs, d_pcm)
        engine.synchronize()
        return d_pcm.cpu().numpy(), [engine.get_state(sids[s], CHANNELS[s]) for s in streams]

    f32, state32 = run(False)
    s16, state16 = run(True)
    plan.destroy()
    for sid in sids:
        engine.close_stream(sid)

    for s in streams:
        coeffs, seqs, shapes, delay0, want, final, final_shape = batch[s]
        mine = np.stack([f32[at[(s, f)]:at[(s, f)] + CHANNELS[s]] for f in range(N_FRAMES)])
        for f in range(N_FRAMES):
            for c in range(CHANNELS[s]):
                err = rel_rms(mine[f, c], want[f, c])
                print("stream %d frame %d ch %d seq %d: rel-rms %.3e max-abs %.3e" % (s, f, c, seqs[f, c], err, np.abs(mine[f, c] - want[f, c]).max()))
                assert err < RMS_TOL, (s, f, c)
        assert np.abs(mine - want).max() < 2e-6 * np.abs(want).max(), s
        # a first frame on a given overlap is test_every_sequence_and_shape_pair's case: its bound
        assert np.abs(mine[0] - want[0]).max() < 3e-7 * max(1.0, np.abs(want[0]).max()), s
        for c in range(CHANNELS[s]):
            assert rel_rms(state32[s][0][c], final[c]) < RMS_TOL, (s, c)
            assert state32[s][1][c] == final_shape[c], (s, c)
        # the s16 launch carries the same overlap, bit for bit
        assert np.array_equal(state16[s][0].view(np.int32), state32[s][0].view(np.int32)) and np.array_equal(state16[s][1], state32[s][1]), s
    # s16 = float_sample_to_i16 of the kernel's own f32 output
    assert np.array_equal(s16, oracle.pcm_convert("FLOAT_TO_I16_ROUND", f32.ravel()).reshape(-1, 1024))
    assert np.abs(s16.astype(np.int32)).max() > 1000  # far above the rounding step


def test_fixed_pattern_and_seeds_against_the_direct_form(engine, oracle):
    """test_reference_fixed_pattern_and_seeds' four inputs and its 4e-8; the relative RMS error of the four together is printed
    (profiles/synth_valu_diet.md records it for this arithmetic and for the one before)"""
    win = oracle.sine_window(2048)
    num = den = 0.0
    for x in fixed_pattern_inputs(oracle):
        sid = engine.open_stream(48000, 1)
        pcm, _ = aac_lc.synthesize_batch(engine, [sid], 1, x[None, None], [[0, 0]], [[0, 0]])
        delay, _ = engine.get_state(sid, 1)
        engine.close_stream(sid)
        direct = oracle.imdct_direct_f64(x)
        want = direct * win
        got = np.concatenate([pcm[0, 0], delay[0]]).astype(np.float64)
        num += np.sum((got - want) ** 2)
        den += np.sum(want ** 2)
        print("max-abs %.3e / %.3e" % (np.abs(pcm[0, 0] - want[:1024]).max(), np.abs(delay[0] - want[1024:]).max()))
        assert np.abs(pcm[0, 0] - direct[:1024] * win[:1024]).max() < 4.0e-8
        assert np.abs(delay[0] - direct[1024:] * win[1024:]).max() < 4.0e-8
    print("relative RMS error of the four inputs together: %.4e" % np.sqrt(num / den))

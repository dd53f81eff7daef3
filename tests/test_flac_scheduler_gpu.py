"""FLAC streams through the batch scheduler: found by their `fLaC` marker (a short prefix waits), read on the entropy threads, budgeted
in whole frames, decoded by the FLAC tick; one AudioData per frame, in stream order.  The reference's fixture and a dozen streams of
tests/flac_builder.py beside ADTS, MP3 and WAV streams equal FlacDecoder byte for byte at two frame budgets, on one and two lanes, fed
in 1 KiB pieces and whole; rate, depth and channel changes meet a raw PCM stream fed the decoded PCM; a stream with a frame the device
rejects, or one the framer rejects, ends alone with its text.  On the parent commit the first `fLaC` byte ends the stream in the ADTS
path."""
import os
import random
import threading
import time

import numpy as np
import pytest

import flac_builder as B
import flac_model as M
from soundkit_amd import pipeline
from soundkit_amd import engine as E
from test_pcm_pipeline_gpu import as_model, drain, read

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "flac", "A_Tusk_is_used_to_make_costly_gifts.flac")
KINDS = [{"type": "verbatim"}, {"type": "fixed", "order": 2, "params": "auto"},
         {"type": "lpc", "order": 4, "precision": 12, "shift": 11, "coefs": [2000, -900, 300, -50], "params": "auto"}]


def build(seed, bits, nch, rate, sizes, variable=False, assignment=None, scale=0.5, damage=None):
    """-> (stream bytes, [[channel][sample]] per frame)"""
    rng = random.Random(seed)
    lim = int((1 << (bits - 1)) * scale)
    blocks = [[[rng.randrange(-lim, lim) for _ in range(n)] for _ in range(nch)] for n in sizes]

    def specs(i, ch):
        out = [KINDS[(i + c) % 3 if len(ch[0]) >= 4 else 0] for c in range(len(ch))]
        if damage == i:
            out[0] = dict(KINDS[2], raw_shift=0x1F)  # a negative LPC shift: the framer passes it, the device rejects it
        return out
    data, _ = B.stream(blocks, bits, rate, specs, variable=variable, assignment=assignment)
    return data, blocks


def contract(samples, bits):
    if bits <= 16:
        return samples.astype("<i2").tobytes()
    return samples.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()


def decoder_frames(engine, data):
    """FlacDecoder on the whole stream -> (rate, channels, bits, the contract's bytes of all frames)"""
    from soundkit_amd import flac
    dec = flac.FlacDecoder(engine=engine)
    out, got = np.zeros(1 << 20, np.int32), []
    n = dec.decode_i32(data, out)
    while n:
        got.append(out[:n].copy())
        n = dec.decode_i32(b"", out)
    info = (dec.sample_rate(), dec.channels(), dec.bits_per_sample())
    dec.close()
    return info + (contract(np.concatenate(got), info[2]),)


def cut(data, n):
    return [data[at:at + n] for at in range(0, len(data), n)]


def feed(handles, chunk_lists):
    """every stream's chunks in turn, then its end; a stream that has ended with an error takes no more"""
    pos = [0] * len(handles)
    pending = set(range(len(handles)))
    while pending:
        for i in list(pending):
            try:
                if pos[i] >= len(chunk_lists[i]):
                    handles[i].finish()
                    pending.discard(i)
                else:
                    handles[i].send(chunk_lists[i][pos[i]])
                    pos[i] += 1
            except pipeline.DecodeError as e:
                if e.kind == "PipelineClosed":
                    pending.discard(i)
                else:
                    assert e.kind == "InputBufferFull", e
        time.sleep(0.0002)


def run(engine, streams, lanes=1, budget=0):
    """streams: (RawPcmFormat or None to detect, DecodeOptions, chunks) -> per stream its outputs"""
    sched = pipeline.BatchScheduler(engine, entropy_threads=4, max_streams=len(streams) + 4, lanes=lanes, max_stream_frames_per_tick=budget)
    try:
        handles = [sched.spawn_raw_pcm(f, o) if f is not None else sched.spawn(o) for f, o, _ in streams]
        lists = [c for _, _, c in streams]
        half = len(handles) // 2
        feeders = [threading.Thread(target=feed, args=(handles[:half], lists[:half])), threading.Thread(target=feed, args=(handles[half:], lists[half:]))]
        for t in feeders:
            t.start()
        outs = drain(handles)
        for t in feeders:
            t.join()
        for h in handles:
            h.cancel()
    finally:
        sched.close()
    return outs


@pytest.fixture(scope="module")
def flac_streams(engine):
    """the fixture and twelve builder streams -- both block strategies, mono / stereo / 6 channels, 16 / 24 bits -- each with what
    FlacDecoder makes of it and its frames' sizes in bytes"""
    out = []
    data = open(FIXTURE, "rb").read()
    out.append(("fixture", data, decoder_frames(engine, data), [2 * 1152] * 41 + [2 * 128]))
    k = 0
    for bits in (16, 24):
        for nch in (1, 2, 6):
            for variable in (False, True):
                sizes = [192, 50, 1152, 7, 576][:3 + k % 3] if not variable else [64, 1000, 33, 1, 400][:3 + k % 3]
                data, blocks = build(300 + k, bits, nch, 44100, sizes, variable=variable, assignment=(8, 9, 10)[k % 3] if nch == 2 else None)
                want = decoder_frames(engine, data)
                assert want[:3] == (44100, nch, bits) and want[3] == b"".join(M.contract_bytes({"bits_per_sample": bits, "block_size": len(ch[0])}, ch) for ch in blocks)
                out.append(("%d bits %d ch %s" % (bits, nch, "variable" if variable else "fixed"), data, want, [n * nch * M.width(bits) for n in sizes]))
                k += 1
    assert len(out) == 13
    return out


@pytest.fixture(scope="module")
def neighbours(engine):
    """an ADTS, an MP3 and a WAV stream, and what the scheduler makes of them alone"""
    chunks = [cut(read("aac/aac-stereo-48k.adts"), 4096), cut(read("mp3/stereo16k_A_Tusk_encoded.mp3")[:576 * 24], 3000), cut(read("wav_24_A_Tusk.wav"), 50000)]
    opts = [pipeline.DecodeOptions(), pipeline.DecodeOptions(), pipeline.DecodeOptions(output_bits_per_sample=16)]
    streams = [(None, o, c) for o, c in zip(opts, chunks)]
    alone = [as_model(o) for o in run(engine, streams)]
    assert all(err is None and got for got, err in alone)
    return streams, [b"".join(g[5] for g in got) for got, _ in alone]


@pytest.mark.parametrize("budget, lanes, piece", [(3, 1, 1024), (64, 2, None), (3, 2, None), (64, 1, 1024)])
def test_flac_beside_other_codecs_equals_the_decoder(engine, flac_streams, neighbours, budget, lanes, piece):
    other, other_want = neighbours
    streams = []
    for i, (name, data, want, sizes) in enumerate(flac_streams):
        streams.append((None, pipeline.DecodeOptions(), cut(data, piece) if piece else [data]))
        if i % 5 == 0:
            streams.append(other[(i // 5) % 3])
    outs = run(engine, streams, lanes=lanes, budget=budget)
    k = 0
    for i, (name, data, want, sizes) in enumerate(flac_streams):
        got, err = as_model(outs[k])
        k += 1
        assert err is None, (name, err)
        assert [len(g[5]) for g in got] == sizes, name  # one AudioData per frame, in stream order
        assert all(g[:5] == (want[2], want[1], want[0], False, False) for g in got), name
        assert b"".join(g[5] for g in got) == want[3], name
        if i % 5 == 0:
            got, err = as_model(outs[k])
            assert err is None and b"".join(g[5] for g in got) == other_want[(i // 5) % 3]
            k += 1


def test_a_marker_that_arrives_byte_by_byte_is_waited_for(engine, flac_streams):
    name, data, want, sizes = flac_streams[1]
    outs = run(engine, [(None, pipeline.DecodeOptions(), [data[i:i + 1] for i in range(8)] + [data[8:]])])
    got, err = as_model(outs[0])
    assert err is None and [len(g[5]) for g in got] == sizes and b"".join(g[5] for g in got) == want[3]


def pcm_format(rate, nch, bits):
    return pipeline.RawPcmFormat(rate, nch, {16: E.FMT_S16LE, 24: E.FMT_S24LE, 32: E.FMT_S32LE}[bits])


def test_rate_depth_and_channel_changes_meet_the_pcm_path(engine, flac_streams):
    """the fixture to 8 kHz, a 48 kHz stereo 24-bit stream to 16 kHz mono s16, and 24 -> 16 bits without a rate change (the exact path):
    the same bytes as a raw PCM stream that is fed the decoded PCM"""
    fixture, fixture_want = flac_streams[0][1], flac_streams[0][2]
    wide, _ = build(400, 24, 2, 48000, [4096, 4096, 1000, 4096, 333], scale=0.7, assignment=8)
    wide_want = decoder_frames(engine, wide)
    deep, deep_blocks = build(401, 24, 1, 16000, [1152, 1152, 100], scale=0.9)
    deep_want = decoder_frames(engine, deep)
    deep_pcm = [M.contract_bytes({"bits_per_sample": 24, "block_size": len(ch[0])}, ch) for ch in deep_blocks]
    to8k, to16k, to16 = pipeline.DecodeOptions(16, 8000, None), pipeline.DecodeOptions(16, 16000, 1), pipeline.DecodeOptions(output_bits_per_sample=16)
    streams = [(None, to8k, cut(fixture, 1024)), (pcm_format(16000, 1, 16), to8k, cut(fixture_want[3], 5000)),
               (None, to16k, [wide]), (pcm_format(48000, 2, 24), to16k, cut(wide_want[3], 6 * 4000)),
               (None, to16, cut(deep, 700)), (pcm_format(16000, 1, 24), to16, deep_pcm)]
    outs = [as_model(o) for o in run(engine, streams, budget=4)]
    assert all(err is None for _, err in outs)
    for k, fields in ((0, (16, 1, 8000)), (2, (16, 1, 16000)), (4, (16, 1, 16000))):
        got, want = outs[k][0], outs[k + 1][0]
        assert got and all(g[:3] == fields for g in got)
        assert b"".join(g[5] for g in got) == b"".join(w[5] for w in want), k
    assert len(b"".join(g[5] for g in outs[0][0])) > 2 * 23000 and len(b"".join(g[5] for g in outs[2][0])) > 2 * 4000
    # without a rate change the outputs stay one per frame
    assert [len(g[5]) for g in outs[4][0]] == [2 * 1152, 2 * 1152, 200] and [g[5] for g in outs[4][0]] == [w[5] for w in outs[5][0]]


def test_a_depth_the_pcm_path_does_not_take_is_refused_with_its_text(engine):
    data, _ = build(410, 20, 1, 44100, [64, 64])
    outs = run(engine, [(None, pipeline.DecodeOptions(output_bits_per_sample=16), [data])])
    got, err = as_model(outs[0])
    assert got == [] and err == "Decoding failed: Output conversion failed: PCM data is unsupported or contains a partial frame"


def test_rejected_streams_end_with_their_text_and_the_neighbours_finish(engine, flac_streams, neighbours):
    other, other_want = neighbours
    bad_device, blocks = build(420, 16, 2, 44100, [100, 60, 80], damage=1)
    first = M.contract_bytes({"bits_per_sample": 16, "block_size": 100}, blocks[0])
    name, good, want, sizes = flac_streams[3]
    flipped = bytearray(flac_streams[0][1])
    flipped[20000] ^= 0x08  # inside a frame: no span satisfies the CRC-16 any more
    truncated = flac_streams[0][1][:-30]
    outs = run(engine, [(None, pipeline.DecodeOptions(), [bad_device]), (None, pipeline.DecodeOptions(), [good]), other[0],
                        (None, pipeline.DecodeOptions(), cut(bytes(flipped), 4096)), (None, pipeline.DecodeOptions(), [truncated]),
                        (None, pipeline.DecodeOptions(16, None, 1), [bad_device]), (None, pipeline.DecodeOptions(), cut(good, 100))])
    got, err = as_model(outs[0])
    assert [g[5] for g in got] == [first] and err.startswith("Decoding failed: FLAC frame rejected"), err
    for k in (1, 6):
        got, err = as_model(outs[k])
        assert err is None and b"".join(g[5] for g in got) == want[3]
    got, err = as_model(outs[2])
    assert err is None and b"".join(g[5] for g in got) == other_want[0]
    got, err = as_model(outs[3])
    assert err.startswith("Decoding failed: FLAC frame") and "CRC" in err and len(got) < 42
    assert flac_streams[0][2][3].startswith(b"".join(g[5] for g in got))  # what came out in front of the damage is exact
    got, err = as_model(outs[4])
    assert err.startswith("Decoding failed: truncated FLAC stream") and len(got) == 41
    got, err = as_model(outs[5])  # behind a downmix the damaged tick gives nothing
    assert err.startswith("Decoding failed: FLAC frame rejected")

"""Compressed WAV through the scheduler (DecodePipeline / BatchScheduler.spawn()): the fixtures of tests/golden/wav_coded whole and in
ragged chunks, beside an ADTS stream and a PCM WAV, on one and two lanes.  The concatenated output is the recording, there is one
AudioData per piece the worker's walk gives (detection gathering as tests/pcm_worker_model.py models it, the walker's pieces from
WavCodedReader), the output options meet the CPU chain, a bad block or a refused header ends its stream alone behind the good units,
and the PCM WAV beside them is what tests/test_pcm_pipeline_gpu.py expects of it: its 16-bit twin, bit for bit."""
import functools
import os
import struct
import time
import wave

import numpy as np
import pytest

import pcm_worker_model as W
import wav_adpcm_model as M
import wav_coded_builder as B

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
DIR = os.path.join(GOLD, "wav_coded")
ADPCM = ["ima_mono_8k", "ima_stereo", "ms_mono_8k", "ms_stereo"]
COEF3 = [(256, 0), (460, -208), (392, -232)]


def read(*path):
    return open(os.path.join(GOLD, *path), "rb").read()


def recording(name):
    if name in ADPCM:
        return read("wav_coded", name + ".decoded.s16le")
    with wave.open(os.path.join(GOLD, "aiff", "g711_%s.decoded.wav" % name[:4])) as w:
        return w.readframes(w.getnframes())


class Walk:
    """the coded walker in the place of the model's WavModel, for pcm_worker_model._wav_pieces"""

    def __init__(self):
        from soundkit_amd import pcm_stream
        self.rd = pcm_stream.WavCodedReader()

    def add(self, data):
        got = self.rd.add(data)
        return got[1] if got else None


def worker_pieces(chunks):
    """-> (info, [the pieces the worker's walk hands on], the walker's text or None)"""
    walk, pieces, err = Walk(), [], None
    try:
        W._wav_pieces(walk, pieces, bytearray(), False, chunks)
    except ValueError as e:
        err = str(e)
    return walk.rd.info(), pieces, err


def model_outputs(info, pieces):
    """what every piece decodes to: s16, cut to the fact count; a piece behind the cap gives nothing.  -> ([bytes], text of a bad block)"""
    import g72x_model
    out, left, ch = [], info["total_frames"], info["channels"]
    for p in pieces:
        if info["tag"] in (6, 7):
            out.append(g72x_model.g711_decode(p, g72x_model.ULAW if info["tag"] == 7 else g72x_model.ALAW).astype("<i2").tobytes())
            continue
        align = info["block_align"]
        p = p[:-(-left // info["frames_per_block"]) * align]
        pcm, status = M.decode(info["tag"], ch, align, p, info["coef"])
        if any(status):
            from soundkit_amd import pcm_stream
            k = [i for i, s in enumerate(status) if s][0]
            pcm = pcm[:k * info["frames_per_block"] * ch]
            if pcm.size:
                out.append(pcm.astype("<i2").tobytes())
            return out, pcm_stream.wav_bad_block_text(info, p[k * align:(k + 1) * align])
        pcm = pcm.astype("<i2").tobytes()[:left * ch * 2]
        left -= len(pcm) // (ch * 2)
        if pcm:
            out.append(pcm)
    return out, None


def through_scheduler(engine, streams, lanes=1):
    """streams: [(DecodeOptions or None, chunks)] -> per stream the AudioData, an error last where the stream ended with one"""
    from soundkit_amd import pipeline
    sched = pipeline.BatchScheduler(engine, entropy_threads=4, max_streams=len(streams) + 4, lanes=lanes)
    outs = [[] for _ in streams]
    try:
        handles = [sched.spawn(o) if o is not None else sched.spawn() for o, _ in streams]
        pos, t0 = [0] * len(streams), time.time()
        live = set(range(len(streams)))
        while live:
            assert time.time() - t0 < 120, "scheduler stalled"
            for i in list(live):
                chunks = streams[i][1]
                try:
                    if pos[i] < len(chunks):
                        handles[i].send(chunks[pos[i]])
                        pos[i] += 1
                    elif pos[i] == len(chunks):
                        handles[i].finish()
                        pos[i] += 1
                except pipeline.DecodeError as e:
                    if e.kind != "InputBufferFull":  # the stream has ended with an error: nothing more is sent
                        pos[i] = len(chunks) + 1
                got = handles[i].try_recv()
                while got is not None:
                    outs[i].append(got)
                    got = handles[i].try_recv()
                if pos[i] > len(chunks) and handles[i].ended():
                    got = handles[i].try_recv()
                    while got is not None:
                        outs[i].append(got)
                        got = handles[i].try_recv()
                    live.discard(i)
        for h in handles:
            h.cancel()
    finally:
        sched.close()
    return outs


def split(outs):
    err = None
    if outs and isinstance(outs[-1], Exception):
        err, outs = str(outs[-1]), outs[:-1]
    assert not any(isinstance(a, Exception) for a in outs)
    return outs, err


@functools.lru_cache(maxsize=None)
def big_files():
    """files long enough for more than one piece behind the detection buffer: 40 blocks of 1024 bytes each"""
    rng = np.random.default_rng(9)
    t = np.arange(40 * 2041 - 700)[:, None]
    mono = np.clip(8000 * np.sin(2 * np.pi * t * 190.0 / 8000) + rng.normal(0, 500, t.shape), -32768, 32767).astype(np.int16)
    return {"ima_long": B.ima_wav(mono[:40 * 2041 - 700], 1024), "ms_long": B.ms_wav(mono[:40 * 2036 - 700], 1024, coef=COEF3)}


@gpu
@pytest.mark.parametrize("lanes", [1, 2])
def test_fixtures_beside_an_adts_stream_and_a_pcm_wav(engine, lanes):
    from soundkit_amd import pipeline
    rng = np.random.default_rng(50 + lanes)
    files = {n: read("wav_coded", n + ".wav") for n in ADPCM}
    files.update({"ulaw": read("wav_coded", "ulaw_A_Tusk.wav"), "alaw": read("wav_coded", "alaw_A_Tusk.wav")})
    files.update(big_files())
    names = sorted(files)
    streams, label = [], []
    for n in names:
        for hi in (None, 3000, 40):
            if hi == 40 and len(files[n]) > 10000:
                continue
            chunks = [files[n]] if hi is None else W.ragged(files[n], rng, 1, hi)
            streams.append((None, chunks))
            label.append((n, hi))
    n_coded = len(streams)
    streams.append((None, W.ragged(read("aac", "aac-stereo-48k.adts"), rng, 1, 4000)))
    streams.append((pipeline.DecodeOptions(output_bits_per_sample=16), W.ragged(read("wav_24_A_Tusk.wav"), rng, 1, 40000)))
    outs = through_scheduler(engine, streams, lanes)
    for k in range(n_coded):
        n, hi = label[k]
        got, err = split(outs[k])
        info, pieces, walk_err = worker_pieces(streams[k][1])
        want, bad = model_outputs(info, pieces)
        assert err is None and walk_err is None and bad is None, (n, hi, err)
        assert [a.data.tobytes() for a in got] == want, (n, hi)  # one AudioData per productive piece, each the model's
        assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, info["channels"], info["sample_rate"]) for a in got)
        if n in ADPCM or n in ("ulaw", "alaw"):
            assert b"".join(want) == recording(n), n
        else:
            assert b"".join(want) == B.model_decode_file(files[n]).astype("<i2").tobytes() and (hi is None or len(want) > 2)
    adts, err = split(outs[n_coded])
    assert err is None and len(adts) == 48
    pcm, err = split(outs[n_coded + 1])
    assert err is None and b"".join(a.data.tobytes() for a in pcm) == read("linear16_A_Tusk.s16le")
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 16000) for a in pcm)


def lsb_check(mine, want, label):
    """tests/test_pcm_pipeline_gpu.py lsb_check: one step, on at most 1 % of the samples"""
    mine, want = np.frombuffer(mine, "<i2").astype(np.int32), np.frombuffer(want, "<i2").astype(np.int32)
    assert mine.size == want.size, (label, mine.size, want.size)
    d = np.abs(mine - want)
    print("\n%s: worst |d| %d, share of samples off by one %.5f of %d" % (label, d.max(), (d > 0).mean(), d.size))
    assert d.max() <= 1 and (d > 0).mean() <= 0.01, (label, int(d.max()), float((d > 0).mean()))


@gpu
def test_output_options_meet_the_cpu_chain(engine, oracle):
    """8 -> 16 kHz mono s16 through the resampler rows (within lsb_check's bound), 24 bits and a downmix without a rate change (exact)"""
    from soundkit_amd import pipeline
    rng = np.random.default_rng(77)
    files = dict(big_files(), ulaw=read("wav_coded", "ulaw_A_Tusk.wav"), ms_stereo=read("wav_coded", "ms_stereo.wav"), ima_stereo=read("wav_coded", "ima_stereo.wav"))
    cases = [("ima_long", 16, 16000, None), ("ms_long", 16, 16000, None), ("ulaw", 16, 16000, None), ("ulaw", 24, None, None), ("ms_stereo", 24, None, None),
             ("ima_stereo", None, None, 1), ("ima_long", 32, None, None)]
    streams = [(pipeline.DecodeOptions(bits, rate, ch), W.ragged(files[n], rng, 1, 9000)) for n, bits, rate, ch in cases]
    outs = through_scheduler(engine, streams)
    for (n, bits, rate, ch), (_, chunks), o in zip(cases, streams, outs):
        got, err = split(o)
        info, pieces, _ = worker_pieces(chunks)
        pcm, _ = model_outputs(info, pieces)
        stage = W.OutputStage(oracle, info["sample_rate"], info["channels"], 16, False, False, bits, rate, ch)
        cpu = [x for p in pcm for x in stage.piece(p)] + stage.flush()
        assert err is None, (n, err)
        assert [(a.bits_per_sample, a.channel_count, a.sampling_rate, a.data.size) for a in got] == [(x[0], x[1], x[2], len(x[5])) for x in cpu], n
        mine, want = b"".join(a.data.tobytes() for a in got), b"".join(x[5] for x in cpu)
        if rate is None:
            assert mine == want, n
        else:
            lsb_check(mine, want, n)


@gpu
def test_a_bad_block_or_a_refused_header_ends_its_stream_alone_behind_the_good_units(engine):
    rng = np.random.default_rng(3)
    files = dict(big_files())
    ima, ms = bytearray(files["ima_long"]), bytearray(files["ms_long"])
    at = ima.index(b"data") + 8
    ima[at + 13 * 1024 + 2] = 91          # block 13: behind the detection buffer's piece
    ms[ms.index(b"data") + 8 + 3 * 1024] = 3   # block 3, with three coefficient sets: inside the first piece
    three = B.wav(B.fmt_payload(0x11, 3, 8000, 36, 4, b""), bytes(360))
    cut = files["ima_long"][:at + 13 * 1024 + 100]  # a data chunk of 13 blocks and 100 bytes; the last send brings no whole block
    cut = cut[:at - 4] + struct.pack("<I", 13 * 1024 + 100) + cut[at:]
    streams = [(None, W.ragged(bytes(ima), rng, 500, 3000)), (None, [bytes(ms)]), (None, [three]), (None, [cut[:9000], cut[9000:-50], cut[-50:]]),
               (None, [files["ms_long"]])]
    outs = through_scheduler(engine, streams)
    texts = ["Decoding failed: WAV IMA ADPCM block step index 91 exceeds 88", "Decoding failed: WAV MS ADPCM block predictor 3 exceeds the 3 coefficient sets",
             "Decoding failed: WAV ADPCM with 3 channels is not built: mono and stereo are", "Decoding failed: WAV data chunk is not block-aligned", None]
    for k, (text, (_, chunks), o) in enumerate(zip(texts, streams, outs)):
        got, err = split(o)
        info, pieces, walk_err = worker_pieces(chunks)
        want, bad = model_outputs(info, pieces) if info["tag"] else ([], None)
        assert (bad or walk_err) == (text[len("Decoding failed: "):] if text else None), k
        if text is None:
            assert err is None
        else:
            assert err is not None and text in err, (k, err)
        assert [a.data.tobytes() for a in got] == want, k
    assert len(split(outs[0])[0]) >= 2 and len(split(outs[1])[0]) == 1 and sum(a.data.size for a in split(outs[1])[0]) == 3 * 2036 * 2
    assert len(split(outs[3])[0]) == 2 and sum(a.data.size for a in split(outs[3])[0]) == 13 * 2041 * 2

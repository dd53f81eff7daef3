"""soundkit_amd.ts.decode_file on the device: every comparison is bit for bit against a decoder that was there before the container --
the ADTS decoder and Mp3Decoder on the golden elementary streams, the scheduler's raw PCM stream on the Blu-ray LPCM payloads -- so the
container adds nothing and loses nothing, with no options and to 16 kHz mono s16."""
import numpy as np
import pytest

import ts_cases as CASES
import ts_model as M
from soundkit_amd import alac, pipeline, ts
from soundkit_amd.audio_types import Endianness
from soundkit_amd.engine import FMT_S16BE

pytestmark = pytest.mark.gpu
OPTIONS = pipeline.DecodeOptions(16, 16000, 1)


def joined(audios):
    return b"".join(a.data.tobytes() for a in audios)


def adts_samples(engine, data):
    from soundkit_amd.aac import AacDecoder, decode_i16_with_drain
    dec, out = AacDecoder(engine), np.zeros(64 * 1024, np.int16)
    got = [s for at in range(0, len(data), 4096) for s in decode_i16_with_drain(dec, data[at:at + 4096], out)]
    dec.close()
    return np.concatenate(got)


def mpa_samples(engine, data):
    from soundkit_amd.mp3 import Mp3Decoder
    dec, out, got = Mp3Decoder(engine=engine), np.zeros(1 << 17, np.int16), []
    n = dec.decode_i16(data, out)
    while n:
        got.append(out[:n].copy())
        n = dec.decode_i16(b"", out)
    dec.close()
    return np.concatenate(got)


@pytest.fixture(scope="module")
def elementary(engine):
    """the golden elementary streams through the decoders that were there before the container, once"""
    return {"aac": adts_samples(engine, CASES.ADTS), "mp2": mpa_samples(engine, CASES.MP2)}


@pytest.fixture(scope="module")
def sched(engine):
    s = pipeline.BatchScheduler(engine, entropy_threads=2, max_streams=4)
    yield s
    s.close()


@pytest.mark.parametrize("name", ["aac.ts", "aac.m2ts", "mp2.ts"])
def test_a_fixture_decodes_to_what_its_elementary_stream_decodes_to(engine, sched, elementary, name):
    want = elementary[name[:3]]
    assert want.size == (48 * 1024 if name.startswith("aac") else 42 * 1152) * 2
    config, got = ts.decode_file(CASES.fixture(name), engine=engine)
    assert (config.codec, config.sample_rate, config.channels) == ("aac" if name.startswith("aac") else "mp2", 48000, 2)
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 2, 48000) for a in got)
    assert joined(got) == want.astype("<i2").tobytes()
    if name.startswith("aac"):
        assert len(got) == 48  # one AudioData per access unit, as the reference hands them out
    config, got = ts.decode_file(CASES.fixture(name), OPTIONS, scheduler=sched, engine=engine)
    twin = alac.output_stage([want.astype("<i2").tobytes()], 48000, 2, 16, OPTIONS, sched)
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 16000) for a in got)
    assert joined(got) == joined(twin) and len(joined(got)) > 2 * 15000


def test_the_lpcm_fixture_is_its_payload_and_converts_like_raw_pcm(engine, sched):
    data = CASES.fixture("lpcm.m2ts")
    payloads = [e["data"] for kind, e in M.demux(data)[0] if kind == "packet"]
    config, got = ts.decode_file(data, engine=engine)
    assert (config.codec, config.bits_per_sample, config.sample_rate, config.channels) == ("pcm", 16, 48000, 2)
    assert [a.data.tobytes() for a in got] == payloads and len(got) == 20
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate, a.endianness) == (16, 2, 48000, Endianness.BigEndian) for a in got)
    config, got = ts.decode_file(data, OPTIONS, scheduler=sched, engine=engine)
    h = sched.spawn_raw_pcm(pipeline.RawPcmFormat(48000, 2, FMT_S16BE), OPTIONS)
    for p in payloads + [b""]:
        h.send(p)
    twin = []
    while True:
        a = h.recv(60000)
        if a is None:
            break
        assert not isinstance(a, Exception), a
        twin.append(a)
    h.cancel()
    assert all((a.bits_per_sample, a.channel_count, a.sampling_rate) == (16, 1, 16000) for a in got)
    assert joined(got) == joined(twin) and len(joined(got)) > 2 * 1500

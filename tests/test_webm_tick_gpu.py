"""skip_frames in the Vorbis tick (sk_vorbis_tick_packet, Engine.tick_run_vorbis): that many of a packet's frames are dropped at its
front, before keep_frames applies to what is left.  With skip on some packets the tick gives the skip = 0 output with those frames
removed -- on the direct route as bytes, behind a rate change and a downmix as what sk_tick_run_pcm makes of the trimmed s16 --
whichever way the packets are dealt out over ticks.  Shapes: the two fixtures' streams, a dozen packets each."""
import pytest

import vorbis_cases as CASES

pytestmark = pytest.mark.gpu

NAMES = ["ogg", "webm"]  # 8 kHz mono, one block size; 44.1 kHz stereo, two
N = 12
# per stream and packet: (skip_frames, keep_frames); packet 0 yields nothing whatever is asked of it
ALL = 0xffffffff
TRIMS = {
    "ogg": [(5, ALL), (0, ALL), (100, ALL), (0, ALL), (255, ALL), (256, ALL), (0, ALL), (1000, ALL), (40, 100), (40, 216), (40, 217), (0, 128)],
    "webm": [(0, ALL), (1, ALL), (0, ALL), (63, ALL), (0, ALL), (ALL, ALL), (0, ALL), (7, 9), (7, 0), (0, ALL), (3, ALL), (2, 1)],
}


def case(name):
    return next(c for c in CASES.all_cases() if c.name == name)


@pytest.fixture(scope="module")
def setups():
    from soundkit_amd import vorbis
    return {n: vorbis.Setup(vorbis.parse_ident(case(n).headers[0]), case(n).headers[2]) for n in NAMES}


@pytest.fixture(scope="module")
def untrimmed(engine, setups):
    """the decode call's s16 of each stream's first dozen packets, per packet"""
    from soundkit_amd import vorbis
    return {n: [pcm.astype("<i2").tobytes() for _, pcm in engine.vorbis_decode_packets([(vorbis.StreamState(setups[n]), case(n).packets[:N])])[0]]
            for n in NAMES}


def trimmed(untrimmed, name):
    """what skip and keep leave of every packet: the yardstick, cut out of the skip = 0 decode on the host"""
    width = 2 * case(name).ident["channels"]
    return [b[min(skip, len(b) // width) * width:][:keep * width] for b, (skip, keep) in zip(untrimmed[name], TRIMS[name])]


def deal(engine, setups, deals, entry, flush=False):
    """the NAMES streams over the ticks of `deals`, with TRIMS -> [records per stream]"""
    from soundkit_amd import vorbis
    states = [vorbis.StreamState(setups[n]) for n in NAMES]
    at, out = [0] * len(NAMES), [[] for _ in NAMES]
    for t, d in enumerate(deals):
        table, packets, skip, keep = [], [], [], []
        for i, n in enumerate(NAMES):
            table.append(dict(entry(i), state=states[i], n_units=d[i], flush=int(flush and t + 1 == len(deals))))
            packets += case(n).packets[at[i]:at[i] + d[i]]
            skip += [s for s, _ in TRIMS[n][at[i]:at[i] + d[i]]]
            keep += [k for _, k in TRIMS[n][at[i]:at[i] + d[i]]]
            at[i] += d[i]
        recs, status = engine.tick_run_vorbis(table, packets, skip_frames=skip, keep_frames=keep)
        assert not any(status)
        for r in recs:
            assert r[1] == 0
            out[r[0]].append(r)
    assert at == [N] * len(NAMES)
    return out


def plain(i):
    return {"out_bits": 16, "out_channels": case(NAMES[i]).ident["channels"]}


def test_the_yardstick_has_every_case(untrimmed):
    assert [len(b) // 2 for b in untrimmed["ogg"]] == [0] + [256] * 11
    kept = [len(b) // 2 for b in trimmed(untrimmed, "ogg")]
    assert kept == [0, 256, 156, 256, 1, 0, 256, 0, 100, 216, 216, 128]  # skip >= frames: nothing; skip and keep on one packet
    full, kept = [len(b) // 4 for b in untrimmed["webm"]], [len(b) // 4 for b in trimmed(untrimmed, "webm")]
    assert full[0] == 0 and len(set(full[1:])) > 1 and min(full[1:]) >= 64  # both block sizes are among them
    assert kept[5] == 0 and kept[8] == 0 and kept[7] == 9 and kept[11] == 1 and kept[1] == full[1] - 1


@pytest.mark.parametrize("deals", [[[N, N]], [[4, 5], [4, 1], [4, 6]], [[1, 1]] * N], ids=["one tick", "three ticks", "a packet a tick"])
def test_direct_route_is_the_untrimmed_output_with_those_frames_removed(engine, setups, untrimmed, deals):
    got = deal(engine, setups, deals, plain)
    for name, recs in zip(NAMES, got):
        ch = case(name).ident["channels"]
        want = [b for b in trimmed(untrimmed, name) if b]  # a packet of which nothing is left yields no output
        assert [(r[2], r[3], r[4], r[5]) for r in recs] == [(len(b) // (2 * ch), ch, 16, b) for b in want], name


def test_no_trim_is_what_it_was(engine, setups, untrimmed):
    from soundkit_amd import vorbis
    for name in NAMES:
        st = vorbis.StreamState(setups[name])
        recs, status = engine.tick_run_vorbis([dict(plain(NAMES.index(name)), state=st, n_units=N)], case(name).packets[:N])
        assert not any(status) and [r[5] for r in recs] == [b for b in untrimmed[name] if b]
        st = vorbis.StreamState(setups[name])
        again, _ = engine.tick_run_vorbis([dict(plain(NAMES.index(name)), state=st, n_units=N)], case(name).packets[:N], skip_frames=[0] * N)
        assert again == recs


@pytest.mark.parametrize("deals", [[[N, N]], [[4, 5], [4, 1], [4, 6]]], ids=["one tick", "three ticks"])
def test_behind_a_rate_change_and_a_downmix_it_is_the_pcm_tick_on_the_trimmed_s16(engine, setups, untrimmed, deals):
    """8 -> 16 kHz mono and 44.1 -> 16 kHz stereo to mono, the resampler flushed with the last tick"""
    import soundkit_amd.engine as E
    rates = [(8000, 16000), (44100, 16000)]

    def run(kind):
        sids = []
        for name, (rate, out_rate) in zip(NAMES, rates):
            sids.append(engine.open_stream(rate, case(name).ident["channels"]))
            engine.resampler_open(sids[-1], rate, out_rate)
        try:
            if kind == "vorbis":
                recs = deal(engine, setups, deals, lambda i: {"out_bits": 16, "out_channels": 1, "stream": sids[i], "resample": 1}, flush=True)
                return [b"".join(r[5] for r in rs) for rs in recs]
            units = [[b for b in trimmed(untrimmed, n) if b] for n in NAMES]
            rows = [{"format": E.FMT_S16LE, "channels": case(n).ident["channels"], "out_bits": 16, "out_channels": 1, "stream": sids[i], "resample": 1, "flush": 1,
                     "n_units": len(units[i])} for i, n in enumerate(NAMES)]
            out = [b"", b""]
            for r in engine.tick_run_pcm(rows, units[0] + units[1]):
                assert r[1] == 0
                out[r[0]] += r[5]
            return out
        finally:
            for sid in sids:
                engine.resampler_close(sid)
                engine.close_stream(sid)

    want = run("pcm")
    assert len(want[0]) > 2 * 2500 and len(want[1]) > 2 * 500  # 1 585 frames at twice the rate; 11 packets of at least 121 frames at a third
    assert run("vorbis") == want

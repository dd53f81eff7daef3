"""Every stream family in one scheduler round: the main tick's ADTS, MP3 and MP2 streams and the six PCM-family ticks behind it (AIFF,
FLAC, ALAC, telephony, GSM, PCM) share the rounds of one BatchScheduler -- one staged input blob, one output buffer, one record array,
one delivery pass (csrc/pipeline.cpp: claim_tick_row, follow_on_bound, follow_on_tick, submit_body, deliver_body, lane_spawn).

The streams are the table of tests/family_rounds.py (tests/test_family_rounds_cpu.py holds it to the recordings).  Expected values never
come from the mixed run:
* a PCM-family stream with default options: the model's bytes record by record, the reference's recording concatenated, the shape of
  every AudioData;
* the same behind output options: what raw PCM streams make of the model's samples, sent in the same pieces, in a BatchScheduler that
  holds nothing else (the path tests/test_pcm_pipeline_gpu.py pins to the CPU chain);
* an ADTS, MP3 or MP2 stream: the bytes it gives alone in a scheduler of its own with the same front end, budget and lanes.
All comparisons are bit for bit.

A round is shared when `ticks` stays below what a run without a shared round needs (family_rounds.rounds_without_sharing); the counts
seen are in profiles/scheduler_pcm_family.md."""
import threading
import time

import pytest

import family_rounds as T
from soundkit_amd import SoundkitError, pipeline
from test_flac_scheduler_gpu import feed
from test_pcm_pipeline_gpu import drain

pytestmark = pytest.mark.gpu

TICK_WAIT_US = 20000  # a round gathers every stream that has input
SK_ERR_CAPACITY = -7


def options_of(s):
    return pipeline.DecodeOptions(*s.options) if s.options else None


def spawn(sched, s):
    k, o = s.spawn, options_of(s)
    if k[0] == "auto":
        return sched.spawn(o)
    if k[0] == "aiff":
        return sched.spawn_aiff(o)
    if k[0] == "alac":
        return sched.spawn_alac_packets(k[1], o)
    if k[0] == "g711":
        return sched.spawn_g711(k[1], k[2], k[3], o)
    if k[0] == "g722":
        return sched.spawn_g722(o)
    if k[0] == "g726":
        return sched.spawn_g726(k[1], k[2], o)
    if k[0] == "gsm":
        return sched.spawn_gsm(k[1], o)
    assert k[0] == "raw", k
    return sched.spawn_raw_pcm(pipeline.RawPcmFormat(k[1], k[2], k[3]), o)


def feed_and_drain(handles, lists, take=drain, deadline_s=60):
    half = len(handles) // 2
    feeders = [threading.Thread(target=feed, args=(handles[:half], lists[:half])), threading.Thread(target=feed, args=(handles[half:], lists[half:]))]
    for t in feeders:
        t.start()
    try:
        return take(handles, deadline_s)
    finally:
        for t in feeders:
            t.join()


def run(engine, streams, take=drain, **config):
    """-> (per stream its outputs, the scheduler's stats)"""
    config.setdefault("max_streams", len(streams) + 4)
    sched = pipeline.BatchScheduler(engine, entropy_threads=4, **config)
    try:
        handles = [spawn(sched, s) for s in streams]
        outs = feed_and_drain(handles, [s.sends for s in streams], take)
        stats = sched.stats()
        for h in handles:
            h.cancel()
    finally:
        sched.close()
    return outs, stats


def audio(outs):
    assert all(not isinstance(o, pipeline.DecodeError) for o in outs), [str(o) for o in outs if isinstance(o, pipeline.DecodeError)]
    return b"".join(o.data.tobytes() for o in outs)


def shapes(outs):
    return {(o.bits_per_sample, o.channel_count, o.sampling_rate) for o in outs}


# ---- expected values ------------------------------------------------------------------------------------------------------------------
_RAW, _ALONE = {}, {}


def raw_references(engine, streams, n_units=None):
    """what raw PCM streams make of the model's first n_units units (all of them by default) under each stream's options, sent in the
    same pieces, in a scheduler that holds nothing else -> per stream (bytes, the set of AudioData shapes); each computed once"""
    n_units = n_units or [None] * len(streams)
    keys = [(s.name, s.options, n) for s, n in zip(streams, n_units)]
    todo = [i for i, k in enumerate(keys) if k not in _RAW and k not in keys[:i]]
    if todo:
        raws = []
        for i in todo:
            s = streams[i]
            bits, channels, rate = s.shape
            raws.append(T.Stream(s.name, "pcm", ("raw", rate, channels, s.fmt), s.model()[0][:n_units[i]], options=s.options))
        outs, stats = run(engine, raws)
        assert stats["errors"] == 0
        for i, o in zip(todo, outs):
            _RAW[keys[i]] = (audio(o), shapes(o))
    return [_RAW[k] for k in keys]


def alone(engine, s, **config):
    """an ADTS / MP3 / MP2 stream's bytes alone in a scheduler of its own (the default wait: nothing else is there to gather)"""
    key = (s.name,) + tuple(sorted(config.items()))
    if key not in _ALONE:
        outs, stats = run(engine, [s], **config)
        assert stats["errors"] == 0 and outs[0]
        _ALONE[key] = audio(outs[0])
    return _ALONE[key]


def check_plain(s, outs):
    units, text = s.model()
    assert text is None
    assert [o.data.tobytes() for o in outs if not isinstance(o, pipeline.DecodeError)] == units and len(outs) == len(units), s.name
    assert shapes(outs) == {s.shape}, (s.name, shapes(outs))
    if s.twin is not None:
        assert audio(outs) == s.twin, s.name


def check_converted(s, outs, want):
    want_bytes, want_shapes = want
    assert audio(outs) == want_bytes and len(want_bytes) > 8000, s.name
    assert shapes(outs) == want_shapes, (s.name, shapes(outs), want_shapes)
    bits, rate, channels = s.options
    assert all((o.bits_per_sample, o.sampling_rate) == (bits or s.shape[0], rate or s.shape[2]) for o in outs), s.name


def check_all(engine, plain, converted, main, outs, **config):
    at = 0
    for s in plain:
        check_plain(s, outs[at])
        at += 1
    for s, want in zip(converted, raw_references(engine, converted)):
        check_converted(s, outs[at], want)
        at += 1
    for s in main:
        assert audio(outs[at]) == alone(engine, s, **config), s.name
        at += 1
    assert at == len(outs)


# ---- 1 and 2: every family in shared rounds -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("front_end", [0, 3], ids=["host_front_end", "gpu_front_end"])
@pytest.mark.parametrize("budget, lanes", [(1, 1), (3, 1), (3, 2), (0, 1)])
def test_all_families_in_shared_rounds(engine, budget, lanes, front_end):
    plain, converted, main = T.table()
    streams = plain + converted + main
    config = dict(max_stream_frames_per_tick=budget, lanes=lanes, gpu_entropy=front_end)
    outs, stats = run(engine, streams, tick_wait_us=TICK_WAIT_US, **config)
    quota = budget or (32 if front_end else 8)  # sk_pipeline_create's defaults
    rounds, ideal = T.rounds_without_sharing(streams, quota)
    print("\nbudget %d, %d lane(s), gpu_entropy %d: %d ticks; %d without a shared round, %d at best" % (budget, lanes, front_end, stats["ticks"], rounds, ideal))
    check_all(engine, plain, converted, main, outs, **config)
    assert stats["errors"] == 0
    # At least one round was shared (on two lanes each lane counts its own rounds).  Not with the default quota of the GPU front end:
    # at 32 units a pass the rounds are no longer set by the quota but by the 16-deep output queues and the pace at which this file's
    # feeders and drain loop run (17 ticks seen against 18), which is a timing and no condition.
    if lanes == 1 and quota <= 8:
        assert stats["ticks"] < rounds, (stats["ticks"], rounds)


# ---- 3: one stream of every family ends alone ------------------------------------------------------------------------------------------
def test_one_stream_of_every_family_ends_alone_in_shared_rounds(engine):
    plain, _, main = T.table()
    bad = T.failing_streams()
    config = dict(max_stream_frames_per_tick=3, lanes=1, gpu_entropy=0)
    outs, stats = run(engine, plain + main + bad, tick_wait_us=TICK_WAIT_US, **config)
    print("\n%d ticks" % stats["ticks"])
    check_all(engine, plain, [], main, outs[:len(plain) + len(main)], **config)  # every healthy stream is what it is without them
    behind_a_conversion = [s for s in bad if s.options]
    wants = dict(zip([s.name for s in behind_a_conversion], raw_references(engine, behind_a_conversion, [s.good_units for s in behind_a_conversion])))
    for s, got in zip(bad, outs[len(plain) + len(main):]):
        assert got and isinstance(got[-1], pipeline.DecodeError) and str(got[-1]) == s.end_text(), (s.name, [str(o) for o in got[-1:]])
        units, _ = s.model()
        assert len(units) == s.good_units
        print("%s: %d of %d units in front of the damage delivered" % (s.name, len(got) - 1, s.good_units))
        if not s.options:  # everything in front of the damage, record by record
            assert [o.data.tobytes() for o in got[:-1]] == units, s.name
            assert shapes(got[:-1]) == {s.shape}, s.name
        elif s.name == "ALAC, the same behind a downmix":
            # what the device rejects behind a conversion takes the other packets of its row in that tick with it (as
            # test_flac_scheduler_gpu.py says of FLAC): of five good packets at three a round, at most two; the rest went out before
            want_bytes, want_shapes = wants[s.name]
            assert len(got) - 1 >= s.good_units - 2 and want_bytes.startswith(audio(got[:-1])) and shapes(got[:-1]) == want_shapes, s.name
        else:  # found on the host: the units in front of it are staged and go out, one AudioData each (no resampler)
            want_bytes, want_shapes = wants[s.name]
            assert audio(got[:-1]) == want_bytes and len(got) - 1 == s.good_units and shapes(got[:-1]) == want_shapes, s.name
    assert stats["errors"] == len(bad) == 9


# ---- 4: a slot changes family --------------------------------------------------------------------------------------------------------
def send_all(handle, chunks):
    for c in chunks:
        while True:
            try:
                handle.send(c)
                break
            except pipeline.DecodeError as e:
                assert e.kind == "InputBufferFull", e
                time.sleep(0.0005)


def spawn_when_free(sched, s, deadline_s=30):
    """a slot whose stream was cancelled with a pass in flight is free once that round has been delivered"""
    t0 = time.time()
    while True:
        try:
            return spawn(sched, s)
        except SoundkitError as e:
            assert e.status == SK_ERR_CAPACITY and time.time() - t0 < deadline_s, e
            time.sleep(0.001)


def test_a_slot_changes_family(engine):
    plain, converted, _ = T.table()
    by_name = {s.name.split(" -> ")[0]: s for s in converted}
    # one converted stream per kind, each with a resampler (and, where the codec has one, a carry)
    first = [by_name[n] for n in ("AIFF-C IMA4", "FLAC", "ALAC fixture", "G.711 mu-law", "G.722", "G.726 24k right", "GSM standard", "raw PCM", "WAV 24 bit")]
    # the kinds once more with other source rates, widths and channel counts where the table has them
    other = [by_name[n] for n in ("AIFF-C s24be", "FLAC", "ALAC built", "G.711 A-law stereo", "G.722", "G.726 40k left", "GSM Microsoft", "raw PCM", "WAV 24 bit")]
    n = len(first)
    wants = dict(zip([s.name for s in first + other], raw_references(engine, first + other)))
    sched = pipeline.BatchScheduler(engine, entropy_threads=4, max_streams=n, max_stream_frames_per_tick=3, tick_wait_us=2000)
    try:
        # round A
        handles = [spawn(sched, s) for s in first]
        kind_of = {h.id: k for k, h in enumerate(handles)}
        assert len(kind_of) == n
        with pytest.raises(SoundkitError):  # freed slots are the only ones there are
            spawn(sched, first[0])
        for s, got in zip(first, feed_and_drain(handles, [s.sends for s in first])):
            check_converted(s, got, wants[s.name])
        for h in handles:
            h.cancel()
        # round B: the slots are handed out last freed first; each gets the kind one position on (the GSM slot a G.726 stream, the
        # G.726 slot a G.722 stream, the G.722 slot an ALAC stream ... -- read towards the front of the list)
        second, handles = [], []
        for k in reversed(range(n)):
            second.append(other[(k - 1) % n])
            handles.append(spawn(sched, second[-1]))
        assert sorted(h.id for h in handles) == sorted(kind_of)
        for s, h in zip(second, handles):
            assert other.index(s) != kind_of[h.id], (s.name, h.id)  # every slot has changed its kind
            kind_of[h.id] = other.index(s)
        for s, got in zip(second, feed_and_drain(handles, [s.sends for s in second])):
            check_converted(s, got, wants[s.name])
        for h in handles:
            h.cancel()
        # third pass: half of the streams are cancelled mid-stream and other kinds take their slots while the other half runs on
        handles = [spawn(sched, s) for s in first]
        slot_kind = {h.id: k for k, h in enumerate(handles)}
        gone, stay = list(range(0, n, 2)), list(range(1, n, 2))
        third = {k: len(first[k].sends) // 3 for k in range(n)}
        for k in range(n):
            send_all(handles[k], first[k].sends[:third[k]])
        for k in gone:
            got = handles[k].recv(30000)  # at least one output from each before it goes
            assert got is not None and not isinstance(got, pipeline.DecodeError), first[k].name
        for k in gone:
            handles[k].cancel()
        late = [by_name[name] for name in ("FLAC", "G.711 A-law stereo", "G.726 40k left", "raw PCM", "G.711 mu-law")]
        late_handles = [spawn_when_free(sched, s) for s in late]
        assert sorted(h.id for h in late_handles) == sorted(handles[k].id for k in gone)
        for s, h in zip(late, late_handles):  # AIFF, ALAC, G.722, GSM and WAV slots: none of them gets its own kind back
            assert first[slot_kind[h.id]].name.split()[0] != s.name.split()[0], (s.name, first[slot_kind[h.id]].name)
        running = [handles[k] for k in stay] + late_handles
        outs = feed_and_drain(running, [first[k].sends[third[k]:] for k in stay] + [s.sends for s in late])
        for s, got in zip([first[k] for k in stay] + late, outs):
            check_converted(s, got, wants[s.name])
        assert sched.stats()["errors"] == 0
        for h in running:
            h.cancel()
    finally:
        sched.close()


# ---- 5: a full output queue holds every family back -----------------------------------------------------------------------------------
class Slowly:
    """a handle whose consumer takes one output per 2 ms"""

    def __init__(self, handle, every_s=0.002):
        self.handle, self.every_s, self.last = handle, every_s, 0.0

    def try_recv(self):
        if time.time() - self.last < self.every_s:
            return None
        got = self.handle.try_recv()
        if got is not None:
            self.last = time.time()
        return got

    def ended(self):
        return self.handle.ended()


def test_a_full_output_queue_holds_every_family_back_without_loss(engine):
    plain, converted, _ = T.table()  # (no MP3: Layer III behind a one-deep queue is an open question of its own)

    def take(handles, deadline_s):
        return drain([Slowly(h) for h in handles], deadline_s=30)  # a stall fails here
    outs, stats = run(engine, plain + converted, take=take, output_buffer=1, max_stream_frames_per_tick=0, tick_wait_us=2000)
    print("\n%d ticks, %d outputs" % (stats["ticks"], stats["outputs"]))
    check_all(engine, plain, converted, [], outs)
    assert stats["errors"] == 0

"""The stream table of tests/test_family_rounds_cpu.py and tests/test_family_rounds_gpu.py: every stream family the batch scheduler runs,
cut into sends, with what the models under tests/ make of those sends -- nothing here touches the GPU.

A Stream names its family (the tick of a round that decodes it), how it is spawned, its sends, and through `model()` the decoded PCM
unit by unit (one entry per send that completes something: a frame, a packet, a group, a piece) and the text that ends it, if any.
`units` is what the round-sharing condition counts.  Options are (bits, rate, channels) with None for "as decoded"."""
import math
import os

import aiff_model
import alac_builder
import alac_cases
import alac_model
import flac_model
import g72x_model as G
import gsm_model
import pcm_worker_model as W

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = "A_Tusk_is_used_to_make_costly_gifts"
FAMILIES = ["main", "aiff", "flac", "alac", "g72x", "gsm", "pcm"]  # the order of the ticks in a round
CONVERSION_TEXT = "Decoding failed: Output conversion failed: PCM data is unsupported or contains a partial frame"
ALAC_SYNTAX_TEXT = "Decoding failed: ALAC packet rejected: the elements break the syntax or miss the packet's end"
FLAC_SYNTAX_TEXT = "Decoding failed: FLAC frame rejected: the subframes break the syntax or miss the frame's end"


def read(path):
    with open(os.path.join(GOLD, path), "rb") as f:
        return f.read()


def wav_data(path):
    w = read(path)
    return w[w.index(b"data") + 8:]


def cut(data, n):
    return [data[at:at + n] for at in range(0, len(data), n)]


class Stream:
    def __init__(self, name, family, spawn, sends, decode=None, shape=None, fmt=W.FMT_S16LE, twin=None, options=None, text=None, good_units=None,
                 n_units=None):
        self.name, self.family, self.spawn, self.sends, self.decode = name, family, spawn, sends, decode
        self.shape, self.fmt, self.twin, self.options = shape, fmt, twin, options  # shape: (bits, channels, rate) as decoded
        self.text, self.good_units = text, good_units  # a failing stream: its last output's text, the units that go out in front of it
        self._n_units, self._model = n_units, None

    def end_text(self):
        """the text of a failing stream's last output: the family's own scheduler test's, or where that test takes it from the model, the model's"""
        return self.text if self.text is not None else self.model()[1]

    def model(self):
        """-> ([the decoded bytes of every unit], the text that ends the stream or None); computed once"""
        if self._model is None:
            self._model = self.decode(self.sends)
        return self._model

    @property
    def units(self):
        return self._n_units if self._n_units is not None else len(self.model()[0])

    def with_options(self, options):
        return Stream("%s -> %s" % (self.name, options), self.family, self.spawn, self.sends, self._shared_decode(), self.shape, self.fmt, None, options,
                      n_units=self._n_units)

    def _shared_decode(self):
        return lambda sends: self.model()  # the same sends: the same units


# ---- what the models make of a stream's sends -------------------------------------------------------------------------------------
def failing(exc):
    return "Decoding failed: " + str(exc)


def gsm_units(variant):
    def decode(sends):
        dec, out = gsm_model.GsmDecoder(variant), []
        for s in sends:
            try:
                got = dec.decode(s)
            except ValueError as exc:  # a frame without the magic nibble: nothing of its send is decoded
                return out, failing(exc)
            if len(got):
                out.append(got.astype("<i2").tobytes())
        try:
            dec.flush()
        except ValueError as exc:
            return out, failing(exc)
        return out, None
    return decode


def g726_units(rate, packing):
    def decode(sends):
        dec, out = G.G726Decoder(rate, packing), []
        for s in sends:
            got = dec.decode(s)
            if len(got):
                out.append(got.astype("<i2").tobytes())
        try:
            dec.flush()
        except ValueError as exc:
            return out, failing(exc)
        return out, None
    return decode


def g722_units(sends):
    dec = G.G722Decoder()
    return [dec.decode(s).astype("<i2").tobytes() for s in sends], None


def g711_units(law, channels=1, converting=False):
    def decode(sends):
        out = []
        for s in sends:
            if converting and len(s) % channels:  # a conversion refuses a send that splits a frame (audio_data_to_f32_channels)
                return out, CONVERSION_TEXT
            out.append(G.g711_decode(s, law).astype("<i2").tobytes())
        return out, None
    return decode


def alac_units(cookie):
    def decode(sends):
        cfg, out = alac_model.parse_cookie(cookie), []
        for packet in sends:
            try:
                out.append(alac_model.decode_packet_bytes(cfg, packet))
            except alac_model.AlacError as exc:
                assert exc.kind == alac_model.INVALID, exc
                return out, ALAC_SYNTAX_TEXT
        return out, None
    return decode


def flac_units(sends):
    data = b"".join(sends)
    info, _, pos = flac_model.split_stream(data)
    out = []
    while pos < len(data):
        try:
            h, ch = flac_model.decode_frame(data[pos:], info)
        except flac_model.FlacError as exc:
            assert str(exc) == "negative shift", exc  # the one damage this table holds: the framer passes it, the device rejects it
            return out, FLAC_SYNTAX_TEXT
        out.append(flac_model.contract_bytes(h, ch))
        pos += h["frame_bytes"]
    return out, None


def aiff_units(sends):
    """spawn_aiff: one add per send, then the finalising empty add"""
    m, out = aiff_model.AiffModel(), []
    for s in list(sends) + [b""]:
        try:
            got = m.add(s)
        except ValueError as exc:
            return out, failing(exc)
        if got is not None:
            out.append(got.data)
    return out, None


def raw_units(frame_bytes):
    def decode(sends):
        m, out = W.RawModel(frame_bytes), []
        for s in sends:
            piece = m.add(s)
            if piece:
                out.append(bytes(piece))
        try:
            m.flush()
        except ValueError as exc:
            return out, failing(exc)
        return out, None
    return decode


def wav_units(sends):
    _, pieces, err = W.wav_pieces(sends)
    return [bytes(p) for p in pieces], (failing(err) if err else None)


# ---- frame counts of the main tick's streams (headers only) --------------------------------------------------------------------------
def adts_frames(data):
    n, pos = 0, 0
    while pos + 7 <= len(data) and data[pos] == 0xFF and data[pos + 1] & 0xF0 == 0xF0:
        pos += ((data[pos + 3] & 3) << 11) | (data[pos + 4] << 3) | (data[pos + 5] >> 5)
        n += 1
    assert pos == len(data)
    return n


def mp3_frames(data):
    from oracle import mp3_bitstream
    return len(mp3_bitstream.scan(data)[0])


def mpa_frames(data):
    """Layer I / II frames of a stream of whole frames without tags (the MP2 fixture is)"""
    import mp12_model
    n, pos = 0, 0
    while pos + 4 <= len(data):
        h = mp12_model.parse_header(data[pos:pos + 4])
        pos += h["frame_bytes"]
        n += 1
    assert pos == len(data)
    return n


# ---- the table ----------------------------------------------------------------------------------------------------------------------
TO16K, TO8K = (16, 16000, 1), (16, 8000, 1)


def alac_fixture():
    data = read("alac/%s.caf" % NAME)
    at, size = alac_model.caf_chunks(data)["kuki"]
    _, packets, valid, priming, _ = alac_model.caf_index(data)
    assert (len(packets), valid, priming) == (6, 23680, 0)
    return data[at:at + size], packets


def alac_built():
    """44.1 kHz stereo, short packets of 300, 4096 and 77 frames (tests/test_alac_scheduler_gpu.py's)"""
    cfg = alac_builder.config(4096, 16, 2, 44100)
    good = [alac_cases.signal("tone", n, 16, n, 2) for n in (300, 4096, 77)]
    return cfg, good, [alac_builder.packet(cfg, ch, order=4, shift=6, mix_weight=1, mix_shift=2) for ch in good]


def repacked_right(data, rate):
    """a G.726 fixture (packed from the left) with the same codes packed from the right"""
    gb, bits = G.G726_GROUP_BYTES[rate], G.G726_BITS[rate]
    assert len(data) % gb == 0
    return b"".join(G.pack_code_group(G.unpack_code_group(data[g:g + gb], bits, G.LEFT), bits, G.RIGHT) for g in range(0, len(data), gb))


_TABLE = []


def table():
    """-> (the PCM-family streams with default options, their converted twins, the main tick's streams); built once"""
    if _TABLE:
        return _TABLE[0]
    twin8k = read("linear16_8k_A_Tusk.s16le")
    gsm = read("gsm/%s.gsm" % NAME)
    cookie, packets = alac_fixture()
    cfg, _, built = alac_built()
    alaw = read("g711/%s.alaw" % NAME)
    wav24 = read("wav_24_A_Tusk.wav")
    plain = [
        Stream("AIFF-C IMA4", "aiff", ("aiff",), cut(read("aiff/stream-ima4.aifc"), 1024), aiff_units, (16, 1, 8000)),
        Stream("AIFF-C s24be", "aiff", ("aiff",), cut(read("aiff/stream-s24be.aifc"), 1024), aiff_units, (24, 1, 8000), W.FMT_S24LE),
        Stream("FLAC", "flac", ("auto",), cut(read("flac/%s.flac" % NAME), 1024), flac_units, (16, 1, 16000), twin=read("linear16_A_Tusk.s16le")),
        # (the CAF fixture holds six packets and the built stream three: ALAC packets carry nothing from one to the next, so the
        # fixture's are sent twice and the built ones four times -- twelve units each, the recording twice)
        Stream("ALAC fixture", "alac", ("alac", cookie), packets * 2, alac_units(cookie), (16, 1, 8000), twin=wav_data("alac/%s.decoded.wav" % NAME) * 2),
        Stream("ALAC built", "alac", ("alac", alac_builder.cookie(cfg)), built * 4, alac_units(alac_builder.cookie(cfg)), (16, 2, 44100)),
        Stream("G.711 mu-law", "g72x", ("g711", G.ULAW, 8000, 1), cut(read("g711/%s.ulaw" % NAME), 200), g711_units(G.ULAW), (16, 1, 8000),
               twin=wav_data("aiff/g711_ulaw.decoded.wav")),
        Stream("G.711 A-law stereo", "g72x", ("g711", G.ALAW, 8000, 2), cut(alaw, 200), g711_units(G.ALAW, 2), (16, 2, 8000)),
        Stream("G.722", "g72x", ("g722",), cut(read("g722/%s.g722" % NAME), 200), g722_units, (16, 1, 16000), twin=wav_data("g722/%s.decoded.wav" % NAME)),
        Stream("G.726 24k right", "g72x", ("g726", 24000, G.RIGHT), cut(repacked_right(read("g726/%s_24.g726" % NAME), 24000), 100),
               g726_units(24000, G.RIGHT), (16, 1, 8000), twin=wav_data("g726/%s_24.decoded.wav" % NAME)),
        Stream("G.726 40k left", "g72x", ("g726", 40000, G.LEFT), cut(read("g726/%s_40.g726" % NAME), 333), g726_units(40000, G.LEFT), (16, 1, 8000),
               twin=wav_data("g726/%s_40.decoded.wav" % NAME)),
        Stream("GSM standard", "gsm", ("gsm", gsm_model.STANDARD), cut(gsm, 41), gsm_units(gsm_model.STANDARD), (16, 1, 8000), twin=wav_data("gsm/%s.decoded.wav" % NAME)),
        Stream("GSM Microsoft", "gsm", ("gsm", gsm_model.MICROSOFT), cut(gsm_model.standard_to_microsoft(gsm), 41), gsm_units(gsm_model.MICROSOFT), (16, 1, 8000),
               twin=wav_data("gsm/%s.decoded.wav" % NAME)),
        Stream("raw PCM", "pcm", ("raw", 8000, 1, W.FMT_S16LE), cut(twin8k, 1999), raw_units(2), (16, 1, 8000), twin=twin8k),
        Stream("WAV 24 bit", "pcm", ("auto",), cut(wav24, 1024), wav_units, (24, 1, 16000), W.FMT_S24LE, twin=wav_data("wav_24_A_Tusk.wav")),
    ]
    # every kind once more behind a conversion: 16 kHz mono s16 (8 kHz where the source has 16 kHz), one to 24 bits, one mono source to two channels
    options = {"FLAC": TO8K, "G.722": TO8K, "WAV 24 bit": TO8K, "G.726 40k left": (24, None, None), "GSM Microsoft": (16, None, 2)}
    converted = [s.with_options(options.get(s.name, TO16K)) for s in plain]
    main = [Stream("ADTS", "main", ("auto",), cut(read("aac/aac-stereo-48k.adts"), 1024), n_units=adts_frames(read("aac/aac-stereo-48k.adts"))),
            Stream("MP3", "main", ("auto",), cut(read("mp3/mono16k_A_Tusk.mp3"), 1024), n_units=mp3_frames(read("mp3/mono16k_A_Tusk.mp3"))),
            Stream("MP2", "main", ("auto",), cut(read("mp2/stereo48k_A_Tusk_1s.mp2"), 1024), n_units=mpa_frames(read("mp2/stereo48k_A_Tusk_1s.mp2")))]
    _TABLE.append((plain, converted, main))
    return _TABLE[0]


def failing_streams():
    """one stream per row of the issue's table that ends alone, each built the way its family's own scheduler test builds it; the damage
    lies behind at least four good units"""
    from test_flac_scheduler_gpu import build  # (the module needs the library, not a GPU)
    gsm = read("gsm/%s.gsm" % NAME)
    rejected = bytearray(gsm[:33 * 30])
    rejected[33 * 20] = 0x90 | (rejected[33 * 20] & 15)  # the twenty-first frame: in the seventh 99-byte send
    cfg, good, built = alac_built()
    bad_packet = alac_builder.packet(cfg, good[1], ptype=3)
    device_rejects = [built[0], built[1], built[2], built[0], built[1], bad_packet, built[2]]
    flac_bad, _ = build(420, 16, 2, 44100, [100, 60, 80, 50, 70, 90, 40], damage=5)
    g726 = read("g726/%s_40.g726" % NAME)
    alaw = read("g711/%s.alaw" % NAME)
    twin8k = read("linear16_8k_A_Tusk.s16le")
    qt, mp4 = alac_builder.cookie(cfg, "qt"), alac_builder.cookie(cfg, "mp4")
    return [
        Stream("FLAC, a frame the device rejects", "flac", ("auto",), cut(flac_bad, 1024), flac_units, (16, 2, 44100), text=FLAC_SYNTAX_TEXT, good_units=5),
        Stream("ALAC, a packet the device rejects", "alac", ("alac", qt), device_rejects, alac_units(qt), (16, 2, 44100), text=ALAC_SYNTAX_TEXT, good_units=5),
        Stream("ALAC, the same behind a downmix", "alac", ("alac", mp4), device_rejects, alac_units(mp4), (16, 2, 44100), options=(16, None, 1),
               text=ALAC_SYNTAX_TEXT, good_units=5),
        Stream("GSM, a frame without the magic nibble", "gsm", ("gsm", gsm_model.STANDARD), cut(bytes(rejected), 99), gsm_units(gsm_model.STANDARD), (16, 1, 8000),
               text="Decoding failed: GSM decoder rejected frame", good_units=6),
        Stream("GSM, a trailing partial packet", "gsm", ("gsm", gsm_model.STANDARD), cut(gsm[:33 * 10 + 3], 41), gsm_units(gsm_model.STANDARD), (16, 1, 8000),
               text="Decoding failed: GSM stream ended with 3 trailing partial-frame byte(s)", good_units=9),
        Stream("G.726, a trailing partial group", "g72x", ("g726", 40000, G.LEFT), cut(g726[:5 * 400 + 3], 333), g726_units(40000, G.LEFT), (16, 1, 8000),
               text="Decoding failed: G.726 stream ended with 3 trailing partial-packet byte(s)", good_units=7),
        Stream("G.711 stereo behind a conversion, a send that splits a frame", "g72x", ("g711", G.ALAW, 8000, 2), cut(alaw[:500], 100) + [alaw[500:601], alaw[601:700]],
               g711_units(G.ALAW, 2, converting=True), (16, 2, 8000), options=(16, None, 1), text=CONVERSION_TEXT, good_units=5),
        Stream("AIFF-C truncated inside the sound", "aiff", ("aiff",), cut(read("aiff/stream-s24be.aifc")[:30000], 997), aiff_units, (24, 1, 8000), W.FMT_S24LE,
               good_units=31),  # (its text is the model's, as in test_failing_streams_end_alone)
        Stream("raw PCM behind a conversion, a partial frame at the end", "pcm", ("raw", 8000, 1, W.FMT_S16LE), cut(twin8k[:10001], 1000), raw_units(2), (16, 1, 8000),
               options=(24, None, None), text="Decoding failed: Raw PCM stream ended with 1 trailing partial-frame byte(s)", good_units=10),
    ]


# ---- the round-sharing condition ----------------------------------------------------------------------------------------------------
def rounds_without_sharing(streams, quota):
    """-> (R, the ideal): with a per-stream quota q a round of one family holds at most S_f * q of its U_f units, so a run in which no two
    families ever share a round needs at least R = sum_f ceil(U_f / (S_f * q)) rounds; the ideal is max_f of the same terms.  The
    main tick's units are counted in frames, of which a stream hands a round at most q as well (a Layer II stream fewer): a lower bound
    there too."""
    terms = []
    for f in FAMILIES:
        mine = [s for s in streams if s.family == f]
        if mine:
            terms.append(math.ceil(sum(s.units for s in mine) / (len(mine) * quota)))
    return sum(terms), max(terms)

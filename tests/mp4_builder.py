"""Writes MP4 files from (config, units): regular with `moov` first or `mdat` first, and fragmented, each with the variations the demuxer
has a path for.  config: dict(codec "aac" / "alac", sample_rate, channels, private = the AudioSpecificConfig or the `alac` box payload).
The files are valid ISO base media as far as an audio demuxer reads them; the video track's samples are filler bytes."""
import struct


def box(name, payload, wide=False):
    if wide:  # size 1: the real size follows the name in 64 bits
        return struct.pack(">I4sQ", 1, name, 16 + len(payload)) + payload
    return struct.pack(">I4s", 8 + len(payload), name) + payload


def full(name, version, flags, payload):
    return box(name, struct.pack(">I", version << 24 | flags) + payload)


def descriptor(tag, body, length_bytes=1):
    n = len(body)
    digits = [n >> 7 * k & 0x7f for k in reversed(range(length_bytes))]
    assert n < 1 << 7 * length_bytes
    return bytes([tag] + [d | 0x80 for d in digits[:-1]] + [digits[-1]]) + body


def esds(asc, length_bytes=1):
    config = descriptor(5, asc, length_bytes)
    decoder = descriptor(4, bytes([0x40, 0x15, 0, 0, 0]) + struct.pack(">II", 128000, 128000) + config, length_bytes)
    return full(b"esds", 0, 0, descriptor(3, struct.pack(">HB", 0, 0) + decoder + descriptor(6, b"\x02", length_bytes), length_bytes))


def audio_entry(config, length_bytes=1):
    rate = config["sample_rate"] if config["sample_rate"] < 65536 else 0
    head = bytes(6) + struct.pack(">H", 1) + bytes(8) + struct.pack(">HHHHI", config["channels"], config.get("bits", 16), 0, 0, rate << 16)
    if config["codec"] == "aac":
        return box(b"mp4a", head + esds(config["private"], length_bytes))
    return box(b"alac", head + box(b"alac", config["private"]))


def video_entry():
    return box(b"avc1", bytes(6) + struct.pack(">H", 1) + bytes(16) + struct.pack(">HH", 64, 48) + bytes(50) + box(b"avcC", bytes([1, 66, 0, 30, 255, 224, 0])))


def stbl(entry, sizes, durations, chunks, per_chunk, co64=False, constant=False):
    """chunks: the offset of every chunk; per_chunk samples in each (the last may hold fewer)"""
    runs = []
    for d in durations:
        if runs and runs[-1][1] == d:
            runs[-1][0] += 1
        else:
            runs.append([1, d])
    stsc = [(1, per_chunk, 1)]
    if len(sizes) % per_chunk and len(chunks) > 1:
        stsc.append((len(chunks), len(sizes) % per_chunk, 1))
    elif len(sizes) % per_chunk:
        stsc = [(1, len(sizes), 1)]
    if constant:
        assert len(set(sizes)) == 1
        stsz = struct.pack(">II", sizes[0], len(sizes))
    else:
        stsz = struct.pack(">II", 0, len(sizes)) + struct.pack(">%dI" % len(sizes), *sizes)
    offsets = full(b"co64", 0, 0, struct.pack(">I%dQ" % len(chunks), len(chunks), *chunks)) if co64 else \
        full(b"stco", 0, 0, struct.pack(">I%dI" % len(chunks), len(chunks), *chunks))
    return box(b"stbl", full(b"stsd", 0, 0, struct.pack(">I", 1) + entry) +
               full(b"stts", 0, 0, struct.pack(">I", len(runs)) + b"".join(struct.pack(">II", *r) for r in runs)) +
               full(b"stsc", 0, 0, struct.pack(">I", len(stsc)) + b"".join(struct.pack(">III", *e) for e in stsc)) +
               full(b"stsz", 0, 0, stsz) + offsets)


def trak(track_id, handler, timescale, table, edit=None, movie_duration=0):
    """edit: [(segment duration in the movie's timescale, media time)] -> edts/elst"""
    tkhd = full(b"tkhd", 0, 3, struct.pack(">IIIII", 0, 0, track_id, 0, movie_duration) + bytes(60))
    edts = b""
    if edit:
        edts = box(b"edts", full(b"elst", 0, 0, struct.pack(">I", len(edit)) + b"".join(struct.pack(">IiHH", d, m, 1, 0) for d, m in edit)))
    mdhd = full(b"mdhd", 0, 0, struct.pack(">IIIIHH", 0, 0, timescale, 0, 0x55c4, 0))
    hdlr = full(b"hdlr", 0, 0, struct.pack(">I4s", 0, handler) + bytes(12) + b"handler\0")
    header = full(b"smhd", 0, 0, bytes(4)) if handler == b"soun" else full(b"vmhd", 0, 1, bytes(8))
    return box(b"trak", tkhd + edts + box(b"mdia", mdhd + hdlr + box(b"minf", header + table)))


def mvhd(timescale, version=0):
    if version == 1:
        return full(b"mvhd", 1, 0, struct.pack(">QQIQ", 0, 0, timescale, 0) + bytes(80))
    return full(b"mvhd", 0, 0, struct.pack(">IIII", 0, 0, timescale, 0) + bytes(80))


FTYP = box(b"ftyp", b"M4A \0\0\0\0M4A mp42isom")
JUNK = [box(b"free", bytes(11)), box(b"skip", bytes(5000)), box(b"uuid", bytes(range(40)))]


def regular(config, units, layout="moov_first", durations=None, timescale=None, movie_timescale=600, per_chunk=1, co64=False, constant=False,
            wide_mdat=False, video=False, junk=False, edit=None, length_bytes=1, mvhd_version=0):
    """layout "moov_first" or "mdat_first".  video: a video track in front of the audio track, its chunks interleaved with the audio's.
    junk: free / skip / uuid boxes between the top-level boxes.  edit: [(segment duration, media time)]"""
    timescale = timescale or config["sample_rate"]
    durations = durations or [1024] * len(units)
    groups = [units[k:k + per_chunk] for k in range(0, len(units), per_chunk)]
    filler = [bytes([0x55, k & 255]) * (37 + k % 5) for k in range(len(groups))] if video else []

    def tail(first_offset):
        """(the mdat box, audio chunk offsets, video chunk offsets) with the mdat's payload beginning at first_offset - header"""
        payload, audio, vid = bytearray(), [], []
        for k, g in enumerate(groups):
            if video:
                vid.append(first_offset + len(payload))
                payload += filler[k]
            audio.append(first_offset + len(payload))
            payload += b"".join(g)
        return box(b"mdat", bytes(payload), wide_mdat), audio, vid

    def moov(audio, vid):
        traks = b""
        if video:
            vt = stbl(video_entry(), [len(f) for f in filler], [512] * len(filler), vid, 1, co64)
            traks += trak(1, b"vide", 12800, vt)
        at = stbl(audio_entry(config, length_bytes), [len(u) for u in units], durations, audio, per_chunk, co64, constant)
        traks += trak(2 if video else 1, b"soun", timescale, at, edit)
        return box(b"moov", mvhd(movie_timescale, mvhd_version) + traks)

    gap = b"".join(JUNK) if junk else b""
    mdat_header = 16 if wide_mdat else 8
    if layout == "mdat_first":
        mdat, audio, vid = tail(len(FTYP) + len(gap) + mdat_header)
        return FTYP + gap + mdat + gap + moov(audio, vid)
    size = len(moov([0] * len(groups), [0] * len(groups)))
    mdat, audio, vid = tail(len(FTYP) + len(gap) + size + len(gap) + mdat_header)
    out = FTYP + gap + moov(audio, vid) + gap + mdat + (gap if junk else b"")
    assert len(moov(audio, vid)) == size
    return out


def fragmented(config, units, durations=None, timescale=None, per_moof=16, per_trun=None, base="moof", video=False, junk=False, trex_defaults=False,
               tfdt_version=1, edit=None, movie_timescale=600):
    """per_moof samples in every moof / mdat pair; per_trun: several trun boxes in a traf (None: one).  base: "moof" (default-base-is-moof),
    "explicit" (base-data-offset in tfhd) or "none" (neither flag: the first traf counts from its moof, a later one from where the traf
    before it ended).  video: a video traf in front of the audio traf in every moof, its data in front of the audio's.  trex_defaults:
    duration and size come from trex / tfhd where all samples of a fragment agree, so trun carries fewer fields."""
    timescale = timescale or config["sample_rate"]
    durations = durations or [1024] * len(units)
    audio_id = 2 if video else 1
    empty = box(b"stbl", full(b"stsd", 0, 0, struct.pack(">I", 1) + audio_entry(config)) + full(b"stts", 0, 0, bytes(4)) +
                full(b"stsc", 0, 0, bytes(4)) + full(b"stsz", 0, 0, bytes(8)) + full(b"stco", 0, 0, bytes(4)))
    traks, trex = b"", b""
    if video:
        vempty = box(b"stbl", full(b"stsd", 0, 0, struct.pack(">I", 1) + video_entry()) + full(b"stts", 0, 0, bytes(4)) +
                     full(b"stsc", 0, 0, bytes(4)) + full(b"stsz", 0, 0, bytes(8)) + full(b"stco", 0, 0, bytes(4)))
        traks += trak(1, b"vide", 12800, vempty)
        trex += full(b"trex", 0, 0, struct.pack(">IIIII", 1, 1, 512, 0, 0))
    traks += trak(audio_id, b"soun", timescale, empty, edit)
    trex += full(b"trex", 0, 0, struct.pack(">IIIII", audio_id, 1, 1024 if trex_defaults else 0, 0, 0))
    out = bytearray(FTYP + box(b"moov", mvhd(movie_timescale) + traks + box(b"mvex", trex)))
    time = 0
    for n, k in enumerate(range(0, len(units), per_moof)):
        if junk:
            out += JUNK[n % len(JUNK)]
        us, ds = units[k:k + per_moof], durations[k:k + per_moof]
        vdata = bytes([0xaa, n & 255]) * 61 if video else b""
        step = per_trun or len(us)
        runs = [(us[j:j + step], ds[j:j + step]) for j in range(0, len(us), step)]
        same_duration = trex_defaults and all(d == 1024 for d in ds)
        same_size = trex_defaults and len(set(len(u) for u in us)) == 1

        def moof(moof_at, size):
            data_at = moof_at + size + 8  # the mdat's payload
            trafs = b""
            if video:
                flags = 0x20000 if base == "moof" else 1 if base == "explicit" else 0
                tfhd = struct.pack(">I", 1) + (struct.pack(">Q", moof_at) if base == "explicit" else b"")
                trun = full(b"trun", 0, 0x201, struct.pack(">IiI", 1, data_at - moof_at, len(vdata)))
                trafs += box(b"traf", full(b"tfhd", 0, flags, tfhd) + full(b"tfdt", 0, 0, struct.pack(">I", n * 512)) + trun)
            flags = (0x20000 if base == "moof" else 1 if base == "explicit" else 0) | (0x10 if same_size else 0)
            tfhd = struct.pack(">I", audio_id) + (struct.pack(">Q", moof_at) if base == "explicit" else b"") + \
                (struct.pack(">I", len(us[0])) if same_size else b"")
            body = full(b"tfhd", 0, flags, tfhd)
            body += full(b"tfdt", 1, 0, struct.pack(">Q", time)) if tfdt_version == 1 else full(b"tfdt", 0, 0, struct.pack(">I", time))
            at = data_at + len(vdata)
            for j, (ru, rd) in enumerate(runs):
                f = (0 if same_duration else 0x100) | (0 if same_size else 0x200)
                fields = b"".join((b"" if same_duration else struct.pack(">I", d)) + (b"" if same_size else struct.pack(">I", len(u))) for u, d in zip(ru, rd))
                # base "none" behind a video traf: the audio's first run follows the video's data without an offset of its own
                offset = None if (base == "none" and video and j == 0) or j > 0 else at - moof_at
                if offset is None:
                    body += full(b"trun", 0, f, struct.pack(">I", len(ru)) + fields)
                else:
                    body += full(b"trun", 0, f | 1, struct.pack(">Ii", len(ru), offset) + fields)
                at += sum(len(u) for u in ru)
            return box(b"moof", full(b"mfhd", 0, 0, struct.pack(">I", n + 1)) + trafs + box(b"traf", body))

        size = len(moof(0, 0))
        out += moof(len(out), size)
        out += box(b"mdat", vdata + b"".join(us))
        time += sum(ds)
    return bytes(out)


def faststart(data):
    """a `mdat`-first file rewritten with `moov` in front of `mdat`: every stco entry moved by the moov's size"""
    import mp4_model as M
    tops = {name: (p - 8, q) for name, p, q in M.boxes(data)}
    (ma, mb), (da, db) = tops[b"moov"], tops[b"mdat"]
    assert da < ma
    moov = bytearray(data[ma:mb])
    at = moov.find(b"stco")
    n = struct.unpack_from(">I", moov, at + 8)[0]
    for k in range(n):
        old = struct.unpack_from(">I", moov, at + 12 + 4 * k)[0]
        struct.pack_into(">I", moov, at + 12 + 4 * k, old + len(moov))
    return bytes(data[:da]) + bytes(moov) + bytes(data[da:ma]) + bytes(data[mb:])

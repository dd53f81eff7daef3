"""Writes the MP4 / MOV files the PCM and FLAC sample-entry tests need, beside mp4_builder.py (whose boxes it uses): QuickTime sound
descriptions of version 0, 1 and 2 under any entry name, `enda` / `wave` / `dfLa` children, sample tables with any chunking (gaps between
chunks, a constant or a listed `stsz`), fragmented files under any entry, and FLAC-in-MP4 files cut from the FLAC fixtures, one frame per sample."""
import struct

import mp4_builder as B

SIGNED, PACKED, ALIGNED_HIGH, NON_INTERLEAVED = 1 << 2, 1 << 3, 1 << 4, 1 << 5
FLOAT, BIG = 1, 2


def sound_entry(name, version=0, channels=2, bits=16, rate=48000, children=b"", v1=None, v2=None):
    """v1: (frames per packet, bytes per packet, bytes per frame, bytes per sample); v2: dict(rate, channels, bits, flags,
    bytes_per_packet, frames_per_packet), the base fields then hold what QuickTime writes there (3 channels slots, 16 bits, rate 1)"""
    head = bytes(6) + struct.pack(">H", 1) + struct.pack(">HHI", version, 0, 0) + struct.pack(">HHHHI", channels, bits, 0, 0, (rate if rate < 65536 else 0) << 16)
    if version == 1:
        head += struct.pack(">IIII", *(v1 or (1, (bits + 7) // 8, (bits + 7) // 8 * channels, (bits + 7) // 8)))
    elif version == 2:
        v = dict(rate=float(rate), channels=channels, bits=bits, flags=SIGNED | PACKED, bytes_per_packet=(bits + 7) // 8 * channels, frames_per_packet=1)
        v.update(v2 or {})
        head = bytes(6) + struct.pack(">H", 1) + struct.pack(">HHI", 2, 0, 0) + struct.pack(">HHHHI", 3, 16, 0xfffe, 0, 0x10000)
        head += struct.pack(">IdIIIIII", 72, v["rate"], v["channels"], 0x7f000000, v["bits"], v["flags"], v["bytes_per_packet"], v["frames_per_packet"])
    elif version != 0:
        pass  # (a version nothing reads: the 28-byte head alone)
    return B.box(name, head + children)


def enda(flag):
    return B.box(b"enda", struct.pack(">H", flag))


def wave(*children):
    return B.box(b"wave", B.box(b"frma", b"in24") + b"".join(children) + B.box(b"\0\0\0\0", b""))


def movie(entry, chunks, sample_size=None, sizes=None, durations=None, timescale=48000, gaps=None, edit=None, layout="moov_first", movie_timescale=600,
          stts=None):
    """chunks: [bytes]: one chunk each.  sample_size: a constant `stsz` of that size, every chunk holding len / sample_size samples of
    duration 1; otherwise sizes = [[sample sizes of chunk k]] with durations in the same shape.  gaps: bytes in front of chunk k inside
    `mdat`.  stts: the (count, duration) pairs in place of the ones derived."""
    gaps = gaps or [0] * len(chunks)
    if sample_size:
        per = [len(c) // sample_size for c in chunks]
        stsz = struct.pack(">II", sample_size, sum(per))
        runs = stts or [(sum(per), 1)]
    else:
        per = [len(s) for s in sizes]
        flat = [n for s in sizes for n in s]
        stsz = struct.pack(">II", 0, len(flat)) + struct.pack(">%dI" % len(flat), *flat)
        runs = stts or []
        if not stts:
            for d in (d for ds in durations for d in ds):
                if runs and runs[-1][1] == d:
                    runs[-1] = (runs[-1][0] + 1, d)
                else:
                    runs.append((1, d))
    stsc = []
    for k, n in enumerate(per):
        if not stsc or stsc[-1][1] != n:
            stsc.append((k + 1, n, 1))

    def moov(offsets):
        table = B.box(b"stbl", B.full(b"stsd", 0, 0, struct.pack(">I", 1) + entry) +
                      B.full(b"stts", 0, 0, struct.pack(">I", len(runs)) + b"".join(struct.pack(">II", *r) for r in runs)) +
                      B.full(b"stsc", 0, 0, struct.pack(">I", len(stsc)) + b"".join(struct.pack(">III", *e) for e in stsc)) +
                      B.full(b"stsz", 0, 0, stsz) + B.full(b"stco", 0, 0, struct.pack(">I%dI" % len(offsets), len(offsets), *offsets)))
        return B.box(b"moov", B.mvhd(movie_timescale) + B.trak(1, b"soun", timescale, table, edit))

    def mdat(first):
        payload, offsets = bytearray(), []
        for c, g in zip(chunks, gaps):
            payload += bytes([0xee]) * g
            offsets.append(first + len(payload))
            payload += c
        return B.box(b"mdat", bytes(payload)), offsets

    if layout == "mdat_first":
        m, offsets = mdat(len(B.FTYP) + 8)
        return B.FTYP + m + moov(offsets)
    size = len(moov([0] * len(chunks)))
    m, offsets = mdat(len(B.FTYP) + size + 8)
    return B.FTYP + moov(offsets) + m


def fragmented(entry, units, durations, timescale=48000, per_moof=4):
    """a fragmented file (mvex in moov, empty sample tables) under any sample entry: per_moof samples in every moof / mdat pair"""
    empty = B.box(b"stbl", B.full(b"stsd", 0, 0, struct.pack(">I", 1) + entry) + B.full(b"stts", 0, 0, bytes(4)) + B.full(b"stsc", 0, 0, bytes(4)) +
                  B.full(b"stsz", 0, 0, bytes(8)) + B.full(b"stco", 0, 0, bytes(4)))
    trex = B.full(b"trex", 0, 0, struct.pack(">IIIII", 1, 1, 0, 0, 0))
    out = bytearray(B.FTYP + B.box(b"moov", B.mvhd(600) + B.trak(1, b"soun", timescale, empty) + B.box(b"mvex", trex)))
    time = 0
    for n, k in enumerate(range(0, len(units), per_moof)):
        us, ds = units[k:k + per_moof], durations[k:k + per_moof]

        def moof(size):
            fields = b"".join(struct.pack(">II", d, len(u)) for u, d in zip(us, ds))
            trun = B.full(b"trun", 0, 0x301, struct.pack(">Ii", len(us), size + 8) + fields)
            traf = B.box(b"traf", B.full(b"tfhd", 0, 0x20000, struct.pack(">I", 1)) + B.full(b"tfdt", 1, 0, struct.pack(">Q", time)) + trun)
            return B.box(b"moof", B.full(b"mfhd", 0, 0, struct.pack(">I", n + 1)) + traf)

        out += moof(len(moof(0)))
        out += B.box(b"mdat", b"".join(us))
        time += sum(ds)
    return bytes(out)


# ---- FLAC in MP4 ---------------------------------------------------------------------------------------------------------------------

def flac_frames(data):
    """a FLAC fixture (with or without `fLaC` and STREAMINFO) -> (the 34-byte STREAMINFO, [frame bytes], [block size per frame]).  The
    host framer cuts the frames; a fixture without STREAMINFO gets one made from its first frame's header."""
    from soundkit_amd import flac
    at = 0
    info = None
    if data[:4] == b"fLaC":
        at = 4
        while True:
            last, kind, n = data[at] >> 7, data[at] & 0x7f, int.from_bytes(data[at + 1:at + 4], "big")
            if kind == 0:
                info = data[at + 4:at + 4 + n]
            at += 4 + n
            if last:
                break
    rc, found, used = flac.scan(data[at:], None, final=True, cap=4096)
    assert rc == 0 and found and used == len(data) - at, (rc, len(found), used)
    frames = [data[at + f["offset"]:at + f["offset"] + f["frame_bytes"]] for f in found]
    if info is None:
        f = found[0]
        block = max(x["block_size"] for x in found)
        total = sum(x["block_size"] for x in found)
        packed = f["sample_rate"] << 44 | (f["channels"] - 1) << 41 | (f["bits_per_sample"] - 1) << 36 | total
        info = struct.pack(">HH", block, block) + bytes(3) + bytes(3) + packed.to_bytes(8, "big") + bytes(16)
    assert len(info) == 34
    return info, frames, [f["block_size"] for f in found], found[0]


def dfla(streaminfo, form):
    """the three forms normalize_mp4_flac_decoder_configuration takes: "dfla" (version and flags, then the blocks), "bare" (the 34 bytes
    alone), "stream" (already `fLaC` + blocks)"""
    block = bytes([0x80, 0, 0, 34]) + streaminfo
    return {"dfla": bytes(4) + block, "bare": streaminfo, "stream": b"fLaC" + block}[form]


def flac_in_mp4(data, form="dfla", edit=None, layout="moov_first", per_chunk=3):
    """-> (the file, the frames, the block sizes, the first frame's header).  One frame per sample, per_chunk samples a chunk"""
    info, frames, blocks, first = flac_frames(data)
    entry = sound_entry(b"fLaC", 0, first["channels"], first["bits_per_sample"], first["sample_rate"], B.box(b"dfLa", dfla(info, form)))
    groups = [list(range(k, min(k + per_chunk, len(frames)))) for k in range(0, len(frames), per_chunk)]
    file = movie(entry, [b"".join(frames[i] for i in g) for g in groups], sizes=[[len(frames[i]) for i in g] for g in groups],
                 durations=[[blocks[i] for i in g] for g in groups], timescale=first["sample_rate"], edit=edit, layout=layout)
    return file, frames, blocks, first

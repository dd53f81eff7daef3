"""What the WebM tests share: the two fixtures, the files tests/webm_builder.py writes for the demuxer cases, and the fixtures of the
other codecs rewrapped as WebM (Ogg Vorbis, ADTS AAC, native FLAC), each with the packets it was made from.  Host only."""
import os

import webm_builder as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"vorbis": os.path.join("vorbis", "yt_itag_171_vorbis.webm"), "opus": os.path.join("webm", "A_Tusk_is_used_to_make_costly_gifts.webm")}


def golden(*path):
    with open(os.path.join(GOLDEN, *path), "rb") as f:
        return f.read()


def fixture(name):
    return golden(FIXTURES[name])


def frames_of(seed, sizes):
    return [bytes((seed + 7 * k + i) & 0xff for i in range(n)) for k, n in enumerate(sizes)]


def builder_cases():
    """name -> file, for the comparison with the model: every one demuxes to the end"""
    a = B.track(1, b"A_AAC", private=b"\x14\x08", rate=16000.0, channels=1, default_duration=64000000)
    f = lambda seed, *sizes: frames_of(seed, sizes)  # noqa: E731
    cases = {}
    for lacing, sizes in (("none", (40,)), ("xiph", (300, 255, 0, 7, 510)), ("fixed", (16, 16, 16)), ("ebml", (100, 90, 400, 8, 70))):
        cases["lacing_" + lacing] = B.webm([a], [B.cluster(0, [B.simple_block(1, 0, f(1, 9)), B.simple_block(1, 64, f(2, *sizes), lacing)])])
    cases["ebml_lacing_of_one_frame"] = B.webm([a], [B.cluster(0, [B.simple_block(1, 0, f(3, 33), "ebml")])])
    cases["unknown_sizes"] = B.webm([a], [B.cluster(0, [B.simple_block(1, 5, f(4, 12))], unknown=True),
                                          B.cluster(1000, [B.simple_block(1, -3, f(5, 14))], unknown=True)], unknown_segment=True)
    plain = B.track(1, b"A_FLAC", private=b"fLaC" + bytes(38), rate=8000.0, rate_width=4, channels=1)
    cases["block_groups"] = B.webm([plain], [B.cluster(100, [
        B.block_group(1, 0, f(6, 20)), B.block_group(1, 10, f(7, 21), reference=-10), B.block_group(1, 20, f(8, 5, 6, 7), "xiph", duration=9),
        B.block_group(1, 30, f(9, 30), discard=16000000), B.block_group(1, 40, f(10, 31), discard=-1, duration=4),
        B.block_group(1, 50, f(11, 8, 8), "fixed", duration=7, discard=-129), B.block_group(1, 60, f(12, 9), extra=B.el(0xEC, bytes(5)))])])
    stripped = B.track(1, b"A_AAC", private=b"\x12\x10", rate=44100.0, channels=2, default_duration=23219955, encodings=B.header_stripping(b"\x21\x1a"))
    cases["header_stripping"] = B.webm([stripped], [B.cluster(0, [B.simple_block(1, 0, f(13, 40)), B.simple_block(1, 23, f(14, 3, 0, 4), "xiph")])])
    pad = B.el(B.VOID, bytes(300)) + B.el(B.SEEK_HEAD, bytes(40)) + B.el(B.CUES, bytes(70)) + B.el(B.TAGS, bytes(25))
    cases["padding_elements"] = B.webm([a], [B.cluster(0, [B.simple_block(1, 0, f(15, 10))]), B.cluster(64, [B.el(B.VOID, bytes(9)), B.simple_block(1, 0, f(16, 11))])],
                                       before=pad, between=B.el(B.CUES, bytes(33)) + B.el(B.TAGS, bytes(3)))
    scaled = B.track(1, b"A_VORBIS", private=b"\x02\x01\x01abc", rate=48000.0, channels=2, scale=2.5, codec_delay=6500000, seek_pre_roll=80000000)
    cases["scales"] = B.webm([scaled], [B.cluster(7, [B.simple_block(1, -7, f(17, 10)), B.simple_block(1, 3, f(18, 10)),
                                                      B.block_group(1, 9, f(19, 4, 4), "fixed", duration=3)])], timecode_scale=333333)
    video = B.track(1, b"V_VP9", kind=1)
    second = B.track(130, b"A_OPUS", private=b"OpusHead\x01\x02\x38\x01\x80\xbb\x00\x00\x00\x00\x00", channels=2)
    other = B.track(4, b"A_PCM/INT/LIT", rate=8000.0, channels=1)
    cases["two_audio_and_video"] = B.webm([video, a.replace(B.uint(0xD7, 1), B.uint(0xD7, 2)), second, other], [B.cluster(0, [
        B.simple_block(1, 0, f(20, 50)), B.simple_block(2, 0, f(21, 9)), B.simple_block(130, 0, [b"\x08abc"], number_width=2), B.simple_block(4, 0, f(22, 6)),
        B.simple_block(130, 20, [b"\xfc\xff\xfe", b"\x00a", b"\x0b\x02y"], "xiph", number_width=2), B.simple_block(2, 64, f(23, 9), number_width=3)])])
    cases["duplicate_track_number"] = B.webm([a, B.track(1, b"A_FLAC", private=b"fLaC", rate=8000.0, channels=2), video], [B.cluster(0, [B.simple_block(1, 0, f(24, 9))])])
    cases["rate_and_channels_by_default"] = B.webm([B.track(1, b"A_OPUS")], [B.cluster(0, [B.simple_block(1, 0, [b"\x78z"])])])
    return cases


def adts_frames(data):
    """an ADTS stream -> (the two-byte AudioSpecificConfig, [raw access units])"""
    at, out, asc = 0, [], None
    while at + 7 <= len(data):
        h = data[at:at + 7]
        assert h[0] == 0xff and h[1] & 0xf6 == 0xf0 and h[1] & 1, "an ADTS header without CRC"
        n = (h[3] & 3) << 11 | h[4] << 3 | h[5] >> 5
        aot, index, ch = (h[2] >> 6) + 1, (h[2] >> 2) & 15, (h[2] & 1) << 2 | h[3] >> 6
        asc = bytes([aot << 3 | index >> 1, (index & 1) << 7 | ch << 3])
        out.append(data[at + 7:at + n])
        at += n
    assert at == len(data)
    return asc, out


def ogg_packets(data):
    """-> ([ident, comment, setup], [audio packets]) of an Ogg Vorbis file"""
    from soundkit_amd.vorbis import OggPacketParser
    p = OggPacketParser()
    packets = [k.data for k in p.add(data) + p.finish()]
    p.close()
    return packets[:3], packets[3:]


def flac_parts(data):
    """a native FLAC file -> (`fLaC` and the metadata blocks, [frames])"""
    from soundkit_amd.flac import FlacReader
    r = FlacReader()
    frames = [b for _, b in r.add(data) + r.add(b"")]
    r.close()
    head = len(data) - sum(len(b) for b in frames)
    assert data[head:head + len(frames[0])] == frames[0]
    return data[:head], frames


def wrap(codec_id, private, packets, rate, channels, ms_per_packet, discard=None, per_cluster=40):
    """packets as one frame per SimpleBlock of track 1; discard: {packet index: DiscardPadding in ns} puts those into BlockGroups"""
    clusters = []
    for first in range(0, len(packets), per_cluster):
        blocks = []
        for k in range(first, min(first + per_cluster, len(packets))):
            relative = int((k - first) * ms_per_packet)
            blocks.append(B.block_group(1, relative, [packets[k]], discard=discard[k]) if discard and k in discard else B.simple_block(1, relative, [packets[k]]))
        clusters.append(B.cluster(int(first * ms_per_packet), blocks))
    return B.webm([B.track(1, codec_id, private=private, rate=float(rate), channels=channels)], clusters)


def wrapped_ogg(discard=None):
    """the Ogg Vorbis fixture (8 kHz mono, 94 audio packets) -> (file, headers, packets)"""
    headers, packets = ogg_packets(golden("vorbis", "A_Tusk_is_used_to_make_costly_gifts.ogg"))
    return wrap(b"A_VORBIS", B.xiph_private(headers), packets, 8000, 1, 32, discard), headers, packets


def wrapped_aac():
    """-> (file, the ADTS stream it was made from)"""
    adts = golden("aac", "mono16k_A_Tusk.aac")
    asc, units = adts_frames(adts)
    return wrap(b"A_AAC", asc, units, 16000, 1, 64), adts


def wrapped_flac():
    """-> (file, the native stream it was made from)"""
    flac = golden("flac", "A_Tusk_is_used_to_make_costly_gifts.flac")
    head, frames = flac_parts(flac)
    return wrap(b"A_FLAC", head, frames, 16000, 1, 72), flac

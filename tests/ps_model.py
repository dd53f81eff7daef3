"""A Python restatement of the reference's MPEG program stream reader (soundkit-decoder/src/lib.rs:572-804), for the tests: what
csrc/ps_stream.h must hand out for a whole file, and what DVD LPCM unpacks to.  Function for function, with the line ranges.

Where the walker is its own (csrc/ps_stream.h says why) the model follows the walker and says so: packets are walked by their length
field (the reference rescans every payload for 00 00 01), only the first LPCM substream is the track, MPEG audio PES is a track, the
sample bytes leave in whole blocks.  `demux(data, mode)` -> (events, error): ("config", {...}) in front of the first packet,
("packet", bytes) per PES that completed something; error: the refusal's text or None."""

TRACK_FIRST, TRACK_LPCM, TRACK_MPEG_AUDIO = 0, 1, 2
MAX_PAYLOAD = 512 * 1024 * 1024  # lib.rs:621


class Refused(Exception):
    pass


def looks_like_mpeg_ps(data):  # lib.rs:572-574
    return data[:4] == b"\x00\x00\x01\xba"


def parse_mpeg_pes_payload(packet):  # lib.rs:686-728 -> the payload, or None where the packet is ignored
    cursor = 0
    while cursor < len(packet) and packet[cursor] == 0xFF:
        cursor += 1
    if cursor >= len(packet):
        return None
    first = packet[cursor]
    if first & 0xC0 == 0x80:
        if len(packet) - cursor < 3:
            raise Refused("MPEG-2 PES header is truncated")
        cursor += 3 + packet[cursor + 2]
        if cursor > len(packet):
            raise Refused("MPEG-2 PES optional header is truncated")
    else:
        if first & 0xC0 == 0x40:
            cursor += 2
        if cursor >= len(packet):
            raise Refused("MPEG-1 PES header is truncated")
        first = packet[cursor]
        if first & 0xF0 == 0x20:
            cursor += 5
        elif first & 0xF0 == 0x30:
            cursor += 10
        elif first == 0x0F:
            cursor += 1
        else:
            return None
        if cursor > len(packet):
            raise Refused("MPEG-1 PES timestamp is truncated")
    return packet[cursor:]


def parse_dvd_lpcm_header(header):  # lib.rs:730-748
    bits = 16 + ((header[1] >> 6) & 3) * 4
    if bits not in (16, 20, 24):
        raise Refused("unsupported DVD LPCM sample depth %d" % bits)
    return dict(rate=[48000, 96000, 44100, 32000][(header[1] >> 4) & 3], channels=(header[1] & 7) + 1, bits=bits)


def block_size(bits, channels):  # unpack_dvd_lpcm, lib.rs:752-782
    if bits == 16:
        return channels * 2
    return 12 if channels in (1, 2, 4) else (24 if channels == 8 else channels * 12)


def unpack_dvd_lpcm(packed, bits, channels):  # lib.rs:750-804 -> little-endian PCM
    if bits == 16:
        if len(packed) % (channels * 2):
            raise Refused("DVD LPCM ends with a partial sample block")
        out = bytearray(len(packed))
        out[0::2], out[1::2] = packed[1::2], packed[0::2]
        return bytes(out)
    if bits == 20:
        raise Refused("20-bit DVD LPCM decoding is not implemented")
    groups_per_block = 1 if channels in (1, 2, 4) else (2 if channels == 8 else channels)
    size = block_size(bits, channels)
    if len(packed) % size:
        raise Refused("DVD LPCM ends with a partial 24-bit sample block")
    out = bytearray()
    for at in range(0, len(packed), size):
        block, cursor = packed[at:at + size], 0
        for _ in range(groups_per_block):
            high, low = block[cursor:cursor + 8], block[cursor + 8:cursor + 12]
            for sample in range(4):
                out += bytes([low[sample], high[sample * 2 + 1], high[sample * 2]])
            cursor += 12
    return bytes(out)


def demux(data, mode=TRACK_FIRST):
    events, config, carry, total = [], None, bytearray(), 0

    def wanted(stream_id):  # the walker's track choice
        if stream_id == 0xBD:
            return mode != TRACK_MPEG_AUDIO and (config is None or config["kind"] == "pcm-dvd")
        if 0xC0 <= stream_id <= 0xDF:
            return mode != TRACK_LPCM and (config is None or (config["kind"] == "mpeg-audio" and config["stream_id"] == stream_id))
        return False

    try:
        pos, n = 0, len(data)
        while n - pos >= 4:  # find_start_code (lib.rs:677-684) wants the id behind the three bytes
            if data[pos:pos + 3] != b"\x00\x00\x01":
                pos = data.find(b"\x00\x00\x01", pos + 1)
                if pos < 0:
                    break
                continue
            stream_id = data[pos + 3]
            if stream_id == 0xBA:  # the walker's: the pack header by its own layout
                if n - pos < 5:
                    break
                if data[pos + 4] & 0xC0 == 0x40:
                    if n - pos < 14:
                        break
                    pos += 14 + (data[pos + 13] & 7)
                else:
                    pos += 12 if data[pos + 4] & 0xF0 == 0x20 else 4
                continue
            if stream_id < 0xBB:
                pos += 4
                continue
            want = wanted(stream_id)
            if n - pos < 6:
                if want:
                    raise Refused("MPEG-PS PES length is truncated")  # lib.rs:593-595
                break
            length = (data[pos + 4] << 8) | data[pos + 5]
            if not want:  # the walker's: stepped over by its length; a video packet of length 0: back to the scan
                pos += 4 if 0xE0 <= stream_id <= 0xEF and length == 0 else 6 + length
                continue
            if n - pos < 6 + length:
                raise Refused("MPEG-PS PES packet is truncated")  # lib.rs:597-602
            payload = parse_mpeg_pes_payload(data[pos + 6:pos + 6 + length])
            pos += 6 + length
            if payload is None:
                continue
            if stream_id != 0xBD:  # the walker's: an MPEG audio track
                if not payload:
                    continue
                if config is None:
                    config = dict(kind="mpeg-audio", stream_id=stream_id, substream_id=None, rate=None, channels=None, bits=None, block_bytes=None)
                    events.append(("config", dict(config)))
                total += len(payload)
                events.append(("packet", bytes(payload)))
                continue
            if len(payload) < 7 or not 0xA0 <= payload[0] <= 0xAF:  # lib.rs:604
                continue
            if config is not None and payload[0] != config["substream_id"]:  # the walker's: one substream
                continue
            fmt = parse_dvd_lpcm_header(payload[4:7])
            if config is not None:
                if (fmt["bits"], fmt["rate"], fmt["channels"]) != (config["bits"], config["rate"], config["channels"]):
                    raise Refused("DVD LPCM format changes mid-stream")  # lib.rs:609-614
            else:
                if fmt["bits"] == 20:  # the walker's: at the first packet, not at the unpacking
                    raise Refused("20-bit DVD LPCM decoding is not implemented")
                config = dict(kind="pcm-dvd", stream_id=0xBD, substream_id=payload[0], block_bytes=block_size(fmt["bits"], fmt["channels"]), **fmt)
                events.append(("config", dict(config)))
            total += len(payload) - 7
            if total > MAX_PAYLOAD:
                raise Refused("MPEG-PS audio payload exceeds budget")
            carry += payload[7:]
            whole = len(carry) // config["block_bytes"] * config["block_bytes"]
            if whole:
                events.append(("packet", bytes(carry[:whole])))
                del carry[:whole]
        if carry:
            raise Refused("DVD LPCM ends with a partial sample block" if config["bits"] == 16 else "DVD LPCM ends with a partial 24-bit sample block")
        if config is None:
            raise Refused("MPEG-PS has no supported DVD LPCM track")  # lib.rs:635-637
    except Refused as e:
        return events, str(e)
    return events, None

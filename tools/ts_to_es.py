#!/usr/bin/env python3
"""Extract the PES payload of one PID of an MPEG-TS file (188-byte packets): the elementary stream as the decoder takes it.
Used once to turn the reference's MP2 fixture (testdata/mpeg-ts/mp2-stereo-48k.ts, PID 0x100: 42 Layer II frames of 576 bytes,
testdata/mpeg-ts/README.md) into tests/golden/mp2/stereo48k_A_Tusk_1s.mp2.

    python tools/ts_to_es.py IN.ts OUT.es [PID, default 0x100]
"""
import sys


def packets(data):
    for off in range(0, len(data) - 187, 188):
        p = data[off:off + 188]
        if p[0] != 0x47:
            raise ValueError("lost TS sync at %d" % off)
        pid = ((p[1] & 0x1F) << 8) | p[2]
        start = bool(p[1] & 0x40)
        afc = (p[3] >> 4) & 3
        body = 4
        if afc & 2:
            body += 1 + p[4]
        if afc & 1 and body < 188:
            yield pid, start, p[body:]


def extract(data, want_pid):
    out = bytearray()
    for pid, start, payload in packets(data):
        if pid != want_pid:
            continue
        if start:
            if payload[:3] != b"\x00\x00\x01":
                raise ValueError("bad PES start code")
            payload = payload[9 + payload[8]:]
        out += payload
    return bytes(out)


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    es = extract(open(sys.argv[1], "rb").read(), int(sys.argv[3], 0) if len(sys.argv) > 3 else 0x100)
    open(sys.argv[2], "wb").write(es)
    print("%d bytes" % len(es))

"""Writes tests/golden/g711_expected.json: the 16-bit linear value of every G.711 code, mu-law and A-law, as CPython's audioop decodes
them (audioop.ulaw2lin / alaw2lin, the ITU-T G.711 tables).  Needs a Python that still ships audioop (3.12 or older); the tests read only
the committed file."""
import audioop
import json
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))


def table(fn):
    return [struct.unpack("<h", fn(bytes([c]), 2))[0] for c in range(256)]


def main():
    out = {"source": "audioop.ulaw2lin / audioop.alaw2lin, width 2, codes 0 .. 255", "mulaw": table(audioop.ulaw2lin), "alaw": table(audioop.alaw2lin)}
    assert max(out["mulaw"]) == 32124 and min(out["mulaw"]) == -32124 and out["mulaw"][0x7F] == 0 and out["mulaw"][0xFF] == 0
    assert max(out["alaw"]) == 32256 and min(out["alaw"]) == -32256 and out["alaw"][0x55] == -8 and out["alaw"][0xD5] == 8
    with open(os.path.join(HERE, "..", "g711_expected.json"), "w") as f:
        json.dump(out, f)
        f.write("\n")


if __name__ == "__main__":
    main()

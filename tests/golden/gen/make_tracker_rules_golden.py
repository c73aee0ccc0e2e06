#!/usr/bin/env python3
"""Regenerates tests/golden/tracker_rules_expected.json: what the REFERENCE's own accumulate_fm and finalize make of every case of
tests/tracker_rule_cases.py, run under Node through ref_driver.js at the output levels 3 (the ranked tracks as stored) and 10 (the straightened frames per
syllable) — per case segments_ci, syllables_ci and both levels' callbacks, every number of a callback as an index into the file's table of distinct
doubles (big-endian hex), a string (a syllable's time) as {"s": ...}.  The inputs are not stored (the cases module builds them again); a digest of each
case's bytes is.

Build-container only (needs /root/reference and node).  Nothing of the reference's source is written anywhere.

    python3 tests/golden/gen/make_tracker_rules_golden.py
"""
import json
import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(GOLD)))
from tests import tracker_rule_cases as rc  # noqa: E402

REF = "/root/reference"
LEVELS = (3, 10)
NONFINITE = ("NaN", "Infinity", "-Infinity")


def main():
    with tempfile.TemporaryDirectory() as td:
        clips = []
        for k, c in enumerate(rc.CASES):
            sp = rc.spectra(c)
            path = os.path.join(td, "c%03d.bin" % k)
            sp.tofile(path)
            s = c["settings"]
            for level in LEVELS:
                clips.append(dict(spectra=path, frames=int(sp.shape[0]), bands=c["bands"], level=level, window_step=s["window_step"], pause_length=s["pause_length"],
                                  min_seg_length=s["min_seg_length"], auto_noise_gate=bool(s["auto_noise_gate"]), voiced_max_dB=s["voiced_max_dB"],
                                  voiced_min_dB=s["voiced_min_dB"], trace=False))
        jp, op = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        json.dump(dict(bundle=os.path.join(REF, "dist/main.js"), clips=clips), open(jp, "w"))
        subprocess.run(["node", os.path.join(HERE, "ref_driver.js"), jp, op], check=True, timeout=1800)
        got = json.load(open(op))
    values, index = [], {}

    def enc(x):
        if isinstance(x, list):
            return [enc(y) for y in x]
        if x is None:
            return None
        if isinstance(x, str) and x not in NONFINITE:
            return {"s": x}
        h = struct.pack(">d", float(x)).hex()
        if h not in index:
            index[h] = len(values)
            values.append(h)
        return index[h]

    cases = []
    for k, c in enumerate(rc.CASES):
        r3, r10 = got["results"][2 * k], got["results"][2 * k + 1]
        assert r3["segments_ci"] == r10["segments_ci"], c["name"]
        cases.append(dict(name=c["name"], digest=rc.digest(c), segments_ci=r10["segments_ci"], syllables_ci=r10["syllables_ci"],
                          callbacks_3=enc(r3["callbacks"]), callbacks_10=enc(r10["callbacks"])))
    out = dict(generator="tests/golden/gen/make_tracker_rules_golden.py", node=got["node"], values=values, cases=cases)
    path = os.path.join(GOLD, "tracker_rules_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases,", len(values), "distinct doubles")


if __name__ == "__main__":
    sys.exit(main())

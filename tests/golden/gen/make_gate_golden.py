#!/usr/bin/env python3
"""Regenerates tests/golden/gate_expected.json: what the REFERENCE's own frame loop makes of every case of tests/gate_cases.py, run under Node
through ref_driver.js (output level 5, state trace on) — per case segments_ci and the 10-column trace (c_ci, c_started, no_fm_segs, ctx_max,
floor, n, p, h, d, g just before `c_ci++`), as indices into the file's table of distinct doubles (big-endian hex).  The inputs are not stored (the
cases module builds them again); a digest of each case's bytes is.

Build-container only (needs /root/reference and node).  Nothing of the reference's source is written anywhere.

    python3 tests/golden/gen/make_gate_golden.py
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
from tests import gate_cases as gc  # noqa: E402
from tests.util import jsnum  # noqa: E402

REF = "/root/reference"


def main():
    with tempfile.TemporaryDirectory() as td:
        clips = []
        for k, c in enumerate(gc.CASES):
            sp = gc.spectra(c)
            path = os.path.join(td, "c%03d.bin" % k)
            sp.tofile(path)
            s = c["settings"]
            clips.append(dict(spectra=path, frames=int(sp.shape[0]), bands=c["bands"], level=5, window_step=s["window_step"], pause_length=s["pause_length"],
                              min_seg_length=s["min_seg_length"], auto_noise_gate=bool(s["auto_noise_gate"]), voiced_max_dB=s["voiced_max_dB"],
                              voiced_min_dB=s["voiced_min_dB"], trace=True))
        jp, op = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        json.dump(dict(bundle=os.path.join(REF, "dist/main.js"), clips=clips), open(jp, "w"))
        subprocess.run(["node", os.path.join(HERE, "ref_driver.js"), jp, op], check=True, timeout=1800)
        got = json.load(open(op))
    values, index, cases, nfr = [], {}, [], 0
    for c, r in zip(gc.CASES, got["results"]):
        tr = r.get("trace", [])
        assert len(tr) == len(gc.spectra(c)), c["name"]
        flat = []
        for row in tr:
            assert len(row) == 10
            for x in row:
                h = struct.pack(">d", jsnum(x)).hex()
                if h not in index:
                    index[h] = len(values)
                    values.append(h)
                flat.append(index[h])
        nfr += len(tr)
        cases.append(dict(name=c["name"], digest=gc.digest(c), segments_ci=r["segments_ci"], trace=flat))
    out = dict(generator="tests/golden/gen/make_gate_golden.py", node=got["node"], values=values, cases=cases)
    path = os.path.join(GOLD, "gate_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases,", nfr, "frames,", len(values), "distinct doubles")


if __name__ == "__main__":
    sys.exit(main())

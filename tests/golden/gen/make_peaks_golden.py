#!/usr/bin/env python3
"""Regenerates tests/golden/peaks_expected.json: what the REFERENCE's own frame loop makes of every case of tests/peak_cases.py, run under Node through
ref_driver.js with the per-clip option "peaks" — per frame the candidate list [i, s, l] that accumulate_fm receives (after the shoulder shrink) and
n, p, h, d, g.  Every case runs with the FIXED gate at a floor below 1 (auto_noise_gate off, voiced_min_dB -20: v = 0.1; the segmenter takes the value
unchecked), where the reference accepts every candidate of amplitude 1 and more and its list is the device's table; the cases of
peak_cases.FLOOR_RUNS run again at floors inside their amplitudes.  Triples are stored as bytes (hex, three per candidate: no case has more than 256
bands), the five numbers as decimal strings of exact integers or floats; the inputs are not stored (the cases module builds them again), a digest of
each case's bytes is.

Build-container only (needs /root/reference and node).  Nothing of the reference's source is written anywhere.

    python3 tests/golden/gen/make_peaks_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(GOLD)))
from tests import peak_cases as pc  # noqa: E402
from tests.util import jsnum  # noqa: E402

REF = "/root/reference"
EVERY = -20.0                     # voiced_min_dB of the run that keeps every candidate: v = 10 ** -1


def main():
    runs = [(c, EVERY) for c in pc.CASES] + [(pc.by_name(n), dB) for n, dBs in pc.FLOOR_RUNS.items() for dB in dBs]
    with tempfile.TemporaryDirectory() as td:
        clips = []
        for k, (c, dB) in enumerate(runs):
            path = os.path.join(td, "c%03d.bin" % k)
            c["frames"].tofile(path)
            clips.append(dict(spectra=path, frames=int(c["frames"].shape[0]), bands=c["bands"], level=5, window_step=25.0, pause_length=200.0, min_seg_length=50.0,
                              auto_noise_gate=False, voiced_max_dB=100.0, voiced_min_dB=dB, trace=False, peaks=True))
        jp, op = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        json.dump(dict(bundle=os.path.join(REF, "dist/main.js"), clips=clips), open(jp, "w"))
        subprocess.run(["node", os.path.join(HERE, "ref_driver.js"), jp, op], check=True, timeout=1800)
        got = json.load(open(op))
    out_runs, nfr, ncand = [], 0, 0
    for (c, dB), r in zip(runs, got["results"]):
        pk = r["peaks"]
        assert len(pk) == len(c["frames"]), c["name"]
        counts, triples, nums = [], bytearray(), []
        for cands, five in pk:
            counts.append(len(cands))
            for t in cands:
                assert len(t) == 3 and all(0 <= x < 256 for x in t)
                triples += bytes(t)
            nums.append([repr(jsnum(x)) for x in five])
        nfr += len(pk); ncand += sum(counts)
        out_runs.append(dict(name=c["name"], voiced_min_dB=dB, digest=pc.digest(c), counts=counts, triples=bytes(triples).hex(), nphdg=nums))
    out = dict(generator="tests/golden/gen/make_peaks_golden.py", node=got["node"], runs=out_runs)
    path = os.path.join(GOLD, "peaks_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes;", len(out_runs), "runs,", nfr, "frames,", ncand, "candidates")


if __name__ == "__main__":
    sys.exit(main())

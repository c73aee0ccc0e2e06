#!/usr/bin/env python3
"""Regenerates tests/golden/fuzz_spectra.npz + fuzz_expected.json: twelve random synthetic clips (seeds 9000 .. 9011, 300 frames,
128 bands; synth_spectra.synth_clip) at levels 5 and 13 with the default settings, run through the reference's own back end
(formantanalyzer@1.1.6, dist/main.js module 584) under Node by ref_driver.js.  tests/test_oracle_backend.py holds the oracle to
these results, bit for bit.  Outputs are data: the input spectra + what the reference returned.

    python3 tests/golden/gen/make_fuzz_golden.py <path of the reference's dist/main.js>
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from synth_spectra import synth_clip  # noqa: E402

SEEDS = range(9000, 9012)
FRAMES = 300
LEVELS = (5, 13)
SETTINGS = dict(window_step=25, pause_length=200, min_seg_length=50, auto_noise_gate=True, voiced_max_dB=100, voiced_min_dB=10)


def main():
    bundle = os.path.abspath(sys.argv[1])
    tmp = tempfile.mkdtemp(prefix="wsa_fuzz_")
    spectra, clips, meta = {}, [], []
    for seed in SEEDS:
        key = f"s{seed}_f{FRAMES}"
        spectra[key] = synth_clip(seed, FRAMES)
        spectra[key].tofile(os.path.join(tmp, key + ".bin"))
        for lv in LEVELS:
            clips.append(dict(SETTINGS, spectra=os.path.join(tmp, key + ".bin"), frames=FRAMES, bands=128, level=lv, trace=False))
            meta.append(dict(key=key, level=lv))
    job, out = os.path.join(tmp, "job.json"), os.path.join(tmp, "out.json")
    json.dump({"bundle": bundle, "clips": clips}, open(job, "w"))
    subprocess.run(["node", os.path.join(HERE, "ref_driver.js"), job, out], check=True)
    res = json.load(open(out))
    cases = [dict(m, segments_ci=r["segments_ci"], callbacks=r["callbacks"]) for m, r in zip(meta, res["results"])]
    np.savez_compressed(os.path.join(GOLD, "fuzz_spectra.npz"), **spectra)
    json.dump({"generator": "tests/golden/gen/make_fuzz_golden.py", "node": res["node"],
               "reference": "formantanalyzer@1.1.6 (dist/main.js module 584)", "settings": SETTINGS, "cases": cases},
              open(os.path.join(GOLD, "fuzz_expected.json"), "w"), separators=(",", ":"))
    for f in ("fuzz_spectra.npz", "fuzz_expected.json"):
        print(f, os.path.getsize(os.path.join(GOLD, f)))


if __name__ == "__main__":
    main()

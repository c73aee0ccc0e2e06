#!/usr/bin/env python3
"""Regenerates tests/golden/long_spectra.npz + long_expected.json: the 2600-frame clip designed_clip("long_voiced", 2600) — one voiced
span of 2580 frames at a 10 ms step, 69 energy events per formant column — at levels 5 and 13, run through the reference's own back end
(formantanalyzer@1.1.6, dist/main.js module 584) under Node by ref_driver.js.  tests/test_oracle_backend.py holds the oracle to these
results, bit for bit: the oracle is the reference of the GPU tests of spans past 2048 frames.  Outputs are data: the input spectrum + what
the reference returned.

    python3 tests/golden/gen/make_long_golden.py <path of the reference's dist/main.js>
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
from synth_spectra import designed_clip  # noqa: E402

FRAMES = 2600
LEVELS = (5, 13)
SETTINGS = dict(window_step=10, pause_length=200, min_seg_length=50, auto_noise_gate=True, voiced_max_dB=100, voiced_min_dB=10)


def main():
    bundle = os.path.abspath(sys.argv[1])
    tmp = tempfile.mkdtemp(prefix="wsa_long_")
    key = f"long_voiced_f{FRAMES}"
    spec = designed_clip("long_voiced", FRAMES)
    spec.tofile(os.path.join(tmp, key + ".bin"))
    clips = [dict(SETTINGS, spectra=os.path.join(tmp, key + ".bin"), frames=FRAMES, bands=128, level=lv, trace=False) for lv in LEVELS]
    job, out = os.path.join(tmp, "job.json"), os.path.join(tmp, "out.json")
    json.dump({"bundle": bundle, "clips": clips}, open(job, "w"))
    subprocess.run(["node", os.path.join(HERE, "ref_driver.js"), job, out], check=True)
    res = json.load(open(out))
    cases = [dict(key=key, level=lv, segments_ci=r["segments_ci"], callbacks=r["callbacks"]) for lv, r in zip(LEVELS, res["results"])]
    np.savez_compressed(os.path.join(GOLD, "long_spectra.npz"), **{key: spec})
    json.dump({"generator": "tests/golden/gen/make_long_golden.py", "node": res["node"],
               "reference": "formantanalyzer@1.1.6 (dist/main.js module 584)", "settings": SETTINGS, "cases": cases},
              open(os.path.join(GOLD, "long_expected.json"), "w"), separators=(",", ":"))
    for f in ("long_spectra.npz", "long_expected.json"):
        print(f, os.path.getsize(os.path.join(GOLD, f)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Regenerates tests/golden/dispatch_spectra.npz + dispatch_expected.json: the reference pin for MORE THAN ONE dropped segment.

A segment whose straighten step throws in the reference stays in segments_ci without a result; from then on the dispatcher P() (dist/main.js:2
@B28869) reports result k with the timestamps of segments_ci[k] (@B29138 / @B29622).  The other fixtures hold clips with one such segment.  This
generator SEARCHES synth_spectra.synth_clip seeds with the C oracle (oracle/backend.c, on the CPU) for clips where the rule is exercised harder:

    two-drops         two or more dropped segments in one clip
    drop-first        the clip's first segment is dropped and a result follows
    drop-two-results  a dropped segment with at least two results behind it

The search is bounded: seeds SEARCH_SEEDS (0 .. 19 999) of FRAMES = 400 frames, 128 bands, the default settings; per kind the smallest seed that
qualifies is taken.  It goes in blocks of 400 seeds and STOPS at the end of the first block that completes the set: the committed fixture was made by a
search that looked at 7 600 seeds (15 of them held a dropped segment at all), as its "search" record says.  A kind nobody qualifies for within the bound is reported in the output's "search" record and simply has no clip.  What is found
goes through the reference's own back end (formantanalyzer@1.1.6, dist/main.js module 584) under Node by ref_driver.js at levels 5, 13 and 11.
tests/test_dispatch_reference.py holds the oracle and the dispatcher's restatement (tests/dispatch_ref.py) to these results.  Outputs are data: the
input spectra + what the reference returned.

    python3 tests/golden/gen/make_dispatch_golden.py <path of the reference's dist/main.js>
"""
import json
import multiprocessing
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLD))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from synth_spectra import synth_clip  # noqa: E402

SEARCH_SEEDS = range(0, 20000)
FRAMES = 400
LEVELS = (5, 13, 11)
KINDS = ("two-drops", "drop-first", "drop-two-results")
SETTINGS = dict(window_step=25, pause_length=200, min_seg_length=50, auto_noise_gate=True, voiced_max_dB=100, voiced_min_dB=10)


def kinds_of(flags):
    """which of KINDS a clip's per-segment flags (< 0: dropped) qualify for"""
    drops = [i for i, f in enumerate(flags) if f < 0]
    out = []
    if len(drops) >= 2:
        out.append("two-drops")
    if drops and drops[0] == 0 and len(flags) > len(drops):
        out.append("drop-first")
    if drops and sum(1 for f in flags[drops[0] + 1:] if f >= 0) >= 2:
        out.append("drop-two-results")
    return out


def _probe(seed):
    from oracle import pyoracle
    out = pyoracle.run_backend(synth_clip(seed, FRAMES), pyoracle.default_cfg(level=5))
    return seed, kinds_of(out["flags"]), sum(1 for f in out["flags"] if f < 0)


def search(seeds=SEARCH_SEEDS, workers=8, block=400):
    """smallest qualifying seed per kind, and how many seeds were looked at / held a drop at all"""
    found, looked, with_drop = {}, 0, 0
    seeds = list(seeds)
    with multiprocessing.Pool(workers) as pool:
        for b in range(0, len(seeds), block):
            for seed, kinds, drops in pool.map(_probe, seeds[b:b + block]):
                looked += 1
                with_drop += 1 if drops else 0
                for k in kinds:
                    found.setdefault(k, seed)
            if all(k in found for k in KINDS):      # (seeds come back in order: the first block that completes the set holds the smallest ones)
                break
    return found, looked, with_drop


def main():
    bundle = os.path.abspath(sys.argv[1])
    found, looked, with_drop = search()
    print("search:", found, "seeds looked at", looked, "with a drop", with_drop)
    tmp = tempfile.mkdtemp(prefix="wsa_dispatch_")
    spectra, clips, meta = {}, [], []
    for seed in sorted(set(found.values())):
        key = f"s{seed}_f{FRAMES}"
        spectra[key] = synth_clip(seed, FRAMES)
        spectra[key].tofile(os.path.join(tmp, key + ".bin"))
        for lv in LEVELS:
            clips.append(dict(SETTINGS, spectra=os.path.join(tmp, key + ".bin"), frames=FRAMES, bands=128, level=lv, trace=False))
            meta.append(dict(key=key, level=lv, kinds=[k for k in KINDS if found.get(k) == seed]))
    cases, node = [], None
    if clips:
        job, out = os.path.join(tmp, "job.json"), os.path.join(tmp, "out.json")
        json.dump({"bundle": bundle, "clips": clips}, open(job, "w"))
        subprocess.run(["node", os.path.join(HERE, "ref_driver.js"), job, out], check=True)
        res = json.load(open(out))
        node = res["node"]
        cases = [dict(m, segments_ci=r["segments_ci"], callbacks=r["callbacks"]) for m, r in zip(meta, res["results"])]
    np.savez_compressed(os.path.join(GOLD, "dispatch_spectra.npz"), **spectra)
    json.dump({"generator": "tests/golden/gen/make_dispatch_golden.py", "node": node, "reference": "formantanalyzer@1.1.6 (dist/main.js module 584)",
               "settings": SETTINGS, "search": dict(seeds=[SEARCH_SEEDS.start, SEARCH_SEEDS.stop], frames=FRAMES, looked=looked, with_drop=with_drop, found=found),
               "cases": cases}, open(os.path.join(GOLD, "dispatch_expected.json"), "w"), separators=(",", ":"))
    for f in ("dispatch_spectra.npz", "dispatch_expected.json"):
        print(f, os.path.getsize(os.path.join(GOLD, f)))


if __name__ == "__main__":
    main()

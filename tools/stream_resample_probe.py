#!/usr/bin/env python3
"""512 paced streams converted inside the step (wsa_stream_create_mixed: 44.1 -> 48 kHz, 16 -> 48 kHz, and a set already at 48 kHz that is
only copied) beside the plain 48 kHz step of the same build: p50 / p99 per step from wsa_stream_time_steps (profiles/stream_resample.md).

    python tools/stream_resample_probe.py [--only plain48|mixed441|mixed16|mixed48copy] [--steps 3000] [--rounds 2] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/stream_resample_probe.py --only mixed441 --rounds 1 --steps 1000"""
import argparse
import json
import sys

import numpy as np

import math
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webspeechanalyzer_amd as wsa
from webspeechanalyzer_amd.synth import synth_clips

ap = argparse.ArgumentParser()
ap.add_argument("--only", default="")
ap.add_argument("--steps", type=int, default=3000)
ap.add_argument("--warmup", type=int, default=200)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--out", default="")
args = ap.parse_args()
n, F, fs_out, seconds = 512, 1, 48000, 2.0
an = wsa.Analyzer(wsa.Config(output_level=5))
g = an.geometry(fs_out)
res = []
cases = [("plain48", None), ("mixed441", 44100), ("mixed16", 16000), ("mixed48copy", 48000)]
for rnd in range(args.rounds):
    for name, rate in cases:
        if args.only and name != args.only:
            continue
        if rate is None:
            st = an.streams(n, fs_out, frames_per_step=F)
            rate_in = fs_out
        else:
            st = an.streams(n, rate, frames_per_step=F, resample_to=fs_out)
            rate_in = rate
        st.enable_graph(True)
        sig = synth_clips(n, int(seconds * rate_in), fs=rate_in, seed=5, device="cuda").cpu().numpy()
        b, ratio = F * g["hop"], rate_in / fs_out           # the paced counts: what keeps a source on real time (include/wsa.h)
        counts = [math.floor((s + 1) * b * ratio) - math.floor(s * b * ratio) for s in range(int(seconds * fs_out) // b - 1)]
        feed = np.zeros((len(counts), n, st.input_stride), np.float32)
        pos = 0
        for k, c in enumerate(counts):
            feed[k, :, :c] = sig[:, pos:pos + c]
            pos += c
        st.time_steps(args.warmup, feed)
        us, rows = st.time_steps(args.steps, feed)
        r = dict(case=name, round=rnd, steps=args.steps, p50_ms=float(np.percentile(us, 50)) / 1e3, p99_ms=float(np.percentile(us, 99)) / 1e3,
                 mean_ms=float(us.mean()) / 1e3, max_ms=float(us.max()) / 1e3, rows=int(rows), input_stride=st.input_stride, frame_capacity=st.frame_capacity)
        print(json.dumps(r), flush=True)
        res.append(r)
        st.close()
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)

#!/usr/bin/env python3
"""Tuning helper: K0 on a mixed-rate batch (1024 ten-second clips, rates dealt evenly from 16 / 22.05 / 44.1 / 48 kHz -> 48 kHz, level 5) against
the same clips as per-rate batches of the single-rate entry point (the 48 kHz group needs no K0 there).  Per-kernel times via rocprofv3:
   rocprofv3 --kernel-trace --stats -d /tmp/p -o r -- python3 tools/mixed_rate_probe.py [mixed|one_launch|split]; tools/rocprof_summary.py /tmp/p/.../r_results.db
mixed: one launch per rate class (default); one_launch: one launch over the whole work list (WSA_RS_ONE_LAUNCH); split: four single-rate batches back to back."""
import os
os.environ.setdefault("WSA_TUNING_ENV", "1")   # libwsa reads its tuning switches only when this is set
import sys
import time
mode = sys.argv[1] if len(sys.argv) > 1 else "mixed"
if mode == "one_launch":
    os.environ["WSA_RS_ONE_LAUNCH"] = "1"
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from webspeechanalyzer_amd import Analyzer, Config
from webspeechanalyzer_amd.synth import synth_clips

RATES, n, reps = [16000, 22050, 44100, 48000], 1024, 7
groups = {r: synth_clips(n // len(RATES), 10 * r, fs=r, seed=1 + k, device="cuda:0") for k, r in enumerate(RATES)}
an = Analyzer(Config(output_level=5), device=0)
s = torch.cuda.current_stream().cuda_stream
if mode == "split":
    batches = [(an.batch([10 * r] * (n // len(RATES)), r, resample_to=48000) if r != 48000 else an.batch([10 * r] * (n // len(RATES)), r), groups[r]) for r in RATES]
else:
    rates = [RATES[i % len(RATES)] for i in range(n)]
    pcm = torch.zeros((n, 10 * max(RATES)), dtype=torch.float32, device="cuda:0")
    for i, r in enumerate(rates):
        pcm[i, :10 * r] = groups[r][i // len(RATES)]
    batches = [(an.batch([10 * r for r in rates], [float(r) for r in rates], resample_to=48000), pcm)]


def once():
    rows, fe = 0, 0.0
    for b, x in batches:
        b.run(x.data_ptr(), x.stride(0), s)
    for b, x in batches:
        rows += b.device_result(s).n_rows
        fe += float(b.stage_ms()[0])
    return rows, fe


for _ in range(2):
    once()
times, fes = [], []
for _ in range(reps):
    t0 = time.perf_counter()
    rows, fe = once()
    times.append((time.perf_counter() - t0) * 1e3); fes.append(fe)
print(f"{mode}: whole batch ms min {min(times):.3f} median {sorted(times)[reps // 2]:.3f} max {max(times):.3f}; K0 + front end (stage 0) ms min {min(fes):.3f} max {max(fes):.3f}; rows {rows}")

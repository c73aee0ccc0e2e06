#!/usr/bin/env python3
"""Step time of stream sets fed packed PCM beside the same sets fed floats (spec PK-1; profiles/stream_pcm.md): p50 / p99 per step from
wsa_stream_time_steps / _packed (the library's clock), every case warmed, the cases of a group alternating in chunks inside one process.

  group 48k   512 sources at 48 kHz, one 25 ms frame per step: fed float ("f32_a"), fed i16 ("i16"), fed float again on a second set
              ("f32_b": the two float cases differ by nothing, their distance is the spread of the call)
  group 8k    512 mu-law sources at 8 kHz converted to 48 kHz ("mulaw_8k") beside the same set fed floats ("f32_8k")

The condition of profiles/stream_pcm.md: p50(i16) - p50(f32_a) <= |p50(f32_a) - p50(f32_b)|.  Bytes per step on the link come from the shapes.

    timeout -k 10 600 python tools/stream_pcm_probe.py [--steps 2000] [--chunks 4] [--group 48k|8k] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webspeechanalyzer_amd as wsa
from webspeechanalyzer_amd import capi
from webspeechanalyzer_amd.synth import synth_clips

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=2000, help="timed steps per case (at least 2000 for the note)")
ap.add_argument("--chunks", type=int, default=4, help="the cases of a group alternate in this many chunks")
ap.add_argument("--warmup", type=int, default=200)
ap.add_argument("--group", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()
n, F, fs_out, seconds = 512, 1, 48000, 2.0
an = wsa.Analyzer(wsa.Config(output_level=5))
hop = an.geometry(fs_out)["hop"]


def mulaw_encode(x):
    """floats -> the mu-law code whose linear value lies nearest (the decode formula of PK-1 gives the table)"""
    table = (capi.pcm_decode("mulaw", np.arange(256, dtype=np.uint8)).astype(np.float64) * 32768).astype(np.int64)
    order = np.argsort(table, kind="stable")
    srt = table[order]
    v = np.clip(np.rint(x.astype(np.float64) * 32767.0), -32768, 32767).astype(np.int64)
    hi = np.clip(np.searchsorted(srt, v), 1, 255)
    return order[np.where(np.abs(srt[hi] - v) < np.abs(srt[hi - 1] - v), hi, hi - 1)].astype(np.uint8)


def open_case(fmt, rate, sig):
    """sig [n, samples] in the case's format -> (set, feed blocks, bytes one step puts on the link)"""
    st = an.streams(n, rate, frames_per_step=F, resample_to=fs_out) if rate != fs_out else an.streams(n, fs_out, frames_per_step=F)
    st.enable_graph(True)
    b, ratio = F * hop, rate / fs_out
    counts = [int(np.floor(float((s + 1) * b) * ratio)) - int(np.floor(float(s * b) * ratio)) for s in range(int(seconds * fs_out) // b - 1)]
    if fmt == "f32":
        feed = np.zeros((len(counts), n, st.input_stride), np.float32)
        link = n * st.input_stride * 4                       # stream_pull_kernel copies whole rows
    else:
        st.set_input_format(fmt)
        dt = np.int16 if fmt == "i16" else np.uint8
        feed = np.zeros((len(counts), n, st.input_stride_bytes // np.dtype(dt).itemsize), dt)
        per = 8 if fmt == "i16" else 16                      # stream_pull_packed_kernel reads the 16-byte chunks that hold the step's count
        link = n * 16 * ((max(counts) + per - 1) // per)
    pos = 0
    for k, c in enumerate(counts):
        feed[k, :, :c] = sig[:, pos:pos + c]
        pos += c
    return st, feed, link


def time_case(st, fmt, feed, steps):
    return (st.time_steps if fmt == "f32" else st.time_steps_packed)(steps, feed)


res = []
groups = [("48k", fs_out, "i16", [("f32_a", "f32"), ("i16", "i16"), ("f32_b", "f32")]),
          ("8k", 8000, "mulaw", [("mulaw_8k", "mulaw"), ("f32_8k", "f32")])]
for gname, rate, pfmt, cases in groups:
    if args.group and args.group != gname:
        continue
    sig = synth_clips(n, int(seconds * rate), fs=rate, seed=5, device="cuda").cpu().numpy()
    packed_sig = np.clip(np.rint(sig * 32767.0), -32768, 32767).astype(np.int16) if pfmt == "i16" else mulaw_encode(sig)
    float_sig = np.stack([capi.pcm_decode(pfmt, np.ascontiguousarray(r)) for r in packed_sig])      # every case of a group is fed the same samples
    opened = [(name, fmt) + open_case(fmt, rate, float_sig if fmt == "f32" else packed_sig) for name, fmt in cases]
    for name, fmt, st, feed, link in opened:
        time_case(st, fmt, feed, args.warmup)
    us = {name: [] for name, _ in cases}
    rows = {name: 0 for name, _ in cases}
    per_chunk = (args.steps + args.chunks - 1) // args.chunks
    for c in range(args.chunks):
        for name, fmt, st, feed, link in opened:
            t, r = time_case(st, fmt, feed, per_chunk)
            us[name].append(t); rows[name] += int(r)
    for name, fmt, st, feed, link in opened:
        t = np.concatenate(us[name])
        r = dict(case=name, group=gname, format=fmt, steps=int(t.size), p50_ms=float(np.percentile(t, 50)) / 1e3, p99_ms=float(np.percentile(t, 99)) / 1e3,
                 mean_ms=float(t.mean()) / 1e3, rows=rows[name], link_bytes_per_step=int(link), input_stride=st.input_stride, input_stride_bytes=st.input_stride_bytes)
        print(json.dumps(r), flush=True)
        res.append(r)
        st.close()
by = {r["case"]: r for r in res}
if "i16" in by:
    spread = abs(by["f32_a"]["p50_ms"] - by["f32_b"]["p50_ms"])
    excess = by["i16"]["p50_ms"] - by["f32_a"]["p50_ms"]
    verdict = dict(case="verdict", spread_ms=spread, i16_minus_f32_ms=excess, holds=bool(excess <= spread))
    print(json.dumps(verdict), flush=True)
    res.append(verdict)
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)

#!/usr/bin/env python3
"""One wsa_batch_classify_ensemble against as many consecutive wsa_batch_classify calls, on bench.py's level-13 batch (config 3:
1024 clips x 10 s @16 kHz, synth seed 1000) with the six-shape ensemble: the app's models 1 (53-256-64-16-4) and 2 (53-4-4) and four
seeded 53-512-512-8 networks (the shape of models 4 .. 7).  Each of `--iters` iterations is timed on its own between two events on
the run's stream; min / median / max of both paths.  Then the step latency (p50 / p99 of wsa_stream_time_steps) of 512 x 48 kHz
streams with no model, with model 1 and with the ensemble.  Prints one JSON line.

    python3 tools/ensemble_probe.py [--clips 1024] [--seconds 10] [--iters 50] [--streams 512] [--steps 2000] [--warmup 200]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(us):
    import numpy as np
    return {"min_us": float(np.min(us)), "median_us": float(np.median(us)), "max_us": float(np.max(us))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--stream-seconds", type=float, default=20.0, help="length of the synthetic signal each stream loops over")
    a = ap.parse_args()
    import numpy as np
    import torch
    from webspeechanalyzer_amd import Analyzer, Config
    from webspeechanalyzer_amd.synth import synth_clips
    from tests.classify_ref import seeded_spec
    nn = os.path.join(ROOT, "tests", "golden", "nn")
    srcs = [os.path.join(nn, "1", "cats_emotion"), os.path.join(nn, "2", "cats_emotion")] + [seeded_spec(seed=k) for k in (5, 6, 7, 8)]
    out = {}

    fs = 16000
    ns = int(a.seconds * fs)
    pcm = synth_clips(a.clips, ns, fs=fs, seed=1000, device="cuda")
    an = Analyzer(Config(output_level=13))
    models = [an.load_model(s) for s in srcs]
    ens = an.ensemble(models)
    b = an.batch([ns] * a.clips, fs)
    s = torch.cuda.current_stream()
    b.run(pcm.data_ptr(), pcm.stride(0), s.cuda_stream)
    rows = int(b.device_result(s.cuda_stream).n_rows)

    def sequential():
        for m in models:
            b.classify(m, s.cuda_stream)

    def grouped():
        b.classify_ensemble(ens, s.cuda_stream)

    def timed(fn):
        for _ in range(5):
            fn()
        s.synchronize()
        us = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        return _stats(us)

    grouped()
    r = b.ensemble_classes(s.cuda_stream)
    seq, grp = timed(sequential), timed(grouped)
    spread = seq["max_us"] - seq["min_us"]
    out["batch"] = {"workload": f"{a.clips} clips x {a.seconds:g} s @16 kHz, level 13", "rows": rows, "callbacks": int(len(r["cb"])), "iters": a.iters,
                    "members": [m.spec.units for m in models], "sequential": seq, "ensemble": grp, "sequential_spread_us": spread,
                    "ensemble_median_below_sequential_by_us": seq["median_us"] - grp["median_us"],
                    "faster_by_more_than_the_spread": bool(seq["median_us"] - grp["median_us"] > spread),
                    "cb_db_counts": {str(k): int(v) for k, v in zip(*np.unique(r["cb_db"], return_counts=True))}}
    b.close(); ens.close()
    for m in models:
        m.close()
    an.close()
    del pcm

    if a.steps <= 0:                              # (--steps 0: the batch part alone, e.g. under a kernel trace)
        print(json.dumps(out))
        return
    sfs = 48000
    an = Analyzer(Config(output_level=13))
    models = [an.load_model(x) for x in srcs]
    ens = an.ensemble(models)
    st = an.streams(a.streams, sfs, frames_per_step=1, max_span_frames=1024)
    st.enable_graph(True)
    sps = st.samples_per_step
    loop = max(1, int(a.stream_seconds * sfs) // sps)
    feed = synth_clips(a.streams, loop * sps, fs=sfs, seed=5, device="cuda").cpu().numpy().reshape(a.streams, loop, sps).transpose(1, 0, 2).copy()
    out["streams"] = {"workload": f"{a.streams} streams x {sfs} Hz, 1 frame per step, graph on, level 13", "steps": a.steps, "warmup": a.warmup,
                      "period_ms": 1e3 * sps / sfs, "runs": {}}
    for name in ("none", "model 1", "six-shape ensemble"):
        if name == "model 1":
            st.set_model(models[0])
        elif name != "none":
            st.set_ensemble(ens)
        st.time_steps(a.warmup, feed)
        us, nrows = st.time_steps(a.steps, feed)
        out["streams"]["runs"][name] = {"p50_ms": float(np.percentile(us, 50)) / 1e3, "p99_ms": float(np.percentile(us, 99)) / 1e3,
                                        "mean_ms": float(us.mean()) / 1e3, "rows_per_step": nrows / a.steps}
        st.set_model(None); st.set_ensemble(None)
    st.close(); ens.close()
    for m in models:
        m.close()
    an.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

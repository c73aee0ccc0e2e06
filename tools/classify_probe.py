#!/usr/bin/env python3
"""K6 + K6b time on bench.py's level-13 batch (config 3: 1024 clips x 10 s @16 kHz, synth seed 1000): one run, then `--iters`
wsa_batch_classify calls between two events on the run's stream, for the app's model 1 (53-256-64-16-4) and a seeded
53-512-512-8 network (the shape of models 4 .. 7).  Prints one JSON line.

    python3 tools/classify_probe.py [--clips 1024] [--seconds 10] [--iters 50]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    import numpy as np
    import torch
    from webspeechanalyzer_amd import Analyzer, Config
    from webspeechanalyzer_amd.synth import synth_clips
    from tests.classify_ref import seeded_spec
    fs = 16000
    ns = int(a.seconds * fs)
    pcm = synth_clips(a.clips, ns, fs=fs, seed=1000, device="cuda")
    an = Analyzer(Config(output_level=13))
    b = an.batch([ns] * a.clips, fs)
    s = torch.cuda.current_stream()
    b.run(pcm.data_ptr(), pcm.stride(0), s.cuda_stream)
    rows = int(b.device_result(s.cuda_stream).n_rows)
    out = {"workload": f"{a.clips} clips x {a.seconds:g} s @16 kHz, level 13", "rows": rows, "iters": a.iters, "models": {}}
    for name, src in (("1/cats_emotion", os.path.join(ROOT, "tests", "golden", "nn", "1", "cats_emotion")), ("seeded 53-512-512-8", seeded_spec())):
        m = an.load_model(src)
        b.classify(m, s.cuda_stream)
        r = b.classes(s.cuda_stream)
        flops = 2 * rows * sum(int(k.size) for k in m.spec.kernels)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(5):
            b.classify(m, s.cuda_stream)
        e0.record(s)
        for _ in range(a.iters):
            b.classify(m, s.cuda_stream)
        e1.record(s)
        e1.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.iters
        out["models"][name] = {"us_per_classify_and_fold": us, "gflop": flops / 1e9, "tflops": flops / us / 1e6,
                               "callbacks": int(len(r["cb"])), "null_labels": int(np.sum(r["cb_label"] == -1))}
        m.close()
    b.close(); an.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

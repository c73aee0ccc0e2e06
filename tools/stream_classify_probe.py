#!/usr/bin/env python3
"""Step latency of BASELINE config 5 (512 streams x 48 kHz, one 25 ms frame per step, graph on) with the classifier inside the step
(wsa_stream_set_model): p50 / p99 of wsa_stream_time_steps (step_host + collect, timed inside the library) without a model, with the
app's model 1 (53-256-64-16-4) and with a seeded 53-512-512-8 network (the shape of models 4 .. 7).  The streams loop over a synthetic
signal (seed 5, as bench_stream.py).  Prints one JSON line.

    python3 tools/stream_classify_probe.py [--streams 512] [--level 13] [--steps 4000] [--warmup 400]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--fs", type=int, default=48000)
    ap.add_argument("--level", type=int, default=13)
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=400)
    ap.add_argument("--seconds", type=float, default=20.0, help="length of the synthetic signal each stream loops over")
    a = ap.parse_args()
    import numpy as np
    from webspeechanalyzer_amd import Analyzer, Config
    from webspeechanalyzer_amd.synth import synth_clips
    from tests.classify_ref import seeded_spec
    an = Analyzer(Config(output_level=a.level))
    st = an.streams(a.streams, a.fs, frames_per_step=1, max_span_frames=1024)
    st.enable_graph(True)
    sps = st.samples_per_step
    loop = max(1, int(a.seconds * a.fs) // sps)
    feed = synth_clips(a.streams, loop * sps, fs=a.fs, seed=5, device="cuda").cpu().numpy().reshape(a.streams, loop, sps).transpose(1, 0, 2).copy()
    out = {"workload": f"{a.streams} streams x {a.fs} Hz, 1 frame per step, graph on, level {a.level}", "steps": a.steps, "warmup": a.warmup,
           "period_ms": 1e3 * sps / a.fs, "runs": {}}
    models = [("none", None), ("1/cats_emotion", os.path.join(ROOT, "tests", "golden", "nn", "1", "cats_emotion")), ("seeded 53-512-512-8", seeded_spec())]
    for name, src in models:
        m = an.load_model(src) if src is not None else None
        st.set_model(m)
        st.time_steps(a.warmup, feed)
        us, rows = st.time_steps(a.steps, feed)
        out["runs"][name] = {"p50_ms": float(np.percentile(us, 50)) / 1e3, "p99_ms": float(np.percentile(us, 99)) / 1e3,
                             "mean_ms": float(us.mean()) / 1e3, "rows_per_step": rows / a.steps}
        st.set_model(None)
        if m is not None:
            m.close()
    st.close(); an.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

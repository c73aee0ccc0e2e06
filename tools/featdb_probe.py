"""What handing a run's rows to a trainer costs, through the host and on the device (specification FD-1, profiles/featdb.md).

One level-13 run of 1024 ten-second clips, then two ways from its rows to a ready trainer over all of them, each timed with the host's
clock after its own warm-up:
  host    wsa_batch_copy_rows (metadata and features) followed by wsa_trainer_create on the copied rows — the code of the commit before
          the device feature DB, unchanged by it: the yardstick;
  device  wsa_featdb_append_batch, wsa_batch_copy_rows for the metadata alone, then wsa_trainer_create_db.
Prints both times, the row count and the bytes each path moves over PCIe.  python tools/featdb_probe.py [--clips N] [--seconds S] [--reps R]

--only stream (specification FD-2, profiles/stream_featdb.md): what collecting a live stream set's rows costs per step.  BASELINE config 5
(512 streams x 48 kHz, one frame per step, level 13), one stream set in one process, `--rounds` rounds alternating
  a       nothing attached                                   (wsa_stream_time_steps)
  b       a device DB attached: the step stores its rows     (wsa_stream_time_steps)
  a_loop  nothing attached, step + collect called from here  (the yardstick of c: the same loop without the append)
  c       nothing attached, wsa_featdb_append_host of the collected rows after every step, inside the timed region
and prints p50 / p99 of every round in microseconds.  [--streams N] [--steps K] [--rounds R]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from webspeechanalyzer_amd import capi, nnmodel, train  # noqa: E402
from webspeechanalyzer_amd.synth import synth_clips  # noqa: E402


def stream_probe(args):
    import ctypes
    import torch
    n, fs = args.streams, 48000
    an = capi.Analyzer(capi.Config(output_level=13), device=0)
    st = an.streams(n, fs, frames_per_step=1, max_span_frames=1024)
    st.enable_graph(True)
    sps = st.samples_per_step
    loop = max(1, int(5 * fs) // sps)
    feed = np.ascontiguousarray(synth_clips(n, loop * sps, fs=fs, seed=5, device="cuda").cpu().numpy().reshape(n, loop, sps).transpose(1, 0, 2))
    db = an.device_db(53, (args.steps + args.warmup) * 256)
    hin = st.host_input()
    L, h = st.L, st.h
    out = capi._StreamRows()
    state = dict(k=0)

    def timed(n_steps):
        us, _ = st.time_steps(n_steps, feed)
        return us

    def loop_steps(n_steps, append):
        us = np.zeros(n_steps)
        for i in range(n_steps):
            hin[:] = feed[state["k"] % loop]
            state["k"] += 1
            t0 = time.perf_counter()
            rc = L.wsa_stream_step_host(h, None, None) or L.wsa_stream_collect(h, None, ctypes.byref(out))
            if append and out.n_rows and not rc:
                rc = L.wsa_featdb_append_host(db.h, out.row_feat, min(out.n_rows, 1024), None)
            us[i] = (time.perf_counter() - t0) * 1e6
            if rc:
                an._check(rc)
        return us

    def variant(name):
        db.clear()
        if name == "b":
            st.set_featdb(db)
        run = (lambda k: timed(k)) if name in ("a", "b") else (lambda k: loop_steps(k, name == "c"))
        run(args.warmup)                                 # the graph is captured again after an attach or a detach
        us = run(args.steps)
        rows = db.count
        if name == "b":
            st.set_featdb(None)
        return float(np.percentile(us, 50)), float(np.percentile(us, 99)), rows

    print(f"{n} streams x {fs} Hz, level 13, 1 frame per step, {args.steps} steps per round after {args.warmup} of warm-up; microseconds")
    res = {v: [] for v in ("a", "b", "a_loop", "c")}
    for r in range(args.rounds):
        for v in res:
            p50, p99, rows = variant(v)
            res[v].append((p50, p99))
            print(f"round {r} {v:7s} p50 {p50:8.1f}  p99 {p99:8.1f}  DB rows {rows}")
    for v in res:
        a = np.array(res[v])
        print(f"{v:7s} p50 median {np.median(a[:, 0]):8.1f} (min {a[:, 0].min():.1f}, max {a[:, 0].max():.1f})   p99 median {np.median(a[:, 1]):8.1f} (min {a[:, 1].min():.1f}, max {a[:, 1].max():.1f})")
    db.close(); st.close(); an.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["batch", "stream"], default="batch")
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    if args.only == "stream":
        return stream_probe(args)
    import torch
    fs = 16000
    ns = int(args.seconds * fs)
    an = capi.Analyzer(capi.Config(output_level=13), device=0)
    s = torch.cuda.current_stream().cuda_stream
    pcm = synth_clips(args.clips, ns, fs=fs, seed=3, device="cuda")
    b = an.batch([ns] * args.clips, fs)
    b.run(pcm.data_ptr(), pcm.stride(0), s)
    n = b.device_result(s).n_rows
    db = an.device_db(53, n)
    db.append_batch(b, s)
    lo, hi = db.ranges(None, s)
    hi = np.where(hi > lo, hi, lo + 1.0)                 # a column the synthetic clips leave constant still has to normalise
    units = [53, 8, 3]
    ks, bs = train.glorot_init(units, 0)
    spec = nnmodel.ModelSpec(units, ["relu", "softmax"], ks, bs, lo, hi, ["a", "b", "c"])
    labels = np.arange(n, dtype=np.int32) % 3
    rows = np.arange(n, dtype=np.uint32)
    n_val = n // 10

    # like for like: both paths bring the 32 B of metadata per row to the host (a host needs them for file, part tag and time), into
    # arrays allocated once; neither copies the segment table or the offsets
    meta, feat = np.zeros((n, 8), np.int32), np.zeros((n, 53), np.float64)

    def host():
        an._check(an.L.wsa_batch_copy_rows(b.h, s, meta.ctypes.data, feat.ctypes.data, n, None, 0, None, None))
        tr = an.trainer(spec, feat, labels, n_val, 32, 0.2)
        tr.close()

    def device():
        db.clear()
        db.append_batch(b, s)
        an._check(an.L.wsa_batch_copy_rows(b.h, s, meta.ctypes.data, None, n, None, 0, None, None))
        tr = db.trainer(spec, rows, labels, n_val, 32, 0.2)
        tr.close()

    out = {}
    for name, fn in (("host", host), ("device", device)):
        fn(); fn()                                       # warm-up of its own
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = (min(ts), float(np.median(ts)))
    host_bytes = n * (53 * 8 + 8 * 4) + n * 53 * 8 + n * 4            # rows and metadata up, rows and labels down
    dev_bytes = n * 8 * 4 + n * 4 + n * 4                               # the metadata up, the row list and labels down (levels 5 / 13: the kept list is the identity, filled on the host)
    print(f"clips {args.clips} x {args.seconds:g} s, level 13: {n} rows of 53 features")
    print(f"host path   (copy_rows + trainer_create):       min {out['host'][0]:.2f} ms, median {out['host'][1]:.2f} ms, {host_bytes} bytes over PCIe")
    print(f"device path (append_batch + trainer_create_db): min {out['device'][0]:.2f} ms, median {out['device'][1]:.2f} ms, {dev_bytes} bytes over PCIe")
    db.close(); b.close(); an.close()


if __name__ == "__main__":
    main()

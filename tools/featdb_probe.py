"""What handing a run's rows to a trainer costs, through the host and on the device (specification FD-1, profiles/featdb.md).

One level-13 run of 1024 ten-second clips, then two ways from its rows to a ready trainer over all of them, each timed with the host's
clock after its own warm-up:
  host    wsa_batch_copy_rows (metadata and features) followed by wsa_trainer_create on the copied rows — the code of the commit before
          the device feature DB, unchanged by it: the yardstick;
  device  wsa_featdb_append_batch, wsa_batch_copy_rows for the metadata alone, then wsa_trainer_create_db.
Prints both times, the row count and the bytes each path moves over PCIe.  python tools/featdb_probe.py [--clips N] [--seconds S] [--reps R]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from webspeechanalyzer_amd import capi, nnmodel, train  # noqa: E402
from webspeechanalyzer_amd.synth import synth_clips  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
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

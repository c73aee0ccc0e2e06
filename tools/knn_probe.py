#!/usr/bin/env python3
"""K9 (wsa_knn_classify_rows) timed with device events: `--store` stored rows x `--queries` query rows of `--width` features, k
neighbours, rows drawn inside the ranges of the shipped model 1 (tests/knn_cases.py).  Defaults are the project's usual sizes: the
74 249 stored syllables x the 15 907 rows of a 1024-clip batch x 53 features, k = 10; `--small` adds one small size.  Each of `--iters`
calls is timed on its own between two events on the call's stream, after `--warmup` untimed calls; min / median / max.  Beside them the
two floors the time is read against (peaks from the MI355X data sheet: 157.3 TFLOP/s f32 matrix, 8 TB/s HBM):
  arithmetic  2 N Q W flops at the f32 MFMA rate (W as the kernel pads it, to a multiple of 8)
  bytes       the store streamed once per resident query tile: ceil(Q / query tile) x N x padded W x 4 bytes (it is re-read from the
              last-level cache, not from HBM, when it fits there: the floor is stated at the HBM rate all the same)
Prints one JSON line.

    python3 tools/knn_probe.py [--store 74249] [--queries 15907] [--width 53] [--k 10] [--iters 20] [--warmup 3] [--small 2000x512]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA, PEAK_HBM = 157.3e12, 8.0e12


def measure(torch, an, store_n, query_n, width, k, iters, warmup, classes=5):
    import numpy as np
    from tests import knn_cases
    from webspeechanalyzer_amd.capi import KnnStore
    _, qt = KnnStore.tile_info()
    store = torch.from_numpy(knn_cases.draw(width, store_n, 11)).cuda()
    cls = torch.from_numpy((knn_cases.mix(np.arange(store_n), 1, 11) % np.uint64(classes)).astype(np.int32)).cuda()
    queries = torch.from_numpy(knn_cases.draw(width, query_n, 12, first=10 ** 6)).cuda()
    s = torch.cuda.current_stream()
    st = an.knn_store(width, classes, store_n)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    st.add(store.data_ptr(), cls.data_ptr(), store_n, s.cuda_stream)
    e1.record(s)
    e1.synchronize()
    add_ms = e0.elapsed_time(e1)
    label = torch.empty(query_n, dtype=torch.int32, device="cuda")
    conf = torch.empty((query_n, classes), dtype=torch.float64, device="cuda")
    nbr = torch.empty((query_n, k), dtype=torch.int32, device="cuda")
    sim = torch.empty((query_n, k), dtype=torch.float32, device="cuda")

    def call():
        st.classify_rows(queries.data_ptr(), query_n, k, label.data_ptr(), conf.data_ptr(), nbr.data_ptr(), sim.data_ptr(), s.cuda_stream)

    for _ in range(warmup):
        call()
    s.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        call()
        e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    wp = (width + 7) & ~7
    flops = 2.0 * store_n * query_n * wp
    streamed = float(-(-query_n // qt)) * store_n * wp * 4
    floor_flops_ms, floor_bytes_ms = 1e3 * flops / PEAK_F32_MFMA, 1e3 * streamed / PEAK_HBM
    med = float(np.median(ms))
    out = dict(store=store_n, queries=query_n, width=width, k=k, iters=iters, add_ms=add_ms,
               classify_ms=dict(min=float(np.min(ms)), median=med, max=float(np.max(ms))),
               flops=flops, bytes_streamed=streamed, floor_arithmetic_ms=floor_flops_ms, floor_bytes_ms=floor_bytes_ms,
               tflops_at_median=flops / (med * 1e-3) / 1e12, share_of_the_larger_floor=max(floor_flops_ms, floor_bytes_ms) / med,
               label_counts=np.bincount(label.cpu().numpy(), minlength=classes).tolist())
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", type=int, default=74249)
    ap.add_argument("--queries", type=int, default=15907)
    ap.add_argument("--width", type=int, default=53)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", default="2000x512", help="STORExQUERIES of one small size measured as well ('' for none)")
    a = ap.parse_args()
    import torch
    from webspeechanalyzer_amd import Analyzer, Config
    if not torch.cuda.is_available():
        sys.exit("knn_probe needs a GPU: a CPU run says nothing about these times")
    an = Analyzer(Config(output_level=13))
    out = {"usual": measure(torch, an, a.store, a.queries, a.width, a.k, a.iters, a.warmup)}
    if a.small:
        n, q = (int(v) for v in a.small.split("x"))
        out["small"] = measure(torch, an, n, q, a.width, a.k, a.iters, a.warmup)
    an.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

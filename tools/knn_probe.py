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

`--few 16,64,256,1024` instead measures the launches of a stream step's row counts against the same store: K9 (wsa_knn_classify_rows) and
K9s (partial + merge through wsa_debug_knn_split, the slice count its rule picks for that many rows, or `--slices`), both event-timed, and checks that the two gave the
same bits.  `--step` instead times the stream step of BASELINE config 5 (512 streams x 48 kHz, one frame per graph-replayed step, here at
output_level 13) inside libwsa (wsa_stream_time_steps) with nothing attached, with `--model` attached and with the `--store` rows
attached: p50 / p99 in ms against the 25 ms a step represents.  (profiles/knn_stream.md)

    python3 tools/knn_probe.py --few 16,64,256,1024 [--iters 10]
    python3 tools/knn_probe.py --step [--model tests/golden/nn/1/cats_emotion] [--steps 2000]
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


def _stats(ms):
    import numpy as np
    return dict(min=float(np.min(ms)), median=float(np.median(ms)), max=float(np.max(ms)))


def rule_slices(n_cu, store_n, rows, k):
    """K9s' slice count as include/wsa.h states it (the library applies it when a store is attached or `slices` is 0)"""
    q_tiles, tiles = -(-max(rows, 1) // 64), -(-store_n // 64)
    by_scratch = (64 << 20) // (max(rows, 1) * (12 * k + 4))
    return max(1, min(-(-2 * n_cu // q_tiles), -(-tiles // 4), 256, by_scratch))


def measure_few(torch, an, store_n, counts, width, k, iters, warmup, slices=0, classes=5):
    """K9 and K9s at a stream step's row counts against one store"""
    import numpy as np
    from tests import knn_cases
    from webspeechanalyzer_amd import capi
    store = torch.from_numpy(knn_cases.draw(width, store_n, 11)).cuda()
    cls = torch.from_numpy((knn_cases.mix(np.arange(store_n), 1, 11) % np.uint64(classes)).astype(np.int32)).cuda()
    s = torch.cuda.current_stream()
    st = an.knn_store(width, classes, store_n)
    st.add(store.data_ptr(), cls.data_ptr(), store_n, s.cuda_stream)
    s.synchronize()
    out = []
    for q in counts:
        queries = torch.from_numpy(knn_cases.draw(width, q, 12, first=10 ** 6)).cuda()
        tabs = [dict(label=torch.empty(q, dtype=torch.int32, device="cuda"), conf=torch.empty((q, classes), dtype=torch.float64, device="cuda"),
                     nbr=torch.empty((q, k), dtype=torch.int32, device="cuda"), sim=torch.empty((q, k), dtype=torch.float32, device="cuda")) for _ in range(2)]
        ptrs = [[t[n].data_ptr() for n in ("label", "conf", "nbr", "sim")] for t in tabs]
        for _ in range(warmup):
            st.classify_rows(queries.data_ptr(), q, k, *ptrs[0], s.cuda_stream)
        s.synchronize()
        ms = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            st.classify_rows(queries.data_ptr(), q, k, *ptrs[0], s.cuda_stream)
            e1.record(s)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        chosen = slices or rule_slices(torch.cuda.get_device_properties(0).multi_processor_count, store_n, q, k)
        for _ in range(warmup):                                 # (the first call allocates the scratch table, which stays with the store)
            capi.debug_knn_split(st, queries.data_ptr(), q, k, chosen, *ptrs[1], s.cuda_stream)
        s.synchronize()
        split_ms = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            capi.debug_knn_split(st, queries.data_ptr(), q, k, chosen, *ptrs[1], s.cuda_stream)
            e1.record(s)
            e1.synchronize()
            split_ms.append(e0.elapsed_time(e1))
        same = all(torch.equal(tabs[0][n].view(torch.uint8), tabs[1][n].view(torch.uint8)) for n in tabs[0])
        out.append(dict(store=store_n, queries=q, width=width, k=k, iters=iters, slices=chosen, k9_ms=_stats(ms), k9s_ms=_stats(split_ms), same_bits=bool(same)))
    st.close()
    return out


def measure_step(torch, store_n, k, steps, warmup, model_dir, n=512, fs=48000, classes=5):
    """the step of config 5 at level 13: nothing attached, the model, the store"""
    import numpy as np
    from tests import knn_cases
    from webspeechanalyzer_amd import Analyzer, Config
    from webspeechanalyzer_amd.synth import synth_clips
    an = Analyzer(Config(output_level=13))
    s = torch.cuda.current_stream()
    store = torch.from_numpy(knn_cases.draw(53, store_n, 11)).cuda()
    cls = torch.from_numpy((knn_cases.mix(np.arange(store_n), 1, 11) % np.uint64(classes)).astype(np.int32)).cuda()
    ks = an.knn_store(53, classes, store_n)
    ks.add(store.data_ptr(), cls.data_ptr(), store_n, s.cuda_stream)
    s.synchronize()
    model = an.load_model(model_dir)
    out = {}
    for what in ("nothing", "model", "store"):
        st = an.streams(n, fs, frames_per_step=1, max_span_frames=1024)
        st.enable_graph(True)
        if what == "model":
            st.set_model(model)
        if what == "store":
            st.set_knn(ks, k)
        sps = st.samples_per_step
        loop = 400                                              # 10 s of signal per stream, cycled (bench.py's feed)
        feed = synth_clips(n, loop * sps, fs=fs, seed=5, device="cuda").cpu().numpy().reshape(n, loop, sps).transpose(1, 0, 2).copy()
        st.time_steps(warmup, feed)
        us, rows = st.time_steps(steps, feed)
        ms = us / 1e3
        out[what] = dict(steps=steps, rows=int(rows), p50_ms=float(np.percentile(ms, 50)), p99_ms=float(np.percentile(ms, 99)), max_ms=float(ms.max()),
                         step_represents_ms=1e3 * sps / fs)
        if what == "store":
            out[what]["slices"] = st.knn_classes()["slices"]
        st.close()
    model.close(); ks.close(); an.close()
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
    ap.add_argument("--few", default="", help="comma-separated query row counts: K9 against K9s at each")
    ap.add_argument("--slices", type=int, default=0, help="--few: a forced slice count (0: K9s' rule)")
    ap.add_argument("--step", action="store_true", help="time the stream step of config 5 with nothing, a model and the store attached")
    ap.add_argument("--model", default=os.path.join(ROOT, "tests", "golden", "nn", "1", "cats_emotion"))
    ap.add_argument("--steps", type=int, default=2000)
    a = ap.parse_args()
    import torch
    from webspeechanalyzer_amd import Analyzer, Config
    if not torch.cuda.is_available():
        sys.exit("knn_probe needs a GPU: a CPU run says nothing about these times")
    if a.step:
        print(json.dumps({"step": measure_step(torch, a.store, a.k, a.steps, 200, a.model)}))
        return
    an = Analyzer(Config(output_level=13))
    if a.few:
        print(json.dumps({"few": measure_few(torch, an, a.store, [int(v) for v in a.few.split(",")], a.width, a.k, a.iters, a.warmup, a.slices)}))
        an.close()
        return
    out = {"usual": measure(torch, an, a.store, a.queries, a.width, a.k, a.iters, a.warmup)}
    if a.small:
        n, q = (int(v) for v in a.small.split("x"))
        out["small"] = measure(torch, an, n, q, a.width, a.k, a.iters, a.warmup)
    an.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

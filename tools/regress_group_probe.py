#!/usr/bin/env python3
"""Regression groups timed on the GPU (profiles/regress_group.md).  Three heads, each the app's default ords stack (53-64-16-1 sigmoid,
nn_default_options_ords) with seeded weights and the input ranges of the 50-row training fixture.

  --batch   1024 synthetic clips x 10 s at 16 kHz, output_level 13.  After one wsa_batch_run, each of `--iters` repeats is timed between two
            events on the call's stream, after `--warmup` untimed ones: `group` = wsa_batch_regress_group (the grouped K6 launch, the fold
            RG-1 and its compaction), `single` = three wsa_batch_regress calls, one per head (values only: there is no fold to call).  The
            two are timed in turns; `--what single` times the three calls alone (all a library before regression groups can do).  Also
            says whether every head's values are the single calls' bits.  `group_rows` / `single_rows` are the launches alone, in turns again:
            wsa_regress_group_rows against three wsa_regress_rows over the batch's rows as dense device rows.  With `--level 5` the batch has
            segment rows and no fold, so `group` is the batch's grouped launch alone against the three single launches.
  --step    the stream step of BASELINE config 5 (512 streams x 48 kHz, one frame per graph-replayed step) at output_level 13 inside libwsa
            (wsa_stream_time_steps): nothing attached, and the 3-head group attached (`--what nothing` for the first alone).

Prints one JSON line.

    python3 tools/regress_group_probe.py --batch [--iters 10] [--what both|single] [--level 13|5]
    python3 tools/regress_group_probe.py --step [--steps 2000] [--what both|nothing]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ms):
    import numpy as np
    return dict(min=float(np.min(ms)), median=float(np.median(ms)), max=float(np.max(ms)))


def head_specs():
    import numpy as np
    from tests import regress_ref
    from webspeechanalyzer_amd import nnmodel, train
    fx = regress_ref.load_fixture()
    mn, mx = np.array(fx["in_min"], np.float64), np.array(fx["in_max"], np.float64)
    out = []
    for seed, (lo, hi) in ((1, (-1.0, 1.0)), (2, (0.0, 1.0)), (3, (1.0, 9.0))):           # V, A, D
        ks, bs = train.glorot_init([53, 64, 16, 1], seed)
        out.append(nnmodel.ModelSpec([53, 64, 16, 1], ["sigmoid"] * 3, ks, bs, mn, mx, [], lo, hi))
    return out


def _timed(torch, s, call, iters):
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        call()
        e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def measure_batch(torch, what, iters, warmup, level=13, n=1024, seconds=10, fs=16000):
    from webspeechanalyzer_amd import Analyzer, Config
    from webspeechanalyzer_amd.synth import synth_clips
    an = Analyzer(Config(output_level=level))
    s = torch.cuda.current_stream()
    pcm = synth_clips(n, seconds * fs, fs=fs, seed=5, device="cuda")
    models = [an.load_model(sp) for sp in head_specs()]
    b = an.batch([pcm.shape[1]] * n, fs)
    b.run(pcm.data_ptr(), pcm.stride(0), s.cuda_stream)
    rows = len(b.rows(s.cuda_stream)["meta"])

    def single():
        for m in models:
            b.regress(m, stream=s.cuda_stream)

    out = dict(level=level, clips=n, seconds=seconds, rows=rows, iters=iters)
    group = None
    if what == "both":
        group = an.regress_group(models)

        def grouped():
            b.regress_group(group, s.cuda_stream)
        for _ in range(warmup):
            grouped(); single()
        s.synchronize()
        g_ms, s_ms = [], []
        for _ in range(iters):                                   # in turns: the two see the same machine
            g_ms += _timed(torch, s, grouped, 1)
            s_ms += _timed(torch, s, single, 1)
        # the launches alone, over the same rows as dense device rows: one grouped launch (wsa_regress_group_rows, its table copied in front)
        # against three wsa_regress_rows launches
        d_feat = int(b.device_result(s.cuda_stream).d_row_feat)
        outs = torch.empty((2, len(models), max(rows, 1)), dtype=torch.float64, device="cuda")

        def grouped_rows():
            group.regress_rows(d_feat, rows, [outs[0, h].data_ptr() for h in range(len(models))], s.cuda_stream)

        def single_rows():
            for h, m in enumerate(models):
                m.regress_rows(d_feat, rows, outs[1, h].data_ptr(), stream=s.cuda_stream)
        for _ in range(warmup):
            grouped_rows(); single_rows()
        s.synchronize()
        gr_ms, sr_ms = [], []
        for _ in range(iters):
            gr_ms += _timed(torch, s, grouped_rows, 1)
            sr_ms += _timed(torch, s, single_rows, 1)
        out.update(group_rows_ms=_stats(gr_ms), single_rows_ms=_stats(sr_ms), rows_same_bits=bool(torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64))))
        grouped()
        got = b.value_fold(s.cuda_stream)
        same = True
        for h, m in enumerate(models):
            b.regress(m, stream=s.cuda_stream)
            same = same and b.values(s.cuda_stream).tobytes() == got["value"][h].tobytes()
        out.update(group_ms=_stats(g_ms), single_ms=_stats(s_ms), callbacks=int(len(got["cb"])) if "cb" in got else 0, same_bits=bool(same))
        group.close()
    else:
        for _ in range(warmup):
            single()
        s.synchronize()
        out.update(single_ms=_stats(_timed(torch, s, single, iters)))
    b.close()
    for m in models:
        m.close()
    an.close()
    return out


def measure_step(torch, what, steps, warmup, n=512, fs=48000):
    import numpy as np
    from webspeechanalyzer_amd import Analyzer, Config
    from webspeechanalyzer_amd.synth import synth_clips
    an = Analyzer(Config(output_level=13))
    models = [an.load_model(sp) for sp in head_specs()]
    group = an.regress_group(models) if what == "both" else None
    out = {}
    for attached in (("nothing", "group", "nothing", "group") if what == "both" else ("nothing", "nothing")):
        st = an.streams(n, fs, frames_per_step=1, max_span_frames=1024)
        st.enable_graph(True)
        if attached == "group":
            st.set_regress(group)
        sps = st.samples_per_step
        loop = 400                                              # 10 s of signal per stream, cycled (bench.py's feed)
        feed = synth_clips(n, loop * sps, fs=fs, seed=5, device="cuda").cpu().numpy().reshape(n, loop, sps).transpose(1, 0, 2).copy()
        st.time_steps(warmup, feed)
        us, rows = st.time_steps(steps, feed)
        ms = us / 1e3
        out.setdefault(attached, []).append(dict(steps=steps, rows=int(rows), p50_ms=float(np.percentile(ms, 50)), p99_ms=float(np.percentile(ms, 99)),
                                                 max_ms=float(ms.max()), step_represents_ms=1e3 * sps / fs))
        st.close()
    if group is not None:
        group.close()
    for m in models:
        m.close()
    an.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--what", default="both", choices=["both", "single", "nothing"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--level", type=int, default=13, choices=[5, 13], help="--batch: the output level; at 5 wsa_batch_regress_group is the grouped launch alone")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("regress_group_probe needs a GPU: a CPU run says nothing about these times")
    out = {}
    if a.batch:
        out["batch"] = measure_batch(torch, "both" if a.what == "both" else "single", a.iters, a.warmup, a.level)
    if a.step:
        out["step"] = measure_step(torch, "both" if a.what == "both" else "nothing", a.steps, 200)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

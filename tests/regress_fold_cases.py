"""Specification RG-1 restated in float64, and the hand-built tables the fold is tested on (tests/test_regress_fold_host.py on
the CPU, tests/test_gpu_regress_group.py through the test entry wsa_debug_regress_fold): row meta [n, 8] i32 (slot 0 the clip or stream, 1 the
callback index si, 3 the syllable's length in frames), H value columns [H, n] f64 and step_s; for streams also the dealing of each stream's
rows over steps with the steps' control bytes.

rg1_ref follows the specification's order literally: Python's float is an IEEE double, every `*`, `+` and `/` below rounds once, math.sqrt is
correctly rounded.  rg1_ref(fused=True) is the WRONG variant that forms v w + S with one rounding (what a contracted multiply-add would do)."""
import math
from fractions import Fraction

import numpy as np

from tests.classify_ref import fixed3

ACTIVE, START, STOP = 1, 2, 4            # WSA_STREAM_ACTIVE / _START / _STOP
NAN = float("nan")


def _fma(a, b, c):
    """a b + c rounded once (float(Fraction) is correctly rounded)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def rg1_ref(meta, values, step_s, run=None, fused=False):
    """One table of rows (a batch's, or one stream step's) in row order.  meta [n, 8], values [H, n]; run: {clip or stream: (A [H], B [H])},
    the running sums to continue from (missing: zeros) — not modified.
    Returns (callbacks [dict(who, si, first, rows, skipped, value [H], weight [H])], run after the table)."""
    meta = np.asarray(meta).reshape(-1, 8)
    values = np.asarray(values, np.float64)
    H = values.shape[0]
    run = {k: (list(a), list(b)) for k, (a, b) in (run or {}).items()}
    cbs = []
    r, n = 0, len(meta)
    while r < n:
        who, si = int(meta[r][0]), int(meta[r][1])
        e = r + 1
        while e < n and int(meta[e][0]) == who and int(meta[e][1]) == si:
            e += 1
        A, B = run.setdefault(who, ([0.0] * H, [0.0] * H))
        d = [fixed3((int(meta[q][3]) + 1) * step_s) for q in range(r, e)]
        seg_weight = 0.0
        for x in d:
            seg_weight = seg_weight + x
        if not seg_weight > 0:
            cbs.append(dict(who=who, si=si, first=r, rows=e - r, skipped=True, value=[NAN] * H, weight=[0.0] * H))
            r = e
            continue
        value, weight = [], []
        for h in range(H):
            S = W = 0.0
            for q in range(r, e):
                v, w = float(values[h][q]), math.sqrt(d[q - r])
                if not math.isfinite(v):
                    continue
                if fused:
                    S, A[h] = _fma(v, w, S), _fma(v, w, A[h])
                else:
                    t = v * w
                    S = S + t
                    A[h] = A[h] + t
                W = W + w
                B[h] = B[h] + w
            value.append(S / W if W != 0 else NAN)
            weight.append(W)
        cbs.append(dict(who=who, si=si, first=r, rows=e - r, skipped=False, value=value, weight=weight))
        r = e
    return cbs, run


def run_value(run, who, H):
    """(run_sum [H], run_weight [H], run_value [H]) of one clip or stream; zeros and NaN where it has none"""
    A, B = run.get(who, ([0.0] * H, [0.0] * H))
    return list(A), list(B), [a / b if b != 0 else NAN for a, b in zip(A, B)]


def rg1_streams(case):
    """A stream case step by step: START (control bit) zeroes the stream's running sums before the step's rows, a stream without rows keeps
    them.  Returns per step (callbacks with `first` counted from the step's first row, run after the step)."""
    H, n = case["values"].shape[0], case["n"]
    run, out, row0 = {}, [], 0
    for off, ctl in zip(case["row_off"], case["ctl"]):
        rows = int(off[-1])
        for s in range(n):
            if int(ctl[s]) & START:
                run[s] = ([0.0] * H, [0.0] * H)
        cbs, run = rg1_ref(case["meta"][row0:row0 + rows], case["values"][:, row0:row0 + rows], case["step_s"], run)
        out.append((cbs, {k: (list(a), list(b)) for k, (a, b) in run.items()}))
        row0 += rows
    return out


# ---- building tables

def _rows(clips, first_si=3):
    """clips: per clip a list of callbacks, each a list of syllable lengths -> (meta [n, 8], row_off [len(clips) + 1])"""
    meta, off = [], [0]
    for c, cbs in enumerate(clips):
        t = 0
        for k, lens in enumerate(cbs):
            for ln in lens:
                meta.append([c, first_si + 2 * k, t, ln, 0, 0, t, ln + 1])
                t += ln + 1
        off.append(len(meta))
    return np.array(meta, np.int32).reshape(-1, 8), np.array(off, np.uint32)


def _values(H, n, seed, lo=0.2, hi=0.8):
    return np.random.default_rng(seed).uniform(lo, hi, (H, n))


def _lens(rng, k, lo=1, hi=40):
    return [int(x) for x in rng.integers(lo, hi, k)]


SIZES = (1, 2, 63, 64, 65, 130)


def batch_cases():
    out = []
    rng = np.random.default_rng(11)
    # every callback size alone in a clip, all of them in one clip (callbacks then straddle the 64-row blocks at every offset), a clip with
    # no rows in the middle and at the end
    clips = [[_lens(rng, k)] for k in SIZES[:3]] + [[]] + [[_lens(rng, k)] for k in SIZES[3:]] + [[_lens(rng, k) for k in SIZES], [_lens(rng, k) for k in reversed(SIZES)], []]
    for H in (1, 3, 8):
        meta, off = _rows(clips)
        out.append(dict(name=f"sizes_H{H}", step_s=0.025, meta=meta, row_off=off, values=_values(H, len(meta), 100 + H)))
    # durations that fixed3 turns into 0: with step_s = 1e-6 a syllable of fewer than 500 frames has d = 0.  Clip 0: a skipped callback between
    # two others, and a callback with a d = 0 row among positive ones; clip 1: only skipped callbacks; clip 2: a skipped callback first
    clips = [[[40000, 2500], [100, 200], [3000], [100, 40000, 300, 700]], [[10], [499 - 1, 3]], [[5], [600, 9000]]]
    meta, off = _rows(clips)
    out.append(dict(name="zero_durations", step_s=1e-6, meta=meta, row_off=off, values=_values(3, len(meta), 7), skipped=4))
    # NaN, +Inf and -Inf in head 1 only; head 2 loses every row of the clip's second callback; head 0 keeps everything
    clips = [[_lens(rng, 5), _lens(rng, 4), _lens(rng, 70)], [_lens(rng, 3)]]
    meta, off = _rows(clips)
    v = _values(3, len(meta), 9)
    v[1, [0, 3, 6, 20, 77]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    v[2, 5:9] = [np.nan, np.inf, -np.inf, np.nan]
    v[1, int(off[1]):] = np.nan                                    # ... and head 1 has no usable row in clip 1 at all
    out.append(dict(name="unusable_rows", step_s=0.025, meta=meta, row_off=off, values=v))
    # values across many magnitudes and signs: most products are inexact, so v w + S rounded once differs from the two roundings
    clips = [[_lens(rng, 9, 1, 400), _lens(rng, 66, 1, 400)], [_lens(rng, 2, 1, 400)]]
    meta, off = _rows(clips)
    v = _values(2, len(meta), 13, -1.0, 1.0) * 10.0 ** np.random.default_rng(14).integers(-3, 4, (2, len(meta)))
    out.append(dict(name="separate_rounding", step_s=0.01, meta=meta, row_off=off, values=v))
    return out


def _deal(case_name, per_stream, H, seed, steps, step_s=0.025):
    """per_stream: per stream its callbacks (lists of lengths), in order; steps: [(rows taken from each stream, control bytes)].  The
    tables hold each step's rows in stream order, one step after the other."""
    n = len(per_stream)
    full, off = _rows(per_stream)
    vals = _values(H, len(full), seed)
    taken = [0] * n
    meta, cols, row_off, ctl = [], [], [], []
    for counts, bytes_ in steps:
        o = [0]
        for s in range(n):
            a = int(off[s]) + taken[s]
            assert a + counts[s] <= int(off[s + 1]), case_name
            meta.extend(full[a:a + counts[s]]); cols.extend(range(a, a + counts[s]))
            taken[s] += counts[s]
            o.append(o[-1] + counts[s])
        row_off.append(o); ctl.append(list(bytes_))
    assert all(taken[s] == int(off[s + 1]) - int(off[s]) for s in range(n)), case_name
    return dict(name=case_name, step_s=step_s, n=n, meta=np.array(meta, np.int32).reshape(-1, 8), values=vals[:, cols],
                row_off=np.array(row_off, np.uint32), ctl=np.array(ctl, np.uint8), whole=(full, off, vals))


def stream_cases():
    out = []
    rng = np.random.default_rng(21)
    A = ACTIVE
    # one row per step (a callback of five rows is then five callbacks of one row, one per step), stream 1 two rows per step
    per = [[_lens(rng, 5), _lens(rng, 1)], [_lens(rng, 4), _lens(rng, 8)]]
    steps = [([1, 2], [A | (START if k == 0 else 0)] * 2) for k in range(6)]
    out.append(_deal("one_row_per_step", per, 3, 31, steps))
    # a callback of 130 rows split 1 + 64 + 65 across steps, with whole callbacks before and after it in the same steps
    per = [[_lens(rng, 2), _lens(rng, 130), _lens(rng, 3)], [_lens(rng, 65)]]
    steps = [([3, 0], [A | START, A | START]), ([64, 65], [A, A]), ([68, 0], [A | STOP, A | STOP])]
    out.append(_deal("callback_split", per, 8, 32, steps))
    # stream 0 gets a START mid-run; stream 1 idles (no rows, not active) between two active steps; stream 2 STOPs, idles, then STARTs
    per = [[_lens(rng, 3), _lens(rng, 2), _lens(rng, 4), _lens(rng, 1)], [_lens(rng, 2), _lens(rng, 2)], [_lens(rng, 3), _lens(rng, 2), _lens(rng, 5)]]
    steps = [([3, 2, 3], [A | START] * 3), ([2, 0, 2], [A, 0, A | STOP]), ([4, 0, 0], [A | START, 0, 0]), ([1, 2, 5], [A | STOP, A | STOP, A | START | STOP])]
    out.append(_deal("restart_idle_stop_start", per, 1, 33, steps))
    # a step with no rows at all, and a START on a stream that has no rows in that step
    per = [[_lens(rng, 2)], [_lens(rng, 3)]]
    steps = [([2, 3], [A | START] * 2), ([0, 0], [A, A | START]), ([0, 0], [0, 0])]
    out.append(_deal("empty_steps", per, 3, 34, steps))
    return out


def model_specs():
    """The fixture models of the GPU tests, as nnmodel.ModelSpecs with the 50-row fixture's input ranges and the output range (0.2, 0.8):
    'tfjs' — the last case of tests/golden/regress_expected.json whose trained weights are kept whole (53-8-1 relu / linear, trained by
    tfjs; the file's very last case keeps only a few kernel rows) — and three seeded train.glorot_init stacks: 53-64-16-1 sigmoid (the app's
    default), 53-8-1 linear, 53-16-1 tanh."""
    from tests import regress_ref, train_ref
    from webspeechanalyzer_amd import nnmodel, train
    fx = regress_ref.load_fixture()
    mn, mx = np.array(fx["in_min"], np.float64), np.array(fx["in_max"], np.float64)
    whole = [c for c in fx["cases"] if "keep_rows" not in c][-1]
    last = train_ref.expected_epochs(whole)[-1]
    specs = dict(tfjs=nnmodel.ModelSpec(list(whole["units"]), list(whole["activations"]), last["kernels"], last["biases"], mn, mx, [], fx["out_min"], fx["out_max"]))
    for name, units, acts, seed in (("sigmoid_64_16", [53, 64, 16, 1], ["sigmoid"] * 3, 1), ("linear_8", [53, 8, 1], ["linear", "linear"], 2),
                                    ("tanh_16", [53, 16, 1], ["tanh", "tanh"], 3)):
        ks, bs = train.glorot_init(units, seed)
        specs[name] = nnmodel.ModelSpec(units, acts, ks, bs, mn, mx, [], fx["out_min"], fx["out_max"])
    return specs

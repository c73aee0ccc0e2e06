"""Two references for the batch rate converter K0 (csrc/resample.hip).

(a) device_forms(): a numpy restatement of the device forms as rs_block and resample_mixed_kernel have them — per run the staged array with its clamp and edge
    rules (16-byte path: whole words and guarded singles; word path), the window start as (int)(pos - lo_taps), the kernel rows a lane holds and re-reads, the
    j loop's break, the runs of a block, the copy run — with a switch for each one-line fault (FAULTS).  Faultless it equals oracle/resample.c bit for bit
    (tests/test_resample_reference.py); the faults show that the cases of tests/resample_cases.py notice each of them.
(b) rs1_longdouble(): RS-1 evaluated from the text of DESIGN.md §3 in numpy.longdouble — the table unrounded, exact products, one final rounding — and the
    running-error bound of the float evaluation against it.
"""
import math

import numpy as np

from tests import resample_cases as rc

RS_TAPS, RS_OFFS = rc.RS_TAPS, rc.RS_OFFS
F32, F64, I64 = np.float32, np.float64, np.int64

# fault -> what the one line becomes
FAULTS = {
    "back-edge-last-dropped": "16-byte path, guarded singles behind the last whole word: `<= q_hi` becomes `< q_hi`",
    "q_hi-one-short": "q_hi = n_in - 2 - lo4",
    "v_lo-rounded-down": "v_lo = q_lo & ~3 (EQUIVALENT: q_lo is a multiple of 4)",
    "rows-not-reloaded": "a lane keeps the rows of its first output of the run",
    "window-start-rounded": "w = (int)rint(pos - lo_taps)",
    "break-left-out": "the j loop runs to J: outputs beyond n_out are written over the sentinel",
    "subnormals-flushed": "inputs and results of the multiply-adds flushed to zero",
    "blend-one-fma": "out = (float)fma(f, s2, (1 - f) * s1)",
    "taps-descending": "the 32 multiply-adds from tap 31 down to tap 0",
    "span-4-short": "rs_xlen(span - 4) samples staged, the rest read as zeros",
    "chunks-first-run-only": "the chunk loop stops after its first run",
    "copy-run-off-by-one": "the copy run ends at n0 + RS_COPY_RUN - 1",
    "copy-bounded-by-n_in": "lim = n_in (EQUIVALENT: resample_length gives n_out == n_in for the copy class)",
}
EQUIVALENT = ("v_lo-rounded-down", "copy-bounded-by-n_in")


def table(fs_in, fs_out):
    """K[33][32] as build_resample_table and oracle/resample.c form it: fp64, rounded once to float"""
    ratio = fs_in / fs_out
    scale = (1.0 / ratio if ratio > 1.0 else 1.0) * 0.9
    pi = 3.14159265358979323846
    K = np.zeros((RS_OFFS + 1, RS_TAPS), F32)
    for o in range(RS_OFFS + 1):
        s = o / RS_OFFS
        for i in range(RS_TAPS):
            pre = pi * (float(i - RS_TAPS // 2) - s)
            x = (float(i) - s) / RS_TAPS
            w = 0.42 - 0.5 * math.cos(2.0 * pi * x) + 0.08 * math.cos(4.0 * pi * x)
            K[o, i] = F32(w * (scale if pre == 0.0 else math.sin(scale * pre) / pre))
    return K


def _flush(a):
    return np.where(np.abs(a) < F32(2.0 ** -126), F32(0) * a, a).astype(F32)


def fma32(x, k, s, ftz=False):
    """fmaf on float32 arrays, exactly: the product is exact in fp64; the sum is rounded to odd in fp64 (TwoSum tells on which side the exact sum lies), which the
    final rounding to float cannot tell from the exact sum (53 >= 24 + 2 bits)"""
    if ftz:
        x, k, s = _flush(x), _flush(k), _flush(s)
    with np.errstate(all="ignore"):
        p = x.astype(F64) * k.astype(F64)
        s64 = s.astype(F64)
        t = p + s64
        bp = t - p
        e = (p - (t - bp)) + (s64 - bp)
        fix = np.isfinite(t) & np.isfinite(e) & (e != 0) & ((t.view(I64) & 1) == 0)
        step = np.where((e > 0) == (t > 0), 1, -1)
        t = (t.view(I64) + np.where(fix, step, 0)).view(F64)
        r = t.astype(F32)
    return _flush(r) if ftz else r


def _fma64(a, b, c):
    """fma on Python floats, exactly rounded: Dekker's exact product, then math.fsum"""
    def split(v):
        t = 134217729.0 * v
        hi = t - (t - v)
        return hi, v - hi
    p = a * b
    if not (math.isfinite(p) and math.isfinite(c)):
        return p + c
    ah, al = split(a)
    bh, bl = split(b)
    pe = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return math.fsum((p, pe, c))


def _stage(x, n_in, r, xlen, path16, faults):
    """s_x0[q] = x[lo4 + q] inside the clip, zeros outside, as the run's path writes it"""
    q = np.arange(xlen, dtype=I64)
    q_lo, q_hi, v_lo, v_hi = r["q_lo"], r["q_hi"], r["v_lo"], r["v_hi"]
    if "q_hi-one-short" in faults:
        q_hi -= 1
        v_hi = (q_hi - 3) & ~3
    if "v_lo-rounded-down" in faults:
        v_lo = q_lo & ~3
    src = np.clip(r["lo4"] + q, 0, max(n_in - 1, 0))
    val = x[src] if n_in else np.zeros(xlen, F32)
    if path16:
        whole = (q >= v_lo) & (q <= v_hi + 3)                       # 16-byte words that lie inside the clip
        back = q <= q_hi if "back-edge-last-dropped" not in faults else np.where(q > v_hi + 3, q < q_hi, q <= q_hi)
        inside = whole | ((q >= q_lo) & back)
    else:
        inside = (q >= q_lo) & (q <= q_hi)
    return np.where(inside, val, F32(0)).astype(F32)


def device_forms(case, x, stride_out, sentinel, aligned=True, faults=(), copy=False):
    """one clip through the device forms -> (row of stride_out floats starting as the sentinel bit pattern, n_out)"""
    faults = set(faults)
    assert faults <= set(FAULTS), faults
    out = np.full(stride_out, sentinel, np.uint32).view(F32)
    n_in, n_out = case.n_in, case.n_out
    if copy:                                                        # resample_mixed_kernel's copy class: RS_COPY_RUN samples per block, bounded by lim
        lim = n_in if "copy-bounded-by-n_in" in faults else min(n_in, n_out)
        for blk in range((n_out + rc.RS_COPY_RUN - 1) // rc.RS_COPY_RUN):
            n0 = blk * rc.RS_COPY_RUN
            end = min(n0 + rc.RS_COPY_RUN - (1 if "copy-run-off-by-one" in faults else 0), lim)
            out[n0:end] = x[n0:end]
        return out, n_out
    p = case.plan
    S, J = p["S"], p["J"]
    K = table(case.fs_in, case.fs_out)
    xlen = rc.rs_xlen(p["span"])
    staged = rc.rs_xlen(p["span"] - 4) if "span-4-short" in faults else xlen
    ftz = "subnormals-flushed" in faults
    for r in rc.iter_runs(p, n_in, n_out):
        if isinstance(r, tuple):
            continue
        if "chunks-first-run-only" in faults and r["c"] > 0:
            continue
        path16 = aligned and r["v_hi"] >= r["v_lo"] and r["q_hi"] >= 3
        s_x = _stage(x, n_in, r, xlen, path16, faults)
        s_x[staged:] = 0
        m = min(S * J, stride_out - r["n0"]) if "break-left-out" in faults else r["m"]
        pos, w, o, f = rc.run_outputs(p, r, m)
        if "window-start-rounded" in faults:
            w = np.rint(pos - float(r["lo4"] + RS_TAPS // 2)).astype(I64)
        rows = o
        if "rows-not-reloaded" in faults:                           # lane t = index % S keeps the row of its j = 0 output
            rows = o[np.arange(m) % S]
        win = s_x[np.clip(w[:, None] + np.arange(RS_TAPS)[None, :], 0, xlen - 1)]
        s1, s2 = np.zeros(m, F32), np.zeros(m, F32)
        for i in (range(RS_TAPS - 1, -1, -1) if "taps-descending" in faults else range(RS_TAPS)):
            s1 = fma32(win[:, i], K[rows, i], s1, ftz)
            s2 = fma32(win[:, i], K[rows + 1, i], s2, ftz)
        with np.errstate(all="ignore"):
            if "blend-one-fma" in faults:
                y = np.array([_fma64(float(b), float(d), (1.0 - float(b)) * float(a)) for a, b, d in zip(s1.astype(F64), f, s2.astype(F64))], F64).astype(F32)
            else:
                y = ((1.0 - f) * s1.astype(F64) + f * s2.astype(F64)).astype(F32)
        out[r["n0"]:r["n0"] + m] = y
    return out, n_out


# ---- (b) RS-1 from DESIGN.md §3, in long double
LD = np.longdouble


def rs1_longdouble(x, fs_in, fs_out):
    """-> (out, mag): out[n] = (1 - f) sum x K[o] + f sum x K[o + 1] with the table unrounded and every product and sum in long double; mag[n] the same
    with |x| |K|.  Positions, o and f are the specification's fp64 values (pos = n * ratio in double is part of RS-1)."""
    ratio = fs_in / fs_out
    scale = LD((1.0 / ratio if ratio > 1.0 else 1.0) * 0.9)
    pi = LD("3.14159265358979323846264338327950288")
    o_ = np.arange(RS_OFFS + 1, dtype=LD)[:, None] / LD(RS_OFFS)
    i_ = np.arange(RS_TAPS, dtype=LD)[None, :]
    pre = pi * (i_ - LD(RS_TAPS // 2) - o_)
    xx = (i_ - o_) / LD(RS_TAPS)
    w = LD("0.42") - LD("0.5") * np.cos(2 * pi * xx) + LD("0.08") * np.cos(4 * pi * xx)
    with np.errstate(all="ignore"):
        K = w * np.where(pre == 0, scale, np.sin(scale * pre) / np.where(pre == 0, LD(1), pre))
    n_out = rc.resample_length(len(x), fs_in, fs_out)
    n = np.arange(n_out, dtype=F64)
    pos = n * ratio
    fl = np.floor(pos)
    vo = (pos - fl) * RS_OFFS
    o = vo.astype(I64)
    f = (vo - o).astype(LD)
    xp = np.concatenate([np.zeros(RS_TAPS, LD), x.astype(LD), np.zeros(RS_TAPS, LD)])
    out, mag = np.zeros(n_out, LD), np.zeros(n_out, LD)
    src = fl.astype(I64) - RS_TAPS // 2 + RS_TAPS
    for i in range(RS_TAPS):
        xi = xp[np.clip(src + i, 0, len(xp) - 1)]
        k = (1 - f) * K[o, i] + f * K[o + 1, i]
        out += xi * k
        mag += np.abs(xi) * ((1 - f) * np.abs(K[o, i]) + f * np.abs(K[o + 1, i]))
    return out, mag


def error_bound(ref, mag):
    """|float evaluation - ref| allowed: 32 multiply-adds of one rounding each and one table rounding per tap give (RS_TAPS + 2) 2^-24 sum |x_i| |K_i| in a
    running-error analysis (the + 2: the fp64 blend and slack for the second-order terms), the final conversion half an ulp of the result; below the normal
    range a rounding is absolute, 2^-149 per tap.  Derived, not tuned."""
    ulp = np.spacing(np.abs(ref).astype(F32)).astype(LD)
    return LD(RS_TAPS + 2) * LD(2.0 ** -24) * mag + ulp / 2 + LD(RS_TAPS) * LD(2.0 ** -149)

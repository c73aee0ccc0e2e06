"""Hand-built clips for the batch rate converter K0 (csrc/resample.hip rs_block, resample_kernel, resample_mixed_kernel) and a geometry model that is worked
out from no kernel output: resample_stride, rs_j, resample_span, rs_xlen and the run arithmetic of rs_block restated in Python integers and fp64.

geometry(case) walks a clip's runs (a run = the S * J outputs a block converts from one staging) and counts the ARMS each run sits on.  Every case name says
which arm it was built for, REQUIRED lists the arms that must occur, and check_cases() (called at import) fails when one of them has count 0 over the whole list
or when any run of any case needs more staged samples than rs_xlen(span) holds.

What the model PROVES UNREACHABLE instead of counting (asserted on every run, UNREACHABLE below gives the reason):
  * q_lo that is no multiple of 4 (lo4 = lo & ~3 is one, and q_lo is -lo4 or 0), so v_lo == q_lo: the 16-byte path has no partial word at the FRONT edge;
  * q_hi < 16 in a run that has outputs (an output's position is below n_in, so its window starts below n_in - 16): `q_hi < 3` never decides the staging path
    and the clip never ends inside a run's first staged word.  The word path is taken for two reasons: the base alignment, and v_hi < v_lo (clips of 1 .. 3 samples).
"""
import math
import zlib
from collections import Counter
from fractions import Fraction

import numpy as np

RS_TAPS, RS_OFFS, RS_STAGED, RS_COPY_RUN = 32, 32, 4300, 8192
TABLE_BYTES = 4 * 2 * RS_OFFS * (RS_TAPS + 1)
MAX_IN, MAX_OUT, MAX_OUT_ROUNDING = 15000, 50000, 1 << 20


# ---- the host plan (csrc/resample.hip), restated
def period(fs_in, fs_out):
    """outputs per period of the conversion, None for a non-integer rate"""
    if fs_in != math.floor(fs_in) or fs_out != math.floor(fs_out) or not (0 < fs_in < 4e9 and 0 < fs_out < 4e9):
        return None
    return int(fs_out) // math.gcd(int(fs_in), int(fs_out))


def _waste(S):
    lanes = (S + 63) // 64 * 64
    return (lanes - S) / lanes


def resample_stride(fs_in, fs_out):
    """-> (S, arm): first / search / long / non-integer"""
    L = period(fs_in, fs_out)
    if L is None:
        return 256, "non-integer"
    if L > 512:
        return 256, "long"
    S0 = L * max(256 // L, 1)
    if _waste(S0) <= 0.2:
        return S0, "first"
    best = S0
    for S in range(L, 513, L):
        if S >= 128 and _waste(S) < _waste(best):
            best = S
    return best, "search"


def rs_j(S, ratio):
    j = float(RS_STAGED) / (float(S) * ratio)
    return 1 if j < 1.0 else (96 if j > 96.0 else int(j))


def resample_span(ratio, S, J):
    return int(math.ceil(float(S * J - 1) * ratio)) + RS_TAPS + 2


def rs_xlen(span):
    return (span + 6) & ~3


def resample_length(n_in, fs_in, fs_out):
    return int(float(n_in) / (float(fs_in) / float(fs_out)))


def plan(fs_in, fs_out, S=0, J=0, C=0):
    """what launch_resample / plan_resample_mixed choose: {S, J, span, block, lds, copy} (+ chunks, ratio); copy only in a mixed batch"""
    ratio = float(fs_in) / float(fs_out)
    S = S if S > 0 else resample_stride(fs_in, fs_out)[0]
    J = J if J > 0 else rs_j(S, ratio)
    span = resample_span(ratio, S, J)
    return dict(S=S, J=J, span=span, block=(S + 63) // 64 * 64, lds=TABLE_BYTES + 4 * rs_xlen(span), copy=0, chunks=C if C > 0 else 1, ratio=ratio)


COPY_PLAN = dict(S=0, J=0, span=0, block=256, lds=0, copy=1)


def plan_row(p):
    return [p["S"], p["J"], p["span"], p["block"], p["lds"], p["copy"]]


# ---- cases
class Case:
    def __init__(self, name, fs_in, fs_out, n_in, S=0, J=0, C=0, sig="edge"):
        self.name, self.fs_in, self.fs_out, self.n_in, self.S, self.J, self.C, self.sig = name, float(fs_in), float(fs_out), int(n_in), S, J, C, sig

    @property
    def n_out(self):
        return resample_length(self.n_in, self.fs_in, self.fs_out)

    @property
    def plan(self):
        return plan(self.fs_in, self.fs_out, self.S, self.J, self.C)

    @property
    def mid(self):
        return self.n_in // 2

    def __repr__(self):
        return self.name


def signal(case):
    """the case's clip.  edge: quiet noise with an impulse on sample 0 and on sample n_in - 1 (a dropped edge sample is one bit pattern away from right)"""
    n, k = case.n_in, case.sig
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    x = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    if n:
        x[-1] = -0.75
        x[0] = 1.0
    if k == "dc":
        x[:] = 1.0
    elif k == "alt":
        x[:] = 1.0
        x[1::2] = -1.0
    elif k == "sub":
        x[:] = np.float32(1e-40)
    elif k == "subimp":
        x[:] = 0.0
        x[case.mid] = np.float32(1e-40)
    elif k == "negzero":
        x[:] = np.float32(-0.0)
    elif k == "nan":
        x[case.mid] = np.nan
    elif k == "inf":
        x[case.mid] = np.inf
    elif k == "big":
        x[:] = np.float32(3e38)
    elif k == "cancel":
        x = _cancelling_pairs(case)
    else:
        assert k == "edge", k
    return x


def _cancelling_pairs(case):
    """Pairs of neighbouring impulses 32 samples apart, the second of each pair sized so that ONE output's blend (1 - f) s1 + f s2 cancels down to the rounding of
    that size: there the rounding of the fp64 product f s2 is 2^-29 of the result instead of 2^-53, and about one such output in a hundred tells the specified
    blend from a contracted one (a single fma); the second impulse's size is picked among its 128 neighbours for that.  Needs the table: the oracle's own formula, in fp64."""
    ratio = case.fs_in / case.fs_out
    scale = (1.0 / ratio if ratio > 1.0 else 1.0) * 0.9

    def K(o, i):
        pi, s = 3.14159265358979323846, o / RS_OFFS
        pre, xx = pi * (float(i - RS_TAPS // 2) - s), (float(i) - s) / RS_TAPS
        return float(np.float32((0.42 - 0.5 * math.cos(2.0 * pi * xx) + 0.08 * math.cos(4.0 * pi * xx)) * (scale if pre == 0.0 else math.sin(scale * pre) / pre)))
    x = np.zeros(case.n_in, np.float32)
    n = np.arange(case.n_out, dtype=np.float64)
    pos = n * ratio
    src = np.floor(pos).astype(np.int64)
    vo = (pos - np.floor(pos)) * RS_OFFS
    for u in range(40, case.n_in - 40, 32):
        hit = [k for k in np.nonzero(src == u)[0] if 8 <= int(vo[k]) <= 24]
        if hit:
            o = int(vo[hit[0]])
            f = float(vo[hit[0]]) - o
            x[u] = 1.0                                              # tap 16 of that output, tap 17 the next sample
            k1, k2, k3, k4 = K(o, 16), K(o + 1, 16), K(o, 17), K(o + 1, 17)
            b = np.float32(-((1.0 - f) * k1 + f * k2) / ((1.0 - f) * k3 + f * k4))
            x[u + 1] = b
            for d in range(-64, 65):                                # among the neighbouring sizes, one at which the two blends differ (where there is one)
                bb = (b.view(np.int32) + np.int32(d)).view(np.float32)
                s1, s2 = float(np.float32(k1 + float(bb) * k3)), float(np.float32(k2 + float(bb) * k4))
                a = (1.0 - f) * s1
                if np.float32(a + f * s2) != np.float32(float(Fraction(f) * Fraction(s2) + Fraction(a))):
                    x[u + 1] = bb
                    break
    return x


def nonfinite_expected(case):
    """the outputs whose 32-tap window holds the one NaN / Inf sample (sig nan / inf), from the positions alone"""
    n = np.arange(case.n_out, dtype=np.float64)
    src = np.floor(n * (case.fs_in / case.fs_out)).astype(np.int64)
    return (src - RS_TAPS // 2 <= case.mid) & (case.mid <= src + RS_TAPS // 2 - 1)


# ---- the run arithmetic of rs_block
def iter_runs(p, n_in, n_out):
    """the runs a clip's blocks convert, in order: dict(bx, c, n0, m = outputs of the run, lo, lo4, q_lo, q_hi, v_lo, v_hi); then the grid block and chunk
    at which the last block's loop ended as ('end', bx, c)"""
    SJ, C = p["S"] * p["J"], p["chunks"]
    per_block = SJ * C
    for bx in range((n_out + per_block - 1) // per_block):
        for c in range(C):
            n0 = (bx * C + c) * SJ
            if n0 >= n_out:
                yield ("end", bx, c)
                break
            lo = int(math.floor(float(n0) * p["ratio"])) - RS_TAPS // 2
            lo4 = lo & ~3
            q_lo = -lo4 if lo4 < 0 else 0
            q_hi = n_in - 1 - lo4
            yield dict(bx=bx, c=c, n0=n0, m=min(SJ, n_out - n0), lo=lo, lo4=lo4, q_lo=q_lo, q_hi=q_hi, v_lo=(q_lo + 3) & ~3, v_hi=(q_hi - 3) & ~3)


def run_outputs(p, r, m=None):
    """per output of run r: position, window start relative to lo4, kernel row, blend weight — as the kernel forms them"""
    n = np.arange(r["n0"], r["n0"] + (r["m"] if m is None else m), dtype=np.float64)
    pos = n * p["ratio"]
    w = np.trunc(pos - float(r["lo4"] + RS_TAPS // 2)).astype(np.int64)
    vo = (pos - np.floor(pos)) * RS_OFFS
    o = vo.astype(np.int64)
    return pos, w, o, vo - o


def geometry(case, aligned=True):
    """-> dict(plan, n_out, arms = Counter, runs = [...], need_minus_span = the largest over the runs, max_w, reloads)"""
    p, n_in, n_out = case.plan, case.n_in, case.n_out
    S, J, SJ, xlen = p["S"], p["J"], p["S"] * p["J"], rs_xlen(p["span"])
    arms, runs, worst, max_w, reloads = Counter(), [], -10**9, 0, 0
    rs = [r for r in iter_runs(p, n_in, n_out)]
    ends = [r for r in rs if isinstance(r, tuple)]
    rs = [r for r in rs if not isinstance(r, tuple)]
    for i, r in enumerate(rs):
        assert r["q_lo"] % 4 == 0 and r["v_lo"] == r["q_lo"] and r["q_hi"] >= 16, (case, r)          # UNREACHABLE, above
        where = "only" if len(rs) == 1 else ("first" if i == 0 else ("last" if i == len(rs) - 1 else "middle"))
        path16 = aligned and r["v_hi"] >= r["v_lo"] and r["q_hi"] >= 3
        if path16:
            arms["stage:16B"] += 1
            arms["front:lo4<0" if r["lo4"] < 0 else "front:lo4>=0"] += 1
            if r["q_hi"] < xlen:                                    # the clip ends inside what the run stages
                arms[f"back:e={r['q_hi'] % 4}:{where}"] += 1
            else:
                arms["back:not-staged"] += 1
        else:
            arms["stage:word:unaligned" if not aligned else "stage:word:v_hi<v_lo"] += 1
        arms[f"win:lo-lo4={r['lo'] - r['lo4']}"] += 1
        pos, w, o, f = run_outputs(p, r)
        need = int(w.max()) + RS_TAPS
        assert w.min() >= 0 and need <= xlen, f"{case}: run at {r['n0']} needs {need} staged samples, rs_xlen(span) = {xlen}"
        worst, max_w = max(worst, need - p["span"]), max(max_w, int(w.max()))
        if need == p["span"] + 1:
            arms["need:span+1"] += 1
        if int(w[-1]) + RS_TAPS - 1 == r["q_hi"] and where in ("first", "middle"):
            arms["back:end-on-last-tap"] += 1
        # the j loop: lane t converts n0 + t + j S while that is below n_out
        if r["m"] < S:
            arms["break:lane-without-output"] += 1
        if r["m"] <= (J - 1) * S:
            arms["break:mid-j"] += 1
        o2 = np.full(S * J, -1, np.int64)
        o2[:r["m"]] = o
        o2 = o2.reshape(J, S)
        ch = int(((o2[1:] != o2[:-1]) & (o2[1:] >= 0)).sum())
        reloads += ch
        runs.append(dict(r, need=need, where=where, path16=path16, reloads=ch))
    L = period(case.fs_in, case.fs_out)
    if n_out:
        m = rs[-1]["m"]
        for tag, v in (("1", 1), ("S-1", S - 1), ("S", S), ("S+1", S + 1), ("SJ-1", SJ - 1), ("SJ", SJ)):
            if m == v:
                arms[f"last:{tag}"] += 1
        if n_out % SJ == 0 and n_out >= 2 * SJ:
            arms["nout=k*S*J"] += 1
        if L is None:
            arms["rows:non-integer-rate"] += 1
        elif L > 512:
            arms["rows:period>512"] += 1
        elif S % L:
            arms["rows:S%L!=0"] += 1
        else:
            arms["rows:S%L==0:rounding-reload" if reloads else "rows:S%L==0:no-reload"] += 1
        if J == 1:
            arms["J=1"] += 1
        if J == 96:
            arms["J=96"] += 1
        if p["chunks"] > 1:
            arms[f"chunks={p['chunks']}"] += 1
            for (_, bx, c) in ends:
                arms[f"chunks:last-block-ends@c={c}"] += 1
            if n_out % SJ == 0:
                arms["chunks:nout-on-chunk-end"] += 1
    if n_in in (0, 1, 3, 15, 16, 17, 31):
        arms[f"n_in={n_in}"] += 1
    arms[f"stride:{resample_stride(case.fs_in, case.fs_out)[1]}"] += 1
    return dict(plan=p, n_out=n_out, arms=arms, runs=runs, need_minus_span=worst, max_w=max_w, reloads=reloads)


def _search(name, fs_in, fs_out, arm, start, stop, **kw):
    """the first length in [start, stop) whose geometry sits on `arm`"""
    for n in range(start, stop):
        c = Case(name, fs_in, fs_out, n, **kw)
        if geometry(c)["arms"][arm]:
            return c
    raise AssertionError(f"no length in [{start}, {stop}) puts {fs_in} -> {fs_out} on {arm}")


def _n_in_for(n_out, fs_in, fs_out):
    n = int(math.ceil(n_out * (fs_in / fs_out)))
    for k in range(max(n - 3, 0), n + 4):
        if resample_length(k, fs_in, fs_out) == n_out:
            return k
    raise AssertionError(f"{fs_in} -> {fs_out} has no clip of {n_out} outputs")


def _first_rounding_reload(fs_in, fs_out):
    """the smallest clip with an output whose kernel row is not its period's (fp64 rounding of n * ratio) and is re-read for it, or None below MAX_OUT_ROUNDING"""
    L, p = period(fs_in, fs_out), plan(fs_in, fs_out)
    n = np.arange(MAX_OUT_ROUNDING, dtype=np.float64)
    pos = n * p["ratio"]
    o = ((pos - np.floor(pos)) * RS_OFFS).astype(np.int64)
    for k in np.nonzero(o != o[np.arange(MAX_OUT_ROUNDING) % L])[0]:
        if int(k) + 1 >= MAX_OUT_ROUNDING:
            break
        c = Case(f"rows-rounding-reload-{int(fs_in)}", fs_in, fs_out, _n_in_for(int(k) + 1, fs_in, fs_out))
        if geometry(c)["reloads"]:
            return c
    return None


def _rate_with_stride(S_want):
    """the integer rate closest below 48000 whose conversion to 48000 ends resample_stride's search at S_want"""
    for fs in range(47999, 40000, -1):
        if resample_stride(fs, 48000) == (S_want, "search"):
            return fs
    raise AssertionError(S_want)


LONG_24414 = "need-span+1-24414-run-9"
STRIDE_TABLE = [(44100, 48000, 160, 192), (8000, 48000, 252, 256), (32000, 48000, 255, 256), (48000, 16000, 256, 256), (22050, 48000, 320, 320),
                (44032, 48000, 375, 384), (48000, 44100, 441, 448), (16000, 44100, 441, 448), (42336, 48000, 500, 512)]
FS_300, FS_400 = _rate_with_stride(300), _rate_with_stride(400)
ROUNDING = {fs: _first_rounding_reload(fs, 48000) for fs in (44100, 16000)}       # None: the model finds none below MAX_OUT_ROUNDING outputs


def _build():
    cs = []
    add = cs.append
    A, B = (44100, 48000), (48000, 44100)          # S = 160, J = 29 (4640 outputs per run) / S = 441, J = 8 (3528)
    pA, pB = plan(*A), plan(*B)
    sjA, sjB = pA["S"] * pA["J"], pB["S"] * pB["J"]
    for n in (0, 1, 3, 15, 16, 17, 31):
        add(Case(f"n_in-{n}", *A, n))
    add(Case("word-path-v_hi<v_lo-2-samples", 16000, 48000, 2))
    add(Case("16B-path-one-whole-word-4-samples", *A, 4))
    # the back edge of the 16-byte path: the clip ends e samples into a staged word, in the first, a middle and the last run
    for where, base in (("first", _n_in_for(sjA, *A)), ("middle", _n_in_for(2 * sjA, *A)), ("last", 9000)):
        for e in range(4):
            add(_search(f"back-e{e}-{where}-run", *A, f"back:e={e}:{where}", base, base + 60))
    add(_search("back-end-on-last-tap", *A, "back:end-on-last-tap", _n_in_for(sjA, *A), _n_in_for(sjA, *A) + 60))
    for d, runs in ((0, 0), (3, 1), (2, 2), (1, 3)):      # lo = floor(k S J ratio) - 16 = -16, 4247, 8510, 12773 at the start of run k
        start = _n_in_for(runs * sjA, *A) + 40
        add(_search(f"window-start-lo-lo4-{d}", *A, f"win:lo-lo4={d}", start, start + 60))
    # outputs of the last run (48000 -> 44100 reaches every output count)
    for tag, m in (("1", 1), ("S-1", pB["S"] - 1), ("S", pB["S"]), ("S+1", pB["S"] + 1), ("SJ-1", sjB - 1), ("SJ", sjB)):
        add(Case(f"last-run-{tag}-outputs", *B, _n_in_for(sjB + m, *B)))
    add(Case("n_out-3-S-J-exactly", *B, _n_in_for(3 * sjB, *B)))
    add(Case("break-mid-j-short-beside-long", *B, 700))
    add(Case("J-1-ratio-16-128000-8000", 128000, 8000, 14000))
    add(Case("J-1-ratio-16-48000-3000", 48000, 3000, 9000))
    add(Case("J-96-ratio-1/16", 3000, 48000, 3000))
    add(Case("period-8000-24414", 24414, 48000, 14900))
    add(Case(LONG_24414, 24414, 48000, 43000))          # need = span + 1 first at the start of run 9 (outputs 76032 ...): the one case beyond MAX_IN / MAX_OUT
    add(Case("period-47999-least-slack", 47999, 48000, 14000))
    add(Case("period-640-11025", 11025, 48000, 9000))
    add(Case("non-integer-rate-44100.5", 44100.5, 48000, 9000))
    add(Case("rows-no-reload-44100", *A, 9001))
    add(Case("rows-no-reload-16000", 16000, 48000, 9001))
    for fs, c in ROUNDING.items():
        if c is not None:
            add(c)
    add(Case("rows-S-64-override", *A, 9000, S=64))
    add(Case("rows-S-100-override", *A, 9000, S=100))
    add(Case("J-7-override", 16000, 48000, 5000, J=7))
    # runs per block
    p2 = plan(*A, J=8)
    sj2 = p2["S"] * p2["J"]                              # 1280 outputs per run
    add(Case("chunks-2-ends-at-c-1", *A, _search_len(A, 2 * sj2 + 1, 3 * sj2), J=8, C=2))
    add(Case("chunks-3-ends-at-c-1", *A, _search_len(A, 3 * sj2 + 1, 4 * sj2), J=8, C=3))
    add(Case("chunks-3-ends-at-c-2", *A, _search_len(A, 4 * sj2 + 1, 5 * sj2), J=8, C=3))
    add(Case("chunks-2-n_out-on-chunk-end", *B, _n_in_for(3 * sjB, *B), C=2))
    add(Case("chunks-3-n_out-on-block-end", *B, _n_in_for(3 * sjB, *B), C=3))
    # stride classes
    for fs_in, fs_out, S, blk in STRIDE_TABLE:
        add(Case(f"stride-{S}-in-{blk}-lanes-{fs_in}-{fs_out}", fs_in, fs_out, min(MAX_IN - 1000, int((MAX_OUT - 1000) * fs_in / fs_out))))
    add(Case(f"stride-300-search-{FS_300}", FS_300, 48000, 9000))
    add(Case(f"stride-400-search-{FS_400}", FS_400, 48000, 9000))
    # arithmetic
    add(Case("signal-cancel-blend-roundings", 44100.5, 48000, 12000, sig="cancel"))
    for sig in ("dc", "alt", "sub", "subimp", "negzero", "nan", "inf", "big"):
        add(Case(f"signal-{sig}-44100", *A, 5003, sig=sig))
        add(Case(f"signal-{sig}-48000-16000", 48000, 16000, 5003, sig=sig))
    # the copy class of a mixed batch
    for n in (8191, 8192, 8193, 16385):
        add(Case(f"copy-{n}", 48000, 48000, n))
    add(Case("copy-empty", 48000, 48000, 0))
    add(Case("class-of-empty-clips-only", 22050, 44100, 0))
    add(Case("one-launch-160-in-448-lanes", *A, 4700))
    return cs


def _search_len(pair, lo, hi):
    """a clip length whose output count lies in [lo, hi)"""
    return _n_in_for(next(n for n in range((lo + hi) // 2, hi) if _reachable(n, *pair)), *pair)


def _reachable(n_out, fs_in, fs_out):
    try:
        _n_in_for(n_out, fs_in, fs_out)
        return True
    except AssertionError:
        return False


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

REQUIRED = (["stage:16B", "stage:word:v_hi<v_lo", "front:lo4<0", "front:lo4>=0", "back:not-staged", "back:end-on-last-tap"]
            + [f"back:e={e}:{w}" for w in ("first", "middle", "last") for e in range(4)]
            + [f"win:lo-lo4={d}" for d in range(4)] + ["need:span+1"]
            + [f"last:{t}" for t in ("1", "S-1", "S", "S+1", "SJ-1", "SJ")] + ["nout=k*S*J", "break:lane-without-output", "break:mid-j", "J=1", "J=96"]
            + [f"n_in={n}" for n in (0, 1, 3, 15, 16, 17, 31)]
            + ["rows:S%L==0:no-reload", "rows:S%L!=0", "rows:period>512", "rows:non-integer-rate"]
            + ["stride:first", "stride:search", "stride:long", "stride:non-integer"]
            + ["chunks=2", "chunks=3", "chunks:last-block-ends@c=1", "chunks:last-block-ends@c=2", "chunks:nout-on-chunk-end"])
if any(c is not None for c in ROUNDING.values()):
    REQUIRED.append("rows:S%L==0:rounding-reload")
UNREACHABLE = {"front:q_lo%4!=0": "lo4 = lo & ~3 is a multiple of 4, so is q_lo, and v_lo == q_lo",
               "stage:word:q_hi<3": "an output's position is below n_in, its window starts below n_in - 16: q_hi >= 16 in every run with outputs",
               "back:clip-ends-in-first-staged-word": "q_hi >= 16, as above"}


# ---- launches: which clips go together
def single_rate_groups():
    """form 0: the cases of one rate pair and one set of overrides share a launch (short clips beside long ones: blocks past a clip's end return)"""
    g = {}
    for c in CASES:
        g.setdefault((c.fs_in, c.fs_out, c.S, c.J, c.C, c.n_out > MAX_OUT), []).append(c)
    return list(g.values())


def mixed_batches():
    """forms 1 and 2: per output rate every case's clip (overrides do not exist there), classes interleaved in clip order; the long rounding cases in a batch of their own"""
    b = {}
    for c in CASES:
        b.setdefault((c.fs_out, c.n_out > MAX_OUT), []).append(c)
    out = []
    for (fs_out, big), cs in sorted(b.items()):
        by_rate = {}
        for c in cs:
            by_rate.setdefault(c.fs_in, []).append(c)
        lists, order = list(by_rate.values()), []
        while any(lists):                                   # round robin over the classes
            for l in lists:
                if l:
                    order.append(l.pop(0))
        if big:
            order.append(Case("small-beside-long", 16000, fs_out, 300))
        out.append(order)
    return out


def mixed_plan(batch):
    """plan_resample_mixed for a batch: classes in order of first appearance -> (rows of plan_row, max_block, max_lds, arms)"""
    rates, arms = [], Counter()
    for c in batch:
        if c.fs_in not in rates:
            rates.append(c.fs_in)
    plans = [COPY_PLAN if r == batch[0].fs_out else plan(r, batch[0].fs_out) for r in rates]
    max_block, max_lds = max([64] + [p["block"] for p in plans]), max([0] + [p["lds"] for p in plans])
    cls = [rates.index(c.fs_in) for c in batch]
    if any(cls[i] > cls[i + 1] for i in range(len(cls) - 1)):
        arms["mixed:classes-interleaved"] += 1
    for k, r in enumerate(rates):
        mine = [c for c in batch if c.fs_in == r]
        if all(c.n_out == 0 for c in mine):
            arms["mixed:class-all-empty"] += 1
        if plans[k]["copy"]:
            for c in mine:
                arms[f"mixed:copy-{c.n_in}"] += 1
        elif plans[k]["block"] < max_block:
            arms["mixed:one-launch-block<max_block"] += 1
            if plans[k]["S"] == 160 and max_block >= 448:
                arms["mixed:one-launch-160-in-448+"] += 1
    return [plan_row(p) for p in plans], max_block, max_lds, arms


REQUIRED_MIXED = ["mixed:classes-interleaved", "mixed:class-all-empty", "mixed:one-launch-block<max_block", "mixed:one-launch-160-in-448+"] + [f"mixed:copy-{n}" for n in (8191, 8192, 8193, 16385)]


def arm_table():
    """arm -> (count over all cases, the first case that sits on it)"""
    t = {}
    for c in CASES:
        for a, k in geometry(c)["arms"].items():
            n, first = t.get(a, (0, c.name))
            t[a] = (n + k, first)
    n_un = sum(len(geometry(c, aligned=False)["runs"]) for c in CASES)
    t["stage:word:unaligned"] = (n_un, CASES[0].name)
    groups = single_rate_groups()
    past = sum(1 for g in groups for c in g
               if (max(x.n_out for x in g) + c.plan["S"] * c.plan["J"] * c.plan["chunks"] - 1) // (c.plan["S"] * c.plan["J"] * c.plan["chunks"])
               > (c.n_out + c.plan["S"] * c.plan["J"] * c.plan["chunks"] - 1) // (c.plan["S"] * c.plan["J"] * c.plan["chunks"]))
    t["grid:clip-with-blocks-past-its-end"] = (past, "break-mid-j-short-beside-long")
    for b in mixed_batches():
        for a, k in mixed_plan(b)[3].items():
            n, first = t.get(a, (0, b[0].name))
            t[a] = (n + k, first)
    return t


def check_cases():
    t = arm_table()
    missing = [a for a in REQUIRED + REQUIRED_MIXED + ["stage:word:unaligned", "grid:clip-with-blocks-past-its-end"] if t.get(a, (0,))[0] == 0]
    assert not missing, f"arms without a case: {missing}"
    for c in CASES:
        assert (c.n_in < MAX_IN or c.fs_in == c.fs_out) and (c.n_out < MAX_OUT or c in ROUNDING.values()) and c.n_out < MAX_OUT_ROUNDING or c.name == LONG_24414, c
    g = geometry(BY_NAME[LONG_24414])
    assert [r["need"] - g["plan"]["span"] for r in g["runs"]].index(1) == 9, "24414 -> 48000: the need exceeds span first in run 9"
    return t


ARMS = check_cases()

"""Hand-built syllables for output level 12's polynomial fits (csrc/coeffs.hip, K5) (test helper): the deterministic table of cases, the search that
found the throwing ones, and the layouts that put the cases into the frame tables of a batch or of streams' rings.

A case is one syllable as sep_syllables can hand it over: `fr` [sl, 9] float32 (integer-valued bins 0 .. 255 in columns 0, 3, 6 — what the fits
read; the energy and width columns carry filler), `sums` [sl] float32 >= 0 (the per-frame energy sum, order-4 fit of 10 log10), sl >= 2, a zero
marking a frame without a point.  Fit q of a syllable: 0 the sums (order 4), 1 / 2 the bins of formants 1 / 2 (order 3), 3 the bin of formant 3
(order 1).  All randomness is a 64-bit LCG written out here, so the table does not depend on a library's generator; the fixture
tests/golden/coeffs_expected.json keeps a digest of every case's bytes.

Families (the tag set `fam` of a case; tests/test_coeffs_reference.py asserts each is present and counts what the oracle did on it):
  counts    every fit with 0 .. 7 points, the four columns of a syllable with different counts, at sl 9 (LDS) and sl 40 (scratch)
  length    dense columns at sl 2, 3, 31, 32, 33, 63, 64, 65, 300: both sides of COEF_LDS_PTS = 32
  sparse    sl 33, 64, 65, 300 with 3 .. 5 points per fit: the scratch path with few points
  gap       the first point late (first = 1, 17, sl - 3): the design matrix in r, the residuals in r - first
  retry     constant columns (the energy sum too) and exact polynomials of the fit's order or lower: the h / 16 retry of numeric.gradient
  gapretry  constant and exactly linear columns behind a leading gap of 3 .. 259 frames: the powers of r are large, the cost of the exact fit is
            rounding noise, and the h / 16 retries decide the result's bits (retry_sensitive() counts the fits that change when the retry divides by
            8 instead: without the gap one fit of the table does).  Their gradients take up to 17 of numeric.gradient's 20 trials (with a divisor of 8
            some run out of them); search_gradient_fails() looks through the grid for one that does under numeric's own 16: none
  thrower   three points of one value at the row sets THROW_SETS (found by search_throwers: `uncmin: f(x0) is a NaN!` in an order-3 fit), on
            fit 1 and on fit 2, short and padded past 32 frames
  twin      a case again with frames without points appended until sl = 40: the same points through the other storage path, the same 23 numbers
What the searches did not find (a throw in fits 0 and 3, `Numerical gradient fails`, numeric.inv without a pivot) is recorded in NOT_FOUND and re-established by the CPU test, not
faked."""
import hashlib
import itertools

import numpy as np

COEF_LDS_PTS = 32                  # csrc/coeffs.hip: syllables of up to this many frames keep their points in LDS
NFEAT = 53                         # WSA_NFEAT: width of a compacted row
NCOEF = 23
FIT_COL = (None, 0, 3, 6)          # fit q reads this column of fr (q = 0: sums)
FIT_ORDER = (4, 3, 3, 1)
FIT_OFF = (0, 7, 13, 19)           # first slot of fit q in a row: order + 1 coefficients, rms error, points
RING = 64                          # the stream layouts' ring


class Lcg:
    """Knuth's MMIX LCG; the high 32 bits of each state."""
    def __init__(self, seed):
        self.s = (seed * 0x9E3779B97F4A7C15 + 1) & (2 ** 64 - 1)
        for _ in range(4):
            self.u32()

    def u32(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return self.s >> 32

    def below(self, n):
        return self.u32() % n

    def unit(self):
        return self.u32() / 2.0 ** 32

    def choose(self, n, k):
        """k distinct numbers below n, ascending."""
        pool = list(range(n))
        for i in range(k):
            j = i + self.below(n - i)
            pool[i], pool[j] = pool[j], pool[i]
        return sorted(pool[:k])


def _syllable(sl, cols, sums):
    """cols: three sequences of sl bins (fits 1, 2, 3), sums: sl energy sums."""
    fr = np.zeros((sl, 9), np.float32)
    for k, c in enumerate(cols):
        c = np.asarray(c, np.float64)
        assert c.shape == (sl,) and (c == np.floor(c)).all() and c.min() >= 0 and c.max() <= 255
        fr[:, 3 * k] = c
        fr[:, 3 * k + 1] = np.where(c > 0, 1000.0 + 7 * k, 0)        # energy and width: not read by the fits
        fr[:, 3 * k + 2] = np.where(c > 0, 3.0 + k, 0)
    sums = np.asarray(sums, np.float32)
    assert sums.shape == (sl,) and (sums >= 0).all() and sl >= 2
    return fr, sums


def _case(name, fam, fr, sums, twin_of=None):
    return dict(name=name, fam=frozenset(fam), fr=fr, sums=sums, sl=len(sums), twin_of=twin_of)


def _dense(rng, sl, keep=1.0):
    """A wandering bin track 1 .. 255, a point on every frame with probability keep."""
    base, amp, w, ph = 40 + rng.below(150), 5 + rng.below(30), 2.0 + 9 * rng.unit(), 6.28 * rng.unit()
    v = [min(255, max(1, int(round(base + amp * np.sin(r / w + ph) + 4 * (rng.unit() - 0.5))))) for r in range(sl)]
    return [x if rng.unit() < keep else 0 for x in v]


def _energy(rng, sl, keep=1.0):
    lvl, w = 10.0 ** (1 + 6 * rng.unit()), 1.5 + 6 * rng.unit()
    v = [lvl * (1.2 + np.sin(r / w)) * (0.8 + 0.4 * rng.unit()) for r in range(sl)]
    return [x if rng.unit() < keep else 0.0 for x in v]


def _at(sl, rows, vals):
    c = [0.0] * sl
    for r, v in zip(rows, vals):
        c[r] = v
    return c


def _points(rng, sl, n, lo=0, energy=False):
    """n points at random rows lo .. sl - 1."""
    rows = [lo + r for r in rng.choose(sl - lo, n)]
    return _at(sl, rows, [10.0 ** (1 + 5 * rng.unit()) if energy else 1 + rng.below(255) for _ in rows])


# Row sets within rows 0 .. 10 whose three points of one value (100) make the order-3 fit throw `uncmin: f(x0) is a NaN!`; search_throwers()
# finds exactly these among all 165 + 330 + 462 sets of three, four and five rows, and nothing for orders 4 (on the sums) and 1.
THROW_SETS = ((0, 3, 6), (0, 8, 9), (1, 5, 8))
# paths the search and the whole table never reached (tests/test_coeffs_reference.py establishes the same again from the oracle)
NOT_FOUND = ("throw in fit 0 (order 4)", "throw in fit 3 (order 1)", "Numerical gradient fails", "inv: no pivot")
# the grid of the gapretry family: first row, points, constant energy sum
GAP_FIRSTS, GAP_POINTS, GAP_SUMS = (3, 10, 20, 27, 50, 100, 200, 259), (4, 5, 8, 12), (3.0, 250.0, 1.0e6, 7.7e8)
THROW_VALUE = 100.0
# what the oracle did over the whole table, counted by tests/test_coeffs_reference.py (which asserts this very table) with oracle_stats() below
RECORDED = {"cases": 158, "fits": 632, "fits_refined": 562, "gradients": 3005, "bfgs_iterations": 2443, "max_iterations": 18, "fits_over_10_iterations": 62,
            "halvings": 13226, "halving_fits": 483, "max_gradient_trials": 17, "retries_lds": 570, "retrying_fits_lds": 78, "retry_sensitive_fits_lds": 15,
            "retries_scratch": 795, "retrying_fits_scratch": 111, "retry_sensitive_fits_scratch": 42, "throws_lds": 12, "throws_scratch": 6}


def search_throwers(sizes=(3, 4, 5), rows=11):
    """{(fit order, row set): message} over every set of `sizes` rows below `rows`, all points of value THROW_VALUE (the order-4 fit reads it as an
    energy sum: 10 log10).  Oracle only."""
    from oracle import pyoracle
    found = {}
    for n in sizes:
        for rs in itertools.combinations(range(rows), n):
            col = np.zeros((rs[-1] + 1, 2))
            col[list(rs), :] = THROW_VALUE
            for order, log in ((4, True), (3, False), (1, False)):
                try:
                    pyoracle._polyfit(col, 1, order, log)
                except ValueError as e:
                    found[(order, rs)] = str(e)
    return found


def search_gradient_fails():
    """{(first, points, sum): message} over GAP_FIRSTS x GAP_POINTS x GAP_SUMS: the order-4 fit of `points` equal energy sums from row `first` on."""
    from oracle import pyoracle
    found = {}
    for first in GAP_FIRSTS:
        for n in GAP_POINTS:
            for v in GAP_SUMS:
                col = np.zeros((first + n, 2), np.float32)
                col[first:, 1] = v
                try:
                    pyoracle._polyfit(col, 1, 4, True)
                except ValueError as e:
                    found[(first, n, v)] = str(e)
    return found


def _build():
    out = []
    add = lambda *a, **k: out.append(_case(*a, **k))
    # counts: column q of syllable c holds (c + 3 q) % 8 points (every count meets every fit), LDS and scratch
    for sl in (9, 40):
        for c in range(8):
            rng = Lcg(1000 + 10 * sl + c)
            n = [(c + 3 * q) % 8 for q in range(4)]
            add(f"counts-sl{sl}-{c}", {"counts"}, *_syllable(sl, [_points(rng, sl, n[q]) for q in (1, 2, 3)], _points(rng, sl, n[0], energy=True)))
    # lengths: dense, and with a fifth of the frames empty
    for sl in (2, 3, 31, 32, 33, 63, 64, 65, 300):
        for v, keep in enumerate((1.0, 0.8)):
            rng = Lcg(2000 + 10 * sl + v)
            add(f"length-sl{sl}-{v}", {"length"}, *_syllable(sl, [_dense(rng, sl, keep) for _ in range(3)], _energy(rng, sl, keep)))
    # sparse long syllables
    for sl in (33, 64, 65, 300):
        for n in (3, 4, 5):
            rng = Lcg(3000 + 10 * sl + n)
            add(f"sparse-sl{sl}-n{n}", {"sparse"}, *_syllable(sl, [_points(rng, sl, n) for _ in range(3)], _points(rng, sl, n, energy=True)))
    # leading gap
    for sl in (24, 40, 300):
        for first in (1, 17, sl - 3):
            rng = Lcg(4000 + 10 * sl + first)
            cols = [[0] * first + _dense(rng, sl - first) for _ in range(3)]
            add(f"gap-sl{sl}-first{first}", {"gap"}, *_syllable(sl, cols, [0.0] * first + _energy(rng, sl - first)))
    # retry inducers: constants ...
    for sl in (3, 4, 5, 8, 12, 20, 31, 32, 33, 64, 65, 300):
        k = sl % 7
        add(f"retry-const-sl{sl}", {"retry"}, *_syllable(sl, [[100 + k] * sl, [37 + k] * sl, [200 + k] * sl], [5000.0 * (k + 1)] * sl))
    # ... exact lines (a point on every second row where the slope is 1 / 2), parabolas and cubics inside a window of rows
    for sl in (5, 9, 17, 31, 32, 33, 64, 65, 300):
        ev = [10 + r // 2 if r % 2 == 0 else 0 for r in range(sl)]
        dn = [200 - r // 2 if r % 2 == 0 else 0 for r in range(sl)]
        one = [3 + r if r < 250 else 0 for r in range(sl)]
        add(f"retry-line-sl{sl}", {"retry"}, *_syllable(sl, [ev, dn, one], [250.0] * sl))
    for sl, lo in ((11, 0), (31, 0), (32, 1), (33, 2), (65, 30), (300, 260)):
        par = [2 + (r - lo - 15) ** 2 if 0 <= r - lo <= 30 else 0 for r in range(sl)]
        cub = [128 + (r - lo - 5) ** 3 if 0 <= r - lo <= 10 else 0 for r in range(sl)]
        lin = [250 - 3 * (r - lo) if 0 <= r - lo <= 60 else 0 for r in range(sl)]
        add(f"retry-poly-sl{sl}", {"retry"}, *_syllable(sl, [par, cub, lin], [1.0e6 if 0 <= r - lo <= 40 else 0.0 for r in range(sl)]))
    # throwers: the failing fit on column 1 or 2, ordinary fits around it; short, and padded past 32 frames
    for i, rs in enumerate(THROW_SETS):
        for q in (1, 2):
            for sl in (rs[-1] + 1, 12, 45):
                rng = Lcg(5000 + 100 * i + 10 * q + sl)
                cols = [_dense(rng, sl) for _ in range(3)]
                cols[q - 1] = _at(sl, rs, [THROW_VALUE] * len(rs))
                add(f"thrower-{'_'.join(map(str, rs))}-q{q}-sl{sl}", {"thrower"}, *_syllable(sl, cols, _energy(rng, sl)))
    # constant and linear columns behind a leading gap
    for first in GAP_FIRSTS:
        for n in GAP_POINTS:
            v = GAP_SUMS[(first + n) % len(GAP_SUMS)]
            sl = first + n
            gap = [0] * first
            cols = [gap + [100 + first % 50] * n, gap + [40 + k for k in range(n)], gap + ([200 - 2 * k for k in range(n)] if n % 2 else [37] * n)]
            add(f"gapretry-first{first}-n{n}", {"gapretry"}, *_syllable(sl, cols, [0.0] * first + [v] * n))
    # twins: the same points, frames without points appended until the syllable takes the scratch path
    for c in list(out):
        if c["sl"] <= 12 and c["name"].split("-")[0] in ("counts", "retry", "gap", "length", "gapretry") or c["name"] in ("length-sl31-0", "length-sl32-1", "gap-sl24-first17"):
            pad = 40 - c["sl"]
            add("twin-" + c["name"], c["fam"] | {"twin"}, np.concatenate([c["fr"], np.zeros((pad, 9), np.float32)]), np.concatenate([c["sums"], np.zeros(pad, np.float32)]), twin_of=c["name"])
    assert len({c["name"] for c in out}) == len(out)
    return out


CASES = _build()
INDEX = {c["name"]: i for i, c in enumerate(CASES)}
FAMILIES = ("counts", "length", "sparse", "gap", "retry", "gapretry", "thrower", "twin")


def digest(c):
    return hashlib.sha256(c["name"].encode() + b"\0" + np.ascontiguousarray(c["fr"]).tobytes() + np.ascontiguousarray(c["sums"]).tobytes()).hexdigest()[:16]


def sums3(c):
    """The syllable's sums rows as the reference holds them: three floats per frame, the energy sum in slot 1."""
    s = np.zeros((c["sl"], 3), np.float32)
    s[:, 1] = c["sums"]
    return s


# ---- what the oracle did on a case ------------------------------------------------------------------------------------------------------------

def column(c, q):
    """[sl, 2] float: fit q's column of the case in slot 1 (what pyoracle._polyfit(rows, 1, order, log) reads)."""
    v = c["sums"] if q == 0 else c["fr"][:, FIT_COL[q]]
    return np.stack([np.zeros(c["sl"], np.float32), v], axis=1)


def polyfit(c, q):
    """Fit q of the case on its own: order + 3 numbers from the oracle, or ValueError where numeric throws."""
    from oracle import pyoracle
    return pyoracle._polyfit(column(c, q), 1, FIT_ORDER[q], q == 0)


def retry_sensitive(c):
    """The fits of the case whose result (or throw) changes when numeric.gradient's retry divides h by 8 instead of 16: what a wrong retry on the device
    would change.  Oracle only."""
    from oracle import numeric_js as nj
    orig = nj.gradient
    out = []
    for q in range(4):
        if (column(c, q)[:, 1] > 0).sum() <= 2:
            continue
        res = []
        for shrink in (16, 8):
            nj.gradient = lambda f, x, shrink=shrink: orig(f, x, shrink)
            try:
                res.append(np.array(polyfit(c, q)).view(np.uint64).tolist())
            except ValueError as e:
                res.append(str(e))
            finally:
                nj.gradient = orig
        if res[0] != res[1]:
            out.append(q)
    return out


def oracle_stats(c):
    """The oracle on one case, every fit on its own, with numeric_js.gradient and the cost function wrapped to count:
    (row | None, [per fit dict(cnt, grads, retries, trials, iters, halvings, threw, values)]).  row = the 23 numbers as pyoracle.syllable_coeffs joins them, None if
    a fit threw.  grads = calls of numeric.gradient, retries = its h / 16 retries (trials beyond one per coordinate), iters = BFGS updates (a gradient
    behind an accepted step), trials = the most trials one call of numeric.gradient took (it throws past 20), halvings = cost evaluations of the line search that were not accepted."""
    from oracle import numeric_js as nj
    fits, parts = [], []
    orig = nj.gradient
    for q in range(4):
        st = dict(cnt=int((column(c, q)[:, 1] > 0).sum()), grads=0, retries=0, trials=0, iters=0, halvings=0, threw=None, direct=0)
        inside = [False]

        def gradient(f, x, st=st, inside=inside):
            n_eval = [0]

            def g(v):
                n_eval[0] += 1
                return f(v)
            st["grads"] += 1
            inside[0] = True
            try:
                return orig(g, x)
            finally:
                inside[0] = False
                st["retries"] += max(0, (n_eval[0] - 1) // 2 - len(x)) if n_eval[0] > 1 else 0
                st["trials"] = max(st["trials"], (n_eval[0] - 1) // 2)

        real_uncmin = nj.uncmin

        def uncmin(f, x0, st=st, inside=inside):
            def g(v):
                if not inside[0]:
                    st["direct"] += 1
                return f(v)
            return real_uncmin(g, x0)
        nj.gradient, nj.uncmin = gradient, uncmin
        try:
            parts.append(polyfit(c, q))
        except ValueError as e:
            st["threw"] = str(e)
            parts.append(None)
        finally:
            nj.gradient, nj.uncmin = orig, real_uncmin
        if st["grads"]:
            st["iters"] = st["grads"] - 1
            st["halvings"] = st["direct"] - 1 - st["iters"]          # direct evaluations: f(x0), then per line search the rejected ones and the accepted one
        st["values"] = parts[-1]
        fits.append(st)
    return (None if any(p is None for p in parts) else np.array(sum(parts, []))), fits


# ---- layouts: where the cases sit in the frame tables of one launch -----------------------------------------------------------------------------
# A layout = dict(name, geometry "batch" | "stream", clips [frames per clip], rows [(case index, clip, start frame)], rows_cap, ring_mask,
# scratch_stride).  tables() fills every frame outside the syllables with points (bins and sums that are never zero), so a fit that reads one frame
# too many, or a neighbour's, gets other numbers.

def _filler(n, salt):
    rng = Lcg(7000 + salt)
    fr = np.zeros((n, 9), np.float32)
    fr[:, 0::3] = np.array([[1 + rng.below(255) for _ in range(3)] for _ in range(n)], np.float32).reshape(n, 3)
    fr[:, 1::3] = 777.0
    fr[:, 2::3] = 2.0
    return fr, np.array([1.0 + 9999 * rng.unit() for _ in range(n)], np.float32)


def _pack(name, order, clip_sizes, gaps, rows_cap_extra=0):
    """Batch geometry: the cases `order` dealt over len(clip_sizes) clips in turn; gaps[i % len(gaps)] filler frames in front of the i-th syllable of a clip
    (0: back to back with the one before, or at frame 0), clip_sizes[c] filler frames behind the last (0: it ends on the clip's last frame)."""
    n_clips = len(clip_sizes)
    used, rows = [0] * n_clips, []
    for i, ci in enumerate(order):
        c = i % n_clips
        st = used[c] + gaps[(i // n_clips) % len(gaps)]
        rows.append((ci, c, st))
        used[c] = st + CASES[ci]["sl"]
    clips = [u + t for u, t in zip(used, clip_sizes)]
    # rows as the compaction leaves them: clip by clip
    rows.sort(key=lambda r: (r[1], r[2]))
    return dict(name=name, geometry="batch", clips=clips, rows=rows, rows_cap=len(rows) + rows_cap_extra, ring_mask=0xFFFFFFFF, scratch_stride=0)


def _mixed_order(n, salt):
    """n cases: LDS and scratch syllables alternating, throwers among them (so a wave of 16 rows holds both strides and a thrower)."""
    short = [i for i, c in enumerate(CASES) if c["sl"] <= COEF_LDS_PTS and "thrower" not in c["fam"]]
    long_ = [i for i, c in enumerate(CASES) if COEF_LDS_PTS < c["sl"] <= 65 and "thrower" not in c["fam"]]
    thr = [i for i, c in enumerate(CASES) if "thrower" in c["fam"]]
    rng = Lcg(8000 + salt)
    out = []
    for k in range(n):
        pool = thr if (thr and k % 6 == 3) else (long_ if k % 2 else short)
        out.append(pool[rng.below(len(pool))])
    return out


def _stream(name, streams, salt):
    """Stream geometry: streams = per stream a list of (case index, start frame): the frames of stream c live at ring rows (start + r) & (RING - 1)."""
    rows = [(ci, c, st) for c, lst in enumerate(streams) for ci, st in lst]
    for c, lst in enumerate(streams):                          # the syllables of one ring do not overlap
        seen = set()
        for ci, st in lst:
            cells = {(st + r) % RING for r in range(CASES[ci]["sl"])}
            assert len(cells) == CASES[ci]["sl"] and not (cells & seen), (name, c)
            seen |= cells
    return dict(name=name, geometry="stream", clips=[RING] * len(streams), rows=rows, rows_cap=len(rows), ring_mask=RING - 1, scratch_stride=2 * RING)


def layouts():
    I = INDEX
    out = []
    for n in (1, 15, 16, 17, 33):
        out.append(_pack(f"batch-{n}", _mixed_order(n, n), [0, 5, 3][:min(n, 3)], [0, 2, 0, 7]))
    # every case once; rows_cap far above the row count (the kernel's `row >= n_rows` guard), five clips, the first syllable of each at frame 0,
    # clips 0 and 3 ending on their last syllable's last frame (so a syllable of the next clip starts on the very next row of the tables)
    out.append(_pack("batch-all", list(range(len(CASES))), [0, 4, 1, 0, 9], [0, 0, 3, 1, 0, 11], rows_cap_extra=83))
    thr_s = [i for i, c in enumerate(CASES) if "thrower" in c["fam"] and c["sl"] <= 12]
    thr_l = [i for i, c in enumerate(CASES) if "thrower" in c["fam"] and c["sl"] > COEF_LDS_PTS]
    # wrapping the ring's end with sl <= 32 (st & 63 = 60, 12 frames) and with sl > 32 (st & 63 = 40, 40 frames); far into the stream (st > 2^20)
    out.append(_stream("stream-wrap", [[(I["retry-const-sl5"], 64 * 5 + 20), (I["twin-counts-sl9-3"], (1 << 20) + 40), (I["counts-sl9-3"], 64 * 5 + 28)],
                                      [(I["length-sl31-0"], 64 * 9 + 50), (I["gap-sl24-first17"], 64 * 9 + 17)]] , 1))
    # a syllable starting on the ring's last row, one of 63 frames and one that fills the ring, a thrower in a ring
    out.append(_stream("stream-edge", [[(I["length-sl3-0"], 64 * 3 + 63), (I["retry-line-sl33"], 64 * 4 + 2)] + ([(thr_s[0], 64 * 4 + 40)] if thr_s else []),
                                      [(I["length-sl63-0"], 64 * 7 + 13)], [(I["length-sl64-1"], 64 * 2 + 63)]], 2))
    out.append(_stream("stream-thrower", [([(thr_l[0], 64 * 2 + 30)] if thr_l else []) + [(I["counts-sl9-5"], 64 * 3 + 12)],
                                         [(I["retry-poly-sl33"], 64 * 11 + 45), (I["retry-poly-sl11"], 64 * 11 + 20), (I["length-sl2-0"], 64 * 11 + 33)]], 3))
    # retries that decide the result, through a wrapping ring on either storage path (sl 32 and sl 58)
    out.append(_stream("stream-gapretry", [[(I["gapretry-first27-n5"], 64 * 6 + 50), (I["gapretry-first3-n8"], 64 * 7 + 20)], [(I["gapretry-first50-n8"], 64 * 21 + 30)]], 4))
    return out


def tables(lay):
    """(formants [F, 9] f32, sums [F] f32, frame_off [clips + 1] u32, row_meta [rows, 8] i32) of a layout."""
    off = np.concatenate([[0], np.cumsum(lay["clips"])]).astype(np.uint32)
    fr, sm = _filler(int(off[-1]), len(lay["rows"]))
    ring = lay["ring_mask"] + 1 if lay["geometry"] == "stream" else None
    meta = np.zeros((len(lay["rows"]), 8), np.int32)
    for k, (ci, c, st) in enumerate(lay["rows"]):
        case = CASES[ci]
        idx = int(off[c]) + ((st + np.arange(case["sl"])) % ring if ring else st + np.arange(case["sl"]))
        assert ring or st + case["sl"] <= lay["clips"][c]
        fr[idx] = case["fr"]
        sm[idx] = case["sums"]
        meta[k] = (c, 0, st, case["sl"], 0, k, st, case["sl"])
    return fr, sm, off, meta


if __name__ == "__main__":
    for (order, rs), msg in sorted(search_throwers().items()):
        print(order, rs, msg)

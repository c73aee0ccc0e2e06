"""Device-side pieces tested on their own (through the test entries of libwsa that are not part of include/wsa.h)."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

from tests import peak_ref
from tests.util import GOLDEN, rel_err, same_f64

pytestmark = pytest.mark.gpu


def test_device_log10_and_pow_are_bit_exact_with_v8():
    """csrc/jsmath_device.hpp (fdlibm log10 / V8's variant of e_pow) on every vector of tests/golden/jsmath_v8.json — what Node's own
    Math.log10 / Math.pow returned (tests/golden/gen/make_jsmath.js), incl. the arguments around the `parseInt(pow(10, t - 3) / 20)`
    boundaries of the noise gate (ref dist/main.js:2 @B28615) — plus a dense sweep of the gate's own argument range against the CPU oracle
    (itself pinned to the same vectors, tests/test_oracle_backend.py)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle import pyoracle
    from webspeechanalyzer_amd import capi
    L = capi.lib()
    d = json.load(open(os.path.join(GOLDEN, "jsmath_v8.json")))
    h2d = lambda h: struct.unpack(">d", bytes.fromhex(h))[0]

    def run(fn, x, y=None):
        x = np.ascontiguousarray(x, np.float64)
        y = np.ascontiguousarray(y, np.float64) if y is not None else None
        out = np.zeros_like(x)
        assert L.wsa_debug_jsmath(0, fn, x.ctypes.data, y.ctypes.data if y is not None else None, out.ctypes.data, len(x)) == 0
        return out

    lx = np.array([h2d(a) for a, _ in d["log10"]]); lw = np.array([h2d(b) for _, b in d["log10"]])
    assert len(lx) > 1000 and np.array_equal(run(0, lx).view(np.uint64), lw.view(np.uint64))
    # jsm::log10_fin (fn 2): the branch-free form the feature reductions use, for positive normal finite arguments — the V8 vectors of that kind, every
    # power of two and its neighbours (log_e's |f| < 2^-20 arm), fp32 energies as the features see them, and a dense random sweep against jsm::log10
    ok = np.isfinite(lx) & (lx >= 2.3e-308)
    assert ok.sum() > 800 and np.array_equal(run(2, lx[ok]).view(np.uint64), lw[ok].view(np.uint64))
    rng2 = np.random.default_rng(11)
    p2 = 2.0 ** np.arange(-1000, 1000, dtype=np.float64)
    near = np.concatenate([p2, np.nextafter(p2, np.inf), np.nextafter(p2, 0), p2 * (1 + 2.0 ** -21), p2 * (1 - 2.0 ** -22), p2 * (1 + 2.0 ** -19), p2 * 1.4142135623730951, p2 * 1.41421356237])
    f32 = np.abs(rng2.standard_normal(400000).astype(np.float32) * np.float32(10.0) ** rng2.integers(-3, 12, 400000).astype(np.float32)).astype(np.float64)
    f32 = f32[f32 > 0]
    wide = np.exp(rng2.uniform(-700, 700, 400000))
    ints = np.arange(1, 300001, dtype=np.float64)
    for v in (near, f32, wide, ints):
        assert np.array_equal(run(2, v).view(np.uint64), run(0, v).view(np.uint64))
    pw = [(h2d(a), h2d(b), h2d(c)) for a, b, c in d["pow"] if h2d(a) > 0 and np.isfinite(h2d(c)) and h2d(c) > 1e-300]     # pow_pos: x > 0, normal results
    px, py, pz = (np.array(v) for v in zip(*pw))
    assert len(px) > 4000 and np.array_equal(run(1, px, py).view(np.uint64), pz.view(np.uint64))
    # the gate's arguments: y = ctx_max in [1, 2^33], t = log10(y), then 10 ** (t - 3), 10 ** (t - 2), 10 ** (t / 3)
    rng = np.random.default_rng(5)
    ys = np.concatenate([np.arange(1, 200001, dtype=np.float64), np.floor(10 ** rng.uniform(0, 9.9, 300000)),
                         np.array([10.0 ** k for k in range(10)]), np.array([2e4 * k for k in range(1, 5000)], dtype=np.float64)])
    Lo = pyoracle.lib()
    t_ref = np.array([Lo.wsa_or_log10(float(v)) for v in ys[:60000]])
    t_dev = run(0, ys)
    assert np.array_equal(t_dev[:60000].view(np.uint64), t_ref.view(np.uint64))
    for shift in ("m3", "m2", "d3"):
        e = t_dev - 3 if shift == "m3" else (t_dev - 2 if shift == "m2" else t_dev / 3)
        got = run(1, np.full_like(e, 10.0), e)
        ref = np.array([Lo.wsa_or_pow(10.0, float(v)) for v in e[:60000]])
        assert np.array_equal(got[:60000].view(np.uint64), ref.view(np.uint64)), shift


def test_integer_floor_law_equals_the_f64_evaluation_for_every_ctx_max():
    """gate_floor.hpp: the gate kernel evaluates the noise floor v(ctx_max) (ref dist/main.js:2 @B28615) in integer arithmetic and
    only takes the V8 log10 / pow route where the f64 result's last bit can matter (y a multiple of the arm's divisor, a perfect
    cube, a power of ten).  Compared on the device against the f64 evaluation for ALL 2^32 values of ctx_max."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from webspeechanalyzer_amd import capi
    L = capi.lib()
    out = (ctypes.c_uint64 * 3)()
    total_exact = 0
    for lo in range(0, 1 << 32, 1 << 30):
        assert L.wsa_debug_floor_law(0, lo, lo + (1 << 30), out) == 0
        assert out[0] == 0, f"{out[0]} values of ctx_max in [{lo}, {lo + (1 << 30)}) differ, the first is {out[1]}"
        total_exact += out[2]
    assert 0 < total_exact < (1 << 32) // 1000          # the f64 route is the exception


def test_device_match_score_equals_the_reference_function():
    """csrc/tracker_score.hpp on the rows of tests/golden/score_expected.json (what the reference's own `_` returned under Node), bit for bit:
    the x / 1, x / 2, 10 / gap special cases of the device version included."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from webspeechanalyzer_amd import capi
    L = capi.lib()
    d = json.load(open(os.path.join(GOLDEN, "score_expected.json")))
    args = np.ascontiguousarray(np.array(d["args"], dtype=np.float64))
    want = np.array([struct.unpack(">d", bytes.fromhex(h))[0] for h in d["expected_f64_hex"]])
    out = np.zeros(len(args))
    assert L.wsa_debug_score(0, args.ctypes.data, out.ctypes.data, len(args)) == 0
    bad = np.flatnonzero(out.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, f"{len(bad)} rows differ, first {args[bad[0]].tolist()}: {out[bad[0]]!r} vs {want[bad[0]]!r}"


def _peak_scan_reference(e):
    """The reference's scan of one u32 frame (ref dist/main.js:2 @B25827) with the noise floor left out
    (every candidate is kept; the gate applies `e[l] > v` later): candidates (i, s, l, last) after the /10 shoulder shrink, g.  The restatement
    itself is tests/peak_ref.py, which tests/test_peaks_reference.py pins to the oracle and to the reference's own run."""
    r = peak_ref.scan(e)
    return r["cands"], r["g"]


def _peak_frames(rng, n, B):
    """frames that reach every corner of the scan: smooth humps, noise, plateaus, long ramps (candidates wider than the LDS
    ring of the lane-per-frame kernel), amplitudes up to 2^32 - 1 (prefix sums above 2^32), zeros"""
    rows = []
    x = np.arange(B)
    for k in range(n):
        kind = k % 8
        if kind == 0:
            r = rng.integers(0, 1 << rng.integers(4, 33), B, dtype=np.uint64)
        elif kind == 1:
            r = sum(rng.uniform(10, 1e6) * np.exp(-0.5 * ((x - rng.uniform(0, B)) / rng.uniform(0.7, 6)) ** 2) for _ in range(rng.integers(1, 12))) + rng.uniform(0, 30, B)
        elif kind == 2:
            r = np.repeat(rng.integers(0, 50, (B + 3) // 4), 4)[:B] * rng.integers(1, 1000)          # plateaus: flat runs
        elif kind == 3:
            r = np.cumsum(rng.integers(0, 3, B)) * rng.integers(1, 1 << 20)                          # long weak ramps
            if k % 16 == 3: r = r[::-1].copy()
        elif kind == 4:
            r = np.full(B, (1 << 32) - 1, dtype=np.uint64) - rng.integers(0, 5, B).astype(np.uint64)   # saturated: P crosses 2^32 every bin
        elif kind == 5:
            r = np.where(rng.random(B) < 0.3, rng.integers(0, 1 << 31, B), rng.integers(0, 20, B))
        elif kind == 6:
            r = np.zeros(B) if k % 16 == 6 else np.abs(np.sin(x * rng.uniform(0.05, 1.5))) * 10 ** rng.uniform(1, 9)
        else:
            base = np.cumsum(rng.integers(1, 4, B)).astype(np.float64) ** rng.uniform(1, 4)          # strictly rising over the whole frame
            r = base if k % 16 == 7 else np.concatenate([base[: B // 2], base[: B - B // 2][::-1]])
        rows.append(np.clip(np.asarray(r, dtype=np.float64), 0, 2.0 ** 32 - 1).astype(np.uint32))
    return np.stack(rows)


@pytest.mark.parametrize("bands", [128, 96, 33, 1, 2, 3, 4, 31, 32, 64, 65, 127, 200, 256])
def test_peak_scan_kernels_equal_the_reference_scan(bands):
    """Frame records of the peak-scan kernels (modes 4 / 3: lane per frame — bit masks + event-driven state machine — in rounds of 32 / 16
    bins; mode 2: wave per frame) against a plain restatement of the reference's scan, field by field: candidates, shrunk shoulders, exact prefix sums,
    g, n, the largest candidate."""
    from webspeechanalyzer_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(100 + bands)
    n = 64 * 5 + 17
    spec = np.ascontiguousarray(_peak_frames(rng, n, bands))
    want = [_peak_scan_reference(row) for row in spec]
    for mode in (4, 3, 2):
        if mode == 2 and bands > 128:
            continue
        hdr = np.zeros((n, 4), np.uint32); amp = np.zeros((n, 64), np.uint32); ent = np.zeros((n, 64, 4), np.uint32); flags = np.zeros(1, np.uint32)
        assert L.wsa_debug_peaks(0, spec.ctypes.data, n, bands, mode, hdr.ctypes.data, amp.ctypes.data, ent.ctypes.data, flags.ctypes.data) == 0
        for f in range(n):
            cands, g = want[f]
            row = [int(v) for v in spec[f]]
            P = np.concatenate([[0], np.cumsum(np.asarray(row, dtype=object))])          # P[x + 1] = sum e[0..x]
            if len(cands) > 64:
                assert flags[0] & 1
                continue
            hy = int(hdr[f, 1])
            assert (int(hdr[f, 0]) | ((hy & 0xff) << 32)) == g, (mode, f)
            assert (hy >> 8) & 0xff == len(cands), (mode, f, (hy >> 8) & 0xff, len(cands))
            assert int(hdr[f, 3]) == f * 64
            best_amp, best_bin = 0, 0
            for k, (qi, qs, l, last) in enumerate(cands):
                w = int(ent[f, k, 0])
                assert (w & 0xff, (w >> 8) & 0xff, (w >> 16) & 0xff, w >> 24) == (qi, qs, l, last), (mode, f, k)
                assert int(amp[f, k]) == row[l]
                hi = int(ent[f, k, 3])
                assert int(ent[f, k, 1]) | ((hi & 0xff) << 32) == int(P[qi]), (mode, f, k)
                assert int(ent[f, k, 2]) | (((hi >> 8) & 0xff) << 32) == int(P[qs + 1]), (mode, f, k)
                if not last and row[l] > best_amp:
                    best_amp, best_bin = row[l], l
            assert (int(hdr[f, 2]), (hy >> 16) & 0xff) == (best_amp, best_bin), (mode, f)
        assert flags[0] == 0 or bands > 128


# ---- the 53-feature reduction (csrc/tracker_features.hpp) on hand-built frames -------------------------------------------------------------
FEAT_FRCAP = (126, 288)          # frames the LDS block of the default / the full tracker variant holds (FRCAP = AC * 36 / 40 for AC = 140, 320)
FEAT_LDS_MAX = 2048              # formant_features_lds: one event bit per 64-frame block in a 32-bit word; longer spans take formant_features_wave
FEAT_DBG_LDS = 1024              # frames the test kernel of selector 2 holds in LDS
FEAT_LENGTHS = sorted({1, 2, 3, 14, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4095, 4096, 4097, 6000, 20000}
                      | {c + d for c in FEAT_FRCAP for d in (-1, 0, 1)})
FEAT_PAIRS = 985                 # (variant, case) pairs inside the variants' domains over the 310 cases of _feat_cases()
FEAT_COUNTS = (7, 8, 9, 10, 11)  # results of a column that are counts / integer sums: valid frames, runs, upward and downward bin jumps, events
F32_TINY = float(np.float32(1e-45))
F32_MAX = float(np.finfo(np.float32).max)


def _feat_domain(sel, n):
    """frames the variant behind selector `sel` of wsa_debug_features accepts"""
    return n >= 1 and n <= {0: 1 << 24, 1: 128, 2: FEAT_DBG_LDS, 3: FEAT_LDS_MAX, 4: 15}[sel]


def _feat_frames(kind, n, seed):
    """n frames x [bin, energy, width] x 3 columns (float32).  Bins are integer-valued floats below 256 and the device sums them as integers: the
    straighten step (oracle/backend.c, finalize: `fr[...] = (float)f` with f = a track's peak bin, a band index of a spectrum of at most 256 bands — the
    tracker packs it into 8 bits) can produce nothing else."""
    rng = np.random.default_rng(seed)
    fr = np.zeros((n, 3, 3), np.float32)
    t = np.arange(n)
    fr[:, :, 2] = rng.integers(1, 30, (n, 3))
    if kind == "speech":
        # mostly valid, an energy event (a peak, then a frame below half of it) every 20 - 60 frames at positions of their own in every column: over
        # many blocks the events of block b and block b + 32 sit at different lanes
        for c in range(3):
            fr[:, c, 0] = np.clip(40 + 70 * c + np.cumsum(rng.integers(-3, 4, n)), 1, 255)
            E = 10.0 ** rng.uniform(3, 5) * (1 + 0.3 * np.sin(t / rng.uniform(5, 15))) * rng.uniform(0.9, 1.1, n)
            p = int(rng.integers(1, 20))
            while p < n:
                E[p:p + int(rng.integers(1, 4))] *= rng.uniform(0.05, 0.45)
                p += int(rng.integers(20, 61))
            fr[:, c, 1] = E
            gone = rng.random(n) < 0.04
            fr[gone, c, int(rng.integers(0, 2))] = 0
    elif kind == "all_invalid":
        fr[:, :, 0] = rng.integers(1, 256, (n, 3)); fr[:, :, 1] = 10.0 ** rng.uniform(0, 6, (n, 3))
        z = rng.random((n, 3)) < 0.5
        fr[:, :, 0][z] = 0; fr[:, :, 1][~z] = 0
    elif kind.startswith("one_valid_"):
        pos = {"first": 0, "last": n - 1, "63": 63, "64": 64}[kind[10:]]
        fr[pos, :, 0] = (17, 120, 255); fr[pos, :, 1] = (5000.0, 0.25, 3.0e7)
    elif kind == "alternating_validity":
        # every run has length 1: no frame ever has a valid predecessor (column 2 starts one frame later)
        for c in range(3):
            on = (t + (c == 2)) % 2 == 0
            fr[on, c, 0] = rng.integers(1, 256, int(on.sum())); fr[on, c, 1] = 10.0 ** rng.uniform(-2, 7, int(on.sum()))
    elif kind in ("events_on_last_lanes", "events_on_first_lanes"):
        # an event exactly on frames 63, 127, 2047 / on frames 64, 128, 2048 (an event clears the running maximum, so two neighbours cannot both be
        # events): for lane 0 the predecessor's validity and bin and the running maximum come from the block before.
        # column 0: the plain case, with a bin jump over the edge; column 1: one frame later, a falling jump; column 2: the frame before the edge is invalid,
        # so the edge frame opens a run and is NO event
        fr[:, :, 0] = (30, 90, 200); fr[:, :, 1] = (1000.0, 64.0, 2.0e6)
        for p in ((63, 127, 2047) if kind == "events_on_last_lanes" else (64, 128, 2048)):
            for c, q in ((0, p), (1, p + 1), (2, p)):
                if 1 <= q < n:
                    fr[q, c, 1] *= np.float32(0.375)
                    fr[q:, c, 0] += (7, -5, 3)[c]
            if 1 <= p < n:
                fr[p - 1, 2, 1] = 0
    elif kind == "comparison_edges":
        # runs of [opening frame, L, x] between invalid frames, x at, just below and just above L / 2 (an event needs x < L / 2 exactly) and L at 10 and
        # the next fp32 above it (an event is kept only for L > 10); separators of one or two frames move the runs over the block edges
        f32 = np.float32
        Ls = [f32(10.0), np.nextafter(f32(10.0), f32(np.inf)), f32(1000.0), f32(3.0), np.nextafter(f32(20.0), f32(0)), f32(16777215.0), f32(12.5)]
        for c in range(3):
            fr[:, c, 0] = 0
            p = c
            while p + 3 <= n:
                L = Ls[int(rng.integers(0, len(Ls)))]
                h = f32(L / f32(2))
                x = (h, np.nextafter(h, f32(0)), np.nextafter(h, f32(np.inf)))[int(rng.integers(0, 3))]
                fr[p:p + 3, c, 0] = rng.integers(1, 256, 3); fr[p:p + 3, c, 1] = (f32(1.0), L, x)
                p += 3 + int(rng.integers(1, 3))
    elif kind == "energy_range":
        # from the smallest fp32 denormal to FLT_MAX; dB <= 0 (energy <= 1) is left out of the mean of the positive dB
        fr[:, :, 0] = rng.integers(1, 256, (n, 3))
        E = 10.0 ** rng.uniform(-44.8, 38.5, (n, 3))
        pick = rng.integers(0, 12, (n, 3))
        E[pick == 0] = 1.0; E[pick == 1] = F32_TINY; E[pick == 2] = F32_MAX; E[pick == 3] = 0.99999994
        fr[:, :, 1] = np.minimum(E, F32_MAX)
    elif kind == "bin_jumps":
        # bins alternating 1 and 255: every frame jumps by 254, upward and downward in turn (column 1 the other way round, column 2 with pauses)
        fr[:, 0, 0] = np.where(t % 2 == 0, 1, 255); fr[:, 1, 0] = np.where(t % 2 == 0, 255, 1); fr[:, 2, 0] = np.where(t % 2 == 0, 1, 255)
        fr[:, :, 1] = rng.uniform(500, 900, (n, 3))
        fr[t % 97 == 96, 2, 1] = 0
    else:
        raise ValueError(kind)
    return fr.reshape(n, 9)


def _feat_exact(fr, ctx_max, log10):
    """The oracle's formulas (oracle/backend.c wsa_or_formant_features, ref dist/main.js:2 @B32369) with every sum in np.longdouble (pairwise): what the
    features are before the rounding of a summation order.  dB = 20 log10 E as the oracle and the device compute it (bit-identical, first test above)."""
    ld = np.longdouble
    n = len(fr)
    out = np.zeros((3, 16))
    for c in range(3):
        r, E, wd = (fr[:, 3 * c + k].astype(np.float64) for k in range(3))
        v = (r > 0) & (E > 0)
        m = int(v.sum())
        out[c, 7] = m; out[c, 15] = float(ld(100) * m / n)
        if m == 0:
            continue
        dB = np.array([20 * log10(float(e)) for e in E[v]])
        rl, El, wl, dl = r[v].astype(ld), E[v].astype(ld), wd[v].astype(ld), dB.astype(ld)
        idx = np.flatnonzero(v)
        first = np.concatenate([[True], np.diff(idx) > 1])
        jumps = np.diff(r[v])[~first[1:]]
        out[c, 8] = first.sum(); out[c, 9] = jumps[jumps > 1].sum(); out[c, 10] = -jumps[jumps < -1].sum()
        A, L, S = [], 0.0, 0
        for e, d, f in zip(E[v].tolist(), dB.tolist(), first.tolist()):
            if f:
                L, S = 0.0, 0
            elif e > L:
                L, S = e, 1
            elif S == 1 and e < L / 2:
                if L > 10:
                    A.append(d)
                L, S = 0.0, -1
        with np.errstate(all="ignore"):
            sT, sK = El.sum(), dl.sum()
            mw, mk = rl.sum() / m, dl[dl > 0].sum() / ld(int((dl > 0).sum()))
            out[c, 0] = (rl * dl).sum() / sK; out[c, 1] = np.sqrt(((rl - mw) ** 2).sum() / m); out[c, 2] = mk; out[c, 3] = np.sqrt(((dl - mk) ** 2).sum() / m)
            out[c, 4] = sT / n * 100 / ld(ctx_max); out[c, 5] = sT / m * 100 / ld(ctx_max); out[c, 6] = (wl * dl).sum() / sK
            out[c, 11] = len(A)
            if A:
                Al = np.array(A).astype(ld)
                ma = Al[Al > 0].sum() / ld(int((Al > 0).sum()))
                out[c, 12] = ma; out[c, 13] = np.sqrt(((Al - ma) ** 2).sum() / len(A)); out[c, 14] = 100 * (ma / (sK / m) - 1)
    return out


def _feat_cases():
    cases = []
    for k, c in enumerate(json.load(open(os.path.join(GOLDEN, "features_expected.json")))["cases"]):
        cases.append((f"golden{k}", np.array(c["fr"], np.float32).reshape(-1, 9), float(c["ctx_max"]), np.array([float(x) if isinstance(x, str) else x for x in c["expected"]], np.float64)))
    for n in FEAT_LENGTHS:
        kinds = ["speech", "all_invalid", "one_valid_first", "one_valid_last", "alternating_validity", "events_on_last_lanes", "events_on_first_lanes", "comparison_edges", "energy_range"]
        kinds += [f"one_valid_{p}" for p in (63, 64) if p < n]
        for j, kind in enumerate(kinds):
            cases.append((f"{kind}-{n}", _feat_frames(kind, n, 1000 * n + j), 10.0 ** (3 + j % 5) * 1.37, None))
    # 2^20 of summed upward jumps is crossed near 8260 frames; 1025 / 1089 frames: a lane's own share of 254 per block passes 2^12 in the 17th block
    for n in (1024, 1025, 1089, 2047, 2048, 8000, 8400, 20000):
        cases.append((f"bin_jumps-{n}", _feat_frames("bin_jumps", n, n), 54321.0, None))
    return cases


def test_formant_features_device_functions_against_the_oracle():
    """wsa_debug_features runs ONE wavefront of formant_features_wave (selector 0), formant_features_lds with walking events (1), with block events and
    the frames in LDS (2) or in global memory (3), and the packed form (4) over hand-built frames; the reference is pyoracle.formant_features (pinned to
    formantanalyzer's own function by features_expected.json, whose cases run here against the reference's own outputs).  The device functions write
    x[5 .. 52] — the three columns' sixteen results; x[0 .. 4] (length, its root, the two running sums' quotient, log10 ctx_max, the floor) are the
    caller's in the tracker — so those 48 are compared.  Every variant runs every case inside its domain (1: at most 128 frames, 2: 1024, 3: 2048 —
    formant_features_lds keeps one event bit per 64-frame block in a 32-bit word —, 4: 15) and is refused outside it.
    Tolerances: the project's contract, 1e-4 relative with an absolute floor of 1e-6; counts and NaN patterns exact; and the canary 1e-12 for up to 128
    frames, 1e-12 x a / 128 above (a sum's rounding error grows at most linearly with its terms).  Correct kernels exceed that canary in one family of
    cases: a column whose dB values are all equal has a standard deviation of exactly 0, the device's tree sums give 0.0, and the ORACLE's left-to-right
    mean is an ulp off and returns up to 9.9e-14 — 9.95e-8 in the contract's metric with its floor of 1e-6 (measured against _feat_exact, the same
    formulas in np.longdouble; everywhere else the oracle is within 1.9e-13 of it).  So the canary of a case is the larger of the derived one and eight
    times the oracle's own distance from _feat_exact on that case (tree and left-to-right sums both sit within a small multiple of the same bound),
    and that distance is itself held to the measured 1e-7."""
    from oracle import pyoracle
    from webspeechanalyzer_amd import capi
    L = capi.lib()
    cases = _feat_cases()
    ran = refused = 0
    worst = {}
    fails = []
    for name, fr, ctx_max, want in cases:
        n = len(fr)
        fr = np.ascontiguousarray(fr, np.float32)
        assert np.array_equal(fr[:, 0::3], np.floor(fr[:, 0::3])) and fr[:, 0::3].min() >= 0 and fr[:, 0::3].max() < 256
        if want is None:
            want = pyoracle.formant_features(fr, ctx_max, 0.0, 0.0)
        exact = _feat_exact(fr, ctx_max, pyoracle.lib().wsa_or_log10)
        assert all(same_f64(exact[:, q], want[5:].reshape(3, 16)[:, q]) for q in FEAT_COUNTS), name
        oracle_err = rel_err(want[5:].reshape(3, 16), exact)
        assert oracle_err <= 1e-7, (name, oracle_err)
        worst["oracle vs long double"] = max(worst.get("oracle vs long double", 0.0), oracle_err)
        for sel in range(5):
            out = np.full(53, -7.0)
            rc = L.wsa_debug_features(0, fr.ctypes.data, n, ctx_max, sel, out.ctypes.data)
            if not _feat_domain(sel, n):
                assert rc == 1 and (out == -7.0).all(), (name, sel, rc)           # WSA_ERR_INVALID, nothing run
                refused += 1
                continue
            assert rc == 0, (name, sel, rc)
            ran += 1
            g, w = out[5:].reshape(3, 16), want[5:].reshape(3, 16)
            canary = max(1e-12 * max(1.0, n / 128.0), 8 * oracle_err)
            err = rel_err(g, w)
            worst[sel] = max(worst.get(sel, 0.0), err if np.isfinite(err) else 1e300)
            counts_ok = all(same_f64(g[:, q], w[:, q]) for q in FEAT_COUNTS)
            if not counts_ok or not err <= 1e-4:
                bad = [(c, q, g[c, q], w[c, q]) for c in range(3) for q in range(16) if not rel_err(g[c, q:q + 1], w[c, q:q + 1]) <= 1e-4 or (q in FEAT_COUNTS and not same_f64(g[c, q:q + 1], w[c, q:q + 1]))]
                fails.append(f"{name} selector {sel}: contract: rel err {err:.3g}; (column, result, device, oracle) {bad[:6]}")
            elif not err <= canary:
                bad = [(c, q, g[c, q], w[c, q]) for c in range(3) for q in range(16) if not rel_err(g[c, q:q + 1], w[c, q:q + 1]) <= canary]
                fails.append(f"{name} selector {sel}: canary {canary:.3g}: rel err {err:.3g}; {bad[:6]}")
    print("formant features: pairs run", ran, "refused", refused, "worst rel err per selector", worst)
    for f in fails:
        print("FAIL", f)
    assert not fails, f"{len(fails)} (variant, case) pairs differ from the oracle, the first: {fails[0]}"
    assert len(cases) == 310 and ran == sum(_feat_domain(s, len(c[1])) for c in cases for s in range(5)) == FEAT_PAIRS and ran + refused == 5 * len(cases)

"""The front-end specification FE-1 twice: oracle/frontend.c (fp32, the statement the kernels must equal bit for bit) against tests/fe_ref.py (float64,
numpy.fft.rfft, triangles rebuilt from the DESIGN text) on every hand-built case of tests/fe_cases.py — F1-F8, not only the power spectrum — and the
modelled device-form faults of fe_ref, each of which must change at least one case.  No GPU.

The bound.  A band's u32 may differ from floor(E64[m]) by 1 (truncation of a value a hair off an integer) plus the fp32 transform's error, which is
relative to the LARGEST power bin of the frame: |u32 - floor(E64)| <= 1 + c gain emph[m] sum_k(w[m][k]) max_k(P64[k]); square-root bins take the root of
the power-domain error, |sqrt a - sqrt b| <= sqrt |a - b|: 1 + gain emph[m] sqrt(c 0.25 max P64).  floor(E64) is clamped to [0, 2^32 - 1] (F8), the
maximum runs over the finite bins, and a band whose E64 is not finite is compared arm for arm (+Inf -> 0xffffffff, NaN -> 0).
c is measured, not chosen: the worst ratio (|u32 - floor(E64)| - 1) / (gain emph sum w max P64) over all cases is WORST_RATIO below (the test prints
it and fails if a case exceeds it, so it cannot drift unseen), c = 4 WORST_RATIO, and c must stay under the 5e-5 that tests/test_oracle_frontend.py
allows the power spectrum alone.

Measured (this file's output, `pytest -s`), 521 cases over 22 geometries:
  worst ratio 9.98e-08 (geometry 48k-win1280, case tone-mod3-0, frame 1, band 88); WORST_RATIO is that rounded up, c = 4e-07
  FE_ARMS: all 19 arms taken, none shut (3 bands clamp at kmax and take the fr == 0 arm, 414 narrow bands interpolate, 3232 band values are NaN,
  520 saturate)
  fault                     first case it changes (the model on the oracle's power rows; the partner fault inside the float64 statement)
  padded_tap_multiplies     16k-default overflow-one-bin: bands 2, 3, 4 become 0 where FE-1 gives 8419362, 41122908, 50420660
  flush_denormals           16k-default denormal
  window_by_multiply        none: EQUIVALENT below, with the proof
  odd_last_sample_dropped   16k-win383 tone-64
  saturate_at_2_31          16k-default overflow-one-bin
  emph_index_off_by_one     16k-win256 noise-emphasis
  taps_lo_3                 16k-win258 tone-64
  lane0_partner             16k-win256 tone-64
"""
import numpy as np
import pytest

from tests import fe_cases as fc
from tests import fe_ref

WORST_RATIO = 1.0e-7          # measured: see the docstring
C = 4 * WORST_RATIO


# modelled faults that change no case, each with the proof that none can
EQUIVALENT = {
    "window_by_multiply": "a lane whose samples lie behind the window reads the pair (win - 2, win - 1): its index is clamped INTO the window (fe_pair_index), so "
                          "what is multiplied by the window's 0 is a sample of the frame itself.  x * 0 differs from the select's 0 only for x = Inf or NaN, and "
                          "a frame that holds one is NaN in every power bin already (measured on the oracle: an infinite sample at 0, win / 2, win - 2 or "
                          "win - 1 leaves 257 of 257 bins NaN at 8, 16 and 48 kHz), so both forms write zeros.  The poison cases keep the clamp itself honest.",
}


def _ulp_apart(a, b):
    """distance in fp32 units in the last place between two positive fp32 arrays"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("gname", [g.name for g in fc.GEOMETRIES])
def test_geometry_and_mel_table_against_the_float64_statement(gname):
    g = fc.BY_NAME[gname]
    fe, r = g.oracle(), g.ref()
    assert (fe.nfft, fe.win, fe.hop, fe.kmax, fe.bands) == (r.nfft, r.win, r.hop, r.kmax, r.bands)
    assert np.array_equal(fe.table(0), r.window.astype(np.float32))
    mb = fe.mel_bands()
    if r.spec_type != 1:
        assert mb is None
        return
    assert np.array_equal(mb[0], r.k0) and np.array_equal(mb[1], r.cnt), np.flatnonzero((mb[0] != r.k0) | (mb[1] != r.cnt))
    w32 = fe.table(4)
    w64 = np.concatenate(r.weights)
    assert w32.shape == w64.shape
    # the two evaluate log10 and pow independently: at most one unit in the last place apart
    assert _ulp_apart(w32, w64.astype(np.float32)).max() <= 1


def _compare(case):
    """(worst ratio, where) of one case; asserts the arm-for-arm part and the +-1 where the frame is silent"""
    g = case.geometry
    r = g.ref(case.gain, case.emph)
    want = fc.expected(case).astype(np.float64)
    worst, where = 0.0, None
    for f in range(len(want)):
        E, _, sw, P = r.frame(case.clip[f * r.hop:f * r.hop + r.win])
        fin = np.isfinite(E)
        assert np.array_equal(want[f][~fin], np.where(np.isnan(E[~fin]), 0.0, 4294967295.0)), (g.name, case.name, f)
        pmax = float(P[np.isfinite(P)].max()) if np.isfinite(P).any() else 0.0
        fl = np.clip(np.floor(np.where(fin, E, 0.0)), 0.0, 4294967295.0)
        d = np.maximum(np.abs(want[f] - fl) - 1.0, 0.0)[fin]
        if r.spec_type == 3:
            scale = (r.gain * r.emph) ** 2 * 0.25 * pmax
            d = d * d
        else:
            scale = r.gain * r.emph * sw * pmax
        scale = scale[fin]
        assert not d[scale == 0].any(), (g.name, case.name, f)
        ratio = np.divide(d, scale, out=np.zeros_like(d), where=scale > 0)
        if len(ratio) and ratio.max() > worst:
            worst, where = float(ratio.max()), (g.name, case.name, f, int(np.flatnonzero(fin)[ratio.argmax()]))
    return worst, where


def test_oracle_against_the_float64_statement_on_every_case_and_every_arm_taken():
    fe_ref.FE_ARMS.clear()
    for g in fc.GEOMETRIES:                      # (the triangles are built once per geometry and cached: count them again)
        fe_ref.FeRef(fs=g.fs, **g.oracle_kw())
    worst, where, n = 0.0, None, 0
    for g in fc.GEOMETRIES:
        for case in fc.cases(g.name):
            w, at = _compare(case)
            n += 1
            if w > worst:
                worst, where = w, at
    print(f"\n{n} cases; worst ratio {worst:.3g} at {where}; c = 4 x = {4 * worst:.3g}")
    print("FE_ARMS:", dict(fe_ref.FE_ARMS))
    assert worst <= WORST_RATIO, (worst, where)
    assert C <= 5e-5
    shut = [a for a in fe_ref.ARM_NAMES if fe_ref.FE_ARMS[a] == 0]
    assert not shut, shut
    assert set(fe_ref.FE_ARMS) <= set(fe_ref.ARM_NAMES)


def test_the_searched_cases_sit_inside_their_conditions():
    for gname in fc.OVERFLOW_GEOMETRIES:
        g = fc.BY_NAME[gname]
        fr, gain, bad, padded, own = fc.overflow_search(gname)
        P = g.oracle().power4(fr)
        assert 1 <= len(bad) <= 9 and not np.isnan(P).any() and np.isfinite(fr).all()
        assert padded and own
        out = g.oracle(gain).run(fr)[0]
        assert (out[own] == 0xFFFFFFFF).all() and (out[padded] > 0).all() and (out[padded] < 0xFFFFFFFF).all(), (gname, out[own], out[padded])
    for gname in fc.DEFAULTS:
        g = fc.BY_NAME[gname]
        fr, gain = fc.denormal_search(gname)
        assert int((g.oracle(gain).run(fr)[0] > 0).sum()) >= 8
        fr, gain = fc.f8_search(gname)
        out = g.oracle(gain).run(fr)[0].astype(np.int64)
        E = g.ref(gain).frame(fr, count=False)[0]
        assert any(m > 0 and 0 < out[m - 1] < 0xFFFFFFFF for m in np.flatnonzero(out == 0xFFFFFFFF))
        assert ((out >= 2 ** 31) & (out < 0xFFFFFFFF)).any() and ((E > 0) & (E < 1) & (out == 0)).any()
    narrow, clamp, three = fc.BY_NAME["16k-narrow-low"].ref(), fc.BY_NAME["16k-clamp-kmax"].ref(), fc.BY_NAME["16k-mel160"].ref()
    assert narrow.narrow[:41].sum() >= 5 and not narrow.clamped.any()
    assert clamp.clamped[-1] and (clamp.k0[clamp.clamped] == clamp.kmax).all() and (clamp.cnt[clamp.clamped] == 1).all()
    assert three.bands > 128 and not fc.BY_NAME["16k-mel160"].form()["two_band"]
    ny = fc.BY_NAME["8k-nyquist-narrow"].ref()
    assert ny.kmax == ny.n2 and (ny.k0 + ny.cnt - 1 == ny.n2).any()          # a band reads P[N2]
    assert fc.BY_NAME["8k-nyquist-linear"].ref().kmax == fc.BY_NAME["8k-nyquist-linear"].ref().n2
    gap = fc.BY_NAME["16k-gap"].oracle()
    assert gap.hop > gap.win
    for g in fc.GEOMETRIES:                      # every same_as names a case, and equal frames are what the oracle says too
        by = {c.name: c for c in fc.cases(g.name)}
        for c in by.values():
            if c.same_as:
                assert np.array_equal(fc.expected(c), fc.expected(by[c.same_as])), (g.name, c.name)


def _frames_under(case, fault):
    """the case's u32 frames as the modelled device forms give them (fault None: must be the oracle's)"""
    g = case.geometry
    fe, r, f = g.oracle(case.gain, case.emph), g.ref(case.gain, case.emph), g.form()
    row = np.concatenate([case.clip, case.tail, np.zeros(2, np.float32)])
    out = []
    for k in range(fe.n_frames(len(case.clip))):
        x, behind = fe_ref.device_frame_input(row, k * fe.hop, fe.win, fault if fault in ("window_by_multiply", "odd_last_sample_dropped") else None)
        if not fe_ref.device_frame_is_clean(behind):
            assert np.isnan(behind).any()
            out.append(np.zeros(fe.bands, np.uint32))              # 0 x Inf = NaN enters the transform: every bin NaN, F8 writes zeros
            continue
        if fault in ("lane0_partner", "lane0_partner_as_fe1"):
            out.append(r.frame_from_power(r.power4_split(x, fe_ref.split_partner_bins(fe.kmax, r.n2, f["R8"], fault))))
            continue
        out.append(fc.device_frame(g, fe.power4(x), case.gain, case.emph, fault))
    return np.stack(out)


def test_every_modelled_fault_changes_a_case_and_the_faultless_model_is_the_oracle():
    first = {}
    for g in fc.GEOMETRIES:
        for case in fc.cases(g.name):
            if not case.model:
                continue
            want = fc.expected(case)
            assert np.array_equal(_frames_under(case, None), want), (g.name, case.name)
            for fault in fe_ref.FAULTS:
                if fault in first:
                    continue
                # (the partner fault is judged inside the float64 statement: the packed split with FE-1's partners against the one with lane 0's wrong)
                base = _frames_under(case, "lane0_partner_as_fe1") if fault == "lane0_partner" else want
                if not np.array_equal(_frames_under(case, fault), base):
                    first[fault] = (g.name, case.name)
    print()
    for fault in fe_ref.FAULTS:
        print(f"{fault:26s}{first.get(fault)}")
    assert set(first) | set(EQUIVALENT) == set(fe_ref.FAULTS) and not set(first) & set(EQUIVALENT), (sorted(first), sorted(set(fe_ref.FAULTS) - set(first)))
    # the issue's prediction, on the CPU: the fixed-length chain over zero weights loses the bands whose padded taps see the infinite bin
    g = fc.BY_NAME["16k-default"]
    case = {c.name: c for c in fc.cases(g.name)}["overflow-one-bin"]
    _, _, _, padded, own = fc.overflow_search(g.name)
    bad = _frames_under(case, "padded_tap_multiplies")[1]
    # (a band whose OWN tap is infinite stays 0xffffffff either way: Inf w + finite is Inf, and no padded tap of such a band sees the one infinite bin)
    assert (bad[padded] == 0).all() and (bad[own] == 0xFFFFFFFF).all() and (fc.expected(case)[1][own] == 0xFFFFFFFF).all()

"""The syllables of tests/coeffs_cases.py, from the oracle alone (CPU): pyoracle.syllable_coeffs equals, bit for bit and throw for throw, what the
reference's own make_coeffs returned for every case (tests/golden/coeffs_expected.json, tests/golden/gen/make_coeffs_golden.py), and the cases reach
the paths of csrc/coeffs.hip that tests/test_gpu_coeffs.py is there for — counted here, in the oracle (numeric_js.gradient and the cost function
wrapped by coeffs_cases.oracle_stats), so that the GPU test cannot pass while a path goes unused: the h / 16 retry of numeric.gradient on both sides
of COEF_LDS_PTS = 32 frames — with fits on each side whose bits depend on that retry's step —, a throw on each side, every point count 0 .. 7 in every fit, long BFGS runs and line searches that halve.
The counts are printed (pytest -s) and equal the table coeffs_cases.RECORDED, which the GPU test prints with its layouts."""
import collections
import json
import os
import struct

import numpy as np
import pytest

from oracle import pyoracle
from tests import coeffs_cases as cc
from tests.util import GOLDEN

NAN_COST = "uncmin: f(x0) is a NaN!"


@pytest.fixture(scope="module")
def golden():
    d = json.load(open(os.path.join(GOLDEN, "coeffs_expected.json")))
    return {c["name"]: c for c in d["cases"]}


@pytest.fixture(scope="module")
def stats():
    return {c["name"]: cc.oracle_stats(c) for c in cc.CASES}


def _row(g):
    return np.array([struct.unpack(">d", bytes.fromhex(h))[0] for h in g["row"]])


def test_cases_are_syllables_as_sep_syllables_hands_them_over(golden):
    assert [c["name"] for c in cc.CASES] == list(golden) and 100 <= len(cc.CASES) <= 400
    for c in cc.CASES:
        fr, sm = c["fr"], c["sums"]
        assert fr.dtype == np.float32 and fr.shape == (c["sl"], 9) and sm.dtype == np.float32 and sm.shape == (c["sl"],) and 2 <= c["sl"] <= 300
        bins = fr[:, 0::3]
        assert (bins == np.floor(bins)).all() and bins.min() >= 0 and bins.max() <= 255 and (sm >= 0).all() and np.isfinite(sm).all()
        assert golden[c["name"]]["digest"] == cc.digest(c) and golden[c["name"]]["sl"] == c["sl"], c["name"]      # the fixture is of these very bytes
        assert c["fam"] <= set(cc.FAMILIES) and c["fam"]


def test_oracle_equals_the_reference_bit_for_bit_and_throws_where_it_threw(golden):
    threw = 0
    for c in cc.CASES:
        g = golden[c["name"]]
        try:
            got = pyoracle.syllable_coeffs(c["fr"], cc.sums3(c))
        except ValueError as e:
            assert g["row"] is None and g["threw"] == str(e), (c["name"], g["threw"], str(e))
            threw += 1
            continue
        assert g["threw"] is None, (c["name"], g["threw"])
        want = _row(g)
        assert got.shape == (cc.NCOEF,) and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (c["name"], got, want)
    assert threw == sum(1 for c in cc.CASES if "thrower" in c["fam"]) > 0


def test_fits_on_their_own_join_to_the_row_and_twins_agree(golden, stats):
    """oracle_stats runs every fit by itself (what the GPU test expects of the fits beside a failed one): joined they are the reference's row; a twin
    (frames without points appended past 32 frames) has its original's 23 numbers."""
    for c in cc.CASES:
        row, fits = stats[c["name"]]
        g = golden[c["name"]]
        if g["row"] is None:
            assert row is None and [f["threw"] for f in fits].count(g["threw"]) == 1 and sum(f["threw"] is not None for f in fits) == 1
        else:
            assert np.array_equal(row.view(np.uint64), _row(g).view(np.uint64)), c["name"]
        if c["twin_of"]:
            assert c["sl"] > cc.COEF_LDS_PTS >= cc.CASES[cc.INDEX[c["twin_of"]]]["sl"] and g["row"] == golden[c["twin_of"]]["row"], c["name"]


def test_the_search_finds_the_committed_throwers_and_nothing_else():
    found = cc.search_throwers()
    assert {rs for (order, rs), msg in found.items() if order == 3} == set(cc.THROW_SETS) and len(cc.THROW_SETS) >= 1
    assert set(found.values()) == {NAN_COST}
    others = sorted(k for k in found if k[0] != 3)
    print("throwers outside the order-3 fits:", others or "none found")
    assert ("throw in fit 0 (order 4)" in cc.NOT_FOUND) == (not [k for k in others if k[0] == 4])
    assert ("throw in fit 3 (order 1)" in cc.NOT_FOUND) == (not [k for k in others if k[0] == 1])
    fails = cc.search_gradient_fails()
    print("constant energy sums behind a leading gap that throw:", fails or "none found")


def test_the_cases_reach_the_paths(stats):
    tot = collections.Counter()
    cnt_seen = collections.defaultdict(set)
    msgs = collections.Counter()
    fams = set()
    for c in cc.CASES:
        row, fits = stats[c["name"]]
        side = "lds" if c["sl"] <= cc.COEF_LDS_PTS else "scratch"
        fams |= c["fam"]
        line = []
        for q, f in enumerate(fits):
            cnt_seen[cc.FIT_ORDER[q]].add(f["cnt"])
            assert (f["grads"] > 0 or f["threw"] is not None) == (f["cnt"] > 2) and f["halvings"] >= 0, (c["name"], q, f)
            tot["fits"] += 1
            tot["fits_refined"] += f["grads"] > 0
            tot["gradients"] += f["grads"]
            tot["retries_" + side] += f["retries"]
            tot["retrying_fits_" + side] += f["retries"] > 0
            tot["bfgs_iterations"] += f["iters"]
            tot["max_iterations"] = max(tot["max_iterations"], f["iters"])
            tot["halvings"] += f["halvings"]
            tot["halving_fits"] += f["halvings"] > 0
            tot["fits_over_10_iterations"] += f["iters"] > 10
            tot["throws_" + side] += f["threw"] is not None
            tot["max_gradient_trials"] = max(tot["max_gradient_trials"], f["trials"])
            if f["threw"]:
                msgs[f["threw"]] += 1
            line.append(f"q{q}: {f['cnt']} pts, {f['grads']} grad, {f['retries']} retry, {f['iters']} it, {f['halvings']} halv" + (", THREW" if f["threw"] else ""))
        if c["fam"] & {"retry", "gapretry"}:                     # which of the retrying fits depend on the retry's step
            sens = cc.retry_sensitive(c)
            assert all(fits[q]["retries"] > 0 for q in sens), (c["name"], sens)
            tot["retry_sensitive_fits_" + side] += len(sens)
            line.append(f"a retry by h / 8 changes {sens}")
        print(f"{c['name']:34s} sl {c['sl']:3d}  " + " | ".join(line))
    tot["cases"] = len(cc.CASES)
    print("totals:", dict(tot))
    print("throws by message:", dict(msgs))
    gradient_fails = msgs.get("Numerical gradient fails", 0) > 0
    no_pivot = msgs.get("inv: no pivot", 0) > 0
    # (recorded, not asserted either way: the two paths no case is known to reach)
    print("`Numerical gradient fails`:", "found" if gradient_fails else "not found", "| numeric.inv without a pivot:", "found" if no_pivot else "not found")
    assert fams == set(cc.FAMILIES)
    assert tot["retrying_fits_lds"] >= 20 and tot["retrying_fits_scratch"] >= 20
    assert tot["throws_lds"] >= 1 and tot["throws_scratch"] >= 1
    # retries whose step decides the result's bits: not one lucky fit on either side
    assert tot["retry_sensitive_fits_lds"] >= 10 and tot["retry_sensitive_fits_scratch"] >= 10
    for order in (4, 3, 1):
        assert set(range(8)) <= cnt_seen[order], (order, cnt_seen[order])
    assert tot["fits_over_10_iterations"] >= 1 and tot["halving_fits"] >= 1
    # throwers on fit 1 and on fit 2, LDS and scratch
    where = {(q, c["sl"] <= cc.COEF_LDS_PTS) for c in cc.CASES for q, f in enumerate(stats[c["name"]][1]) if f["threw"]}
    assert {(1, True), (1, False), (2, True), (2, False)} <= where
    assert dict(tot) == cc.RECORDED, dict(tot)


def test_the_families_sit_where_their_names_say():
    by = collections.defaultdict(list)
    for c in cc.CASES:
        for f in c["fam"]:
            by[f].append(c)
    assert {2, 3, 31, 32, 33, 64, 65, 300} <= {c["sl"] for c in by["length"]}
    assert all(c["sl"] > cc.COEF_LDS_PTS and all(3 <= (cc.column(c, q)[:, 1] > 0).sum() <= 5 for q in range(4)) for c in by["sparse"]) and len(by["sparse"]) >= 4
    firsts = {(int(np.flatnonzero(c["fr"][:, 0] > 0)[0]), c["sl"]) for c in by["gap"] if "twin" not in c["fam"]}
    assert {f for f, sl in firsts} >= {1, 17} and any(f == sl - 3 for f, sl in firsts)
    const = [c for c in by["retry"] if len(set(c["sums"].tolist())) == 1 and len(set(c["fr"][:, 0].tolist())) == 1]
    assert {c["sl"] for c in const} >= {3, 31, 32, 33, 64, 65, 300}
    assert {int(np.flatnonzero(c["sums"] > 0)[0]) for c in by["gapretry"]} >= set(cc.GAP_FIRSTS) and len(by["gapretry"]) >= len(cc.GAP_FIRSTS) * len(cc.GAP_POINTS)
    for c in by["counts"]:
        if "twin" not in c["fam"]:
            assert len({int((cc.column(c, q)[:, 1] > 0).sum()) for q in range(4)}) >= 3          # the four columns of a syllable differ in their counts
    assert any(c["sl"] <= cc.COEF_LDS_PTS for c in by["thrower"]) and any(c["sl"] > cc.COEF_LDS_PTS for c in by["thrower"])


def test_layouts_cover_the_geometries():
    lays = {l["name"]: l for l in cc.layouts()}
    assert {len(l["rows"]) for l in lays.values() if l["geometry"] == "batch"} >= {1, 15, 16, 17, 33}
    assert {ci for ci, _, _ in lays["batch-all"]["rows"]} == set(range(len(cc.CASES)))
    assert lays["batch-all"]["rows_cap"] >= len(cc.CASES) + 64                                  # whole waves of rows past n_rows
    thr = {i for i, c in enumerate(cc.CASES) if "thrower" in c["fam"]}
    for name in ("batch-16", "batch-17", "batch-33"):                                            # the first wave: both strides and a thrower
        first = [ci for ci, _, _ in lays[name]["rows"][:16]]
        assert any(cc.CASES[i]["sl"] <= cc.COEF_LDS_PTS for i in first) and any(cc.CASES[i]["sl"] > cc.COEF_LDS_PTS for i in first) and thr & set(first), name
    back_to_back = across = at_zero = at_end = False
    for l in lays.values():
        if l["geometry"] != "batch":
            continue
        fr, sm, off, meta = cc.tables(l)
        for k, (ci, c, st) in enumerate(l["rows"]):
            end = st + cc.CASES[ci]["sl"]
            at_zero |= st == 0
            at_end |= end == l["clips"][c]
            nxt = l["rows"][k + 1] if k + 1 < len(l["rows"]) else None
            if nxt and nxt[1] == c:
                back_to_back |= nxt[2] == end
            if nxt and nxt[1] == c + 1:
                across |= end == l["clips"][c] and nxt[2] == 0
    assert back_to_back and across and at_zero and at_end
    ring = cc.RING
    wraps = {(cc.CASES[ci]["sl"] <= cc.COEF_LDS_PTS) for l in lays.values() if l["geometry"] == "stream" for ci, _, st in l["rows"] if st % ring + cc.CASES[ci]["sl"] > ring}
    assert wraps == {True, False}
    srows = [(ci, c, st) for l in lays.values() if l["geometry"] == "stream" for ci, c, st in l["rows"]]
    assert any(st % ring == ring - 1 for _, _, st in srows) and any(ring - 2 <= cc.CASES[ci]["sl"] <= ring for ci, _, _ in srows)
    assert all(len(l["clips"]) >= 2 and l["ring_mask"] == ring - 1 and l["scratch_stride"] == 2 * ring for l in lays.values() if l["geometry"] == "stream")
    assert any(ci in thr for ci, _, _ in srows)

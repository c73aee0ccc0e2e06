"""The restatement of specification EV-1 (tests/dbeval_ref.py) against the reference application's own code: only_mean / variance /
covariance of src/stats.js and the CCC expression of calc_ccc on each ordinal case, and Label_conf_all after a file's callbacks went
through src/prediction.js, as recorded in tests/golden/dbeval_expected.json (tests/golden/gen/make_dbeval_golden.py).  Counts and file
classes exactly, meter sums bit for bit, the ordinal figures inside the restatement's own running-error bound.  No GPU."""
import math

import numpy as np
import pytest

from . import classify_ref
from . import dbeval_cases as dc
from . import dbeval_ref as ref
from . import dbstats_ref

FX = dc.load_fixture()
ORD = {c["name"]: c for c in FX["ordinal"]}
FOLD = {c["name"]: c for c in FX["fold"]}


def test_fixture_holds_the_cases_of_dbeval_cases():
    assert [c["input"] for c in FX["ordinal"]] == dc.ordinal_golden_cases()
    assert [c["input"] for c in FX["fold"]] == dc.fold_golden_cases()


# ---- part 2 against src/stats.js
@pytest.mark.parametrize("name", sorted(ORD))
def test_agreement_lies_within_its_bound_of_the_references_in_order_values(name):
    c = ORD[name]
    t, p = [dc.dec(v) for v in c["input"]["true"]], [dc.dec(v) for v in c["input"]["pred"]]
    got, plain = ref.agreement(t, p), ref.in_order_agreement(t, p)
    assert got["n"] == plain["n"] == c["n"]
    worst = 0.0
    for k in ref.KEYS:
        want = dc.dec(c[k])
        # the plain in-order form restated in Python is the reference's to the bit (same operations, same order) ...
        assert ref.same_f64([plain[k]], [want]) or k in ("var_true", "var_pred", "ccc", "pearson"), (k, plain[k], want)     # (Math.pow(x, 2) is V8's own)
        # ... and EV-1's chunked two-pass value lies inside the bound of it (two evaluations can be 2 x bound apart; the single bound is asserted)
        if want != want:
            assert got[k] != got[k], (k, got[k])
            continue
        bound = got["bound"][k]
        assert bound == bound, (k, "no bound")
        diff = abs(got[k] - want)
        worst = max(worst, diff / bound if bound else (0.0 if diff == 0 else math.inf))
        print(f"{name}.{k}: EV-1 {got[k]!r}, reference {want!r}, difference {diff:.3e}, bound {bound:.3e}")
        assert diff <= bound, (k, got[k], want, bound)
    assert worst <= 1


def test_the_deviation_from_calc_ccc_is_what_the_fixture_records():
    """calc_ccc passes covariance(y1, y1), which is the variance again; EV-1 passes (y1, y2)"""
    c = ORD["clean_300"]
    assert c["cov_y1_y1"] == c["var_true"] != c["cov"]


def test_rows_up_to_a_chunk_are_summed_in_row_order():
    """with at most R rows chunk order is row order: the restatement equals its own in-order form bit for bit"""
    t, p = dc.ordinal_columns(ref.R, 3, "special")
    got, plain = ref.agreement(t, p), ref.in_order_agreement(t, p)
    assert all(ref.same_f64([got[k]], [plain[k]]) for k in ("mean_true", "mean_pred", "cov"))
    t, p = dc.ordinal_columns(4 * ref.R + 9, 3, "clean")
    got, plain = ref.agreement(t, p), ref.in_order_agreement(t, p)
    assert any(not ref.same_f64([got[k]], [plain[k]]) for k in ref.KEYS), "the chunked order never showed"
    assert all(abs(got[k] - plain[k]) <= got["bound"][k] for k in ref.KEYS)


# ---- part 3 against src/prediction.js
@pytest.mark.parametrize("name", sorted(FOLD))
def test_file_fold_is_prediction_js_bit_for_bit(name):
    c = FOLD[name]
    legend = c["input"]["legend"]
    f_col, c_col, dur, prob, n_files = dc.fold_case_columns(c["input"])
    assert ref.check_files(f_col, dur, n_files) is None
    sums, classes = ref.fold_files(f_col, c_col, dur, prob, legend, list(range(len(legend))), n_files)
    for f, want in enumerate(c["files"]):
        acc = {k: dc.dec(v) for k, v in want["label_conf_all"]}
        for i, lab in enumerate(legend):
            assert ref.same_f64([sums[f][i]], [acc.get(lab, 0.0)]), (f, lab, sums[f][i], acc.get(lab))
        # the file's class by EV-1's rule on the REFERENCE's own table: its keys are in Object.keys order
        best, mx = None, 0.0
        for k, v in want["label_conf_all"]:
            if dc.dec(v) > mx:
                best, mx = k, dc.dec(v)
        assert classes[f] == (-1 if best is None else legend.index(best))


def test_file_classes_of_the_named_cases():
    got = {}
    for name, c in FOLD.items():
        f_col, c_col, dur, prob, n_files = dc.fold_case_columns(c["input"])
        legend = c["input"]["legend"]
        got[name] = [legend[i] if i >= 0 else None for i in ref.fold_files(f_col, c_col, dur, prob, legend, list(range(len(legend))), n_files)[1]]
    assert got == {"plain": ["A", "S"], "one_syllable_callbacks": ["N"], "tie": ["N"], "index_keys": ["3"], "zero_overwritten": ["A"],
                   "skipped_and_blank": [None, "S"]}


# ---- every arm
def test_every_arm_is_taken():
    ref.ARMS.clear()
    classify_ref.FOLD_ARMS.clear()
    for c in FX["ordinal"]:
        ref.agreement([dc.dec(v) for v in c["input"]["true"]], [dc.dec(v) for v in c["input"]["pred"]])
    for c in FX["fold"]:
        f_col, c_col, dur, prob, n_files = dc.fold_case_columns(c["input"])
        ref.fold_files(f_col, c_col, dur, prob, c["input"]["legend"], list(range(4)), n_files)
    t, p = dc.class_columns(300, 5, 1)
    ref.confusion(5, t, p)
    lay = dc.file_layout("straddle")
    v = np.where(np.arange(len(lay["durations"])) % 9 == 4, np.nan, 2.0)
    ref.fold_file_values(lay["file_of_row"], lay["callback_of_row"], lay["durations"], v, lay["n_files"])
    for arm in ("pred.blank", "row.not_counted", "pred.correct", "pred.wrong", "pair.left_out", "pair.taken", "n.zero", "n.positive", "variance.zero",
                "file.tie", "file.blank", "file.class", "file.none", "callback.one_syllable", "callback.several", "value.not_finite", "value.callback_skipped"):
        assert ref.ARMS[arm] > 0, arm
    for arm in ("syllables.one", "all.zero", "skip.zero", "key.index", "key.string"):        # the fold's own arms (tests/classify_ref.py)
        assert classify_ref.FOLD_ARMS[arm] > 0, arm


# ---- part 1: the four invariants against DS-1's table, on the restatements
@pytest.mark.parametrize("variant", ["mixed", "blank", "none", "one"])
def test_confusion_invariants_against_the_table(variant):
    V, n = 7, 300
    t, p = dc.class_columns(n, V, 2, variant)
    m = ref.confusion(V, t, p)
    cat, cls, _ = dbstats_ref.table(np.ones(n), [(V, t, p)], [])
    for v in range(V):
        assert sum(m[v]) == cls["count"][v] and m[v][v] == cls["correct"][v] and sum(m[v][:V]) - m[v][v] == cls["wrong"][v]
    assert sum(m[v][V] for v in range(V)) == cat["blank"][0]
    hot = [(a, b) for a in range(V) for b in range(V + 1) if m[a][b]]
    if variant == "one":
        assert len(hot) == 1 and m[hot[0][0]][hot[0][1]] == n and hot[0][0] != hot[0][1]
    if variant == "none":
        assert hot == []


# ---- one-line faults in the restatement are caught
def _fold_all(fold):
    out = []
    for c in FX["fold"]:
        f_col, c_col, dur, prob, n_files = dc.fold_case_columns(c["input"])
        out.append(fold(f_col, c_col, dur, prob, c["input"]["legend"], list(range(4)), n_files))
    return out


def _file_results_match(results):
    for c, (sums, classes) in zip(FX["fold"], results):
        legend = c["input"]["legend"]
        for f, want in enumerate(c["files"]):
            acc = {k: dc.dec(v) for k, v in want["label_conf_all"]}
            if not all(ref.same_f64([sums[f][i]], [acc.get(lab, 0.0)]) for i, lab in enumerate(legend)):
                return False
            best, mx = None, 0.0
            for k, v in want["label_conf_all"]:
                if dc.dec(v) > mx:
                    best, mx = k, dc.dec(v)
            if classes[f] != (-1 if best is None else legend.index(best)):
                return False
    return True


def test_one_line_faults_are_caught(monkeypatch):
    assert _file_results_match(_fold_all(ref.fold_files))
    # a tie that goes to the LAST key instead of the first
    def last_wins(*a):
        sums, classes = ref.fold_files(*a)
        legend = a[4]
        for f in range(len(classes)):
            mx = sums[f].max()
            if mx > 0:
                order = classify_ref._keys({lab: 1 for lab in legend})
                classes[f] = legend.index([k for k in order if sums[f][legend.index(k)] == mx][-1])
        return sums, classes
    assert not _file_results_match(_fold_all(last_wins))
    # the one-syllable quirk dropped: every class of a lone syllable added
    monkeypatch.setattr(classify_ref, "fold_segment", lambda acc_all, durs, probs, labels: _all_classes(acc_all, durs, probs, labels))
    assert not _file_results_match(_fold_all(ref.fold_files))
    monkeypatch.undo()
    # a present 0 kept instead of overwritten (`if(!acc[label]) acc[label] = wconf`)
    monkeypatch.setattr(classify_ref, "_add", _keep_zero)
    assert not _file_results_match(_fold_all(ref.fold_files))
    monkeypatch.undo()
    # ordinal faults against the fixture: the sample variance, calc_ccc's covariance(y1, y1), a dropped square in the denominator
    c = ORD["clean_300"]
    t, p = [dc.dec(v) for v in c["input"]["true"]], [dc.dec(v) for v in c["input"]["pred"]]
    good = ref.agreement(t, p)
    n = good["n"]
    faults = dict(sample_variance=good["var_true"] * n / (n - 1), cov_y1_y1=good["var_true"],
                  no_square=2 * good["cov"] / (good["var_true"] + good["var_pred"] + abs(good["mean_pred"] - good["mean_true"])))
    for (name, wrong), key in zip(faults.items(), ("var_true", "cov", "ccc")):
        assert abs(wrong - c[key]) > 2 * good["bound"][key], name
    # a row that does not take part counted all the same: a zero in the predicted column
    t2, p2 = dc.ordinal_columns(40, 51, "special")
    loose = ref.in_order_agreement(np.where(t2 == 0, 1e-300, t2), p2)
    assert loose["n"] != ORD["special_40"]["n"]


def _keep_zero(acc, label, w, arm="all"):
    v = acc.get(label)
    if v is None or v != v:
        acc[label] = w
    elif v != 0:
        acc[label] += w


def _all_classes(acc_all, durs, probs, labels):
    acc_seg = {}
    for d, p in zip(durs, probs):
        for lab, conf in classify_ref.classify_multiple(p, labels):
            classify_ref._add(acc_all, lab, conf * math.sqrt(d), "all")
            classify_ref._add(acc_seg, lab, conf * math.sqrt(d), "seg")
    return acc_seg


def test_refusals_of_the_file_columns_are_restated():
    lay = dc.file_layout("straddle")
    f, d, nf = lay["file_of_row"].copy(), lay["durations"].copy(), lay["n_files"]
    assert ref.check_files(f, d, nf) is None
    g = f.copy(); g[210] = 0
    assert ref.check_files(g, d, nf) == ("decreasing", 210)
    g = f.copy(); g[5] = nf
    assert ref.check_files(g, d, nf) == ("outside", 5)
    e = d.copy(); e[7] = 0.0125
    assert ref.check_files(f, e, nf) == ("milliseconds", 7)
    e = d.copy(); e[0] = 0.0125                          # a row without a file may have any duration
    assert ref.check_files(f, e, nf) is None

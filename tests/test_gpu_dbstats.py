"""K8 on the GPU (wsa_dbstats_*, csrc/dbstats.hip) through capi: the decision kernel and the two table passes against the restatement of
specification DS-1 (tests/dbstats_ref.py) — exactly, every f64 bit for bit — and DB prediction end to end against the reference
application's own output (tests/golden/dbstats_expected.json).  Shapes in tests/dbstats_cases.py."""
import copy

import numpy as np
import pytest

from webspeechanalyzer_amd import capi, dbstats

from . import dbstats_cases as dc
from . import dbstats_ref

pytestmark = pytest.mark.gpu

FX = dc.load_fixture()
R = dc.R


@pytest.fixture(scope="module")
def an():
    a = capi.Analyzer(capi.Config(output_level=13), device=0)
    yield a
    a.close()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def test_header_constants_are_the_bindings():
    assert (capi.DBSTATS_MAX_CLASSES, capi.DBSTATS_MAX_HEADS, capi.DBSTATS_CHUNK_ROWS) == (dc.MAX_CLASSES, dc.MAX_HEADS, R) == \
        (dbstats.MAX_CLASSES, dbstats.MAX_HEADS, dbstats.CHUNK_ROWS)


@pytest.mark.parametrize("C", dc.DECIDE_C)
def test_decide_kernel_is_the_restatement(an, torch, C):
    for n in dc.DECIDE_N:
        prob, m = dc.decide_table(n, C, seed=100 * C + n)
        want = dbstats_ref.decide(prob, m)
        db = an.feature_db(None, np.zeros(n), [C], 0)
        d_prob = torch.from_numpy(prob).cuda()
        db.decide_rows(0, d_prob.data_ptr(), C, m, torch.cuda.current_stream().cuda_stream)
        got = db.pred_classes(0, torch.cuda.current_stream().cuda_stream)
        db.close()
        assert got.tolist() == want.tolist(), f"n = {n}, C = {C}"
        if n >= 9:                                   # every crafted row is in the table: ties, zeros, negatives, NaN
            assert -1 in want.tolist() and len(set(want.tolist())) > 1 or C == 1


def _table_cases():
    cases = []
    for i, n in enumerate(dc.TABLE_N):
        cases.append((n, 1, 0, dc.TABLE_V[i % 4], "mixed"))
        cases.append((n, 0, 1, 1, "mixed"))
        cases.append((n, dc.MAX_HEADS, dc.MAX_HEADS, dc.TABLE_V[(i + 1) % 4], "mixed"))
    cases += [(8 * R + 3, dc.MAX_HEADS, dc.MAX_HEADS, dc.MAX_CLASSES, "mixed"), (2 * R + 1, 1, 1, 65, "late"), (2 * R + 1, 2, 2, 2, "blank"),
              (R + 1, 2, 2, 65, "none"), (dc.TABLE_N_LARGE, 1, 1, 65, "late")]
    return cases


def _same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("n,n_cat,n_ord,V,variant", _table_cases())
def test_table_kernels_are_the_restatement_bit_for_bit(an, n, n_cat, n_ord, V, variant):
    dur, cats, ords = dc.table_columns(n, n_cat, n_ord, V, seed=n + 7 * V + n_cat, variant=variant)
    want = dbstats_ref.table(dur, cats, ords)
    db = an.feature_db(None, dur, [V] * n_cat, n_ord)
    for h, (_, t, p) in enumerate(cats):
        db.set_classes(h, t, p)
    for o, (t, p) in enumerate(ords):
        db.set_values(o, t, p)
    got, again = db.table(), db.table()
    db.close()
    assert _same_bits(got, again), "two runs differ"
    for name, g, w in zip(("cat", "cls", "ord"), got, want):
        for f in w.dtype.names:
            assert g[f].tobytes() == w[f].tobytes(), f"{name}.{f}: {g[f][:8]} != {w[f][:8]}"
    if variant == "late" and n_cat:
        assert got[1]["first_row"][V - 1] == n - 1
    if variant == "none":
        assert (got[1]["first_row"] == 0xFFFFFFFF).all() and (got[2]["min"] == np.inf).all() and (got[2]["max"] == 0).all()
    if variant == "blank" and n_cat:
        assert (got[0]["correct"] == 0).all() and (got[0]["wrong"] == 0).all() and (got[0]["blank"] > 0).all()


def _rows(name):
    return copy.deepcopy(FX["scenarios"][name]["rows"])


def test_scenario_a_end_to_end_is_the_references(an):
    sc = FX["scenarios"]["a"]
    rows, heads = _rows("a"), (sc["class_labels"], sc["ordinal_labels"])
    cats_run, ords_run = sc["ml5"]
    preds = dbstats.predict_db(an, rows, heads, "cats", "emotion", dc.model_spec("cats_emotion"))
    assert preds == [res[0]["label"] for res in cats_run["results"]]           # the fixture's margin condition makes this a fair demand
    spec = dc.model_spec("ords_V")
    values = dbstats.predict_db(an, rows, heads, "ords", "V", spec)
    want = np.array(ords_run["results"])
    tol = dc.VALUE_TOL * (spec.out_max - spec.out_min)
    err = float(np.abs(np.array(values) - want).max())
    print(f"predicted values against ml5's: {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
    assert [r["pred"][0] for r in rows] == [p[0] for p in sc["pred_after"]]
    table = dbstats.stats_table(an, rows, *heads)
    # the integers, from the restatement fed ml5's own results (tests/test_dbstats_reference.py holds that to the reference)
    ref_rows = _rows("a")
    for r, p in zip(ref_rows, sc["pred_after"]):
        r["pred"] = copy.deepcopy(p)
    col = dbstats.build_columns(ref_rows, *heads)
    cat, cls, od = dbstats_ref.table(col["durations"], [(len(c["vocab"]), c["true_idx"], c["pred_idx"]) for c in col["cats"]],
                                     [(c["true_value"], c["pred_value"]) for c in col["ords"]])
    ref = dbstats.assemble_table(col, cat, cls, od)
    for g, w in zip(table["cats"], ref["cats"]):
        assert g == w                                                          # durations too: the same rows in the same order
    for g, w in zip(table["ords"], ref["ords"]):
        assert (g["true_n"], g["pred_n"], g["min"], g["max"]) == (w["true_n"], w["pred_n"], w["min"], w["max"])
        print(f"RMSE {g['rmse']:.9f} against the reference's {w['rmse']:.9f}")
        assert abs(g["rmse"] - w["rmse"]) <= tol                               # it cannot move by more than the largest per-row difference
    assert dbstats.stats_lines(table) == sc["lines"]


@pytest.mark.parametrize("name", ["b", "c"])
def test_quirk_scenarios_print_the_references_table(an, name):
    sc = FX["scenarios"][name]
    rows, heads = _rows(name), (sc["class_labels"], sc["ordinal_labels"])
    for run in sc["ml5"]:
        dbstats.predict_db(an, rows, heads, run["type"], run["label"], dc.model_spec(run["model"]))
    assert [r["pred"] for r in rows] == sc["pred_after"]
    assert dbstats.stats_lines(dbstats.stats_table(an, rows, *heads)) == sc["lines"]


def test_predictions_use_the_bits_of_k6(an, torch):
    sc = FX["scenarios"]["a"]
    rows, heads = _rows("a"), (sc["class_labels"], sc["ordinal_labels"])
    feat = np.array([r["features"] for r in rows], np.float64)
    d_feat = torch.from_numpy(feat).cuda()
    s = torch.cuda.current_stream().cuda_stream
    m = an.load_model(dc.model_spec("cats_emotion"))
    d_prob = torch.zeros((len(feat), m.n_classes), dtype=torch.float32, device="cuda")
    m.classify_rows(d_feat.data_ptr(), len(feat), d_prob.data_ptr(), s)
    torch.cuda.synchronize()
    _, raw = dbstats.predict_db(an, rows, heads, "cats", "emotion", m, return_raw=True)
    assert raw.tobytes() == d_prob.cpu().numpy().tobytes()
    m.close()
    m = an.load_model(dc.model_spec("ords_V"))
    d_val = torch.zeros(len(feat), dtype=torch.float64, device="cuda")
    m.regress_rows(d_feat.data_ptr(), len(feat), d_val.data_ptr(), stream=s)
    torch.cuda.synchronize()
    _, raw = dbstats.predict_db(an, rows, heads, "ords", "V", m, return_raw=True)
    assert raw.tobytes() == d_val.cpu().numpy().tobytes()
    m.close()


def test_device_object_refusals(an):
    feat, dur = np.zeros((4, 53)), np.ones(4)
    with pytest.raises(capi.WsaError, match="vocabulary of 257 classes"):
        an.feature_db(feat, dur, [dc.MAX_CLASSES + 1], 0)
    with pytest.raises(capi.WsaError, match="vocabulary of 0 classes"):
        an.feature_db(feat, dur, [0], 0)
    with pytest.raises(capi.WsaError, match=r"9 categorical heads \(limit 8\)"):
        an.feature_db(feat, dur, [2] * (dc.MAX_HEADS + 1), 0)
    with pytest.raises(capi.WsaError, match=r"9 ordinal heads \(limit 8\)"):
        an.feature_db(feat, dur, [], dc.MAX_HEADS + 1)
    with pytest.raises(capi.WsaError, match="at least one row"):
        an.feature_db(np.zeros((0, 53)), np.zeros(0), [2], 0)
    with pytest.raises(capi.WsaError, match="at least one head"):
        an.feature_db(feat, dur, [], 0)
    cls, reg = an.load_model(dc.model_spec("cats_emotion")), an.load_model(dc.model_spec("ords_V"))
    db = an.feature_db(feat, dur, [4], 1)
    with pytest.raises(capi.WsaError, match="regression model"):
        db.predict_classes(0, reg, [0])
    with pytest.raises(capi.WsaError, match="one output unit|softmax"):
        db.predict_values(0, cls, 0.0, 1.0)
    with pytest.raises(capi.WsaError, match="outside -1 .. 3"):
        db.set_classes(0, [0, 1, 4, 0])
    with pytest.raises(capi.WsaError, match="outside -1 .. 3"):
        db.predict_classes(0, cls, [0, 1, 2, 4])
    with pytest.raises(capi.WsaError, match="head 1 of 1"):
        db.set_values(1, np.zeros(4))
    with pytest.raises(capi.WsaError, match="no class prediction"):
        db.probs(4)
    other = capi.Analyzer(capi.Config(output_level=13), device=0)
    foreign_cls, foreign_reg = other.load_model(dc.model_spec("cats_emotion")), other.load_model(dc.model_spec("ords_V"))
    with pytest.raises(capi.WsaError, match="another context"):
        db.predict_classes(0, foreign_cls, [0, 1, 2, 3])
    with pytest.raises(capi.WsaError, match="another context"):
        db.predict_values(0, foreign_reg)
    foreign_cls.close(); foreign_reg.close(); other.close()
    nofeat = an.feature_db(None, dur, [4], 1)
    with pytest.raises(capi.WsaError, match="without feature rows"):
        nofeat.predict_classes(0, cls, [0, 1, 2, 3])
    nofeat.close(); db.close(); cls.close(); reg.close()

"""The row widths of output levels 11 (264 features) and 12 (23) without a GPU: the width-generic float64 restatements pinned to tfjs on
tests/golden/wide_expected.json (tests/golden/gen/make_wide_golden.py; the inputs are regenerated from tests/wide_cases.py's hash), the
recorded distances of tests/wide_cases.py, and the host layers at those widths: nnmodel's files, train's selection and balancing,
dbstats.predict_db.

Measured once, restatement against tfjs 1.7.2's CPU backend (the families' fixture bounds: TR-1 1.82e-6, TR-2 6.44e-6), and D32:
  w264_one_layer  tfjs 2.66e-08   D32 1.49e-08
  w264_stack      (not in the fixture)  D32 2.98e-08
  w23_stack       tfjs 5.93e-08   D32 2.98e-08
  r_w264          (not in the fixture)  D32 7.30e-07
  r_w23           tfjs 5.96e-08   D32 5.96e-08
  forward passes  f264 4.5e-08, f23 3.9e-08 in a probability (bound 1e-5, tests/test_classify_reference.py's)"""
import json
import os

import numpy as np
import pytest

from tests import classify_ref, train_ref
from tests import wide_cases as wc
from tests.test_regress_reference import BOUND as BOUND_TR2
from tests.test_train_reference import BOUND as BOUND_TR1
from webspeechanalyzer_amd import dbstats, nnmodel, train

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLD, "wide_expected.json")) as _f:
    FX = json.load(_f)
PROB_TOL = 1e-5        # a probability of the float64 forward against tfjs's f32 one: the bound of tests/test_classify_reference.py


def expected_epochs(key):
    u = wc.CASES[key]["units"]
    out = []
    for e in FX["cases"][key]["epochs"]:
        ks = [train_ref.unpack(s, (u[l], u[l + 1])) for l, s in enumerate(e["kernels"])]
        bs = [train_ref.unpack(s, (u[l + 1],)) for l, s in enumerate(e["biases"])]
        out.append(dict(e, kernels=ks, biases=bs))
    return out


def forward_spec(name):
    f = wc.forward_inputs(name)
    return nnmodel.ModelSpec(list(f["units"]), list(f["activations"]), [k.copy() for k in f["kernels"]], [b.copy() for b in f["biases"]],
                             f["in_min"].copy(), f["in_max"].copy(), list(f["labels"]))


def test_the_fixture_holds_the_cases_of_the_table():
    assert tuple(FX["cases"]) == wc.FIXTURE_KEYS and tuple(FX["forward"]) == tuple(wc.FORWARD)
    assert FX["tfjs"] == "1.7.2" and FX["backend"] == "cpu"
    assert FX["cases"]["r_w23"]["optimizer"] == "Adam"
    assert os.path.getsize(os.path.join(GOLD, "wide_expected.json")) <= max(
        os.path.getsize(os.path.join(GOLD, n)) for n in os.listdir(GOLD) if n.endswith(".json") and n != "wide_expected.json")


@pytest.mark.parametrize("key", wc.FIXTURE_KEYS)
def test_restatement_matches_tfjs(key):
    c, got, want = wc.CASES[key], wc.restated(key), expected_epochs(key)
    n_train = c["n"] - c["n_val"]
    assert len(got) == len(want) == c["epochs"]
    for g, w in zip(got, want):
        assert g.get("ambiguous", 0) == 0 and g.get("val_ambiguous", 0) == 0     # no row whose count a correct f32 run may turn
        assert (g["correct"], g["val_correct"]) == (w["correct"], w["val_correct"])
        assert w["correct"] == round(w["acc"] * n_train)
    d = train_ref.distance(c, got, want)
    print(f"{key}: restatement vs tfjs {d:.3e} (recorded {c['tfjs']:.3e})")
    assert d <= (BOUND_TR2 if c["regression"] else BOUND_TR1)
    assert d <= 4 * c["tfjs"]                                                     # the recorded figure still describes the case


@pytest.mark.parametrize("key", list(wc.CASES))
def test_recorded_d32_and_bound(key):
    c = wc.CASES[key]
    d = wc.d32(key)
    print(f"{key}: D32 {d:.3e} (recorded {c['d32']:.3e}, bound {wc.bound(c):.3e})")
    assert 0.25 * c["d32"] <= d <= 4 * c["d32"]                                   # libm differences between numpy builds, not another case
    assert wc.bound(c) == max(BOUND_TR2 if c["regression"] else BOUND_TR1, 4 * c["d32"])
    assert (c["tfjs"] is not None) == (key in wc.FIXTURE_KEYS)


@pytest.mark.parametrize("key", list(wc.CASES))
def test_every_case_moves_every_layer(key):
    i, r = wc.inputs(key), wc.restated(key)
    assert i["feat"].shape == (wc.CASES[key]["n"], wc.CASES[key]["units"][0])
    for l in range(len(i["kernels"])):
        assert np.abs(r[-1]["kernels"][l] - i["kernels"][l]).max() > 1e-3
        assert np.abs(r[-1]["kernels"][l][-1] - i["kernels"][l][-1]).max() > 0      # the LAST input row too (input 263 / 22 at layer 0)


@pytest.mark.parametrize("name", list(wc.FORWARD))
def test_forward_matches_tfjs(name):
    f, spec = wc.forward_inputs(name), forward_spec(name)
    want = train_ref.unpack(FX["forward"][name]["prob"], (FX["forward"][name]["rows"], spec.units[-1]))
    got = classify_ref.forward(spec, f["feat"])
    err = float(np.abs(got - want).max())
    print(f"{name}: float64 forward vs tfjs {err:.3e}")
    assert got.shape == want.shape == (wc.FORWARD[name]["rows"], spec.units[-1]) and err <= PROB_TOL
    assert np.ptp(want, axis=0).min() > 0.05                                      # the rows tell the classes apart: not a flat table


# ---- nnmodel at the three widths
@pytest.mark.parametrize("name", list(wc.FORWARD))
def test_save_dir_load_dir_round_trip(name, tmp_path):
    spec = forward_spec(name)
    w = spec.units[0]
    nnmodel.save_dir(spec, str(tmp_path / "a"))
    back = nnmodel.load_dir(str(tmp_path / "a"))
    assert back.units == spec.units and back.activations == spec.activations and back.labels == spec.labels
    assert all(a.tobytes() == b.tobytes() for a, b in zip(back.kernels + back.biases, spec.kernels + spec.biases))
    assert back.in_min.tobytes() == spec.in_min.tobytes() and back.in_max.tobytes() == spec.in_max.tobytes()
    nnmodel.save_dir(back, str(tmp_path / "b"))
    for fn in ("model.json", "model_meta.json", "model.weights.bin"):
        assert open(tmp_path / "a" / fn, "rb").read() == open(tmp_path / "b" / fn, "rb").read()
    meta = json.load(open(tmp_path / "a" / "model_meta.json"))
    assert meta["inputUnits"] == [w] and list(meta["inputs"]) == [str(k) for k in range(w)]


def test_regression_round_trip_at_23():
    c, i = wc.CASES["r_w23"], wc.inputs("r_w23")
    spec = nnmodel.ModelSpec(list(c["units"]), list(c["activations"]), i["kernels"], i["biases"], i["in_min"], i["in_max"], [], i["out_min"], i["out_max"])
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        nnmodel.save_dir(spec, td)
        back = nnmodel.load_dir(td)
    assert back.is_regression and back.units == [23, 8, 1] and (back.out_min, back.out_max) == (i["out_min"], i["out_max"])
    assert back.in_min.tobytes() == i["in_min"].tobytes()


@pytest.mark.parametrize("width", [63, 9, 52, 265])
def test_other_widths_are_refused(width, tmp_path):
    s = forward_spec("f23")
    ks, bs = train_ref.hash_init([width, 8, 3], 1)
    bad = nnmodel.ModelSpec([width, 8, 3], s.activations, ks, bs, np.zeros(width), np.ones(width), s.labels)
    nnmodel.save_dir(bad, str(tmp_path))
    with pytest.raises(nnmodel.ModelFormatError, match=f"the model takes {width} inputs; the feature rows have 53"):
        nnmodel.load_dir(str(tmp_path))
    with pytest.raises(ValueError, match="expected"):
        train.prepare(np.zeros((12, width)), ["a"] * 12, ["a"])
    with pytest.raises(ValueError, match="expected"):
        train.prepare_ordinal(np.zeros((12, width)), [0.5] * 12)


# ---- train.prepare / prepare_ordinal: the same rows selected and duplicated whatever the width
def _labels(n):
    lab = [("a", "b", "c", None, "zz")[int(h) % 5] for h in wc.mix(np.arange(n), 1, 5)]
    return lab, [None if int(h) % 7 == 0 else float(h % 120) / 100.0 for h in wc.mix(np.arange(n), 2, 5)]


@pytest.mark.parametrize("width", wc.WIDTHS)
def test_prepare_selects_and_balances_as_at_53(width):
    n = 64
    lab, vals = _labels(n)
    wide, _ = wc.cluster_rows(n, width, 3, 3)
    narrow, _ = wc.cluster_rows(n, 53, 3, 3)
    a, b = train.prepare(wide, lab, ["a", "b", "c"]), train.prepare(narrow, lab, ["a", "b", "c"])
    assert a["rows"] == b["rows"] and a["counts"] == b["counts"] and a["legend"] == b["legend"] and np.array_equal(a["y"], b["y"])
    assert len(set(a["counts"])) == 1 and len(a["rows"]) > len(set(a["rows"]))         # balanced, by duplicates
    assert a["features"].shape == (len(a["rows"]), width) and np.array_equal(a["features"], wide[a["rows"]])
    assert np.array_equal(a["in_min"], wide[a["rows"]].min(axis=0)) and a["in_max"].shape == (width,)
    assert train.stack(train.DEFAULT_LAYERS, 3, width)[0] == [width, 8, 3] and train.stack(train.DEFAULT_LAYERS, 3)[0] == [53, 8, 3]
    o, p = train.prepare_ordinal(wide, vals), train.prepare_ordinal(narrow, vals)
    assert o["rows"] == p["rows"] and o["counts"] == p["counts"] and np.array_equal(o["values"], p["values"])
    assert o["features"].shape == (len(o["rows"]), width) and (o["out_min"], o["out_max"]) == (p["out_min"], p["out_max"])
    assert train.stack_regression(train.DEFAULT_LAYERS_ORDS, width)[0] == [width, 64, 16, 1]


# ---- dbstats.predict_db takes the width from the rows (the device behind a stand-in: K8 itself runs in tests/test_gpu_wide.py)
class _Model:
    def __init__(self, spec):
        self.spec, self.labels, self.n_classes, self.n_inputs = spec, list(spec.labels), spec.n_classes, int(spec.units[0])

    def close(self):
        pass


class _DB:
    def __init__(self, log, feat):
        self.log, self.feat = log, feat

    def predict_classes(self, head, model, legend_to_vocab, stream=0):
        self.log.append("predict_classes")
        self.prob = classify_ref.forward(model.spec, self.feat)

    def pred_classes(self, head, stream=0):
        return self.prob.argmax(axis=1).astype(np.int32)

    def close(self):
        pass


class _Analyzer:
    def __init__(self):
        self.log = []

    def load_model(self, spec):
        return _Model(spec)

    def feature_db(self, feat, dur, vocab, n_ord):
        self.log.append(("feature_db", feat.shape))
        return _DB(self.log, feat)


def test_predict_db_takes_the_width_from_the_rows():
    f, spec = wc.forward_inputs("f264"), forward_spec("f264")
    rows = [dict(time=["0.000", "0.100"], features=list(x), true=None, pred=None) for x in f["feat"]]
    an = _Analyzer()
    preds = dbstats.predict_db(an, rows, ([{"k": ["*"]}], []), "cats", "k", spec)
    assert an.log == [("feature_db", (40, 264)), "predict_classes"]
    assert preds == [spec.labels[c] for c in classify_ref.forward(spec, f["feat"]).argmax(axis=1)] and len(set(preds)) > 1
    assert all(r["pred"] == [{"k": p}, {}] for r, p in zip(rows, preds))


def test_predict_db_refuses_a_53_input_model_on_264_wide_rows_before_the_device():
    f = wc.forward_inputs("f264")
    rows = [dict(time=["0.000", "0.100"], features=list(x), true=None, pred=None) for x in f["feat"][:3]]
    narrow = classify_ref.seeded_spec(widths=(4, 4))
    assert narrow.units[0] == 53
    an = _Analyzer()
    with pytest.raises(ValueError, match="the model takes 53 inputs; the DB's rows have 264 features"):
        dbstats.predict_db(an, rows, ([{"k": ["*"]}], []), "cats", "k", narrow)
    assert an.log == [] and all(r["pred"] is None for r in rows)
    with pytest.raises(ValueError, match="53 features"):
        dbstats.predict_db(an, [dict(time=[0, 1], features=[0.0] * 63)], ([], []), "cats", "k", narrow)

"""Specification TR-2 against tfjs itself: the float64 restatement (tests/regress_ref.py) on the fixture's cases
(tests/golden/regress_expected.json, trained by the reference's own ml5 / tfjs 1.7.2 with meanSquaredError and tf.train.adam on given
initial weights and orders, four epochs each).

D, the largest absolute difference in any weight or per-epoch loss between the restatement and tfjs, measured once per case:
a 5.96e-8, b 1.609e-6 (learning rate 0.2: Adam moves every weight by about the rate per step, whatever the gradient's size, so tfjs's
f32 gradients show most here), c 5.96e-8, d 2.28e-8."""
import numpy as np
import pytest

from tests import regress_ref, train_ref

D_MEASURED = 1.609e-6
BOUND = 4 * D_MEASURED          # the project's margin for the f32-versus-f64 noise of a correct implementation (test_train_reference.BOUND)

FX = regress_ref.load_fixture()
CASES = {c["key"]: c for c in FX["cases"]}
KEYS = sorted(CASES)
WRONG = dict(no_bias_correction=dict(bias_correction=False), acc_beta_reset_every_epoch=dict(carry_acc=False),
             epsilon_inside_the_root=dict(eps_inside=True), nominal_batch_size=dict(own_batch_size=False), raw_targets=dict(raw_targets=True))


@pytest.fixture(scope="module")
def restated():
    return {k: regress_ref.run_case(FX, c) for k, c in CASES.items()}


def test_the_fixture_has_the_cases_the_specification_needs():
    assert FX["ml5"] == "0.6.0" and FX["tfjs"] == "1.7.2" and FX["backend"] == "cpu"
    assert [k[0] for k in KEYS] == ["a", "b", "c", "d"] and "feat" not in json_keys() and FX["rows_from"] == "train_expected.json"
    a, b, c, d = (CASES[k] for k in KEYS)
    n_train = len(FX["feat"]) - a["n_val"]
    assert len(FX["feat"]) == len(FX["values"]) == 50 and all(x["n_val"] == 5 and len(x["orders"]) == 4 for x in CASES.values())
    assert (a["units"], a["activations"], a["batch"], a["lr"]) == ([53, 16, 1], ["sigmoid", "sigmoid"], 16, 0.01)
    assert (b["units"], b["activations"], b["batch"], b["lr"]) == ([53, 64, 16, 1], ["sigmoid"] * 3, 10, 0.2)      # nn_default_options_ords
    assert (c["units"], c["activations"], c["batch"]) == ([53, 8, 1], ["relu", "linear"], 7) and n_train % 7 == 3 and "dead_unit" in c["init"]
    assert (d["units"], d["activations"], d["batch"]) == ([53, 272, 1], ["tanh", "sigmoid"], 64) and d["batch"] > n_train
    for x in CASES.values():
        assert len({tuple(o) for o in x["orders"]}) == 4               # a different order per epoch
    t = regress_ref.normalise_target(FX["values"], FX["out_min"], FX["out_max"])
    assert FX["out_min"] == min(FX["values"]) and FX["out_max"] == max(FX["values"]) and (FX["out_min"], FX["out_max"]) != (0.0, 1.0)
    assert ((t == 0) | (t == 1)).sum() >= 10                           # rows that can count as accurate


def json_keys():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regress_expected.json")) as f:
        return set(json.load(f))


def test_the_fixture_is_no_larger_than_the_classifiers():
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(gold, "regress_expected.json")) <= os.path.getsize(os.path.join(gold, "train_expected.json"))


@pytest.mark.parametrize("key", KEYS)
def test_restatement_matches_tfjs(key, restated):
    case, got, want = CASES[key], restated[key], train_ref.expected_epochs(CASES[key])
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g["min_gap"] >= 1e-3                                  # the condition under which counts are compared exactly
        assert (g["correct"], g["val_correct"]) == (w["correct"], w["val_correct"])
    assert sum(w["correct"] + w["val_correct"] for w in want) > 0    # the accuracy rule is exercised: some rows do count
    d = train_ref.distance(case, got, want)
    print(f"{key}: D = {d:.3e}")
    assert d <= BOUND


@pytest.mark.parametrize("variant", sorted(WRONG))
def test_wrong_variants_miss_the_fixture(variant):
    """Measured: the smallest miss of any variant on any case it applies to is 3.5e-3 (epsilon inside the root, case d), 540 x the bound."""
    for key in KEYS:
        case = CASES[key]
        if variant == "nominal_batch_size" and case["batch"] >= len(FX["feat"]) - case["n_val"]:
            continue                                                 # one step over all training rows: there is no short batch
        d = train_ref.distance(case, regress_ref.run_case(FX, case, **WRONG[variant]), train_ref.expected_epochs(case))
        print(f"{variant} {key}: {d:.3e}")
        assert d > 100 * BOUND


def test_accuracy_is_binary_accuracy_not_categorical():
    """categoricalAccuracy over one unit would count every row (argmax of one column is 0 on both sides); tfjs's counts are far below"""
    for key in KEYS:
        n_train = len(FX["feat"]) - CASES[key]["n_val"]
        assert all(e["correct"] < n_train // 2 for e in CASES[key]["epochs"])


def test_a_dead_unit_never_moves_in_tfjs_either():
    case = next(c for c in CASES.values() if "dead_unit" in c["init"])
    u = case["init"]["dead_unit"]
    k0, b0 = train_ref.case_weights(case)
    last = train_ref.expected_epochs(case)[-1]
    assert (last["kernels"][0][:, u] == k0[0][:, u]).all() and last["biases"][0][u] == b0[0][u]
    assert not np.array_equal(last["kernels"][0], k0[0])


def test_unnormalise_rounds_the_product_and_the_sum_separately():
    p = np.float32(0.3)
    want = float(p) * (0.8 - 0.2) + 0.2
    assert regress_ref.unnormalise([p], 0.2, 0.8)[0] == want


def test_sanity_data_trains_in_the_restatement():
    """the data of the GPU sanity run with the app's default stack: the restatement's own last / first loss ratio is below 0.25.
    Learning rate 0.02: at the app's own 0.2 Adam saturates the sigmoids within the first epoch on these rows and the loss stays at
    the targets' variance (0.094 after 0.142), in the restatement as in tfjs's arithmetic."""
    feat, y, mn, mx = regress_ref.smooth_target()
    ks, bs = train_ref.hash_init([53, 64, 16, 1], 9)
    t = regress_ref.normalise_target(y, y.min(), y.max())
    out = regress_ref.run(train_ref.normalise(feat, mn, mx), t, ks, bs, ["sigmoid"] * 3, 80, 32, 0.02, [None] * 30)
    print(out[0]["loss"], out[-1]["loss"])
    assert out[-1]["loss"] < 0.25 * out[0]["loss"]

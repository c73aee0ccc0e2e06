"""Specification TR-1 against tfjs itself: the float64 restatement (tests/train_ref.py) on the fixture's cases
(tests/golden/train_expected.json, trained by the reference's own ml5 / tfjs 1.7.2 on given initial weights and orders)."""
import pytest

from tests import train_ref

# D: the largest absolute difference in any weight or per-epoch loss between the restatement and tfjs over all fixture cases, measured
# once (4.56e-7, in case d, whose losses are near 4.7; the others 0.6e-7 .. 1.0e-7).  The cases are fixed: the margin only covers libm differences between numpy builds.
D_MEASURED = 4.56e-7
BOUND = 4 * D_MEASURED

FX = train_ref.load_fixture()
CASES = {c["key"]: c for c in FX["cases"]}


@pytest.fixture(scope="module")
def restated():
    return {k: train_ref.run_case(FX, c) for k, c in CASES.items()}


def test_the_fixture_has_the_cases_the_specification_needs():
    assert FX["ml5"] == "0.6.0" and FX["tfjs"] == "1.7.2" and FX["backend"] == "cpu"
    keys = sorted(CASES)
    assert [k[0] for k in keys] == ["a", "b", "c", "d", "e"]
    n_train = len(FX["feat"]) - CASES[keys[0]]["n_val"]
    assert n_train % CASES[keys[0]]["batch"] == 13 and CASES[keys[4]]["batch"] > n_train and 272 in CASES[keys[2]]["units"]


@pytest.mark.parametrize("key", sorted(CASES))
def test_restatement_matches_tfjs(key, restated):
    case, got, want = CASES[key], restated[key], train_ref.expected_epochs(CASES[key])
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert g["min_gap"] >= 1e-3                                  # the condition under which counts are compared exactly
        assert (g["correct"], g["val_correct"]) == (w["correct"], w["val_correct"])
    d = train_ref.distance(case, got, want)
    print(f"{key}: D = {d:.3e}")
    assert d <= BOUND


def test_clipped_rows_pass_no_gradient(restated):
    case = next(c for c in CASES.values() if "dead_unit" in c["init"])
    assert restated[case["key"]][0]["clipped"] >= 1                  # epoch 1 has a row clipped from below ...
    wrong = train_ref.run_case(FX, case, clip_rule=False)
    assert train_ref.distance(case, wrong, train_ref.expected_epochs(case)) > BOUND     # ... and tfjs gives it no gradient
    u = case["init"]["dead_unit"]                                    # the dead relu unit never moves, in tfjs either
    k0 = train_ref.case_weights(case)[0][0]
    assert (train_ref.expected_epochs(case)[-1]["kernels"][0][:, u] == k0[:, u]).all()


def test_the_short_last_batch_is_averaged_over_its_own_size():
    case = CASES[sorted(CASES)[0]]
    wrong = train_ref.run_case(FX, case, own_batch_size=False)
    assert train_ref.distance(case, wrong, train_ref.expected_epochs(case)) > BOUND


def test_sanity_data_trains_in_the_restatement():
    """the data of the GPU sanity run: the restatement's own last / first loss ratio is below 0.25"""
    feat, lab, mn, mx = train_ref.separable_clusters()
    ks, bs = train_ref.hash_init([53, 8, 4], 9)
    out = train_ref.run(train_ref.normalise(feat, mn, mx), lab, ks, bs, ["relu", "softmax"], 80, 32, 0.2, [None] * 30)
    assert out[-1]["loss"] < 0.25 * out[0]["loss"]

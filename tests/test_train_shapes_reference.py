"""The cases of tests/train_cases.py through the float64 restatements alone: every condition under which tests/test_gpu_train_shapes.py
compares K7 with them holds, and each case tells the wrong variant of the kernel edge it exists for (train_ref.FAULTS) from the right
one by more than its bound.

Measured, as the distance of the faulted run from the unfaulted one (the bounds are 1.82e-6 for TR-1 and 6.44e-6 for TR-2): "last_row"
1.3e-3 (r_big_batch) and 5.1e-3 (big_batch) at the least, up to 1.5 (batch_1, where the last row is the only one); "rows_past_1024" 7.8e-2
and 1.9e-2; "steps_past_256" 9.3e-2 and 6.8e-3; "last_unit" 2.2e-1 and 9.1e-2.  Ambiguous rows: at most 7 of an epoch's 3400 evaluated
rows (big_batch), 3 of 440 (widest), 2 of 220 (classes_33), none elsewhere; the stillest kernel of any case moves 3.6e-3 (r_wide)."""
import numpy as np
import pytest

from tests import train_cases as tc
from tests import train_ref

KEYS = list(tc.CASES)
FAULT_CASES = [("last_row", k) for k in KEYS] + [("rows_past_1024", "big_batch"), ("rows_past_1024", "r_big_batch"), ("steps_past_256", "batch_1"),
                                                 ("steps_past_256", "r_batch_1"), ("last_unit", "width_edges"), ("last_unit", "r_width_edges")]


def test_the_table_has_the_shapes_the_edges_need():
    c = tc.CASES
    steps = lambda k: [min(c[k]["batch"], c[k]["n"] - c[k]["n_val"] - s) for s in range(0, c[k]["n"] - c[k]["n_val"], c[k]["batch"])]
    assert len(c["one_layer"]["units"]) == 2 and len(c["r_one_layer"]["units"]) == 2
    assert c["width_edges"]["units"][1:5] == [16, 17, 15, 1] and c["width_edges"]["n_val"] == 0 and steps("width_edges") == [17, 17, 17, 17, 13]
    assert c["r_width_edges"]["units"][1:] == [16, 17, 15, 1] and c["r_width_edges"]["n_val"] == 0 and "linear" in c["width_edges"]["activations"][:-1]
    assert len(c["eight_layers"]["units"]) == 9 and steps("eight_layers") == [16] * 4
    assert c["widest"]["units"][1:] == [1024, 64] and c["r_wide"]["units"][1] == 1024 and c["classes_33"]["units"][-1] == 33
    for k in ("big_batch", "r_big_batch"):
        assert steps(k) == [1100, 1100, 170] and c[k]["n_val"] == 1030 and (1100 + 15) // 16 * 16 // 16 == 69
    for k in ("batch_1", "r_batch_1"):
        assert steps(k) == [1] * 300 and c[k]["n_val"] > c[k]["batch"]
    assert steps("last_of_1") == [16, 16, 1]
    assert c["r_relu_out"]["activations"][-1] == "relu" and c["r_width_edges"]["activations"][-1] == "tanh" and c["r_big_batch"]["activations"] == ["sigmoid"] * 3
    for k in KEYS:
        orders = tc.inputs(k)["orders"]
        n_train = c[k]["n"] - c[k]["n_val"]
        assert len(orders) == c[k]["epochs"] in (2, 3) and orders[1] is None
        assert sorted(orders[0].tolist()) == list(range(n_train)) and orders[0].tolist() != list(range(n_train))
        i = tc.inputs(k)
        assert (i["in_min"] < i["feat"].min(axis=0)).all() and (i["in_max"] > i["feat"].max(axis=0)).all()


@pytest.mark.parametrize("key", KEYS)
def test_the_case_meets_the_conditions_of_the_gpu_comparison(key):
    c, i, got = tc.CASES[key], tc.inputs(key), tc.restated(key)
    n_train = c["n"] - c["n_val"]
    assert len(got) == c["epochs"]
    for e in got:
        assert all(np.isfinite(a).all() for a in e["kernels"] + e["biases"]) and np.isfinite([e["loss"], e["val_loss"]]).all()
    moved = [float(np.abs(got[-1]["kernels"][l].astype(np.float64) - i["kernels"][l]).max()) for l in range(len(i["kernels"]))]
    print(f"{key}: stillest kernel moved {min(moved):.2e}")
    assert min(moved) >= 1e-3
    if c["regression"]:
        t = i["t"]
        assert (t[:n_train] == 0.0).any() and (t == 1.0).any() and t.min() == 0.0 and t.max() == 1.0     # rows binaryAccuracy can count
        for e in got:
            assert e["min_gap"] >= 1e-3                                  # the condition under which counts are compared exactly
    else:
        for e in got:
            assert e["clipped"] == 0                                     # no case is built to have clipped rows
            print(f"{key}: ambiguous rows {e['ambiguous']} of {n_train}, {e['val_ambiguous']} of {c['n_val']}")
            assert e["ambiguous"] + e["val_ambiguous"] <= 0.02 * c["n"]  # the rows evaluated in the epoch: every row once


@pytest.mark.parametrize("key", KEYS)
def test_d32_is_the_recorded_one(key):
    d = tc.d32(key)
    print(f"{key}: D32 = {d:.3e} (recorded {tc.CASES[key]['d32']:.3e}, bound {tc.bound(tc.CASES[key]):.3e})")
    assert 0.0 < d <= 2.0 * tc.CASES[key]["d32"]


def test_the_bounds_are_the_fixtures_own_where_d32_is_small():
    for key in KEYS:
        c = tc.CASES[key]
        assert tc.bound(c) == max(6.436e-6 if c["regression"] else 1.824e-6, 4 * c["d32"])


@pytest.mark.parametrize("fault,key", FAULT_CASES)
def test_the_wrong_variant_is_told_apart(fault, key):
    c = tc.CASES[key]
    d = train_ref.distance(c, tc.restate(key, fault=fault), tc.restated(key))
    print(f"{fault} on {key}: {d:.3e} (bound {tc.bound(c):.3e})")
    assert d > tc.bound(c)


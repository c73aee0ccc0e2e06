"""K7 on the GPU at its kernels' tile, batch and width edges: the cases of tests/train_cases.py (its docstring names the edge each one
reaches) against the float64 restatements of TR-1 and TR-2, which tests/test_train_shapes_reference.py shows to meet every condition
used here.  bound(case) = max(the family's fixture bound, 4 x D32(case)) comes from the references alone.

Measured on an MI355X, device against restatement (D32 beside it; bound 1.82e-6 for TR-1, 6.44e-6 for TR-2):
  one_layer      4.47e-08  (D32 2.98e-08)
  width_edges    8.94e-08  (D32 5.96e-08)
  eight_layers   8.94e-08  (D32 5.96e-08)
  widest         1.42e-07  (D32 1.45e-07)
  classes_33     1.79e-07  (D32 1.19e-07)
  big_batch      5.96e-08  (D32 5.96e-08)
  batch_1        1.79e-07  (D32 1.79e-07)
  last_of_1      2.98e-08  (D32 1.49e-08)
  r_one_layer    5.37e-08  (D32 1.49e-08)
  r_width_edges  5.96e-08  (D32 5.96e-08)
  r_wide         2.34e-06  (D32 4.75e-07)
  r_relu_out     5.96e-08  (D32 2.98e-08)
  r_big_batch    8.94e-08  (D32 5.96e-08)
  r_batch_1      1.19e-07  (D32 1.19e-07)
Counts equal the restatement's in every epoch of every case, the ambiguous ones included.  K6 over the trained weights: eight_layers
5.9e-8, widest 2.4e-7, classes_33 2.4e-7 (bound 1e-5); r_wide 5.8e-7 (bound 1e-5 of the range = 6.9e-6)."""
import hashlib

import numpy as np
import pytest

from tests import classify_ref, regress_ref, train_ref
from tests import train_cases as tc
from webspeechanalyzer_amd import capi, nnmodel

pytestmark = pytest.mark.gpu

K6_KEYS = ("eight_layers", "widest", "classes_33", "r_wide")    # K6 over the trained weights at the same limits
RERUN_KEYS = ("big_batch", "batch_1", "r_big_batch", "r_batch_1")


@pytest.fixture(scope="module")
def an():
    a = capi.Analyzer(capi.Config(output_level=13), device=0)
    yield a
    a.close()


def spec_of(key):
    c, i = tc.CASES[key], tc.inputs(key)
    ks, bs = [k.copy() for k in i["kernels"]], [b.copy() for b in i["biases"]]
    if c["regression"]:
        return nnmodel.ModelSpec(list(c["units"]), list(c["activations"]), ks, bs, i["in_min"].copy(), i["in_max"].copy(), [], i["out_min"], i["out_max"])
    return nnmodel.ModelSpec(list(c["units"]), list(c["activations"]), ks, bs, i["in_min"].copy(), i["in_max"].copy(), [f"c{j}" for j in range(c["units"][-1])])


def _k6(model, spec, feat, regression):
    """K6 over `feat` with the trainer's snapshot, and the float64 forward of the same weights"""
    import torch
    d_feat = torch.from_numpy(np.ascontiguousarray(feat, np.float64)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    if regression:
        d_out = torch.full((len(feat),), -7.0, dtype=torch.float64, device="cuda")
        model.regress_rows(d_feat.data_ptr(), len(feat), d_out.data_ptr(), None, None, s)
        want = regress_ref.predict(feat, spec.kernels, spec.biases, spec.activations, spec.in_min, spec.in_max, spec.out_min, spec.out_max)[1]
    else:
        d_out = torch.full((len(feat), spec.units[-1]), -1.0, dtype=torch.float32, device="cuda")
        model.classify_rows(d_feat.data_ptr(), len(feat), d_out.data_ptr(), s)
        want = classify_ref.forward(spec, feat)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), want


def device_run(an, key, lr=None):
    """one trainer over the case's epochs: [dict(stats, kernels, biases)] and, for K6_KEYS, (K6's output, the float64 forward)"""
    c, i = tc.CASES[key], tc.inputs(key)
    lr = c["lr"] if lr is None else lr
    if c["regression"]:
        tr = an.regress_trainer(spec_of(key), i["feat"], i["values"], c["n_val"], c["batch"], lr)
    else:
        tr = an.trainer(spec_of(key), i["feat"], i["labels"], c["n_val"], c["batch"], lr)
    out = []
    for o in i["orders"]:
        tr.epoch(o)
        st = tr.stats()
        k, b = tr.weights()
        out.append(dict(st, kernels=k, biases=b))
    k6 = None
    if key in K6_KEYS and lr == c["lr"]:
        m = tr.model()
        k6 = _k6(m, tr.spec_now(), i["feat"], c["regression"])
        m.close()
    tr.close()
    return out, k6


@pytest.fixture(scope="module")
def device_runs(an):
    """each case's run, made when first asked for and shared: read-only"""
    done = {}

    def get(key):
        if key not in done:
            done[key] = device_run(an, key)
        return done[key]
    return get


def same_bits(a, b):
    return all(x["kernels"][l].tobytes() == y["kernels"][l].tobytes() and x["biases"][l].tobytes() == y["biases"][l].tobytes()
               for x, y in zip(a, b) for l in range(len(x["kernels"]))) and \
        all(x[k] == y[k] for x, y in zip(a, b) for k in ("loss", "acc", "val_loss", "val_acc", "epochs_done"))


# sha256 of every epoch's kernels, biases, loss, acc, val_loss, val_acc and epochs_done (digest_of), recorded once on an MI355X from the
# library of the commit before train.hip was split by job (9cdca6b's tree, built into a directory of its own and selected with
# WSA_LIB_DIR): a change to the trainer that is not meant to move a bit is held to these
DIGESTS = {
    "one_layer": "224268c9a49e80984c9db56ecc2974e35e0c268a7f72ce3ea4f67bc7f5fbcfd1",
    "width_edges": "a2a06bcbf4814c7876a07014cb76575ae0e4a6d477eac1d7370913990d544a76",
    "eight_layers": "54e18517903f42d98410b16851c9658126ba08ec92dd813888cb89263a70f32c",
    "widest": "170e5aab7ab6b93978364b1696998d85b55b559086feada7337c554ecefe38b2",
    "classes_33": "5c2fb82b2cd05395d2028839562977f4b3e363532e8f9a3c06b4b559f775d769",
    "big_batch": "2add8bf79e3b15a22fbc8e9f1e6f42afdfa5d9070f8fe025e053df6614308245",
    "batch_1": "1621ff5fe7b7fed57b76b5e81b7a0c15aee871a13bf697d535783b6ace798cd4",
    "last_of_1": "605ca11418ef536c5a36101f74a42e012b7dbfe6dc322d014d97f5092d42b116",
    "r_one_layer": "5e16915bf133dd3aa52f2b09c3844d9702848011b9a02477771d01a5a144fae7",
    "r_width_edges": "76e591dcbcb59685cdf3958b3296db16b60da71dc9d88b40ca058131ca9ad853",
    "r_wide": "58568d630f60a40e5054028b20fb5f5e3a57000f034a11a124f445dac2e1f7ae",
    "r_relu_out": "9fb9ab753f8d1d4b38963fe4e56722a01f026b1b94b759ce08a0525114635696",
    "r_big_batch": "c01bb47f823250a41b5cc23ab1726674ad5689b2715926e4648b4c4116354908",
    "r_batch_1": "98532cd8e962dfcf9370c0c76f31c1a0f25e5db4275737bc882154f1915bfb8a",
}


def digest_of(run):
    h = hashlib.sha256()
    for e in run:
        for a in e["kernels"] + e["biases"]:
            h.update(np.ascontiguousarray(a).tobytes())
        h.update(np.array([e["loss"], e["acc"], e["val_loss"], e["val_acc"]], "<f8").tobytes())
        h.update(np.array([e["epochs_done"]], "<u4").tobytes())
    return h.hexdigest()


def check_count(got_fraction, rows, want, ambiguous):
    """the device's count against the restatement's: exactly (the fraction's bits too) where no row of the evaluation is ambiguous,
    else within the number of ambiguous rows"""
    count = round(got_fraction * rows)
    assert got_fraction == count / rows
    if ambiguous == 0:
        assert count == want and got_fraction == want / rows
    else:
        assert abs(count - want) <= ambiguous


@pytest.mark.parametrize("key", list(tc.CASES))
def test_case_matches_the_restatement(key, device_runs):
    c, got, want = tc.CASES[key], device_runs(key)[0], tc.restated(key)
    n_train = c["n"] - c["n_val"]
    d = train_ref.distance(c, got, want)
    print(f"{key}: device vs restatement {d:.3e} (D32 {c['d32']:.3e}, bound {tc.bound(c):.3e})")
    assert len(got) == len(want) == c["epochs"]
    for e, (g, w) in enumerate(zip(got, want)):
        assert g["epochs_done"] == e + 1
        check_count(g["acc"], n_train, w["correct"], w.get("ambiguous", 0))
        if c["n_val"]:
            check_count(g["val_acc"], c["n_val"], w["val_correct"], w.get("val_ambiguous", 0))
        else:
            assert g["val_loss"] == 0.0 and g["val_acc"] == 0.0
    assert d <= tc.bound(c)


@pytest.mark.parametrize("key", list(tc.CASES))
def test_case_keeps_its_bits(key, device_runs):
    """the solo trainer's bits at every edge of tests/train_cases.py, pinned (the grouped runs are held to the solo runs byte for byte
    by tests/test_gpu_train_group.py)"""
    got = digest_of(device_runs(key)[0])
    print(f"{key}: {got}")
    assert got == DIGESTS[key]


@pytest.mark.parametrize("key", RERUN_KEYS)
def test_two_runs_are_bit_identical(key, an, device_runs):
    assert same_bits(device_run(an, key)[0], device_runs(key)[0])


@pytest.mark.parametrize("key", ["width_edges", "r_width_edges"])
def test_zero_learning_rate_writes_no_weight(key, an):
    """lr = 0 through every width edge (16, 17, 15, 1) and every step size of the case: each weight and bias keeps its bits (in the
    regression case through Adam: 0 . step + w)"""
    i = tc.inputs(key)
    got, _ = device_run(an, key, lr=0.0)
    assert len(got) == tc.CASES[key]["epochs"]
    for e in got:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(e["kernels"] + e["biases"], i["kernels"] + i["biases"]))


@pytest.mark.parametrize("key", K6_KEYS)
def test_k6_over_the_trained_weights_at_the_same_limits(key, device_runs):
    """the bounds of test_classify_rows_512_wide_against_the_restatement (1e-5 in a probability) and of tests/test_gpu_regress.py
    (1e-5 of the output range in a value)"""
    c, i = tc.CASES[key], tc.inputs(key)
    got, want = device_runs(key)[1]
    tol = 1e-5 * (i["out_max"] - i["out_min"]) if c["regression"] else 1e-5
    err = float(np.abs(got - want).max())
    print(f"{key}: K6 against the float64 forward {err:.3e} (bound {tol:.3e})")
    assert got.shape == want.shape and err <= tol

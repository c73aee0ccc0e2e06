"""K7 on the GPU (wsa_trainer_*) against the float64 restatement of specification TR-1 (tests/train_ref.py), which
tests/test_train_reference.py pins to tfjs: never against tfjs's numbers directly, never against the library itself."""
import ctypes

import numpy as np
import pytest

from tests import train_ref
from tests.test_train_reference import BOUND          # 4 x D, D = the f32-versus-f64 noise of a correct implementation on these cases
from webspeechanalyzer_amd import capi, nnmodel

pytestmark = pytest.mark.gpu

FX = train_ref.load_fixture()
CASES = {c["key"]: c for c in FX["cases"]}
KEYS = sorted(CASES)


@pytest.fixture(scope="module")
def an():
    a = capi.Analyzer(capi.Config(output_level=13), device=0)
    yield a
    a.close()


def spec_of(case, ks, bs, mn=None, mx=None):
    return nnmodel.ModelSpec(list(case["units"]), list(case["activations"]), ks, bs, np.array(FX["in_min"] if mn is None else mn, np.float64),
                             np.array(FX["in_max"] if mx is None else mx, np.float64), [f"c{i}" for i in range(case["units"][-1])])


def device_run(an, case, orders, lr=None, keep=False):
    feat, _, y, ks, bs = train_ref.case_inputs(FX, case)
    tr = an.trainer(spec_of(case, ks, bs), feat, y, case["n_val"], case["batch"], case["lr"] if lr is None else lr)
    out = []
    for o in orders:
        tr.epoch(o)
        st = tr.stats()
        k, b = tr.weights()
        out.append(dict(st, kernels=k, biases=b))
    if keep:
        return out, tr
    tr.close()
    return out


def same_bits(a, b):
    return all(x["kernels"][l].tobytes() == y["kernels"][l].tobytes() and x["biases"][l].tobytes() == y["biases"][l].tobytes()
               for x, y in zip(a, b) for l in range(len(x["kernels"]))) and \
        all(x[k] == y[k] for x, y in zip(a, b) for k in ("loss", "acc", "val_loss", "val_acc", "epochs_done"))


@pytest.fixture(scope="module")
def device_runs(an):
    return {k: device_run(an, CASES[k], CASES[k]["orders"]) for k in KEYS}


@pytest.fixture(scope="module")
def restated():
    return {k: train_ref.run_case(FX, CASES[k]) for k in KEYS}


@pytest.mark.parametrize("key", KEYS)
def test_fixture_case_matches_the_restatement(key, device_runs, restated):
    """Measured on an MI355X (bound 4 D = 1.82e-6): a 6.0e-8, b 6.0e-8, c 1.5e-8, d 6.0e-8, e 3.0e-8."""
    case, got, want = CASES[key], device_runs[key], restated[key]
    n_train = len(FX["feat"]) - case["n_val"]
    d = train_ref.distance(case, got, want)
    print(f"{key}: device vs restatement {d:.3e} (bound {BOUND:.3e})")
    for e, (g, w) in enumerate(zip(got, want)):
        assert g["epochs_done"] == e + 1
        assert (round(g["acc"] * n_train), round(g["val_acc"] * case["n_val"])) == (w["correct"], w["val_correct"])
        assert g["acc"] == w["correct"] / n_train and g["val_acc"] == w["val_correct"] / case["n_val"]
    assert d <= BOUND


def test_two_runs_are_bit_identical(an, device_runs):
    for key in (KEYS[1], KEYS[2]):
        assert same_bits(device_run(an, CASES[key], CASES[key]["orders"]), device_runs[key])


def test_zero_learning_rate_moves_nothing(an):
    case = CASES[KEYS[1]]
    _, _, _, ks, bs = train_ref.case_inputs(FX, case)
    got = device_run(an, case, case["orders"][:2], lr=0.0)
    for e in got:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(e["kernels"] + e["biases"], ks + bs))


def test_a_permutation_changes_the_result_as_the_restatement_says(an):
    case = CASES[KEYS[0]]
    perm = [case["orders"][0][::-1]]
    got, plain = device_run(an, case, perm), device_run(an, case, [None])
    assert not same_bits(got, plain)
    assert train_ref.distance(case, got, train_ref.run_case(FX, case, orders=perm)) <= BOUND
    assert train_ref.distance(case, plain, train_ref.run_case(FX, case, orders=[None])) <= BOUND
    assert train_ref.distance(case, got, train_ref.run_case(FX, case, orders=[None])) > BOUND


def test_trainer_model_is_the_copied_weights(an):
    import torch
    case = CASES[KEYS[0]]
    got, tr = device_run(an, case, case["orders"][:1], keep=True)
    m1 = tr.model()
    m2 = an.load_model(tr.spec_now())
    tr.close()
    feat = torch.tensor(np.array(FX["feat"]), dtype=torch.float64, device="cuda:0")
    p1 = torch.zeros((feat.shape[0], 4), dtype=torch.float32, device="cuda:0")
    p2 = torch.zeros_like(p1)
    s = torch.cuda.current_stream().cuda_stream
    m1.classify_rows(feat.data_ptr(), feat.shape[0], p1.data_ptr(), s)
    m2.classify_rows(feat.data_ptr(), feat.shape[0], p2.data_ptr(), s)
    torch.cuda.synchronize()
    a, b = p1.cpu().numpy(), p2.cpu().numpy()
    assert a.tobytes() == b.tobytes() and np.allclose(a.sum(axis=1), 1, atol=1e-5)
    m1.close(); m2.close()


def test_refusals(an):
    case = CASES[KEYS[0]]
    feat, _, y, ks, bs = train_ref.case_inputs(FX, case)
    ok = spec_of(case, ks, bs)

    def refused(msg, spec=ok, y=y, n_val=5, batch=16, lr=0.1):
        with pytest.raises(capi.WsaError, match=msg) as e:
            an.trainer(spec, feat, y, n_val, batch, lr)
        assert "libwsa error 1:" in str(e.value)          # WSA_ERR_INVALID

    lin = spec_of(case, ks, bs); lin.activations = ["relu", "linear"]
    refused("softmax output layer", spec=lin)
    bad = y.copy(); bad[7] = 4
    refused("label 4 of row 7 is outside 0 .. 3", y=bad)
    bad[7] = -1
    refused("label -1 of row 7", y=bad)
    refused("leaves no training rows", n_val=50)
    refused("batch_size must be at least 1", batch=0)
    refused("learning rate is not finite", lr=float("nan"))
    refused("learning rate is not finite", lr=float("inf"))
    refused("learning rate is not finite as an f32", lr=1e300)
    mx = np.array(FX["in_max"]); mx[17] = FX["in_min"][17]
    refused("feature 17 has max == min", spec=spec_of(case, ks, bs, mx=mx))
    tr = an.trainer(ok, feat, y, 5, 16, 0.1)
    order = np.arange(45, dtype=np.uint32); order[3] = 45
    with pytest.raises(capi.WsaError, match=r"order\[3\] = 45 is outside 0 .. 44"):
        tr.epoch(order)
    assert tr.stats()["epochs_done"] == 0                 # nothing was enqueued
    tr.close()


def test_separable_clusters_train(an):
    feat, lab, mn, mx = train_ref.separable_clusters()
    ks, bs = train_ref.hash_init([53, 8, 4], 9)
    spec = nnmodel.ModelSpec([53, 8, 4], ["relu", "softmax"], ks, bs, mn, mx, list("NASH"))
    tr = an.trainer(spec, feat, lab, 80, 32, 0.2)
    tr.epoch(None)
    first = tr.stats()["loss"]
    for _ in range(29):
        tr.epoch(None)
    last = tr.stats()
    tr.close()
    print(f"loss {first:.4f} -> {last['loss']:.4f}, acc {last['acc']:.3f}, val_acc {last['val_acc']:.3f}")
    assert last["epochs_done"] == 30 and last["loss"] < 0.5 * first

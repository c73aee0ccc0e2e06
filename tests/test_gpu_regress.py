"""K7's regression kernels and K6's un-normalising epilogue on the GPU (wsa_regress_*) against the float64 restatement of
specification TR-2 (tests/regress_ref.py), which tests/test_regress_reference.py pins to tfjs: never against tfjs's numbers directly,
never against the library itself."""
import numpy as np
import pytest

from tests import regress_ref, train_ref
from tests.test_regress_reference import BOUND        # 4 x D, D = the f32-versus-f64 noise of a correct implementation on these cases
from webspeechanalyzer_amd import capi, nnmodel

pytestmark = pytest.mark.gpu

FX = regress_ref.load_fixture()
CASES = {c["key"]: c for c in FX["cases"]}
KEYS = sorted(CASES)
OUT = (FX["out_min"], FX["out_max"])


@pytest.fixture(scope="module")
def an():
    a = capi.Analyzer(capi.Config(output_level=13), device=0)
    yield a
    a.close()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def spec_of(case, ks, bs, mx=None, out=OUT):
    return nnmodel.ModelSpec(list(case["units"]), list(case["activations"]), ks, bs, np.array(FX["in_min"], np.float64),
                             np.array(FX["in_max"] if mx is None else mx, np.float64), [], out[0], out[1])


def device_run(an, case, orders, lr=None, keep=False):
    feat, _, y, _, ks, bs = regress_ref.case_inputs(FX, case)
    tr = an.regress_trainer(spec_of(case, ks, bs), feat, y, case["n_val"], case["batch"], case["lr"] if lr is None else lr)
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
    return {k: regress_ref.run_case(FX, CASES[k]) for k in KEYS}


@pytest.mark.parametrize("key", KEYS)
def test_fixture_case_matches_the_restatement(key, device_runs, restated):
    """Measured on an MI355X (bound 4 D = 6.44e-6): a 5.96e-8, b 1.07e-6, c 5.96e-8, d 7.5e-9 (DESIGN.md "K7, regression")."""
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
    for key in (KEYS[1], KEYS[3]):
        assert same_bits(device_run(an, CASES[key], CASES[key]["orders"]), device_runs[key])


def test_zero_learning_rate_moves_nothing(an):
    case = CASES[KEYS[1]]
    ks, bs = regress_ref.case_inputs(FX, case)[4:]
    got = device_run(an, case, case["orders"][:2], lr=0.0)
    for e in got:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(e["kernels"] + e["biases"], ks + bs))


def test_the_dead_unit_is_left_bit_for_bit(device_runs):
    """gradients of exactly 0 with m = v = 0: 0 / (0 + epsilon) . (-lr) + w = w, through 4 epochs of 7 steps"""
    case = next(c for c in CASES.values() if "dead_unit" in c["init"])
    u = case["init"]["dead_unit"]
    ks, bs = regress_ref.case_inputs(FX, case)[4:]
    last = device_runs[case["key"]][-1]
    assert last["kernels"][0][:, u].tobytes() == ks[0][:, u].tobytes() and last["biases"][0][u].tobytes() == bs[0][u].tobytes()
    assert not np.array_equal(last["kernels"][0], ks[0]) and not np.array_equal(last["kernels"][1], ks[1])


def test_a_reversed_order_changes_the_result_as_the_restatement_says(an):
    case = CASES[KEYS[0]]
    perm = [case["orders"][0][::-1]]
    got, plain = device_run(an, case, perm), device_run(an, case, [None])
    assert not same_bits(got, plain)
    assert train_ref.distance(case, got, regress_ref.run_case(FX, case, orders=perm)) <= BOUND
    assert train_ref.distance(case, plain, regress_ref.run_case(FX, case, orders=[None])) <= BOUND
    assert train_ref.distance(case, got, regress_ref.run_case(FX, case, orders=[None])) > BOUND


def test_moments_and_accumulated_betas_are_carried_across_epochs(an):
    """eight epochs in one trainer against a fresh trainer started from the first one's weights after four: the fresh one has m = v = 0
    and accBeta = beta again, so its four epochs must differ from the first trainer's epochs 5 .. 8"""
    case = CASES[KEYS[0]]
    orders = case["orders"] + case["orders"]
    one = device_run(an, case, orders)
    feat, _, y, _, _, _ = regress_ref.case_inputs(FX, case)
    tr = an.regress_trainer(spec_of(case, one[3]["kernels"], one[3]["biases"]), feat, y, case["n_val"], case["batch"], case["lr"])
    fresh = []
    for o in orders[4:]:
        tr.epoch(o)
        k, b = tr.weights()
        fresh.append(dict(tr.stats(), kernels=k, biases=b))
    tr.close()
    assert same_bits(one[:4], device_run(an, case, orders[:4]))
    d = train_ref.distance(case, fresh, one[4:])
    print(f"carried against reset after four epochs: {d:.3e}")
    assert d > 100 * BOUND
    # and the carried run is the restatement's eight epochs
    assert train_ref.distance(case, one, regress_ref.run_case(FX, case, orders=orders)) <= BOUND


def _values(torch, model, feat, out=None):
    d_feat = torch.tensor(np.ascontiguousarray(feat), dtype=torch.float64, device="cuda:0")
    d_val = torch.full((len(feat),), -7.0, dtype=torch.float64, device="cuda:0")
    lo, hi = out if out is not None else (None, None)
    model.regress_rows(d_feat.data_ptr(), len(feat), d_val.data_ptr(), lo, hi, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_val.cpu().numpy()


def test_trainer_model_is_the_copied_weights_and_predicts_the_float64_forward(an, torch):
    case = CASES[KEYS[1]]
    _, tr = device_run(an, case, case["orders"][:2], keep=True)
    now = tr.spec_now()
    m1, m2 = tr.model(), an.load_model(now)
    tr.close()
    lo, hi = np.array(FX["in_min"]), np.array(FX["in_max"])
    rng = np.random.default_rng(3)
    outside = lo + (hi - lo) * rng.uniform(-0.1, 1.1, (37, 53))                  # up to 10 % outside the input ranges
    outside[:4] = [lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), lo, hi]
    feat = np.concatenate([np.array(FX["feat"]), outside])
    a, b = _values(torch, m1, feat), _values(torch, m2, feat)
    assert a.tobytes() == b.tobytes()
    p, want = regress_ref.predict(feat, now.kernels, now.biases, now.activations, lo, hi, *OUT)
    err = float(np.abs(a - want).max())
    print(f"values against the float64 forward: {err:.3e} (bound {1e-5 * (OUT[1] - OUT[0]):.3e})")
    assert err <= 1e-5 * (OUT[1] - OUT[0])
    # the un-normalise rule itself, exactly: some f32 p gives every value by a separately rounded product and sum
    span = OUT[1] - OUT[0]
    p32 = ((a - OUT[0]) / span).astype(np.float32)
    cand = np.stack([np.nextafter(p32, np.float32(-1)), p32, np.nextafter(p32, np.float32(2))]).astype(np.float64) * span + OUT[0]
    assert (cand == a[None, :]).any(axis=0).all()
    # another range through the arguments
    c = _values(torch, m1, feat[:5], out=(-3.0, 5.0))
    assert np.abs(c - (p[:5] * 8.0 - 3.0)).max() <= 1e-5 * 8.0
    m1.close(); m2.close()


def test_batch_regress_levels_5_and_13(torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    case = CASES[KEYS[0]]
    ks, bs = regress_ref.case_inputs(FX, case)[4:]
    pcm = synth_clips(2, 32000, fs=16000, seed=2, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for level in (5, 13):
        an = wsa.Analyzer(wsa.Config(output_level=level))
        m = an.load_model(spec_of(case, ks, bs))
        b = an.batch([pcm.shape[1]] * 2, 16000)
        b.run(pcm.data_ptr(), pcm.stride(0), s)
        b.regress(m, stream=s)
        got = b.values(s)
        rows = b.rows(s)
        assert len(got) == len(rows["meta"]) > 0
        assert got.tobytes() == _values(torch, m, rows["feat"]).tobytes()
        n = capi.ctypes.c_uint32()
        small = np.zeros(len(got) - 1)
        with pytest.raises(wsa.WsaError, match="value buffer too small"):
            an._check(b.L.wsa_batch_copy_values(b.h, s, small.ctypes.data, len(small), capi.ctypes.byref(n)))
        assert n.value == len(got)
        with pytest.raises(wsa.WsaError, match="wsa_batch_regress"):
            b.classes(s)
        b.close(); m.close(); an.close()


def test_refusals(an, torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    case = CASES[KEYS[0]]
    feat, _, y, _, ks, bs = regress_ref.case_inputs(FX, case)
    ok = spec_of(case, ks, bs)

    def refused(msg, spec=ok, y=y, n_val=5, batch=16, lr=0.1, out=(None, None)):
        with pytest.raises(capi.WsaError, match=msg) as e:
            an.regress_trainer(spec, feat, y, n_val, batch, lr, *out)
        assert "libwsa error 1:" in str(e.value)          # WSA_ERR_INVALID

    two = train_ref.hash_init([53, 16, 2], 1)
    refused("one output unit, got 2", spec=nnmodel.ModelSpec([53, 16, 2], ["sigmoid", "sigmoid"], two[0], two[1], ok.in_min, ok.in_max, [], *OUT))
    sm = spec_of(case, ks, bs); sm.activations = ["sigmoid", "softmax"]
    refused("not softmax", spec=sm)
    bad = y.copy(); bad[7] = np.nan
    refused("target of row 7 is not finite", y=bad)
    bad[7] = np.inf
    refused("target of row 7 is not finite", y=bad)
    bad[7] = 1e300
    refused("target of row 7 is not finite as a normalised f32", y=bad)
    refused("output has max == min", out=(0.4, 0.4))
    refused("non-finite out_min / out_max", out=(0.0, float("inf")))
    refused("leaves no training rows", n_val=50)
    refused("batch_size must be at least 1", batch=0)
    refused("learning rate is not finite as an f32", lr=1e300)
    mx = np.array(FX["in_max"]); mx[17] = FX["in_min"][17]
    refused("feature 17 has max == min", spec=spec_of(case, ks, bs, mx=mx))
    # a classification trainer still refuses a stack without softmax, and a regression model still cannot be folded
    with pytest.raises(capi.WsaError, match="training needs a softmax output layer"):
        an.trainer(ok, feat, np.zeros(len(feat), np.int32), 5, 16, 0.1)
    other = capi.Analyzer(capi.Config(output_level=13), device=0)
    m, m_other = an.load_model(ok), other.load_model(ok)
    cls = train_ref.hash_init([53, 8, 4], 1)
    m_cls = an.load_model(nnmodel.ModelSpec([53, 8, 4], ["relu", "softmax"], cls[0], cls[1], ok.in_min, ok.in_max, list("NASH")))
    m_two = an.load_model(nnmodel.ModelSpec([53, 16, 2], ["sigmoid", "sigmoid"], two[0], two[1], ok.in_min, ok.in_max, [], *OUT))
    pcm = synth_clips(2, 32000, fs=16000, seed=2, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    b = an.batch([pcm.shape[1]] * 2, 16000)
    b.run(pcm.data_ptr(), pcm.stride(0), s)
    with pytest.raises(capi.WsaError, match="the model's last layer is not softmax"):
        b.classify(m, s)
    with pytest.raises(capi.WsaError, match="another context"):
        b.regress(m_other, stream=s)
    with pytest.raises(capi.WsaError, match="not softmax"):
        b.regress(m_cls, 0.0, 1.0, s)
    with pytest.raises(capi.WsaError, match="one output unit"):
        b.regress(m_two, stream=s)
    with pytest.raises(capi.WsaError, match="max == min"):
        b.regress(m, 1.0, 1.0, s)
    with pytest.raises(capi.WsaError, match="not wsa_batch_regress"):
        b.values(s)
    d = torch.zeros(53, dtype=torch.float64, device="cuda:0")
    for mm, lo, hi, msg in ((m_cls, 0.0, 1.0, "not softmax"), (m_two, 0.0, 1.0, "one output unit"), (m, 2.0, 2.0, "max == min"), (m, float("nan"), 1.0, "non-finite")):
        with pytest.raises(capi.WsaError, match=msg):
            mm.regress_rows(d.data_ptr(), 1, d.data_ptr(), lo, hi, s)
    b.close()
    low = wsa.Analyzer(wsa.Config(output_level=4))
    b4 = low.batch([pcm.shape[1]] * 2, 16000)
    b4.run(pcm.data_ptr(), pcm.stride(0), s)
    m4 = low.load_model(ok)
    with pytest.raises(capi.WsaError, match="output_level 5"):
        b4.regress(m4, stream=s)
    b4.close(); m4.close(); low.close()
    for x in (m, m_other, m_cls, m_two):
        x.close()
    other.close()


def test_a_smooth_target_trains(an):
    """the app's default stack (nn_default_options_ords) over 800 rows, 30 epochs; learning rate 0.02 (at the app's 0.2 Adam saturates
    the sigmoids in the first epoch on these rows, in the restatement too: tests/test_regress_reference.py)"""
    from webspeechanalyzer_amd import train
    feat, y, mn, mx = regress_ref.smooth_target()
    ks, bs = train_ref.hash_init([53, 64, 16, 1], 9)
    data = dict(features=feat, values=y, in_min=mn, in_max=mx, out_min=float(y.min()), out_max=float(y.max()))
    hist = []
    spec, _ = train.train_regression(an, data, learning_rate=0.02, epochs=30, batch_size=32, init=(ks, bs), orders=[None] * 30,
                                     on_epoch=lambda e, st: hist.append(st))
    print(f"loss {hist[0]['loss']:.4f} -> {hist[-1]['loss']:.4f}, val_loss {hist[-1]['val_loss']:.4f}")
    assert hist[-1]["epochs_done"] == 30 and hist[-1]["loss"] < 0.5 * hist[0]["loss"]
    assert spec.is_regression and spec.units == [53, 64, 16, 1] and (spec.out_min, spec.out_max) == (float(y.min()), float(y.max()))

"""K6, K7 and K8 on the GPU at the row widths of output levels 11 (264 features) and 12 (23): tests/wide_cases.py's models and cases
against the float64 restatements that tests/test_wide_reference.py pins to tfjs; wsa_batch_classify / _regress on the utterance table
(level 11) and on the strided row table (level 12); and the bits of two 53-wide runs against digests recorded on the commit before
the widths were added.

Bounds: a probability within 1e-5 of classify_ref.forward (tests/test_gpu_classify.py's), a value within 1e-5 of the output range
(tests/test_gpu_regress.py's), a training run within wide_cases.bound(case) = max(the family's fixture bound, 4 x D32).

Measured on an MI355X, device against restatement (DESIGN.md "At the kernels' edges" holds the same table):
  K6  f264 1.26e-07, f23 1.08e-07 in a probability; r_w264 2.24e-08, r_w23 8.33e-08 in a value (bound 5.39e-06); level 11's utterance
      rows 7.49e-08
  K7  w264_one_layer  2.98e-08  (D32 1.49e-08)        r_w264  8.08e-07  (D32 7.30e-07)
      w264_stack      5.96e-08  (D32 2.98e-08)        r_w23   5.96e-08  (D32 5.96e-08)
      w23_stack       2.98e-08  (D32 2.98e-08)
Counts equal the restatement's in every epoch of every case."""
import hashlib
import os

import numpy as np
import pytest

from tests import classify_ref, dbstats_ref, regress_ref, train_ref
from tests import train_cases as tc
from tests import wide_cases as wc
from tests.test_gpu_train_shapes import check_count, same_bits
from webspeechanalyzer_amd import capi, nnmodel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PROB_TOL, VALUE_TOL = 1e-5, 1e-5          # tests/test_gpu_classify.py (absolute), tests/test_gpu_regress.py (of the output range)

# sha256 of the bits two 53-wide runs gave on the commit BEFORE this one (recorded there once, on an MI355X): K6 over
# train_cases.inputs("one_layer")'s 60 rows with tests/golden/nn/1/cats_emotion, and K7's weights and statistics after each epoch of
# train_cases "one_layer"
DIGEST_53 = dict(classify="2b02981df66336cc5c3a235168fa1ea7faec7b3a98150b81749409f4db289b31",
                 train="5018a047431f52a15fc33ec3b9eb54c194036b8747ea9d5f238552a1583d322d")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def an():
    a = capi.Analyzer(capi.Config(output_level=13), device=0)
    yield a
    a.close()


def _s(torch):
    return torch.cuda.current_stream().cuda_stream


def tile_rows(units):
    """the rows of one K6 tile, 16 rb, by the library's rule (csrc/classify.hip wsa_model_create): S = the widest padded layer rounded up
    to 64, + 4; rb = 4 halved while two buffers of 16 rb x S floats exceed 160 KiB"""
    S = ((max((u + 15) & ~15 for u in units) + 63) & ~63) + 4
    rb = 4
    while rb > 1 and 2 * 16 * rb * S * 4 > 160 * 1024:
        rb >>= 1
    return 16 * rb


def forward_spec(name):
    f = wc.forward_inputs(name)
    return nnmodel.ModelSpec(list(f["units"]), list(f["activations"]), [k.copy() for k in f["kernels"]], [b.copy() for b in f["biases"]],
                             f["in_min"].copy(), f["in_max"].copy(), list(f["labels"]))


def regress_spec(key, feat, values):
    """the initial weights of a regression case as a model, with the ranges of `feat` / `values`"""
    c = wc.CASES[key]
    ks, bs = train_ref.hash_init(c["units"], c["salt"])
    in_min, in_max = wc._ranges(feat)
    return nnmodel.ModelSpec(list(c["units"]), list(c["activations"]), ks, bs, in_min, in_max, [], float(values.min()), float(values.max()))


def classify_rows(torch, model, feat):
    d_feat = torch.from_numpy(np.ascontiguousarray(feat, np.float64)).cuda()
    d_prob = torch.full((len(feat), model.n_classes), -1.0, dtype=torch.float32, device="cuda")
    model.classify_rows(d_feat.data_ptr(), len(feat), d_prob.data_ptr(), _s(torch))
    torch.cuda.synchronize()
    return d_prob.cpu().numpy()


def regress_rows(torch, model, feat):
    d_feat = torch.from_numpy(np.ascontiguousarray(feat, np.float64)).cuda()
    d_val = torch.full((len(feat),), -7.0, dtype=torch.float64, device="cuda")
    model.regress_rows(d_feat.data_ptr(), len(feat), d_val.data_ptr(), None, None, _s(torch))
    torch.cuda.synchronize()
    return d_val.cpu().numpy()


def test_level_feature_count():
    assert [capi.level_feature_count(l) for l in range(0, 15)] == [0, 0, 0, 0, 0, 53, 0, 0, 0, 0, 0, 264, 23, 53, 0]
    assert capi.level_feature_count(-1) == 0 and capi.lib().wsa_abi_version() == 5


# ---- K6 on dense rows
@pytest.mark.parametrize("name,tile", [("f264", 32), ("f23", 64)])
def test_k6_on_rows(torch, an, name, tile):
    spec = forward_spec(name)
    width, C = spec.units[0], spec.units[-1]
    assert tile_rows(spec.units) == tile                     # 264 pads to 272: S = 324, rb = 2 -- the input layer sets it; 23-8-3: S = 68, rb = 4
    feat, _ = wc.cluster_rows(70, width, C, wc.FORWARD[name]["salt"])
    want = classify_ref.forward(spec, feat)
    m = an.load_model(spec)
    assert m.n_inputs == width
    full = classify_rows(torch, m, feat)
    err = float(np.abs(full - want).max())
    print(f"{name}: K6 against the float64 forward {err:.3e} (bound {PROB_TOL:.0e})")
    assert full.shape == want.shape and err <= PROB_TOL
    assert np.ptp(want, axis=0).min() > 0.05                 # the rows differ: an all-zero input tile would not pass
    assert full.tobytes() == classify_rows(torch, m, feat).tobytes()
    for n in (1, tile - 1, tile, tile + 1):                  # a row's bits do not depend on the rows beside it or on its tile
        assert classify_rows(torch, m, feat[:n]).tobytes() == full[:n].tobytes(), n
    assert classify_rows(torch, m, feat[tile - 1:]).tobytes() == full[tile - 1:].tobytes()
    m.close()


@pytest.mark.parametrize("key,tile", [("r_w264", 32), ("r_w23", 64)])
def test_k6_regress_on_rows(torch, an, key, tile):
    width = wc.CASES[key]["units"][0]
    feat, values = wc.smooth_rows(70, width, 17)
    spec = regress_spec(key, feat, values)
    assert tile_rows(spec.units) == tile
    want = regress_ref.predict(feat, spec.kernels, spec.biases, spec.activations, spec.in_min, spec.in_max, spec.out_min, spec.out_max)[1]
    m = an.load_model(spec)
    full = regress_rows(torch, m, feat)
    tol = VALUE_TOL * (spec.out_max - spec.out_min)
    err = float(np.abs(full - want).max())
    print(f"{key}: K6's values against the float64 forward {err:.3e} (bound {tol:.3e})")
    assert err <= tol and np.ptp(want) > 1e-3 * (spec.out_max - spec.out_min)
    assert full.tobytes() == regress_rows(torch, m, feat).tobytes()
    for n in (1, tile - 1, tile, tile + 1):
        assert regress_rows(torch, m, feat[:n]).tobytes() == full[:n].tobytes(), n
    m.close()


def test_width_refusals(an):
    s = forward_spec("f23")
    for width in (63, 9):
        ks, bs = train_ref.hash_init([width, 8, 3], 1)
        bad = nnmodel.ModelSpec([width, 8, 3], s.activations, ks, bs, np.zeros(width), np.ones(width), s.labels)
        with pytest.raises(capi.WsaError, match=f"{width} inputs; the feature rows have 53"):
            an.load_model(bad)
        with pytest.raises(capi.WsaError, match=f"{width} inputs; the feature rows have 53"):
            an.trainer(bad, np.zeros((20, width)), np.zeros(20, np.int32), 2, 4, 0.1)
    # the range check reaches the last input of the widest row: in_max == in_min at input 263 (what wsa_trainer_create refuses at 53 too)
    c, i = wc.CASES["w264_one_layer"], wc.inputs("w264_one_layer")
    mx = i["in_max"].copy()
    mx[263] = i["in_min"][263]
    flat = nnmodel.ModelSpec(list(c["units"]), list(c["activations"]), i["kernels"], i["biases"], i["in_min"], mx, ["a", "b", "c", "d"])
    with pytest.raises(capi.WsaError, match="feature 263 has max == min"):
        an.trainer(flat, i["feat"], i["labels"], c["n_val"], c["batch"], c["lr"])
    nan = i["in_min"].copy()
    nan[263] = np.nan
    with pytest.raises(capi.WsaError, match="non-finite in_min / in_max of input 263"):
        an.load_model(nnmodel.ModelSpec(list(c["units"]), list(c["activations"]), i["kernels"], i["biases"], nan, i["in_max"], ["a", "b", "c", "d"]))
    with pytest.raises(ValueError, match=r"expected \[n\]\[264\]"):
        an.trainer(flat, np.zeros((20, 53)), np.zeros(20, np.int32), 2, 4, 0.1)


# ---- batches at levels 12 and 11
def _wrap(torch, ptr, shape, typestr):
    """a device table of the library as a torch tensor (no copy): shape and type are the caller's word"""
    class _Dev:
        __cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2, strides=None)
    return torch.as_tensor(_Dev(), device="cuda")


def _check_level_12(torch, an12, b, expect_marked):
    rows = b.rows(_s(torch))
    feat, n = rows["feat"], len(rows["feat"])
    assert n > 0
    marked = feat[:, 23] != 0
    assert bool(marked.any()) == expect_marked and (~marked).any()
    # the models' ranges are those of the rows at hand, widened (no input divides by zero, no logit far outside the trained range)
    lo, hi = feat[~marked][:, :23].min(axis=0) - 0.5, feat[~marked][:, :23].max(axis=0) + 0.5
    f = wc.forward_inputs("f23")
    spec = nnmodel.ModelSpec(list(f["units"]), list(f["activations"]), f["kernels"], f["biases"], lo, hi, list(f["labels"]))
    m = an12.load_model(spec)
    b.classify(m, _s(torch))
    got = b.classes(_s(torch))
    assert got["prob"].shape == (n, 3) and len(got["cb"]) == 0 and got["clip_conf"].shape[0] == 0      # per-row outputs only, as at level 5
    dense = classify_rows(torch, m, np.ascontiguousarray(feat[:, :23]))
    assert got["prob"][~marked].tobytes() == dense[~marked].tobytes()
    assert np.isnan(got["prob"][marked]).all() and np.isfinite(got["prob"][~marked]).all()
    want = classify_ref.forward(spec, feat[~marked][:, :23])
    assert np.abs(got["prob"][~marked] - want).max() <= PROB_TOL
    # nothing past column 22 is read but the mark in slot 23: NaN in slots 24 .. 52 of the batch's own table changes no bit
    r = b.device_result(_s(torch))
    table = _wrap(torch, r.d_row_feat, (n, 53), "<f8")
    assert table.cpu().numpy().tobytes() == feat.tobytes()
    table[:, 24:] = float("nan")
    torch.cuda.synchronize()
    b.classify(m, _s(torch))
    again = b.classes(_s(torch))["prob"]
    assert again.tobytes() == got["prob"].tobytes()
    # the values of a regression model, likewise
    c, rk = wc.CASES["r_w23"], train_ref.hash_init(wc.CASES["r_w23"]["units"], 11)
    rm = an12.load_model(nnmodel.ModelSpec(list(c["units"]), list(c["activations"]), rk[0], rk[1], lo, hi, [], 0.0, 1.0))
    b.regress(rm, None, None, _s(torch))
    vals = b.values(_s(torch))
    assert vals.shape == (n,) and np.isnan(vals[marked]).all()
    assert vals[~marked].tobytes() == regress_rows(torch, rm, np.ascontiguousarray(feat[:, :23]))[~marked].tobytes()
    rm.close(); m.close()
    return n, int(marked.sum())


def test_level_12_batch_reads_the_strided_rows(torch):
    from webspeechanalyzer_amd.synth import synth_clips
    fs, ns = 16000, 32000
    pcm = synth_clips(3, ns, fs=fs, seed=3, device="cuda")
    an12 = capi.Analyzer(capi.Config(output_level=12), device=0)
    b = an12.batch([ns] * 3, fs)
    b.run(pcm.data_ptr(), pcm.stride(0), _s(torch))
    n, marked = _check_level_12(torch, an12, b, expect_marked=False)
    print(f"level 12, three 2 s clips: {n} rows")
    m53 = an12.load_model(os.path.join(GOLD, "nn", "1/cats_emotion"))
    with pytest.raises(capi.WsaError, match=r"output_level 5 .*not 12.*53 inputs"):
        b.classify(m53, _s(torch))
    m53.close(); b.close(); an12.close()


def test_level_12_row_whose_fit_threw_is_nan(torch):
    """the captured spectrum of the level-12 throw fixture (tests/golden/gen/make_golden.py: 96 bands, 15 ms hop) through the back end"""
    cap = np.load(os.path.join(GOLD, "gen", "captured_l12_throw.npy"))
    cfg = capi.Config(output_level=12, N_mel_bins=int(cap.shape[1]), window_step=15.0, window_width=15.0, pause_length=100.0, min_seg_length=100.0,
                      auto_noise_gate=0, voiced_max_dB=140.0, voiced_min_dB=10.0)
    an12 = capi.Analyzer(cfg, device=0)
    g = an12.geometry(16000)
    b = an12.batch([g["win"] + (len(cap) - 1) * g["hop"]], 16000)
    d = torch.from_numpy(np.ascontiguousarray(cap).view(np.int32)).cuda()
    b.run_backend(d.data_ptr(), _s(torch))
    n, marked = _check_level_12(torch, an12, b, expect_marked=True)
    print(f"level 12, the throw clip: {n} rows, {marked} marked")
    b.close(); an12.close()


def test_level_11_batch_classifies_the_utterance_rows(torch, an):
    from webspeechanalyzer_amd.synth import synth_clips
    fs, ns = 16000, 32000
    pcm = synth_clips(3, ns, fs=fs, seed=3, device="cuda")
    an11 = capi.Analyzer(capi.Config(output_level=11), device=0)
    b = an11.batch([ns] * 3, fs)
    b.run(pcm.data_ptr(), pcm.stride(0), _s(torch))
    utt = b.utterance(_s(torch))
    r = b.device_result(_s(torch))
    n = int(r.n_utterance_rows)
    assert n == len(utt["feat"]) > 0 and int(utt["off"][-1]) == n
    # a model whose ranges are those of the rows at hand (constant columns widened, so no input divides by zero)
    f = wc.forward_inputs("f264")
    lo, hi = utt["feat"].min(axis=0), utt["feat"].max(axis=0)
    spec = nnmodel.ModelSpec(list(f["units"]), list(f["activations"]), f["kernels"], f["biases"], lo - 0.5, hi + 0.5, list(f["labels"]))
    m = an11.load_model(spec)
    b.classify(m, _s(torch))
    cr = b.class_result(_s(torch))
    assert (int(cr.n_rows), int(cr.n_classes), int(cr.n_callbacks)) == (n, 4, 0) and not cr.d_cb and not cr.d_clip_conf
    got = b.classes(_s(torch))["prob"]
    d_prob = torch.full((n, 4), -1.0, dtype=torch.float32, device="cuda")
    m.classify_rows(r.d_utt_feat, n, d_prob.data_ptr(), _s(torch))
    torch.cuda.synchronize()
    assert got.tobytes() == d_prob.cpu().numpy().tobytes()
    want = classify_ref.forward(spec, utt["feat"])
    err = float(np.abs(got - want).max())
    print(f"level 11: {n} utterance rows, K6 against the float64 forward {err:.3e}")
    assert err <= PROB_TOL
    # a clip's stored row is its last one (the app stores under part 0): reachable through the offsets
    last = [int(utt["off"][c + 1]) - 1 for c in range(3) if utt["off"][c + 1] > utt["off"][c]]
    assert last and all(0 <= k < n for k in last)
    c, rk = wc.CASES["r_w264"], train_ref.hash_init(wc.CASES["r_w264"]["units"], 11)
    rspec = nnmodel.ModelSpec(list(c["units"]), list(c["activations"]), rk[0], rk[1], lo - 0.5, hi + 0.5, [], 0.25, 2.0)
    rm = an11.load_model(rspec)
    b.regress(rm, None, None, _s(torch))
    vals = b.values(_s(torch))
    d_val = torch.zeros(n, dtype=torch.float64, device="cuda")
    rm.regress_rows(r.d_utt_feat, n, d_val.data_ptr(), None, None, _s(torch))
    torch.cuda.synchronize()
    assert vals.shape == (n,) and vals.tobytes() == d_val.cpu().numpy().tobytes()
    wantv = regress_ref.predict(utt["feat"], rspec.kernels, rspec.biases, rspec.activations, rspec.in_min, rspec.in_max, 0.25, 2.0)[1]
    assert np.abs(vals - wantv).max() <= VALUE_TOL * 1.75
    # refusals: every other pairing of level and width, naming both; ensembles and streams take 53-input models only
    m53 = an11.load_model(os.path.join(GOLD, "nn", "1/cats_emotion"))
    with pytest.raises(capi.WsaError, match=r"output_level 5 .*not 11.*53 inputs"):
        b.classify(m53, _s(torch))
    m23 = an11.load_model(forward_spec("f23"))
    with pytest.raises(capi.WsaError, match=r"output_level 12 .*not 11.*23 inputs"):
        b.classify(m23, _s(torch))
    with pytest.raises(capi.WsaError, match=r"output_level 12 .*not 11.*23 inputs"):
        b.regress(m23, 0.0, 1.0, _s(torch))
    m23.close(); m53.close(); rm.close(); m.close(); b.close(); an11.close()
    # a 264-input model at level 13, in streams and in an ensemble (the module's level-13 context)
    m = an.load_model(forward_spec("f264"))
    b = an.batch([ns] * 3, fs)
    b.run(pcm.data_ptr(), pcm.stride(0), _s(torch))
    with pytest.raises(capi.WsaError, match=r"output_level 11 .*not 13.*264 inputs"):
        b.classify(m, _s(torch))
    with pytest.raises(capi.WsaError, match="264 inputs"):
        an.ensemble([m])
    st = an.streams(2, fs, frames_per_step=4)
    with pytest.raises(capi.WsaError, match="264 inputs"):
        st.set_model(m)
    st.close(); b.close(); m.close()


# ---- K7
def spec_of(key):
    c, i = wc.CASES[key], wc.inputs(key)
    ks, bs = [k.copy() for k in i["kernels"]], [b.copy() for b in i["biases"]]
    if c["regression"]:
        return nnmodel.ModelSpec(list(c["units"]), list(c["activations"]), ks, bs, i["in_min"].copy(), i["in_max"].copy(), [], i["out_min"], i["out_max"])
    return nnmodel.ModelSpec(list(c["units"]), list(c["activations"]), ks, bs, i["in_min"].copy(), i["in_max"].copy(), [f"c{j}" for j in range(c["units"][-1])])


def device_run(torch, an, key):
    """one trainer over the case's epochs: ([dict(stats, kernels, biases)], K6 over the rows with trainer.model(), the same with a model
    loaded from the copied weights)"""
    c, i = wc.CASES[key], wc.inputs(key)
    if c["regression"]:
        tr = an.regress_trainer(spec_of(key), i["feat"], i["values"], c["n_val"], c["batch"], c["lr"])
    else:
        tr = an.trainer(spec_of(key), i["feat"], i["labels"], c["n_val"], c["batch"], c["lr"])
    out = []
    for o in i["orders"]:
        tr.epoch(o)
        st = tr.stats()
        k, b = tr.weights()
        out.append(dict(st, kernels=k, biases=b))
    run = regress_rows if c["regression"] else classify_rows
    snap, copied = tr.model(), an.load_model(tr.spec_now())
    k6 = (run(torch, snap, i["feat"]), run(torch, copied, i["feat"]), tr.spec_now())
    snap.close(); copied.close(); tr.close()
    return out, k6


@pytest.mark.parametrize("key", list(wc.CASES))
def test_k7_case_matches_the_restatement(torch, an, key):
    c, i, want = wc.CASES[key], wc.inputs(key), wc.restated(key)
    got, (by_snapshot, by_copy, spec) = device_run(torch, an, key)
    n_train = c["n"] - c["n_val"]
    d = train_ref.distance(c, got, want)
    print(f"{key}: device vs restatement {d:.3e} (D32 {c['d32']:.3e}, bound {wc.bound(c):.3e})")
    assert len(got) == len(want) == c["epochs"]
    for e, (g, w) in enumerate(zip(got, want)):
        assert g["epochs_done"] == e + 1
        check_count(g["acc"], n_train, w["correct"], w.get("ambiguous", 0))
        if c["n_val"]:
            check_count(g["val_acc"], c["n_val"], w["val_correct"], w.get("val_ambiguous", 0))
        else:
            assert g["val_loss"] == 0.0 and g["val_acc"] == 0.0
    assert d <= wc.bound(c)
    assert same_bits(device_run(torch, an, key)[0], got)                      # two runs, equal in every bit
    assert by_snapshot.tobytes() == by_copy.tobytes()                         # trainer.model() classifies as its copied weights do
    if c["regression"]:
        ref = regress_ref.predict(i["feat"], spec.kernels, spec.biases, spec.activations, spec.in_min, spec.in_max, spec.out_min, spec.out_max)[1]
        assert np.abs(by_snapshot - ref).max() <= VALUE_TOL * (spec.out_max - spec.out_min)
    else:
        assert np.abs(by_snapshot - classify_ref.forward(spec, i["feat"])).max() <= PROB_TOL


# ---- K8
def test_k8_on_a_264_wide_db(torch, an):
    n, C = 300, 4                                            # two DS-1 chunks of 256 rows, the second partial
    spec = forward_spec("f264")
    feat, lab = wc.cluster_rows(n, 264, C, wc.FORWARD["f264"]["salt"])
    h = wc.mix(np.arange(n), 3, 21)
    dur = 0.05 + (h % 400).astype(np.float64) / 1000.0
    true_idx = np.where(h % 11 == 0, -1, lab).astype(np.int32)
    true_val = np.where(h % 7 == 0, np.nan, 0.1 + (h % 90) / 100.0)
    _, rvals = wc.smooth_rows(n, 264, 17)
    rspec = regress_spec("r_w264", feat, rvals)
    m, rm = an.load_model(spec), an.load_model(rspec)
    db = an.feature_db(feat, dur, [C], 1)
    assert db.n_feat == 264
    db.set_classes(0, true_idx)
    db.set_values(0, true_val)
    s = _s(torch)
    db.predict_classes(0, m, np.arange(C), s)
    db.predict_values(0, rm, None, None, s)
    pred_idx, pred_val, prob = db.pred_classes(0, s), db.pred_values(0, s), db.probs(C, s)
    got, again = db.table(s), db.table(s)
    assert prob.tobytes() == classify_rows(torch, m, feat).tobytes() and pred_val.tobytes() == regress_rows(torch, rm, feat).tobytes()
    assert np.abs(prob - classify_ref.forward(spec, feat)).max() <= PROB_TOL
    assert pred_idx.tolist() == dbstats_ref.decide(prob, np.arange(C)).tolist() and len(set(pred_idx.tolist())) > 1
    want = dbstats_ref.table(dur, [(C, true_idx, pred_idx)], [(true_val, pred_val)])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), "two runs differ"
    for name, g, w in zip(("cat", "cls", "ord"), got, want):
        for f in w.dtype.names:
            assert g[f].tobytes() == w[f].tobytes(), f"{name}.{f}: {g[f][:8]} != {w[f][:8]}"
    assert int(got[0]["correct"][0]) > 0 and int(got[0]["wrong"][0]) > 0 and int(got[2]["pred_n"][0]) > 0
    # a model of another width than the DB's is refused by the device object too
    m53 = an.load_model(os.path.join(GOLD, "nn", "1/cats_emotion"))
    with pytest.raises(capi.WsaError, match="the model takes 53 inputs; the DB's rows have 264 features"):
        db.predict_classes(0, m53, np.arange(m53.n_classes) % C, s)
    db53 = an.feature_db(np.zeros((4, 53)), np.ones(4), [C], 1)
    with pytest.raises(capi.WsaError, match="the model takes 264 inputs; the DB's rows have 53 features"):
        db53.predict_values(0, rm, None, None, s)
    db53.close(); m53.close(); db.close(); m.close(); rm.close()


# ---- the 53-wide paths keep their bits
def digests_53(torch, an):
    """(K6, K7) digests of two 53-wide runs: what DIGEST_53 records"""
    i, c = tc.inputs("one_layer"), tc.CASES["one_layer"]
    m = an.load_model(os.path.join(GOLD, "nn", "1/cats_emotion"))
    k6 = hashlib.sha256(classify_rows(torch, m, i["feat"]).tobytes()).hexdigest()
    m.close()
    spec = nnmodel.ModelSpec(list(c["units"]), list(c["activations"]), [k.copy() for k in i["kernels"]], [b.copy() for b in i["biases"]],
                             i["in_min"].copy(), i["in_max"].copy(), [f"c{j}" for j in range(c["units"][-1])])
    tr = an.trainer(spec, i["feat"], i["labels"], c["n_val"], c["batch"], c["lr"])
    h = hashlib.sha256()
    for o in i["orders"]:
        tr.epoch(o)
        st = tr.stats()
        ks, bs = tr.weights()
        for a in ks + bs:
            h.update(a.tobytes())
        h.update(np.array([st["loss"], st["acc"], st["val_loss"], st["val_acc"]], "<f8").tobytes())
    tr.close()
    return k6, h.hexdigest()


def test_53_wide_runs_keep_their_bits(torch, an):
    k6, k7 = digests_53(torch, an)
    print("53-wide digests:", k6, k7)
    assert k6 == DIGEST_53["classify"]
    assert k7 == DIGEST_53["train"]

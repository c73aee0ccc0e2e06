"""Regression groups on the GPU (wsa_regress_group_*, wsa_batch_regress_group; csrc/regress_fold.hip): every head of the grouped K6 launch
against wsa_regress_rows with that model and range, bit for bit; the fold RG-1 through the test entry wsa_debug_regress_fold on the
hand-built cases of tests/regress_fold_cases.py and over a batch's own rows against the float64 restatement rg1_ref, bit for bit; levels,
refusals, the batch's one-last-model-call rule and a hipGraph capture of run + group."""
import os

import numpy as np
import pytest

from tests import regress_fold_cases as C
from tests.test_gpu_stream_classify import GOLD, MODELS
from webspeechanalyzer_amd import capi, nnmodel

pytestmark = pytest.mark.gpu

SPECS = C.model_specs()
TABLES = ("cb", "cb_value", "cb_weight", "clip_sum", "clip_weight", "clip_value")


def _wide_spec():
    """53-400-1 sigmoid: wide enough that K6 gives it two row blocks per tile where the other fixture models get four"""
    from webspeechanalyzer_amd import train
    ks, bs = train.glorot_init([53, 400, 1], 4)
    base = SPECS["tfjs"]
    return nnmodel.ModelSpec([53, 400, 1], ["sigmoid", "sigmoid"], ks, bs, base.in_min, base.in_max, [], base.out_min, base.out_max)


def _rb(units):
    """K6's row blocks per tile for a stack (DESIGN.md "K6": the largest of 4, 2, 1 whose two activation buffers fit 160 KiB of LDS)"""
    S = ((max((u + 15) & ~15 for u in units) + 63) & ~63) + 4
    rb = 4
    while rb > 1 and 2 * 16 * rb * S * 4 > 160 * 1024:
        rb >>= 1
    return rb


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def an():
    a = capi.Analyzer(capi.Config(output_level=13), device=0)
    yield a
    a.close()


@pytest.fixture(scope="module")
def models(an):
    specs = dict(SPECS, wide_400=_wide_spec())
    ms = {k: an.load_model(v) for k, v in specs.items()}
    yield ms
    for m in ms.values():
        m.close()


# name -> [(model key, range or None)]: one head; the same model twice with two ranges; members of different depth; eight heads of both
# row-block factors
GROUPS = {
    1: [("tfjs", None)],
    2: [("sigmoid_64_16", None), ("sigmoid_64_16", (-1.0, 1.0))],
    3: [("sigmoid_64_16", (0.0, 1.0)), ("linear_8", None), ("tanh_16", (1.0, 9.0))],
    8: [("tfjs", None), ("wide_400", (0.0, 5.0)), ("linear_8", (-2.0, 2.0)), ("tanh_16", None), ("sigmoid_64_16", None), ("wide_400", None),
        ("tfjs", (3.0, -3.0)), ("linear_8", None)],
}


def _group(an, models, H):
    return an.regress_group([models[k] for k, _ in GROUPS[H]], [r for _, r in GROUPS[H]])


def _row_counts():
    n = {0, 1, 15, 16, 17, 63, 64, 65}
    for rb in {_rb(s.units) for s in dict(SPECS, w=_wide_spec()).values()}:
        n |= {16 * rb - 1, 16 * rb, 16 * rb + 1, 5 * 16 * rb + 3}
    return sorted(n)


def test_row_counts_cover_both_row_block_factors():
    assert {_rb(s.units) for s in SPECS.values()} == {4} and _rb(_wide_spec().units) == 2
    assert {31, 32, 33, 163, 323} <= set(_row_counts())


@pytest.mark.parametrize("H", sorted(GROUPS))
def test_group_rows_equal_regress_rows_per_head(an, models, torch, H):
    g = _group(an, models, H)
    lo, hi = SPECS["tfjs"].in_min, SPECS["tfjs"].in_max
    rng = np.random.default_rng(H)
    counts = _row_counts()
    feat = lo + (hi - lo) * rng.uniform(-0.1, 1.1, (max(counts), 53))
    d_feat = torch.tensor(feat, dtype=torch.float64, device="cuda:0")
    s = _stream(torch)
    for n in counts:
        out = torch.full((H, max(n, 1) + 1), -7.0, dtype=torch.float64, device="cuda:0")
        g.regress_rows(d_feat.data_ptr(), n, [out[h].data_ptr() for h in range(H)], s)
        want = torch.full((H, max(n, 1) + 1), -7.0, dtype=torch.float64, device="cuda:0")
        for h, (key, _) in enumerate(GROUPS[H]):
            if n:
                models[key].regress_rows(d_feat.data_ptr(), n, want[h].data_ptr(), *g.ranges[h], s)
        torch.cuda.synchronize()
        got, ref = out.cpu().numpy(), want.cpu().numpy()
        assert (got[:, n:] == -7.0).all(), n                       # nothing beyond the rows
        assert n == 0 or np.isfinite(ref[:, :n]).all()
        assert got.tobytes() == ref.tobytes(), (H, n)
    g.close()


def _ref_tables(case, cbs, run, n):
    H = case["values"].shape[0]
    cb = np.array([[c["who"], c["si"], c["first"], c["rows"]] for c in cbs], np.int32).reshape(-1, 4)
    cbv = np.array([c["value"] for c in cbs], np.float64).reshape(-1, H).T
    cbw = np.array([c["weight"] for c in cbs], np.float64).reshape(-1, H).T
    runs = [np.array([C.run_value(run, who, H)[k] for who in range(n)], np.float64).T for k in range(3)]
    return cb, cbv, cbw, runs


@pytest.mark.parametrize("case", C.batch_cases(), ids=lambda c: c["name"])
def test_debug_batch_fold_equals_rg1_ref(case):
    n = len(case["row_off"]) - 1
    got = capi.debug_regress_fold(case["meta"], case["values"], case["step_s"], case["row_off"])
    cbs, run = C.rg1_ref(case["meta"], case["values"], case["step_s"])
    cb, cbv, cbw, runs = _ref_tables(case, cbs, run, n)
    assert got["n_cb"] == len(cbs)
    assert np.array_equal(got["cb"], cb)
    assert got["cb_value"].tobytes() == np.ascontiguousarray(cbv).tobytes()
    assert got["cb_weight"].tobytes() == np.ascontiguousarray(cbw).tobytes()
    for k, name in enumerate(("run_sum", "run_weight", "run_value")):
        assert got[name].tobytes() == np.ascontiguousarray(runs[k]).tobytes(), name
    if case["name"] == "separate_rounding":                         # the device rounds the product and the sum separately
        fused, _ = C.rg1_ref(case["meta"], case["values"], case["step_s"], fused=True)
        assert np.ascontiguousarray(np.array([c["value"] for c in fused]).T).tobytes() != got["cb_value"].tobytes()


@pytest.mark.parametrize("case", C.stream_cases(), ids=lambda c: c["name"])
def test_debug_stream_fold_equals_rg1_ref(case):
    n = case["n"]
    got = capi.debug_regress_fold(case["meta"], case["values"], case["step_s"], case["row_off"], case["ctl"])
    steps = C.rg1_streams(case)
    assert got["n_cb"].tolist() == [len(cbs) for cbs, _ in steps]
    all_cbs = [c for cbs, _ in steps for c in cbs]
    cb, cbv, cbw, _ = _ref_tables(case, all_cbs, {}, n)
    assert np.array_equal(got["cb"], cb)
    assert got["cb_value"].tobytes() == np.ascontiguousarray(cbv).tobytes()
    assert got["cb_weight"].tobytes() == np.ascontiguousarray(cbw).tobytes()
    for k, (cbs, run) in enumerate(steps):
        runs = _ref_tables(case, [], run, n)[3]
        for j, name in enumerate(("run_sum", "run_weight", "run_value")):
            assert got[name][k].tobytes() == np.ascontiguousarray(runs[j]).tobytes(), (k, name)


def test_debug_entry_refuses_tables_that_do_not_fit():
    case = C.batch_cases()[0]
    bad = case["row_off"].copy(); bad[-1] += 1
    with pytest.raises(capi.WsaError):
        capi.debug_regress_fold(case["meta"], case["values"], case["step_s"], bad)
    meta = case["meta"].copy(); meta[0, 0] = 5
    with pytest.raises(capi.WsaError):
        capi.debug_regress_fold(meta, case["values"], case["step_s"], case["row_off"])


def _clips(torch, n=8, ns=32000, seed=2, silent=3):
    from webspeechanalyzer_amd.synth import synth_clips
    pcm = synth_clips(n, ns, fs=16000, seed=seed, device="cuda")
    if silent is not None:
        pcm[silent] = 0.0
    return pcm


def test_level13_batch_values_fold_callbacks_and_a_second_run(an, models, torch):
    s = _stream(torch)
    pcm = _clips(torch)
    g = _group(an, models, 3)
    b = an.batch([pcm.shape[1]] * 8, 16000)
    b.run(pcm.data_ptr(), pcm.stride(0), s)
    b.regress_group(g, s)
    got = b.value_fold(s)
    rows = b.rows(s)
    ro = rows["row_off"]
    assert len(rows["meta"]) > 0 and ro[3] == ro[4] and got["value"].shape == (3, len(rows["meta"]))
    # the fold, bit for bit, over the batch's own rows and values
    case = dict(values=got["value"])
    cbs, run = C.rg1_ref(rows["meta"], got["value"], an.config["window_step"] / 1e3)
    cb, cbv, cbw, runs = _ref_tables(case, cbs, run, 8)
    assert len(cbs) > 8 and np.array_equal(got["cb"], cb)
    assert got["cb_value"].tobytes() == np.ascontiguousarray(cbv).tobytes() and got["cb_weight"].tobytes() == np.ascontiguousarray(cbw).tobytes()
    for k, name in enumerate(("clip_sum", "clip_weight", "clip_value")):
        assert got[name].tobytes() == np.ascontiguousarray(runs[k]).tobytes(), name
    assert np.isnan(got["clip_value"][:, 3]).all() and not got["clip_weight"][:, 3].any()      # the silent clip: zeros and NaN
    # the result kinds stay apart
    with pytest.raises(capi.WsaError, match="no wsa_batch_classify on this batch yet"):
        b.classes(s)
    with pytest.raises(capi.WsaError, match="not wsa_batch_regress"):
        b.values(s)
    # every head's values are wsa_batch_regress' with that model and range
    for h, (key, _) in enumerate(GROUPS[3]):
        b.regress(models[key], *g.ranges[h], stream=s)
        assert b.values(s).tobytes() == got["value"][h].tobytes(), key
    with pytest.raises(capi.WsaError, match="not wsa_batch_regress_group"):
        b.value_fold(s)
    # the callback records are the classifier's for the same run
    m = an.load_model(os.path.join(GOLD, "nn", MODELS[0]))
    b.classify(m, s)
    assert np.array_equal(b.classes(s)["cb"], got["cb"])
    # a second run of the batch gives the same bits
    b.run(pcm.data_ptr(), pcm.stride(0), s)
    b.regress_group(g, s)
    again = b.value_fold(s)
    for name in ("value",) + TABLES:
        assert again[name].tobytes() == got[name].tobytes(), name
    with pytest.raises(capi.WsaError, match="last model call was wsa_batch_regress_group"):
        b.classes(s)
    # capacities are checked, any pointer may be NULL
    h = capi._ValueHost()
    h.rows_cap, h.cb_cap = len(rows["meta"]) - 1, len(cbs) - 1
    small = np.zeros(len(rows["meta"]))
    h.value[1] = small.ctypes.data
    with pytest.raises(capi.WsaError, match="value buffer too small"):
        an._check(b.L.wsa_batch_copy_value_fold(b.h, s, capi.ctypes.byref(h)))
    h.value[1] = None; h.cb_weight[2] = small.ctypes.data
    with pytest.raises(capi.WsaError, match="callback buffer too small"):
        an._check(b.L.wsa_batch_copy_value_fold(b.h, s, capi.ctypes.byref(h)))
    h.cb_cap = len(cbs)
    an._check(b.L.wsa_batch_copy_value_fold(b.h, s, capi.ctypes.byref(h)))
    assert small[:len(cbs)].tobytes() == got["cb_weight"][2].tobytes()
    fresh = an.batch([16000], 16000)
    with pytest.raises(capi.WsaError, match="no wsa_batch_regress_group on this batch yet"):
        fresh.value_fold(s)
    fresh.close(); m.close(); b.close(); g.close()


def test_level5_gives_values_only(torch):
    s = _stream(torch)
    pcm = _clips(torch, n=3, silent=None)
    an5 = capi.Analyzer(capi.Config(output_level=5))
    ms = [an5.load_model(SPECS[k]) for k in ("tfjs", "tanh_16")]
    g = an5.regress_group(ms)
    b = an5.batch([pcm.shape[1]] * 3, 16000)
    b.run(pcm.data_ptr(), pcm.stride(0), s)
    b.regress_group(g, s)
    r = b.value_result(s)
    assert r.n_callbacks == 0 and not r.d_cb and not r.d_cb_value[0] and not r.d_clip_sum[0] and r.n_heads == 2
    got = b.value_fold(s)
    assert sorted(got) == ["value"] and got["value"].shape[1] == len(b.rows(s)["meta"]) > 0
    for h, m in enumerate(ms):
        b.regress(m, stream=s)
        assert b.values(s).tobytes() == got["value"][h].tobytes()
    b.close(); g.close()
    for m in ms:
        m.close()
    an5.close()


@pytest.mark.parametrize("level", [3, 4, 10, 11, 12])
def test_other_levels_are_refused_by_name(level):
    a = capi.Analyzer(capi.Config(output_level=level))
    m = a.load_model(SPECS["linear_8"])
    g = a.regress_group([m])
    b = a.batch([16000], 16000)
    with pytest.raises(capi.WsaError, match=f"wsa_batch_regress_group needs a batch at output_level 5 .*or 13 .*not {level}"):
        b.regress_group(g)
    b.close(); g.close(); m.close(); a.close()


def test_group_refusals(an, models):
    ok = models["linear_8"]
    with pytest.raises(capi.WsaError, match="1 .. 8 heads, got 0"):
        an.regress_group([])
    with pytest.raises(capi.WsaError, match="1 .. 8 heads, got 9"):
        an.regress_group([ok] * 9)
    m_cls = an.load_model(os.path.join(GOLD, "nn", MODELS[0]))
    with pytest.raises(capi.WsaError, match="head 1: a regression model's last layer .* not softmax"):
        an.regress_group([ok, m_cls], [None, (0.0, 1.0)])
    from webspeechanalyzer_amd import train
    ks, bs = train.glorot_init([264, 8, 1], 6)
    m_wide = an.load_model(nnmodel.ModelSpec([264, 8, 1], ["sigmoid", "sigmoid"], ks, bs, np.zeros(264), np.ones(264), [], 0.0, 1.0))
    with pytest.raises(capi.WsaError, match="head 0 takes 264 inputs"):
        an.regress_group([m_wide])
    ks, bs = train.glorot_init([53, 8, 2], 6)
    m_two = an.load_model(nnmodel.ModelSpec([53, 8, 2], ["sigmoid", "sigmoid"], ks, bs, SPECS["tfjs"].in_min, SPECS["tfjs"].in_max, [], 0.0, 1.0))
    with pytest.raises(capi.WsaError, match="head 0: a regression model has one output unit"):
        an.regress_group([m_two])
    other = capi.Analyzer(capi.Config(output_level=13))
    m_other = other.load_model(SPECS["linear_8"])
    with pytest.raises(capi.WsaError, match="head 1 was created on another context"):
        an.regress_group([ok, m_other])
    with pytest.raises(capi.WsaError, match="head 0: the output has max == min"):
        an.regress_group([ok], [(0.5, 0.5)])
    with pytest.raises(capi.WsaError, match="head 2: non-finite out_min / out_max"):
        an.regress_group([ok, ok, ok], [None, None, (0.0, float("inf"))])
    with pytest.raises(capi.WsaError, match="head 1 is NULL"):
        an.regress_group([ok, None])
    g_other = other.regress_group([m_other])
    b = an.batch([16000], 16000)
    with pytest.raises(capi.WsaError, match="another context"):
        b.regress_group(g_other)
    b.close(); g_other.close()
    for m in (m_cls, m_wide, m_two, m_other):
        m.close()
    other.close()


def test_graph_capture_of_run_and_group(an, models, torch):
    s = _stream(torch)
    a, c = _clips(torch, seed=31, silent=None), _clips(torch, seed=32, silent=5)
    g = _group(an, models, 8)
    n, ns = a.shape
    plain = an.batch([ns] * n, 16000)
    refs = []
    for x in (a, c):
        plain.run(x.data_ptr(), x.stride(0), s)
        plain.regress_group(g, s)
        refs.append(plain.value_fold(s))
    b = an.batch([ns] * n, 16000)
    b.enable_timing(False)
    buf = a.clone()
    b.run(buf.data_ptr(), buf.stride(0), s)
    b.regress_group(g, s)                                # the first call allocates; the captured one does not
    b.value_fold(s)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            b.run(buf.data_ptr(), buf.stride(0), side.cuda_stream)
            b.regress_group(g, side.cuda_stream)
        for x, ref in ((c, refs[1]), (a, refs[0]), (c, refs[1])):
            buf.copy_(x)
            graph.replay()
            side.synchronize()
            got = b.value_fold(side.cuda_stream)
            assert len(got["cb"]) > 0
            for name in ("value",) + TABLES:
                assert got[name].tobytes() == ref[name].tobytes(), name
    plain.close(); b.close(); g.close()

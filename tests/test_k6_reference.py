"""The K6 restatement (tests/k6_ref.py, oracle/dense.c) and its cases (tests/k6_cases.py) on the CPU: every arm is reached, the
exact-integer networks are exact in any order, D32 is the recorded one, every modelled fault changes some case's expected bits, and the
restatement lies within the existing 1e-5 of classify_ref.forward.  tests/test_gpu_k6.py runs the same cases on the GPU."""
import numpy as np
import pytest

from tests import classify_ref, k6_cases as kc, k6_ref as kr

INT_KEYS = [k for k, c in kc.CASES.items() if c["kind"] == "int"]
REAL_KEYS = [k for k, c in kc.CASES.items() if c["kind"] == "real"] + list(kc.GROUP_CASES)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """the same f32 values bit for bit, a NaN standing for any NaN (the payload of a generated NaN is the machine's own)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb])


def _group_specs():
    specs, feat = kc.group_build()
    return [specs[k] for k in kc.GROUP], feat


def test_every_arm_is_reached():
    kr.ARMS.clear()
    for key in kc.KEYS:
        c = kc.CASES[key]
        e = kc.expected.__wrapped__(key)
        rb = kc.rb_of(c)
        for n in kc.row_counts(c):
            kr.tile_walk(n, rb, 1)                                              # rows_cap = 1: one workgroup walks every tile
            kr.output_table(np.zeros((kc.n_rows(c), 1), np.float32), n, n + 3)
    spec, feat = kc.build("i_63_64_65")                                         # the strided form: 23 inputs, 24 doubles per row, slot 23 marked
    n = len(feat)
    kr.output_table(kr.forward_bits(spec, feat)["out"], n, n + 3, nan_rows=kc.marked_rows(n, kc.rb_of(kc.CASES["i_63_64_65"])))
    specs, _ = _group_specs()
    order = kr.group_order([s.units for s in specs])
    rbs = [kr.row_blocks(specs[d].units) for d in order]
    for n in kc.GROUP_COUNTS:
        for one_block in (False, True):
            r = [1] * len(rbs) if one_block else rbs
            grid = sum((kc.GROUP_ROWS_CAP + 16 * b - 1) // (16 * b) for b in r)
            rows = kr.group_walk(n, r, grid)
            assert all(s == set(range(n)) for s in rows)
    print({k: kr.ARMS[k] for k in kr.ARM_NAMES})
    assert [k for k in kr.ARM_NAMES if kr.ARMS[k] == 0] == []
    assert set(kr.ARMS) <= set(kr.ARM_NAMES)


def test_the_row_block_factor_changes_where_the_lds_budget_says():
    assert [kr.row_blocks([53, w, 8]) for w in (256, 257, 272, 576, 577, 592, 1024)] == [4, 2, 2, 2, 1, 1, 1]
    assert {kc.rb_of(kc.CASES[k]) for k in ("i_255_256", "i_257", "i_576", "i_577", "i_1024")} == {4, 2, 1}
    assert (kc.rb_of(kc.CASES["i_255_256"]), kc.rb_of(kc.CASES["i_257"]), kc.rb_of(kc.CASES["i_576"]), kc.rb_of(kc.CASES["i_577"])) == (4, 2, 2, 1)
    assert [kr.row_blocks(kc.GROUP_CASES[k]["units"]) for k in kc.GROUP] == [4, 2, 1, 4]
    widths = {u for k in INT_KEYS for u in kc.CASES[k]["units"][1:]}
    assert widths >= {1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 576, 577, 1024}
    assert {kc.CASES[k]["units"][-1] for k in INT_KEYS} >= set(kc.C_EDGES)
    assert {kc.CASES[k]["units"][0] for k in INT_KEYS} == {53, 264, 23}
    assert {len(kc.CASES[k]["units"]) - 1 for k in INT_KEYS} >= {1, 8}


@pytest.mark.parametrize("key", INT_KEYS)
def test_exact_integer_networks_are_exact_in_any_order(key):
    """features are multiples of 1/2 and the weights integers: with 2 (sum |a w| + |b|) < 2^24 at every unit of every layer every partial sum
    is a multiple of 1/2 below 2^23, exact in f32 whatever the order"""
    spec, feat = kc.build(key)
    a = np.abs(feat)
    x = feat.copy()
    for k, b, act in zip(spec.kernels, spec.biases, spec.activations):
        worst = a @ np.abs(k.astype(np.float64)) + np.abs(b.astype(np.float64))
        assert 2.0 * worst.max() < 2.0 ** 24, f"{key}: {worst.max()}"
        x = x @ k.astype(np.float64) + b.astype(np.float64)
        if act == "relu":
            x = np.maximum(x, 0.0)
        a = np.abs(x)
    want = kr.forward_bits(spec, feat)["out"]
    assert np.array_equal(want.astype(np.float64), x)
    assert len(np.unique(want)) > min(8, want.size // 4)                        # no dead network
    for fault in ("k_descending", "pairs", "bias_first"):
        assert np.array_equal(_bits(kr.forward_bits(spec, feat, fault=fault)["out"]), _bits(want))


@pytest.mark.parametrize("key", kc.D32_KEYS)
def test_d32_is_the_recorded_one(key):
    d = kc.d32(key)
    print(f"{key}: D32 = {d:.3e} (recorded {kc.CASES[key]['d32']:.3e}, bound {kc.bound(kc.CASES[key]):.3e})")
    assert 0.0 < d <= 2.0 * kc.CASES[key]["d32"]


@pytest.mark.parametrize("key", REAL_KEYS)
@pytest.mark.parametrize("fault", ["k_descending", "pairs", "bias_first"])
def test_a_wrong_order_gives_other_bits_on_every_real_case(key, fault):
    if key in kc.GROUP_CASES:
        specs, feat = kc.group_build()
        spec = specs[key]
    else:
        spec, feat = kc.build(key)
    feat = feat[:83]
    want, got = kr.forward_bits(spec, feat)["out"], kr.forward_bits(spec, feat, fault=fault)["out"]
    differing = int(np.any(_bits(want) != _bits(got), axis=1).sum())
    print(f"{key} {fault}: {differing} of {len(feat)} rows differ")
    assert differing >= 1


def _changed(key, fault):
    spec, feat = kc.build(key)
    return not _same(kr.forward_bits(spec, feat)["out"], kr.forward_bits(spec, feat, fault=fault)["out"])


def test_a_k_loop_one_block_short_is_noticed():
    assert all(_changed(k, "k_block_short") for k in INT_KEYS)


def test_a_skipped_column_block_is_noticed():
    assert all(_changed(k, "col_block_skipped") for k in ("i_255_256", "i_257", "i_576", "i_577", "i_1024"))


def test_kept_padded_columns_are_noticed():
    """a padded column beside an Inf input holds Inf x 0 = NaN: kept, it poisons the next layer through its zero weight rows.  After relu the
    linear twin's logits show it (+-Inf become NaN); after sigmoid the finite probabilities themselves turn NaN"""
    assert _changed("s_relu", "pad_cols_kept")
    spec, feat = kc.build("s_sigmoid")
    y = kc.expected("s_sigmoid")["yard"]
    for r in (5, 6, 8, 16):                                                     # +-Inf in one input: finite probabilities, as in tfjs
        assert np.all(np.isfinite(y[r])), r
    for r in (1, 3):
        assert np.all(np.isnan(y[r])), r
    # the fault, restated: the padded hidden columns keep sigmoid(NaN) beside an Inf input
    pre0 = kr.forward_bits(kc.twin(spec, 0), feat)["pre"][0]
    assert np.all(np.isnan(pre0[[5, 6, 8, 16], spec.units[1]:]))
    assert not np.any(np.isnan(pre0[[0, 2, 4, 7], spec.units[1]:]))


def test_a_dropped_k_guard_is_noticed():
    for key in ("s_relu", "s_sigmoid"):
        spec, feat = kc.build(key)
        t = kc.twin(spec, 0)
        want, got = kr.forward_bits(t, feat)["out"], kr.forward_bits(t, feat, fault="k_guard")["out"]
        for r in (2, 4):            # the padded k 53 .. 63 of a row read the next row's features 0 .. 10 through zero weights: row 3's NaN at 0, row 5's Inf at 10
            assert np.all(np.isnan(got[r])) and not np.any(np.isnan(want[r])), (key, r)
        assert _same(got[[0, 13, 14]], want[[0, 13, 14]])


def test_a_row_guard_off_by_one_is_noticed():
    spec, feat = kc.build("i_15_16_17")
    v = kr.forward_bits(spec, feat)["out"]
    for n in (1, 16, 17):
        assert not np.array_equal(kr.output_table(v, n, n + 3), kr.output_table(v, n, n + 3, fault="row_guard"))


def test_a_softmax_without_the_max_is_noticed():
    logits = kc.expected("s_logits")["logits"]
    right, wrong = kr.softmax(logits), kr.softmax(logits, fault="no_max")
    assert np.all(np.isfinite(right[:8])) and np.all(wrong[:4] == 0)             # exp(1e4) = Inf: log-sum-exp Inf, every probability 0
    assert np.all(np.isnan(right[8:10]))                                        # one +Inf logit: m = +Inf, Inf - Inf
    assert np.allclose(right[0], [1 / 3, 0, 1 / 3, 0, 1 / 3]) and np.allclose(right[4], 0.2)


@pytest.mark.parametrize("key", ["r_app_reg", "r_app_reg_b"])
def test_a_contracted_epilogue_is_noticed(key):
    c = kc.CASES[key]
    p = kc.expected(key)["logits"][:, 0]
    two, one = kr.unnormalise(p, *c["out_range"]), kr.unnormalise(p, *c["out_range"], fault="fused_epilogue")
    differing = int((two.view(np.uint64) != one.view(np.uint64)).sum())
    print(f"{key}: fma(p, span, min) differs from the two roundings on {differing} of {len(p)} rows")
    assert differing >= 1
    assert np.array_equal(two, p.astype(np.float64) * (c["out_range"][1] - c["out_range"][0]) + c["out_range"][0])


def test_a_walk_that_keeps_the_tile_index_is_noticed():
    specs, _ = _group_specs()
    order = kr.group_order([s.units for s in specs])
    assert order == [2, 1, 0, 3]                                                # by cost per tile: 577 x 1, 257 x 2, then the two 64 x 4 in the given order
    rbs = [kr.row_blocks(specs[d].units) for d in order]
    grid = sum((kc.GROUP_ROWS_CAP + 16 * b - 1) // (16 * b) for b in rbs)
    for n in (17, 33, 65):
        rows = kr.group_walk(n, rbs, grid, fault="tile_kept")
        assert any(s != set(range(n)) for s in rows), n


@pytest.mark.parametrize("key", kc.KEYS)
def test_the_restatement_is_within_1e5_of_the_float64_forward(key):
    spec, feat = kc.build(key)
    if kc.CASES[key]["rows"]:
        feat = feat[:83]
    e = kc.expected(key)
    if key in kc.EXACT_KEYS:
        got = e["logits"][:len(feat)].astype(np.float64)
        if spec.activations[-1] == "softmax":
            got = kr.softmax(got)
    else:
        got = kr.forward64(spec, feat)
    with np.errstate(all="ignore"):
        want = classify_ref.forward(spec, feat)
    ok = np.all(np.isfinite(want), axis=1) & np.all(np.isfinite(got), axis=1)
    if key == "s_flat_range":                                                   # every row has a NaN or an Inf input: NaN throughout, on both sides
        assert np.all(np.isnan(want)) and np.all(np.isnan(got))
        return
    assert ok.sum() >= 4
    scale = np.maximum(1.0, np.abs(want[ok]))
    assert np.max(np.abs(got[ok] - want[ok]) / scale) <= 1e-5

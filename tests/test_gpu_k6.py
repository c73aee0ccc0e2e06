"""K6 / K6e (csrc/classify.hip classify_tile<RB>, classify_kernel, classify_group_kernel) on hand-built networks (-m gpu): the cases of
tests/k6_cases.py through wsa_classify_rows / wsa_regress_rows and through the test entry wsa_debug_classify (csrc/debug_classify.hip), against the literal
restatement tests/k6_ref.py (oracle/dense.c), which tests/test_k6_reference.py examines on the CPU.

What is compared bit for bit (a NaN standing for any NaN: the payload of a generated NaN is the machine's own): the output of every network whose
activations are relu or linear, the logits of every softmax model over such layers (handed out by its linear twin), the first layer's pre-activation
values of the tanh / sigmoid cases (handed out by a truncated twin), the regression values (two roundings), a row's bits whatever the tile, the
row-block factor, the launch form or the group it was computed in, and every table past the row count against its seeded pattern.
What has a tolerance: softmax and tanh / sigmoid layers, whose libm is the device's own: 4 x D32 per case (k6_cases.bound), no row or output left out.

Measured on an MI355X: the bit equality holds on every case, the real-valued ones included — mfma_f32_16x16x4f32 fed K ascending is the f32 fmaf chain
of oracle/dense.c, subnormals and signed zeros included; no fault was found in K6 or K6e.

Arms (k6_ref.ARMS; counts over all cases, tests/test_k6_reference.py::test_every_arm_is_reached):

    pad_k.input          103834  padded K rows of the input (53 -> 64, 264 -> 272, 23 -> 32)
    pad_col.nonzero_act    7545  padded columns of a hidden sigmoid layer (0.5 before they are zeroed)
    row.past_n              145  a row past n in the last tile
    relu.negative       2476514  relu.neg_zero 136 (s_neg_zero: a product that underflows to -0 under a -0 bias; no sum from +0 gets there)   relu.nan 488
    fmax.nan_skipped         16  softmax.m_inf 6 (s_logits)
    nan_slot.set              3  nan_slot.clear 320 (a mark of -0 is clear)
    range0.inf               12  range0.nan 5 (s_flat_range: in_max == in_min with x != min and x == min)
    wg.second_tile          158  a workgroup's second tile (rows_cap = 1; r_widest's 263 tiles on 256 workgroups through wsa_classify_rows)
    group.fell_through       16  K6e's walk reaching the last member without a break

Tolerance cases: D32 (float64 yardstick against its numpy-float32 twin, CPU), the bound 4 x D32 and the device's distance from the yardstick:

    case         D32        bound      device          case         D32        bound      device
    r_app_cls    8.69e-8    3.48e-7    7.92e-8         t_tanh_out   1.45e-7    5.80e-7    1.52e-7
    r_widest     3.21e-8    1.28e-7    5.06e-8         s_relu       5.81e-8    2.32e-7    7.51e-8
    t_17_16      1.32e-7    5.28e-7    1.02e-7         s_sigmoid    1.57e-7    6.28e-7    1.67e-7
    t_257        1.18e-7    4.72e-7    2.07e-7         s_logits     1.06e-4    4.24e-4    1.06e-4  (logits of +-1e4: log-sum-exp 10001.6 has an f32 ulp of 1e-3)
    t_app_reg    6.60e-7    2.64e-6    6.02e-7         s_flat_range, s_one_class: no finite tolerance (all NaN; exactly 1.0f)

Kernel mutations, each built once into a scratch copy of the library and run against this file (no mutated code is kept; every one keeps its reads and
writes inside the tables); the named test is one that fails, the number how many of this file's 108 do:

    mutation (csrc/classify.hip)                                                            fails  a test that fails
    the K loop ends one block of 16 early                                                     103  test_rows_api_at_every_row_count[i_one_unit]
    a wave takes its first column block only (columns past 128 never computed)                 34  test_rows_api_at_every_row_count[i_255_256]
    hidden column 17 comes out 0                                                               60  test_rows_api_at_every_row_count[i_63_64_65]
    `if (col >= L.n && !last) v = 0` dropped                                                   10  test_rows_api_at_every_row_count[s_sigmoid]
    `k < p.nin` dropped (a padded k reads on into the next row)                                14  test_rows_api_at_every_row_count[s_relu]
    `row0 + r >= n` -> `> n` in the epilogue (where the table has room)                        71  test_entry_one_workgroup_walks_every_tile[i_one_unit]
    K descending (blocks and the four steps of a block)                                        49  test_rows_api_at_every_row_count[r_app_cls]
    the K steps of a block in the order 1, 0, 3, 2                                             49  test_rows_api_at_every_row_count[r_app_reg]
    the bias as the chain's start instead of an add of its own                                 49  test_rows_api_at_every_row_count[r_widest]
    the normalisation in f32 instead of double                                                 45  test_rows_api_at_every_row_count[r_app_reg_b]
    relu as fmaxf(v, 0) (-0 -> +0, NaN -> 0)                                                   13  test_rows_api_at_every_row_count[s_neg_zero]
    softmax without the max (m = 0)                                                             8  test_rows_api_at_every_row_count[s_logits]
    unnormalise_value as one fma                                                                8  test_rows_api_at_every_row_count[r_app_reg]
    the nan_slot test `!= 0.0` -> `> 0.0`                                                       3  test_strided_rows_with_the_nan_slot[i_23_one]
    `tile -= t` dropped in classify_group_kernel                                                2  test_group_members_equal_their_solo_runs[own-rb]
    classify_group_kernel runs an RB 4 member's tile as classify_tile<2>                        1  test_group_members_equal_their_solo_runs[own-rb]

A chain in pairs has no form on this instruction; tests/test_k6_reference.py shows on the restatement that every real-valued case would tell it.
"""
import numpy as np
import pytest

from tests import k6_cases as kc
from tests import k6_ref as kr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def capi():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from webspeechanalyzer_amd import capi
    return capi


@pytest.fixture(scope="module")
def an(capi):
    import webspeechanalyzer_amd as wsa
    a = wsa.Analyzer(wsa.Config(output_level=13))
    yield a
    for m in _MODELS.values():
        m.close()
    _MODELS.clear(); _BASE.clear()
    a.close()


_MODELS, _BASE = {}, {}


def _model(an, name, spec):
    if name not in _MODELS:
        _MODELS[name] = an.load_model(spec)
    return _MODELS[name]


def _rows_api(model, feat, out_range=None):
    """wsa_classify_rows / wsa_regress_rows over feat: the output's bits, uint32 [n, C] or uint64 [n, 1]"""
    n = len(feat)
    s = torch.cuda.current_stream().cuda_stream
    d_feat = torch.from_numpy(np.ascontiguousarray(feat, np.float64)).cuda()
    if out_range is not None:
        d_out = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
        model.regress_rows(d_feat.data_ptr(), n, d_out.data_ptr(), out_range[0], out_range[1], s)
        torch.cuda.synchronize()
        return d_out.cpu().numpy().view(np.uint64)[:, None]
    d_out = torch.full((n, model.n_classes), -1.0, dtype=torch.float32, device="cuda")
    model.classify_rows(d_feat.data_ptr(), n, d_out.data_ptr(), s)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint32)


def _values(bits):
    return bits.view(np.float64 if bits.dtype == np.uint64 else np.float32)


def _assert_same(got, want, what):
    """bit for bit, a NaN standing for any NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    g, w = _values(got), _values(want)
    bad = np.argwhere((np.isnan(g) != np.isnan(w)) | (~np.isnan(w) & (got != want)))
    assert len(bad) == 0, (f"{what}: {len(bad)} values differ, first at (row, unit) {bad[0].tolist()}: got {got[tuple(bad[0])]:#x} ({g[tuple(bad[0])]!r}) "
                           f"want {want[tuple(bad[0])]:#x} ({w[tuple(bad[0])]!r})")


def _base(an, key):
    """every row of the case through the rows API, checked against the restatement once: the bits every other form must repeat"""
    if key in _BASE:
        return _BASE[key]
    c = kc.CASES[key]
    spec, feat = kc.build(key)
    e = kc.expected(key)
    got = _rows_api(_model(an, key, spec), feat, c["out_range"])
    if e["logits"] is not None and spec.activations[-1] == "softmax":            # the linear twin hands out the logits
        _assert_same(_rows_api(_model(an, key + "/linear", kc.twin(spec)), feat), e["logits"].view(np.uint32), f"{key}: logits")
    if e["pre0"] is not None:                                                   # the truncated twin: the first layer before its activation
        _assert_same(_rows_api(_model(an, key + "/first", kc.twin(spec, 0)), feat), e["pre0"].view(np.uint32), f"{key}: first layer")
    if e["bits"] is not None:
        _assert_same(got, e["bits"], key)
    if e["yard"] is not None:
        y = e["yard"] if e["yard"].ndim == 2 else e["yard"][:, None]
        d = kr.distance(_values(got), y)
        limit = kc.bound(c) if c["d32"] is not None else 0.0
        print(f"K6DIST {key}: device {d:.3e}  D32 {c['d32']}  bound {limit:.3e}")
        assert d <= limit, f"{key}: {d:.3e} from the float64 yardstick, bound {limit:.3e}"
    _BASE[key] = got
    return got


def _table(base, n, rows):
    out = np.full((rows,) + base.shape[1:], kr.SEED_F64 if base.dtype == np.uint64 else kr.SEED_F32, base.dtype)
    out[:n] = base[:n]
    return out


def _entry(capi, model, feat, c, **kw):
    out = capi.debug_classify(model, feat, out_range=c["out_range"], **kw)
    return out[:, None] if out.ndim == 1 else out


@pytest.mark.parametrize("key", kc.KEYS)
def test_rows_api_at_every_row_count(an, key):
    c = kc.CASES[key]
    spec, feat = kc.build(key)
    base = _base(an, key)
    m = _model(an, key, spec)
    assert np.array_equal(_rows_api(m, feat, c["out_range"]), base), f"{key}: two runs differ"
    for n in kc.row_counts(c):
        if n <= len(feat):
            assert np.array_equal(_rows_api(m, feat[:n], c["out_range"]), base[:n]), f"{key}: {n} rows"


@pytest.mark.parametrize("key", kc.KEYS)
def test_entry_one_workgroup_walks_every_tile(an, capi, key):
    """rows_cap = 1 with the count on the device: a grid of one workgroup, its LDS reused from tile to tile"""
    c = kc.CASES[key]
    spec, feat = kc.build(key)
    base, m = _base(an, key), _model(an, key, spec)
    feat = feat[:5 * 16 * kc.rb_of(c) + 3]
    for n in kc.row_counts(c):
        if n <= len(feat):
            got = _entry(capi, m, feat, c, n_dev=n, rows_cap=1, out_rows=n + 3)
            assert np.array_equal(got, _table(base, n, n + 3)), f"{key}: {n} rows"


@pytest.mark.parametrize("key", kc.KEYS)
def test_entry_count_below_the_capacity(an, capi, key):
    """a grid sized for more rows than the device-side count says: nothing past the count is written"""
    c = kc.CASES[key]
    spec, feat = kc.build(key)
    base, m = _base(an, key), _model(an, key, spec)
    tm = 16 * kc.rb_of(c)
    feat = feat[:5 * tm + 3]
    some = min(tm + 1, len(feat) - 1)
    for n in (0, some):
        got = _entry(capi, m, feat, c, n_dev=n, rows_cap=len(feat), out_rows=len(feat))
        assert np.array_equal(got, _table(base, n, len(feat))), f"{key}: {n} rows of {len(feat)}"
    got = _entry(capi, m, feat, c, n_rows=some, rows_cap=len(feat), out_rows=len(feat))              # the count as a launch argument
    assert np.array_equal(got, _table(base, some, len(feat))), f"{key}: {some} rows of {len(feat)}, counted on the host"


@pytest.mark.parametrize("key", kc.KEYS)
def test_entry_every_row_block_factor(an, capi, key):
    """RB 1 (the form stream steps use), 2 and 4 where the model's LDS allows them (launch_classify keeps the model's own otherwise): the same bits"""
    c = kc.CASES[key]
    spec, feat = kc.build(key)
    base, m = _base(an, key), _model(an, key, spec)
    feat = feat[:5 * 16 * kc.rb_of(c) + 3]
    n = len(feat)
    for rb in (1, 2, 4):
        for cap in (n, 1):
            got = _entry(capi, m, feat, c, n_dev=n, rows_cap=cap, rb=rb, out_rows=n + 3)
            assert np.array_equal(got, _table(base, n, n + 3)), f"{key}: RB {rb}, rows_cap {cap}"


@pytest.mark.parametrize("key", ["s_relu", "s_sigmoid"])
def test_a_poisoned_row_leaves_its_neighbours_alone(an, key):
    spec, feat = kc.build(key)
    base = _base(an, key)
    clean = _rows_api(_model(an, key, spec), kc.clean_rows(key))
    ordinary = [r for r in range(kc.S_ROWS) if r not in kc.POISON]
    assert np.array_equal(base[ordinary], clean[ordinary])
    assert np.all(np.isfinite(_values(clean)))
    first = _model(an, key + "/first", kc.twin(spec, 0))
    assert np.array_equal(_rows_api(first, feat)[ordinary], _rows_api(first, kc.clean_rows(key))[ordinary])


@pytest.mark.parametrize("key", ["i_63_64_65", "i_23_one", "t_tanh_out"])
def test_strided_rows_with_the_nan_slot(an, capi, key):
    """24 doubles per row for a 23-input model, slot 23 the mark: marked rows first, last and alone in a tile get K6's NaN, a mark of -0 is none"""
    c = kc.CASES[key]
    spec, feat = kc.build(key)
    base, m = _base(an, key), _model(an, key, spec)
    n, rb = len(feat), kc.rb_of(c)
    marked = kc.marked_rows(n, rb)
    wide = np.concatenate([feat, np.zeros((n, 1))], axis=1)
    wide[marked, 23] = [7.0, float("nan"), -1e-300][:len(marked)]
    wide[1, 23] = -0.0
    for out_range in (None, (2.0, 5.0)) if spec.units[-1] == 1 and spec.activations[-1] != "softmax" else (None,):
        if out_range is None:
            want = kr.output_table(_values(base), n, n + 3, nan_rows=marked)
        else:                                                                   # the regression epilogue on the device's own f32 output: two roundings
            want = kr.output_table(kr.unnormalise(_values(base)[:, 0], *out_range)[:, None], n, n + 3, nan_rows=marked, f64=True)
        for kw in (dict(n_dev=n, rows_cap=n), dict(n_dev=n, rows_cap=1), dict(n_rows=n, rows_cap=n), dict(n_dev=n, rows_cap=n, rb=1)):
            got = capi.debug_classify(m, wide, nan_slot=23, out_range=out_range, out_rows=n + 3, **kw)
            got = got[:, None] if got.ndim == 1 else got
            assert np.array_equal(got, want), f"{key}: {kw}, range {out_range}"
        plain = capi.debug_classify(m, wide, nan_slot=-1, out_range=out_range, out_rows=n + 3, n_dev=n)
        plain = plain[:, None] if plain.ndim == 1 else plain
        assert np.array_equal(np.delete(plain, marked, 0), np.delete(want, marked, 0)) and not np.array_equal(plain[marked], want[marked])


@pytest.mark.parametrize("one_block", [False, True], ids=["own-rb", "one-block"])
def test_group_members_equal_their_solo_runs(an, capi, one_block):
    """K6e over members with RB 4, 2 and 1 (one model twice), in cost order 577, 257, 64, 64: the (member, tile) walk at counts below, at and one
    above what the grid holds, every member bit for bit its solo run, the tables past the count untouched"""
    specs, feat = kc.group_build()
    models = [_model(an, k, specs[k]) for k in kc.GROUP]
    solo = [_rows_api(m, feat) for m in models]
    for d, k in enumerate(kc.GROUP):
        _assert_same(solo[d], kr.forward_bits(specs[k], feat)["out"].view(np.uint32), f"group member {k} solo")
    R = len(feat) + 3
    for n in kc.GROUP_COUNTS:
        for _ in range(2):
            outs = capi.debug_classify(models, feat, n_dev=n, rows_cap=kc.GROUP_ROWS_CAP, one_block=one_block, out_rows=R)
            for d, k in enumerate(kc.GROUP):
                assert np.array_equal(outs[d], _table(solo[d], n, R)), f"member {d} ({k}), {n} rows"


def test_the_entry_refuses_what_would_leave_its_tables(an, capi):
    spec, feat = kc.build("i_23_one")
    m = _model(an, "i_23_one", spec)
    for kw in (dict(n_dev=len(feat) + 1), dict(n_rows=len(feat) + 1), dict(n_dev=4, out_rows=3), dict(n_dev=4, nan_slot=23), dict(n_dev=4, rb=3),
               dict(n_dev=4, one_block=True), dict(n_dev=4, rows_cap=0)):
        with pytest.raises(capi.WsaError):
            capi.debug_classify(m, feat, **kw)
    with pytest.raises(capi.WsaError):
        capi.debug_classify(m, feat[:, :22], n_dev=4)                           # a stride below the model's inputs
    with pytest.raises(capi.WsaError):
        capi.debug_classify([m, m], feat, n_dev=4)                              # a group takes 53-input members
    with pytest.raises(capi.WsaError):
        capi.debug_classify(m, feat, n_dev=4, out_range=(1.0, 1.0))             # 16 output units, and max == min

"""The KNN kernels (csrc/knn.hip: knn_add_kernel, knn_within_kernel, knn_rank_kernel, knn_classify_kernel<WP>, knn_partial_kernel<WP>,
knn_merge_kernel) on the hand-built exact rows of tests/knn_exact_cases.py, BIT FOR BIT against a model that saw no kernel output:
knn_ref.exact_similarities (integers: places, signs, exponents) plus knn_ref.select.  For every case and k, `label`, `conf`, `nbr` and
`sim` of wsa_knn_classify_rows (K9), and of wsa_debug_knn_split (K9s) at every slice count of the case, equal the model's as bytes — the
whole path from the unit row through the MFMA chain, the threshold compare and the list insert to the vote, with no tolerance and no
device-side similarity in the expectation.  tests/test_knn_exact_reference.py pins the same model to ml5 itself, to the device's own form
(knn_ref.stream_select, every arm counted) and shows on the CPU that a one-line fault changes a named case.

Every output table carries a guard row in front and behind (test_gpu_knn_split.Rows); the stores are filled by the cases' own sequences
of add calls, and wsa_knn_count's figures are checked with them.

Mutation table: the fault, written into the replay of the device form (knn_ref.stream_select(fault=...)), and the case whose tables it
changes — asserted by tests/test_knn_exact_reference.py on every run (knn_ref.FAULTS, knn_exact_cases.FAULT_CASES); this file holds the
device to the unfaulted tables of the same cases:
  `key[i] > thr[i]` for `>=` in the pass test                    tie_kth (row 129 equals the k-th with the lower rank)
  `ck > s_thr[w]` for `>=` in the merge's pass test              tie_kth (K9s: the equal rows lie in different slices)
  `er > crank` for `er < crank`                                  tie_kth
  `s_thr[q] = ck` whatever pos is                                ins_places (place 0 sets the threshold to 9 / 16: the 7 / 16 of block 2 stays out)
  the shift bound `lane + 1 <= k_eff`                            keff (k_eff = 64: the entry pushed out lands in the next query's first place)
  `cv &&` dropped                                                neg_t1 (the padding rows' +0 beats every negative similarity)
  a NaN similarity keyed as +inf                                 nan_rows
  `key != NEG_INF` dropped (sim written as the key)              nan_rows
  vote key `lane` for `63 - lane`                                vote_tie
  `votes / k` for `votes / k_eff`                                k_gt_n
  knn_within_kernel without the chunk's carry                    same_rows (class 0 straddles rows 63 | 64)
  knn_rank_kernel without s_off                                  families
  the merge reading a slice that holds no rows                   tie_kth (S = 7 on three tiles)
  s_cnt / s_thr not reset on a workgroup's second trip           grid
  `er <= crank`                                                  none: ranks are unique and no row reaches a list twice (asserted: no output changes)
  the threshold not re-read after a block                        none in the output: knn_insert refuses by position; stale_blocks's reread.refuses
                                                                 become insert.refused_stale (asserted)

The same on the device (scratch builds of libwsa.so with one line of csrc/knn.hip changed, nothing committed; this file run once per build
on an MI355X without the NaN cases, where a list that a fault leaves unfilled would have the epilogue read an index nobody wrote; the
cases named are the ones that fail):
  `key[i] > thr[i]` for `>=`                     fmap264, mix23, keff, tie_kth, class63, families, same_rows
  `s_thr[q] = ck` whatever pos is                fmap264, mix53, mix23, mix264, ins_places, keff, stale_blocks, class63, families
  `er > crank` for `er < crank`                  33 of 37, tie_kth among them (every list of tied zeros turns round)
  within: `before` from class_count, no carry    fmap264, ins_places, keff, tie_kth, neg_t1, class63, families, same_rows
  `rank[r] = within[r]`                          22 of 37: every case of more than one class
  vote key `lane`, label `best & 63`             fmap23, fmap23_s0, fmap264_s0 .. s4, mix53, mix23, mix264, keff, neg_40, vote_tie, families,
                                                 classes64, late_class
  NaN keyed as POS_INF                           none of the 37 cases without a NaN (nan_rows and nan_last_slice are its cases: model table)"""
import numpy as np
import pytest

from tests import knn_exact_cases as kc
from tests import knn_ref
from tests.test_gpu_knn_split import Rows, _s
from tests.test_knn_exact_reference import TABLES, clamped, expected
from webspeechanalyzer_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def an():
    a = capi.Analyzer(capi.Config(output_level=13), device=0)
    yield a
    a.close()


def fill(torch, an, store, cls, C, adds):
    """the store, filled by add calls of `adds` rows in sequence"""
    st = an.knn_store(store.shape[1], C, len(store))
    base = 0
    for na in adds:
        f = torch.from_numpy(np.ascontiguousarray(store[base:base + na], np.float64)).cuda()
        c = torch.from_numpy(np.ascontiguousarray(cls[base:base + na], np.int32)).cuda()
        st.add(f.data_ptr(), c.data_ptr(), na, _s(torch))
        torch.cuda.synchronize()
        base += na
    return st


def assert_bytes(want, got, what):
    for t in TABLES:
        assert want[t].tobytes() == got[t].tobytes(), (t,) + tuple(what)


def test_the_tiles_are_the_ones_the_cases_were_placed_by():
    assert capi.KnnStore.tile_info() == (kc.T, kc.QT)


@pytest.mark.parametrize("key", [k for k in kc.CASES if k != "grid"])
def test_case_bit_for_bit(torch, an, key):
    c = kc.CASES[key]
    st = fill(torch, an, c["store"], c["cls"], c["C"], c["adds"])
    if key == "bad_class":
        with pytest.raises(capi.WsaError, match=f"row {kc.BAD_ROW} .*class index outside 0 .. {c['C'] - 1}"):
            st.count()
    else:
        n, per = st.count()
        assert n == len(c["store"]) and per.tolist() == np.bincount(c["cls"], minlength=c["C"]).tolist()
    sim = knn_ref.exact_similarities(c["store"], c["queries"])
    for k in c["ks"]:
        want = expected(sim, clamped(c), c["C"], k)
        rows = Rows(torch, st, c["queries"], k)
        assert_bytes(want, rows.run(), (key, k, "K9"))
        for slices in c["slices"]:
            assert_bytes(want, rows.run(slices), (key, k, slices))
    st.close()


def test_the_query_grid_stride(torch, an):
    """8 n_cu 64 + 1 query rows against three store rows: the launch has 8 n_cu workgroups, so the last row sits in the tile workgroup 0
    takes on its second trip through `qt += gridDim.x`; every row gives the bits of its pattern, the last the bits it gives alone"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    store, cls, queries = kc.grid_case(n_cu)
    q = len(queries)
    assert q == 8 * n_cu * kc.QT + 1
    st = fill(torch, an, store, cls, 1, [3])
    pat = expected(knn_ref.exact_similarities(store, kc.grid_queries(kc.GRID_PERIOD)), cls, 1, 1)
    want = {t: pat[t][np.arange(q) % kc.GRID_PERIOD] for t in TABLES}
    got = Rows(torch, st, queries, 1).run()
    assert_bytes(want, got, ("grid", n_cu))
    alone = Rows(torch, st, queries[-1:], 1).run()
    assert all(alone[t].tobytes() == got[t][-1:].tobytes() for t in TABLES)
    st.close()


def test_an_infinite_store_row_is_a_nan_row(torch, an):
    """a store row holding +-Inf has the unit row (0, ..., NaN, ..., 0): every similarity with it is NaN, keyed below every number, for
    a zero query (flag 0, threshold -inf) as for any other; nothing of it passes a full list of numbers"""
    c = kc.CASES["keff"]
    store = c["store"].copy()
    store[[7, 66], 3] = np.inf, -np.inf
    queries = np.concatenate([c["queries"], np.zeros((1, 53))])
    sim = knn_ref.exact_similarities(c["store"], queries)
    sim[:, [7, 66]] = np.nan
    st = fill(torch, an, store, c["cls"], c["C"], c["adds"])
    for k in (1, 64):
        want = expected(sim, c["cls"], c["C"], k)
        rows = Rows(torch, st, queries, k)
        assert_bytes(want, rows.run(), ("inf", k))
        for slices in (2, 3):
            assert_bytes(want, rows.run(slices), ("inf", k, slices))
    assert not set(want["nbr"][0].tolist()) & {7, 66} and np.isnan(want["sim"][3]).all()
    st.close()

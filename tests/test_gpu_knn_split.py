"""K9s (csrc/knn.hip: knn_partial_kernel + knn_merge_kernel), the split-store KNN a stream step runs, against K9 on the same rows through
capi.debug_knn_split with a forced slice count: label, conf, nbr and sim equal wsa_knn_classify_rows' BIT FOR BIT at every slice count —
a similarity is the same MFMA chain in both kernels and the order (similarity descending, grouped rank ascending) is total, so the split
cannot show.  The ml5 cases are also held to tests/golden/knn_expected.json with test_gpu_knn.py's tolerances, which keeps the split
path pinned to ml5 itself.

Every output buffer carries a guard row in front and behind; a kernel that writes outside its rows shows there."""
import json
import os

import numpy as np
import pytest

from tests import knn_cases, knn_ref
from tests.util import GOLDEN
from webspeechanalyzer_amd import capi, knn

pytestmark = pytest.mark.gpu
FIXTURE = json.load(open(os.path.join(GOLDEN, "knn_expected.json")))
BOUND = 4.0 * FIXTURE["D"]                 # test_gpu_knn.py's bound on |device - exact cosine|
T = knn_cases.T
TABLES = ("label", "conf", "nbr", "sim")

SIZES_N = (1, 63, 64, 65, 128, 129, 200)
SIZES_Q = (1, 15, 16, 17, 64, 65)
SIZES_K = (1, 10, 64)
SIZES_S = (1, 2, 3, 4, 7)


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


def fill(torch, an, store, index, n_classes):
    st = an.knn_store(store.shape[1], n_classes, len(store))
    f = torch.from_numpy(np.ascontiguousarray(store, np.float64)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(index, np.int32)).cuda()
    st.add(f.data_ptr(), c.data_ptr(), len(store), _s(torch))
    torch.cuda.synchronize()
    return st


class Rows:
    """query rows on the device and four guarded output tables: row 0 and row n + 1 of each are guards"""

    def __init__(self, torch, st, queries, k):
        self.torch, self.st, self.n, self.k = torch, st, len(queries), k
        self.f = torch.from_numpy(np.ascontiguousarray(queries, np.float64).reshape(self.n, st.width)).cuda()
        C = st.n_classes
        self.shape = dict(label=(torch.int32, 1), conf=(torch.float64, C), nbr=(torch.int32, k), sim=(torch.float32, k))

    def run(self, slices=None):
        """K9 (slices None) or K9s with `slices` slices; the tables of the n rows, guards checked"""
        torch, n = self.torch, self.n
        buf = {t: torch.full((n + 2, w), -9, dtype=dt, device="cuda") for t, (dt, w) in self.shape.items()}
        ptr = {t: b[1:].data_ptr() for t, b in buf.items()}
        if slices is None:
            self.st.classify_rows(self.f.data_ptr(), n, self.k, ptr["label"], ptr["conf"], ptr["nbr"], ptr["sim"], _s(torch))
        else:
            capi.debug_knn_split(self.st, self.f.data_ptr(), n, self.k, slices, ptr["label"], ptr["conf"], ptr["nbr"], ptr["sim"], _s(torch))
        torch.cuda.synchronize()
        out = {}
        for t, b in buf.items():
            h = b.cpu().numpy()
            assert (h[0] == -9).all() and (h[n + 1] == -9).all(), f"{t}: a guard row was written"
            out[t] = h[1:n + 1] if t != "label" else h[1:n + 1, 0]
        return out


def assert_same_bits(want, got, what):
    for t in TABLES:
        assert want[t].tobytes() == got[t].tobytes(), (t,) + tuple(what)


def slice_rows(n, slices):
    """rows per slice as K9s cuts a store of n rows: runs of ceil(tiles / slices) whole tiles of T rows"""
    tiles = (n + T - 1) // T
    per = max(1, (tiles + slices - 1) // slices) * T
    return [max(0, min(n, (s + 1) * per) - s * per) for s in range(slices)]


@pytest.mark.parametrize("key", list(knn_cases.CASES))
def test_ml5_cases_at_every_slice_count(torch, an, key):
    c = FIXTURE["cases"][key]
    b = knn_cases.build(key, c["seed"])
    classes, index = knn.label_order(b["labels"])
    st = fill(torch, an, b["store"], index, len(classes))
    exact = knn_ref.similarities(b["store"], b["queries"])
    n = len(b["store"])
    for k in b["ks"]:
        rows = Rows(torch, st, b["queries"], k)
        want = rows.run()
        k_eff = min(k, n)
        for slices in (1, 2, 3, 5):
            got = rows.run(slices)
            assert_same_bits(want, got, (key, k, slices))
            # ... and ml5's own figures, as test_gpu_knn.py::test_fixture_case holds K9 to them
            err = float(np.abs(got["sim"][:, :k_eff].astype(np.float64) - exact[np.arange(len(exact))[:, None], got["nbr"][:, :k_eff]]).max())
            assert err <= BOUND, (key, k, slices, err)
            for qi, per_k in enumerate(c["results"]):
                w = per_k[str(k)]
                assert classes[got["label"][qi]] == w["label"], (key, k, slices, qi)
                assert got["conf"][qi, :len(classes)].tolist() == w["conf"], (key, k, slices, qi)
                assert sorted(got["nbr"][qi, :k_eff].tolist()) == sorted(w["nbr"]), (key, k, slices, qi)
                if qi in knn_cases.QUERY_IS.get(key, {}):
                    assert got["nbr"][qi, :k_eff].tolist() == w["nbr"], "equal unit rows: the grouped rank orders them"
            assert (got["nbr"][:, k_eff:] == -1).all() and np.isnan(got["sim"][:, k_eff:]).all()
    st.close()


def test_the_size_grid_reaches_the_slice_edges():
    """what test_sizes_at_the_slice_edges runs includes: a slice with fewer than k rows, more slices than tiles (empty slices), k > N,
    and a last slice of one partial tile"""
    combos = [(n, k, s) for n in SIZES_N for k in SIZES_K for s in SIZES_S]
    assert any(0 < min(r for r in slice_rows(n, s) if r) < k <= n for n, k, s in combos), "a slice holding fewer than k rows"
    assert any(s > (n + T - 1) // T and 0 in slice_rows(n, s) for n, k, s in combos), "more slices than the store has tiles"
    assert any(k > n for n, k, s in combos), "k > N"
    assert any(0 < [r for r in slice_rows(n, s) if r][-1] < T and len([r for r in slice_rows(n, s) if r]) > 1 for n, k, s in combos), "a last slice of one partial tile"
    assert all(sum(slice_rows(n, s)) == n for n, k, s in combos)


@pytest.mark.parametrize("n", SIZES_N)
def test_sizes_at_the_slice_edges(torch, an, n):
    store = knn_cases.draw(53, n, 700 + n)
    index = (knn_cases.mix(np.arange(n), 12, n) % np.uint64(5)).astype(np.int32)
    st = fill(torch, an, store, index, 5)
    for q in SIZES_Q:
        queries = knn_cases.draw(53, q, 800 + q, first=100000)
        for k in SIZES_K:
            rows = Rows(torch, st, queries, k)
            want = rows.run()
            assert (want["label"] >= 0).all() and (want["nbr"][:, :min(k, n)] >= 0).all()
            for slices in SIZES_S:
                assert_same_bits(want, rows.run(slices), (n, q, k, slices))
    st.close()


def test_ties_across_slice_boundaries_are_decided_by_rank(torch, an):
    """one row stored four times, in all four tiles of a 200-row store — so on both sides of every slice boundary at 2, 3, 4 and 7
    slices — under classes that give the LATER copies the LOWER ranks; the query is that row, so the four tie exactly at the top"""
    n = 200
    store = knn_cases.draw(53, n, 901)
    copies = {5: 3, 70: 2, 130: 1, 195: 0}                              # row: class
    for r in copies:
        store[r] = store[5] * (2.0 if r == 130 else 1.0)
        assert knn_cases.same_unit_row(store[r], store[5])
    index = np.full(n, 4, np.int32)
    index[::3] = 3
    for r, c in copies.items():
        index[r] = c
    assert [slice_rows(n, s) for s in (2, 4)] == [[128, 72], [64, 64, 64, 8]]
    st = fill(torch, an, store, index, 5)
    queries = np.stack([store[5], knn_cases.draw(53, 1, 902, first=100000)[0]])
    full = Rows(torch, st, queries, 4).run()
    assert full["nbr"][0].tolist() == [195, 130, 70, 5], "classes 0, 1, 2, 3: the grouped rank ascends with the class"
    assert full["sim"][0].tobytes() == full["sim"][0, :1].tobytes() * 4, "four exact f32 ties"
    ties = 0
    for k in (1, 2, 3, 4, 10):
        rows = Rows(torch, st, queries, k)
        want = rows.run()
        if k < 4:
            assert want["nbr"][0].tolist() == [195, 130, 70, 5][:k]
        # a tie at the k-th place: the k-th and the (k + 1)-th best of a query, read from a run at k + 1, are the same f32 bits
        longer = Rows(torch, st, queries, k + 1).run()["sim"]
        ties += int((longer[:, k - 1].view(np.uint32) == longer[:, k].view(np.uint32)).sum())
        for slices in SIZES_S:
            assert_same_bits(want, rows.run(slices), (k, slices))
    assert ties >= 3, ties                                             # k = 1, 2, 3 of the first query
    st.close()


def test_nan_similarities_follow_the_device_rule(torch, an):
    """a zero row and a non-finite row in the store (in different slices) and among the queries: NaN is lower than every number and ranks
    decide among NaNs, exactly as K9 does it (test_gpu_knn.py::test_nan_similarities_follow_the_device_rule)"""
    n = 130
    store = knn_cases.draw(53, n, 911)
    store[2] = 0.0
    store[100, 7] = np.inf
    store[129] = 0.0
    queries = knn_cases.draw(53, 4, 912, first=100000)
    queries[1] = 0.0
    queries[2, 3] = np.nan
    index = (np.arange(n) % 3).astype(np.int32)
    st = fill(torch, an, store, index, 3)
    for k in (1, 5, 64):
        rows = Rows(torch, st, queries, k)
        want = rows.run()
        for slices in (1, 2, 3, 5):
            assert_same_bits(want, rows.run(slices), (k, slices))
    big = Rows(torch, st, queries, 64).run(3)
    assert np.isfinite(big["sim"][0]).all() and np.isnan(big["sim"][1]).all() and np.isnan(big["sim"][2]).all()
    ranks = np.lexsort((np.arange(n), index))                          # insertion indices in grouped-rank order
    assert big["nbr"][1].tolist() == ranks[:64].tolist(), "a zero query takes the rows in rank order"
    all_k = Rows(torch, st, queries[:1], 64)
    assert not set(all_k.run(2)["nbr"][0].tolist()) & {2, 100, 129}, "NaN rows come after 127 finite ones"
    st.close()


def test_no_queries_writes_nothing(torch, an):
    """with zero rows the debug entry still launches both kernels (one query tile, the forced slices, a row count of 0) — what a stream
    step that produced no row runs; nothing is written: the guard rows around the empty tables stand"""
    st = fill(torch, an, knn_cases.draw(53, 70, 1), np.zeros(70, np.int32), 1)
    for slices in (1, 2, 5):
        got = Rows(torch, st, np.zeros((0, 53)), 3).run(slices)
        assert all(len(got[t]) == 0 for t in TABLES)
    st.close()


def test_refusals_and_the_rules_own_choice(torch, an):
    st = an.knn_store(53, 2, 300)
    one = torch.ones((1, 53), dtype=torch.float64, device="cuda")
    with pytest.raises(capi.WsaError, match="no examples"):
        capi.debug_knn_split(st, one.data_ptr(), 1, 3, 2, None, None, None, None, _s(torch))
    f = torch.from_numpy(knn_cases.draw(53, 300, 5)).cuda()
    c = torch.zeros(300, dtype=torch.int32, device="cuda")
    st.add(f.data_ptr(), c.data_ptr(), 300, _s(torch))
    for k in (0, 65):
        with pytest.raises(capi.WsaError, match="k must be 1 .. 64"):
            capi.debug_knn_split(st, one.data_ptr(), 1, k, 2, None, None, None, None, _s(torch))
    with pytest.raises(capi.WsaError, match="at most 256 slices"):
        capi.debug_knn_split(st, one.data_ptr(), 1, 3, 257, None, None, None, None, _s(torch))
    # slices = 0 is the rule's choice (300 rows are 5 tiles, no slice shorter than 4: two slices); whatever it is, the bits are K9's
    rows = Rows(torch, st, knn_cases.draw(53, 3, 6, first=100000), 3)
    assert_same_bits(rows.run(), rows.run(0), ("rule",))
    st.close()

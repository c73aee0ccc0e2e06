"""K9 (csrc/knn.hip, specification KN-1) on the GPU: the app's ml5 KNN classifier.

Two kinds of check, as the numerics contract of DESIGN.md "K9" has two halves:
  * the device's similarities are f32 with an order of their own, so they are held to a TOLERANCE against the exact cosines of
    tests/knn_ref.py: BOUND = 4 x D, D = max |exact - tfjs| over the fixture's similarities (tests/golden/knn_expected.json, 1.67e-7).
    Why 4, as K7's bound: the device and tfjs make the same kinds of rounding (f32 unit rows, f32 products and sums) and the device only
    makes more of them in a row — its sums are chains of up to 17 fused multiply-adds per accumulator pair where tfjs rounds a
    double-precision block sum once per 48 features — so its distance from the exact figure is a small multiple of tfjs's own; an error
    of another kind (a wrong operand, a dropped k step, a row normalised twice) is orders of magnitude larger.  4 x D = 6.7e-7 is also 15
    times below the fixture's margin of 1e-5, so a device within the bound selects what ml5 selects.
  * everything after the similarities is EXACT: against the fixture (labels, confidences, neighbour sets: its margin condition makes
    that legitimate), and, with no margin at all, against knn_ref.select applied to the device's OWN similarities (the crowded case,
    the shape sweep, the NaN case).

The device's full similarity matrix is read back through stores of at most 64 rows with k = 64 (all their similarities come back): a
similarity is a function of its (query row, stored row) pair alone, which those tests thereby also check.

Measured on an MI355X (printed by the last test; DESIGN.md "K9"): max |device - exact cosine| = 3.869e-07 at 53 features, 1.822e-07 at 23,
3.603e-07 at 264, against the bound 4 D = 6.692e-07; every exact comparison held."""
import json
import os

import numpy as np
import pytest

from tests import knn_cases, knn_ref
from tests import wide_cases as wc
from tests.util import GOLDEN
from webspeechanalyzer_amd import capi, knn

pytestmark = pytest.mark.gpu
FIXTURE = json.load(open(os.path.join(GOLDEN, "knn_expected.json")))
BOUND = 4.0 * FIXTURE["D"]
MAX_K = 64
SEEN = {}                                  # largest |device - exact| per width, printed by the last test


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


def fill(torch, an, store, index, n_classes=64, capacity=None):
    st = an.knn_store(store.shape[1], n_classes, capacity or len(store))
    add(torch, st, store, index)
    return st


def add(torch, st, rows, index):
    f = torch.from_numpy(np.ascontiguousarray(rows, np.float64)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(index, np.int32)).cuda()
    st.add(f.data_ptr(), c.data_ptr(), len(rows), _s(torch))
    torch.cuda.synchronize()


def classify(torch, st, queries, k):
    """the four tables of wsa_knn_classify_rows; buffers start as sentinels, so an entry the kernel leaves alone shows"""
    n = len(queries)
    f = torch.from_numpy(np.ascontiguousarray(queries, np.float64)).cuda()
    label = torch.full((max(n, 1),), -9, dtype=torch.int32, device="cuda")
    conf = torch.full((max(n, 1), st.n_classes), -9.0, dtype=torch.float64, device="cuda")
    nbr = torch.full((max(n, 1), k), -9, dtype=torch.int32, device="cuda")
    sim = torch.full((max(n, 1), k), -9.0, dtype=torch.float32, device="cuda")
    st.classify_rows(f.data_ptr(), n, k, label.data_ptr(), conf.data_ptr(), nbr.data_ptr(), sim.data_ptr(), _s(torch))
    torch.cuda.synchronize()
    return dict(label=label.cpu().numpy(), conf=conf.cpu().numpy(), nbr=nbr.cpu().numpy(), sim=sim.cpu().numpy())


def device_sims(torch, an, store, queries):
    """the device's own similarity of every (query, stored row) pair, [q, n] f32: chunks of 64 rows as stores of their own, k = 64"""
    out = np.zeros((len(queries), len(store)), np.float32)
    for r0 in range(0, len(store), MAX_K):
        chunk = store[r0:r0 + MAX_K]
        st = fill(torch, an, chunk, np.zeros(len(chunk), np.int32), 1)
        got = classify(torch, st, queries, len(chunk))
        st.close()
        assert (np.sort(got["nbr"], axis=1) == np.arange(len(chunk))).all()
        np.put_along_axis(out[:, r0:r0 + len(chunk)], got["nbr"].astype(np.int64), got["sim"], axis=1)
    return out


def check_exact(got, sims, index, n_classes, k, what):
    """the device's tables against the restatement's selection on the device's own similarities: bit for bit, order included"""
    want = knn_ref.select(sims, index, n_classes, k)
    k_eff = want["nbr"].shape[1]
    assert np.array_equal(got["nbr"][:, :k_eff], want["nbr"]), what
    assert (got["nbr"][:, k_eff:] == -1).all() and np.isnan(got["sim"][:, k_eff:]).all(), what
    picked = np.take_along_axis(sims, want["nbr"], axis=1)
    assert got["sim"][:, :k_eff].tobytes() == picked.astype(np.float32).tobytes(), what
    assert np.array_equal(got["conf"][:, :n_classes], want["conf"]) and np.array_equal(got["label"], want["label"]), what
    return want


def note(width, got, exact, k_eff):
    rows = np.arange(len(exact))[:, None]
    err = float(np.abs(got["sim"][:, :k_eff].astype(np.float64) - exact[rows, got["nbr"][:, :k_eff]]).max())
    SEEN[width] = max(SEEN.get(width, 0.0), err)
    return err


def test_tile_sizes_are_the_ones_the_cases_were_placed_by():
    assert capi.KnnStore.tile_info() == (knn_cases.T, knn_cases.QT)


@pytest.mark.parametrize("key", list(knn_cases.CASES))
def test_fixture_case(torch, an, key):
    """labels, confidences and neighbour sets are ml5's; the similarities are within BOUND of the exact cosines"""
    c = FIXTURE["cases"][key]
    b = knn_cases.build(key, c["seed"])
    width = knn_cases.CASES[key]["width"]
    classes, index = knn.label_order(b["labels"])
    assert classes == c["class_names"]
    st = fill(torch, an, b["store"], index, len(classes))
    n, per = st.count()
    assert n == len(b["store"]) and per.tolist() == np.bincount(index, minlength=len(classes)).tolist()
    exact = knn_ref.similarities(b["store"], b["queries"])
    for k in b["ks"]:
        got = classify(torch, st, b["queries"], k)
        k_eff = min(k, n)
        err = note(width, got, exact, k_eff)
        print(f"{key} k={k}: |device - exact| <= {err:.3e} (bound {BOUND:.3e})")
        assert err <= BOUND
        for qi, per_k in enumerate(c["results"]):
            want = per_k[str(k)]
            assert classes[got["label"][qi]] == want["label"], (key, k, qi)
            assert got["conf"][qi].tolist() == want["conf"], (key, k, qi)
            assert sorted(got["nbr"][qi, :k_eff].tolist()) == sorted(want["nbr"]), (key, k, qi)
            if qi in knn_cases.QUERY_IS.get(key, {}):
                assert got["nbr"][qi, :k_eff].tolist() == want["nbr"], "equal unit rows: the grouped rank orders them"
        assert (got["nbr"][:, k_eff:] == -1).all() and np.isnan(got["sim"][:, k_eff:]).all()
    st.close()


def crowded(n=3000, q=70, centres=5):
    """rows drawn tightly round a few centres (1e-7 of a feature's range apart): most of a centre's rows share a handful of f32
    similarities with any query, so the k-th place is decided among hundreds of near and exact ties"""
    lo, hi = knn_cases.ranges(53)
    cen = knn_cases.draw(53, centres, 77, first=300000)
    which = (knn_cases.mix(np.arange(n), 9, 77) % np.uint64(centres)).astype(int)
    jit = knn_cases.mix(np.arange(n)[:, None], np.arange(53)[None, :], 78).astype(np.float64) / 4294967296.0 - 0.5
    store = cen[which] + 1e-7 * jit * (hi - lo)
    index = (knn_cases.mix(np.arange(n), 10, 77) % np.uint64(7)).astype(np.int32)
    queries = knn_cases.draw(53, q, 79, first=400000)
    queries[:centres] = cen                                            # queries on the centres themselves, too
    return store, index, queries


def test_crowded_selection_equals_the_restatement_on_the_devices_own_similarities(torch, an):
    store, index, queries = crowded()
    sims = device_sims(torch, an, store, queries)
    st = fill(torch, an, store, index, 7)
    near = 0
    for k in (1, 10, 64):
        got = classify(torch, st, queries, k)
        check_exact(got, sims, index, 7, k, f"k={k}")
        again = classify(torch, st, queries, k)
        assert all(got[t].tobytes() == again[t].tobytes() for t in got), "two runs, the same bits"
        kth = got["sim"][:, k - 1:k]
        near = max(near, int((np.abs(sims - kth) <= 1e-6).sum(axis=1).max()))
    assert near >= 200, near                                           # the case is still crowded
    err = note(53, got, knn_ref.similarities(store, queries), 64)
    assert err <= BOUND
    st.close()


def test_shapes_at_the_tile_edges(torch, an):
    """store sizes 1, 2, T - 1, T, T + 1, 2T + 1 x query counts 1, QT - 1, QT + 1 at width 53; the other widths and class counts at
    (T + 1, QT + 1)"""
    T, QT = knn_cases.T, knn_cases.QT
    combos = [(53, n, q, 2) for n in (1, 2, T - 1, T, T + 1, 2 * T + 1) for q in (1, QT - 1, QT + 1)]
    combos += [(23, T + 1, QT + 1, 1), (264, T + 1, QT + 1, 64), (53, T + 1, QT + 1, 64), (53, T + 1, QT + 1, 1)]
    for width, n, q, classes in combos:
        store = knn_cases.draw(width, n, 500 + n)
        queries = knn_cases.draw(width, q, 600 + q, first=100000)
        index = (knn_cases.mix(np.arange(n), 11, n) % np.uint64(classes)).astype(np.int32)
        sims = device_sims(torch, an, store, queries)
        st = fill(torch, an, store, index, classes)
        for k in (1, 10) + ((64,) if n > T and q > QT else ()):
            got = classify(torch, st, queries, k)
            check_exact(got, sims, index, classes, k, (width, n, q, classes, k))
        assert note(width, got, knn_ref.similarities(store, queries), min(10, n)) <= BOUND
        st.close()


def test_no_queries_writes_nothing(torch, an):
    st = fill(torch, an, knn_cases.draw(53, 5, 1), np.zeros(5, np.int32), 1)
    got = classify(torch, st, np.zeros((0, 53)), 3)
    assert got["label"].tolist() == [-9] and (got["conf"] == -9).all() and (got["nbr"] == -9).all() and (got["sim"] == -9).all()
    st.close()


def test_adding_after_classifying_equals_a_store_filled_in_one_go(torch, an):
    b = knn_cases.build("main53", 4242)
    index = np.array([(3, 1, 0, 2, 1)[i % 5] if i >= 40 else (3, 1)[i % 2] for i in range(len(b["store"]))], np.int32)     # classes 0 and 2 arrive later: every rank moves
    st = fill(torch, an, b["store"][:40], index[:40], 4, capacity=len(index))
    first = classify(torch, st, b["queries"], 10)
    assert first["nbr"].max() < 40
    add(torch, st, b["store"][40:], index[40:])
    second = classify(torch, st, b["queries"], 10)
    fresh = fill(torch, an, b["store"], index, 4)
    want = classify(torch, fresh, b["queries"], 10)
    assert all(second[t].tobytes() == want[t].tobytes() for t in want)
    assert st.count()[1].tolist() == np.bincount(index, minlength=4).tolist()
    with pytest.raises(capi.WsaError, match="no room for 1 more"):
        add(torch, st, b["store"][:1], index[:1])
    st.close(); fresh.close()


def test_nan_similarities_follow_the_device_rule(torch, an):
    """a zero row has no direction: its similarities are NaN, lower than every number, ranks decide among them (not compared with ml5)"""
    store = knn_cases.draw(53, 6, 31)
    store[2] = 0.0
    queries = knn_cases.draw(53, 3, 32, first=100000)
    queries[1] = 0.0
    index = np.array([1, 0, 1, 0, 1, 0], np.int32)
    sims = device_sims(torch, an, store, queries)
    assert np.isnan(sims[:, 2]).all() and np.isnan(sims[1]).all() and np.isfinite(np.delete(sims[[0, 2]], 2, axis=1)).all()
    st = fill(torch, an, store, index, 2)
    for k in (1, 5, 6):
        got = classify(torch, st, queries, k)
        want = check_exact(got, sims, index, 2, k, f"k={k}")
        assert 2 not in want["nbr"][0, :5]                              # the zero row comes last ...
    assert got["nbr"][0, 5] == 2 and np.isnan(got["sim"][0, 5])
    assert got["nbr"][1].tolist() == [1, 3, 5, 0, 2, 4]                 # ... and a zero query takes the rows in rank order
    st.close()


def test_refusals(torch, an):
    with pytest.raises(capi.WsaError, match="63 inputs|takes 63"):
        an.knn_store(63, 4, 10)
    with pytest.raises(capi.WsaError, match="1 .. 64 classes, got 65"):
        an.knn_store(53, 65, 10)
    st = an.knn_store(53, 2, 10)
    with pytest.raises(capi.WsaError, match="no examples"):
        classify(torch, st, np.ones((1, 53)), 3)
    add(torch, st, np.ones((2, 53)), np.array([0, 5], np.int32))
    with pytest.raises(capi.WsaError, match="row 1 .*class index outside 0 .. 1"):
        st.count()
    for k in (0, 65):
        with pytest.raises(capi.WsaError, match="k must be 1 .. 64"):
            classify(torch, st, np.ones((1, 53)), k)
    st.close()


# ---- wsa_batch_knn
def _batch_rows(torch, b, level):
    if level == 11:
        return b.utterance(_s(torch))["feat"]
    return b.rows(_s(torch))["feat"]


def _check_batch(torch, an_l, b, level, width, k=10):
    feat = _batch_rows(torch, b, level)
    n = len(feat)
    assert n > 0
    marked = feat[:, 23] != 0 if level == 12 else np.zeros(n, bool)
    # a store of the wide cases' recipe, scaled onto the rows at hand, and a few of the batch's own rows
    rows, lab = wc.cluster_rows(90, width, 3, 19)
    live = feat[~marked][:, :width]
    m = min(5, len(live))
    store = np.concatenate([np.abs(rows) * (np.abs(live).max(axis=0) + 1.0) / 50.0, live[:m]])
    index = np.concatenate([lab, np.zeros(m, np.int32)]).astype(np.int32)
    st = fill(torch, an_l, store, index, 3)
    b.knn(st, k, _s(torch))
    got = b.knn_classes(_s(torch))
    assert got["label"].shape == (n,) and got["k_eff"] == k
    dense = classify(torch, st, np.ascontiguousarray(feat[:, :width]), k)
    for t in ("label", "conf", "nbr", "sim"):
        assert got[t][~marked].tobytes() == dense[t][~marked].tobytes(), t
    assert (got["label"][marked] == -1).all() and np.isnan(got["conf"][marked]).all() and np.isnan(got["sim"][marked]).all() and (got["nbr"][marked] == -1).all()
    assert (got["label"][~marked] >= 0).all() and np.isfinite(got["sim"][~marked]).all()
    assert got["nbr"][~marked][:m, 0].tolist() == list(range(90, 90 + m))           # a stored row finds itself
    return st, n, int(marked.sum())


@pytest.mark.parametrize("level", [5, 13])
def test_batch_knn_at_levels_5_and_13(torch, level):
    from webspeechanalyzer_amd.synth import synth_clips
    fs, ns = 16000, 48000
    pcm = synth_clips(8, ns, fs=fs, seed=3, device="cuda")
    an_l = capi.Analyzer(capi.Config(output_level=level), device=0)
    b = an_l.batch([ns] * 8, fs)
    b.run(pcm.data_ptr(), pcm.stride(0), _s(torch))
    st, n, _ = _check_batch(torch, an_l, b, level, 53)
    print(f"level {level}: {n} rows")
    st.close(); b.close(); an_l.close()


def test_batch_knn_at_level_11_and_its_refusals(torch):
    from webspeechanalyzer_amd.synth import synth_clips
    fs, ns = 16000, 32000
    pcm = synth_clips(3, ns, fs=fs, seed=3, device="cuda")
    an11 = capi.Analyzer(capi.Config(output_level=11), device=0)
    b = an11.batch([ns] * 3, fs)
    b.run(pcm.data_ptr(), pcm.stride(0), _s(torch))
    with pytest.raises(capi.WsaError, match="no wsa_batch_knn on this batch yet"):
        b.knn_result(_s(torch))
    st, n, _ = _check_batch(torch, an11, b, 11, 264)
    st53, st23 = an11.knn_store(53, 2, 4), an11.knn_store(23, 2, 4)
    with pytest.raises(capi.WsaError, match=r"output_level 5 .*not 11.*rows of 53 features.*output_level 11 have 264"):
        b.knn(st53, 10, _s(torch))
    with pytest.raises(capi.WsaError, match=r"output_level 12 .*not 11.*rows of 23 features"):
        b.knn(st23, 10, _s(torch))
    with pytest.raises(capi.WsaError, match="k must be 1 .. 64, got 65"):
        b.knn(st, 65, _s(torch))
    other = capi.Analyzer(capi.Config(output_level=11), device=0)
    foreign = fill(torch, other, np.ones((2, 264)), np.zeros(2, np.int32), 1)
    with pytest.raises(capi.WsaError, match="another context"):
        b.knn(foreign, 1, _s(torch))
    foreign.close(); other.close(); st53.close(); st23.close(); st.close(); b.close(); an11.close()
    an4 = capi.Analyzer(capi.Config(output_level=4), device=0)
    b = an4.batch([ns] * 3, fs)
    st53 = an4.knn_store(53, 2, 4)
    with pytest.raises(capi.WsaError, match=r"not 4: the KNN store holds rows of 53 features$"):
        b.knn(st53, 10, _s(torch))
    st53.close(); b.close(); an4.close()


def test_batch_knn_at_level_12_with_a_thrown_row(torch):
    """the captured spectrum of the level-12 throw fixture through the back end: the marked row gets label -1 and NaN"""
    cap = np.load(os.path.join(GOLDEN, "gen", "captured_l12_throw.npy"))
    cfg = capi.Config(output_level=12, N_mel_bins=int(cap.shape[1]), window_step=15.0, window_width=15.0, pause_length=100.0, min_seg_length=100.0,
                      auto_noise_gate=0, voiced_max_dB=140.0, voiced_min_dB=10.0)
    an12 = capi.Analyzer(cfg, device=0)
    g = an12.geometry(16000)
    b = an12.batch([g["win"] + (len(cap) - 1) * g["hop"]], 16000)
    d = torch.from_numpy(np.ascontiguousarray(cap).view(np.int32)).cuda()
    b.run_backend(d.data_ptr(), _s(torch))
    st, n, marked = _check_batch(torch, an12, b, 12, 23, k=3)
    assert marked >= 1
    print(f"level 12, the throw clip: {n} rows, {marked} marked")
    st.close(); b.close(); an12.close()


def test_graph_capture_of_run_and_knn(torch):
    from webspeechanalyzer_amd.synth import synth_clips
    fs, n, ns = 16000, 8, 48000
    a = synth_clips(n, ns, fs=fs, seed=31, device="cuda")
    c = synth_clips(n, ns, fs=fs, seed=32, device="cuda")
    an13 = capi.Analyzer(capi.Config(output_level=13), device=0)
    rows, lab = wc.cluster_rows(150, 53, 4, 23)
    st = fill(torch, an13, np.abs(rows), lab, 4)
    plain = an13.batch([ns] * n, fs)
    refs = []
    for x in (a, c):
        plain.run(x.data_ptr(), x.stride(0), _s(torch))
        plain.knn(st, 10, _s(torch))
        refs.append(plain.knn_classes(_s(torch)))
    assert len(refs[0]["label"]) > 0 and refs[0]["sim"].tobytes() != refs[1]["sim"].tobytes()
    b = an13.batch([ns] * n, fs)
    b.enable_timing(False)
    buf = a.clone()
    b.run(buf.data_ptr(), buf.stride(0), _s(torch))
    b.knn(st, 10, _s(torch))                            # the first call allocates; the captured one does not
    b.knn_classes(_s(torch))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            b.run(buf.data_ptr(), buf.stride(0), side.cuda_stream)
            b.knn(st, 10, side.cuda_stream)
        for x, ref in ((c, refs[1]), (a, refs[0]), (c, refs[1])):
            buf.copy_(x)
            g.replay()
            side.synchronize()
            got = b.knn_classes(side.cuda_stream)
            for t in ("label", "conf", "nbr", "sim"):
                assert got[t].tobytes() == ref[t].tobytes(), t
    plain.close(); b.close(); st.close(); an13.close()


# ---- the Python host (webspeechanalyzer_amd/knn.py)
def test_host_knn_renumbers_when_a_label_sorts_in_front(torch, an):
    c = FIXTURE["cases"]["keyorder_num"]
    b = knn_cases.build("keyorder_num", c["seed"])
    h = knn.Knn(an, 53, capacity=len(b["store"]))
    h.add(b["store"][:1], b["labels"][:1])              # 10 alone is class 0 ...
    assert h.classes == ["10"]
    h.add(b["store"][1:], b["labels"][1:])              # ... until 7, 2 and 3 arrive
    assert h.classes == c["class_names"] and h.count() == (40, {"2": 10, "3": 10, "7": 10, "10": 10})
    for k in b["ks"]:
        got = h.classify(b["queries"], k)
        assert got["label"] == [r[str(k)]["label"] for r in c["results"]]
        assert got["conf"].tolist() == [r[str(k)]["conf"] for r in c["results"]]
    h.close()


@pytest.mark.parametrize("variant", list(knn_cases.EVAL_VARIANTS))
def test_host_evaluate_gives_the_apps_figure(torch, an, variant):
    e = FIXTURE["evals"][variant]
    rows, labels = knn_cases.eval_db(e["seed"])
    assert knn.evaluate(rows, labels, e["classes"], k=knn_cases.EVAL_K, analyzer=an) == (e["correct"], e["all"])


def test_zz_report_the_device_maxima():
    """prints what the tests above measured (the figures DESIGN.md "K9" records)"""
    for width, err in sorted(SEEN.items()):
        print(f"width {width}: max |device - exact cosine| = {err:.3e}  (bound 4 D = {BOUND:.3e})")
    assert all(err <= BOUND for err in SEEN.values())

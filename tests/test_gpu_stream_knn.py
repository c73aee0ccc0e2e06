"""The KNN store inside the stream step (wsa_stream_set_knn / wsa_stream_knn_classes): K9s on every step's rows and, at level 13, the fold
of specification KN-2 with one accumulator per stream carried on the device.  A signal fed step by step gives exactly what
wsa_batch_knn + wsa_batch_knn_fold give for the same signal as one clip — label, conf, nbr, sim, callbacks and the per-stream sums, bit for
bit — and the callbacks equal tests/classify_ref.fold_rows fed the stream's own f64 confidences with the class indices as the legend.
START resets a stream's accumulator, idle steps leave it alone; attaching a store changes no row and leaves an attached model alone.

The store holds the level-13 rows of OTHER synthetic clips, labelled row index mod 4, and k = 10: confidences are multiples of 1 / 10
over four classes, so exact ties and exact zeros are everywhere (the fold's `if(!acc[label])` overwrite and the stable order of
classifyMultiple are at work in most callbacks).  The synthetic run (clip seed 23, store seed 57) is asserted to contain one-syllable
callbacks, rows with tied top confidences and zero confidences — on an MI355X: 4, 13 and 13; the one-stream excerpt, whose rows lie far
from every stored row, contains none and is held to the batch and the restatement only."""
import os

import numpy as np
import pytest

from tests import classify_ref
from tests.test_gpu_stream_classify import GOLD, MODELS, _feed, _signals, _stream

pytestmark = pytest.mark.gpu
K, CLASSES = 10, 4
LEGEND = list(range(CLASSES))
ROW_TABLES = ("label", "conf", "nbr", "sim")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _store(torch, an, cfg_fs, seed=57, n_clips=128, extra=0):
    """(KnnStore, rows, classes) from the level-13 rows of `n_clips` synthetic clips of another seed, labelled row index mod 4; `extra`
    rows of capacity stay free"""
    from webspeechanalyzer_amd.synth import synth_clips
    fs = cfg_fs
    pcm = synth_clips(n_clips, 3 * fs, fs=fs, seed=seed, device="cuda")
    b = an.batch([pcm.shape[1]] * n_clips, fs)
    b.run(pcm.data_ptr(), pcm.stride(0), _stream(torch))
    rows = b.rows(_stream(torch))["feat"].copy()
    b.close()
    assert 320 <= len(rows) <= 2000, len(rows)      # at least five store tiles, so that K9s cuts the store into more than one slice
    index = (np.arange(len(rows)) % CLASSES).astype(np.int32)
    st = an.knn_store(53, CLASSES, len(rows) + extra)
    _add(torch, st, rows, index)
    return st, rows, index


def _add(torch, st, rows, index):
    f = torch.from_numpy(np.ascontiguousarray(rows, np.float64)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(index, np.int32)).cuda()
    st.add(f.data_ptr(), c.data_ptr(), len(rows), _stream(torch))
    torch.cuda.synchronize()


def _run(torch, an, pcm, fs, F, graph, host_in, store=None, ctl_of=None, before_step=None, model=None):
    """Steps over pcm [n, ns]; returns (per step (rows, knn tables or None, classes or None), samples used).  before_step(k, streams) may
    attach or detach; ctl_of(k, nsteps) -> control bytes (default: START on the first step, STOP on the last)."""
    import webspeechanalyzer_amd as wsa
    n, ns = pcm.shape
    st = an.streams(n, fs, frames_per_step=F)
    st.enable_graph(graph)
    sps = st.samples_per_step
    nsteps = ns // sps
    state = dict(knn=False, model=False)
    if store is not None:
        st.set_knn(store, K); state["knn"] = True
    if model is not None:
        st.set_model(model); state["model"] = True
    buf = torch.zeros((n, sps), device="cuda", dtype=torch.float32)
    out = []
    for k in range(nsteps):
        if before_step is not None:
            before_step(k, st, state)
        if ctl_of is not None:
            ctl = ctl_of(k, nsteps)
        else:
            ctl = np.full(n, wsa.ACTIVE, np.uint8)
            if k == 0:
                ctl |= wsa.START
            if k == nsteps - 1:
                ctl |= wsa.STOP
        _feed(torch, wsa, st, pcm, k, sps, ctl, host_in, buf)
        r = st.collect(_stream(torch))
        out.append((r, st.knn_classes() if state["knn"] else None, st.classes() if state["model"] else None))
    st.close()
    return out, nsteps * sps


def _per_stream(steps, n):
    """Per stream: rows (meta, feat), the four KNN tables, callbacks [(si, rows, label, conf)] in order; and stream_conf after the last step"""
    acc = [dict(meta=[], feat=[], cbs=[], **{t: [] for t in ROW_TABLES}) for _ in range(n)]
    conf = None
    for r, c, _ in steps:
        assert len(c["label"]) == len(r["meta"])
        for i, m in enumerate(r["meta"]):
            a = acc[int(m[0])]
            a["meta"].append(m); a["feat"].append(r["feat"][i])
            for t in ROW_TABLES:
                a[t].append(c[t][i])
        if c["cb"] is not None:
            for q, e in enumerate(c["cb"]):
                assert np.array_equal(r["meta"][e[2]][:2], [e[0], e[1]])
                acc[int(e[0])]["cbs"].append((int(e[1]), int(e[3]), int(c["cb_label"][q]), float(c["cb_conf"][q])))
            conf = c["stream_conf"]
    for a in acc:
        a["feat"] = np.array(a["feat"]).reshape(-1, 53)
        a["label"] = np.array(a["label"], np.int32)
        a["conf"] = np.array(a["conf"], np.float64).reshape(-1, CLASSES)
        a["nbr"] = np.array(a["nbr"], np.int32).reshape(-1, K)
        a["sim"] = np.array(a["sim"], np.float32).reshape(-1, K)
    return acc, conf


def _batch(torch, an, pcm, fs, used, store, fold=True):
    b = an.batch([used] * pcm.shape[0], fs)
    x = pcm[:, :used].contiguous()
    b.run(x.data_ptr(), x.stride(0), _stream(torch))
    b.knn(store, K, _stream(torch))
    if fold:
        b.knn_fold(_stream(torch))
    got = b.knn_classes(_stream(torch))
    if fold:
        got.update(b.knn_fold_classes(_stream(torch)))
    rows = b.rows(_stream(torch))
    b.close()
    return got, rows


def _check_equal_to_batch(got, conf, want, rows, n, fold=True):
    ro = rows["row_off"]
    for s in range(n):
        a, b = int(ro[s]), int(ro[s + 1])
        g = got[s]
        assert len(g["meta"]) == b - a, f"stream {s}"
        if b == a:
            continue
        assert np.array_equal(np.array(g["meta"])[:, 1:], rows["meta"][a:b, 1:]), f"stream {s}"
        for t in ROW_TABLES:
            assert g[t].tobytes() == want[t][a:b].tobytes(), (t, s)            # bit for bit
        if not fold:
            continue
        wcb = [(int(e[1]), int(e[3]), int(want["cb_label"][k]), float(want["cb_conf"][k])) for k, e in enumerate(want["cb"]) if e[0] == s]
        assert g["cbs"] == wcb, f"stream {s}"
        assert np.array_equal(conf[s], want["clip_conf"][s]), f"stream {s}"


@pytest.mark.parametrize("F,graph,host_in", [(1, True, True), (7, True, False), (1, False, False), (7, False, True)])
@pytest.mark.parametrize("which", ["config1_excerpt", "synthetic"])
def test_stream_knn_equals_the_batch_and_the_restatement(torch, which, F, graph, host_in):
    import webspeechanalyzer_amd as wsa
    cfg, pcm, fs = _signals(torch, which)
    an = wsa.Analyzer(cfg)
    store, _, _ = _store(torch, an, fs)
    steps, used = _run(torch, an, pcm, fs, F, graph, host_in, store=store)
    n = pcm.shape[0]
    got, conf = _per_stream(steps, n)
    want, rows = _batch(torch, an, pcm, fs, used, store)
    assert len(want["cb"]) > 0 and want["k_eff"] == K and steps[0][1]["slices"] >= 2
    _check_equal_to_batch(got, conf, want, rows, n)
    # KN-2, bit-exact against the float64 restatement fed the stream's own confidences and the class-index legend
    one_syllable = tied_top = zero_conf = 0
    for s in range(n):
        if not len(got[s]["meta"]):
            continue
        cbs, accs = classify_ref.fold_rows(np.array(got[s]["meta"]), got[s]["conf"], LEGEND, cfg["window_step"] / 1e3)
        assert [(si, nr, lab, c) for (_, si, _, nr, lab, c) in cbs] == got[s]["cbs"], f"stream {s}"
        acc = accs[int(got[s]["meta"][0][0])]
        assert [acc.get(c, 0.0) for c in LEGEND] == conf[s].tolist(), f"stream {s}"
        one_syllable += sum(1 for c in got[s]["cbs"] if c[1] == 1)
        top = np.sort(got[s]["conf"], axis=1)
        tied_top += int((top[:, -1] == top[:, -2]).sum())
        zero_conf += int((got[s]["conf"] == 0).sum())
    print(f"{which} F={F}: {one_syllable} one-syllable callbacks, {tied_top} rows with tied top confidences, {zero_conf} zero confidences")
    if which == "synthetic":
        assert one_syllable >= 1 and tied_top >= 1 and zero_conf >= 1
    store.close(); an.close()


def test_restart_idle_and_stop_then_start(torch):
    """Four streams: 0 plays through; 1 idles, then STARTs mid-run; 2 STOPs, idles and STARTs again on the rest of its signal; 3 gets a
    START mid-run without a STOP.  Each stream's accumulator equals a fresh batch of only its post-START signal; idle steps keep it."""
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs, F = 16000, 5
    pcm = synth_clips(4, 6 * fs, fs=fs, seed=41, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=13))
    store, _, _ = _store(torch, an, fs)
    sps = an.geometry(fs)["hop"] * F
    nsteps = pcm.shape[1] // sps
    k1, k2a, k2b, k3 = nsteps // 3, nsteps // 3, nsteps // 2, nsteps // 2

    def ctl_of(k, ns):
        c = np.zeros(4, np.uint8)
        c[0] = wsa.ACTIVE | (wsa.START if k == 0 else 0) | (wsa.STOP if k == ns - 1 else 0)
        if k >= k1:
            c[1] = wsa.ACTIVE | (wsa.START if k == k1 else 0) | (wsa.STOP if k == ns - 1 else 0)
        if k < k2a:
            c[2] = wsa.ACTIVE | (wsa.START if k == 0 else 0) | (wsa.STOP if k == k2a - 1 else 0)
        elif k >= k2b:
            c[2] = wsa.ACTIVE | (wsa.START if k == k2b else 0) | (wsa.STOP if k == ns - 1 else 0)
        c[3] = wsa.ACTIVE | (wsa.START if k in (0, k3) else 0) | (wsa.STOP if k == ns - 1 else 0)
        return c

    steps, used = _run(torch, an, pcm, fs, F, True, False, store=store, ctl_of=ctl_of)
    confs = [c["stream_conf"].copy() for _, c, _ in steps]
    assert not confs[k1 - 1][1].any()
    for k in range(k2a, k2b):
        assert np.array_equal(confs[k][2], confs[k2a - 1][2])
    assert confs[k2a - 1][2].any()
    for s, a, e in ((0, 0, nsteps), (1, k1, nsteps), (2, 0, k2a), (2, k2b, nsteps), (3, k3, nsteps)):
        x = pcm[s:s + 1, a * sps:e * sps].contiguous()
        want, _ = _batch(torch, an, x, fs, x.shape[1], store)
        assert len(want["cb"]) > 0
        assert np.array_equal(confs[e - 1][s], want["clip_conf"][0]), (s, a, e)
    store.close(); an.close()


def test_rows_unchanged_reattach_sees_added_rows_and_detach_restores_the_step(torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs = 16000
    pcm = synth_clips(6, 4 * fs, fs=fs, seed=29, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=13))
    store, rows0, _ = _store(torch, an, fs, extra=8)
    n0 = len(rows0)
    plain, used = _run(torch, an, pcm, fs, 3, True, False)
    ns = len(plain)
    first = _batch(torch, an, pcm, fs, used, store)[0]

    def hooks(k, st, state):
        if k == ns // 3:                       # eight of the signal's own later rows join the store: without re-attaching, the step keeps the old count
            _add(torch, store, late_rows[:8], np.zeros(8, np.int32))
        if k == ns // 2:
            st.set_knn(store, K)               # ... and attaching again picks them up
        if k == 3 * ns // 4:
            st.set_knn(None); state["knn"] = False

    late_rows = np.concatenate([r["feat"] for r, _, _ in plain[ns // 2:3 * ns // 4]])
    assert len(late_rows) >= 8
    steps, _ = _run(torch, an, pcm, fs, 3, True, False, store=store, before_step=hooks)
    for (a, _, _), (b, _, _) in zip(plain, steps):
        for key in ("meta", "feat", "segments"):
            assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert steps[-1][1] is None and steps[3 * ns // 4 - 1][1] is not None
    seen_old = seen_new = 0
    for k, (r, c, _) in enumerate(steps):
        if c is None or not len(c["nbr"]):
            continue
        if k < ns // 2:
            assert c["nbr"].max() < n0, "the count of the attach"
            seen_old += len(c["nbr"])
        else:
            seen_new += int((c["nbr"] >= n0).sum())
    second = _batch(torch, an, pcm, fs, used, store)[0]
    assert seen_old > 0 and seen_new > 0 and (second["nbr"] >= n0).any() and first["nbr"].max() < n0
    store.close(); an.close()


def test_a_model_and_a_store_together_give_what_each_gives_alone(torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs = 16000
    pcm = synth_clips(6, 3 * fs, fs=fs, seed=33, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=13))
    store, _, _ = _store(torch, an, fs)
    m = an.load_model(os.path.join(GOLD, "nn", MODELS[0]))
    both, _ = _run(torch, an, pcm, fs, 4, True, False, store=store, model=m)
    only_knn, _ = _run(torch, an, pcm, fs, 4, True, False, store=store)
    only_model, _ = _run(torch, an, pcm, fs, 4, True, False, model=m)
    rows = 0
    for (_, kb, mb), (_, ka, _), (_, _, ma) in zip(both, only_knn, only_model):
        for key in ROW_TABLES + ("cb", "cb_label", "cb_conf", "stream_conf"):
            assert kb[key].tobytes() == ka[key].tobytes(), key
        for key in ("prob", "cb", "cb_label", "cb_conf", "stream_conf"):
            assert mb[key].tobytes() == ma[key].tobytes(), key
        rows += len(kb["label"])
    assert rows > 0
    # attaching a store did not detach the model, and the other way round
    st = an.streams(2, fs)
    st.set_model(m); st.set_knn(store, K); st.set_model(m)
    st.step_host(None, _stream(torch)); st.collect(_stream(torch))
    assert st.knn_classes()["k_eff"] == K and st.classes()["prob"] is not None
    st.close(); m.close(); store.close(); an.close()


def test_level5_rows_only(torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs = 16000
    pcm = synth_clips(6, 3 * fs, fs=fs, seed=4, device="cuda")
    an13 = wsa.Analyzer(wsa.Config(output_level=13))
    st13, rows, index = _store(torch, an13, fs)
    st13.close(); an13.close()                 # (a store goes before its context)
    an = wsa.Analyzer(wsa.Config(output_level=5))
    store = an.knn_store(53, CLASSES, len(rows))
    _add(torch, store, rows, index)
    steps, used = _run(torch, an, pcm, fs, 2, True, True, store=store)
    for _, c, _ in steps:
        assert c["cb"] is None and c["cb_label"] is None and c["stream_conf"] is None
    got, _ = _per_stream(steps, 6)
    want, brows = _batch(torch, an, pcm, fs, used, store, fold=False)
    assert len(brows["meta"]) > 0
    _check_equal_to_batch(got, None, want, brows, 6, fold=False)
    store.close(); an.close()


@pytest.mark.parametrize("level", [3, 4, 10, 11, 12])
def test_refuses_other_levels(torch, level):
    import webspeechanalyzer_amd as wsa
    an = wsa.Analyzer(wsa.Config(output_level=level))
    store = an.knn_store(53, 2, 4)
    _add(torch, store, np.ones((2, 53)), np.zeros(2, np.int32))
    st = an.streams(2, 16000)
    with pytest.raises(wsa.WsaError, match=f"output_level 5 .*at output_level {level}, the KNN store holds rows of 53 features"):
        st.set_knn(store, K)
    st.close(); store.close(); an.close()


def test_refuses_widths_contexts_k_and_empty_stores(torch):
    import webspeechanalyzer_amd as wsa
    an, other = wsa.Analyzer(wsa.Config(output_level=13)), wsa.Analyzer(wsa.Config(output_level=13))
    st = an.streams(2, 16000)
    wide = an.knn_store(264, 2, 4)
    _add(torch, wide, np.ones((2, 264)), np.zeros(2, np.int32))
    with pytest.raises(wsa.WsaError, match="at output_level 13, the KNN store holds rows of 264 features"):
        st.set_knn(wide, K)
    foreign = other.knn_store(53, 2, 4)
    _add(torch, foreign, np.ones((2, 53)), np.zeros(2, np.int32))
    with pytest.raises(wsa.WsaError, match="another context"):
        st.set_knn(foreign, K)
    store = an.knn_store(53, 2, 4)
    with pytest.raises(wsa.WsaError, match="no examples"):
        st.set_knn(store, K)
    _add(torch, store, np.ones((2, 53)), np.zeros(2, np.int32))
    for k in (0, 65):
        with pytest.raises(wsa.WsaError, match="k must be 1 .. 64"):
            st.set_knn(store, k)
    st.step_host(None, _stream(torch))
    st.collect(_stream(torch))
    with pytest.raises(wsa.WsaError, match="no KNN store attached"):
        st.knn_classes()
    b = an.batch([16000], 16000)
    with pytest.raises(wsa.WsaError, match="no wsa_batch_knn on this batch yet"):
        b.knn_fold(_stream(torch))
    b.close(); st.close(); store.close(); foreign.close(); wide.close(); an.close(); other.close()


def test_config5_and_a_step_beyond_the_d2h_window(torch):
    """512 streams at 48 kHz, one frame per graph-replayed step: the same as the batch.  Then 1200 voiced streams all STOPped in one step
    emit more rows than the 1024-row D2H window; that step's tables are complete and equal the batch's (K9s on the window's rows, K9 on
    the rows beyond it)."""
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs = 48000
    an = wsa.Analyzer(wsa.Config(output_level=13))
    store, _, _ = _store(torch, an, fs)
    hop = an.geometry(fs)["hop"]
    pcm = synth_clips(512, 80 * hop, fs=fs, seed=77, device="cuda")
    steps, used = _run(torch, an, pcm, fs, 1, True, False, store=store)
    got, conf = _per_stream(steps, 512)
    want, rows = _batch(torch, an, pcm, fs, used, store)
    assert len(want["cb"]) > 256
    _check_equal_to_batch(got, conf, want, rows, 512)
    del pcm, steps, got

    n, F = 1200, 80                            # one step of 2 s per stream, START and STOP in it: every row of every stream at once
    pcm = synth_clips(n, F * hop, fs=fs, seed=91, device="cuda")
    steps, used = _run(torch, an, pcm, fs, F, True, False, store=store)
    assert len(steps[-1][0]["meta"]) > 1024
    got, conf = _per_stream(steps, n)
    want, rows = _batch(torch, an, pcm, fs, used, store)
    last = steps[-1][1]
    assert len(last["label"]) == len(steps[-1][0]["meta"]) and len(last["cb"]) > 0
    _check_equal_to_batch(got, conf, want, rows, n)
    store.close(); an.close()

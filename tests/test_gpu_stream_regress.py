"""A regression group inside the stream step (wsa_stream_set_regress / wsa_stream_values): the grouped K6 on every step's rows and, at
level 13, the fold RG-1 with the running sums of every (stream, head) carried on the device.  A signal fed step by step gives exactly what
wsa_batch_regress_group gives for the same signal as one clip — values, callbacks and running sums, bit for bit — and both equal the
float64 restatement tests/regress_fold_cases.rg1_ref over the stream's own rows.  START resets a stream's sums, idle steps and STOP keep
them; attaching a group changes no row and no class table, and a model, a KNN store and a group give together what each gives alone."""
import os

import numpy as np
import pytest

from tests import regress_fold_cases as C
from tests.test_gpu_stream_classify import GOLD, MODELS, _feed, _stream

pytestmark = pytest.mark.gpu

HEADS = [("sigmoid_64_16", None), ("tfjs", (-1.0, 1.0)), ("tanh_16", None)]
H = len(HEADS)
SPECS = C.model_specs()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _group(an):
    ms = [an.load_model(SPECS[k]) for k, _ in HEADS]
    return an.regress_group(ms, [r for _, r in HEADS]), ms


def _close(g, ms):
    g.close()
    for m in ms:
        m.close()


def _run(torch, an, pcm, fs, F, graph, host_in, group=None, ctl_of=None, before_step=None, model=None, store=None):
    """Steps over pcm [n, ns]; returns (per step dict(rows, values, classes, knn), samples used).  before_step(k, streams, state) may attach
    or detach; ctl_of(k, nsteps) -> control bytes (default: START on the first step, STOP on the last)."""
    import webspeechanalyzer_amd as wsa
    n, ns = pcm.shape
    st = an.streams(n, fs, frames_per_step=F)
    st.enable_graph(graph)
    sps = st.samples_per_step
    nsteps = ns // sps
    state = dict(group=group is not None, model=model is not None, knn=store is not None)
    if group is not None:
        st.set_regress(group)
    if model is not None:
        st.set_model(model)
    if store is not None:
        st.set_knn(store, 10)
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
        out.append(dict(rows=r, values=st.values() if state["group"] else None, classes=st.classes() if state["model"] else None,
                        knn=st.knn_classes() if state["knn"] else None))
    st.close()
    return out, nsteps * sps


def _per_stream(steps, n, fold=True):
    """Per stream: its rows' meta, values [H, rows], callbacks [(si, rows, values bytes, weights bytes)] in order; and the running tables
    after the last step"""
    acc = [dict(meta=[], value=[], cbs=[]) for _ in range(n)]
    for step in steps:
        r, v = step["rows"], step["values"]
        assert v["value"].shape == (H, len(r["meta"]))
        for i, m in enumerate(r["meta"]):
            a = acc[int(m[0])]
            a["meta"].append(m); a["value"].append(v["value"][:, i])
        if fold:
            for q, e in enumerate(v["cb"]):
                assert np.array_equal(r["meta"][e[2]][:2], [e[0], e[1]])
                acc[int(e[0])]["cbs"].append((int(e[1]), int(e[3]), v["cb_value"][:, q].tobytes(), v["cb_weight"][:, q].tobytes()))
    for a in acc:
        a["meta"] = np.array(a["meta"], np.int32).reshape(-1, 8)
        a["value"] = np.array(a["value"], np.float64).reshape(-1, H).T
    return acc, steps[-1]["values"]


def _batch(torch, an, pcm, fs, used, group):
    b = an.batch([used] * pcm.shape[0], fs)
    x = pcm[:, :used].contiguous()
    b.run(x.data_ptr(), x.stride(0), _stream(torch))
    b.regress_group(group, _stream(torch))
    got = b.value_fold(_stream(torch))
    rows = b.rows(_stream(torch))
    b.close()
    return got, rows


def _check_equal_to_batch(got, last, want, rows, n, step_s, fold=True, restate=True):
    ro = rows["row_off"]
    for s in range(n):
        a, b = int(ro[s]), int(ro[s + 1])
        g = got[s]
        assert len(g["meta"]) == b - a, f"stream {s}"
        if b > a:
            assert np.array_equal(g["meta"][:, 1:], rows["meta"][a:b, 1:]), f"stream {s}"
        assert np.ascontiguousarray(g["value"]).tobytes() == np.ascontiguousarray(want["value"][:, a:b]).tobytes(), f"stream {s}"     # bit for bit
        if not fold:
            continue
        wcb = [(int(e[1]), int(e[3]), want["cb_value"][:, k].tobytes(), want["cb_weight"][:, k].tobytes()) for k, e in enumerate(want["cb"]) if e[0] == s]
        assert g["cbs"] == wcb, f"stream {s}"
        for mine, theirs in (("stream_sum", "clip_sum"), ("stream_weight", "clip_weight"), ("stream_value", "clip_value")):
            assert last[mine][:, s].tobytes() == want[theirs][:, s].tobytes(), (mine, s)
        if restate:                                   # ... and the restatement over the stream's own rows
            cbs, run = C.rg1_ref(g["meta"], g["value"], step_s)
            assert [(c["si"], c["rows"], np.array(c["value"]).tobytes(), np.array(c["weight"]).tobytes()) for c in cbs] == g["cbs"], f"stream {s}"
            A, B, V = C.run_value(run, s, H)
            assert np.array(A).tobytes() == last["stream_sum"][:, s].tobytes() and np.array(B).tobytes() == last["stream_weight"][:, s].tobytes()
            assert np.array(V).tobytes() == last["stream_value"][:, s].tobytes()


@pytest.mark.parametrize("F,graph,host_in", [(1, True, True), (4, True, False), (1, False, False), (4, False, True)])
def test_stream_values_equal_the_batch_and_the_restatement(torch, F, graph, host_in):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs, n = 16000, 6
    cfg = wsa.Config(output_level=13)
    pcm = synth_clips(n, 3 * fs, fs=fs, seed=23, device="cuda")
    an = wsa.Analyzer(cfg)
    g, ms = _group(an)
    steps, used = _run(torch, an, pcm, fs, F, graph, host_in, group=g)
    got, last = _per_stream(steps, n)
    want, rows = _batch(torch, an, pcm, fs, used, g)
    assert len(want["cb"]) >= n and any(e[3] > 1 for e in want["cb"])
    _check_equal_to_batch(got, last, want, rows, n, cfg["window_step"] / 1e3)
    _close(g, ms); an.close()


def test_restart_idle_and_stop_then_start(torch):
    """Four streams: 0 plays through; 1 idles, then STARTs mid-run; 2 STOPs, idles and STARTs again on the rest of its signal; 3 gets a
    START mid-run without a STOP.  Each stream's running sums equal a fresh batch of only its post-START signal; idle steps keep them."""
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs, F = 16000, 5
    pcm = synth_clips(4, 6 * fs, fs=fs, seed=41, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=13))
    g, ms = _group(an)
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

    steps, used = _run(torch, an, pcm, fs, F, True, False, group=g, ctl_of=ctl_of)
    sums = [(s["values"]["stream_sum"].copy(), s["values"]["stream_weight"].copy(), s["values"]["stream_value"].copy()) for s in steps]
    assert not sums[k1 - 1][1][:, 1].any() and np.isnan(sums[k1 - 1][2][:, 1]).all()           # never started: zeros and NaN
    for k in range(k2a, k2b):                                                                   # kept after STOP, untouched while idle
        assert sums[k][0][:, 2].tobytes() == sums[k2a - 1][0][:, 2].tobytes() and sums[k][1][:, 2].tobytes() == sums[k2a - 1][1][:, 2].tobytes()
    assert sums[k2a - 1][1][:, 2].all()
    for s, a, e in ((0, 0, nsteps), (1, k1, nsteps), (2, 0, k2a), (2, k2b, nsteps), (3, k3, nsteps)):
        x = pcm[s:s + 1, a * sps:e * sps].contiguous()
        want, _ = _batch(torch, an, x, fs, x.shape[1], g)
        assert len(want["cb"]) > 0
        for j, name in enumerate(("clip_sum", "clip_weight", "clip_value")):
            assert sums[e - 1][j][:, s].tobytes() == want[name][:, 0].tobytes(), (s, a, e, name)
    _close(g, ms); an.close()


def test_attaching_leaves_rows_and_classes_alone_and_detaching_restores_the_step(torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs = 16000
    pcm = synth_clips(6, 4 * fs, fs=fs, seed=29, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=13))
    g, ms = _group(an)
    m = an.load_model(os.path.join(GOLD, "nn", MODELS[0]))
    plain, used = _run(torch, an, pcm, fs, 3, True, False, model=m)
    ns = len(plain)

    def hooks(k, st, state):
        if k == ns // 3:
            st.set_regress(g); state["group"] = True
        if k == 3 * ns // 4:
            st.set_regress(None); state["group"] = False

    steps, _ = _run(torch, an, pcm, fs, 3, True, False, model=m, before_step=hooks)
    rows = 0
    for a, b in zip(plain, steps):
        for key in ("meta", "feat", "segments"):
            assert np.array_equal(a["rows"][key], b["rows"][key], equal_nan=True), key
        for key in ("prob", "cb", "cb_label", "cb_conf", "stream_conf"):
            assert a["classes"][key].tobytes() == b["classes"][key].tobytes(), key
        rows += len(a["rows"]["meta"])
    assert rows > 0
    assert steps[ns // 3 - 1]["values"] is None and steps[ns // 3]["values"] is not None and steps[-1]["values"] is None
    # attached mid-run: the sums count from the attach (zeroed), and the values are the batch's for the same rows
    want, brows = _batch(torch, an, pcm, fs, used, g)
    seen = 0
    for k in range(ns // 3, 3 * ns // 4):
        r, v = steps[k]["rows"], steps[k]["values"]
        for i, mrow in enumerate(r["meta"]):
            s = int(mrow[0])
            a, b = int(brows["row_off"][s]), int(brows["row_off"][s + 1])
            j = a + int(np.flatnonzero((brows["meta"][a:b, 1:] == mrow[1:]).all(axis=1))[0])
            assert v["value"][:, i].tobytes() == want["value"][:, j].tobytes()
            seen += 1
    assert seen > 0
    st = an.streams(2, fs)
    st.step_host(None, _stream(torch)); st.collect(_stream(torch))
    with pytest.raises(wsa.WsaError, match="no regression group attached"):
        st.values()
    st.close(); m.close(); _close(g, ms); an.close()


def test_a_model_a_store_and_a_group_together_give_what_each_gives_alone(torch):
    import webspeechanalyzer_amd as wsa
    from tests.test_gpu_stream_knn import _store, ROW_TABLES
    from webspeechanalyzer_amd.synth import synth_clips
    fs = 16000
    pcm = synth_clips(6, 3 * fs, fs=fs, seed=33, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=13))
    g, ms = _group(an)
    store, _, _ = _store(torch, an, fs)
    m = an.load_model(os.path.join(GOLD, "nn", MODELS[0]))
    all3, _ = _run(torch, an, pcm, fs, 4, True, False, group=g, model=m, store=store)
    only_g, _ = _run(torch, an, pcm, fs, 4, True, False, group=g)
    only_m, _ = _run(torch, an, pcm, fs, 4, True, False, model=m)
    only_k, _ = _run(torch, an, pcm, fs, 4, True, False, store=store)
    rows = 0
    for x, a, b, c in zip(all3, only_g, only_m, only_k):
        for key in ("value", "cb", "cb_value", "cb_weight", "stream_sum", "stream_weight", "stream_value"):
            assert x["values"][key].tobytes() == a["values"][key].tobytes(), key
        for key in ("prob", "cb", "cb_label", "cb_conf", "stream_conf"):
            assert x["classes"][key].tobytes() == b["classes"][key].tobytes(), key
        for key in ROW_TABLES + ("cb", "cb_label", "cb_conf", "stream_conf"):
            assert x["knn"][key].tobytes() == c["knn"][key].tobytes(), key
        rows += x["values"]["value"].shape[1]
    assert rows > 0
    # attaching a group detaches nothing, and nothing detaches it
    st = an.streams(2, fs)
    st.set_model(m); st.set_regress(g); st.set_knn(store, 10); st.set_model(m)
    st.step_host(None, _stream(torch)); st.collect(_stream(torch))
    assert st.values()["value"] is not None and st.classes()["prob"] is not None and st.knn_classes()["k_eff"] == 10
    st.close(); m.close(); store.close(); _close(g, ms); an.close()


def test_level5_values_only(torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs = 16000
    pcm = synth_clips(4, 3 * fs, fs=fs, seed=4, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=5))
    g, ms = _group(an)
    steps, used = _run(torch, an, pcm, fs, 2, True, True, group=g)
    for s in steps:
        v = s["values"]
        assert v["cb"] is None and v["cb_value"] is None and v["stream_sum"] is None and v["stream_value"] is None
    got, _ = _per_stream(steps, 4, fold=False)
    want, brows = _batch(torch, an, pcm, fs, used, g)
    assert len(brows["meta"]) > 0 and sorted(want) == ["value"]
    _check_equal_to_batch(got, None, want, brows, 4, 0.025, fold=False)
    _close(g, ms); an.close()


@pytest.mark.parametrize("level", [3, 4, 10, 11, 12])
def test_refuses_other_levels_by_name(level):
    import webspeechanalyzer_amd as wsa
    an = wsa.Analyzer(wsa.Config(output_level=level))
    g, ms = _group(an)
    st = an.streams(2, 16000)
    with pytest.raises(wsa.WsaError, match=f"wsa_stream_set_regress needs streams at output_level 5 .*or 13 .*not {level}"):
        st.set_regress(g)
    st.close(); _close(g, ms); an.close()


def test_refuses_a_group_of_another_context():
    import webspeechanalyzer_amd as wsa
    an, other = wsa.Analyzer(wsa.Config(output_level=13)), wsa.Analyzer(wsa.Config(output_level=13))
    g, ms = _group(other)
    st = an.streams(2, 16000)
    with pytest.raises(wsa.WsaError, match="another context"):
        st.set_regress(g)
    st.close(); _close(g, ms); an.close(); other.close()


# The smallest stream count whose STOP-flush step emits more rows than the D2H window of 1024 rows: every stream gets one step of 2 s at 48 kHz
# (synth_clips seed 91) with START and STOP in it, so that all its rows come out of that one step.  Counted on an MI355X with the batch over the
# same clips: 305 streams give 1022 rows, 306 give 1025 (307: 1027, 310: 1038, 1200: 4033).
N_BEYOND = 306


def test_a_step_beyond_the_d2h_window(torch):
    """N_BEYOND voiced streams all STOPped in one step emit more rows than the 1024-row D2H window; that step's tables are complete and
    equal the batch's (values, callbacks and sums fetched from the device at wsa_stream_values)."""
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs, F = 48000, 80
    an = wsa.Analyzer(wsa.Config(output_level=13))
    g, ms = _group(an)
    hop = an.geometry(fs)["hop"]
    pcm = synth_clips(N_BEYOND, F * hop, fs=fs, seed=91, device="cuda")
    steps, used = _run(torch, an, pcm, fs, F, True, False, group=g)
    n_rows = len(steps[-1]["rows"]["meta"])
    print(f"{N_BEYOND} streams: {n_rows} rows in the STOP step")
    assert n_rows > 1024
    got, last = _per_stream(steps, N_BEYOND)
    want, rows = _batch(torch, an, pcm, fs, used, g)
    v = steps[-1]["values"]
    assert v["value"].shape[1] == n_rows and len(v["cb"]) == len(want["cb"]) > 0
    _check_equal_to_batch(got, last, want, rows, N_BEYOND, 0.025, restate=False)
    _close(g, ms); an.close()

"""An ensemble inside the stream step (wsa_stream_set_ensemble / wsa_stream_ensemble_classes): K6e on every step's rows and, at level
13, one accumulator per stream and member plus one running max_inv_entropy / min_entropy_db per stream, carried on the device.  A
signal fed step by step gives exactly the tables wsa_batch_classify_ensemble gives for the same signal as one clip; START resets a
stream's accumulators and running maximum, idle steps and STOP keep them; swapping a model and an ensemble recaptures the graph;
attaching an ensemble changes no row."""
import json
import os

import numpy as np
import pytest

from tests import classify_ref, ensemble_ref
from webspeechanalyzer_amd import nnmodel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DIRS = {1: "1/cats_emotion", 2: "2/cats_emotion"}
SIX = [1, 2, "s5", "s6", "s7", "s8"]
PER_MEMBER = ("cb_label", "cb_conf", "cb_all_max")
SHARED = ("cb_db", "cb_top_label", "cb_top_conf", "cb_min_db", "cb_entropy")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _spec(key):
    if isinstance(key, str):
        return classify_ref.seeded_spec(seed=int(key[1:]))
    return nnmodel.load_dir(os.path.join(GOLD, "nn", DIRS[key]))


def _members(an, keys):
    loaded = {}
    for k in keys:
        if k not in loaded:
            loaded[k] = an.load_model(_spec(k))
    return [loaded[k] for k in keys]


def _close(an, ens, members):
    """the ensemble, then its models, then their context"""
    ens.close()
    for m in {id(m): m for m in members}.values():
        m.close()
    an.close()


def _signals(torch, which):
    """(config, pcm [n, ns] on the GPU at the analysis rate, fs)."""
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    if which == "config1_excerpt":             # the sample file's excerpt, converted to 48 kHz by the batch's own resampler
        exc = np.load(os.path.join(GOLD, "config1_excerpt.npz"))
        S = json.load(open(os.path.join(GOLD, "config1_expected.json")))["settings"]
        cfg = wsa.Config(output_level=13, window_step=S["window_step"], pause_length=S["pause_length"], min_seg_length=S["min_seg_length"])
        x = (exc["pcm_i16"].astype(np.float32) / np.float32(32768.0)).astype(np.float32)
        an = wsa.Analyzer(cfg)
        b = an.batch([len(x)], int(exc["fs"]), resample_to=S["fs_context"])
        src = torch.from_numpy(x).cuda()[None, :].contiguous()
        b.run(src.data_ptr(), src.stride(0), _stream(torch))
        conv = b.converted_pcm(_stream(torch))
        b.close(); an.close()
        return cfg, torch.from_numpy(conv).cuda().contiguous(), int(S["fs_context"])
    return wsa.Config(output_level=13), synth_clips(12, 48000, fs=16000, seed=23, device="cuda"), 16000


def _run(torch, an, pcm, fs, F, graph, host_in, ens=None, ctl_of=None, at=None):
    """Steps over pcm [n, ns]; returns (per step (rows, ensemble classes / model classes / None), samples used).  `at` maps a step
    index to ("ensemble", e) / ("model", m) / ("none", None), applied before that step; `ens` is attached from the start."""
    import webspeechanalyzer_amd as wsa
    n, ns = pcm.shape
    st = an.streams(n, fs, frames_per_step=F)
    st.enable_graph(graph)
    sps = st.samples_per_step
    nsteps = ns // sps
    mode = "none"
    if ens is not None:
        st.set_ensemble(ens); mode = "ensemble"
    buf = torch.zeros((n, sps), device="cuda", dtype=torch.float32)
    out = []
    for k in range(nsteps):
        if at and k in at:
            mode, obj = at[k]
            if mode == "ensemble":
                st.set_ensemble(obj)
            elif mode == "model":
                st.set_model(obj)
            else:
                st.set_ensemble(None); st.set_model(None)
        if ctl_of is not None:
            ctl = ctl_of(k, nsteps)
        else:
            ctl = np.full(n, wsa.ACTIVE, np.uint8)
            if k == 0:
                ctl |= wsa.START
            if k == nsteps - 1:
                ctl |= wsa.STOP
        chunk = pcm[:, k * sps:(k + 1) * sps]
        if host_in:
            st.host_input()[:] = chunk.cpu().numpy()
            st.step_host(ctl, _stream(torch))
        else:
            buf.copy_(chunk)
            st.step(buf.data_ptr(), buf.stride(0), ctl, _stream(torch))
        r = st.collect(_stream(torch))
        if mode == "ensemble":
            with pytest.raises(wsa.WsaError, match="no classifier"):
                st.classes()
            out.append((r, st.ensemble_classes(), mode))
        elif mode == "model":
            with pytest.raises(wsa.WsaError, match="no ensemble"):
                st.ensemble_classes()
            out.append((r, st.classes(), mode))
        else:
            out.append((r, None, mode))
    st.close()
    return out, nsteps * sps


def _per_stream(steps, n, nm):
    """Per stream: its rows, per-member probabilities, and per callback (si, rows) plus every table's entry, in order; and the last
    step's stream_conf / stream_min_db."""
    acc = [dict(meta=[], feat=[], prob=[[] for _ in range(nm)], cb=[], **{k: [[] for _ in range(nm)] for k in PER_MEMBER}, **{k: [] for k in SHARED})
           for _ in range(n)]
    conf = mdb = None
    for r, c, _ in steps:
        for i, m in enumerate(r["meta"]):
            a = acc[int(m[0])]
            a["meta"].append(m); a["feat"].append(r["feat"][i])
            for d in range(nm):
                a["prob"][d].append(c["prob"][d][i])
        if "cb" in c:
            for q, e in enumerate(c["cb"]):
                assert np.array_equal(r["meta"][e[2]][:2], [e[0], e[1]])
                a = acc[int(e[0])]
                a["cb"].append((int(e[1]), int(e[3])))
                for key in PER_MEMBER:
                    for d in range(nm):
                        a[key][d].append(c[key][d][q])
                for key in SHARED:
                    a[key].append(c[key][q])
            conf, mdb = c["stream_conf"], c["stream_min_db"]
    return acc, conf, mdb


def _batch(torch, an, pcm, fs, used, ens):
    b = an.batch([used] * pcm.shape[0], fs)
    x = pcm[:, :used].contiguous()
    b.run(x.data_ptr(), x.stride(0), _stream(torch))
    b.classify_ensemble(ens, _stream(torch))
    got, rows = b.ensemble_classes(_stream(torch)), b.rows(_stream(torch))
    b.close()
    return got, rows


def _check_equal_to_batch(got, conf, mdb, want, rows, n, nm, level=13):
    ro = rows["row_off"]
    for s in range(n):
        a, b = int(ro[s]), int(ro[s + 1])
        g = got[s]
        assert len(g["meta"]) == b - a, f"stream {s}"
        if b == a:
            continue
        assert np.array_equal(np.array(g["meta"])[:, 1:], rows["meta"][a:b, 1:]), f"stream {s}"
        assert np.array_equal(np.array(g["feat"]), rows["feat"][a:b], equal_nan=True), f"stream {s}"
        for d in range(nm):
            assert np.array_equal(np.array(g["prob"][d], np.float32), want["prob"][d][a:b]), (s, d)     # bit for bit
        if level != 13:
            continue
        idx = [k for k, e in enumerate(want["cb"]) if e[0] == s]
        assert g["cb"] == [(int(want["cb"][k][1]), int(want["cb"][k][3])) for k in idx], f"stream {s}"
        for key in PER_MEMBER:
            for d in range(nm):
                assert np.array_equal(np.array(g[key][d]), want[key][d][idx]), (s, key, d)
        for key in SHARED:
            assert np.array_equal(np.array(g[key]), want[key][idx], equal_nan=True), (s, key)
        for d in range(nm):
            assert np.array_equal(conf[d][s], want["clip_conf"][d][s]), (s, d)
        assert mdb[s] == want["clip_min_db"][s], f"stream {s}"


@pytest.mark.parametrize("F,graph,host_in", [(1, True, True), (7, True, False), (1, False, False), (7, False, True)])
@pytest.mark.parametrize("keys", [[1, 2], SIX], ids=["1_2", "six"])
@pytest.mark.parametrize("which", ["config1_excerpt", "synthetic"])
def test_stream_ensemble_tables_equal_the_batch_exactly(torch, which, keys, F, graph, host_in):
    import webspeechanalyzer_amd as wsa
    cfg, pcm, fs = _signals(torch, which)
    an = wsa.Analyzer(cfg)
    members = _members(an, keys)
    ens = an.ensemble(members)
    steps, used = _run(torch, an, pcm, fs, F, graph, host_in, ens=ens)
    n, nm = pcm.shape[0], len(members)
    got, conf, mdb = _per_stream(steps, n, nm)
    want, rows = _batch(torch, an, pcm, fs, used, ens)
    assert len(want["cb"]) > 0 and np.any(want["cb_min_db"] >= 0)
    _check_equal_to_batch(got, conf, mdb, want, rows, n, nm)
    # the decision, bit-exact against the float64 restatement fed the stream's own probabilities
    legends = [m.labels for m in members]
    for s in range(n):
        if not len(got[s]["meta"]):
            continue
        ref = ensemble_ref.fold_rows(np.array(got[s]["meta"]), [np.array(p, np.float64) for p in got[s]["prob"]], legends, cfg["window_step"] / 1e3)
        for key in ("cb_db", "cb_top_label", "cb_top_conf", "cb_min_db"):
            assert [x.item() for x in got[s][key]] == ref[key], (s, key)
        assert np.array_equal(np.array(got[s]["cb_entropy"]), np.array(ref["cb_entropy"]), equal_nan=True)
    _close(an, ens, members)


def test_restart_idle_and_stop_then_start(torch):
    """Four streams: 0 plays through; 1 idles, then STARTs mid-run; 2 STOPs, idles and STARTs again on the rest of its signal; 3 gets a
    START mid-run without a STOP.  After each span a stream's accumulators, min_entropy_db and the span's callbacks equal a fresh batch
    of only its post-START signal (so START reset the running maximum too); idle steps and STOP keep them."""
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs, F = 16000, 5
    pcm = synth_clips(4, 6 * fs, fs=fs, seed=41, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=13))
    members = _members(an, [2, 1, "s5"])
    nm = len(members)
    ens = an.ensemble(members)
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

    steps, used = _run(torch, an, pcm, fs, F, True, False, ens=ens, ctl_of=ctl_of)
    confs = [[x.copy() for x in c["stream_conf"]] for _, c, _ in steps]
    mdbs = [c["stream_min_db"].copy() for _, c, _ in steps]
    # stream 1 has nothing before its START; stream 2's meters and DB stay as they were while it idles after its STOP
    assert mdbs[k1 - 1][1] == -1 and not any(confs[k1 - 1][d][1].any() for d in range(nm))
    for k in range(k2a, k2b):
        assert mdbs[k][2] == mdbs[k2a - 1][2] and all(np.array_equal(confs[k][d][2], confs[k2a - 1][d][2]) for d in range(nm))
    assert mdbs[k2a - 1][2] >= 0 and confs[k2a - 1][0][2].any()

    for s, a, e in ((0, 0, nsteps), (1, k1, nsteps), (2, 0, k2a), (2, k2b, nsteps), (3, k3, nsteps)):
        x = pcm[s:s + 1, a * sps:e * sps].contiguous()
        want, _ = _batch(torch, an, x, fs, x.shape[1], ens)
        assert len(want["cb"]) > 0
        for d in range(nm):
            assert np.array_equal(confs[e - 1][d][s], want["clip_conf"][d][0]), (s, a, e, d)
        assert mdbs[e - 1][s] == want["clip_min_db"][0], (s, a, e)
        span = dict(cb_min_db=[], cb_entropy=[], cb_db=[], cb_top_conf=[], cb_all_max=[])
        for _, c, _ in steps[a:e]:
            for q, cb in enumerate(c["cb"]):
                if cb[0] == s:
                    for key in ("cb_min_db", "cb_entropy", "cb_db", "cb_top_conf"):
                        span[key].append(c[key][q])
                    span["cb_all_max"].append([c["cb_all_max"][d][q] for d in range(nm)])
        for key in ("cb_min_db", "cb_entropy", "cb_db", "cb_top_conf"):
            assert np.array_equal(np.array(span[key]), want[key], equal_nan=True), (s, a, e, key)
        assert np.array_equal(np.array(span["cb_all_max"]).T.reshape(nm, -1), np.array(want["cb_all_max"])), (s, a, e)
    _close(an, ens, members)


def test_rows_unchanged_and_swapping_model_and_ensemble_recaptures(torch):
    """Rows with an ensemble attached are bit-identical to a run without one; a run (graph on) that goes model -> ensemble -> model ->
    nothing gives in every step the tables of the same run without the graph, and each kind's getter refuses while the other is attached."""
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs = 16000
    pcm = synth_clips(6, 4 * fs, fs=fs, seed=29, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=13))
    members = _members(an, [1, 2])
    ens = an.ensemble(members)
    plain, _ = _run(torch, an, pcm, fs, 3, True, False)
    ns = len(plain)
    at = {0: ("model", members[0]), ns // 4: ("ensemble", ens), ns // 2: ("model", members[1]), 3 * ns // 4: ("none", None)}
    runs = [_run(torch, an, pcm, fs, 3, True, False, ens=ens)[0], _run(torch, an, pcm, fs, 3, True, False, at=at)[0]]
    for steps in runs:
        for (a, _, _), (b, _, _) in zip(plain, steps):
            for key in ("meta", "feat", "segments"):
                assert np.array_equal(a[key], b[key], equal_nan=True), key
    eager = _run(torch, an, pcm, fs, 3, False, False, at=at)[0]
    seen = {"model": 0, "ensemble": 0, "none": 0}
    for (_, g, mode), (_, e, mode_e) in zip(runs[1], eager):
        assert mode == mode_e
        if mode == "none":
            assert g is None and e is None
        elif mode == "model":
            for key in ("prob", "cb", "cb_label", "cb_conf", "stream_conf"):
                assert np.array_equal(g[key], e[key]), key
        else:
            for key in ("prob",) + PER_MEMBER + ("stream_conf",):
                for d in range(2):
                    assert np.array_equal(g[key][d], e[key][d]), (key, d)
            for key in ("cb",) + SHARED + ("stream_min_db",):
                assert np.array_equal(g[key], e[key], equal_nan=True), key
        seen[mode] += 0 if g is None else len(g["prob"][0] if mode == "ensemble" else g["prob"])
    assert seen["model"] > 0 and seen["ensemble"] > 0
    _close(an, ens, members)


def test_a_refused_attach_changes_nothing(torch):
    """A wsa_stream_set_* call that is refused (the object belongs to another context) leaves what was attached attached and detaches nothing:
    with the graph on, a run that suffers refused set_model / set_ensemble calls between its steps gives in every step the tables of the
    undisturbed run — once with a model attached, once with an ensemble."""
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs = 16000
    pcm = synth_clips(2, 14400, fs=fs, seed=31, device="cuda")          # 0.9 s, voiced to the end: STOP closes a segment with rows
    an, other = wsa.Analyzer(wsa.Config(output_level=13)), wsa.Analyzer(wsa.Config(output_level=13))
    members = _members(an, [1, 2])
    ens = an.ensemble(members)
    ms_other = _members(other, [2])
    e_other = other.ensemble(ms_other)

    def run(kind, disturb):
        st = an.streams(2, fs, frames_per_step=4)
        st.enable_graph(True)
        (st.set_model if kind == "model" else st.set_ensemble)(members[0] if kind == "model" else ens)
        sps = st.samples_per_step
        buf = torch.zeros((2, sps), device="cuda", dtype=torch.float32)
        out, nsteps = [], pcm.shape[1] // sps
        for k in range(nsteps):
            if disturb and k in (0, 2, nsteps - 1):                     # before the first step, behind a captured one, before the STOP
                with pytest.raises(wsa.WsaError, match="another context"):
                    st.set_ensemble(e_other)
                with pytest.raises(wsa.WsaError, match="another context"):
                    st.set_model(ms_other[0])
            ctl = np.full(2, wsa.ACTIVE | (wsa.START if k == 0 else 0) | (wsa.STOP if k == nsteps - 1 else 0), np.uint8)
            buf.copy_(pcm[:, k * sps:(k + 1) * sps])
            st.step(buf.data_ptr(), buf.stride(0), ctl, _stream(torch))
            r = st.collect(_stream(torch))
            with pytest.raises(wsa.WsaError, match="no ensemble" if kind == "model" else "no classifier"):
                st.ensemble_classes() if kind == "model" else st.classes()       # the other kind was not attached by the refused call
            out.append((r, st.classes() if kind == "model" else st.ensemble_classes()))
        st.close()
        return out

    for kind in ("model", "ensemble"):
        want, got = run(kind, False), run(kind, True)
        rows = sum(len(r["meta"]) for r, _ in want)
        print(kind, "steps", len(want), "rows", rows)
        assert rows > 0 and len(got) == len(want)
        for (rw, cw), (rg, cg) in zip(want, got):
            for key in ("meta", "feat", "segments"):
                assert np.array_equal(rw[key], rg[key], equal_nan=True), (kind, key)
            if kind == "model":
                for key in ("prob", "cb", "cb_label", "cb_conf", "stream_conf"):
                    assert np.array_equal(cw[key], cg[key]), (kind, key)
            else:
                for key in ("prob",) + PER_MEMBER + ("stream_conf",):
                    for d in range(2):
                        assert np.array_equal(cw[key][d], cg[key][d]), (kind, key, d)
                for key in ("cb",) + SHARED + ("stream_min_db",):
                    assert np.array_equal(cw[key], cg[key], equal_nan=True), (kind, key)
    _close(other, e_other, ms_other)
    _close(an, ens, members)


def test_level5_probabilities_only(torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs = 16000
    pcm = synth_clips(6, 3 * fs, fs=fs, seed=4, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=5))
    members = _members(an, [1, "s5"])
    ens = an.ensemble(members)
    steps, used = _run(torch, an, pcm, fs, 2, True, True, ens=ens)
    for _, c, _ in steps:
        assert "cb" not in c and "stream_conf" not in c
    got, _, _ = _per_stream(steps, 6, 2)
    want, rows = _batch(torch, an, pcm, fs, used, ens)
    assert len(rows["meta"]) > 0
    _check_equal_to_batch(got, None, None, want, rows, 6, 2, level=5)
    _close(an, ens, members)


def test_refusals(torch):
    import webspeechanalyzer_amd as wsa
    for level in (3, 4, 10, 11, 12):
        an = wsa.Analyzer(wsa.Config(output_level=level))
        ms = _members(an, [2])
        e = an.ensemble(ms)
        st = an.streams(2, 16000)
        with pytest.raises(wsa.WsaError, match="output_level 5"):
            st.set_ensemble(e)
        st.close()
        _close(an, e, ms)
    an, other = wsa.Analyzer(wsa.Config(output_level=13)), wsa.Analyzer(wsa.Config(output_level=13))
    st = an.streams(2, 16000)
    ms_other = _members(other, [2])
    e_other = other.ensemble(ms_other)
    with pytest.raises(wsa.WsaError, match="another context"):
        st.set_ensemble(e_other)
    s = classify_ref.seeded_spec(widths=(4, 4))
    m_lin = an.load_model(nnmodel.ModelSpec(s.units, ["relu", "linear"], s.kernels, s.biases, s.in_min, s.in_max, s.labels))
    ms = _members(an, [1]) + [m_lin]
    e_lin = an.ensemble(ms)
    with pytest.raises(wsa.WsaError, match="softmax"):
        st.set_ensemble(e_lin)
    st.step_host(None, _stream(torch))
    st.collect(_stream(torch))
    with pytest.raises(wsa.WsaError, match="no ensemble"):
        st.ensemble_classes()
    st.close()
    _close(an, e_lin, ms)
    _close(other, e_other, ms_other)


def test_a_step_beyond_the_d2h_window(torch):
    """1200 voiced streams all STOPped in one step emit more rows than the 1024-row D2H window; that step's ensemble tables are
    complete and equal the batch's."""
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs = 48000
    an = wsa.Analyzer(wsa.Config(output_level=13))
    members = _members(an, [1, 2])
    ens = an.ensemble(members)
    hop = an.geometry(fs)["hop"]
    n, F = 1200, 80
    pcm = synth_clips(n, F * hop, fs=fs, seed=91, device="cuda")
    steps, used = _run(torch, an, pcm, fs, F, True, False, ens=ens)
    assert len(steps[-1][0]["meta"]) > 1024
    got, conf, mdb = _per_stream(steps, n, 2)
    want, rows = _batch(torch, an, pcm, fs, used, ens)
    last = steps[-1][1]
    assert len(last["prob"][0]) == len(steps[-1][0]["meta"]) and len(last["cb"]) > 0
    _check_equal_to_batch(got, conf, mdb, want, rows, n, 2)
    _close(an, ens, members)

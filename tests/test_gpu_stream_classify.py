"""The classifier inside the stream step (wsa_stream_set_model / wsa_stream_classes): K6 on every step's rows and, at level 13, the
fold with one Label_conf_all per stream carried on the device.  A signal fed step by step gives exactly what wsa_batch_classify gives
for the same signal as one clip; START resets a stream's accumulator, idle steps leave it alone; attaching a model changes no row."""
import json
import os

import numpy as np
import pytest

from tests import classify_ref
from tests.classify_ref import seeded_spec
from webspeechanalyzer_amd import nnmodel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MODELS = ["1/cats_emotion", "2/cats_emotion"]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _spec(name):
    return seeded_spec() if name == "seeded_512" else nnmodel.load_dir(os.path.join(GOLD, "nn", name))


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


def _feed(torch, wsa, st, pcm, k, sps, ctl, host_in, buf):
    chunk = pcm[:, k * sps:(k + 1) * sps]
    if host_in:
        st.host_input()[:] = chunk.cpu().numpy()
        st.step_host(ctl, _stream(torch))
    else:
        buf.copy_(chunk)
        st.step(buf.data_ptr(), buf.stride(0), ctl, _stream(torch))


def _run(torch, an, pcm, fs, F, graph, host_in, model=None, ctl_of=None, attach_at=None, detach_at=None):
    """Steps over pcm [n, ns]; returns (per step (rows, classes or None), samples used).  ctl_of(k, nsteps) -> control bytes
    (default: START on the first step, STOP on the last)."""
    import webspeechanalyzer_amd as wsa
    n, ns = pcm.shape
    st = an.streams(n, fs, frames_per_step=F)
    st.enable_graph(graph)
    sps = st.samples_per_step
    nsteps = ns // sps
    if model is not None and attach_at is None:
        st.set_model(model)
    buf = torch.zeros((n, sps), device="cuda", dtype=torch.float32)
    out, on = [], model is not None and attach_at is None
    for k in range(nsteps):
        if model is not None and k == attach_at:
            st.set_model(model); on = True
        if k == detach_at:
            st.set_model(None); on = False
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
        out.append((r, st.classes() if on else None))
    st.close()
    return out, nsteps * sps


def _per_stream(steps, n, C):
    """Per stream: rows (meta, feat), prob, callbacks [(si, rows, label, conf)] in order, and stream_conf after the last step."""
    acc = [dict(meta=[], feat=[], prob=[], cbs=[]) for _ in range(n)]
    conf = None
    for r, c in steps:
        for i, m in enumerate(r["meta"]):
            s = int(m[0])
            acc[s]["meta"].append(m); acc[s]["feat"].append(r["feat"][i]); acc[s]["prob"].append(c["prob"][i])
        if c["cb"] is not None:
            for q, e in enumerate(c["cb"]):
                assert np.array_equal(r["meta"][e[2]][:2], [e[0], e[1]])
                acc[int(e[0])]["cbs"].append((int(e[1]), int(e[3]), int(c["cb_label"][q]), float(c["cb_conf"][q])))
            conf = c["stream_conf"]
    for a in acc:
        a["prob"] = np.array(a["prob"], np.float32).reshape(-1, C)
        a["feat"] = np.array(a["feat"]).reshape(-1, 53)
    return acc, conf


def _batch_classes(torch, an, pcm, fs, used, model):
    b = an.batch([used] * pcm.shape[0], fs)
    x = pcm[:, :used].contiguous()
    b.run(x.data_ptr(), x.stride(0), _stream(torch))
    b.classify(model, _stream(torch))
    got, rows = b.classes(_stream(torch)), b.rows(_stream(torch))
    b.close()
    return got, rows


def _check_equal_to_batch(got, conf, want, rows, n, level=13):
    ro = rows["row_off"]
    for s in range(n):
        a, b = int(ro[s]), int(ro[s + 1])
        g = got[s]
        assert len(g["meta"]) == b - a, f"stream {s}"
        if b == a:
            continue
        assert np.array_equal(np.array(g["meta"])[:, 1:], rows["meta"][a:b, 1:]), f"stream {s}"
        assert np.array_equal(g["feat"], rows["feat"][a:b], equal_nan=True), f"stream {s}"
        assert np.array_equal(g["prob"], want["prob"][a:b]), f"stream {s}"     # bit for bit
        if level != 13:
            continue
        wcb = [(int(e[1]), int(e[3]), int(want["cb_label"][k]), float(want["cb_conf"][k])) for k, e in enumerate(want["cb"]) if e[0] == s]
        assert g["cbs"] == wcb, f"stream {s}"
        assert np.array_equal(conf[s], want["clip_conf"][s]), f"stream {s}"


@pytest.mark.parametrize("F,graph,host_in", [(1, True, True), (7, True, False), (1, False, False), (7, False, True)])
@pytest.mark.parametrize("name", MODELS + ["seeded_512"])
@pytest.mark.parametrize("which", ["config1_excerpt", "synthetic"])
def test_stream_classes_equal_the_batch_exactly(torch, which, name, F, graph, host_in):
    import webspeechanalyzer_amd as wsa
    cfg, pcm, fs = _signals(torch, which)
    an = wsa.Analyzer(cfg)
    spec = _spec(name)
    m = an.load_model(spec)
    steps, used = _run(torch, an, pcm, fs, F, graph, host_in, model=m)
    n = pcm.shape[0]
    got, conf = _per_stream(steps, n, spec.n_classes)
    want, rows = _batch_classes(torch, an, pcm, fs, used, m)
    assert len(want["cb"]) > 0
    _check_equal_to_batch(got, conf, want, rows, n)
    # the fold, bit-exact against the float64 restatement fed the stream's own probabilities
    for s in range(n):
        if not len(got[s]["meta"]):
            continue
        cbs, accs = classify_ref.fold_rows(np.array(got[s]["meta"]), got[s]["prob"].astype(np.float64), spec.labels, cfg["window_step"] / 1e3)
        assert [(si, nr, lab, c) for (_, si, _, nr, lab, c) in cbs] == got[s]["cbs"]
    # the labels the app's own ml5 + prediction.js gave for this excerpt (F = 1 feeds all of it; 7 frames per step cut its tail)
    if which == "config1_excerpt" and name in MODELS and F == 1:
        exp = json.load(open(os.path.join(GOLD, "classify_expected.json")))
        w = next(c for c in exp["models"][name]["clips"] if c["key"] == "config1_excerpt")["callbacks"]
        g = [c for c in got[0]["cbs"] if c[2] != -2]
        assert [c[0] for c in g] == [x["si"] for x in w]
        assert [(spec.labels[c[2]] if c[2] >= 0 else None) for c in g] == [x["pred"][0] for x in w]
    m.close(); an.close()


def test_restart_idle_and_stop_then_start(torch):
    """Four streams: 0 plays through; 1 idles, then STARTs mid-run; 2 STOPs, idles and STARTs again on the rest of its signal; 3 gets a
    START mid-run without a STOP.  Each stream's accumulator equals a fresh batch of only its post-START signal; idle steps keep it."""
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs, F = 16000, 5
    pcm = synth_clips(4, 6 * fs, fs=fs, seed=41, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=13))
    m = an.load_model(os.path.join(GOLD, "nn", MODELS[0]))
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

    steps, used = _run(torch, an, pcm, fs, F, True, False, model=m, ctl_of=ctl_of)
    confs = [c["stream_conf"].copy() for _, c in steps]
    # stream 1 has nothing before its START; stream 2's meters stay as they were while it idles
    assert not confs[k1 - 1][1].any()
    for k in range(k2a, k2b):
        assert np.array_equal(confs[k][2], confs[k2a - 1][2])
    assert confs[k2a - 1][2].any()

    for s, a, e in ((0, 0, nsteps), (1, k1, nsteps), (2, 0, k2a), (2, k2b, nsteps), (3, k3, nsteps)):
        x = pcm[s:s + 1, a * sps:e * sps].contiguous()
        b = an.batch([x.shape[1]], fs)
        b.run(x.data_ptr(), x.stride(0), _stream(torch))
        b.classify(m, _stream(torch))
        want = b.classes(_stream(torch))
        assert len(want["cb"]) > 0
        assert np.array_equal(confs[e - 1][s], want["clip_conf"][0]), (s, a, e)
        b.close()
    m.close(); an.close()


def test_rows_unchanged_by_the_model_and_reattach_recaptures(torch):
    """Rows with a model attached, after detaching, and with a model attached after steps have run (graph on) are bit-identical to a
    run without a model; the classes after a mid-run attach equal those of a run without the graph."""
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs = 16000
    pcm = synth_clips(6, 4 * fs, fs=fs, seed=29, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=13))
    m = an.load_model(os.path.join(GOLD, "nn", MODELS[0]))
    plain, _ = _run(torch, an, pcm, fs, 3, True, False)
    ns = len(plain)
    runs = [_run(torch, an, pcm, fs, 3, True, False, model=m)[0],
            _run(torch, an, pcm, fs, 3, True, False, model=m, detach_at=ns // 2)[0],
            _run(torch, an, pcm, fs, 3, True, False, model=m, attach_at=ns // 3)[0]]
    for steps in runs:
        for (a, _), (b, _) in zip(plain, steps):
            for key in ("meta", "feat", "segments"):
                assert np.array_equal(a[key], b[key], equal_nan=True), key
    eager = _run(torch, an, pcm, fs, 3, False, False, model=m, attach_at=ns // 3)[0]
    nrows = 0
    for (_, g), (_, e) in zip(runs[2], eager):
        if g is None:
            assert e is None
            continue
        for key in ("prob", "cb", "cb_label", "cb_conf", "stream_conf"):
            assert np.array_equal(g[key], e[key]), key
        nrows += len(g["prob"])
    assert nrows > 0
    m.close(); an.close()


def test_level5_probabilities_only(torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs = 16000
    pcm = synth_clips(6, 3 * fs, fs=fs, seed=4, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=5))
    m = an.load_model(os.path.join(GOLD, "nn", MODELS[0]))
    steps, used = _run(torch, an, pcm, fs, 2, True, True, model=m)
    for _, c in steps:
        assert c["cb"] is None and c["cb_label"] is None and c["stream_conf"] is None
    got, _ = _per_stream(steps, 6, m.n_classes)
    want, rows = _batch_classes(torch, an, pcm, fs, used, m)
    assert len(rows["meta"]) > 0
    _check_equal_to_batch(got, None, want, rows, 6, level=5)
    m.close(); an.close()


@pytest.mark.parametrize("level", [3, 4, 10, 11, 12])
def test_refuses_other_levels(torch, level):
    import webspeechanalyzer_amd as wsa
    an = wsa.Analyzer(wsa.Config(output_level=level))
    m = an.load_model(os.path.join(GOLD, "nn", MODELS[1]))
    st = an.streams(2, 16000)
    with pytest.raises(wsa.WsaError, match="output_level 5"):
        st.set_model(m)
    st.close(); m.close(); an.close()


def test_refuses_other_context_non_softmax_and_classes_without_a_model(torch):
    import webspeechanalyzer_amd as wsa
    an, other = wsa.Analyzer(wsa.Config(output_level=13)), wsa.Analyzer(wsa.Config(output_level=13))
    st = an.streams(2, 16000)
    m_other = other.load_model(os.path.join(GOLD, "nn", MODELS[1]))
    with pytest.raises(wsa.WsaError, match="another context"):
        st.set_model(m_other)
    s = seeded_spec(widths=(4, 4))
    lin = nnmodel.ModelSpec(s.units, ["relu", "linear"], s.kernels, s.biases, s.in_min, s.in_max, s.labels)
    m_lin = an.load_model(lin)
    with pytest.raises(wsa.WsaError, match="softmax"):
        st.set_model(m_lin)
    st.step_host(None, _stream(torch))
    st.collect(_stream(torch))
    with pytest.raises(wsa.WsaError, match="no classifier"):
        st.classes()
    st.close(); m_lin.close(); m_other.close(); an.close(); other.close()


def test_config5_and_a_step_beyond_the_d2h_window(torch):
    """512 streams at 48 kHz, one frame per graph-replayed step, model 1: the same as the batch.  Then 1200 voiced streams all
    STOPped in one step emit more rows than the 1024-row D2H window; that step's tables are complete and equal the batch's."""
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs = 48000
    an = wsa.Analyzer(wsa.Config(output_level=13))
    m = an.load_model(os.path.join(GOLD, "nn", MODELS[0]))
    hop = an.geometry(fs)["hop"]
    pcm = synth_clips(512, 80 * hop, fs=fs, seed=77, device="cuda")
    steps, used = _run(torch, an, pcm, fs, 1, True, False, model=m)
    got, conf = _per_stream(steps, 512, m.n_classes)
    want, rows = _batch_classes(torch, an, pcm, fs, used, m)
    assert len(want["cb"]) > 256
    _check_equal_to_batch(got, conf, want, rows, 512)
    del pcm, steps, got

    n, F = 1200, 80                            # one step of 2 s per stream, START and STOP in it: every row of every stream at once
    pcm = synth_clips(n, F * hop, fs=fs, seed=91, device="cuda")
    steps, used = _run(torch, an, pcm, fs, F, True, False, model=m)
    assert len(steps[-1][0]["meta"]) > 1024
    got, conf = _per_stream(steps, n, m.n_classes)
    want, rows = _batch_classes(torch, an, pcm, fs, used, m)
    last = steps[-1][1]
    assert len(last["prob"]) == len(steps[-1][0]["meta"]) and len(last["cb"]) > 0
    _check_equal_to_batch(got, conf, want, rows, n)
    m.close(); an.close()

"""K6 / K6b on the GPU: the app's dense classifier (f32 MFMA) against ml5's own outputs and the float64 restatement, the level-13
fold bit for bit against the restatement fed the device's own probabilities, the refusals, and a hipGraph capture of run + classify."""
import json
import os

import numpy as np
import pytest

from tests import classify_ref
from webspeechanalyzer_amd import nnmodel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
G = json.load(open(os.path.join(GOLD, "classify_expected.json")))
MODELS = ["1/cats_emotion", "2/cats_emotion"]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _rows():
    return np.array([r for c in G["clips"] for cb in c["callbacks"] for r in cb["feat"]], np.float64)


def _classify_rows(torch, model, feat):
    d_feat = torch.from_numpy(np.ascontiguousarray(feat, np.float64)).cuda()
    d_prob = torch.full((len(feat), model.n_classes), -1.0, dtype=torch.float32, device="cuda")
    model.classify_rows(d_feat.data_ptr(), len(feat), d_prob.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    return d_prob.cpu().numpy()


seeded_spec = classify_ref.seeded_spec


@pytest.mark.parametrize("name", MODELS)
def test_classify_rows_matches_ml5(torch, name):
    import webspeechanalyzer_amd as wsa
    an = wsa.Analyzer(wsa.Config(output_level=13))
    m = an.load_model(os.path.join(GOLD, "nn", name))
    assert m.labels == G["models"][name]["legend"]
    got = _classify_rows(torch, m, _rows())
    want = np.array(G["models"][name]["prob"])
    assert got.shape == want.shape and np.all(np.isfinite(got))
    # rows the reference produced: 1e-5.  Rows pushed far outside model_meta's ranges (logits in the hundreds) carry tfjs's own f32
    # rounding (up to 3.9e-6 from the float64 restatement, tests/test_classify_reference.py) plus ours: measured 1.09e-5 on model 1, bound 1.5e-5
    outside = np.array([c["key"].startswith("outside") for c in G["clips"] for cb in c["callbacks"] for _ in cb["feat"]])
    err = np.max(np.abs(got - want), axis=1)
    assert np.max(err[~outside]) <= 1e-5
    assert np.max(err[outside]) <= 1.5e-5
    srt = np.sort(want, axis=1)
    clear = srt[:, -1] - srt[:, -2] > 2e-5
    assert np.array_equal(np.argmax(got, 1)[clear], np.argmax(want, 1)[clear])
    m.close(); an.close()


def test_classify_rows_512_wide_against_the_restatement(torch):
    import webspeechanalyzer_amd as wsa
    spec = seeded_spec()
    rng = np.random.default_rng(9)
    feat = np.concatenate([_rows(), spec.in_min + (spec.in_max - spec.in_min) * rng.random((300, 53))])
    an = wsa.Analyzer(wsa.Config(output_level=13))
    m = an.load_model(spec)
    got = _classify_rows(torch, m, feat)
    want = classify_ref.forward(spec, feat)
    assert np.max(np.abs(got - want)) <= 1e-5
    # a row count that is not a multiple of the row tile, and a single row
    for n in (1, 17, 33):
        assert np.array_equal(_classify_rows(torch, m, feat[:n]), got[:n])
    m.close(); an.close()


def _run(torch, an, pcm, fs, resample_to=None):
    b = an.batch([pcm.shape[1]] * pcm.shape[0], fs, resample_to=resample_to)
    b.run(pcm.data_ptr(), pcm.stride(0), _stream(torch))
    return b


def _clips(torch, which):
    from webspeechanalyzer_amd.synth import synth_clips
    import webspeechanalyzer_amd as wsa
    if which == "config1_excerpt":
        exc = np.load(os.path.join(GOLD, "config1_excerpt.npz"))
        S = json.load(open(os.path.join(GOLD, "config1_expected.json")))["settings"]
        x = (exc["pcm_i16"].astype(np.float32) / np.float32(32768.0)).astype(np.float32)
        cfg = wsa.Config(output_level=13, window_step=S["window_step"], pause_length=S["pause_length"], min_seg_length=S["min_seg_length"])
        return cfg, torch.from_numpy(x).cuda()[None, :].contiguous(), int(exc["fs"]), S["fs_context"]
    return wsa.Config(output_level=13), synth_clips(12, 48000, fs=16000, seed=23, device="cuda"), 16000, None


@pytest.mark.parametrize("which", ["config1_excerpt", "synthetic"])
@pytest.mark.parametrize("name", MODELS + ["seeded_512"])
def test_batch_classify_level13_end_to_end(torch, which, name):
    import webspeechanalyzer_amd as wsa
    cfg, pcm, fs, rs = _clips(torch, which)
    an = wsa.Analyzer(cfg)
    spec = seeded_spec() if name == "seeded_512" else nnmodel.load_dir(os.path.join(GOLD, "nn", name))
    m = an.load_model(spec)
    plain = _run(torch, an, pcm, fs, rs)
    want_rows, want_spec = plain.rows(_stream(torch)), plain.spectra(_stream(torch))
    b = _run(torch, an, pcm, fs, rs)
    b.classify(m, _stream(torch))
    got = b.classes(_stream(torch))
    rows = b.rows(_stream(torch))
    # classification changes nothing of the run's own products
    for k in ("meta", "feat", "segments", "row_off", "seg_off"):
        assert np.array_equal(rows[k], want_rows[k], equal_nan=True), k
    assert all(np.array_equal(x, y) for x, y in zip(b.spectra(_stream(torch)), want_spec))
    n = len(rows["meta"])
    assert n > 0 and got["prob"].shape == (n, spec.n_classes)
    assert np.max(np.abs(got["prob"] - classify_ref.forward(spec, rows["feat"]))) <= 1e-5
    # the fold: bit-exact against the restatement fed the device's own f32 probabilities
    cbs, accs = classify_ref.fold_rows(rows["meta"], got["prob"].astype(np.float64), spec.labels, cfg["window_step"] / 1e3)
    assert len(cbs) == len(got["cb"]) and len(cbs) > 0
    for k, (clip, si, r0, nr, lab, conf) in enumerate(cbs):
        assert list(got["cb"][k]) == [clip, si, r0, nr]
        assert got["cb_label"][k] == lab
        assert got["cb_conf"][k] == conf
    assert got["clip_conf"].shape == (pcm.shape[0], spec.n_classes)
    for clip in range(pcm.shape[0]):
        acc = accs.get(clip, {})
        want = np.array([acc.get(l, 0.0) for l in spec.labels])
        assert np.array_equal(got["clip_conf"][clip], want)
    assert any(r[3] > 1 for r in got["cb"])
    b.close(); plain.close(); m.close(); an.close()


def test_batch_classify_level5_gives_probabilities_only(torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    pcm = synth_clips(6, 48000, fs=16000, seed=4, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=5))
    m = an.load_model(os.path.join(GOLD, "nn", MODELS[0]))
    b = _run(torch, an, pcm, 16000)
    b.classify(m, _stream(torch))
    got = b.classes(_stream(torch))
    rows = b.rows(_stream(torch))
    assert len(rows["meta"]) > 0 and len(got["cb"]) == 0
    assert np.max(np.abs(got["prob"] - classify_ref.forward(m.spec, rows["feat"]))) <= 1e-5
    b.close(); m.close(); an.close()


@pytest.mark.parametrize("level", [4, 10, 11, 12, 3])
def test_batch_classify_refuses_other_levels(torch, level):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    pcm = synth_clips(2, 16000, fs=16000, seed=2, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=level))
    m = an.load_model(os.path.join(GOLD, "nn", MODELS[1]))
    b = _run(torch, an, pcm, 16000)
    with pytest.raises(wsa.WsaError, match="output_level 5"):
        b.classify(m, _stream(torch))
    b.close(); m.close(); an.close()


def test_refusals_other_context_and_63_inputs_and_no_softmax(torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    pcm = synth_clips(2, 32000, fs=16000, seed=2, device="cuda")
    an, other = wsa.Analyzer(wsa.Config(output_level=13)), wsa.Analyzer(wsa.Config(output_level=13))
    m_other = other.load_model(os.path.join(GOLD, "nn", MODELS[1]))
    b = _run(torch, an, pcm, 16000)
    with pytest.raises(wsa.WsaError, match="another context"):
        b.classify(m_other, _stream(torch))
    s = seeded_spec(widths=(4, 4))
    bad = nnmodel.ModelSpec([63, 4, 4], s.activations, [np.zeros((63, 4), np.float32), s.kernels[1]], s.biases, s.in_min, s.in_max, s.labels)
    with pytest.raises(wsa.WsaError, match="63 inputs"):
        an.load_model(bad)
    lin = nnmodel.ModelSpec(s.units, ["relu", "linear"], s.kernels, s.biases, s.in_min, s.in_max, s.labels)
    m_lin = an.load_model(lin)
    with pytest.raises(wsa.WsaError, match="softmax"):
        b.classify(m_lin, _stream(torch))
    wide = seeded_spec(widths=(1040, 4))
    with pytest.raises(wsa.WsaError, match="limit 1024"):
        an.load_model(wide)
    inner = nnmodel.ModelSpec(s.units, ["softmax", "softmax"], s.kernels, s.biases, s.in_min, s.in_max, s.labels)
    with pytest.raises(wsa.WsaError, match="last layer"):
        an.load_model(inner)
    nan_range = nnmodel.ModelSpec(s.units, s.activations, s.kernels, s.biases, np.where(np.arange(53) == 7, np.nan, s.in_min), s.in_max, s.labels)
    with pytest.raises(wsa.WsaError, match="non-finite"):
        an.load_model(nan_range)
    b.close(); m_lin.close(); m_other.close(); an.close(); other.close()


def test_graph_capture_of_run_and_classify(torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs, n, ns = 16000, 16, 64000
    a = synth_clips(n, ns, fs=fs, seed=31, device="cuda")
    c = synth_clips(n, ns, fs=fs, seed=32, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=13))
    m = an.load_model(os.path.join(GOLD, "nn", MODELS[0]))
    plain = an.batch([ns] * n, fs)
    refs = []
    for x in (a, c):
        plain.run(x.data_ptr(), x.stride(0), _stream(torch))
        plain.classify(m, _stream(torch))
        refs.append(plain.classes(_stream(torch)))
    b = an.batch([ns] * n, fs)
    b.enable_timing(False)
    buf = a.clone()
    b.run(buf.data_ptr(), buf.stride(0), _stream(torch))
    b.classify(m, _stream(torch))                       # the first call allocates; the captured one does not
    b.classes(_stream(torch))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            b.run(buf.data_ptr(), buf.stride(0), side.cuda_stream)
            b.classify(m, side.cuda_stream)
        for x, ref in ((c, refs[1]), (a, refs[0]), (c, refs[1])):
            buf.copy_(x)
            g.replay()
            side.synchronize()
            got = b.classes(side.cuda_stream)
            for k in ("prob", "cb", "cb_label", "cb_conf", "clip_conf"):
                assert np.array_equal(got[k], ref[k]), k
    plain.close(); b.close(); m.close(); an.close()


def _fold_case(torch, spec, cfg, pcm, fs):
    """run + classify on `pcm`; the fold checked bit for bit against the restatement fed the device's probabilities; returns the callbacks"""
    import webspeechanalyzer_amd as wsa
    an = wsa.Analyzer(cfg)
    m = an.load_model(spec)
    b = _run(torch, an, pcm, fs)
    b.classify(m, _stream(torch))
    got = b.classes(_stream(torch))
    rows = b.rows(_stream(torch))
    cbs, accs = classify_ref.fold_rows(rows["meta"], got["prob"].astype(np.float64), spec.labels, cfg["window_step"] / 1e3)
    assert [list(r) for r in got["cb"]] == [[c[0], c[1], c[2], c[3]] for c in cbs]
    assert list(got["cb_label"]) == [c[4] for c in cbs]
    assert list(got["cb_conf"]) == [c[5] for c in cbs]
    for clip in range(pcm.shape[0]):
        assert np.array_equal(got["clip_conf"][clip], np.array([accs.get(clip, {}).get(l, 0.0) for l in spec.labels]))
    b.close(); m.close(); an.close()
    return got


def test_fold_single_syllable_callbacks(torch):
    """Short clips give segments of one syllable: the fold's one-input branch (only the top entry is added) runs, next to multi-syllable ones."""
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    pcm = synth_clips(64, 12000, fs=16000, seed=41, device="cuda")
    got = _fold_case(torch, nnmodel.load_dir(os.path.join(GOLD, "nn", MODELS[0])), wsa.Config(output_level=13), pcm, 16000)
    nsyl = got["cb"][:, 3]
    assert np.any(nsyl == 1) and np.any(nsyl > 1)


def test_fold_scans_array_index_labels_first(torch):
    """Labels '10', '2', 'x', '0' with the first two classes given identical weights: their segment sums tie, and the reference's scan over
    Object.keys (array-index keys first, ascending: '0', '2', '10', then 'x') picks '2' in a multi-syllable callback where insertion order
    (ties in legend order) would pick '10'."""
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    spec = seeded_spec(seed=7, widths=(64, 4), labels=["10", "2", "x", "0"])
    spec.kernels[1][:, 1] = spec.kernels[1][:, 0]
    spec.biases[1][:2] = 3.0
    pcm = synth_clips(12, 48000, fs=16000, seed=23, device="cuda")
    got = _fold_case(torch, spec, wsa.Config(output_level=13), pcm, 16000)
    assert np.array_equal(got["prob"][:, 0], got["prob"][:, 1])
    multi = got["cb"][:, 3] > 1
    assert np.any(got["cb_label"][multi] == 1) and not np.any(got["cb_label"][multi] == 0)
    # one syllable: only the top entry is added, and the sort puts the tie in legend order, so '10' is the only one of the two present
    assert not np.any(got["cb_label"][~multi] == 1)

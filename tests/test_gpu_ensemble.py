"""Ensembles on the GPU (wsa_ensemble_create / wsa_batch_classify_ensemble): K6e's probabilities bit for bit those of wsa_classify_rows
per member, K6b-e's per-member tables bit for bit those of wsa_batch_classify with that member alone, the cross-DB decision bit for bit
the float64 restatement (tests/ensemble_ref.py) fed the device's own probabilities, the reference's winners on the golden's rows,
level 5, the refusals, and a hipGraph capture of run + classify_ensemble."""
import json
import os

import numpy as np
import pytest

from tests import classify_ref, ensemble_ref
from webspeechanalyzer_amd import nnmodel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
G = json.load(open(os.path.join(GOLD, "classify_expected.json")))
E = json.load(open(os.path.join(GOLD, "ensemble_expected.json")))
DIRS = {1: "1/cats_emotion", 2: "2/cats_emotion"}
SIX = [1, 2, "s5", "s6", "s7", "s8"]          # the shapes of the app's six DBs: 53-256-64-16-4, 53-4-4 and four times 53-512-512-8


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
    return [loaded[k] for k in keys], list(loaded.values())


def _classify_rows(torch, model, feat):
    d_feat = torch.from_numpy(np.ascontiguousarray(feat, np.float64)).cuda()
    d_prob = torch.full((len(feat), model.n_classes), -1.0, dtype=torch.float32, device="cuda")
    model.classify_rows(d_feat.data_ptr(), len(feat), d_prob.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    return d_prob.cpu().numpy()


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


# batches of the synthetic clips whose row counts are 1, 17 and 33 (counted with the CPU oracle), and the full sets
@pytest.mark.parametrize("shape", [(1, 12000, 23, 1), (6, 32000, 24, 17), (10, 32000, 23, 33), (12, 48000, 23, 57), "config1_excerpt"])
def test_member_probabilities_are_classify_rows_bit_for_bit(torch, shape):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    if shape == "config1_excerpt":
        cfg, pcm, fs, rs = _clips(torch, shape)
        n_want = None
    else:
        n, ns, seed, n_want = shape
        # (generated on the CPU, where the counts were taken: the generator's random numbers differ between devices)
        cfg, pcm, fs, rs = wsa.Config(output_level=13), synth_clips(n, ns, fs=16000, seed=seed, device="cpu").cuda().contiguous(), 16000, None
    an = wsa.Analyzer(cfg)
    members, owned = _members(an, SIX)
    ens = an.ensemble(members)
    b = _run(torch, an, pcm, fs, rs)
    b.classify_ensemble(ens, _stream(torch))
    got = b.ensemble_classes(_stream(torch))
    rows = b.rows(_stream(torch))
    n_rows = len(rows["meta"])
    assert n_rows > 0 and (n_want is None or n_rows == n_want)
    for d, m in enumerate(members):
        assert got["prob"][d].shape == (n_rows, m.n_classes)
        assert np.array_equal(got["prob"][d], _classify_rows(torch, m, rows["feat"])), f"member {d}"
    b.close(); ens.close()
    for m in owned:
        m.close()
    an.close()


def _check_decision(got, rows, legends, step_s, n_clips):
    """every table of the ensemble result against the restatement fed the device's own probabilities, bit for bit"""
    want = ensemble_ref.fold_rows(rows["meta"], [p.astype(np.float64) for p in got["prob"]], legends, step_s)
    k = len(want["cb"])
    assert k > 0 and [list(r) for r in got["cb"]] == [list(c) for c in want["cb"]]
    for d in range(len(legends)):
        assert list(got["cb_label"][d]) == want["cb_label"][d], d
        assert list(got["cb_conf"][d]) == want["cb_conf"][d], d
        assert list(got["cb_all_max"][d]) == want["cb_all_max"][d], d
        for clip in range(n_clips):
            acc = want["clip_conf"].get(clip, [{}] * len(legends))[d]
            assert np.array_equal(got["clip_conf"][d][clip], np.array([acc.get(l, 0.0) for l in legends[d]])), (d, clip)
    for name in ("cb_db", "cb_top_label", "cb_top_conf", "cb_min_db"):
        assert list(got[name]) == want[name], name
    assert np.array_equal(got["cb_entropy"], np.array(want["cb_entropy"]), equal_nan=True)
    assert list(got["clip_min_db"]) == [want["clip_min_db"].get(c, -1) for c in range(n_clips)]
    return want


@pytest.mark.parametrize("which", ["config1_excerpt", "synthetic"])
@pytest.mark.parametrize("keys", [[1, 2], [2, 1], SIX], ids=["1_2", "2_1", "six"])
def test_per_member_fold_and_decision(torch, which, keys):
    import webspeechanalyzer_amd as wsa
    cfg, pcm, fs, rs = _clips(torch, which)
    an = wsa.Analyzer(cfg)
    members, owned = _members(an, keys)
    ens = an.ensemble(members)
    b = _run(torch, an, pcm, fs, rs)
    plain_rows = b.rows(_stream(torch))
    # each member alone, on the same batch
    single = []
    for m in members:
        b.classify(m, _stream(torch))
        single.append(b.classes(_stream(torch)))
    b.classify_ensemble(ens, _stream(torch))
    got = b.ensemble_classes(_stream(torch))
    rows = b.rows(_stream(torch))
    for key in ("meta", "feat", "segments", "row_off", "seg_off"):
        assert np.array_equal(rows[key], plain_rows[key], equal_nan=True), key
    for d, s in enumerate(single):
        assert np.array_equal(got["cb"], s["cb"])
        for a, c in (("prob", "prob"), ("cb_label", "cb_label"), ("cb_conf", "cb_conf"), ("clip_conf", "clip_conf")):
            assert np.array_equal(got[a][d], s[c]), (d, a)
    want = _check_decision(got, rows, [m.labels for m in members], cfg["window_step"] / 1e3, pcm.shape[0])
    assert any(r[3] > 1 for r in got["cb"])
    assert all(0 <= v < len(keys) for v in want["cb_db"])
    if keys == [1, 2]:
        # the single-model entry points, after the ensemble call: unchanged by one bit, and the two results stay separate
        with pytest.raises(wsa.WsaError, match="ensemble"):
            b.classes(_stream(torch))
        b.classify(members[1], _stream(torch))
        again = b.classes(_stream(torch))
        for key in ("prob", "cb", "cb_label", "cb_conf", "clip_conf"):
            assert np.array_equal(again[key], single[1][key]), key
        with pytest.raises(wsa.WsaError, match="one model"):
            b.ensemble_classes(_stream(torch))
    b.close(); ens.close()
    for m in owned:
        m.close()
    an.close()


def test_the_references_winners_on_the_goldens_rows(torch):
    """[1, 2] on the 135 rows of the fixture, classified on the device per member and decided by the restatement: all 43 callbacks give
    the label the application's prediction.js gave with available_DBs = [1, 2], and the DB whose own prediction that pair is."""
    import webspeechanalyzer_amd as wsa
    an = wsa.Analyzer(wsa.Config(output_level=13))
    members, owned = _members(an, [1, 2])
    feat = np.array([r for c in G["clips"] for cb in c["callbacks"] for r in cb["feat"]], np.float64)
    probs = [_classify_rows(torch, m, feat).astype(np.float64) for m in members]
    case = E["cases"][0]
    assert case["dbs"] == [1, 2]
    legends = [m.labels for m in members]
    assert legends == [E["legend"]["1"], E["legend"]["2"]]
    row, n, wins = 0, 0, [0, 0]
    for ck, (clip, wclip) in enumerate(zip(G["clips"], case["clips"])):
        L = ensemble_ref.Launch(legends)
        for k, (cb, w) in enumerate(zip(clip["callbacks"], wclip["callbacks"])):
            nr = len(cb["feat"])
            r = L.callback([float(t[1]) for t in cb["seg_time"]], [p[row:row + nr] for p in probs])
            row += nr
            single = [G["models"][DIRS[d]]["clips"][ck]["callbacks"][k]["pred"] for d in (1, 2)]
            want_db = 0 if single[0][1] >= single[1][1] else 1
            assert single[want_db] == w["pred"]
            assert r["label"] == w["pred"][0], (ck, k)
            assert r["db"] == want_db, (ck, k)
            # K6's bound per probability (1.5e-5, tests/test_gpu_classify.py) through the fold: a label's sum is sum p sqrt(d), the
            # confidence that sum over sum d, and two maxima differ by no more than their terms do
            durs = [float(t[1]) for t in cb["seg_time"]]
            assert abs(r["conf"] - w["pred"][1]) <= 1.5e-5 * sum(np.sqrt(durs)) / sum(durs) + 1e-12
            wins[want_db] += 1
            n += 1
    assert n == 43 and wins[0] > 0 and wins[1] > 0
    for m in owned:
        m.close()
    an.close()


def test_identical_members_tie_to_the_first_and_a_model_may_appear_twice(torch):
    import webspeechanalyzer_amd as wsa
    cfg, pcm, fs, rs = _clips(torch, "synthetic")
    an = wsa.Analyzer(cfg)
    members, owned = _members(an, [2, 2, 1])
    assert members[0] is members[1]
    ens = an.ensemble(members)
    b = _run(torch, an, pcm, fs, rs)
    b.classify_ensemble(ens, _stream(torch))
    got = b.ensemble_classes(_stream(torch))
    rows = b.rows(_stream(torch))
    assert np.array_equal(got["prob"][0], got["prob"][1]) and np.array_equal(got["cb_conf"][0], got["cb_conf"][1])
    assert not np.any(got["cb_db"] == 1) and not np.any(got["cb_min_db"] == 1) and np.any(got["cb_db"] == 0)
    _check_decision(got, rows, [m.labels for m in members], cfg["window_step"] / 1e3, pcm.shape[0])
    b.close(); ens.close()
    for m in owned:
        m.close()
    an.close()


def test_level5_gives_probabilities_only(torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    pcm = synth_clips(6, 48000, fs=16000, seed=4, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=5))
    members, owned = _members(an, [1, "s5", 2])
    ens = an.ensemble(members)
    b = _run(torch, an, pcm, 16000)
    b.classify_ensemble(ens, _stream(torch))
    got = b.ensemble_classes(_stream(torch))
    r = b.ensemble_result(_stream(torch))
    rows = b.rows(_stream(torch))
    assert len(rows["meta"]) > 0 and int(r.n_callbacks) == 0 and not r.d_cb and not r.d_cb_db and not r.d_cb_label[0] and not r.d_clip_conf[0]
    assert "cb" not in got
    for d, m in enumerate(members):
        assert np.array_equal(got["prob"][d], _classify_rows(torch, m, rows["feat"]))
    b.close(); ens.close()
    for m in owned:
        m.close()
    an.close()


def test_refusals(torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    pcm = synth_clips(2, 32000, fs=16000, seed=2, device="cuda")
    an, other = wsa.Analyzer(wsa.Config(output_level=13)), wsa.Analyzer(wsa.Config(output_level=13))
    m1 = an.load_model(_spec(1))
    m_other = other.load_model(_spec(2))
    with pytest.raises(wsa.WsaError, match="1 .. 8 members"):
        an.ensemble([])
    with pytest.raises(wsa.WsaError, match="1 .. 8 members"):
        an.ensemble([m1] * 9)
    with pytest.raises(wsa.WsaError, match="member 1 is NULL"):
        an.ensemble([m1, None])
    with pytest.raises(wsa.WsaError, match="member 1 was created on another context"):
        an.ensemble([m1, m_other])
    an.ensemble([m1] * 8).close()
    b = _run(torch, an, pcm, 16000)
    with pytest.raises(wsa.WsaError, match="no wsa_batch_classify_ensemble"):
        b.ensemble_result(_stream(torch))
    e_other = other.ensemble([m_other])
    with pytest.raises(wsa.WsaError, match="another context"):
        b.classify_ensemble(e_other, _stream(torch))
    s = classify_ref.seeded_spec(widths=(4, 4))
    m_lin = an.load_model(nnmodel.ModelSpec(s.units, ["relu", "linear"], s.kernels, s.biases, s.in_min, s.in_max, s.labels))
    e_lin = an.ensemble([m1, m_lin])
    with pytest.raises(wsa.WsaError, match="softmax"):
        b.classify_ensemble(e_lin, _stream(torch))
    b.classify(m1, _stream(torch))
    with pytest.raises(wsa.WsaError, match="no wsa_batch_classify_ensemble"):
        b.ensemble_result(_stream(torch))
    b.close()
    for level in (4, 10, 11, 12, 3):
        an_l = wsa.Analyzer(wsa.Config(output_level=level))
        m_l = an_l.load_model(_spec(2))
        e_l = an_l.ensemble([m_l])
        b_l = _run(torch, an_l, pcm, 16000)
        with pytest.raises(wsa.WsaError, match="output_level 5"):
            b_l.classify_ensemble(e_l, _stream(torch))
        b_l.close(); e_l.close(); m_l.close(); an_l.close()
    e_lin.close(); e_other.close(); m_lin.close(); m1.close(); m_other.close(); an.close(); other.close()


def test_copy_ensemble_checks_capacities(torch):
    import ctypes
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd import capi
    cfg, pcm, fs, rs = _clips(torch, "synthetic")
    an = wsa.Analyzer(cfg)
    members, owned = _members(an, [1, 2])
    ens = an.ensemble(members)
    b = _run(torch, an, pcm, fs, rs)
    b.classify_ensemble(ens, _stream(torch))
    r = b.ensemble_result(_stream(torch))
    n, k = int(r.n_rows), int(r.n_callbacks)
    assert n > 1 and k > 1
    prob, lab = np.zeros((n, 4), np.float32), np.zeros(k, np.int32)
    h = capi._EnsembleHost()
    h.rows_cap, h.cb_cap = n - 1, k
    h.prob[1] = prob.ctypes.data
    with pytest.raises(wsa.WsaError, match="probability buffer too small"):
        an._check(an.L.wsa_batch_copy_ensemble(b.h, _stream(torch), ctypes.byref(h)))
    h.rows_cap, h.cb_cap = n, k - 1
    h.cb_db = lab.ctypes.data
    with pytest.raises(wsa.WsaError, match="callback buffer too small"):
        an._check(an.L.wsa_batch_copy_ensemble(b.h, _stream(torch), ctypes.byref(h)))
    h.cb_cap = k
    an._check(an.L.wsa_batch_copy_ensemble(b.h, _stream(torch), ctypes.byref(h)))
    full = b.ensemble_classes(_stream(torch))
    assert np.array_equal(prob, full["prob"][1]) and np.array_equal(lab, full["cb_db"])
    b.close(); ens.close()
    for m in owned:
        m.close()
    an.close()


def test_graph_capture_of_run_and_classify_ensemble(torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    fs, n, ns = 16000, 16, 64000
    a = synth_clips(n, ns, fs=fs, seed=31, device="cuda")
    c = synth_clips(n, ns, fs=fs, seed=32, device="cuda")
    an = wsa.Analyzer(wsa.Config(output_level=13))
    members, owned = _members(an, [1, 2, "s5"])
    ens = an.ensemble(members)
    per_member = ("prob", "cb_label", "cb_conf", "cb_all_max", "clip_conf")
    shared = ("cb", "cb_db", "cb_top_label", "cb_top_conf", "cb_min_db", "cb_entropy", "clip_min_db")
    plain = an.batch([ns] * n, fs)
    refs = []
    for x in (a, c):
        plain.run(x.data_ptr(), x.stride(0), _stream(torch))
        plain.classify_ensemble(ens, _stream(torch))
        refs.append(plain.ensemble_classes(_stream(torch)))
    assert not np.array_equal(refs[0]["cb_top_conf"], refs[1]["cb_top_conf"])
    b = an.batch([ns] * n, fs)
    b.enable_timing(False)
    buf = a.clone()
    b.run(buf.data_ptr(), buf.stride(0), _stream(torch))
    b.classify_ensemble(ens, _stream(torch))                       # the first call allocates; the captured one does not
    b.ensemble_classes(_stream(torch))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            b.run(buf.data_ptr(), buf.stride(0), side.cuda_stream)
            b.classify_ensemble(ens, side.cuda_stream)
        for x, ref in ((c, refs[1]), (a, refs[0]), (c, refs[1])):
            buf.copy_(x)
            g.replay()
            side.synchronize()
            got = b.ensemble_classes(side.cuda_stream)
            for key in per_member:
                for d in range(len(members)):
                    assert np.array_equal(got[key][d], ref[key][d]), (key, d)
            for key in shared:
                assert np.array_equal(got[key], ref[key], equal_nan=True), key
    plain.close(); b.close(); ens.close()
    for m in owned:
        m.close()
    an.close()

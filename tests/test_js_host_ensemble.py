"""The Node host with all of the app's model DBs (js/formantanalyzer.js setPredictionModels over the addon's processBatch([models]) and
streamSetEnsemble): on_prediction's [label, confidence] against what the reference's own prediction.js produced with available_DBs = [1, 2]
for the config-1 excerpt (tests/golden/ensemble_expected.json), over LaunchBatch and over StreamOpen; detail.db / min_entropy_db / entropy /
meters against the device tables read through the Python binding; min_entropy_db carried across launches; setPredictionModel as before."""
import json
import os
import shutil
import subprocess
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NODE = shutil.which("node")
DRIVER = os.path.join(ROOT, "tests", "js", "ensemble_host.js")
MODELS = [os.path.join(GOLD, "nn", "1", "cats_emotion"), os.path.join(GOLD, "nn", "2", "cats_emotion")]
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "napi")], check=True)
    return torch


@pytest.fixture(scope="module")
def run(torch, tmp_path_factory):
    """one drive of the Node host, and the device tables of the same clip through the Python binding"""
    import webspeechanalyzer_amd as wsa
    tmp = tmp_path_factory.mktemp("ens")
    S = json.load(open(os.path.join(GOLD, "config1_expected.json")))["settings"]
    exc = np.load(os.path.join(GOLD, "config1_excerpt.npz"))
    wav = str(tmp / "excerpt.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(int(exc["fs"])); w.writeframes(exc["pcm_i16"].astype("<i2").tobytes())
    cfg = dict(output_level=13, window_step=S["window_step"], pause_length=S["pause_length"], min_seg_length=S["min_seg_length"])
    x = (exc["pcm_i16"].astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    an = wsa.Analyzer(wsa.Config(**cfg))
    ms = [an.load_model(m) for m in MODELS]
    ens = an.ensemble(ms)
    st = torch.cuda.current_stream().cuda_stream
    b = an.batch([len(x)], int(exc["fs"]), resample_to=S["fs_context"])
    src = torch.from_numpy(x).cuda()[None, :].contiguous()
    b.run(src.data_ptr(), src.stride(0), st)
    b.classify_ensemble(ens, st)
    py = b.ensemble_classes(st)
    pcm48 = b.converted_pcm(st)[0]
    b.close(); ens.close()
    for m in ms:
        m.close()
    an.close()
    f48, fsil = tmp / "x48k.f32", tmp / "silent.f32"
    pcm48.astype(np.float32).tofile(f48)
    np.zeros(int(S["fs_context"]), np.float32).tofile(fsil)
    job = dict(wav=wav, pcm48=str(f48), fs48=int(S["fs_context"]), silent=str(fsil), settings=dict(cfg, resample_to=S["fs_context"]), models=MODELS)
    jp = tmp / "job.json"
    jp.write_text(json.dumps(job))
    r = subprocess.run([NODE, DRIVER, str(jp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout), py


def _num(v):
    return float(v) if isinstance(v, str) else v


def _golden():
    E = json.load(open(os.path.join(GOLD, "ensemble_expected.json")))
    C = json.load(open(os.path.join(GOLD, "classify_expected.json")))
    case = E["cases"][0]
    assert case["dbs"] == [1, 2]
    k = next(i for i, c in enumerate(C["clips"]) if c["key"] == "config1_excerpt")
    return case["clips"][k]["callbacks"], C["clips"][k]["callbacks"]


@pytest.mark.parametrize("path", ["batch", "stream"])
def test_on_prediction_gives_the_references_pairs(run, path):
    got, _ = run
    want, inputs = _golden()
    preds = got[path]["preds"]
    if path == "stream":                       # (whole steps only: the excerpt's tail may be cut; what is delivered is the batch's of the same samples)
        assert [(p["si"], p["pred"], p["detail"]) for p in preds] == [(p["si"], p["pred"], p["detail"]) for p in got["batch48"]["preds"]]
        assert got["stream"]["meters"] == got["batch48"]["meters"] and got["stream"]["min_entropy_db"] == got["batch48"]["min_entropy_db"]
        want, inputs = want[:len(preds)], inputs[:len(preds)]
        assert len(preds) >= len(_golden()[0]) - 1
    else:
        assert got["batch"]["callbacks"] == [w["si"] for w in want]
        assert [p["after"] for p in preds] == list(range(1, len(want) + 1))       # right after the segment's own callback
    assert [p["si"] for p in preds] == [w["si"] for w in want]
    for p, w, cb in zip(preds, want, inputs):
        assert p["pred"][0] == w["pred"][0]
        # K6's bound on the rows the reference produced (1e-5 per probability, tests/test_gpu_classify.py) through the fold: a label's sum is
        # sum p sqrt(d), the confidence that sum over sum d, and two maxima differ by no more than their terms do
        durs = [float(t[1]) for t in cb["seg_time"]]
        assert abs(p["pred"][1] - w["pred"][1]) <= 1e-5 * sum(np.sqrt(durs)) / sum(durs) + 1e-12
        assert [1, 2][p["detail"]["min_entropy_db"]] == w["min_entropy_db"]
        assert [k for k, _ in p["detail"]["meters"]] == [k for k, _ in w["gauges"]]
        # a gauge is a / S, a label's sum over the launch's sum.  With every probability within e = 1e-5 and W the sum of the weights so
        # far, |da| <= e W and |dS| <= C e W (C = 4 classes), and S >= W / C (a one-syllable callback adds only its top entry, at least
        # 1 / C), so |d(a / S)| <= (|da| + |dS|) / S <= e (1 + C) C = 2e-4; the entropy is 1 - the largest gauge, printed to three decimals
        for (_, a), (_, b) in zip(p["detail"]["meters"], w["gauges"]):
            assert abs(a - b) <= 2e-4
        assert abs(p["detail"]["entropy"] - float(w["entropy_text"])) <= 0.0005 + 2e-4


def test_detail_matches_the_device_tables(run):
    got, py = run
    preds = got["batch"]["preds"]
    labels = py["labels"]
    assert len(preds) == len(py["cb"]) > 1
    for k, p in enumerate(preds):
        d = p["detail"]
        db = int(py["cb_db"][k])
        assert d["db"] == db and db >= 0
        assert p["pred"] == [labels[db][py["cb_top_label"][k]], float(py["cb_top_conf"][k])]
        assert d["min_entropy_db"] == int(py["cb_min_db"][k])
        assert d["entropy"] == float(py["cb_entropy"][k])
        for m in range(2):
            lab, conf, nsyl = d["per_db"][m]
            assert lab == labels[m][py["cb_label"][m][k]] and conf == float(py["cb_conf"][m][k]) and nsyl == int(py["cb"][k][3])
        shares = [v for _, v in d["meters"]]
        assert abs(sum(shares) - 1.0) <= 1e-12 and abs(max(shares) - (1.0 - d["entropy"])) <= 1e-12
    # after the clip's last callback the gauges are the device's per-clip accumulator of the clip's min_entropy_db
    m = int(py["clip_min_db"][0])
    acc = {l: float(v) for l, v in zip(labels[m], py["clip_conf"][m][0]) if v != 0}
    last = dict(preds[-1]["detail"]["meters"])
    assert set(last) == set(acc)
    total = sum(acc.values())
    for l in acc:
        assert abs(last[l] - acc[l] / total) <= 1e-12
    assert got["batch"]["meters"] == [preds[-1]["detail"]["meters"]] and got["batch"]["min_entropy_db"] == [m]


def test_min_entropy_db_is_carried_across_launches(run):
    got, py = run
    m = int(py["clip_min_db"][0])
    assert got["batch"]["shown"] == m and got["second"]["shown"] == m
    assert got["second"]["preds"] == got["batch"]["preds"]
    # a launch without a callback: no prediction, no DB of its own, empty gauges; the DB on show is still the earlier launch's
    assert got["silent"] == dict(npreds=0, meters=[[]], min_entropy_db=[None], shown=m)
    # the members the other way round: the same DBs under the other index
    assert [p["detail"]["min_entropy_db"] for p in got["reversed"]["preds"]] == [1 - p["detail"]["min_entropy_db"] for p in got["batch"]["preds"]]
    assert [p["pred"][0] for p in got["reversed"]["preds"]] == [p["pred"][0] for p in got["batch"]["preds"]]
    assert got["reversed"]["shown"] == 1 - m


def test_set_prediction_model_is_unchanged_beside_it(run):
    got, py = run
    before, after = got["single"]["before"], got["single"]["after"]
    assert before == after and len(before["preds"]) == len(py["cb"])
    assert before["extra"] == [True, True]
    assert [p[1] for p in before["preds"]] == [py["labels"][0][i] for i in py["cb_label"][0]]
    assert [p[2] for p in before["preds"]] == [float(v) for v in py["cb_conf"][0]]
    assert before["meters"][0] == {l: float(v) for l, v in zip(py["labels"][0], py["clip_conf"][0][0])}


def test_refusals(run):
    got, _ = run
    r = got["refusals"]
    assert "1 .. 8" in r["empty"] and "1 .. 8" in r["nine"] and "not one of loadModel" in r["not_a_handle"] and "on_prediction" in r["no_callback"]

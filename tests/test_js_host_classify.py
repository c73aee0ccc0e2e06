"""The Node host's classifier (js/formantanalyzer.js loadModel / setPredictionModel / on_prediction over the addon's modelCreate and
processBatch): on_prediction against what the reference's own prediction.js produced for the same rows (tests/golden/classify_expected.json)
and against the Python binding's fold, the meters on the resolved result, an unchanged callback stream without a model, and handles refused
after shutdown() / destroy()."""
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
DRIVER = os.path.join(ROOT, "tests", "js", "classify_host.js")
MODEL1 = os.path.join(GOLD, "nn", "1", "cats_emotion")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "napi")], check=True)
    return torch


def _drive(tmp_path, job):
    jp = tmp_path / "job.json"
    jp.write_text(json.dumps(job))
    r = subprocess.run([NODE, DRIVER, str(jp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_on_prediction_equals_prediction_js_on_the_sample_file_excerpt(torch, tmp_path):
    import webspeechanalyzer_amd as wsa
    exp = json.load(open(os.path.join(GOLD, "classify_expected.json")))
    c1 = json.load(open(os.path.join(GOLD, "config1_expected.json")))
    S = c1["settings"]
    exc = np.load(os.path.join(GOLD, "config1_excerpt.npz"))
    wav = str(tmp_path / "excerpt.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(int(exc["fs"])); w.writeframes(exc["pcm_i16"].astype("<i2").tobytes())
    settings = dict(output_level=13, resample_to=S["fs_context"], window_step=S["window_step"], pause_length=S["pause_length"], min_seg_length=S["min_seg_length"])
    got = _drive(tmp_path, dict(mode="excerpt", wav=wav, settings=settings, model=MODEL1))
    assert got["resolved"] is True
    want = next(c for c in exp["models"]["1/cats_emotion"]["clips"] if c["key"] == "config1_excerpt")["callbacks"]
    assert [p["si"] for p in got["preds"]] == [w["si"] for w in want] == got["callbacks"]
    for k, (p, w) in enumerate(zip(got["preds"], want)):
        assert p["after"] == k + 1                                   # right after the segment's own callback
        assert p["pred"][0] == w["pred"][0]
        assert p["pred"][1] == pytest.approx(w["pred"][1], rel=1e-6, abs=0)
        # per_syllable has classifyMultiple's shape (one syllable: its sorted list itself) and its confidences
        one = isinstance(w["ml5"][0], dict)
        assert isinstance(p["per"][0], dict) == one
        for gs, ws in ([(p["per"], w["ml5"])] if one else zip(p["per"], w["ml5"])):
            assert len(gs) == len(ws) == 4 and all(set(e) == {e["label"], "label", "confidence"} for e in gs)
            wd = {e["label"]: e["confidence"] for e in ws}
            assert all(abs(e["confidence"] - wd[e["label"]]) <= 1e-5 for e in gs)
            assert all(gs[i]["confidence"] >= gs[i + 1]["confidence"] for i in range(3))
    # bit-equal to the Python binding's fold on the same clip
    x = (exc["pcm_i16"].astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    an = wsa.Analyzer(wsa.Config(output_level=13, window_step=S["window_step"], pause_length=S["pause_length"], min_seg_length=S["min_seg_length"]))
    m = an.load_model(MODEL1)
    pcm = torch.from_numpy(x).cuda()[None, :].contiguous()
    b = an.batch([len(x)], int(exc["fs"]), resample_to=S["fs_context"])
    st = torch.cuda.current_stream().cuda_stream
    b.run(pcm.data_ptr(), pcm.stride(0), st)
    b.classify(m, st)
    py = b.classes(st)
    assert [p["pred"][1] for p in got["preds"]] == list(py["cb_conf"])
    assert [p["pred"][0] for p in got["preds"]] == [m.labels[i] for i in py["cb_label"]]
    assert got["meters"][0] == {l: float(v) for l, v in zip(m.labels, py["clip_conf"][0])}
    b.close(); m.close(); an.close()


def test_callback_stream_unchanged_with_and_without_a_model(torch, tmp_path):
    from webspeechanalyzer_amd.synth import synth_clips
    pcm = synth_clips(6, 48000, fs=16000, seed=23).numpy()
    files = []
    for i, c in enumerate(pcm):
        f = tmp_path / f"c{i}.f32"; c.astype(np.float32).tofile(f); files.append(str(f))
    got = _drive(tmp_path, dict(mode="stream", clips=files, fs=16000, settings=dict(output_level=13), model=MODEL1))
    assert got["before"]["stream"] == got["with_model"]["stream"] == got["after"]["stream"]
    assert got["before"]["resolved"] == got["with_model"]["resolved"] == got["after"]["resolved"]
    assert got["before"]["meters"] is None and got["after"]["meters"] is None and len(got["with_model"]["meters"]) == 6
    n_cb = len(json.loads(got["before"]["stream"]))
    assert len(got["preds"]) == n_cb > 0
    assert any(p[4] == 1 for p in got["preds"]) or any(p[4] > 1 for p in got["preds"])


def test_model_handles_are_refused_after_shutdown_and_destroy(torch, tmp_path):
    got = _drive(tmp_path, dict(mode="release", model=MODEL1))
    assert "released" in got["after_shutdown"]
    assert "destroyed" in got["after_destroy"] or "processBatch" in got["after_destroy"]
    assert "destroyed" in got["destroyed_model"]
    assert "another context" in got["other_ctx"]

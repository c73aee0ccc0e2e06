"""The Node host's KNN classifier (js/formantanalyzer.js KNNClassifier / trainKnn / predictKnn over the addon's knnCreate, knnAdd,
knnClassify and batchKnn; js/knn.js): one fixture case of tests/golden/knn_expected.json gives ml5's labels, confidences and neighbour
sets, trainKnn gives the app's train_knn figure, and batchKnn over a processed batch equals knnClassify over the rows it handed out."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import knn_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NODE = shutil.which("node")
DRIVER = os.path.join(ROOT, "tests", "js", "knn_host.js")
FIXTURE = json.load(open(os.path.join(GOLD, "knn_expected.json")))
CASE = "keyorder_num"            # number labels: 7, 2 and 3 arrive after 10 and sort in front of it, so the host has to renumber
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "napi")], check=True)
    return torch


def _db_rows(rows, labels):
    """the rows of a data_<db>.json file (js/featuredb.js): the label in the categorical half of the `true` pair"""
    return [dict(file=f"f{i}.wav", seg="0", time=[0, 1], features=[float(v) for v in r], origin=None,
                 true=None if lab is None else [{"emotion": lab}, {}], pred=None) for i, (r, lab) in enumerate(zip(rows, labels))]


def test_node_host_gives_ml5s_results_and_the_apps_figure(torch, tmp_path):
    from webspeechanalyzer_amd.synth import synth_clips
    c = FIXTURE["cases"][CASE]
    b = knn_cases.build(CASE, c["seed"])
    evals = []
    for variant, e in FIXTURE["evals"].items():
        rows, labels = knn_cases.eval_db(e["seed"])
        evals.append(dict(key=variant, rows=_db_rows(rows, labels), label="emotion", classes=e["classes"], k=knn_cases.EVAL_K))
    few, labels = knn_cases.eval_db(1)
    evals.append(dict(key="too_few", rows=_db_rows(few[:11], labels[:11]), label="emotion", classes=["*"], k=10))
    files = []
    for i, clip in enumerate(synth_clips(4, 48000, fs=16000, seed=23).numpy()):
        f = tmp_path / f"c{i}.f32"; clip.astype(np.float32).tofile(f); files.append(str(f))
    job = dict(settings=dict(output_level=5), case=dict(store=b["store"].tolist(), labels=b["labels"], queries=b["queries"].tolist(), ks=b["ks"], split=1),
               eval=evals, clips=files, fs=16000)
    jp = tmp_path / "job.json"
    jp.write_text(json.dumps(job))
    r = subprocess.run([NODE, DRIVER, str(jp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    assert got["classes_at_split"] == ["10"] and got["classes"] == c["class_names"] == ["2", "3", "7", "10"]
    assert got["counts"] == {"2": 10, "3": 10, "7": 10, "10": 10}
    for k in b["ks"]:
        for q, (g, want) in enumerate(zip(got["results"][str(k)], (res[str(k)] for res in c["results"]))):
            assert g["label"] == want["label"] and g["classIndex"] == int(want["label"]), (k, q)
            assert g["conf"] == want["conf"] and g["byId"] == dict(zip(c["class_keys"], want["conf"])), (k, q)
            assert sorted(g["nbr"]) == sorted(want["nbr"]), (k, q)
    assert got["one"]["label"] == c["results"][0][str(b["ks"][0])]["label"]
    for variant, e in FIXTURE["evals"].items():
        assert got["evals"][variant] == dict(samples=e["samples"], correct=e["correct"], all=e["all"]), variant
    assert got["evals"]["too_few"] == dict(refused="Sample size 8/11 too small for training")
    assert got["batch"]["rows"] > 0 and got["batch"]["same"] is True
    assert "no example" in got["refusals"]["empty"] and "released" in got["refusals"]["released"]

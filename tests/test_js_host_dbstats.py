"""The Node host's DB prediction and results table (js/formantanalyzer.js predictDB / statsTable over the addon's dbPredict / dbTable) on fixture
scenario (a): the text the reference application printed, the `pred` pairs, and the pred_<name> columns of FeatureDB's CSV export."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webspeechanalyzer_amd import nnmodel

from . import dbstats_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
DRIVER = os.path.join(ROOT, "tests", "js", "dbstats_host.js")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]
FX = dc.load_fixture()


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "napi")], check=True)
    tmp = tmp_path_factory.mktemp("jsdbstats")
    nnmodel.save_dir(dc.model_spec("ords_V"), str(tmp / "1" / "ords_V"))
    sc = FX["scenarios"]["a"]
    job = dict(rows=sc["rows"], class_labels=sc["class_labels"], ordinal_labels=sc["ordinal_labels"], settings=dict(output_level=13),
               predict=[dict(type="cats", label="emotion", modelDir=os.path.join(dc.GOLD, "nn", "1", "cats_emotion")),
                        dict(type="ords", label="V", modelDir=str(tmp / "1" / "ords_V"))])
    (tmp / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, DRIVER, str(tmp / "job.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout), sc


def test_lines_are_the_references(run):
    js, sc = run
    assert js["lines"] == sc["lines"]


def test_predictions_and_pred_pairs(run):
    js, sc = run
    cats_run, ords_run = sc["ml5"]
    assert js["preds"][0] == [res[0]["label"] for res in cats_run["results"]]
    spec = dc.model_spec("ords_V")
    assert np.abs(np.array(js["preds"][1]) - np.array(ords_run["results"])).max() <= dc.VALUE_TOL * (spec.out_max - spec.out_min)
    stored = json.loads(js["json"])
    assert [r["pred"][0] for r in stored] == [p[0] for p in sc["pred_after"]]
    assert [r["pred"][1]["V"] for r in stored] == js["preds"][1]


def test_csv_carries_the_pred_columns(run):
    js, sc = run
    lines = js["csv"].split("\r\n")
    header = lines[0].split(",")
    assert "pred_emotion" in header and "pred_V" in header
    ie, iv = header.index("pred_emotion"), header.index("pred_V")
    cells = [ln.split(",") for ln in lines[1:] if ln]
    assert [c[ie] for c in cells] == js["preds"][0]
    assert [float(c[iv]) for c in cells] == js["preds"][1]


def test_refusals(run):
    js, _ = run
    assert "needs a regression model" in js["refusals"]["kind"]
    assert "no data for prediction" in js["refusals"]["empty"]

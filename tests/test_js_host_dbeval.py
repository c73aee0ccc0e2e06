"""The Node host's evaluation of a labelled DB (js/formantanalyzer.js evaluateDB over the addon's dbEval, js/dbstats.js) on one small case:
the structure it returns — tables, confusion matrices with recall / precision / UAR, agreements, per-file sums, classes and values, the
text lines — equals what webspeechanalyzer_amd.dbstats.evaluate returns for the same rows and models, number for number."""
import copy
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from webspeechanalyzer_amd import capi, dbstats, nnmodel

from . import dbstats_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
DRIVER = os.path.join(ROOT, "tests", "js", "dbeval_host.js")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]
CLASS_LABELS, ORDINAL_LABELS = [{"emotion": ["N", "A", "S", "H"]}, {"sex": ["M", "F"]}], ["V"]


def _rows():
    """fixture scenario (a): 10 files of 5 rows; the part tags rewritten so that a file has callbacks of two, two and one syllable, one
    row without a file, and stored predictions for the head that gets no model"""
    rows = copy.deepcopy(dc.load_fixture()["scenarios"]["a"]["rows"])
    for i, r in enumerate(rows):
        r["seg"] = ("0", "0.01", "1", "1.01", "2")[i % 5]
        r["pred"] = [{"sex": ("M", "F", None)[i % 3]}, {}]
    rows[7]["file"] = ""
    return rows


def _plain(x):
    """numpy and NaN out of the way: what JSON can hold, as the driver writes it"""
    if isinstance(x, dict):
        return {str(k): _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple, np.ndarray)):
        return [_plain(v) for v in x]
    if isinstance(x, (np.integer,)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        x = float(x)
        return "NaN" if x != x else ("Infinity" if x > 0 else "-Infinity") if math.isinf(x) else x
    return x


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "napi")], check=True)
    tmp = tmp_path_factory.mktemp("jsdbeval")
    nnmodel.save_dir(dc.model_spec("ords_V"), str(tmp / "1" / "ords_V"))
    models = dict(emotion=os.path.join(dc.GOLD, "nn", "1", "cats_emotion"), V=str(tmp / "1" / "ords_V"))
    job = dict(rows=_rows(), class_labels=CLASS_LABELS, ordinal_labels=ORDINAL_LABELS, settings=dict(output_level=13), models=models)
    (tmp / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, DRIVER, str(tmp / "job.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    an = capi.Analyzer(capi.Config(output_level=13), device=0)
    rows = _rows()
    want = dbstats.evaluate(an, rows, CLASS_LABELS, ORDINAL_LABELS, models=dict(emotion=dc.model_spec("cats_emotion"), V=dc.model_spec("ords_V")))
    rows_only = dbstats.evaluate(an, rows, CLASS_LABELS, ORDINAL_LABELS, per_file=False)
    an.close()
    return json.loads(r.stdout), _plain(want), _plain(rows_only), rows


def test_evaluate_db_equals_the_python_result(run):
    js, want, _, _ = run
    got = js["result"]
    assert sorted(got) == sorted(want) == ["files", "rows"]
    for level in ("rows", "files"):
        assert sorted(got[level]) == sorted(want[level]), level
        for key in want[level]:
            assert got[level][key] == want[level][key], f"{level}.{key}"
    files = got["files"]
    assert files["folded"] == {"emotion": True, "sex": False} and len(files["names"]) == 10
    assert any(c is not None for c in files["classes"]["emotion"]) and "sex" not in files["classes"]
    assert any(x.startswith("UAR: ") for x in files["lines"]) and any(x.startswith("CCC: ") for x in got["rows"]["lines"])


def test_pred_pairs_are_written_and_evaluated_again_without_models(run):
    js, _, rows_only, rows = run
    assert js["stored"] == [r["pred"] for r in rows]                       # both hosts wrote the same predictions into their rows
    assert js["rows_only"]["files"] is None and js["rows_only"]["rows"] == rows_only["rows"]


def test_refusals(run):
    js, _, _, _ = run
    assert "models names the head mood" in js["refusals"]["head"]
    assert "needs a classifier" in js["refusals"]["kind"]
    assert "at least one row" in js["refusals"]["empty"]

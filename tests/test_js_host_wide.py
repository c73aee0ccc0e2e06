"""The Node host at the row width of output level 11: js/formantanalyzer.js trainModel on 264-wide rows -> saveModel -> loadModel ->
predictDB over a featuredb.js DB gives the Python path's numbers (train.train -> nnmodel.save_dir -> dbstats.predict_db: the same
library calls on the same inputs, so the weights agree in every bit), and setPredictionModel(s) refuse the 264-input handle."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import train_ref
from tests import wide_cases as wc
from tests.train_cases import permutation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
DRIVER = os.path.join(ROOT, "tests", "js", "wide_host.js")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_train_save_load_predict_on_264_wide_rows(tmp_path):
    from webspeechanalyzer_amd import capi, dbstats, nnmodel, train
    n, classes, epochs, batch = 60, ["c0", "c1", "c2", "c3"], 2, 16
    feat, lab = wc.cluster_rows(n, 264, 4, 11)
    labels = [classes[i] for i in lab]
    data = train.prepare(feat, labels, classes)
    assert data["features"].shape == (n, 264) and data["legend"] == classes
    n_train, n_val = train.split(n)
    ks, bs = train_ref.hash_init([264, 8, 4], 5)
    orders = [permutation(n_train, 30 + e) for e in range(epochs)]
    job = dict(features=feat.tolist(), labels=labels, classes=classes, options=dict(learningRate=0.1), epochs=epochs, batchSize=batch, label="emotion",
               init=dict(kernels=[k.ravel().tolist() for k in ks], biases=[b.tolist() for b in bs]), orders=np.concatenate(orders).tolist(),
               save_dir=str(tmp_path / "js_model"))
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, DRIVER, str(tmp_path / "job.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)

    an = capi.Analyzer(capi.Config(output_level=11), device=0)
    spec, history = train.train(an, data, learning_rate=0.1, epochs=epochs, batch_size=batch, init=(ks, bs), orders=orders, on_epoch=lambda e, st: None)
    assert got["units"] == got["loaded_units"] == spec.units == [264, 8, 4] and got["labels"] == classes and got["loaded_equal"] is True
    for l in range(2):
        assert np.array(got["kernels"][l], np.float32).tobytes() == spec.kernels[l].tobytes()
        assert np.array(got["biases"][l], np.float32).tobytes() == spec.biases[l].tobytes()
    assert [(h["loss"], h["acc"], h["val_loss"], h["val_acc"]) for h in got["history"]] == [(h["loss"], h["acc"], h["val_loss"], h["val_acc"]) for h in history]
    assert not np.array_equal(spec.kernels[0], ks[0])
    # the files the two hosts write load to the same model, and predict the same DB rows alike
    nnmodel.save_dir(spec, str(tmp_path / "py_model"))
    a, b = nnmodel.load_dir(str(tmp_path / "js_model")), nnmodel.load_dir(str(tmp_path / "py_model"))
    assert a.units == b.units and a.labels == b.labels and all(x.tobytes() == y.tobytes() for x, y in zip(a.kernels + a.biases + [a.in_min, a.in_max],
                                                                                                          b.kernels + b.biases + [b.in_min, b.in_max]))
    rows = [dict(file=f"file{i}.wav", seg="0", time=[0, 0.5 + i / 100], features=list(x), true=None, pred=None) for i, x in enumerate(feat)]
    preds = dbstats.predict_db(an, rows, ([{"emotion": classes}], []), "cats", "emotion", str(tmp_path / "js_model"))
    an.close()
    assert got["preds"] == preds and len(set(preds)) > 1
    assert got["stored"] == [[{"emotion": p}, {}] for p in preds]
    assert "264 inputs" in got["refusals"]["set_model"] and "264 inputs" in got["refusals"]["set_models"]
    assert "264 inputs" in got["refusals"]["width"] and "53 features" in got["refusals"]["width"]

"""The Node host's regression models (js/formantanalyzer.js trainRegression / predictValues / saveModel / loadModel over the addon): the weights
of a run with given initial weights and orders against the Python host's, bit for bit; the saved directory through nnmodel.load_dir;
predictValues against the Python host's values."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import regress_ref, train_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
DRIVER = os.path.join(ROOT, "tests", "js", "regress_host.js")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]
EPOCHS, BATCH = 3, 10
OPTIONS = dict(layers=[dict(type="dense", units=16, activation="sigmoid"), dict(type="dense", activation="sigmoid")], learningRate=0.01)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "napi")], check=True)
    from webspeechanalyzer_amd import capi, nnmodel, train
    tmp = tmp_path_factory.mktemp("jsregress")
    fx = regress_ref.load_fixture()
    feat = np.array(fx["feat"])
    values = list(fx["values"])
    values[4], values[9] = None, 1.01                         # an unlabelled DB row and one above the last bin: both dropped
    data = train.prepare_ordinal(feat, values)
    n_train, _ = train.split(len(data["values"]))
    ks, bs = train_ref.hash_init([53, 16, 1], 7)
    orders = train.epoch_orders(n_train, EPOCHS, 3)
    an = capi.Analyzer(capi.Config(output_level=13), device=0)
    spec, history = train.train_regression(an, data, layers=OPTIONS["layers"], learning_rate=OPTIONS["learningRate"], epochs=EPOCHS, batch_size=BATCH,
                                           init=(ks, bs), orders=orders, on_epoch=lambda e, st: None)
    rows = feat[:12] * 1.01
    m = an.load_model(spec)
    d_feat = torch.tensor(rows, dtype=torch.float64, device="cuda:0")
    d_val = torch.zeros(len(rows), dtype=torch.float64, device="cuda:0")
    m.regress_rows(d_feat.data_ptr(), len(rows), d_val.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    py_values = d_val.cpu().numpy()
    m.close(); an.close()
    job = dict(features=feat.tolist(), values=values, options=OPTIONS, epochs=EPOCHS, batchSize=BATCH,
               init=dict(kernels=[k.ravel().astype(np.float64).tolist() for k in ks], biases=[b.astype(np.float64).tolist() for b in bs]),
               orders=np.concatenate(orders).tolist(), save_dir=str(tmp / "1" / "ords_V"), rows=rows.tolist(), settings=dict(output_level=13))
    (tmp / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, DRIVER, str(tmp / "job.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return dict(js=json.loads(r.stdout), spec=spec, history=history, data=data, py_values=py_values, saved=nnmodel.load_dir(str(tmp / "1" / "ords_V")))


def test_weights_equal_the_python_hosts_bit_for_bit(runs):
    js, spec = runs["js"], runs["spec"]
    assert js["units"] == spec.units == [53, 16, 1] and js["labels"] == [] and (js["outMin"], js["outMax"]) == (spec.out_min, spec.out_max)
    assert len(runs["data"]["rows"]) > 48                     # the balancing added rows: both hosts made the same set
    for l in range(2):
        assert np.array(js["kernels"][l], np.float32).tobytes() == spec.kernels[l].tobytes()
        assert np.array(js["biases"][l], np.float32).tobytes() == spec.biases[l].tobytes()
    assert not np.array_equal(spec.kernels[0], train_ref.hash_init([53, 16, 1], 7)[0][0])        # it trained
    for h, p in zip(js["history"], runs["history"]):
        assert (h["loss"], h["acc"], h["val_loss"], h["val_acc"]) == (p["loss"], p["acc"], p["val_loss"], p["val_acc"])
    assert [e[0] for e in js["epochs_seen"]] == list(range(EPOCHS))


def test_saved_directory_passes_load_dir(runs):
    saved, spec = runs["saved"], runs["spec"]
    assert saved.is_regression and (saved.out_min, saved.out_max) == (spec.out_min, spec.out_max)
    assert saved.units == spec.units and saved.activations == spec.activations and saved.labels == []
    for a, b in zip(saved.kernels + saved.biases, spec.kernels + spec.biases):
        assert a.tobytes() == b.tobytes()
    assert saved.in_min.tobytes() == np.asarray(spec.in_min, np.float64).tobytes() and saved.in_max.tobytes() == np.asarray(spec.in_max, np.float64).tobytes()


def test_predict_values_equal_the_python_hosts(runs):
    js = runs["js"]
    assert np.array(js["values"]).tobytes() == runs["py_values"].tobytes() == np.array(js["values_loaded"]).tobytes()
    assert np.ptp(runs["py_values"]) > 0


def test_refusals(runs):
    r = runs["js"]["refusals"]
    assert "softmax output layer" in r["train_model"]         # trainModel keeps refusing a stack without softmax
    assert "Sample size 9/9 too small for training" in r["nine_rows"]
    assert "no class probabilities to fold" in r["set_prediction"]

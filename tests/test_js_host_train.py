"""The Node host's training (js/formantanalyzer.js trainModel / saveModel over the addon's train): the weights of a run with given initial
weights and orders against the Python host's, bit for bit; onEpoch once per epoch; the handle in setPredictionModel; the saved directory
through nnmodel.load_dir."""
import json
import os
import shutil
import subprocess
import wave

import numpy as np
import pytest

from tests import train_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NODE = shutil.which("node")
DRIVER = os.path.join(ROOT, "tests", "js", "train_host.js")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]
CLASSES = ["N", "A", "S", "H"]
EPOCHS, BATCH, OPTIONS = 3, 16, dict(layers=[dict(type="dense", units=8, activation="relu"), dict(type="dense", activation="softmax")], learningRate=0.1)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "napi")], check=True)
    from webspeechanalyzer_amd import capi, nnmodel, train
    tmp = tmp_path_factory.mktemp("jstrain")
    fx = train_ref.load_fixture()
    feat = np.array(fx["feat"])
    labels = [CLASSES[c] for c in fx["labels"]]
    labels[4] = None                                          # an unlabelled DB row
    data = train.prepare(feat, labels, CLASSES)
    n_train, _ = train.split(len(data["y"]))
    ks, bs = train_ref.hash_init([53, 8, 4], 7)
    orders = train.epoch_orders(n_train, EPOCHS, 3)
    an = capi.Analyzer(capi.Config(output_level=13), device=0)
    seen = []
    spec, history = train.train(an, data, layers=OPTIONS["layers"], learning_rate=OPTIONS["learningRate"], epochs=EPOCHS, batch_size=BATCH,
                                init=(ks, bs), orders=orders, on_epoch=lambda e, st: seen.append(e))
    an.close()
    assert seen == list(range(EPOCHS))
    c1 = json.load(open(os.path.join(GOLD, "config1_expected.json")))["settings"]
    exc = np.load(os.path.join(GOLD, "config1_excerpt.npz"))
    wav = str(tmp / "excerpt.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(int(exc["fs"])); w.writeframes(exc["pcm_i16"].astype("<i2").tobytes())
    settings = dict(output_level=13, resample_to=c1["fs_context"], window_step=c1["window_step"], pause_length=c1["pause_length"], min_seg_length=c1["min_seg_length"])
    job = dict(features=feat.tolist(), labels=labels, classes=CLASSES, options=OPTIONS, epochs=EPOCHS, batchSize=BATCH,
               init=dict(kernels=[k.ravel().astype(np.float64).tolist() for k in ks], biases=[b.astype(np.float64).tolist() for b in bs]),
               orders=np.concatenate(orders).tolist(), save_dir=str(tmp / "saved"), wav=wav, settings=settings)
    (tmp / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, DRIVER, str(tmp / "job.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return dict(js=json.loads(r.stdout), spec=spec, history=history, data=data, saved=nnmodel.load_dir(str(tmp / "saved")))


def test_weights_equal_the_python_hosts_bit_for_bit(runs):
    js, spec = runs["js"], runs["spec"]
    assert js["units"] == spec.units and js["labels"] == spec.labels == runs["data"]["legend"]
    for l in range(2):
        assert np.array(js["kernels"][l], np.float32).tobytes() == spec.kernels[l].tobytes()
        assert np.array(js["biases"][l], np.float32).tobytes() == spec.biases[l].tobytes()
    assert not np.array_equal(spec.kernels[0], train_ref.hash_init([53, 8, 4], 7)[0][0])        # it trained
    for h, p in zip(js["history"], runs["history"]):
        assert (h["loss"], h["acc"], h["val_loss"], h["val_acc"]) == (p["loss"], p["acc"], p["val_loss"], p["val_acc"])


def test_on_epoch_fires_once_per_epoch(runs):
    js = runs["js"]
    assert [e[0] for e in js["epochs_seen"]] == list(range(EPOCHS))
    assert [e[1:] for e in js["epochs_seen"]] == [[h["loss"], h["acc"], h["val_loss"], h["val_acc"]] for h in js["history"]]


def test_handle_works_in_set_prediction_model(runs):
    js = runs["js"]
    assert js["resolved"] is True and len(js["preds"]) > 0
    assert all(p[1] in CLASSES + [None] for p in js["preds"])


def test_saved_directory_passes_load_dir(runs):
    saved, spec = runs["saved"], runs["spec"]
    assert saved.units == spec.units and saved.activations == spec.activations and saved.labels == spec.labels
    for a, b in zip(saved.kernels + saved.biases, spec.kernels + spec.biases):
        assert a.tobytes() == b.tobytes()
    assert saved.in_min.tobytes() == np.asarray(spec.in_min, np.float64).tobytes() and saved.in_max.tobytes() == np.asarray(spec.in_max, np.float64).tobytes()


def test_seeded_runs_repeat_and_the_wildcard_is_refused(runs):
    assert runs["js"]["seeded_equal"] is True and "wildcard" in runs["js"]["wildcard"]

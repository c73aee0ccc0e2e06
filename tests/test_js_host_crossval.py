"""The Node host's cross-validation (js/formantanalyzer.js crossValidate: js/crossval.js over trainModels and the addon's dbEval with
foldOfRow) on tests/crossval_cases.e2e_db: with the Python host's initial weights and epoch orders handed over (the two hosts draw
theirs from different generators), every fold's weights equal the Python host's bit for bit and the structure it returns — tables,
confusion matrices, agreements, per-file sums, classes and values, the text lines, the folds — equals
webspeechanalyzer_amd.crossval.cross_validate's number for number; and dbEval without foldOfRow still gives what dbstats.evaluate gives."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webspeechanalyzer_amd import capi, crossval, dbstats, nnmodel, train

from . import crossval_cases as cc
from .test_js_host_dbeval import _plain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
DRIVER = os.path.join(ROOT, "tests", "js", "crossval_host.js")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]
K, EPOCHS, BATCH, SEED = 3, 2, 32, 11
HEADS = (cc.E2E_CLASS_LABELS, cc.E2E_ORDINALS)


def _speaker(name):
    return name.split("_")[0]


def _seeded(rows):
    """the Python host's initial weights and orders of every head and fold, as the driver takes them"""
    feat = np.array([r["features"] for r in rows], np.float64)
    fold_of_row, _, _ = crossval.assign_folds(rows, K)
    classes = cc.E2E_CLASS_LABELS[0]["emotion"]
    data = dict(emotion=crossval.fold_data(feat, crossval.head_labels(rows, "emotion", classes), classes, fold_of_row, K),
                V=crossval.fold_data(feat, crossval.head_values(rows, "V"), None, fold_of_row, K))
    units = dict(emotion=train.stack(train.DEFAULT_LAYERS, 3, 53)[0], V=train.stack_regression(train.DEFAULT_LAYERS_ORDS, 53)[0])
    inits, orders = {}, {}
    for name in ("emotion", "V"):
        inits[name], orders[name] = [], []
        for f in range(K):
            ks, bs = train.glorot_init(units[name], SEED + 2 * f)
            n_train, _ = train.split(len(data[name][f]["rows"]))
            inits[name].append(dict(kernels=[k.ravel().astype(np.float64).tolist() for k in ks], biases=[b.astype(np.float64).tolist() for b in bs]))
            orders[name].append(np.concatenate(train.epoch_orders(n_train, EPOCHS, SEED + 2 * f + 1)).tolist())
    return inits, orders


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "napi")], check=True)
    tmp = tmp_path_factory.mktemp("jscrossval")
    an = capi.Analyzer(capi.Config(output_level=13), device=0)
    rows = cc.e2e_db()
    work = cc.clone(rows)
    want = crossval.cross_validate(an, work, *HEADS, ["emotion", "V"], K, epochs=EPOCHS, batch_size=BATCH, seed=SEED, keep_models=True)
    nnmodel.save_dir(want["models"]["emotion"][0], str(tmp / "1" / "cats_emotion"))
    nnmodel.save_dir(want["models"]["V"][0], str(tmp / "1" / "ords_V"))
    plain_rows = cc.clone(rows)
    plain = dbstats.evaluate(an, plain_rows, *HEADS, models=dict(emotion=want["models"]["emotion"][0], V=want["models"]["V"][0]))
    an.close()
    inits, orders = _seeded(rows)
    job = dict(rows=rows, class_labels=HEADS[0], ordinal_labels=HEADS[1], heads=["emotion", "V"], k=K, epochs=EPOCHS, batch_size=BATCH, seed=SEED,
               inits=inits, orders=orders, settings=dict(output_level=13), models=dict(emotion=str(tmp / "1" / "cats_emotion"), V=str(tmp / "1" / "ords_V")))
    (tmp / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, DRIVER, str(tmp / "job.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout), want, work, _plain(plain), rows


def test_every_folds_weights_equal_the_python_hosts(run):
    js, want, _, _, _ = run
    for name in ("emotion", "V"):
        assert len(js["weights"][name]) == K
        for f, (got, spec) in enumerate(zip(js["weights"][name], want["models"][name])):
            for a, b in zip(got["kernels"] + got["biases"], spec.kernels + spec.biases):
                assert np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).ravel().tobytes(), (name, f)
            assert got["labels"] == list(spec.labels)                        # one legend for all folds
            last, hist = got["history"][-1], want["folds"][f]["heads"][name]["history"][-1]
            assert len(got["history"]) == EPOCHS and all(last[k] == hist[k] for k in ("loss", "acc", "val_loss", "val_acc")), (name, f)


def test_cross_validate_equals_the_python_result(run):
    js, want, work, _, rows = run
    got, plain = js["result"], _plain({k: want[k] for k in ("rows", "files")})
    for level in ("rows", "files"):
        assert sorted(got[level]) == sorted(plain[level]), level
        for key in plain[level]:
            assert got[level][key] == plain[level][key], f"{level}.{key}"
    assert got["foldOfRow"] == want["fold_of_row"].tolist() and got["foldOfFile"] == want["fold_of_file"]
    for f in range(K):
        assert got["folds"][f]["files"] == want["folds"][f]["files"] and got["folds"][f]["heldOut"] == want["folds"][f]["held_out"] == 30
    assert js["stored"] == [r["pred"] for r in work]                          # both hosts wrote the same held-out predictions into their rows
    assert sum(1 for p in js["stored"] if p == [{"emotion": None}, {"V": None}]) == 2
    assert got["files"]["folded"] == {"emotion": True}
    fold_of_row, fof, names = crossval.assign_folds(rows, 2, group_of=_speaker)
    assert js["folds"] == dict(foldOfRow=fold_of_row.tolist(), foldOfFile=fof, names=names) and fof == [0, 1, 0] * 3


def test_db_eval_without_folds_gives_what_it_gave(run):
    js, _, _, plain, _ = run
    for level in ("rows", "files"):
        for key in plain[level]:
            assert js["plain"][level][key] == plain[level][key], f"{level}.{key}"


def test_refusals(run):
    js, _, _, _, _ = run
    assert "heads names mood; the settings have emotion,V" in js["refusals"]["head"]
    assert "a cross-validation has 2 .. 32 folds, got 33" in js["refusals"]["k"]
    assert "9 folds for 3 groups (9 files)" in js["refusals"]["groups"]
    assert "head emotion has 0 models for 3 folds" in js["refusals"]["members"]

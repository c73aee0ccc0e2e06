"""The host side of training that needs no GPU: saving a model as ml5 does, the app's balancing loop, the ABI's new symbols."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import classify_ref
from webspeechanalyzer_amd import capi, nnmodel, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_SYMBOLS = ["wsa_trainer_create", "wsa_trainer_destroy", "wsa_trainer_epoch", "wsa_trainer_stats", "wsa_trainer_copy_weights", "wsa_trainer_model"]


def test_save_dir_round_trip_is_bit_exact(tmp_path):
    spec = classify_ref.seeded_spec(seed=3, widths=(20, 12, 5), labels=["N", "A", "S", "H", "7"])
    spec.activations = ["sigmoid", "tanh", "softmax"]
    nnmodel.save_dir(spec, str(tmp_path / "m"))
    back = nnmodel.load_dir(str(tmp_path / "m"))
    assert back.units == spec.units and back.activations == spec.activations and back.labels == spec.labels
    for a, b in zip(spec.kernels + spec.biases, back.kernels + back.biases):
        assert a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes()
    assert back.in_min.tobytes() == np.asarray(spec.in_min, np.float64).tobytes() and back.in_max.tobytes() == np.asarray(spec.in_max, np.float64).tobytes()
    shipped = json.load(open(os.path.join(ROOT, "tests", "golden", "nn", "1", "cats_emotion", "model.json")))
    ours = json.load(open(tmp_path / "m" / "model.json"))
    assert sorted(ours) == sorted(shipped) and sorted(ours["modelTopology"]) == sorted(shipped["modelTopology"])
    assert sorted(ours["modelTopology"]["config"]["layers"][0]["config"]) == sorted(shipped["modelTopology"]["config"]["layers"][0]["config"])
    meta_s = json.load(open(os.path.join(ROOT, "tests", "golden", "nn", "1", "cats_emotion", "model_meta.json")))
    meta_o = json.load(open(tmp_path / "m" / "model_meta.json"))
    assert sorted(meta_o) == sorted(meta_s) and sorted(meta_o["outputs"]["y"]) == sorted(meta_s["outputs"]["y"])


def _db(counts):
    """rows of classes 0 .. in DB order, interleaved, feature 0 = the DB index"""
    lab = []
    left = list(counts)
    while any(left):
        for c in range(len(left)):
            if left[c]:
                lab.append("NASH"[c]); left[c] -= 1
    feat = np.zeros((len(lab), 53)); feat[:, 0] = np.arange(len(lab)); feat[:, 1:] = np.arange(52) + 1.0
    return feat, lab


def test_prepare_balances_as_the_app_does():
    feat, lab = _db([10, 5, 4, 3])
    lab[2] = None                                    # an unlabelled row is skipped
    feat2, lab2 = np.vstack([feat, feat[:1]]), lab + ["S"]
    d = train.prepare(feat2, lab2, ["N", "A", "S", "H"])
    assert d["counts"] == [10, 10, 10, 3] and d["legend"] == ["N", "A", "H", "S"]
    base = [i for i, v in enumerate(lab2) if v is not None]
    assert d["rows"][:len(base)] == base
    a_rows = [i for i, v in enumerate(lab2) if v == "A"]
    s_rows = [i for i, v in enumerate(lab2) if v == "S"]
    extra = d["rows"][len(base):]
    assert extra[:5] == a_rows and extra[5:] == (s_rows * 3)[:6]      # topped up by cycling through the DB in order
    assert len(d["features"]) == 33 and d["in_min"][0] == 0 and d["in_max"][0] == feat2[:, 0].max()
    assert [d["legend"][k] for k in d["y"]] == [lab2[i] for i in d["rows"]]


def test_prepare_refusals():
    feat, lab = _db([3, 3, 3])
    with pytest.raises(ValueError, match="Sample size 9/9 too small"):
        train.prepare(feat, lab, ["N", "A", "S"])
    feat, lab = _db([6, 6])
    with pytest.raises(ValueError, match="wildcard"):
        train.prepare(feat, lab, ["N", "*"])


def test_initialisers_and_orders_are_seeded():
    ks, bs = train.glorot_init([53, 8, 4], 5)
    ks2, _ = train.glorot_init([53, 8, 4], 5)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ks, ks2)) and all(not b.any() for b in bs)
    assert np.abs(ks[0]).max() <= 2 * np.sqrt(2 / 61) + 1e-7 and ks[0].dtype == np.float32
    o = train.epoch_orders(45, 3, 1)
    assert len(o) == 3 and all(sorted(x.tolist()) == list(range(45)) for x in o) and o[0].tolist() != o[1].tolist()
    assert train.split(50) == (45, 5) and train.split(74249) == (66824, 7425)


def test_trainer_symbols_are_declared_listed_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wsa.h")).read(), flags=re.S)
    L = capi.lib()
    for s in TRAIN_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header) and s in capi.ABI_SYMBOLS and hasattr(L, s), s
    assert L.wsa_abi_version() == 5


@pytest.mark.reference
def test_saved_directory_loads_in_the_references_ml5(tmp_path):
    ref = "/root/reference"
    if not os.path.exists(os.path.join(ref, "dist", "ml5.min.js")) or not shutil.which("node"):
        pytest.skip("needs /root/reference and node")
    spec = classify_ref.seeded_spec(seed=4, widths=(8, 4), labels=["N", "A", "S", "H"])
    mdir = str(tmp_path / "1" / "cats_emotion")
    nnmodel.save_dir(spec, mdir)
    rng = np.random.default_rng(2)
    feat = spec.in_min + rng.uniform(0, 1, (6, 53)) * (spec.in_max - spec.in_min)
    job = dict(ml5=os.path.join(ref, "dist/ml5.min.js"), prediction=os.path.join(ref, "src/prediction.js"), models={"m": mdir},
               clips=[dict(key="k", callbacks=[dict(si=0, seg_time=[["0.100", "0.200"]] * 6, feat=feat.tolist())])])
    json.dump(job, open(tmp_path / "job.json", "w"))
    subprocess.run(["node", os.path.join(ROOT, "tests", "golden", "gen", "make_classify_golden.js"), str(tmp_path / "job.json"), str(tmp_path / "out.json")],
                   check=True, timeout=300, capture_output=True)
    out = json.load(open(tmp_path / "out.json"))["models"]["m"]
    assert out["legend"] == spec.labels
    assert np.abs(np.array(out["prob"]) - classify_ref.forward(spec, feat)).max() <= 1e-6

"""The Node host's training groups (js/formantanalyzer.js trainModels over the addon's trainGroup): one classifier job and one regression
job in one call against trainModel / trainRegression one by one, by the bytes of the saved model files; onEpoch per job; more than 32
jobs as consecutive groups."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import regress_ref, train_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
DRIVER = os.path.join(ROOT, "tests", "js", "train_group_host.js")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]
CLASSES = ["N", "A", "S", "H"]
EXTRA = 35


@pytest.fixture(scope="module")
def js(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "napi")], check=True)
    tmp = tmp_path_factory.mktemp("jstraingroup")
    fx, rfx = train_ref.load_fixture(), regress_ref.load_fixture()
    job = dict(classifier=dict(features=np.array(fx["feat"]).tolist(), labels=[CLASSES[c] for c in fx["labels"]], classes=CLASSES, epochs=3, batchSize=16, seed=4,
                               options=dict(layers=[dict(type="dense", units=8, activation="relu"), dict(type="dense", activation="softmax")], learningRate=0.1)),
               regressor=dict(features=np.array(rfx["feat"]).tolist(), values=list(rfx["values"]), epochs=2, batchSize=10, seed=9,
                              options=dict(layers=[dict(type="dense", units=16, activation="sigmoid"), dict(type="dense", activation="sigmoid")], learningRate=0.01)),
               extra=EXTRA, dir=str(tmp), settings=dict(output_level=13))
    (tmp / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, DRIVER, str(tmp / "job.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_saved_model_files_equal_the_one_by_one_calls(js):
    assert js["same_files"] == [True, True] and js["histories_equal"] == [True, True]
    assert sorted(js["labels"][0]) == sorted(CLASSES) and js["labels"][1] == []


def test_on_epoch_is_per_job(js):
    assert js["seen"]["grouped"] == js["seen"]["single"]
    assert [e[0] for e in js["seen"]["grouped"][0]] == [0, 1, 2] and [e[0] for e in js["seen"]["grouped"][1]] == [0, 1]


def test_more_than_32_jobs_run_as_consecutive_groups(js):
    assert js["many"] == EXTRA and js["many_epochs"] == [1 + k % 2 for k in range(EXTRA)] and js["many_equal"] is True


def test_a_refused_job_refuses_the_call(js):
    assert "wildcard" in js["wildcard"]

"""The Node host on the device feature DB (specification FD-1; js/formantanalyzer.js createDeviceDB / setCollectDB / toFeatureDB, trainModel and
trainRegression from a DB): a LaunchBatch under setCollectDB delivers the callbacks it delivers without it and leaves a DB whose export is byte for
byte the FeatureDB the collector fills from those callbacks; training from the DB gives the weights of training from the rows; a device DB is
refused when more than one device is configured."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
DRIVER = os.path.join(ROOT, "tests", "js", "featdb_host.js")
ADDON = os.path.join(ROOT, "webspeechanalyzer_amd", "lib", "wsa_napi.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]
LEVELS = [13, 5, 11]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert os.path.exists(ADDON), "the N-API addon is not built (__graft_entry__.build())"
    from webspeechanalyzer_amd.synth import synth_clips
    tmp = tmp_path_factory.mktemp("jsfeatdb")
    fs, ns, nc = 16000, 48000, 8
    pcm = synth_clips(nc, ns, fs=fs, seed=3).numpy()
    paths = []
    for c in range(nc):
        paths.append(str(tmp / f"clip{c}.f32"))
        pcm[c].tofile(paths[-1])
    job = tmp / "job.json"
    job.write_text(json.dumps(dict(clips=paths, fs=fs, levels=LEVELS, capacity=4096, epochs=2, batchSize=16)))
    r = subprocess.run([NODE, DRIVER, str(job)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return {x["level"]: x for x in json.loads(r.stdout)}


@pytest.mark.parametrize("level", LEVELS)
def test_collected_db_exports_the_collectors_feature_db(runs, level):
    x = runs[level]
    assert x["callbacks"] > 0 and x["callbacks_equal"], x
    assert x["rows"] == x["records"] > 0
    assert x["json_bytes"] > 0 and x["json_equal"], x
    assert x["again"] is not None and "already holds" in x["again"] and x["rows_after_refusal"] == x["rows"]


def test_launch_batches_collects_batch_by_batch(runs):
    x = runs[13]
    assert x["batches"] == 8 and x["batches_json_equal"], x


def test_training_from_the_device_db_equals_training_from_the_rows(runs):
    x = runs[13]
    assert x["train_rows"] == x["rows"] >= 12
    assert x["train_equal"] and x["regress_equal"], x
    assert all(v == v for v in x["train_loss"])
    assert x["short_labels"] is not None and "labels for a device DB of" in x["short_labels"]


def test_a_device_db_is_refused_with_several_devices(runs):
    x = runs[13]
    assert x["multi"] is not None and "lives on one device" in x["multi"] and "2 entries" in x["multi"]
    # devices: [0, 0] is two contexts and two shards on one GPU: refused alike, at setCollectDB and at a launch while a DB collects, with
    # nothing run, nothing stored and no file marked as held
    assert x["twice"] is not None and "2 entries" in x["twice"]
    assert x["twice_launch"] is not None and "2 entries" in x["twice_launch"] and x["twice_calls"] == 0
    assert x["rows_after_twice"] == x["rows"] == x["records_after_twice"]
    assert x["rows_after_more"] == 2 * x["rows"] == x["records_after_more"]

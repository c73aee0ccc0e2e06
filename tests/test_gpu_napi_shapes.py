"""The shape of every result object the N-API addon (webspeechanalyzer_amd/napi/) hands to JavaScript: per object its key set, per key the
typed-array constructor and length or the number itself, `ens` one level down.  Two 3 s clips at 16 kHz (synth_clips, seed 3) go through
processBatch at output levels 3, 4, 11 and 13 (13: with one model, a two-model ensemble, neither), then batchRegressGroup, batchKnn and
batchKnnFold, then as two streams in 4-frame steps with a model, a KNN store, an ensemble and a regress group attached in turn (the first step
with rows and the last).  tests/golden/napi_shapes.json holds what the addon gave before the binding was cut into files
(tests/golden/gen/make_napi_shapes.py records it); no recorded object is without rows."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
PROBE = os.path.join(ROOT, "tests", "js", "napi_shapes_probe.js")
ADDON = os.path.join(ROOT, "webspeechanalyzer_amd", "lib", "wsa_napi.node")
GOLDEN = os.path.join(ROOT, "tests", "golden", "napi_shapes.json")
CLASSIFIERS = [os.path.join(ROOT, "tests", "golden", "nn", db, "cats_emotion") for db in ("1", "2")]
HEADS = ("sigmoid_64_16", "tfjs", "tanh_16")
FS, SECONDS, CLIPS, SEED, FRAMES_PER_STEP = 16000, 3, 2, 3, 4


def record(addon, tmp):
    """the probe's output for the addon at `addon` (beside a libwsa.so), scratch files under `tmp`"""
    from tests import regress_fold_cases as C
    from webspeechanalyzer_amd import nnmodel
    from webspeechanalyzer_amd.synth import synth_clips
    pcm = synth_clips(CLIPS, SECONDS * FS, fs=FS, seed=SEED, device="cpu").numpy().astype(np.float32)
    sig = os.path.join(tmp, "clips.f32")
    pcm.tofile(sig)
    specs, dirs = C.model_specs(), []
    for i, name in enumerate(HEADS):
        dirs.append(os.path.join(tmp, f"ords_{'VAD'[i]}"))
        nnmodel.save_dir(specs[name], dirs[-1])
    job = os.path.join(tmp, "job.json")
    with open(job, "w") as f:
        json.dump(dict(addon=addon, pcm=sig, n=CLIPS, ns=SECONDS * FS, fs=FS, classifiers=CLASSIFIERS, regress=dirs, frames_per_step=FRAMES_PER_STEP), f)
    r = subprocess.run([NODE, PROBE, job], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def rows_of(name, shape):
    """how many entries the table that the recorded object `name` is about holds (level 3: track points, 4: formant frames, 11: utterance rows)"""
    if name == "knn_add":
        return shape["rows"]
    special = {"batch_level_3": "trackPoints", "batch_level_4": "formants", "batch_level_11": "uttMeta"}
    if name in special:
        return shape[special[name]][1]
    for key in ("meta", "label", "value", "cbLabel"):
        if key in shape:
            return shape[key][1]
    raise AssertionError(f"{name}: no row table among {sorted(shape)}")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_result_objects_have_the_recorded_shapes(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert os.path.exists(ADDON), "the N-API addon is built by build()"
    want = json.load(open(GOLDEN))
    assert len(want) == 18 and all(rows_of(name, shape) > 0 for name, shape in want.items())
    got = record(ADDON, str(tmp_path))
    assert sorted(got) == sorted(want)
    for name in want:
        print(name, json.dumps(got[name]))
        assert sorted(got[name]) == sorted(want[name]), name
        for key in want[name]:
            assert got[name][key] == want[name][key], (name, key)
    assert got == want

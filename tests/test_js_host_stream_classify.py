"""The Node host's classifier on live streams (js/formantanalyzer.js StreamOpen with setPredictionModel, over the addon's
streamSetModel): the on_prediction sequence of a stream fed the sample file's excerpt step by step equals LaunchBatch's on the same
signal (the clip index replaced by the stream index), the meters after close() equal the batch's, the callback sequence does not depend
on the model, and modelDestroy refuses while a stream holds the model."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NODE = shutil.which("node")
DRIVER = os.path.join(ROOT, "tests", "js", "stream_classify_host.js")
MODEL1 = os.path.join(GOLD, "nn", "1", "cats_emotion")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "napi")], check=True)
    return torch


@pytest.mark.parametrize("F", [1, 5])
def test_stream_on_prediction_equals_the_batch(torch, tmp_path, F):
    import webspeechanalyzer_amd as wsa
    S = json.load(open(os.path.join(GOLD, "config1_expected.json")))["settings"]
    exc = np.load(os.path.join(GOLD, "config1_excerpt.npz"))
    x = (exc["pcm_i16"].astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    cfg = dict(output_level=13, window_step=S["window_step"], pause_length=S["pause_length"], min_seg_length=S["min_seg_length"])
    an = wsa.Analyzer(wsa.Config(**cfg))
    b = an.batch([len(x)], int(exc["fs"]), resample_to=S["fs_context"])
    src = torch.from_numpy(x).cuda()[None, :].contiguous()
    b.run(src.data_ptr(), src.stride(0), torch.cuda.current_stream().cuda_stream)
    pcm = b.converted_pcm(torch.cuda.current_stream().cuda_stream)[0]
    b.close(); an.close()
    f = tmp_path / "x48k.f32"
    pcm.astype(np.float32).tofile(f)
    job = dict(pcm=str(f), fs=int(S["fs_context"]), settings=dict(cfg, resample_to=0), model=MODEL1, frames_per_step=F)
    jp = tmp_path / "job.json"
    jp.write_text(json.dumps(job))
    r = subprocess.run([NODE, DRIVER, str(jp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    assert len(got["batch"]["preds"]) >= 2
    assert got["stream"]["preds"] == got["batch"]["preds"]              # si, label, confidence, index 0, per_syllable
    assert got["stream"]["meters"] == got["batch"]["meters"]                # one {label: Label_conf_all} per stream / clip
    assert got["stream"]["callbacks"] == got["plain"]["callbacks"] and got["plain"]["meters"] is None
    assert "in use" in got["destroy_while_held"]
    assert got["destroy_after_close"] == "destroyed"

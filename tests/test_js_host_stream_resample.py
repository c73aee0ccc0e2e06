"""StreamOpen over live sources of different rates with configure({resample_to: 48000}): fed paced through push(), every source's callbacks
are those LaunchBatch gives for the same three signals as clips (the stream in place of the clip), the predictions too when a model is set."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL1 = os.path.join(ROOT, "tests", "golden", "nn", "1", "cats_emotion")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]
RATES = [44100, 16000, 48000]


@pytest.fixture(scope="module")
def signals(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from webspeechanalyzer_amd.synth import synth_clips
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "napi")], check=True)
    d = tmp_path_factory.mktemp("streams")
    clips = []
    for k, fs in enumerate(RATES):
        p = str(d / f"s{k}.f32")
        n = 4 * fs + 123                                     # not a whole number of paced steps: the last push carries counts
        synth_clips(1, n, fs=fs, seed=91 + k, device="cpu").numpy()[0].astype(np.float32).tofile(p)
        clips.append(dict(pcm=p, fs=fs))
    return d, clips


def _run(d, job):
    jp = d / "job.json"
    jp.write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "stream_resample_host.js"), str(jp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.mark.parametrize("level,F,model", [(5, 1, None), (13, 4, MODEL1)])
def test_stream_open_of_three_rates_equals_launch_batch(signals, level, F, model):
    d, clips = signals
    out = _run(d, dict(clips=clips, settings=dict(output_level=level, resample_to=48000), model=model, frames_per_step=F))
    h = out["stream"]["handle"]
    assert h["samplesPerStep"] == F * 1200 and h["capacity"] == [int(np.ceil(F * 1200 * 44100 / 48000)), F * 400, F * 1200]
    assert h["inputStride"] >= max(h["capacity"])
    assert out["stream"]["pushes"]["paced"] > 10 * out["stream"]["pushes"]["explicit"] > 0
    for s in range(len(clips)):
        assert len(out["batch"]["callbacks"][s]) > 0
        a, b = out["stream"]["callbacks"][s], out["batch"]["callbacks"][s]
        assert [c[:3] for c in a] == [c[:3] for c in b], s
        for x, y in zip(a, b):
            assert np.allclose(np.array(x[3], dtype=np.float64), np.array(y[3], dtype=np.float64), rtol=1e-9, atol=1e-12, equal_nan=True), s
    if model:
        assert len(out["batch"]["preds"]) > 0
        key = lambda p: (p[3], p[0])                         # (the streams' predictions arrive step by step, the batch's clip by clip)
        assert sorted(out["stream"]["preds"], key=key) == sorted(out["batch"]["preds"], key=key)

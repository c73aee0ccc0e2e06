"""LaunchBatch over WAV files of different rates with configure({resample_to: 48000}): per clip the callbacks of the oracle chain
resample -> front end -> back end and of one LaunchAudioNodes per file; with a prediction model set, one prediction per callback."""
import json
import os
import shutil
import subprocess
import wave

import numpy as np
import pytest

from tests.util import callbacks_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "webspeechanalyzer_amd", "js", "formantanalyzer.js")
MODEL1 = os.path.join(ROOT, "tests", "golden", "nn", "1", "cats_emotion")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]
RATES = [16000, 44100, 48000]


def _write_wav(path, pcm, fs):
    q = np.clip(np.round(pcm * 32768.0), -32768, 32767).astype(np.int16)
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(fs); w.writeframes(q.tobytes())
    return (q.astype(np.float64) / 32768.0).astype(np.float32)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from webspeechanalyzer_amd.synth import synth_clips
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "napi")], check=True)
    d = tmp_path_factory.mktemp("mixed")
    out = []
    for k, fs in enumerate(RATES):
        p = str(d / f"c{k}.wav")
        out.append((p, fs, _write_wav(p, synth_clips(1, 4 * fs, fs=fs, seed=81 + k, device="cpu").numpy()[0], fs)))
    return d, out


def _run(d, job):
    jp = d / "job.json"
    jp.write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "node_runner.js"), str(jp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.mark.parametrize("level", [5, 13])
def test_launch_batch_of_wav_files_with_different_rates(files, level):
    from oracle import pyoracle
    d, clips = files
    spec = [dict(file=p, kind="wav") for p, _, _ in clips]
    batch = _run(d, dict(level=level, clips=spec, batch=True, config=dict(resample_to=48000)))
    single = _run(d, dict(level=level, clips=spec, config=dict(resample_to=48000)))
    fe = pyoracle.FrontEnd(pyoracle.fe_cfg(fs=48000.0))
    strip = lambda cbs: [[c[0], [], c[2], c[3]] for c in cbs]
    for c, (_, fs, host) in enumerate(clips):
        x = host if fs == 48000 else pyoracle.resample(host, fs, 48000)
        ref = pyoracle.run_backend(fe.run(x), pyoracle.default_cfg(level=level, bands=fe.bands))
        ok, why = callbacks_equal(level, strip(ref["callbacks"]), strip(batch[c]), exact=False, tol=1e-4)
        assert ok, (c, why)
        assert len(batch[c]) > 0
        assert json.dumps(strip(batch[c])) == json.dumps(strip(single[c]["calls"])), c


def test_launch_batch_of_mixed_rates_with_prediction_model(files):
    d, clips = files
    script = f"""
const fs = require('fs');
const fa = require({json.dumps(JS)});
fa.configure(Object.assign({{}}, fa._settings, {{output_level: 13, resample_to: 48000}}));
const h = fa.loadModel({json.dumps(MODEL1)});
const cbs = [0, 0, 0], preds = [0, 0, 0];
fa.setPredictionModel(h, (si, lc, clip, per) => {{ preds[clip]++; }});
fa.LaunchBatch({json.dumps([p for p, _, _ in clips])}.map((f) => fs.readFileSync(f)), (si, label, t, f, clip) => {{ cbs[clip]++; }}, [])
  .then((r) => console.log(JSON.stringify({{cbs, preds, meters: r.meters.length}})), (e) => {{ console.error(e); process.exit(1); }});
"""
    r = subprocess.run([NODE, "-e", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out["cbs"] == out["preds"] and all(n > 0 for n in out["cbs"]) and out["meters"] == 3

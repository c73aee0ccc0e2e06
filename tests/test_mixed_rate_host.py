"""Mixed-rate batches, the parts that need no GPU: wsa_batch_create_mixed is declared, exported and bound, and the Node module accepts
clips of different rates when a conversion is configured (and only then)."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "webspeechanalyzer_amd", "js", "formantanalyzer.js")
NODE = shutil.which("node")


def test_mixed_entry_point_declared_exported_and_bound():
    from webspeechanalyzer_amd import capi
    capi.build_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wsa.h")).read(), flags=re.S)
    assert re.search(r"\bwsa_batch_create_mixed\s*\(", header)
    assert "#define WSA_ABI_VERSION 5" in header
    assert hasattr(capi.lib(), "wsa_batch_create_mixed")
    assert "wsa_batch_create_mixed" in capi.ABI_SYMBOLS


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_launch_batch_accepts_mixed_rates_only_with_a_conversion():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "napi")], check=True)
    script = f"""
const fa = require({json.dumps(JS)});
const clips = [{{pcm: new Float32Array(16000), sampleRate: 16000}}, {{pcm: new Float32Array(44100), sampleRate: 44100}}];
const cfg = {{spec_type:1, output_level:5, f_min:50, high_f_emph:0, auto_noise_gate:true, voiced_min_dB:10}};
const out = {{}};
(async () => {{
  fa.configure(Object.assign({{}}, cfg, {{resample_to: 48000}}));
  out.converted = await fa.LaunchBatch(clips, () => {{}}).then(() => 'RESOLVED', (e) => String(e));
  out.batches = await fa.LaunchBatches([clips], () => {{}}).then(() => 'RESOLVED', (e) => String(e));
  fa.configure(Object.assign({{}}, cfg, {{resample_to: 0}}));
  out.plain = await fa.LaunchBatch(clips, () => {{}}).then(() => 'RESOLVED', (e) => String(e));
  console.log(JSON.stringify(out));
}})();
"""
    r = subprocess.run([NODE, "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    shared = "All clips of one launch must share a sample rate"
    assert shared not in out["converted"] and "no CPU path" in out["converted"]
    assert shared not in out["batches"] and "no CPU path" in out["batches"]
    assert out["plain"] == shared

"""The JavaScript host's batch launches on clips of every encoding (spec PK-2): in-memory WAVs (G.711, 8 / 24 / 32-bit, float64, stereo) and
mixed Float32Array / Int16Array batches go to the device as the bytes they hold; their callbacks equal those of the same signals handed
over as decoded Float32Arrays.  A mu-law WAV no longer throws, a WAV nothing decodes still does."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests.batch_pcm_cases import encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "webspeechanalyzer_amd", "lib", "wsa_napi.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]
FS = 16000
# name: (format tag, bits, the format decode_wav names, channels)
WAVS = {"mulaw": (7, 8, "mulaw", 1), "alaw": (6, 8, "alaw", 2), "pcm24": (1, 24, "i24", 2), "float64": (3, 64, "f64", 1),
        "pcm8": (1, 8, "u8", 1), "pcm32": (1, 32, "i32", 1), "float32": (3, 32, "f32", 3)}


def riff(tag, ch, rate, bits, data, lead=b""):
    fmt = struct.pack("<HHIIHH", tag, ch, rate, rate * ch * bits // 8, ch * bits // 8, bits)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + lead + b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert os.path.exists(ADDON), "the N-API addon is not built"
    from webspeechanalyzer_amd.synth import synth_clips
    d = tmp_path_factory.mktemp("batch_pcm")
    ns = int(1.2 * FS)
    x = synth_clips(len(WAVS) + 4, ns, fs=FS, seed=77, device="cpu").numpy()
    wavs = {}
    for k, (name, (tag, bits, f, ch)) in enumerate(WAVS.items()):
        data = encode(x[k], f, ch, 200 + k).view(np.uint8).tobytes()
        lead = b"LIST" + struct.pack("<I", 1) + b"z\0" if name == "pcm24" else b""       # an odd-sized chunk in front of the data: its pad byte is skipped
        p = d / (name + ".wav")
        p.write_bytes(riff(tag, ch, FS, bits, data, lead))
        wavs[name] = str(p)
    bad = d / "adpcm.wav"
    bad.write_bytes(riff(2, 1, FS, 4, bytes(4096)))
    f32, i16 = [], []
    for k in range(2):
        p = d / f"f{k}.f32"
        x[len(WAVS) + k].astype("<f4").tofile(p)
        f32.append(str(p))
        p = d / f"s{k}.i16"
        np.clip(np.rint(x[len(WAVS) + 2 + k] * 32767.0), -32768, 32767).astype("<i2").tofile(p)
        i16.append(str(p))
    jp = d / "job.json"
    jp.write_text(json.dumps(dict(settings=dict(output_level=5), fs=FS, wavs=wavs, bad=str(bad), f32=f32, i16=i16)))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "batch_pcm_host.js"), str(jp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_wavs_of_every_encoding_equal_their_decoded_floats(out):
    assert out["kinds"] == {name: "%s/%d" % (f, ch) for name, (_, _, f, ch) in WAVS.items()}       # none of them was decoded on the host
    for name in WAVS:
        assert len(out["floats"][name]) > 0, name                # a condition on the input: every clip has callbacks to compare
        assert out["wav"][name] == out["floats"][name], name
    assert out["solo"] == out["floats"][out["solo_name"]]
    assert out["object"] == out["floats"][out["solo_name"]]
    assert len(out["cut_want"]) > 0 and out["cut"] == out["cut_want"] and out["cut"] != out["floats"]["pcm24"]


def test_mixed_float_and_int16_clips_equal_the_float_batch(out):
    assert all(len(c) > 0 for c in out["mixed_floats"])
    assert out["mixed"] == out["mixed_floats"]
    assert out["batches"] == out["batches_want"]


def test_what_nothing_decodes_still_throws(out):
    assert out["bad"] == "Unable to decode audio data"
    assert out["bad_object"] == "Invalid audio source"

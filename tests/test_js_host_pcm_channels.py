"""The JavaScript host's `channel` key (spec PK-3): 'each' on a stereo WAV gives the callbacks of two mono launches, labels extended by
'ch' + c; 'mix' and a channel number give those of the host-decoded floats; 'first' stays what it was; StreamOpen's input_format takes
select and source; decodePcm takes a select."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests.batch_pcm_cases import encode
from webspeechanalyzer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "webspeechanalyzer_amd", "lib", "wsa_napi.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]
FS = 16000


def riff(tag, ch, rate, bits, data):
    fmt = struct.pack("<HHIIHH", tag, ch, rate, rate * ch * bits // 8, ch * bits // 8, bits)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert os.path.exists(ADDON), "the N-API addon is not built"
    from webspeechanalyzer_amd.synth import synth_clips
    d = tmp_path_factory.mktemp("pcm_channels")
    ns = int(1.2 * FS)
    x = synth_clips(5, ns, fs=FS, seed=91, device="cpu").numpy()
    cols = [encode(x[k], "i16", 1, 300 + k) for k in range(2)]
    stereo = np.stack(cols, axis=1).reshape(-1)
    tri = np.stack([encode(x[2 + k], "i24", 1, 310 + k).reshape(ns, 3) for k in range(3)], axis=1).reshape(-1)
    paths = {}

    def put(name, data):
        p = d / name
        p.write_bytes(data)
        paths[name] = str(p)
        return str(p)

    put("stereo.wav", riff(1, 2, FS, 16, stereo.astype("<i2").tobytes()))
    put("tri.wav", riff(1, 3, FS, 24, tri.tobytes()))
    mono = [put(f"mono{k}.wav", riff(1, 1, FS, 16, cols[k].astype("<i2").tobytes())) for k in range(2)]
    put("mix.f32", capi.pcm_decode("i16", stereo, 2, "mix").astype("<f4").tobytes())
    put("tri_mix.f32", capi.pcm_decode("i24", tri, 3, "mix").astype("<f4").tobytes())
    put("tri_last.f32", capi.pcm_decode("i24", tri, 3, 2).astype("<f4").tobytes())
    jp = d / "job.json"
    jp.write_text(json.dumps(dict(settings=dict(output_level=5), fs=FS, stereo=paths["stereo.wav"], mono=mono, mix=paths["mix.f32"], tri=paths["tri.wav"],
                                  tri_mix=paths["tri_mix.f32"], tri_last=paths["tri_last.f32"])))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "pcm_channels_host.js"), str(jp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def _of(cbs, clip):
    return [c[2:] for c in cbs if c[0] == clip]


def test_each_on_a_stereo_wav_gives_the_callbacks_of_two_mono_launches(out):
    each, mono = out["each"], out["mono"]
    assert len(_of(mono, 0)) > 0 and len(_of(mono, 1)) > 0 and _of(mono, 0) != _of(mono, 1)         # both speakers have callbacks, and different ones
    # analyses 0 and 1 are the call's channels, 2 .. 4 the room's: callbacks in (clip, channel) order, labels extended by 'ch' + c
    assert [c[0] for c in each] == sorted(c[0] for c in each) and {c[0] for c in each} == {0, 1, 2, 3, 4}
    assert [c for c in each if c[0] < 2] == mono
    for a, (name, c) in enumerate([("call", 0), ("call", 1), ("room", 0), ("room", 1), ("room", 2)]):
        assert all(cb[1] == [name, "ch%d" % c] for cb in each if cb[0] == a)
    assert _of(each, 4) == _of(out["last_want"], 0) and _of(each, 2) == _of(out["first"], 1)
    assert out["each_solo"] == [c[1:] for c in mono]               # LaunchAudioNodes: the channels one after the other


def test_mix_and_a_channel_number_equal_the_decoded_floats(out):
    assert len(_of(out["mix_want"], 0)) > 0 and len(_of(out["mix_want"], 1)) > 0
    assert out["mix"] == out["mix_want"]
    assert [c[1] for c in out["mix"]] == [["call"]] * len(_of(out["mix"], 0)) + [["room"]] * len(_of(out["mix"], 1))       # labels as given
    assert _of(out["one"], 0) == _of(out["mono"], 1) and _of(out["two"], 0) == _of(out["last_want"], 0)
    assert _of(out["first"], 0) == _of(out["mono"], 0)             # 'first' is channel 0, as before
    assert "clip 1: select 2 is neither a channel below 2 nor WSA_CHANNEL_MIX" in out["two_on_stereo"]
    assert "LaunchBatches analyses channel 0" in out["batches"]
    assert "channel: 'first', 'mix', 'each' or a channel number" in out["bad_key"]


def test_streams_share_a_packed_row(out):
    want = out["stream_want"]
    assert all(len(w) > 0 for w in want) and want[0] != want[1] and want[2] != want[0]
    assert out["stream"] == want
    assert "stream 1: select 2 is neither a channel below 2 nor WSA_CHANNEL_MIX" in out["stream_bad"]


def test_decode_pcm_takes_a_select(out):
    d = out["decode"]
    assert d["ch0"] == [100 / 32768, 300 / 32768, 500 / 32768] and d["ch1"] == [-200 / 32768, -400 / 32768]
    assert d["mix"] == [(100 - 200) / 32768 * 0.5, (300 - 400) / 32768 * 0.5]
    assert "select is neither a channel" in d["bad"]

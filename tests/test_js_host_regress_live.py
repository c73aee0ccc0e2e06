"""The Node host's value models on live streams and batches (js/formantanalyzer.js setPredictionValues over the addon's streamSetRegress and
batchRegressGroup): for one stream set and one LaunchBatch over the same signal, the on_values sequence (si, values, index, weights,
per-syllable values, running values) is the one the Python path gives (Streams.set_regress + values, Batch.regress_group + value_fold),
bit for bit; the handler follows on_prediction of the same callback and leaves it alone; a skipped callback gets no call; a classifier
handle, nine handles and a released handle are refused."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import regress_fold_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
DRIVER = os.path.join(ROOT, "tests", "js", "stream_values_host.js")
ADDON = os.path.join(ROOT, "webspeechanalyzer_amd", "lib", "wsa_napi.node")
CLASSIFIER = os.path.join(ROOT, "tests", "golden", "nn", "1", "cats_emotion")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]
HEADS = ("sigmoid_64_16", "tfjs", "tanh_16")
F = 3


def _num(x):
    return float(x) if np.isfinite(x) else str(float(x))


def _nums(a):
    return [_num(x) for x in a]


def _calls(meta, value, step_s, unit=0):
    """the calls RG-1 asks for over one unit's rows: [si, values, unit, weights, per-syllable values, running values], skipped callbacks left out"""
    out, run = [], {}
    cbs, _ = C.rg1_ref(meta, value, step_s)
    H = value.shape[0]
    for cb in cbs:
        a, b = cb["first"], cb["first"] + cb["rows"]
        _, run = C.rg1_ref(meta[a:b], value[:, a:b], step_s, run)
        if cb["skipped"]:
            continue
        out.append([cb["si"], _nums(cb["value"]), unit, _nums(cb["weight"]), [_nums(value[:, q]) for q in range(a, b)],
                    _nums(C.run_value(run, int(meta[a][0]), H)[2])])
    return out


def test_node_values_equal_the_python_path(tmp_path):
    import torch
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd import capi, nnmodel
    from webspeechanalyzer_amd.synth import synth_clips
    assert os.path.exists(ADDON), "the N-API addon is built by build()"
    fs = 16000
    s = torch.cuda.current_stream().cuda_stream
    specs = C.model_specs()
    dirs = []
    for i, name in enumerate(HEADS):                 # the app's directories: dist/nnmodel/<db>/ords_<label>/
        d = tmp_path / f"ords_{'VAD'[i]}"
        nnmodel.save_dir(specs[name], str(d))
        dirs.append(str(d))
    an = wsa.Analyzer(wsa.Config(output_level=13))
    models = [an.load_model(d) for d in dirs]
    g = an.regress_group(models)
    step_s = an.config["window_step"] / 1e3
    # the Python path over one stream ...
    pcm = synth_clips(1, 6 * fs, fs=fs, seed=23, device="cuda")
    st = an.streams(1, fs, frames_per_step=F)
    st.set_regress(g)
    sps = st.samples_per_step
    nsteps = pcm.shape[1] // sps
    used = nsteps * sps
    metas, vals, dev_cbs, last = [], [], [], None
    for k in range(nsteps + 1):                      # (the last step is the flush close() makes: STOP without new samples)
        ctl = np.array([wsa.STOP if k == nsteps else wsa.ACTIVE | (wsa.START if k == 0 else 0)], np.uint8)
        st.host_input()[:] = pcm[:, k * sps:(k + 1) * sps].cpu().numpy() if k < nsteps else 0
        st.step_host(ctl, s)
        r = st.collect(s)
        v = st.values()
        metas.append(r["meta"]); vals.append(v["value"])
        dev_cbs += [[int(e[1]), _nums(v["cb_value"][:, q]), 0, _nums(v["cb_weight"][:, q])] for q, e in enumerate(v["cb"])]
        last = v
    st.close()
    meta, value = np.concatenate(metas), np.concatenate(vals, axis=1)
    py_stream = _calls(meta, value, step_s)
    assert len(py_stream) >= 2 and [c[:4] for c in py_stream] == dev_cbs          # the restatement's calls are the device's callbacks
    assert py_stream[-1][5] == _nums(last["stream_value"][:, 0])
    # ... and over the same signal as one clip
    b = an.batch([used], fs)
    x = pcm[:, :used].contiguous()
    b.run(x.data_ptr(), x.stride(0), s)
    b.regress_group(g, s)
    f = b.value_fold(s)
    rows = b.rows(s)
    py_batch = _calls(rows["meta"], f["value"], step_s)
    b.close()
    assert py_batch == py_stream
    values = [dict(sum=_nums(f["clip_sum"][:, 0]), weight=_nums(f["clip_weight"][:, 0]), value=_nums(f["clip_value"][:, 0]))]
    g.close()
    for m in models:
        m.close()
    an.close()
    # a hand-built case with skipped callbacks, through the device's fold
    z = next(c for c in C.batch_cases() if c["name"] == "zero_durations")
    dev = capi.debug_regress_fold(z["meta"], z["values"], z["step_s"], z["row_off"])
    hand = dict(meta=z["meta"].reshape(-1).tolist(), window_step=z["step_s"] * 1e3, cb=dev["cb"].reshape(-1).tolist(), nHeads=3,
                value=_nums(z["values"].reshape(-1)), cbValue=_nums(dev["cb_value"].reshape(-1)), cbWeight=_nums(dev["cb_weight"].reshape(-1)))
    py_hand = []
    for clip in range(len(z["row_off"]) - 1):
        a, e = int(z["row_off"][clip]), int(z["row_off"][clip + 1])
        for c in _calls(z["meta"][a:e], z["values"][:, a:e], z["step_s"], clip):
            py_hand.append(c)
    assert len(py_hand) == len(dev["cb"]) - z["skipped"]

    sig, jp = tmp_path / "x.f32", tmp_path / "job.json"
    pcm[0].cpu().numpy().astype(np.float32).tofile(sig)
    jp.write_text(json.dumps(dict(pcm=str(sig), fs=fs, settings=dict(output_level=13), models=dirs, classifier=CLASSIFIER, frames_per_step=F, hand=hand)))
    r = subprocess.run([NODE, DRIVER, str(jp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    assert got["stream"]["calls"] == py_stream
    assert got["batch"]["calls"] == py_batch
    assert got["stream"]["values"] == values and got["batch"]["values"] == values and got["batch"]["meters"] is None
    assert got["batches"]["calls"] == [py_batch, py_batch] and got["batches"]["values"] == [values, values]
    # beside a prediction model: callback, prediction, values per segment, in that order; the values unchanged
    order = got["both"]["order"]
    assert got["both"]["calls_equal"] and got["both"]["meters"] and got["both"]["values"] == values
    sis = [c[0] for c in py_batch]
    assert [o for o in order if o[0] == "v"] == [["v", si] for si in sis]
    for si in sis:
        assert order.index(["c", si]) < order.index(["p", si]) < order.index(["v", si])
    assert got["independent"] == dict(values_kept=len(py_batch), after_null=True)
    # the hand-built case: no call for the skipped callbacks, running values per clip
    assert got["hand"]["calls"] == py_hand
    ref = got["refusals"]
    assert "a classifier has no value to fold" in ref["classifier"]
    assert "1 .. 8 regression model handles" in ref["nine"] and "1 .. 8 regression model handles" in ref["none"]
    assert "on_values" in ref["no_handler"]
    assert "regression model has no class probabilities" in ref["regression_as_classifier"]
    assert "released" in ref["released"]

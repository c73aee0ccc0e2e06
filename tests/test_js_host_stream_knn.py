"""The Node host's KNN store on live streams and batches (js/formantanalyzer.js setPredictionKnn over the addon's streamSetKnn, batchKnn and
batchKnnFold): for one stream set and one LaunchBatch over the same signal, the on_prediction sequence (si, label, confidence, index) is the
one the Python path gives (knn.Knn.attach + stream_classes, Knn.fold_batch), the meters are the Python path's accumulators, the callback
sequence does not depend on the store, setPredictionModel(null) replaces it, and knnDestroy refuses while the store's context has an open
stream set."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
DRIVER = os.path.join(ROOT, "tests", "js", "stream_knn_host.js")
ADDON = os.path.join(ROOT, "webspeechanalyzer_amd", "lib", "wsa_napi.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]
NAMES = ["ang", "hap", "neu", "sad"]
K, F = 10, 3


def test_node_callbacks_equal_the_python_path(tmp_path):
    import torch
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd import knn
    from webspeechanalyzer_amd.synth import synth_clips
    assert os.path.exists(ADDON), "the N-API addon is built by build()"
    fs = 16000
    s = torch.cuda.current_stream().cuda_stream
    an = wsa.Analyzer(wsa.Config(output_level=13))
    # the store: the level-13 rows of other clips, labelled by row index mod 4
    other = synth_clips(96, 3 * fs, fs=fs, seed=57, device="cuda")
    b = an.batch([other.shape[1]] * 96, fs)
    b.run(other.data_ptr(), other.stride(0), s)
    rows = b.rows(s)["feat"].copy()
    b.close()
    assert len(rows) >= 320
    labels = [NAMES[i % 4] for i in range(len(rows))]
    host = knn.Knn(an, 53, capacity=len(rows))
    host.add(rows, labels)
    # the Python path over one stream ...
    pcm = synth_clips(1, 6 * fs, fs=fs, seed=23, device="cuda")
    st = an.streams(1, fs, frames_per_step=F)
    host.attach(st, K)
    sps = st.samples_per_step
    nsteps = pcm.shape[1] // sps
    used = nsteps * sps
    py_stream, conf = [], None
    for k in range(nsteps + 1):                      # (the last step is the flush close() makes: STOP without new samples)
        ctl = np.array([wsa.STOP if k == nsteps else wsa.ACTIVE | (wsa.START if k == 0 else 0)], np.uint8)
        st.host_input()[:] = pcm[:, k * sps:(k + 1) * sps].cpu().numpy() if k < nsteps else 0
        st.step_host(ctl, s)
        st.collect(s)
        c = host.stream_classes(st)
        py_stream += [[int(e[1]), c["cb_label"][q], float(c["cb_conf"][q]), 0] for q, e in enumerate(c["cb"]) if c["cb_index"][q] != -2]
        conf = c["stream_conf"]
    st.close()
    # ... and over the same signal as one clip
    b = an.batch([used], fs)
    x = pcm[:, :used].contiguous()
    b.run(x.data_ptr(), x.stride(0), s)
    f = host.fold_batch(b, K, s)
    py_batch = [[int(e[1]), f["cb_label"][q], float(f["cb_conf"][q]), 0] for q, e in enumerate(f["cb"]) if f["cb_index"][q] != -2]
    b.close()
    assert len(py_batch) >= 2 and py_stream == py_batch
    meters = [{name: float(conf[0][c]) for c, name in enumerate(NAMES)}]
    host.close(); an.close()

    sig, store, jp = tmp_path / "x.f32", tmp_path / "store.json", tmp_path / "job.json"
    pcm[0].cpu().numpy().astype(np.float32).tofile(sig)
    store.write_text(json.dumps(dict(rows=rows.tolist(), labels=labels)))
    jp.write_text(json.dumps(dict(pcm=str(sig), fs=fs, settings=dict(output_level=13), store=str(store), k=K, frames_per_step=F)))
    r = subprocess.run([NODE, DRIVER, str(jp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    assert [p[:4] for p in got["stream"]["preds"]] == py_stream
    assert [p[:4] for p in got["batch"]["preds"]] == py_batch
    assert got["stream"]["preds"] == got["batch"]["preds"]                  # the per-syllable lists too
    assert got["stream"]["meters"] == meters and got["batch"]["meters"] == meters
    per = got["batch"]["preds"][0][4]
    assert all([lab for lab, _ in syl] != [] and sorted(lab for lab, _ in syl) == NAMES for syl in per)
    assert got["stream"]["callbacks"] == got["plain"]["callbacks"] and got["plain"]["meters"] is None
    assert got["replaced_by_model"] is True
    assert got["step_keys"] == ["knnCb", "knnCbConf", "knnCbLabel", "knnConf", "knnLabel", "knnNClasses", "knnStreamConf"] and got["step_keys_detached"] == []
    assert "open streams" in got["destroy_while_open"]

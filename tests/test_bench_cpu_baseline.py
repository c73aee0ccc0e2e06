"""bench.py's cpu_baseline leg (the only place outside tests/ and smoke() that may run the oracle) on a tiny sample."""
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpu_baseline_reports_node_and_c_ports():
    import bench
    from webspeechanalyzer_amd.synth import synth_clips
    pcm = synth_clips(4, 3 * 16000, fs=16000, seed=3)
    r = bench.cpu_baseline(pcm, 16000, 5, 4)
    assert r["cpu_parity"] == "not compared"
    assert r["unit"] == "frames/s" and r["cores"] == 1 and r["kind"] == "port" and r["value"] > 0
    if shutil.which("node"):
        assert "JS oracle" in r["sample"] and r["c_port"]["value"] > 0
        assert r["many_cores"]["value"] > 0 and r["many_cores"]["cores"] >= 1
    else:
        assert "C oracle" in r["sample"]


@pytest.mark.gpu
def test_bench_multi_rank_code_path_on_one_gpu(tmp_path):
    """bench.py's N > 1 path (clip shards per rank, pipelined slots, the per-step gather to rank 0, max-over-ranks timing)
    with two ranks sharing ONE GPU over gloo (WSA_BENCH_BACKEND test hook; numbers meaningless): the JSON line must come out
    with n_gpus = 2 and twice the frames of one rank per step."""
    import json
    import subprocess
    import sys
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["WSA_BENCH_BACKEND"] = "gloo"
    # no launcher: `bench.py --gpus 2` starts its own two ranks (torch.distributed.run as a child process)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1",
                        "--clips", "48", "--seconds", "4", "--master-port", "29541"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["steps"] == 4 and out["scaling"] == "weak" and "cpu_baseline" not in out
    assert out["rows_gathered_on_rank0_last_step"] >= 2 * out["config"]["feature_rows_per_step_per_gpu"] - 40 and out["backend_reruns"] == 0
    assert out["config"]["frames_per_step_per_gpu"] == 48 * 160
    assert abs(out["value"] * out["ms_per_step"] / 1e3 - 2 * 48 * 160) < 1e-6 * 2 * 48 * 160


def test_dump_outputs_float64_and_seeded_sample_above_the_cap(tmp_path, monkeypatch):
    """bench.py --dump-outputs: every array as float64 .npy; above the cap a fixed sample of rows, the same for arrays of equal length."""
    import numpy as np
    import bench
    meta = np.arange(4000 * 8, dtype=np.int32).reshape(4000, 8)
    feat = np.random.default_rng(1).random((4000, 53))
    bench.dump_outputs(str(tmp_path / "all"), {"meta": meta, "feat": feat})
    assert np.array_equal(np.load(tmp_path / "all" / "meta.npy"), meta.astype(np.float64))
    assert np.load(tmp_path / "all" / "feat.npy").dtype == np.float64 and not (tmp_path / "all" / "feat_rows.npy").exists()
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 1 << 20)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"meta": meta, "feat": feat})
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["feat.npy", "feat_rows.npy", "meta.npy", "meta_rows.npy"]
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= (1 << 20) + 4096
    idx = np.load(tmp_path / "a" / "meta_rows.npy").astype(np.int64)
    assert np.array_equal(idx, np.load(tmp_path / "a" / "feat_rows.npy")) and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "feat.npy"), feat[idx]) and np.array_equal(np.load(tmp_path / "a" / "meta.npy"), meta[idx])
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W`: one timed region of exactly K steps, the headline fields only, and with
    --dump-outputs the rows of the last timed step, identical from run to run (seeded inputs)."""
    import json
    import subprocess
    import sys
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--clips", "32",
                            "--seconds", "3", "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    out = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out
    assert out["steps"] == 5 and out["repeats"]["n"] == 1 and out["ms_per_step"] > 0
    assert out["config"]["frames_per_step_per_gpu"] == 32 * 120
    assert abs(out["value"] * out["ms_per_step"] / 1e3 - 32 * 120) < 1e-6 * 32 * 120
    assert not {"roofline", "issue_bound", "single_batch", "extra", "cpu_baseline"} & set(out)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["feat.npy", "meta.npy", "row_off.npy", "seg_off.npy", "segments.npy"]
    feat, meta, roff = (np.load(tmp_path / "a" / n) for n in ("feat.npy", "meta.npy", "row_off.npy"))
    assert feat.dtype == np.float64 and feat.shape == (out["config"]["feature_rows_per_step_per_gpu"], 53) and feat.shape[0] > 0
    assert meta.shape == (feat.shape[0], 8) and roff.shape == (33,) and roff[-1] == feat.shape[0]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), n

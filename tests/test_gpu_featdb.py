"""The device feature DB on the GPU (specification FD-1; kernels K10, csrc/featdb.hip): every comparison is bit for bit,
against tests/featdb_ref.py or against the host-row path that existed before (wsa_trainer_create, wsa_wide_dbstats_create, Knn.add)."""
import os

import numpy as np
import pytest

from tests import featdb_cases as fc
from tests import featdb_ref
from webspeechanalyzer_amd import capi, dbstats, featdb, knn, nnmodel, train

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def an():
    a = capi.Analyzer(capi.Config(output_level=13), device=0)
    yield a
    a.close()


def _s(torch):
    return torch.cuda.current_stream().cuda_stream


def _sizes():
    wave, wg, per_pass = capi.FeatDB.tile_info()
    assert (wave, wg) == (64, 1024) and per_pass % wg == 0 and per_pass > wg
    return wave, wg, per_pass


COUNTS = ["0", "1"] + [f"{name}{d:+d}" for name in ("wave", "workgroup", "pass") for d in (-1, 0, 1)]


# ---- keep, scan and copy on hand-built tables
@pytest.mark.parametrize("count", COUNTS)
def test_append_every_row_at_the_tile_sizes(torch, an, count):
    sizes = dict(zip(("wave", "workgroup", "pass"), _sizes()))
    n = int(count) if count in ("0", "1") else sizes[count[:-2]] + int(count[-2:])
    feat = fc.feature_table(n, 53, 7) if n else np.zeros((0, 53))
    db = an.device_db(53, n + 5)
    head = fc.feature_table(3, 53, 8)
    db.append_host(head)
    first, kept = capi.debug_featdb_append(db, 13, None, feat, None, _s(torch))
    want_kept, want_rows = featdb_ref.append(13, head, feat=feat)
    assert first == 3 and np.array_equal(kept, want_kept) and db.count == 3 + n
    assert featdb_ref.same_bits(db.copy_rows(), want_rows)
    db.close()
    # levels 5 / 13 need no keep kernel: the same count through level 12's, marks in the table's fixed places
    meta, feat12 = fc.l12_seam_table(n, [])
    db = an.device_db(23, n + 1)
    first, kept = capi.debug_featdb_append(db, 12, meta, feat12, None, _s(torch))
    want_kept, want_rows = featdb_ref.append(12, np.zeros((0, 23)), meta, feat12)
    assert first == 0 and np.array_equal(kept, want_kept) and (n < 64 or 0 < len(kept) < n)
    assert featdb_ref.same_bits(db.copy_rows(), want_rows)
    db.close()


def test_level_12_marks_across_every_seam(torch, an):
    wave, wg, per_pass = _sizes()
    n = per_pass + per_pass // 2 + 3 * wave + 7
    # callbacks across a wave seam, a workgroup seam (also a wave seam), a seam of both further in, and source row `per_pass`; each is
    # marked on the last row before its seam.  More rows are kept than one pass of the copy kernel takes, so its grid loops; its own seam,
    # which counts KEPT rows, is met exactly by the all-kept tables of per_pass and per_pass + 1 rows below
    seams = [wave, 2 * wave, wg, 2 * wg, 5 * wg + 3 * wave, per_pass]
    meta, feat = fc.l12_seam_table(n, seams)
    kept_want = featdb_ref.keep(12, meta, feat)
    assert len(kept_want) > per_pass + wave                       # the copy kernel's grid is capped: more than one pass
    for s in seams:
        assert s - 2 in kept_want and s not in kept_want and s + 2 not in kept_want and s + 3 in kept_want
    db = an.device_db(23, n)
    first, kept = capi.debug_featdb_append(db, 12, meta, feat, None, _s(torch))
    want_kept, want_rows = featdb_ref.append(12, np.zeros((0, 23)), meta, feat)
    assert first == 0 and np.array_equal(kept, want_kept) and db.count == len(want_kept)
    assert featdb_ref.same_bits(db.copy_rows(), want_rows)
    # every row kept, exactly one pass of the copy kernel and one row more
    for m in (per_pass, per_pass + 1):
        db.clear()
        meta2, feat2 = fc.meta_table([(0, r // 3) for r in range(m)]), fc.feature_table(m, 53, 9)
        feat2[:, 23] = 0.0
        first, kept = capi.debug_featdb_append(db, 12, meta2, feat2, None, _s(torch))
        assert np.array_equal(kept, np.arange(m)) and featdb_ref.same_bits(db.copy_rows(), feat2[:, :23])
    db.close()


@pytest.mark.parametrize("name", sorted(fc.L12_SMALL))
def test_level_12_small_cases(torch, an, name):
    meta, feat = fc.l12_small(name)
    db = an.device_db(23, 8)
    first, kept = capi.debug_featdb_append(db, 12, meta, feat, None, _s(torch))
    assert kept.tolist() == fc.L12_SMALL[name]["kept"] and db.count == len(kept)
    assert featdb_ref.same_bits(db.copy_rows(), feat[kept.tolist(), :23] if len(kept) else np.zeros((0, 23)))
    db.close()


def test_level_11_last_utterance_row_per_clip(torch, an):
    wave, wg, _ = _sizes()
    for name, c in sorted(fc.L11_SMALL.items()):
        off = np.array(c["off"], np.uint32)
        feat = fc.feature_table(max(int(off[-1]), 1), 264, 5)[:int(off[-1])]
        db = an.device_db(264, 4)
        _, kept = capi.debug_featdb_append(db, 11, None, feat if len(feat) else np.zeros((0, 264)), off, _s(torch))
        assert kept.tolist() == c["kept"], name
        assert featdb_ref.same_bits(db.copy_rows(), feat[c["kept"]] if c["kept"] else np.zeros((0, 264)))
        db.close()
    for n_clips in (wave - 1, wave + 1, wg + 1):
        off, feat = fc.l11_table(n_clips)
        db = an.device_db(264, n_clips)
        _, kept = capi.debug_featdb_append(db, 11, None, feat, off, _s(torch))
        want_kept, want_rows = featdb_ref.append(11, np.zeros((0, 264)), feat=feat, off=off)
        assert np.array_equal(kept, want_kept) and featdb_ref.same_bits(db.copy_rows(), want_rows)
        db.close()


# ---- append_batch
def _synth_batch(torch, level):
    from webspeechanalyzer_amd.synth import synth_clips
    fs, ns = 16000, 32000
    pcm = synth_clips(3, ns, fs=fs, seed=3, device="cuda")
    a = capi.Analyzer(capi.Config(output_level=level), device=0)
    b = a.batch([ns] * 3, fs)
    b.run(pcm.data_ptr(), pcm.stride(0), _s(torch))
    return a, b


def _source(b, level, stream):
    if level == 11:
        u = b.utterance(stream)
        return dict(meta=None, feat=u["feat"], off=u["off"])
    r = b.rows(stream)
    return dict(meta=r["meta"], feat=r["feat"], off=None)


@pytest.mark.parametrize("level", [5, 13, 11])
def test_append_batch_twice_and_capacity(torch, level):
    a, b = _synth_batch(torch, level)
    s = _s(torch)
    src = _source(b, level, s)
    W = featdb_ref.WIDTH[level]
    want_kept, want_rows = featdb_ref.append(level, np.zeros((0, W)), **src)
    n = len(want_kept)
    assert n >= 2
    db = a.device_db(W, 2 * n)                                    # exactly full after the second append
    first, kept = db.append_batch(b, s)
    assert first == 0 and np.array_equal(kept, want_kept) and featdb_ref.same_bits(db.copy_rows(), want_rows)
    first, kept = db.append_batch(b, s)
    assert first == n and np.array_equal(kept, want_kept) and db.count == 2 * n
    assert featdb_ref.same_bits(db.copy_rows(), np.concatenate([want_rows, want_rows]))
    with pytest.raises(capi.WsaError, match=rf"holds {2 * n} rows, {n} rows to add do not fit its capacity of {2 * n}"):
        db.append_batch(b, s)
    assert db.count == 2 * n and featdb_ref.same_bits(db.copy_rows(), np.concatenate([want_rows, want_rows]))
    db.close()
    small = a.device_db(W, n - 1)                                 # one row short
    small.append_host(want_rows[:0])
    with pytest.raises(capi.WsaError, match="do not fit its capacity"):
        small.append_batch(b, s)
    assert small.count == 0
    small.close(); b.close(); a.close()


def test_append_batch_level_12_throw_fixture(torch):
    cap = np.load(os.path.join(GOLD, "gen", "captured_l12_throw.npy"))
    cfg = capi.Config(output_level=12, N_mel_bins=int(cap.shape[1]), window_step=15.0, window_width=15.0, pause_length=100.0, min_seg_length=100.0,
                      auto_noise_gate=0, voiced_max_dB=140.0, voiced_min_dB=10.0)
    a = capi.Analyzer(cfg, device=0)
    g = a.geometry(16000)
    b = a.batch([g["win"] + (len(cap) - 1) * g["hop"]], 16000)
    d = torch.from_numpy(np.ascontiguousarray(cap).view(np.int32)).cuda()
    s = _s(torch)
    b.run_backend(d.data_ptr(), s)
    r = b.rows(s)
    want_kept, want_rows = featdb_ref.append(12, np.zeros((0, 23)), r["meta"], r["feat"])
    assert 0 < len(want_kept) < len(r["meta"])                    # the fixture has a thrown syllable
    db = featdb.DeviceDB(a, 12, len(r["meta"]))
    new = db.append(b, ["throw.wav"], s)
    assert [x["row"] for x in new] == list(range(len(want_kept))) and featdb_ref.same_bits(db.copy_rows(), want_rows)
    want_rec = featdb.records(12, 0.015, r["meta"], want_kept.tolist(), ["throw.wav"])
    assert [(x["seg"], x["time"]) for x in new] == [(x["seg"], x["time"]) for x in want_rec]
    with pytest.raises(ValueError, match="already holds 'throw.wav'"):
        db.append(b, ["throw.wav"], s)
    db.close(); b.close(); a.close()


def test_refusals(torch, an):
    s = _s(torch)
    with pytest.raises(capi.WsaError, match="feature DB of 63"):
        an.device_db(63, 4)
    with pytest.raises(capi.WsaError, match="at least one row"):
        an.device_db(53, 0)
    a5, b5 = _synth_batch(torch, 5)
    db23, db53 = a5.device_db(23, 64), a5.device_db(53, 64)
    with pytest.raises(capi.WsaError, match=r"output_level 5 .* 23 features"):
        db23.append_batch(b5, s)
    other = an.device_db(53, 64)
    with pytest.raises(capi.WsaError, match="another context"):
        other.append_batch(b5, s)
    fresh = a5.batch([32000], 16000)
    with pytest.raises(capi.WsaError, match="no run"):
        db53.append_batch(fresh, s)
    assert db53.count == 0 and db23.count == 0 and other.count == 0
    db53.append_batch(b5, s)
    n = db53.count
    out = torch.zeros((2, 53), dtype=torch.float64, device="cuda")
    with pytest.raises(capi.WsaError, match=rf"rows\[1\] = {n} is outside"):
        db53.gather([0, n], out.data_ptr(), s)
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()                            # refused before anything ran
    with pytest.raises(capi.WsaError, match=rf"rows\[0\] = {n + 7} is outside"):
        db53.ranges([n + 7], s)
    spec = _spec([53, 4, 2], ["relu", "softmax"], np.zeros(53), np.ones(53), ["a", "b"])
    rows = [i % n for i in range(12)]
    with pytest.raises(capi.WsaError, match=rf"rows\[3\] = {n} is outside"):
        db53.trainer(spec, rows[:3] + [n] + rows[4:], [0, 1] * 6, 2, 4, 0.1)
    with pytest.raises(capi.WsaError, match="another context"):
        capi.Trainer(an, spec, rows, [0, 1] * 6, 2, 4, 0.1, db=db53)
    spec23 = _spec([23, 4, 2], ["relu", "softmax"], np.zeros(23), np.ones(23), ["a", "b"])
    with pytest.raises(capi.WsaError, match="takes 23 inputs; the DB's rows have 53"):
        db53.trainer(spec23, rows, [0, 1] * 6, 2, 4, 0.1)
    with pytest.raises(capi.WsaError, match="n_val 12 leaves no training rows"):
        db53.trainer(spec, rows, [0, 1] * 6, 12, 4, 0.1)
    for d in (db23, db53, other):
        d.close()
    fresh.close(); b5.close(); a5.close()


# ---- gather and ranges
def test_gather_and_ranges(torch, an):
    s = _s(torch)
    n = 300
    feat = fc.feature_table(n, 53, 11)
    nan_cols = np.isnan(feat).any(axis=0)
    feat[:, 1] = np.where(np.arange(n) % 2 == 0, -0.0, 0.0)      # one column with both zeros
    feat[:, 2] = np.nan_to_num(feat[:, 2], nan=1.0); feat[7, 2] = np.nan      # one column with one NaN
    feat[:, 3:9] = np.nan_to_num(feat[:, 3:9], nan=-3.5)          # columns without NaN and without a zero of either sign
    feat[:, 3:9] = np.where(feat[:, 3:9] == 0, 1.25, feat[:, 3:9])
    db = an.device_db(53, n)
    db.append_host(feat, s)
    for rows in ([5], [(i * 37) % n for i in range(257)], [3, 3, 299, 0, 3, 299]):
        out = torch.full((len(rows), 53), -1.0, dtype=torch.float64, device="cuda")
        db.gather(rows, out.data_ptr(), s)
        torch.cuda.synchronize()
        assert featdb_ref.same_bits(out.cpu().numpy(), feat[rows])
        mn, mx = db.ranges(rows, s)
        wmn, wmx = featdb_ref.ranges(feat[rows])
        assert featdb_ref.same_bits(mn, wmn) and featdb_ref.same_bits(mx, wmx)
        plain = ~np.isnan(feat[rows]).any(axis=0) & ~((feat[rows] == 0).any(axis=0))
        assert plain[3:9].all() and np.array_equal(mn[plain], feat[rows].min(axis=0)[plain]) and np.array_equal(mx[plain], feat[rows].max(axis=0)[plain])
    mn, mx = db.ranges(None, s)
    assert np.isnan(mn[2]) and np.isnan(mx[2]) and np.signbit(mn[1]) and mn[1] == 0 and not np.signbit(mx[1]) and mx[1] == 0
    assert featdb_ref.same_bits(mn, featdb_ref.ranges(feat)[0]) and featdb_ref.same_bits(mx, featdb_ref.ranges(feat)[1])
    assert nan_cols.any()
    db.close()


# ---- trainers
def _spec(units, acts, in_min, in_max, labels, out=None):
    ks, bs = train.glorot_init(units, 5)
    if out is None:
        return nnmodel.ModelSpec(list(units), list(acts), ks, bs, np.asarray(in_min, np.float64), np.asarray(in_max, np.float64), list(labels))
    return nnmodel.ModelSpec(list(units), list(acts), ks, bs, np.asarray(in_min, np.float64), np.asarray(in_max, np.float64), [], out[0], out[1])


def _finite(n, width, seed):
    return np.nan_to_num(fc.feature_table(n, width, seed), nan=0.5, posinf=7.0)


TRAIN_CASES = {
    "default_53": dict(units=[53, 8, 3], acts=["relu", "softmax"], lr=0.2),          # the app's default stack (src/neuralmodel_aux.js:106-124)
    "small_23": dict(units=[23, 5, 2], acts=["tanh", "softmax"], lr=0.1),
    "small_264": dict(units=[264, 6, 4], acts=["sigmoid", "softmax"], lr=0.1),
    "regress_53": dict(units=[53, 64, 16, 1], acts=["sigmoid", "sigmoid", "sigmoid"], lr=0.2, regress=True),
}
N_ROWS, N_VAL, BATCH, EPOCHS = 37, 4, 32, 2                       # 33 training rows: the second step is ragged


def _train_pair(an, key):
    """(db-made trainer, host-made trainer, orders) of a case: 37 rows with duplicates out of a DB of 20"""
    c = TRAIN_CASES[key]
    W = c["units"][0]
    feat = _finite(20, W, 13)
    db = an.device_db(W, 24)
    db.append_host(feat[:9]); db.append_host(feat[9:])
    rows = [(i * 7 + i // 5) % 20 for i in range(N_ROWS)]
    assert len(set(rows)) < N_ROWS
    in_min, in_max = db.ranges(rows)
    assert np.array_equal(in_min, feat[rows].min(axis=0)) and np.array_equal(in_max, feat[rows].max(axis=0))
    orders = train.epoch_orders(N_ROWS - N_VAL, EPOCHS, 3)
    if c.get("regress"):
        y = np.array([((i * 29) % 17) / 16.0 for i in range(N_ROWS)])
        spec = _spec(c["units"], c["acts"], in_min, in_max, [], (float(y.min()), float(y.max())))
        a = db.regress_trainer(spec, rows, y, N_VAL, BATCH, c["lr"])
        b = an.regress_trainer(spec, feat[rows], y, N_VAL, BATCH, c["lr"])
    else:
        C = c["units"][-1]
        y = np.array([(i * 5) % C for i in range(N_ROWS)], np.int32)
        spec = _spec(c["units"], c["acts"], in_min, in_max, [f"c{j}" for j in range(C)])
        a = db.trainer(spec, rows, y, N_VAL, BATCH, c["lr"])
        b = an.trainer(spec, feat[rows], y, N_VAL, BATCH, c["lr"])
    db.append_host(feat[:4])                                      # the trainer keeps no reference: append, then destroy
    db.close()
    return a, b, orders


def _state(tr):
    st = tr.stats()
    ks, bs = tr.weights()
    return b"".join(k.tobytes() for k in ks) + b"".join(x.tobytes() for x in bs) + np.array([st[k] for k in ("epochs_done", "loss", "acc", "val_loss", "val_acc")], np.float64).tobytes()


@pytest.mark.parametrize("key", sorted(TRAIN_CASES))
def test_trainer_from_the_db_equals_the_host_trainer(an, key):
    a, b, orders = _train_pair(an, key)
    assert _state(a) == _state(b)
    for o in orders:
        a.epoch(o); b.epoch(o)
        sa, sb = _state(a), _state(b)
        assert sa == sb
    assert a.stats()["epochs_done"] == EPOCHS and np.isfinite(a.stats()["loss"])
    a.close(); b.close()


def test_training_group_mixes_db_and_host_members(an):
    a0, b0, orders = _train_pair(an, "default_53")
    a1, b1, _ = _train_pair(an, "regress_53")
    for o in orders:                                              # solo: the host-made classifier, the DB-made regression model
        b0.epoch(o); a1.epoch(o)
    g = an.train_group([a0, b1])                                  # group: the DB-made classifier, the host-made regression model
    for o in orders:
        g.epoch([o, o])
    g.stats()
    assert _state(a0) == _state(b0) and _state(b1) == _state(a1)
    g.close()
    for t in (a0, b0, a1, b1):
        t.close()


# ---- DB statistics and KNN
def test_dbstats_from_the_db_equals_the_host_db(torch, an):
    s = _s(torch)
    n = 300                                                       # more than one chunk of K8
    feat = _finite(n, 53, 17)
    db = an.device_db(53, n)
    db.append_host(feat, s)
    dur = np.array([0.25 + (i % 9) / 8 for i in range(n)])
    spec = _spec([53, 8, 3], ["relu", "softmax"], feat.min(axis=0), feat.max(axis=0), ["a", "b", "c"])
    rspec = _spec([53, 6, 1], ["sigmoid", "sigmoid"], feat.min(axis=0), feat.max(axis=0), [], (0.0, 2.0))
    m, rm = an.load_model(spec), an.load_model(rspec)
    t_idx = np.array([i % 4 - 1 for i in range(n)], np.int32)
    t_val = np.array([np.nan if i % 5 == 0 else (i % 7) / 3 for i in range(n)])
    got = []
    for src in (db, feat):
        st = an.feature_db(src, dur, [3], 1)
        st.set_classes(0, t_idx); st.set_values(0, t_val)
        st.predict_classes(0, m, np.arange(3), s); st.predict_values(0, rm, None, None, s)
        cat, cls, od = st.table(s)
        got.append((cat.tobytes(), cls.tobytes(), od.tobytes(), st.pred_classes(0, s).tobytes(), st.pred_values(0, s).tobytes(), st.probs(3, s).tobytes()))
        st.close()
    assert got[0] == got[1]
    assert len(set(np.frombuffer(got[0][3], np.int32).tolist())) > 1
    # a range that does not start at row 0: the offset into the DB's table
    got = []
    for src, first in ((db, 37), (feat[37:187], 0)):
        st = an.feature_db(src, dur[37:187], [3], 1, first_row=first)
        st.set_classes(0, t_idx[37:187]); st.set_values(0, t_val[37:187])
        st.predict_classes(0, m, np.arange(3), s); st.predict_values(0, rm, None, None, s)
        cat, cls, od = st.table(s)
        got.append((cat.tobytes(), cls.tobytes(), od.tobytes(), st.pred_classes(0, s).tobytes(), st.pred_values(0, s).tobytes(), st.probs(3, s).tobytes()))
        st.close()
    assert got[0] == got[1]
    with pytest.raises(capi.WsaError, match="rows 295 .. 305 are outside the DB's 300 rows"):
        an.feature_db(db, dur[:10], [3], 0, first_row=295)
    with pytest.raises(TypeError, match="featdb.DeviceDB"):
        dbstats.predict_db(an, db, ([], []), "cats", "x", spec)
    m.close(); rm.close(); db.close()


def test_knn_filled_from_the_db_equals_one_filled_from_host_rows(an):
    n = 90
    feat = _finite(n, 53, 19)
    db = an.device_db(53, n)
    db.append_host(feat)
    rows = [(i * 11) % n for i in range(70)]
    labels = ["abc"[i % 3 if i % 4 else 1] for i in range(70)]
    a, b = knn.Knn(an, 53, 128), knn.Knn(an, 53, 128)
    a.add_db(db, rows[:40], labels[:40]); a.add_db(db, rows[40:], labels[40:])
    b.add(feat[rows[:40]], labels[:40]); b.add(feat[rows[40:]], labels[40:])
    assert a.count() == b.count() and a.classes == b.classes
    q = _finite(33, 53, 23)
    ra, rb = a.classify(q, 10), b.classify(q, 10)
    assert ra["label"] == rb["label"] and all(ra[k].tobytes() == rb[k].tobytes() for k in ("index", "conf", "nbr", "sim"))
    with pytest.raises(capi.WsaError, match=r"rows\[0\] = 90 is outside"):
        a.add_db(db, [90], ["a"])
    a.close(); b.close(); db.close()


# ---- end to end: batch -> DeviceDB -> prepare_db -> train -> predict_db -> stats_table, against the host-row path
def test_end_to_end_equals_the_host_row_path(torch):
    from webspeechanalyzer_amd.synth import synth_clips
    fs, ns, nc = 16000, 48000, 8
    s = _s(torch)
    pcm = synth_clips(nc, ns, fs=fs, seed=3, device="cuda")
    a = capi.Analyzer(capi.Config(output_level=13), device=0)
    b = a.batch([ns] * nc, fs)
    b.run(pcm.data_ptr(), pcm.stride(0), s)
    files = [f"clip{c}.wav" for c in range(nc)]
    r = b.rows(s)
    n = len(r["meta"])
    assert n >= 12, f"{n} rows"
    host_rows = [dict({k: v for k, v in rec.items() if k != "row"}, features=[float(x) for x in f])
                 for rec, f in zip(featdb.records(13, 0.025, r["meta"], list(range(n)), files), r["feat"])]
    db = featdb.DeviceDB(a, 13, n)
    db.append(b, files, s)
    got_rows = db.to_rows(s)
    assert [{k: v for k, v in x.items() if k != "features"} for x in got_rows] == [{k: v for k, v in x.items() if k != "features"} for x in host_rows]
    assert featdb_ref.same_bits([x["features"] for x in got_rows], r["feat"]) and featdb_ref.same_bits(db.copy_rows(), r["feat"])
    labels = [("low", "high", None)[i % 3 if i % 7 else 0] for i in range(n)]
    heads = ([{"emotion": ["low", "high"]}], [])
    for rows in (db.records, host_rows):
        for rec, lab in zip(rows, labels):
            rec["true"] = None if lab is None else [{"emotion": lab}, {}]
    d_db, d_host = train.prepare_db(db, labels, ["low", "high"], s), train.prepare(r["feat"], labels, ["low", "high"])
    assert d_db["rows"] == d_host["rows"] and np.array_equal(d_db["in_min"], d_host["in_min"]) and np.array_equal(d_db["in_max"], d_host["in_max"])
    spec_db, hist_db = train.train(a, d_db, epochs=2, seed=4, stream=s)
    spec_host, hist_host = train.train(a, d_host, epochs=2, seed=4, stream=s)
    assert hist_db == hist_host and spec_db.labels == spec_host.labels and spec_db.units == spec_host.units
    assert all(x.tobytes() == y.tobytes() for x, y in zip(spec_db.kernels + spec_db.biases, spec_host.kernels + spec_host.biases))
    p_db = dbstats.predict_db(a, db, heads, "cats", "emotion", spec_db, stream=s, return_raw=True)
    p_host = dbstats.predict_db(a, host_rows, heads, "cats", "emotion", spec_host, stream=s, return_raw=True)
    assert p_db[0] == p_host[0] and p_db[1].tobytes() == p_host[1].tobytes()
    assert [x["pred"] for x in db.records] == [x["pred"] for x in host_rows]
    assert dbstats.stats_table(a, db, *heads, stream=s) == dbstats.stats_table(a, host_rows, *heads, stream=s)
    db.close(); b.close(); a.close()

"""K8e on the GPU (csrc/dbeval.hip through capi): the confusion matrix, the agreement and the per-file results against the restatement of
specification EV-1 (tests/dbeval_ref.py) — counts exactly, every f64 bit for bit (one NaN) — at the smallest shapes where the kernels
can go wrong (tests/dbeval_cases.py), on objects made in all three ways, with the invariants against wsa_dbstats_table, whose own output
stays byte-identical, and a file's meter sums against Batch's own fold."""
import numpy as np
import pytest

from webspeechanalyzer_amd import capi, dbstats, featdb

from . import dbeval_cases as dc
from . import dbeval_ref as ref
from . import dbstats_ref

pytestmark = pytest.mark.gpu

HEAD_V = [1, 2, 64, 65, 256, 33, 32, 7]                     # 8 categorical heads: every vocabulary of the issue, and the band edge 32 | 33
HEAD_ORD = ["special", "infinite", "clean", "empty", "constant", "special", "clean", "infinite"]


@pytest.fixture(scope="module")
def an():
    a = capi.Analyzer(capi.Config(output_level=13), device=0)
    yield a
    a.close()


@pytest.fixture(scope="module")
def s():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _bytes(tables):
    return [t.tobytes() for t in tables]


def _check_agreement(got, want_list):
    for o, want in enumerate(want_list):
        assert int(got["n"][o]) == want["n"], (o, got["n"][o], want["n"])
        for k in ref.KEYS:
            assert ref.same_f64([got[k][o]], [want[k]]), f"head {o} {k}: {got[k][o]!r} != {want[k]!r}"
            if got[k][o] != got[k][o]:
                assert np.array([got[k][o]]).view(np.uint64)[0] == 0x7FF8000000000000, "K8e writes one NaN"


def _invariants(m, V, cat_h, cls_h):
    for v in range(V):
        assert sum(m[v]) == cls_h["count"][v] and m[v][v] == cls_h["correct"][v] and sum(m[v][:V]) - m[v][v] == cls_h["wrong"][v], v
    assert sum(m[v][V] for v in range(V)) == cat_h["blank"]


@pytest.mark.parametrize("n", dc.ROWS)
def test_eight_heads_of_each_kind_are_the_restatement(an, s, n):
    dur = 0.25 + (np.arange(n) % 9) / 8
    cats = [dc.class_columns(n, V, 100 * V + n) for V in HEAD_V]
    ords = [dc.ordinal_columns(n, 7 * o + n, variant) for o, variant in enumerate(HEAD_ORD)]
    db = an.feature_db(None, dur, HEAD_V, len(ords))
    for h, (t, p) in enumerate(cats):
        db.set_classes(h, t, p)
    for o, (t, p) in enumerate(ords):
        db.set_values(o, t, p)
    before = _bytes(db.table(s))
    agree = db.agreement(s)
    matrices = [db.confusion(h, s) for h in range(len(HEAD_V))]
    again = [db.confusion(h, s) for h in (4, 0)] + [db.agreement(s)]
    cat, cls, od = db.table(s)
    assert _bytes((cat, cls, od)) == before, "wsa_dbstats_table's output changed across the new calls"
    db.close()
    assert again[0].tobytes() == matrices[4].tobytes() and again[1].tobytes() == matrices[0].tobytes() and again[2].tobytes() == agree.tobytes()
    off = 0
    for h, (V, (t, p)) in enumerate(zip(HEAD_V, cats)):
        assert matrices[h].shape == (V, V + 1) and matrices[h].tolist() == ref.confusion(V, t, p), f"head {h} (V = {V})"
        _invariants(matrices[h].tolist(), V, cat[h], cls[off:off + V])
        off += V
    want = [ref.agreement(t, p) for t, p in ords]
    _check_agreement(agree, want)
    assert [int(x) for x in agree["n"]] == [int(x) for x in od["pred_n"]]               # n is the table's pred_n: both columns pass DS-1's rule
    if n >= 40:
        assert want[3]["n"] == 0 and want[4]["var_true"] == 0 and want[0]["n"] > 0 and want[1]["mean_true"] != want[1]["mean_true"]


@pytest.mark.parametrize("V", [2, 65, 256])
@pytest.mark.parametrize("variant", ["blank", "none", "one"])
def test_confusion_edges_have_one_hot_counter(an, s, variant, V):
    n = 513
    t, p = dc.class_columns(n, V, 3 + V, variant)
    db = an.feature_db(None, np.ones(n), [V], 0)
    db.set_classes(0, t, p)
    m = db.confusion(0, s)
    cat, cls, _ = db.table(s)
    db.close()
    assert m.tolist() == ref.confusion(V, t, p)
    _invariants(m.tolist(), V, cat[0], cls)
    if variant == "one":
        assert np.count_nonzero(m) == 1 and int(m.max()) == n and int(np.trace(m[:, :V])) == 0
    if variant == "none":
        assert not m.any()
    if variant == "blank":
        assert int(m[:, V].sum()) == n and not m[:, :V].any()


def test_groups_of_several_chunks(an, s):
    """more than 64 chunks: K8e's confusion deals two chunks to a group, and the agreement's second pass runs its LDS window once more"""
    n, V = 70 * dc.R + 5, 65
    t, p = dc.class_columns(n, V, 9)
    tv, pv = dc.ordinal_columns(n, 9, "special")
    db = an.feature_db(None, np.ones(n), [V], 1)
    db.set_classes(0, t, p)
    db.set_values(0, tv, pv)
    m, agree = db.confusion(0, s), db.agreement(s)
    db.close()
    assert m.tolist() == ref.confusion(V, t, p)
    _check_agreement(agree, [ref.agreement(tv, pv)])
    n = 300 * dc.R + 17                                       # more than 256 chunks: the sums' window moves
    tv, pv = dc.ordinal_columns(n, 10, "clean")
    db = an.feature_db(None, np.ones(n), [], 1)
    db.set_values(0, tv, pv)
    agree = db.agreement(s)
    db.close()
    _check_agreement(agree, [ref.agreement(tv, pv)])


# ---- per file
def _file_case(an, s, lay, V, width, kind, maker="host", seed=1):
    """One object with one categorical head (64 model classes mapped into V entries) and one ordinal head, files set, both folded;
    returns everything the checks need, the restatement's results among it."""
    f_col, c_col, dur, n_files = lay["file_of_row"], lay["callback_of_row"], lay["durations"], lay["n_files"]
    n = len(f_col)
    C = dc.MODEL_CLASSES
    feat = dc.features(n, width, seed)
    spec = dc.model_spec(width, C, seed, kind)
    lmap = dc.legend_to_vocab(C, V)
    t_idx, _ = dc.class_columns(n, V, seed + 1)
    tv, pv = dc.ordinal_columns(n, seed + 2, "infinite")
    src, held = feat, None
    if maker == "featdb":
        held = an.device_db(width, n + 3)
        held.append_host(np.vstack([dc.features(3, width, 99), feat]), s)      # a range that does not start at row 0
        src = held
    db = an.feature_db(src, dur, [V], 1, first_row=3 if maker == "featdb" else 0)
    model = an.load_model(spec)
    try:
        db.set_classes(0, t_idx)
        db.set_values(0, tv, pv)
        db.set_files(f_col, c_col, n_files)
        rng = np.random.default_rng(seed + 3)
        ft, fv = rng.integers(-1, V, n_files).astype(np.int32), np.where(rng.random(n_files) < 0.2, np.nan, 1 + 8 * rng.random(n_files))
        db.set_file_classes(0, ft.astype(np.int64))          # (another dtype: the binding converts, and keeps the copy alive over the call)
        db.set_file_values(0, [float(v) for v in fv])
        before = _bytes(db.table(s))
        db.predict_classes(0, model, lmap, s)
        row_table = _bytes(db.table(s))
        db.fold_files(0, s)
        db.fold_file_values(0, s)
        got = dict(prob=db.probs(C, s), sums=db.file_sums(0, C, s), classes=db.file_classes(0, s), values=db.file_values(0, s),
                   table=db.file_table(s), confusion=db.file_confusion(0, s), agreement=db.file_agreement(s), pred_rows=db.pred_classes(0, s))
        assert _bytes(db.table(s)) == row_table and before != row_table, "the folds touched the row-level table, or the prediction did not reach it"
    finally:
        model.close()
        db.close()
        if held is not None:
            held.close()
    ref.ARMS.clear()
    sums, classes = ref.fold_files(f_col, c_col, dur, got["prob"], list(spec.labels), lmap, n_files)
    values = ref.fold_file_values(f_col, c_col, dur, pv, n_files)
    got.update(want_sums=sums, want_classes=classes, want_values=values, arms=dict(ref.ARMS), file_true=(ft, fv), labels=list(spec.labels), lmap=lmap)
    return got


def _check_file_case(g, lay, V):
    n_files = lay["n_files"]
    assert g["classes"].tolist() == g["want_classes"].tolist()
    assert ref.same_f64(g["sums"], g["want_sums"]), "meter sums differ from the restatement"
    assert ref.same_f64(g["values"], g["want_values"]), "file values differ from the restatement"
    ft, fv = g["file_true"]
    want = dbstats_ref.table(ref.file_durations(lay["file_of_row"], lay["durations"], n_files), [(V, ft, g["want_classes"])], [(fv, g["want_values"])])
    for name, a, b in zip(("cat", "cls", "ord"), g["table"], want):
        for f in b.dtype.names:
            assert a[f].tobytes() == b[f].tobytes(), f"file table {name}.{f}"
    assert g["confusion"].tolist() == ref.confusion(V, ft, g["want_classes"])
    _check_agreement(g["agreement"], [ref.agreement(fv, g["want_values"])])


@pytest.mark.parametrize("name", ["one_row_per_file", "chunk_sizes", "straddle", "one_syllable", "gap_inside", "empty_file"])
def test_file_layouts_are_the_restatement(an, s, name):
    lay = dc.file_layout(name)
    V = {"one_row_per_file": 256, "chunk_sizes": 65, "straddle": 64, "one_syllable": 2, "gap_inside": 1, "empty_file": 65}[name]
    g = _file_case(an, s, lay, V, 53, "random", seed=len(name))
    _check_file_case(g, lay, V)
    arms = g["arms"]
    if name == "straddle":
        assert arms.get("file.none", 0) > 0 and arms.get("callback.one_syllable", 0) >= 7 and arms.get("value.not_finite", 0) > 0
    if name == "one_syllable":
        assert "callback.several" not in arms
    if name == "empty_file":
        assert g["classes"][1] == -1 and g["values"][1] != g["values"][1] and not g["sums"][1].any()
    if name == "one_row_per_file":                            # a file of one row: its class is the row's own decision unless the syllable has no length
        keep = lay["durations"] > 0
        assert (g["classes"][keep] == g["pred_rows"][keep]).all() and (g["classes"][~keep] == -1).all() and (~keep).any()


def test_an_exact_tie_goes_to_the_first_key_in_object_keys_order(an, s):
    lay = dc.file_layout("pairs")                             # two syllables in every callback: a lone syllable would add its first class only
    g = _file_case(an, s, lay, 65, 53, "tie", seed=4)
    _check_file_case(g, lay, 65)
    assert g["arms"].get("file.tie", 0) > 0
    one, two = g["labels"][1], g["labels"][2]
    assert not one.isdigit() and two.isdigit()
    f = 0                                                     # twenty callbacks: both sums grew alike
    assert g["sums"][f][1] == g["sums"][f][2] == g["sums"][f].max() > 0
    assert g["classes"][f] == g["lmap"][2]                    # the array-index key is scanned first, though class 1 was inserted first


@pytest.mark.parametrize("maker,width", [("wide", 23), ("host", 53), ("featdb", 53)])
def test_same_object_three_makers(an, s, maker, width):
    lay = dc.file_layout("straddle")
    g = _file_case(an, s, lay, 64, width, "random", maker=maker, seed=2)
    _check_file_case(g, lay, 64)
    if maker == "featdb":                                     # the same features from host rows: the same bits throughout
        h = _file_case(an, s, lay, 64, width, "random", maker="host", seed=2)
        assert h["prob"].tobytes() == g["prob"].tobytes() and h["sums"].tobytes() == g["sums"].tobytes() and h["values"].tobytes() == g["values"].tobytes()


def test_refusals_leave_the_object_usable(an, s):
    lay = dc.file_layout("straddle")
    f_col, c_col, dur, nf = lay["file_of_row"], lay["callback_of_row"], lay["durations"].copy(), lay["n_files"]
    n = len(f_col)
    dur[7] = 0.0125                                           # row 7 has a file
    V = 5
    t, p = dc.class_columns(n, V, 1)
    tv, pv = dc.ordinal_columns(n, 2, "special")
    feat = dc.features(n, 53, 1)
    model = an.load_model(dc.model_spec(53, 4, 1))
    bad = an.feature_db(feat, dur, [V, V], 1)
    with pytest.raises(capi.WsaError, match=r"the duration 0\.0125\d* of row 7 is not a whole number of milliseconds"):
        bad.set_files(f_col, c_col, nf)
    with pytest.raises(capi.WsaError, match="the DB's rows have no files yet: wsa_dbstats_set_files"):
        bad.fold_files(0, s)
    bad.close()
    dur[7] = 0.012
    db = an.feature_db(feat, dur, [V, V], 1)
    only_cat = an.feature_db(None, dur, [V], 0)
    try:
        db.set_classes(0, t, p); db.set_classes(1, t, p); db.set_values(0, tv, pv)
        with pytest.raises(capi.WsaError, match="categorical head 2 of 2"):
            db.confusion(2, s)
        with pytest.raises(capi.WsaError, match="the DB has no ordinal head"):
            only_cat.agreement(s)
        for call in (lambda: db.fold_files(0, s), lambda: db.fold_file_values(0, s), lambda: db.file_table(s), lambda: db.file_confusion(0, s),
                     lambda: db.file_agreement(s), lambda: db.file_classes(0, s), lambda: db.file_values(0, s), lambda: db.file_sums(0, 4, s)):
            with pytest.raises(capi.WsaError, match="no files yet"):
                call()
        g = f_col.copy(); g[210] = 0
        with pytest.raises(capi.WsaError, match=r"file_of_row is not non-decreasing: row 210 has file 0 after file 1 of row 209"):
            db.set_files(g, c_col, nf)
        g = f_col.copy(); g[5] = nf
        with pytest.raises(capi.WsaError, match=rf"file {nf} of row 5 is outside -1 \.\. {nf - 1}"):
            db.set_files(g, c_col, nf)
        with pytest.raises(capi.WsaError, match="at least one file"):
            db.set_files(np.full(n, -1, np.int32), c_col, 0)
        db.set_files(f_col, c_col, nf)                        # after three refusals: accepted
        with pytest.raises(capi.WsaError, match="set already"):
            db.set_files(f_col, c_col, nf)
        with pytest.raises(capi.WsaError, match="no class prediction has run on this DB yet"):
            db.fold_files(0, s)
        with pytest.raises(capi.WsaError, match="has not been folded per file yet"):
            db.file_sums(0, 4, s)
        with pytest.raises(capi.WsaError, match=r"true class 5 of file 1 is outside -1 \.\. 4"):
            db.set_file_classes(0, np.array([0, 5, 0, 0], np.int32))
        db.predict_classes(0, model, np.arange(4), s)
        with pytest.raises(capi.WsaError, match="the kept probabilities are those of categorical head 0, not of head 1"):
            db.fold_files(1, s)
        db.fold_files(0, s)
        with pytest.raises(capi.WsaError, match="folded with a model of 4 classes, not 5"):
            db.file_sums(0, 5, s)
        # the object works: everything against the restatement
        assert db.confusion(1, s).tolist() == ref.confusion(V, t, p)
        _check_agreement(db.agreement(s), [ref.agreement(tv, pv)])
        sums, classes = ref.fold_files(f_col, c_col, dur, db.probs(4, s), list(model.labels), np.arange(4), nf)
        assert ref.same_f64(db.file_sums(0, 4, s), sums) and db.file_classes(0, s).tolist() == classes.tolist()
    finally:
        model.close(); db.close(); only_cat.close()


# ---- the fold is Batch's: a small level-13 run, appended to a DeviceDB and evaluated
def test_a_files_meter_sums_are_the_batch_folds_clip_conf(s):
    from webspeechanalyzer_amd.synth import synth_clips
    fs, ns, nc = 16000, 48000, 6
    pcm = synth_clips(nc, ns, fs=fs, seed=3, device="cuda")
    a = capi.Analyzer(capi.Config(output_level=13), device=0)
    b = a.batch([ns] * nc, fs)
    b.run(pcm.data_ptr(), pcm.stride(0), s)
    files = [f"clip{c}.wav" for c in range(nc)]
    n = len(b.rows(s)["meta"])
    assert n >= 8, f"{n} rows"
    db = featdb.DeviceDB(a, 13, n)
    db.append(b, files, s)
    assert len(db.records) == n                               # every row is stored: a clip's rows are its file's rows
    spec = dc.model_spec(53, 4, 6)
    mn, mx = db.ranges(stream=s)
    spec.in_min, spec.in_max = mn, np.where(mx > mn, mx, mn + 1)
    model = a.load_model(spec)
    b.classify(model, s)
    want = b.classes(s)
    for i, r in enumerate(db.records):
        r["true"] = [{"emotion": spec.labels[i % 4]}, {"V": 1.0 + i % 5}]
        r["pred"] = [{}, {"V": 1.5 + i % 4}]
    out = dbstats.evaluate(a, db, [{"emotion": list(spec.labels)}], ["V"], models={"emotion": model}, stream=s)
    got = out["files"]
    assert got["names"] == [f for c, f in enumerate(files) if any(int(m[0]) == c for m in b.rows(s)["meta"])]
    for k, name in enumerate(got["names"]):
        c = files.index(name)
        assert got["sums"]["emotion"][k].tobytes() == want["clip_conf"][c].tobytes(), f"{name}: {got['sums']['emotion'][k]} != {want['clip_conf'][c]}"
    # the host structure: both levels, text included; the row level equals stats_table's on the records evaluate() wrote
    assert out["rows"]["table"] == dbstats.stats_table(a, db, [{"emotion": list(spec.labels)}], ["V"], stream=s)
    assert sum(sum(r) for r in out["rows"]["confusion"][0]["matrix"]) == n
    assert sum(sum(r) for r in got["confusion"][0]["matrix"]) == len(got["names"]) == got["agreement"][0]["n"]
    assert any(x.startswith("UAR: ") for x in got["lines"]) and any(x.startswith("CCC: ") for x in out["rows"]["lines"])
    assert got["classes"]["emotion"] == [spec.labels[int(np.argmax(row))] if row.max() > 0 else None for row in got["sums"]["emotion"]]
    model.close(); db.close(); b.close(); a.close()

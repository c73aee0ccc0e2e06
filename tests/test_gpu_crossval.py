"""K6f and specification CV-1 on the GPU (csrc/classify.hip, csrc/crossval.hip through capi; webspeechanalyzer_amd.crossval).

K6f against K6 alone, bit for bit: every member of a launch has hand-made weights (tests/crossval_cases.py) and its own row list; the
expectation gathers the member's rows densely on the host and runs wsa_classify_rows / wsa_regress_rows on them.  One launch holds
every stack of the issue (53-8-4: rb 4, a tile of 64 rows; 53-300-4: rb 2, 32; 53-1024-4: rb 1, 16) at every list length (0, 1,
tile - 1, tile, tile + 1, 2 tile + 1): 18 members, 566 held-out rows interleaved with 34 rows of no fold (the issue's "about 400" does
not hold all eighteen lists; none was dropped).  The same at widths 264 and 23, and through the value epilogue.  Before every
fold-wise call a whole-DB prediction fills every row, so a row of no fold that kept a stale probability or value would show.

cross_validate end to end on tests/crossval_cases.e2e_db: every fold's model and history against train.train / train_regression on
fold_data's dict, and the evaluation against one composed on the host from K whole-DB predictions (dbstats.predict_db), the per-file
class fold against tests/dbeval_ref.fold_files on the composed probability table; then the same from a DeviceDB."""
import numpy as np
import pytest

from webspeechanalyzer_amd import capi, crossval, dbstats, featdb, nnmodel, train

from . import crossval_cases as cc
from . import dbeval_ref as ref

pytestmark = pytest.mark.gpu

STACKS = {53: [([53, 8], 64), ([53, 300], 32), ([53, 1024], 16)], 264: [([264, 20], 32)], 23: [([23, 8], 64)]}
QNAN = 0x7FF8000000000000


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def an():
    a = capi.Analyzer(capi.Config(output_level=13), device=0)
    yield a
    a.close()


@pytest.fixture(scope="module")
def s(torch):
    return torch.cuda.current_stream().cuda_stream


def _members(width, regression):
    """[(spec, list length)]: one member per stack and list length, in stack order — K6f's work list has to reorder them by cost"""
    out = []
    for i, (units, tile) in enumerate(STACKS[width]):
        units = units + [1 if regression else 4]
        assert cc.tile_rows(units) == tile, units
        out += [(cc.member_spec(units, 10 * i + j, regression), n) for j, n in enumerate(cc.list_lengths(tile))]
    return out


def _k6(torch, s, model, feat, ranges=None):
    """K6 alone over dense rows: probabilities [n][C] f32, or with ranges the values [n] f64"""
    d_feat = torch.from_numpy(np.ascontiguousarray(feat, np.float64)).cuda()
    if ranges is None:
        d_out = torch.full((len(feat), model.n_classes), -1.0, dtype=torch.float32, device="cuda")
        model.classify_rows(d_feat.data_ptr(), len(feat), d_out.data_ptr(), s)
    else:
        d_out = torch.full((len(feat),), -7.0, dtype=torch.float64, device="cuda")
        model.regress_rows(d_feat.data_ptr(), len(feat), d_out.data_ptr(), ranges[0], ranges[1], s)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _want_probs(torch, s, models, fold, feat, C):
    want = np.zeros((len(fold), C), np.float32)
    for k, m in enumerate(models):
        rows = np.flatnonzero(fold == k)
        if len(rows):
            want[rows] = _k6(torch, s, m, feat[rows])
    return want


def _decided(prob):
    """DS-1's decision with the identity map: the first largest probability above 0, else blank"""
    key = np.where(prob > 0, prob, 0)
    return np.where(key.max(axis=1) > 0, key.argmax(axis=1), -1).astype(np.int32)


@pytest.mark.parametrize("width", [53, 264, 23])
def test_k6f_probabilities_are_k6s_bit_for_bit(torch, an, s, width):
    members = _members(width, False)
    K, lengths = len(members), [n for _, n in members]
    fold = cc.fold_column(lengths, 2 * K - 2, seed=width)
    n = len(fold)
    assert [int((fold == k).sum()) for k in range(K)] == lengths and int((fold < 0).sum()) == 2 * K - 2
    feat = cc.dense_rows(n, width, width + 1)
    models = [an.load_model(spec) for spec, _ in members]
    db = an.feature_db(feat, np.full(n, 0.25), [4], 0)
    try:
        db.set_classes(0, np.zeros(n, np.int32))
        db.set_folds(fold, K)
        db.predict_classes(0, models[-1], np.arange(4), s)            # every row gets a probability, the rows of no fold too
        assert (db.probs(4, s)[fold < 0] > 0).all()
        db.predict_classes_folds(0, models, np.arange(4), s)
        got, idx = db.probs(4, s), db.pred_classes(0, s)
        want = _want_probs(torch, s, models, fold, feat, 4)
        held = fold >= 0
        assert np.ptp(want[held], axis=0).min() > 0.05                 # the rows differ
        assert got[held].tobytes() == want[held].tobytes()
        assert not got[~held].any() and (idx[~held] == -1).all()       # zero, not stale; decided blank
        assert idx.tolist() == _decided(want).tolist() and (idx[held] >= 0).all()
        assert got.tobytes() == want.tobytes()
        # the other table of the launch: the plan the host can compute
        assert capi.crossval_tiles(lengths, [cc.tile_rows(spec.units) // 16 for spec, _ in members]) == sum(-(-c // cc.tile_rows(spec.units)) for spec, c in members)
    finally:
        db.close()
        for m in models:
            m.close()


@pytest.mark.parametrize("width", [53, 264, 23])
def test_k6f_values_are_k6s_bit_for_bit(torch, an, s, width):
    members = _members(width, True)
    K, lengths = len(members), [n for _, n in members]
    fold = cc.fold_column(lengths, 2 * K - 2, seed=width + 7)
    n = len(fold)
    feat = cc.dense_rows(n, width, width + 8)
    models = [an.load_model(spec) for spec, _ in members]
    # a member's own range (its spec's: all differ), and for every other member one given at the call
    ranges = [None if k % 2 else (-1.0 - k, 2.5 + 0.5 * k) for k in range(K)]
    used = [r if r is not None else (spec.out_min, spec.out_max) for r, (spec, _) in zip(ranges, members)]
    assert len(set(used)) == K
    db = an.feature_db(feat, np.full(n, 0.25), [], 1)
    try:
        db.set_values(0, np.ones(n))
        db.set_folds(fold, K)
        db.predict_values(0, models[-1], None, None, s)                # every row gets a value
        assert np.isfinite(db.pred_values(0, s)).all()
        db.predict_values_folds(0, models, ranges, s)
        got = db.pred_values(0, s)
        want = np.full(n, np.nan)
        for k, m in enumerate(models):
            rows = np.flatnonzero(fold == k)
            if len(rows):
                want[rows] = _k6(torch, s, m, feat[rows], used[k])
        held = fold >= 0
        assert np.ptp(want[held]) > 0.5 and np.isfinite(want[held]).all()
        assert got[held].tobytes() == want[held].tobytes()
        assert (got[~held].view(np.uint64) == QNAN).all()              # NaN, not stale
    finally:
        db.close()
        for m in models:
            m.close()


def test_a_second_call_with_swapped_models_overwrites_cleanly(torch, an, s):
    """The folds are set once, so what changes between two calls is who predicts a list.  Every row of a list is rewritten by the list's
    new model, a list that is empty (fold 0) stays without a row whichever model it gets, and the rows of no fold stay zero / NaN."""
    members = _members(23, False)
    K, lengths = len(members), [n for _, n in members]
    fold = cc.fold_column(lengths, 9, seed=2)
    feat = cc.dense_rows(len(fold), 23, 3)
    models = [an.load_model(spec) for spec, _ in members]
    db = an.feature_db(feat, np.full(len(fold), 0.25), [4], 0)
    try:
        db.set_classes(0, np.zeros(len(fold), np.int32))
        db.set_folds(fold, K)
        db.predict_classes_folds(0, models, np.arange(4), s)
        first = db.probs(4, s)
        db.predict_classes_folds(0, models[::-1], np.arange(4), s)
        second = db.probs(4, s)
        assert first.tobytes() == _want_probs(torch, s, models, fold, feat, 4).tobytes()
        assert second.tobytes() == _want_probs(torch, s, models[::-1], fold, feat, 4).tobytes()
        held = fold >= 0
        assert (first[held] != second[held]).any(axis=1).all() and not second[~held].any()
        db.predict_classes_folds(0, models, np.arange(4), s)           # back again, enqueued twice without a wait between
        db.predict_classes_folds(0, models, np.arange(4), s)
        assert db.probs(4, s).tobytes() == first.tobytes()
    finally:
        db.close()
        for m in models:
            m.close()


def test_refusals_leave_the_object_usable(torch, an, s):
    n = 40
    feat = cc.dense_rows(n, 53, 1)
    fold = np.array([k % 3 - 1 for k in range(n)], np.int32)             # -1, 0, 1, ..
    a, b = an.load_model(cc.member_spec([53, 8, 4], 1)), an.load_model(cc.member_spec([53, 8, 4], 2))
    three = an.load_model(cc.member_spec([53, 8, 3], 3))
    narrow = an.load_model(cc.member_spec([23, 8, 4], 4))
    keyed = an.load_model(cc.member_spec([53, 8, 4], 5, labels=["c0", "7", "c2", "c3"]))
    reg, reg2 = an.load_model(cc.member_spec([53, 8, 1], 6, True)), an.load_model(cc.member_spec([53, 8, 1], 7, True))
    # neither a classifier nor a regression model: two linear units
    two = an.load_model(nnmodel.ModelSpec([53, 2], ["linear"], [np.zeros((53, 2), np.float32)], [np.zeros(2, np.float32)], np.zeros(53), np.ones(53), [], 0.0, 1.0))
    other = capi.Analyzer(capi.Config(output_level=13), device=0)
    foreign = other.load_model(cc.member_spec([53, 8, 4], 1))
    db = an.feature_db(feat, np.full(n, 0.25), [4], 1)
    counted = an.feature_db(None, np.full(n, 0.25), [4], 1)
    ident = np.arange(4)
    try:
        with pytest.raises(capi.WsaError, match="the DB's rows have no folds yet: wsa_dbstats_set_folds"):
            db.predict_classes_folds(0, [a, b], ident, s)
        with pytest.raises(capi.WsaError, match="the DB's rows have no folds yet: wsa_dbstats_set_folds"):
            db.predict_values_folds(0, [reg, reg2], None, s)
        for k in (0, 1, 33):
            with pytest.raises(capi.WsaError, match=rf"a cross-validation has 2 \.\. 32 folds, got {k}$"):
                db.set_folds(fold, k)
        bad = fold.copy(); bad[5] = 2
        with pytest.raises(capi.WsaError, match=r"fold 2 of row 5 is outside -1 \.\. 1$"):
            db.set_folds(bad, 2)
        bad[5], bad[4] = 0, -2
        with pytest.raises(capi.WsaError, match=r"fold -2 of row 4 is outside -1 \.\. 1$"):
            db.set_folds(bad, 2)
        with pytest.raises(capi.WsaError, match="the DB was created without feature rows"):
            counted.set_folds(fold, 2)
        db.set_folds(fold, 2)                                             # after the refusals: accepted
        with pytest.raises(capi.WsaError, match="the DB's folds are set already; they are set once"):
            db.set_folds(fold, 2)
        with pytest.raises(capi.WsaError, match="categorical head 1 of 1"):
            db.predict_classes_folds(1, [a, b], ident, s)
        with pytest.raises(capi.WsaError, match="ordinal head 1 of 1"):
            db.predict_values_folds(1, [reg, reg2], None, s)
        with pytest.raises(capi.WsaError, match="3 models for 2 folds: one model per fold"):
            db.predict_classes_folds(0, [a, b, a], ident, s)
        with pytest.raises(capi.WsaError, match="1 models for 2 folds: one model per fold"):
            db.predict_values_folds(0, [reg], None, s)
        with pytest.raises(capi.WsaError, match="member 1 is NULL"):
            db.predict_classes_folds(0, [a, None], ident, s)
        ident32 = ident.astype(np.int32)
        assert an.L.wsa_dbstats_predict_classes_folds(db.h, 0, None, 2, ident32.ctypes.data, s) != 0
        assert "null member array" in an.L.wsa_last_error(an.h).decode()
        with pytest.raises(capi.WsaError, match="member 1 belongs to another context"):
            db.predict_classes_folds(0, [a, foreign], ident, s)
        with pytest.raises(capi.WsaError, match=r"member 1 is a regression model \(one unit, no softmax\)"):
            db.predict_classes_folds(0, [a, reg], ident, s)
        with pytest.raises(capi.WsaError, match="member 0 takes 23 inputs; the DB's rows have 53 features"):
            db.predict_classes_folds(0, [narrow, a], ident, s)
        with pytest.raises(capi.WsaError, match="member 1 has 3 classes, member 0 has 4"):
            db.predict_classes_folds(0, [a, three], ident, s)
        with pytest.raises(capi.WsaError, match="member 1's legend has other key ranks than member 0's"):
            db.predict_classes_folds(0, [a, keyed], ident, s)
        with pytest.raises(capi.WsaError, match=r"legend_to_vocab\[3\] = 9 is outside -1 \.\. 3"):
            db.predict_classes_folds(0, [a, b], [0, 1, 2, 9], s)
        with pytest.raises(capi.WsaError, match="member 1: a regression model's last layer is linear, relu, sigmoid or tanh, not softmax"):
            db.predict_values_folds(0, [reg, a], [None, (0.0, 1.0)], s)
        with pytest.raises(capi.WsaError, match="member 0: a regression model has one output unit"):
            db.predict_values_folds(0, [two, reg], [(0.0, 1.0), None], s)
        with pytest.raises(capi.WsaError, match="member 1: the output has max == min"):
            db.predict_values_folds(0, [reg, reg2], [None, (2.0, 2.0)], s)
        with pytest.raises(capi.WsaError, match="member 0: non-finite out_min / out_max"):
            db.predict_values_folds(0, [reg, reg2], [(0.0, float("inf")), None], s)
        with pytest.raises(capi.WsaError, match="member 1 takes 23 inputs"):
            db.predict_values_folds(0, [reg, narrow], [None, (0.0, 1.0)], s)
        with pytest.raises(capi.WsaError, match="no class prediction has run on this DB yet"):
            db.probs(4, s)                                                # no refusal left anything behind
        # the object works
        db.set_classes(0, np.zeros(n, np.int32)); db.set_values(0, np.ones(n))
        db.predict_classes_folds(0, [a, b], ident, s)
        db.predict_values_folds(0, [reg, reg2], None, s)
        assert db.probs(4, s).tobytes() == _want_probs(torch, s, [a, b], fold, feat, 4).tobytes()
        v = db.pred_values(0, s)
        for k, m in enumerate((reg, reg2)):
            rows = np.flatnonzero(fold == k)
            assert v[rows].tobytes() == _k6(torch, s, m, feat[rows], (m.spec.out_min, m.spec.out_max)).tobytes()
        assert np.isnan(v[fold < 0]).all()
    finally:
        db.close(); counted.close()
        for m in (a, b, three, narrow, keyed, reg, reg2, two, foreign):
            m.close()
        other.close()


# ---- cross_validate end to end
E2E = dict(epochs=2, batch_size=32, seed=11)
HEADS = (cc.E2E_CLASS_LABELS, cc.E2E_ORDINALS)


def _same(a, b):
    """== over plain data, with NaN equal to NaN (a precision of a class that is never predicted is 0 / 0) and arrays by their bytes"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.tobytes() == np.asarray(b).tobytes()
    if isinstance(a, float) and a != a:
        return isinstance(b, float) and b != b
    return a == b


def _same_spec(a, b):
    assert a.units == b.units and a.activations == b.activations and list(a.labels) == list(b.labels)
    assert np.asarray(a.in_min).tobytes() == np.asarray(b.in_min).tobytes() and np.asarray(a.in_max).tobytes() == np.asarray(b.in_max).tobytes()
    assert (getattr(a, "out_min", None), getattr(a, "out_max", None)) == (getattr(b, "out_min", None), getattr(b, "out_max", None))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.kernels + a.biases, b.kernels + b.biases))


@pytest.fixture(scope="module")
def e2e(an, s):
    rows = cc.e2e_db()
    work = cc.clone(rows)
    out = crossval.cross_validate(an, work, *HEADS, ["emotion", "V"], 3, keep_models=True, stream=s, **E2E)
    return dict(rows=rows, work=work, out=out)


def test_cross_validate_folds_and_models(an, s, e2e):
    rows, out = e2e["rows"], e2e["out"]
    fold_of_row, fof, names = crossval.assign_folds(rows, 3)
    assert len(rows) == 92 and len(names) == 9 and fof == [0, 1, 2] * 3
    assert out["fold_of_row"].tolist() == fold_of_row.tolist() and out["fold_of_file"] == fof and int((fold_of_row < 0).sum()) == 2
    feat = np.array([r["features"] for r in rows], np.float64)
    classes = cc.E2E_CLASS_LABELS[0]["emotion"]
    cdata = crossval.fold_data(feat, crossval.head_labels(rows, "emotion", classes), classes, fold_of_row, 3)
    vdata = crossval.fold_data(feat, crossval.head_values(rows, "V"), None, fold_of_row, 3)
    for f in range(3):
        info = out["folds"][f]
        assert info["files"] == [n for n, g in zip(names, fof) if g == f] and info["held_out"] == 30
        assert info["heads"]["emotion"]["train_rows"] == len(cdata[f]["rows"]) and info["heads"]["emotion"]["counts"] == list(cdata[f]["counts"])
        assert not (fold_of_row[np.array(cdata[f]["rows"])] == f).any() and not (fold_of_row[np.array(vdata[f]["rows"])] == f).any()
        spec, hist = train.train(an, cdata[f], seed=E2E["seed"] + 2 * f, epochs=2, batch_size=32, stream=s)
        _same_spec(out["models"]["emotion"][f], spec)
        assert info["heads"]["emotion"]["history"] == hist and len(hist) == 1 and hist[0]["epochs_done"] == 2
        rspec, rhist = train.train_regression(an, vdata[f], seed=E2E["seed"] + 2 * f, epochs=2, batch_size=32, stream=s)
        _same_spec(out["models"]["V"][f], rspec)
        assert info["heads"]["V"]["history"] == rhist
        assert out["models"]["emotion"][f].labels == out["models"]["emotion"][0].labels == cdata[0]["legend"]


def test_cross_validate_is_the_evaluation_of_composed_predictions(an, s, e2e):
    rows, work, out = e2e["rows"], e2e["work"], e2e["out"]
    cats, ords = dbstats.head_settings(*HEADS)
    fold = out["fold_of_row"]
    n, legend = len(rows), list(out["models"]["emotion"][0].labels)
    comp, probs = cc.clone(rows), np.zeros((n, len(legend)), np.float32)
    for i in np.flatnonzero(fold < 0):
        dbstats.update_pred_label(comp[i], cats, ords, "emotion", None)
        dbstats.update_pred_label(comp[i], cats, ords, "V", float("nan"))
    for f in range(3):                                                    # K predictions over the whole DB, merged on the host
        labels, raw = dbstats.predict_db(an, cc.clone(rows), HEADS, "cats", "emotion", out["models"]["emotion"][f], stream=s, return_raw=True)
        values = dbstats.predict_db(an, cc.clone(rows), HEADS, "ords", "V", out["models"]["V"][f], stream=s)
        for i in np.flatnonzero(fold == f):
            dbstats.update_pred_label(comp[i], cats, ords, "emotion", labels[i])
            dbstats.update_pred_label(comp[i], cats, ords, "V", values[i])
            probs[i] = raw[i]
    assert [r["pred"] for r in work] == [r["pred"] for r in comp]         # the held-out predictions were written into the records
    assert all(r["pred"] == [{"emotion": None}, {"V": None}] for r, k in zip(work, fold) if k < 0)
    assert len({r["pred"][0]["emotion"] for r in work} - {None}) >= 2     # two epochs already tell classes apart
    want = dbstats.evaluate(an, comp, *HEADS, stream=s)
    assert _same(out["rows"], want["rows"])
    assert sum(sum(r) for r in out["rows"]["confusion"][0]["matrix"]) == n and sum(r[-1] for r in out["rows"]["confusion"][0]["matrix"]) == 2
    assert out["rows"]["agreement"][0]["n"] == n - 2
    # per file: the ordinal head folds the predicted column, so the composed evaluation gives it too; the class fold needs the
    # probabilities, which the composed evaluation has not: the restatement folds the composed table
    gf, wf = out["files"], want["files"]
    assert gf["names"] == wf["names"] and gf["folded"] == {"emotion": True} and wf["folded"] == {"emotion": False}
    assert ref.same_f64(gf["values"]["V"], wf["values"]["V"]) and _same(gf["agreement"], wf["agreement"]) and _same(gf["table"]["ords"], wf["table"]["ords"])
    col = dbstats.build_columns(rows, *HEADS, {"emotion": legend})
    f_col, c_col, names = dbstats.file_columns(rows)
    lmap = [col["cats"][0]["vocab"].index(x) for x in legend]
    sums, classes = ref.fold_files(f_col, c_col, col["durations"], probs, legend, lmap, len(names))
    assert ref.same_f64(gf["sums"]["emotion"], sums)
    vocab = col["cats"][0]["vocab"]
    assert gf["classes"]["emotion"] == [vocab[i] if i >= 0 else None for i in classes]
    truth = dbstats.file_truths(col, f_col, len(names))[0][0]
    assert gf["confusion"][0]["matrix"] == ref.confusion(len(vocab), truth, classes)
    assert gf["table"]["cats"][0]["correct"] == sum(int(t == p) for t, p in zip(truth, classes)) and gf["table"]["cats"][0]["blank"] == 0


def test_cross_validate_from_a_device_db(an, s, e2e):
    rows, out = e2e["rows"], e2e["out"]
    ddb = featdb.DeviceDB(an, 13, len(rows))
    try:
        ddb.append_rows(cc.clone(rows), s)
        got = crossval.cross_validate(an, ddb, *HEADS, ["emotion", "V"], 3, keep_models=True, stream=s, **E2E)
        assert ddb.count == len(rows)
        for name in ("emotion", "V"):
            for a, b in zip(got["models"][name], out["models"][name]):
                _same_spec(a, b)
        assert _same(got["rows"], out["rows"]) and _same(got["folds"], out["folds"])
        assert [r["pred"] for r in ddb.records] == [r["pred"] for r in e2e["work"]]
        gf, wf = got["files"], out["files"]
        assert gf["sums"]["emotion"].tobytes() == wf["sums"]["emotion"].tobytes() and ref.same_f64(gf["values"]["V"], wf["values"]["V"])
        for key in ("names", "classes", "folded", "table", "confusion", "agreement", "lines"):
            assert _same(gf[key], wf[key]), key
    finally:
        ddb.close()


def test_host_refusals_name_the_head_and_the_fold(an, s):
    rows = cc.e2e_db()
    with pytest.raises(ValueError, match="heads names 'mood'; the settings have \\['emotion', 'V'\\]"):
        crossval.cross_validate(an, rows, *HEADS, ["mood"], 3)
    few = cc.clone(rows)
    for r in few[12:]:
        r["true"] = None
    with pytest.raises(ValueError, match=r"^fold 0: Sample size 2/92 too small for training$"):
        crossval.cross_validate(an, few, *HEADS, ["emotion"], 3, stream=s, **E2E)

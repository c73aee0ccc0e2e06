"""The host half of specification CV-1 without a GPU: the new entries are exported and declared once (include/wsa_crossval.h ==
capi.CROSSVAL_TABLE, by the parser tests/test_dbeval_host.py holds include/wsa_eval.h with), the folds derived from records, the
leakage checks on fold_data's dicts, and wsa_crossval_tiles against its restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

from webspeechanalyzer_amd import capi, crossval, train

from . import crossval_cases as cc
from .test_dbeval_host import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wsa_dbstats_set_folds", "wsa_dbstats_predict_classes_folds", "wsa_dbstats_predict_values_folds", "wsa_crossval_tiles"]


def test_new_symbols_are_exported_and_declared_once():
    L = capi.lib()
    assert L.wsa_abi_version() == capi.ABI_VERSION == 5
    assert capi.CROSSVAL_SYMBOLS == NEW == list(capi.CROSSVAL_TABLE)
    for name in NEW:
        assert hasattr(L, name), f"{name} is not exported by libwsa.so"
        assert name not in capi.ABI_TABLE and name not in capi.EVAL_TABLE
    path = os.path.join(ROOT, "include", "wsa_crossval.h")
    protos = _prototypes(path)
    assert sorted(protos) == sorted(capi.CROSSVAL_TABLE)
    scalar = {"uint32_t": ctypes.c_uint32}
    for name, (res, params) in protos.items():
        restype, argtypes = capi.CROSSVAL_TABLE[name]
        assert res == "wsa_status" and restype is ctypes.c_int and len(argtypes) == len(params), name
        for p, t in zip(params, argtypes):
            assert (t is ctypes.c_void_p) if "*" in p else (t is scalar[p.split()[0]]), (name, p, t)
    code = open(path).read()
    assert re.search(r"#define\s+WSA_CROSSVAL_MAX_FOLDS\s+32\b", code) and re.search(r"#if\s+WSA_CROSSVAL_MAX_FOLDS\s*!=\s*WSA_TRAIN_GROUP_MAX", code)
    assert capi.CROSSVAL_MAX_FOLDS == crossval.MAX_FOLDS == capi.TRAIN_GROUP_MAX == 32


def _rows(files):
    return [dict(file=f, seg=str(i), time=["0.000", "0.250"], true=None, pred=None) for i, f in enumerate(files)]


def test_assign_folds():
    files = ["anna_1", "anna_1", "bob_1", None, "anna_2", "cara_1", "cara_1", "", "bob_2", "dan_1"]
    rows = _rows(files)
    # the default: a file is its own group, files in order of first appearance, file g in fold g mod k
    rf, ff, names = crossval.assign_folds(rows, 3)
    assert names == ["anna_1", "bob_1", "anna_2", "cara_1", "bob_2", "dan_1"] and ff == [0, 1, 2, 0, 1, 2]
    assert rf.dtype == np.int32 and rf.tolist() == [0, 0, 1, -1, 2, 0, 0, -1, 1, 2]      # a row without a file: -1
    # by speaker: groups in order of first appearance (anna, bob, cara, dan), group g in fold g mod k; a speaker's files stay together
    speaker = lambda name: name.split("_")[0]      # noqa: E731
    rf, ff, _ = crossval.assign_folds(rows, 2, group_of=speaker)
    assert ff == [0, 1, 0, 0, 1, 1] and rf.tolist() == [0, 0, 1, -1, 0, 0, 0, -1, 1, 1]
    # k = the number of groups: leave one group out
    rf, ff, _ = crossval.assign_folds(rows, 4, group_of=speaker)
    assert ff == [0, 1, 0, 2, 1, 3] and sorted(set(ff)) == [0, 1, 2, 3]
    # an explicit list overrides both rules
    rf, ff, _ = crossval.assign_folds(rows, 2, group_of=speaker, fold_of_file=[1, 1, 0, 0, 1, 0])
    assert ff == [1, 1, 0, 0, 1, 0] and rf.tolist() == [1, 1, 1, -1, 0, 0, 0, -1, 1, 0]
    for k in (1, 33, 0):
        with pytest.raises(ValueError, match=rf"a cross-validation has 2 \.\. 32 folds, got {k}"):
            crossval.assign_folds(rows, k)
    with pytest.raises(ValueError, match=r"5 folds for 4 groups \(6 files\)"):
        crossval.assign_folds(rows, 5, group_of=speaker)
    with pytest.raises(ValueError, match="7 folds for 6 groups"):
        crossval.assign_folds(rows, 7)
    with pytest.raises(ValueError, match="fold_of_file has 2 entries, the DB has 6 files"):
        crossval.assign_folds(rows, 2, fold_of_file=[0, 1])
    with pytest.raises(ValueError, match=r"fold_of_file\[2\] = 2 \('anna_2'\) is outside 0 \.\. 1"):
        crossval.assign_folds(rows, 2, fold_of_file=[0, 1, 2, 0, 1, 0])


@pytest.fixture(scope="module")
def leak():
    rows, labels = cc.leak_db()
    fold_of_row, fof, names = crossval.assign_folds(rows, 3)
    feat = np.array([r["features"] for r in rows], np.float64)
    return dict(rows=rows, labels=labels, fold_of_row=fold_of_row, feat=feat,
                data=crossval.fold_data(feat, labels, cc.LEAK_CLASSES, fold_of_row, 3))


def test_no_selected_row_is_held_out(leak):
    assert leak["fold_of_row"].tolist() == [f % 3 for f in range(6) for _ in range(10)]
    for f, d in enumerate(leak["data"]):
        rows = np.array(d["rows"])
        assert not (leak["fold_of_row"][rows] == f).any(), f                 # duplicates included
        assert len(rows) > len(set(rows.tolist()))                           # the top-up loop ran
        assert d["features"].tobytes() == leak["feat"][rows].tobytes()       # rows are DB indices
        # the fold's own selection: train.select with the fold's labels blanked, re-indexed against the common legend
        own = train.select([None if leak["fold_of_row"][i] == f else v for i, v in enumerate(leak["labels"])], cc.LEAK_CLASSES)
        assert own["rows"] == d["rows"] and [own["legend"][j] for j in own["y"]] == [d["legend"][j] for j in d["y"]]
    counts = [d["counts"] for d in leak["data"]]
    assert counts == [[22, 22, 22], [26, 26, 0], [20, 20, 20]]               # N, A, S: every class above 3 rows is topped up to the largest


def test_ranges_come_from_training_rows_only(leak):
    assert leak["fold_of_row"][37] == 0 and leak["feat"][37, 5] == cc.EXTREME
    for f, d in enumerate(leak["data"]):
        x = leak["feat"][d["rows"]]
        assert d["in_min"].tobytes() == x.min(axis=0).tobytes() and d["in_max"].tobytes() == x.max(axis=0).tobytes()
        assert (d["in_max"][5] == cc.EXTREME) == (f != 0)
    assert leak["data"][0]["in_max"].max() <= 1.0


def test_one_legend_for_all_folds(leak):
    common = train.select(leak["labels"], cc.LEAK_CLASSES)["legend"]
    assert common == ["N", "A", "S"]
    for d in leak["data"]:
        assert d["legend"] == common
    y1 = leak["data"][1]["y"]
    assert leak["data"][1]["counts"][2] == 0 and set(y1.tolist()) == {0, 1}  # fold 1 trains without an S row and keeps S's output unit
    assert y1.dtype == np.int32
    # a fold whose own legend would start with another class: hold out the file that holds the DB's first rows
    labels = ["A"] * 10 + ["N"] * 20
    fold = np.array([0] * 10 + [1] * 10 + [-1] * 10, np.int32)
    d = crossval.fold_data(np.zeros((30, 53)), labels, ["N", "A"], fold, 2)
    assert d[0]["legend"] == d[1]["legend"] == ["A", "N"] and set(d[0]["y"].tolist()) == {1} and sorted(set(d[1]["y"].tolist())) == [0, 1]


def test_too_small_names_the_fold():
    labels = ["N"] * 10 + ["A"] * 5 + ["N"] * 4 + [None] * 6
    fold = np.array([0] * 10 + [1] * 5 + [2] * 4 + [-1] * 6, np.int32)
    with pytest.raises(ValueError, match=r"^fold 0: Sample size 9/25 too small for training$"):
        crossval.fold_data(np.zeros((25, 53)), labels, ["N", "A"], fold, 3)
    values = [0.5] * 12 + [None] * 13
    with pytest.raises(ValueError, match=r"^fold 1: Sample size 7/25 too small for training$"):
        crossval.fold_data(np.zeros((25, 53)), values, None, np.array([0] * 2 + [1] * 5 + [2] * 5 + [-1] * 13, np.int32), 3)


def test_ordinal_folds_take_their_range_from_training_values():
    rows, _ = cc.leak_db()
    fold_of_row, _, _ = crossval.assign_folds(rows, 3)
    values = crossval.head_values(rows, "V")
    values[37] = 0.999                                    # the largest value, held out in fold 0
    values[3] = None
    feat = np.array([r["features"] for r in rows], np.float64)
    data = crossval.fold_data(feat, values, None, fold_of_row, 3)
    for f, d in enumerate(data):
        rows_f = np.array(d["rows"])
        assert not (fold_of_row[rows_f] == f).any() and 3 not in d["rows"]
        assert d["out_max"] == max(values[i] for i in d["rows"]) and d["out_min"] == min(values[i] for i in d["rows"])
        assert (d["out_max"] == 0.999) == (f != 0)
        want = train.prepare_ordinal(feat, [None if fold_of_row[i] == f else v for i, v in enumerate(values)])
        assert want["rows"] == d["rows"] and want["in_max"].tobytes() == d["in_max"].tobytes() and want["values"].tobytes() == d["values"].tobytes()


def test_head_labels_and_values():
    rows = [dict(true=[{"emotion": "N"}, {"V": "0.5"}]), dict(true=[{"emotion": "X"}, {"V": None}]), dict(true=None), dict(true=[{"emotion": 3}, {"V": 2}]),
            dict(true=[{}, {"V": "abc"}])]
    assert crossval.head_labels(rows, "emotion", ["N", 3]) == ["N", None, None, "3", None]
    assert crossval.head_values(rows, "V") == [0.5, None, None, 2.0, None]


def test_tiles_against_the_restatement():
    rng = np.random.default_rng(3)
    for n in range(1, 33):
        rows = rng.choice(cc.COUNT_ROWS, n)
        rb = rng.choice([1, 2, 4], n)
        assert capi.crossval_tiles(rows, rb) == cc.tiles(rows, rb), (rows, rb)
    for r in cc.COUNT_ROWS:                               # every count at every factor on its own, and all of them mixed in one launch
        for b in (1, 2, 4):
            assert capi.crossval_tiles([r], [b]) == (r + 16 * b - 1) // (16 * b)
    rows = list(cc.COUNT_ROWS) * 3
    rb = [1] * 8 + [2] * 8 + [4] * 8
    assert capi.crossval_tiles(rows, rb) == cc.tiles(rows, rb) == 18 + 11 + 8
    assert capi.crossval_tiles([0, 0], [4, 1]) == 0       # nothing to launch
    assert capi.crossval_tiles([0xffffffff], [1]) == 1 << 28
    for rows, rb in (([1] * 33, [1] * 33), ([], []), ([5], [3]), ([5], [0])):
        with pytest.raises(capi.WsaError, match="wsa_crossval_tiles refused"):
            capi.crossval_tiles(rows, rb)
    L, out, one = capi.lib(), ctypes.c_uint64(), np.ones(1, np.uint32)
    assert L.wsa_crossval_tiles(None, one.ctypes.data, 1, ctypes.byref(out)) != 0
    assert L.wsa_crossval_tiles(one.ctypes.data, one.ctypes.data, 1, None) != 0

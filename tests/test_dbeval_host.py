"""The host half of specification EV-1 without a GPU: the new entries are exported and declared once (include/wsa_eval.h ==
capi.EVAL_TABLE, as tests/test_abi.py holds include/wsa.h to capi.ABI_TABLE), the file / callback columns derived from records, a
file's label, the metrics and the text lines, and the refusals the host makes itself."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from webspeechanalyzer_amd import capi, dbstats

from . import dbeval_cases as dc
from . import dbeval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wsa_dbstats_confusion", "wsa_dbstats_agreement", "wsa_dbstats_set_files", "wsa_dbstats_set_file_classes", "wsa_dbstats_set_file_values",
       "wsa_dbstats_fold_files", "wsa_dbstats_fold_file_values", "wsa_dbstats_file_table", "wsa_dbstats_file_confusion", "wsa_dbstats_file_agreement",
       "wsa_dbstats_copy_file_sums", "wsa_dbstats_copy_file_classes", "wsa_dbstats_copy_file_values"]


def _prototypes(path):
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M).replace('extern "C" {', " ")
    while True:
        text, n = re.subn(r"\{[^{}]*\}", " ", text)
        if not n:
            break
    protos = {}
    for stmt in text.split(";"):
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(wsa_\w+)\s*\(([^()]*)\)\s*", stmt)
        if m and m.group(1).split()[0] != "typedef":
            protos[m.group(2)] = (" ".join(m.group(1).split()), [" ".join(p.split()) for p in m.group(3).split(",")])
    return protos


def test_new_symbols_are_exported_and_declared_once():
    L = capi.lib()
    assert L.wsa_abi_version() == capi.ABI_VERSION == 5
    assert capi.EVAL_SYMBOLS == NEW == list(capi.EVAL_TABLE)
    for name in NEW:
        assert hasattr(L, name), f"{name} is not exported by libwsa.so"
        assert name not in capi.ABI_TABLE
    protos = _prototypes(os.path.join(ROOT, "include", "wsa_eval.h"))
    assert sorted(protos) == sorted(capi.EVAL_TABLE)
    scalar = {"uint32_t": ctypes.c_uint32}
    for name, (res, params) in protos.items():
        restype, argtypes = capi.EVAL_TABLE[name]
        assert res == "wsa_status" and restype is ctypes.c_int and len(argtypes) == len(params), name
        for p, t in zip(params, argtypes):
            assert (t is ctypes.c_void_p) if "*" in p else (t is scalar[p.split()[0]]), (name, p, t)
    assert ctypes.sizeof(ctypes.c_uint64) + 7 * ctypes.sizeof(ctypes.c_double) == capi._DB_AGREE.itemsize == 64


def _rows():
    rows = []
    for f, segs in (("a.wav", ["0", "0.01", "1", "2", "2.01", "2.02"]), (None, ["0"]), ("b.wav", ["3", "3.01"]), ("c.wav", ["0"])):
        for s in segs:
            rows.append(dict(file=f, seg=s, time=["0.000", "0.250"], true=None, pred=None))
    return rows


def test_file_and_callback_columns_from_records():
    rows = _rows()
    f, c, names = dbstats.file_columns(rows)
    assert names == ["a.wav", "b.wav", "c.wav"]
    assert f.tolist() == [0] * 6 + [-1] + [1, 1, 2] and c.tolist() == [0, 0, 1, 2, 2, 2, 0, 3, 3, 0]
    assert f.dtype == c.dtype == np.int32
    assert ref.check_files(f, [0.25] * len(f), 3) is None
    rows.append(dict(file="a.wav", seg="9", time=["0", "0.1"]))              # a file whose rows are not together: the library refuses the column
    f, _, _ = dbstats.file_columns(rows)
    assert ref.check_files(f, [0.25] * len(f), 3) == ("decreasing", 10)
    # a level-5 tag, a tag that is no number
    assert dbstats.file_columns([dict(file="x", seg="17"), dict(file="x", seg="seventeen")])[1].tolist() == [17, 0]


def test_a_files_label_is_that_of_its_first_counted_row():
    rows = _rows()
    labels = [None, "low", "high", "high", None, None, "low", None, None, "high"]
    values = [0, None, 2.5, 3.5, None, None, 9.0, math.nan, 4.0, None]
    for r, lab, v in zip(rows, labels, values):
        r["true"] = [{"emotion": lab}, {"V": v}]
    col = dbstats.build_columns(rows, [{"emotion": ["low", "high"]}], ["V"])
    f, _, names = dbstats.file_columns(rows)
    cats, ords = dbstats.file_truths(col, f, len(names))
    vocab = col["cats"][0]["vocab"]
    assert [vocab[i] if i >= 0 else None for i in cats[0]] == ["low", None, "high"]          # the row without a file is nobody's
    assert ords[0][0] == 2.5 and ords[0][1] == 4.0 and ords[0][2] != ords[0][2]              # a 0 does not count (DS-1), nor NaN


def test_metrics_and_lines():
    m = [[2, 1, 0, 1], [0, 0, 0, 0], [1, 0, 3, 0]]
    got = dbstats.confusion_metrics(m)
    assert got["recall"][0] == 0.5 and got["recall"][2] == 0.75 and got["recall"][1] != got["recall"][1]
    assert got["precision"] == [2 / 3, 0.0, 1.0] and got["uar"] == 0.625                      # the class without a counted row is left out of UAR
    conf = dbstats.assemble_confusion(dict(cats=[dict(name="emotion", vocab=["a", "b", "c"])]), [np.array(m, np.uint64)])
    assert dbstats.confusion_lines(conf) == [
        "Label: emotion, Type: Class, Confusion", "True \\ Predicted: a,b,c,NaN", "a : 2 1 0 1 recall: 50.00%", "b : 0 0 0 0 recall: NaN%",
        "c : 1 0 3 0 recall: 75.00%", "Precision: a 66.67%, b 0.00%, c 100.00%", "UAR: 62.50%"]
    # a class that neither occurs nor is predicted is left out of the text; an empty matrix prints NaN as the panel does for 0 / 0
    conf = dbstats.assemble_confusion(dict(cats=[dict(name="h", vocab=["a", "b"])]), [[[0, 0, 0], [0, 0, 0]]])
    assert dbstats.confusion_lines(conf) == ["Label: h, Type: Class, Confusion", "True \\ Predicted: NaN", "Precision:", "UAR: NaN%"]
    a = ref.agreement(*dc.ordinal_columns(40, 51, "special"))
    rec = np.zeros(1, capi._DB_AGREE)
    for k in ("n",) + ref.KEYS:
        rec[k][0] = a[k]
    agree = dbstats.assemble_agreement(dict(ords=[dict(name="V")]), rec)
    assert agree[0]["n"] == a["n"] and agree[0]["ccc"] == a["ccc"]
    lines = dbstats.agreement_lines(agree)
    assert lines[0] == "Label: V, Type: Ordinal, Agreement" and lines[1] == f"Pairs: {a['n']}"
    assert lines[4] == "CCC: " + dbstats.to_fixed(a["ccc"], 3) and lines[5] == "Pearson: " + dbstats.to_fixed(a["pearson"], 3)
    rec["ccc"][0] = math.nan
    assert dbstats.agreement_lines(dbstats.assemble_agreement(dict(ords=[dict(name="V")]), rec))[4] == "CCC: NaN"


def test_host_refusals():
    with pytest.raises(ValueError, match="models names the head 'mood'; the settings have \\['emotion', 'V'\\]"):
        dbstats.evaluate(None, _rows(), [{"emotion": ["low"]}], ["V"], models={"mood": None})
    with pytest.raises(ValueError, match="a feature DB has at least one row"):
        dbstats.evaluate(None, [], [{"emotion": ["low"]}], [])

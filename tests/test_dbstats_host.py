"""The host half of specification DS-1 without a GPU: webspeechanalyzer_amd/dbstats.py's vocabularies and index columns on the fixture's quirk
scenario, its refusals and their messages, js/dbstats.js's text against the fixture through node, and the new ABI symbols."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from webspeechanalyzer_amd import capi, dbstats

from . import dbstats_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = dbstats_cases.load_fixture()
NODE = shutil.which("node")


def _after(name):
    sc = FX["scenarios"][name]
    rows = json.loads(json.dumps(sc["rows"]))
    for r, p in zip(rows, sc["pred_after"]):
        r["pred"] = p
    return sc, rows


def test_quirk_columns():
    sc, rows = _after("b")
    col = dbstats.build_columns(rows, sc["class_labels"], sc["ordinal_labels"])
    by = {c["name"]: c for c in col["cats"]}
    n = len(rows)
    no_true = [i for i, r in enumerate(rows) if r["true"] is None]
    assert no_true, "the scenario has rows without a true pair"
    for c in col["cats"]:
        assert c["true_idx"].shape == c["pred_idx"].shape == (n,) and (c["true_idx"][no_true] == -1).all()
    # labels outside the class list do not count, and do not enter the vocabulary through the true column
    emo = by["emotion"]
    assert [emo["vocab"][i] for i in sorted(set(emo["true_idx"]) - {-1})] == ["N", "A"]
    assert all((emo["true_idx"][i] >= 0) == (r["true"] is not None and r["true"][0]["emotion"] in ("N", "A")) for i, r in enumerate(rows))
    assert "H" in emo["vocab"] and (emo["pred_idx"] == emo["vocab"].index("H")).all()          # predictions outside the class list are still labels
    # a numeric true label and a string prediction share one vocabulary entry (3 == "3")
    dig = by["digit"]
    assert sorted(dig["vocab"]) == ["3", "7"]
    three = dig["vocab"].index("3")
    assert any(t == three and p == three for t, p in zip(dig["true_idx"], dig["pred_idx"]))
    # '*' counts every truthy label; a null prediction (the non-softmax classifier) is blank
    assert len(by["word"]["vocab"]) >= 25 and (by["word"]["pred_idx"] == -1).all()
    assert (by["flat"]["pred_idx"] == -1).all() and set(by["flat"]["vocab"]) == {"x", "y"}
    # ordinal values: the host hands over numbers and NaN; 0 stays 0 for the device to drop
    v = {c["name"]: c for c in col["ords"]}["V"]
    assert np.isnan(v["true_value"][no_true]).all()
    kinds = [r["true"][1]["V"] if r["true"] else None for r in rows]
    assert any(k == 0 and v["true_value"][i] == 0.0 for i, k in enumerate(kinds) if k is not None and not isinstance(k, str))
    assert all(np.isnan(v["true_value"][i]) for i, k in enumerate(kinds) if k is None or isinstance(k, str))
    assert (v["pred_value"] == 0.0).any() and np.isnan(v["pred_value"]).any()
    assert np.allclose(col["durations"], [float(r["time"][1]) for r in rows], rtol=0, atol=0)


def test_update_pred_label_rule():
    cats, ords = dbstats.head_settings([{"emotion": ["A"]}], ["V"])
    row = dict(pred=None)
    dbstats.update_pred_label(row, cats, ords, "nohead", "A")
    assert row["pred"] == [{}, {}]                                                            # stored in every case
    dbstats.update_pred_label(row, cats, ords, "emotion", None)
    dbstats.update_pred_label(row, cats, ords, "V", float("nan"))
    assert row["pred"] == [{"emotion": None}, {"V": None}]                                     # NaN goes through JSON as null
    dbstats.update_pred_label(row, cats, ords, "V", 0.25)
    assert row["pred"] == [{"emotion": None}, {"V": 0.25}]


def test_refusals_and_their_messages():
    rows = [dict(time=["0.000", "0.100"], features=[0.0] * 53, true=[{"k": "v%d" % i}, {}], pred=None) for i in range(dbstats.MAX_CLASSES + 1)]
    with pytest.raises(ValueError, match=r"head 'k' has 257 distinct labels \(limit 256\)"):
        dbstats.build_columns(rows, [{"k": ["*"]}], [])
    with pytest.raises(ValueError, match=r"9 categorical heads \(limit 8\)"):
        dbstats.build_columns(rows[:2], [{"h%d" % i: ["*"]} for i in range(9)], [])
    with pytest.raises(ValueError, match=r"9 ordinal heads \(limit 8\)"):
        dbstats.build_columns(rows[:2], [], ["o%d" % i for i in range(9)])
    with pytest.raises(ValueError, match="at least one row"):
        dbstats.build_columns([], [{"k": ["*"]}], [])
    with pytest.raises(ValueError, match="one-key objects"):
        dbstats.head_settings(["emotion"], [])
    with pytest.raises(ValueError, match="'cats' or 'ords'"):
        dbstats.predict_db(None, rows[:2], ([{"k": ["*"]}], []), "cat", "k", None)
    with pytest.raises(ValueError, match="53 features"):
        dbstats.predict_db(None, [dict(time=[0, 1], features=[0.0] * 9)], ([], []), "cats", "k", None)


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_lines_are_the_fixtures():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "dbstats_lines.js"), os.path.join(ROOT, "tests", "golden", "dbstats_expected.json")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    assert sorted(got) == sorted(FX["scenarios"])
    for name, sc in FX["scenarios"].items():
        assert got[name] == sc["lines"], name


def test_header_declares_the_new_symbols_and_limits():
    header = open(os.path.join(ROOT, "include", "wsa.h")).read()
    names = [s for s in capi.ABI_SYMBOLS if s.startswith("wsa_dbstats_")]
    assert len(names) == 11
    for s in names:
        assert re.search(r"\b%s\s*\(" % s, header), s
    lim = {k: int(v) for k, v in re.findall(r"#define (WSA_DBSTATS_[A-Z_]+)\s+(\d+)", header)}
    assert lim == {"WSA_DBSTATS_MAX_CLASSES": dbstats.MAX_CLASSES, "WSA_DBSTATS_MAX_HEADS": dbstats.MAX_HEADS, "WSA_DBSTATS_CHUNK_ROWS": dbstats.CHUNK_ROWS}
    assert lim["WSA_DBSTATS_MAX_CLASSES"] >= 256 and lim["WSA_DBSTATS_MAX_HEADS"] >= 8
    assert (capi.DBSTATS_MAX_CLASSES, capi.DBSTATS_MAX_HEADS, capi.DBSTATS_CHUNK_ROWS) == (dbstats.MAX_CLASSES, dbstats.MAX_HEADS, dbstats.CHUNK_ROWS)

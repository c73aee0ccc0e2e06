"""CPU-side checks of the device feature DB (specification FD-1): the keep rule against lists written out by hand, the
label-only selection of train.select / select_ordinal against train.prepare / prepare_ordinal, and the part tags and time strings of the
host records.  The device half is tests/test_gpu_featdb.py."""
import numpy as np
import pytest

from tests import featdb_cases as fc
from tests import featdb_ref
from webspeechanalyzer_amd import featdb, train


@pytest.mark.parametrize("name", sorted(fc.L12_SMALL))
def test_level_12_keep_rule(name):
    meta, feat = fc.l12_small(name)
    want = fc.L12_SMALL[name]["kept"]
    assert featdb_ref.keep(12, meta, feat) == want
    kept, rows = featdb_ref.append(12, np.zeros((0, 23)), meta, feat)
    assert kept.tolist() == want and rows.shape == (len(want), 23)
    assert featdb_ref.same_bits(rows, feat[want, :23] if want else np.zeros((0, 23)))


@pytest.mark.parametrize("name", sorted(fc.L11_SMALL))
def test_level_11_keeps_the_last_utterance_row_of_a_clip(name):
    c = fc.L11_SMALL[name]
    assert featdb_ref.keep(11, off=c["off"]) == c["kept"]


def test_levels_5_and_13_keep_every_row():
    feat = fc.feature_table(7, 53, 4)
    assert featdb_ref.keep(13, feat=feat) == list(range(7))
    kept, rows = featdb_ref.append(5, feat[:2], feat=feat)
    assert kept.tolist() == list(range(7)) and featdb_ref.same_bits(rows, np.concatenate([feat[:2], feat]))


def test_seam_table_drops_rows_behind_a_seam():
    """the generator of the GPU cases does what its docstring says at a seam"""
    meta, feat = fc.l12_seam_table(200, [64, 128])
    kept = featdb_ref.keep(12, meta, feat)
    for s in (64, 128):
        assert feat[s - 1, 23] == 1 and len({tuple(m[:2]) for m in meta[s - 2:s + 3]}) == 1
        assert tuple(meta[s - 3][:2]) != tuple(meta[s - 2][:2]) != tuple(meta[s + 3][:2])
        assert s - 2 in kept and not {s - 1, s, s + 1, s + 2} & set(kept) and s + 3 in kept
    assert 0 < len(kept) < 200


def test_ranges_rule():
    rows = np.array([[1.0, -0.0, np.nan, 0.0, -0.0, 5.0], [-2.0, 0.0, 1.0, 0.0, -0.0, 5.0]])
    mn, mx = featdb_ref.ranges(rows)
    assert featdb_ref.same_bits(mn, [-2.0, -0.0, np.nan, 0.0, -0.0, 5.0])
    assert featdb_ref.same_bits(mx, [1.0, 0.0, np.nan, 0.0, -0.0, 5.0])


def _feat(n, seed=5):
    return np.nan_to_num(fc.feature_table(n, 53, seed), nan=0.25, posinf=3.0)


def test_select_is_the_label_half_of_prepare():
    c = fc.SELECT_TOPPED                                 # a class of 3 (not topped up), one of 4 (topped up to 5), unlabelled rows
    sel = train.select(c["labels"], c["classes"])
    assert sel["rows"] == c["rows"] and sel["y"].tolist() == c["y"] and sel["legend"] == c["legend"] and sel["counts"] == c["counts"]
    feat = _feat(len(c["labels"]))
    d = train.prepare(feat, c["labels"], c["classes"])
    assert d["rows"] == sel["rows"] and d["y"].tolist() == c["y"] and d["legend"] == sel["legend"] and d["counts"] == sel["counts"]
    assert featdb_ref.same_bits(d["features"], feat[c["rows"]])
    assert featdb_ref.same_bits(d["in_min"], feat[c["rows"]].min(axis=0)) and featdb_ref.same_bits(d["in_max"], feat[c["rows"]].max(axis=0))
    assert sorted(d) == ["counts", "features", "in_max", "in_min", "legend", "rows", "y"]


def test_select_two_classes_tied_at_the_maximum():
    c = fc.SELECT_TIED
    sel = train.select(c["labels"], c["classes"])
    assert sel["rows"] == c["rows"] and sel["y"].tolist() == c["y"] and sel["legend"] == c["legend"] and sel["counts"] == c["counts"]
    d = train.prepare(_feat(len(c["labels"])), c["labels"], c["classes"])
    assert d["rows"] == c["rows"] and d["y"].tolist() == c["y"]


def test_select_ordinal_is_the_label_half_of_prepare_ordinal():
    c = fc.SELECT_ORDINAL                                # values above 1.0 and None dropped, 0.25 and 0.5 in the lower bin
    sel = train.select_ordinal(c["values"])
    assert sel["rows"] == c["rows"] and sel["counts"] == c["counts"]
    assert sel["values"].tolist() == [c["values"][i] for i in c["rows"]]
    assert (sel["out_min"], sel["out_max"]) == (0.1, 1.0)
    feat = _feat(len(c["values"]))
    d = train.prepare_ordinal(feat, c["values"])
    assert d["rows"] == sel["rows"] and d["values"].tolist() == sel["values"].tolist() and d["counts"] == sel["counts"]
    assert (d["out_min"], d["out_max"]) == (sel["out_min"], sel["out_max"]) and featdb_ref.same_bits(d["features"], feat[c["rows"]])
    assert sorted(d) == ["counts", "features", "in_max", "in_min", "out_max", "out_min", "rows", "values"]


def test_select_refusals():
    with pytest.raises(ValueError, match="Sample size 9/12 too small"):
        train.select(["a"] * 9 + [None] * 3, ["a"])
    with pytest.raises(ValueError, match="Sample size 9/12 too small"):
        train.prepare(_feat(12), ["a"] * 9 + [None] * 3, ["a"])
    with pytest.raises(ValueError, match="Sample size 9/11 too small"):
        train.select_ordinal([0.5] * 9 + [1.5, None])
    with pytest.raises(ValueError, match=r"'\*' wildcard"):
        train.select(["a"] * 12, ["a", "*"])
    with pytest.raises(ValueError, match=r"'\*' wildcard"):
        train.prepare(_feat(12), ["a"] * 12, ["*"])


def test_records_part_tags_and_times():
    meta = np.zeros((len(fc.RECORD_META), 8), np.int32)
    meta[:, :4] = fc.RECORD_META
    kept = list(range(len(meta)))
    got = featdb.records(13, fc.RECORD_STEP, meta, kept, fc.RECORD_FILES)
    assert [(r["file"], r["seg"], r["time"]) for r in got] == fc.RECORDS_13
    assert all(r["true"] is None and r["pred"] is None and set(r) == {"file", "seg", "time", "true", "pred", "row"} for r in got)
    assert [(r["file"], r["seg"], r["time"]) for r in featdb.records(12, fc.RECORD_STEP, meta, kept, fc.RECORD_FILES)] == fc.RECORDS_13
    got5 = featdb.records(5, fc.RECORD_STEP, meta, kept, fc.RECORD_FILES)
    assert [(r["file"], r["seg"], r["time"]) for r in got5] == fc.RECORDS_5
    # a dropped row keeps the later rows' tags where they were: k is the position in the source callback
    some = featdb.records(12, fc.RECORD_STEP, meta, [0, 2, 3, 5], fc.RECORD_FILES)
    assert [r["seg"] for r in some] == ["2", "0", "0.01", "0.03"]
    # level 11: utterance metadata {clip, result, t_start, t_sum}, always part 0, numbers
    utt = np.array([[0, 0, 5, 4], [0, 1, 5, 9], [1, 0, 0, 7]], np.int32)
    got11 = featdb.records(11, fc.RECORD_STEP, utt, [1, 2], fc.RECORD_FILES)
    assert [(r["file"], r["seg"], r["time"]) for r in got11] == [("a.wav", "0", [0.0625, 0.125]), ("b.wav", "0", [0.0, 0.1])]

"""The float64 restatement of the multi-DB prediction path (tests/ensemble_ref.py) against the reference application's own
src/prediction.js with `available_DBs` set to [1, 2], [2, 1] and the six shipped DBs (tests/golden/ensemble_expected.json, generated
by tests/golden/gen/make_ensemble_golden.py).  The restatement is fed the golden's own probabilities, so everything it derives is
exact double arithmetic: labels, winning DB and min_entropy_db must be equal, sums and confidences agree to 1e-12 relative (the
order of additions is the reference's; the bound only allows for JSON's decimal round trip, which is exact for doubles in practice),
gauges to 1e-12, and the entropy to the three decimals the application prints.  No GPU."""
import json
import math
import os

import numpy as np
import pytest

from tests import classify_ref, ensemble_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = json.load(open(os.path.join(GOLD, "ensemble_expected.json")))
CG = json.load(open(os.path.join(GOLD, "classify_expected.json")))
CLIPS = CG["clips"]


def _close(a, b, rel=1e-12):
    return abs(a - b) <= rel * max(abs(a), abs(b))


def _replay(case):
    """Every clip of a case through the restatement; the reference's own carry of min_entropy_db across launches (it resets only
    max_inv_entropy) is applied here, as a host of the device tables does: the last non-negative value stays."""
    dbs = [str(d) for d in case["dbs"]]
    legends = [G["legend"][d] for d in dbs]
    row, carried, out = 0, None, []
    for clip in CLIPS:
        L = ensemble_ref.Launch(legends)
        res = []
        for cb in clip["callbacks"]:
            n = len(cb["feat"])
            durs = [float(t[1]) for t in cb["seg_time"]]
            r = L.callback(durs, [[G["prob"][d][q] for q in range(row, row + n)] for d in dbs])
            row += n
            if r["min_db"] is not None:
                carried = r["min_db"]
            res.append((r, carried))
        out.append((L, res))
    assert row == len(G["prob"][dbs[0]]) == 135
    return dbs, legends, out


def test_golden_covers_the_issue_cases():
    assert [c["dbs"] for c in G["cases"]] == [[1, 2], [2, 1], [1, 2, 4, 5, 6, 7]]
    assert len(CLIPS) == 20 and sum(len(c["callbacks"]) for c in CLIPS) == 43
    for d in ("1", "2"):                         # the same rows, the same models: the probabilities of the single-model fixture
        assert np.array_equal(np.array(G["prob"][d]), np.array(CG["models"][d + "/cats_emotion"]["prob"]))


@pytest.mark.parametrize("ci", range(3))
def test_restatement_reproduces_prediction_js(ci):
    case = G["cases"][ci]
    dbs, legends, out = _replay(case)
    n_checked = 0
    for (L, res), want_clip in zip(out, case["clips"]):
        assert len(res) == len(want_clip["callbacks"])
        for (r, carried), w in zip(res, want_clip["callbacks"]):
            if w["pred"] is None:                # the reference made no prediction: durations sum to 0
                assert r["skipped"]
            else:
                assert not r["skipped"]
                assert w["pred"][0] == r["label"]
                assert _close(w["pred"][1], r["conf"])
            assert (None if carried is None else case["dbs"][carried]) == w["min_entropy_db"]
            if r["min_db"] is not None and not r["skipped"]:
                assert [k for k, _ in r["meters"]] == [k for k, _ in w["gauges"]]
                for (_, a), (_, b) in zip(r["meters"], w["gauges"]):
                    assert abs(a - b) <= 1e-12
                assert abs(r["entropy"] - float(w["entropy_text"])) <= 0.0005 + 1e-12
                assert (r["entropy"] > 0.5) == w["entropy_red"]
            n_checked += 1
        for di, d in enumerate(dbs):
            acc, want = L.acc_all[di], want_clip["label_conf_all"][d]
            assert classify_ref._keys(acc) == [k for k, _ in want]
            for k, v in want:
                assert _close(acc[k], v)
    assert n_checked == 43


@pytest.mark.parametrize("ci", [0, 1])
def test_winning_db_is_the_one_whose_own_fold_gives_the_pair(ci):
    """The reference hands out only [label, confidence]; which DB won shows in the single-model fixture: the winner's own prediction
    is the pair, and it is the first of the (here never equal) largest confidences.  Both DBs win callbacks."""
    case = G["cases"][ci]
    dbs, legends, out = _replay(case)
    wins = {d: 0 for d in dbs}
    for ck, ((L, res), want_clip) in enumerate(zip(out, case["clips"])):
        for k, ((r, _), w) in enumerate(zip(res, want_clip["callbacks"])):
            single = {d: CG["models"][d + "/cats_emotion"]["clips"][ck]["callbacks"][k]["pred"] for d in dbs}
            best = max(dbs, key=lambda d: single[d][1])
            assert single[best] == w["pred"]
            assert dbs[r["db"]] == best
            for di, d in enumerate(dbs):
                assert r["per_db"][di][0] == single[d][0] and _close(r["per_db"][di][1], single[d][1])
            wins[best] += 1
    assert all(v > 0 for v in wins.values()) and sum(wins.values()) == 43


def test_per_db_fold_is_fold_clip():
    """The restatement's per-DB part is classify_ref.fold_clip's arithmetic: same labels and confidences, bit for bit."""
    case = G["cases"][2]
    dbs, legends, out = _replay(case)
    row = 0
    for clip, (L, res) in zip(CLIPS, out):
        n = sum(len(cb["feat"]) for cb in clip["callbacks"])
        for di, d in enumerate(dbs):
            items, q = [], row
            for cb in clip["callbacks"]:
                items.append(([float(t[1]) for t in cb["seg_time"]], G["prob"][d][q:q + len(cb["feat"])]))
                q += len(cb["feat"])
            want, acc = classify_ref.fold_clip(items, legends[di])
            assert [(r["per_db"][di][0], r["per_db"][di][1]) for r, _ in res] == want
            assert acc == L.acc_all[di]
        row += n


def _seeded_probs(seed, n, C):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, C))
    p = np.exp(x) / np.exp(x).sum(1, keepdims=True)
    return p.astype(np.float32).astype(np.float64)


def test_two_identical_members_every_tie_goes_to_the_first():
    labels = ["N", "A", "S", "H"]
    p = _seeded_probs(3, 12, 4)
    L = ensemble_ref.Launch([labels, labels])
    q = 0
    for n in (1, 3, 2, 1, 5):
        r = L.callback([0.1 + 0.025 * i for i in range(n)], [p[q:q + n], p[q:q + n]])
        q += n
        assert r["db"] == 0 and r["min_db"] == 0
        assert r["per_db"][0] == r["per_db"][1]
        assert r["label"] == r["per_db"][0][0] and r["conf"] == r["per_db"][0][1]


def test_a_launch_whose_first_callback_is_skipped():
    labels = [["N", "A", "S", "H"], ["x", "y"]]
    p0, p1 = _seeded_probs(4, 6, 4), _seeded_probs(5, 6, 2)
    L = ensemble_ref.Launch(labels)
    r = L.callback([0.0, 0.0], [p0[:2], p1[:2]])
    assert r["skipped"] and r["db"] == "skip" and r["min_db"] is None and math.isnan(r["entropy"]) and r["meters"] == []
    assert L.acc_all == [{}, {}] and L.max_inv_entropy == 0.0
    r = L.callback([0.2, 0.1, 0.3], [p0[2:5], p1[2:5]])
    assert not r["skipped"] and r["db"] in (0, 1) and r["min_db"] in (0, 1)
    acc = L.acc_all[r["min_db"]]
    total = 0
    for k in classify_ref._keys(acc):
        total += acc[k]
    assert abs(sum(v for _, v in r["meters"]) - 1.0) <= 1e-12 and 0.0 <= r["entropy"] < 1.0
    assert r["entropy"] == 1 - max(acc.values()) / total
    # a skipped callback later in the launch touches nothing
    before = (json.dumps(L.acc_all), L.max_inv_entropy, L.min_entropy_db)
    r2 = L.callback([0.0], [p0[5:6], p1[5:6]])
    assert r2["skipped"] and r2["min_db"] == r["min_db"] and r2["entropy"] == r["entropy"]
    assert before == (json.dumps(L.acc_all), L.max_inv_entropy, L.min_entropy_db)
    # fold_rows reports the device's codes: -2 skipped, -1 while no DB
    meta = np.zeros((5, 8), np.int32)
    meta[:, 1] = [0, 0, 1, 1, 1]
    meta[:2, 3] = -1                              # (t_len + 1) * step = 0: the skipped callback
    meta[2:, 3] = [7, 3, 11]
    out = ensemble_ref.fold_rows(meta, [p0[:5], p1[:5]], labels, 0.025)
    assert out["cb_db"][0] == -2 and out["cb_min_db"][0] == -1 and math.isnan(out["cb_entropy"][0]) and out["cb_label"][0][0] == -2
    assert out["cb_db"][1] in (0, 1) and out["cb_min_db"][1] in (0, 1) and out["clip_min_db"][0] == out["cb_min_db"][1]

"""CPU-side checks of specification FD-2 (what a stream step stores in the attached device feature DB): the restatement
tests/stream_featdb_ref.py against FD-1's restatement (tests/featdb_ref.py) for one step on a fresh state, every arm of it taken by
some hand-built case, a few outcomes written out by hand, and level 11 against the collector of js/featuredb.js under the local Node.
The device half is tests/test_gpu_stream_featdb.py."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import featdb_cases as fc
from tests import featdb_ref
from tests import stream_featdb_cases as sc
from tests import stream_featdb_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


def run_case(case):
    """the restatement over every step of a case: (state, the steps' outcomes)"""
    pattern, head = sc.initial(case)
    st = ref.State(case["level"], case["capacity"], case["n_streams"], fill=pattern)
    st.db[:case["start"]] = head
    st.count = case["start"]
    return st, [ref.step(st, **s) for s in case["steps"]]


@pytest.mark.parametrize("level", [5, 13, 12])
@pytest.mark.parametrize("n", [0, 1, 65, 1030])
def test_one_step_on_a_fresh_state_is_fd1(level, n):
    meta, feat = fc.l12_seam_table(n, [64, 1024]) if n > 1 else (fc.meta_table([(0, 0)] * n), fc.feature_table(n, 53, 1) if n else np.zeros((0, 53)))
    st = ref.State(level, n + 1)
    out = ref.step(st, meta=meta, feat=feat)
    want_kept, want_rows = featdb_ref.append(level, np.zeros((0, ref.WIDTH[level])), meta, feat)
    assert np.array_equal(out["kept"], want_kept) and out["n_added"] == len(want_kept) == st.count and out["first_row"] == 0
    assert ref.same_bits(st.rows(), want_rows)
    assert (out["n_replaced"], out["not_fitted"], out["flags"]) == (0, 0, 0)
    if level == 12 and n > 64:
        assert 0 < len(want_kept) < n


def test_every_arm_is_taken_by_some_case():
    arms = set()
    for name, make in sc.CASES.items():
        st, _ = run_case(make())
        arms |= set(st.arms)
    assert arms == set(sc.ARMS), (sorted(arms - set(sc.ARMS)), sorted(set(sc.ARMS) - arms))


def test_the_cases_sit_where_their_names_say():
    kept = lambda name: run_case(sc.CASES[name]())[1][0]["kept"].tolist()
    k = kept("l12_mark_last_row_of_wave")
    assert 62 in k and 63 not in k and 64 not in k and 65 in k and len(k) == 128
    k = kept("l12_mark_first_row_of_next_wave")
    assert 63 in k and 64 not in k and 65 in k and len(k) == 129
    k = kept("l12_mark_first_row_of_wave_and_callback")
    assert 63 in k and not {64, 65, 66, 67} & set(k) and 68 in k
    k = kept("l12_mark_before_walk_seam")
    assert 1022 in k and 1023 not in k and 1024 not in k and 1025 in k
    k = kept("l12_mark_behind_walk_seam")
    assert 1023 in k and 1024 not in k and 1025 in k
    k = kept("l12_mark_first_row_behind_walk_seam")
    assert 1023 in k and not {1024, 1025, 1026, 1027} & set(k) and 1028 in k
    k = kept("l12_mark_carried_over_two_waves")
    assert k == list(range(10)) + list(range(200, 256))
    assert kept("l12_nan_and_minus_zero") == [0, 1, 4, 5]


def test_the_capacity_decision():
    st, outs = run_case(sc.CASES["fit_exact_13"]())
    assert [o["n_added"] for o in outs] == [5, 7, 0] and [o["not_fitted"] for o in outs] == [0, 0, 1] and st.count == 12
    assert [o["flags"] for o in outs] == [0, 0, ref.FLAG_DB_FULL]
    st, outs = run_case(sc.CASES["fit_one_too_many_13"]())
    assert [o["n_added"] for o in outs] == [5, 0, 1] and [o["not_fitted"] for o in outs] == [0, 7, 0] and st.count == 6
    assert [o["first_row"] for o in outs] == [0, 5, 5]
    st, outs = run_case(sc.CASES["fit_one_too_many_12"]())
    assert [o["n_added"] for o in outs] == [4, 0, 1] and [o["not_fitted"] for o in outs] == [0, 68, 0] and st.count == 7
    st, outs = run_case(sc.CASES["capacity_flag_13"]())
    assert [o["n_added"] for o in outs] == [5, 0, 1] and [o["not_fitted"] for o in outs] == [0, 0, 0] and [o["flags"] for o in outs] == [0, 1, 0]
    # a step that stores nothing leaves every byte
    case = sc.CASES["fit_one_too_many_13"]()
    pattern, head = sc.initial(case)
    st = ref.State(13, case["capacity"], fill=pattern)
    ref.step(st, **case["steps"][0])
    before = st.db.copy()
    ref.step(st, **case["steps"][1])
    assert ref.same_bits(before, st.db)


def test_level_11_one_row_per_launch():
    st, outs = run_case(sc.CASES["l11_stop_then_start"]())
    assert [(o["n_added"], o["n_replaced"]) for o in outs] == [(2, 0), (0, 1), (0, 1), (1, 0), (0, 2)]
    assert st.slot.tolist() == [2, 1] and st.count == 3
    assert outs[4]["replaced"].tolist() == [[0, 2], [1, 1]]
    st, outs = run_case(sc.CASES["l11_two_results_last_wins"]())
    assert outs[0]["kept"].tolist() == [1, 2] and outs[1]["replaced"].tolist() == [[2, 0]]
    assert ref.same_bits(st.db[0], sc.CASES["l11_two_results_last_wins"]()["steps"][1]["feat"][2])
    st, outs = run_case(sc.CASES["l11_no_room_for_one_new_row"]())
    assert [(o["n_added"], o["n_replaced"], o["not_fitted"]) for o in outs] == [(2, 0, 0), (0, 0, 1), (0, 2, 0)] and st.slot.tolist() == [0, 1, -1]
    st, outs = run_case(sc.CASES["l11_full_step_start_still_forgets"]())
    assert outs[1]["not_fitted"] == 1 and st.slot.tolist() == [-1, 1] and [o["n_replaced"] for o in outs] == [0, 0, 1]
    st, outs = run_case(sc.CASES["l11_capacity_flag"]())
    assert [(o["n_added"], o["n_replaced"]) for o in outs] == [(2, 0), (0, 0), (1, 1)] and st.slot.tolist() == [2, 1]


L11_AGAINST_THE_COLLECTOR = ["l11_first_result", "l11_two_results_last_wins", "l11_result_on_start_step", "l11_stop_then_start", "l11_start_without_result",
                             "l11_idle_between_active", "l11_exact_fit", "l11_65_streams"]


@pytest.mark.skipif(NODE is None, reason="node not installed")
@pytest.mark.parametrize("name", L11_AGAINST_THE_COLLECTOR)
def test_level_11_holds_what_the_js_collector_holds(name, tmp_path):
    """the same results in order into the collector of js/featuredb.js, part "0", one file name per stream launch (a START begins the
    next): per launch the DB holds the collector's vector, and the DB's rows are in the collector's order.  The collector stores
    through JSON, so the vectors here are ordinary numbers."""
    case = sc.CASES[name]()
    n = case["n_streams"]
    st = ref.State(11, case["capacity"] - case["start"], n)
    launch = [-1] * n
    calls, row_name = [], {}
    for k, s in enumerate(case["steps"]):
        feat = np.nan_to_num(s["feat"], nan=0.5, posinf=7.0, neginf=-7.0) + 0.0      # (+ 0.0: no -0)
        for i in range(n):
            if int(s["bits"][i]) & sc.START:
                launch[i] += 1
            for u in range(int(s["utt_off"][i]), int(s["utt_off"][i + 1])):
                calls.append([f"stream{i}_launch{launch[i]}", [0.25 * k, 0.5], [float(x) for x in feat[u]]])
        out = ref.step(st, feat=feat, utt_off=s["utt_off"], bits=s["bits"], flags=s["flags"])
        assert out["not_fitted"] == 0
        stream_of = np.searchsorted(s["utt_off"], out["kept"], side="right") - 1
        for j, i in enumerate(stream_of):
            row_name[out["first_row"] + j] = f"stream{i}_launch{launch[i]}"
    job = tmp_path / "calls.json"
    job.write_text(json.dumps(calls))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "stream_featdb_collect.js"), str(job)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout)
    assert got["refused"] == [] and len(got["samples"]) == st.count > 0
    assert [x["file"] for x in got["samples"]] == [row_name[r] for r in range(st.count)]
    assert all(x["seg"] == "0" for x in got["samples"])
    assert ref.same_bits(np.array([x["features"] for x in got["samples"]], np.float64), st.rows())

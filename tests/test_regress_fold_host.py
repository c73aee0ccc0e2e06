"""Specification RG-1 on the CPU: the float64 restatement tests/regress_fold_cases.rg1_ref against numpy's weighted average on every
hand-built case, the invariance of a stream's running sums under any dealing of its rows over steps, the CPU check that the
separate-rounding case really tells a fused multiply-add from two roundings, and the built library's new entries."""
import math

import numpy as np
import pytest

from tests import regress_fold_cases as C
from tests.classify_ref import fixed3

BATCH = C.batch_cases()
STREAMS = C.stream_cases()
# relative to the weighted average itself; sums of at most 1024 f64 terms: n 2^-53 = 1.1e-13, with ten times margin
REL = 1e-12


def _weights(meta, step_s):
    d = np.array([fixed3((int(m[3]) + 1) * step_s) for m in meta])
    return d, np.sqrt(d)


def _close(got, want):
    """both NaN, or within REL of the weighted average, relative"""
    if math.isnan(want) or math.isnan(got):
        return math.isnan(want) and math.isnan(got)
    return abs(got - want) <= REL * abs(want)


def _average(v, w):
    """np.average over the finite values; NaN when no weight is left"""
    ok = np.isfinite(v)
    if not ok.any() or w[ok].sum() == 0:
        return C.NAN
    return float(np.average(v[ok], weights=w[ok]))


@pytest.mark.parametrize("case", BATCH, ids=[c["name"] for c in BATCH])
def test_rg1_ref_is_the_weighted_average_per_callback_and_per_clip(case):
    meta, values, off = case["meta"], case["values"], case["row_off"]
    H = values.shape[0]
    assert len(meta) <= 1024
    d, w = _weights(meta, case["step_s"])
    cbs, run = C.rg1_ref(meta, values, case["step_s"])
    assert sum(cb["skipped"] for cb in cbs) == case.get("skipped", 0)
    kept = np.zeros(len(meta), bool)
    for cb in cbs:
        a, b = cb["first"], cb["first"] + cb["rows"]
        assert cb["skipped"] == (not d[a:b].sum() > 0)
        for h in range(H):
            if cb["skipped"]:
                assert math.isnan(cb["value"][h]) and cb["weight"][h] == 0.0
                continue
            want = _average(values[h, a:b], w[a:b])
            assert _close(cb["value"][h], want), (case["name"], cb["si"], h)
            assert abs(cb["weight"][h] - w[a:b][np.isfinite(values[h, a:b])].sum()) <= REL * max(cb["weight"][h], 1e-300)
        kept[a:b] = not cb["skipped"]
    for clip in range(len(off) - 1):
        a, b = int(off[clip]), int(off[clip + 1])
        A, B, V = C.run_value(run, clip, H)
        for h in range(H):
            sel = kept[a:b]
            want = _average(values[h, a:b][sel], w[a:b][sel]) if sel.any() else C.NAN
            assert _close(V[h], want), (case["name"], clip, h)
        if a == b:
            assert A == [0.0] * H and B == [0.0] * H and all(math.isnan(x) for x in V)


def test_the_cases_hold_what_they_are_built_for():
    by = {c["name"]: c for c in BATCH}
    sizes = sorted({cb["rows"] for cb in C.rg1_ref(by["sizes_H3"]["meta"], by["sizes_H3"]["values"], 0.025)[0]})
    assert sizes == list(C.SIZES)
    assert {c["values"].shape[0] for c in BATCH} >= {1, 3, 8}
    assert any(int(o[k]) == int(o[k + 1]) for o in [by["sizes_H1"]["row_off"]] for k in range(len(o) - 1))      # a clip with no rows
    z = by["zero_durations"]
    d, _ = _weights(z["meta"], z["step_s"])
    cbs, run = C.rg1_ref(z["meta"], z["values"], z["step_s"])
    assert any(not cb["skipped"] and (d[cb["first"]:cb["first"] + cb["rows"]] == 0).any() for cb in cbs)           # a d = 0 row among positive ones
    # a skipped callback leaves the running sums untouched: the same rows without the skipped callbacks give the same bits
    keep = np.concatenate([np.arange(cb["first"], cb["first"] + cb["rows"]) for cb in cbs if not cb["skipped"]])
    assert C.rg1_ref(z["meta"][keep], z["values"][:, keep], z["step_s"])[1] == {k: v for k, v in run.items() if v[1][0] != 0}
    assert run[1] == ([0.0] * 3, [0.0] * 3)
    u = by["unusable_rows"]
    cbs, run = C.rg1_ref(u["meta"], u["values"], u["step_s"])
    fine = np.where(np.isfinite(u["values"]), u["values"], 0.25)
    cbs_fine, run_fine = C.rg1_ref(u["meta"], fine, u["step_s"])
    assert not np.isfinite(u["values"][1]).all() and np.isfinite(u["values"][0]).all()
    for cb, cf in zip(cbs, cbs_fine):                                 # the other heads never notice
        assert cb["value"][0] == cf["value"][0] and cb["weight"][0] == cf["weight"][0]
    assert run[0][0][0] == run_fine[0][0][0] and run[0][1][0] == run_fine[0][1][0]
    assert math.isnan(cbs[1]["value"][2]) and cbs[1]["weight"][2] == 0.0 and not cbs[1]["skipped"]      # head 2 lost the whole callback
    only_first, _ = C.rg1_ref(u["meta"][:5], u["values"][:, :5], u["step_s"])
    third_alone, _ = C.rg1_ref(u["meta"][9:int(u["row_off"][1])], u["values"][:, 9:int(u["row_off"][1])], u["step_s"])
    assert math.isnan(C.run_value(run, 1, 3)[2][1]) and run[1][1][1] == 0.0                             # head 1 has nothing in clip 1
    assert only_first[0]["value"][2] == cbs[0]["value"][2] and third_alone[0]["value"][2] == cbs[2]["value"][2]


def test_a_fused_multiply_add_gives_other_bits_on_the_separate_rounding_case():
    c = next(c for c in BATCH if c["name"] == "separate_rounding")
    two, run_two = C.rg1_ref(c["meta"], c["values"], c["step_s"])
    one, run_one = C.rg1_ref(c["meta"], c["values"], c["step_s"], fused=True)
    differ = sum(a["value"][h] != b["value"][h] for a, b in zip(two, one) for h in range(2))
    print(f"{differ} of {2 * len(two)} callback values differ between two roundings and one")
    assert differ >= 1 and run_two != run_one
    for a, b in zip(two, one):                                          # ... by rounding only
        assert np.allclose(a["value"], b["value"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", STREAMS, ids=[c["name"] for c in STREAMS])
def test_dealing_rows_over_steps_gives_the_bits_of_one_pass(case):
    """Per stream, the running sums after the last step equal one pass over the rows the stream got since its last START, however the
    rows were dealt; every other dealing of the same rows (one step, one row per step, random cuts) gives the same bits too."""
    steps = C.rg1_streams(case)
    H, n = case["values"].shape[0], case["n"]
    since = {s: [] for s in range(n)}
    row0 = 0
    for off, ctl in zip(case["row_off"], case["ctl"]):
        for s in range(n):
            if int(ctl[s]) & C.START:
                since[s] = []
            since[s].extend(range(row0 + int(off[s]), row0 + int(off[s + 1])))
        row0 += int(off[-1])
    final = steps[-1][1]
    rng = np.random.default_rng(5)
    for s in range(n):
        rows = np.array(since[s], np.int64)
        whole = C.rg1_ref(case["meta"][rows], case["values"][:, rows], case["step_s"])[1]
        assert C.run_value(whole, s, H)[:2] == C.run_value(final, s, H)[:2], (case["name"], s)
        for cuts in ([], list(range(1, len(rows))), sorted(set(rng.integers(0, len(rows) + 1, 4).tolist()))):
            run = {}
            for a, b in zip([0] + cuts, cuts + [len(rows)]):
                run = C.rg1_ref(case["meta"][rows[a:b]], case["values"][:, rows[a:b]], case["step_s"], run)[1]
            assert C.run_value(run, s, H)[:2] == C.run_value(final, s, H)[:2], (case["name"], s, cuts)


def test_stream_cases_hold_what_they_are_built_for():
    by = {c["name"]: c for c in STREAMS}
    assert (np.diff(by["one_row_per_step"]["row_off"], axis=1)[:, 0] == 1).all()
    split = C.rg1_streams(by["callback_split"])
    assert [cb["rows"] for cbs, _ in split for cb in cbs if cb["who"] == 0] == [2, 1, 64, 65, 3]
    r = by["restart_idle_stop_start"]
    assert (r["ctl"][2:, 0] & C.START).any() and (r["ctl"][1:3, 1] == 0).all() and r["ctl"][1, 2] & C.STOP and r["ctl"][3, 2] & C.START
    e = C.rg1_streams(by["empty_steps"])
    assert e[1][1][1] == ([0.0] * 3, [0.0] * 3) and e[1][1][0] == e[0][1][0] and e[2][1] == e[1][1]


def test_library_exports_the_regression_group_entries():
    from webspeechanalyzer_amd import capi
    capi.build_library()
    L = capi.lib()
    for name in ("wsa_regress_group_create", "wsa_regress_group_destroy", "wsa_regress_group_rows", "wsa_batch_regress_group",
                 "wsa_batch_value_result", "wsa_batch_copy_value_fold", "wsa_stream_set_regress", "wsa_stream_values", "wsa_debug_regress_fold"):
        assert hasattr(L, name), name
        assert name in capi.ABI_SYMBOLS or name.startswith("wsa_debug_")

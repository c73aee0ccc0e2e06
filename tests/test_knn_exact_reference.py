"""The hand-built exact rows of tests/knn_exact_cases.py on the CPU: what tests/test_gpu_knn_exact.py holds the KNN kernels to, bit for
bit, is pinned here before anything runs on a GPU.

* knn_ref.exact_similarities (integers: places, signs, exponents) equals knn_ref.similarities (float64 cosines) bit for bit on every case;
* knn_ref.stream_select — the device's own form: tiles, blocks, the pass order, `key >= thr` against the threshold read at the block's
  start, knn_insert, the re-read, K9s's partial lists and merge — equals knn_ref.select on every case, at every k and slice count used;
* every arm of knn_ref.KNN_ARM_NAMES is reached, each case reaches the arms it was built for, and the two forms no input can reach are
  listed in knn_ref.UNREACHABLE with the argument;
* every fault of knn_ref.FAULTS changes the output of the case named for its arm (knn_exact_cases.FAULT_CASES); the two one-line changes
  that cannot show (knn_ref.EQUIVALENT) change no output of any case, and `no_reread` turns reread.refuses into insert.refused_stale;
* tests/golden/knn_exact_expected.json: ml5's own similarities on these rows equal exact_similarities bit for bit, and its neighbours,
  confidences and label equal knn_ref.select's — no margin condition: the arithmetic is exact for tfjs too."""
import base64
import json
import os
import zlib
from collections import Counter

import numpy as np
import pytest

from tests import knn_exact_cases as kc
from tests import knn_ref
from tests.util import GOLDEN

TABLES = ("label", "conf", "nbr", "sim")
_RUNS = {}


def expected(sim, cls, C, k):
    """the four tables as the device writes them, from given similarities and knn_ref.select: the model the GPU is held to"""
    sim = np.asarray(sim, np.float32)
    q, n = sim.shape
    r = knn_ref.select(sim, cls, C, k)
    k_eff = min(k, n)
    nbr = np.full((q, k), -1, np.int32)
    nbr[:, :k_eff] = r["nbr"]
    s = np.full((q, k), np.nan, np.float32)
    s[:, :k_eff] = sim[np.arange(q)[:, None], r["nbr"]]
    s[np.isnan(s)] = np.float32(np.nan)                          # one NaN: the quiet NaN the kernel writes (0x7fc00000)
    return dict(label=r["label"].astype(np.int32), conf=r["conf"], nbr=nbr, sim=s)


def clamped(c):
    return np.where((c["cls"] < 0) | (c["cls"] >= c["C"]), 0, c["cls"])


def variants(c):
    """(k, slices) of every run of a case"""
    return [(k, s) for k in c["ks"] for s in (None,) + tuple(c["slices"])]


def runs(key):
    """every run of a case through stream_select, once: {(k, slices): out}, and the exact similarities"""
    if key not in _RUNS:
        c = kc.CASES[key]
        sim = knn_ref.exact_similarities(c["store"], c["queries"])
        _RUNS[key] = (sim, {(k, s): knn_ref.stream_select(sim, c["cls"], k, s, n_classes=c["C"], adds=c["adds"], grid=kc.GRID.get(key) if s is None else None)
                            for k, s in variants(c)})
    return _RUNS[key]


def same(a, b):
    return all(np.asarray(a[t]).tobytes() == np.asarray(b[t]).tobytes() for t in TABLES)


@pytest.mark.parametrize("key", list(kc.CASES))
def test_exact_similarities_equal_the_float64_cosines(key):
    c = kc.CASES[key]
    exact = knn_ref.exact_similarities(c["store"], c["queries"])
    ref = knn_ref.similarities(c["store"], c["queries"])
    assert exact.dtype == np.float32 and (ref.astype(np.float32).astype(np.float64) == ref)[~np.isnan(ref)].all(), "the cosines are f32 numbers"
    assert np.array_equal(np.isnan(exact), np.isnan(ref))
    assert np.array_equal(exact.astype(np.float64), ref, equal_nan=True)
    assert not np.signbit(exact[~np.isnan(exact)] == 0).any() and not (np.signbit(exact) & (exact == 0)).any(), "expected zeros are +0"
    assert c["ml5"] == (not np.isnan(exact).any() and key != "grid" and key != "bad_class")


@pytest.mark.parametrize("key", list(kc.CASES))
def test_the_device_form_equals_the_restatement(key):
    c = kc.CASES[key]
    sim, out = runs(key)
    for (k, s), got in out.items():
        want = expected(sim, clamped(c), c["C"], k)
        for t in TABLES:
            assert got[t].tobytes() == want[t].tobytes(), (key, k, s, t)
        assert np.array_equal(got["rank"], knn_ref.grouped_rank(clamped(c))), "the ranks of the add calls are ml5's grouped ranks"
        assert got["counts"] == np.bincount(clamped(c), minlength=c["C"]).tolist()
    assert (out[c["ks"][0], None]["bad"] == kc.BAD_ROW + 1) if key == "bad_class" else out[c["ks"][0], None]["bad"] == 0


def test_every_case_takes_the_arms_it_was_built_for():
    for key, c in kc.CASES.items():
        arms = Counter()
        for o in runs(key)[1].values():
            arms.update(o["arms"])
        assert set(arms) <= set(knn_ref.KNN_ARM_NAMES), sorted(set(arms) - set(knn_ref.KNN_ARM_NAMES))
        short = [a for a in c["expect"] if not arms[a]]
        assert not short, f"{key}: arms not taken: {short}"


def test_no_arm_is_left_out():
    total = dict.fromkeys(knn_ref.KNN_ARM_NAMES + tuple(knn_ref.UNREACHABLE), 0)
    first = {}
    for key in kc.CASES:
        for o in runs(key)[1].values():
            for a, v in o["arms"].items():
                total[a] += v
                first.setdefault(a, key)
    never = sorted(a for a, v in total.items() if v == 0)
    assert never == sorted(knn_ref.UNREACHABLE), never
    assert all(len(why) > 40 for why in knn_ref.UNREACHABLE.values())
    assert set(first) == set(knn_ref.KNN_ARM_NAMES)              # each arm has a case that reaches it


def test_the_global_counter_counts_as_the_others_do():
    c = kc.CASES["ins_fill"]
    knn_ref.KNN_ARMS.clear()
    o = knn_ref.stream_select(knn_ref.exact_similarities(c["store"], c["queries"]), c["cls"], 4)
    assert knn_ref.KNN_ARMS == o["arms"] and knn_ref.KNN_ARMS["insert.fills"] == 2


def _faulty(key, fault):
    """the (k, slices) runs of a case whose output the fault changes"""
    c = kc.CASES[key]
    sim, out = runs(key)
    changed = []
    for (k, s), good in out.items():
        bad = knn_ref.stream_select(sim, c["cls"], k, s, n_classes=c["C"], adds=c["adds"], grid=kc.GRID.get(key) if s is None else None, fault=fault)
        if not same(good, bad):
            changed.append((k, s))
    return changed


@pytest.mark.parametrize("fault", list(knn_ref.FAULTS))
def test_every_fault_changes_the_output_of_its_case(fault):
    assert set(kc.FAULT_CASES) == set(knn_ref.FAULTS) and len(knn_ref.FAULTS) >= 10
    key = kc.FAULT_CASES[fault]
    changed = _faulty(key, fault)
    assert changed, f"fault {fault} ({knn_ref.FAULTS[fault]}) goes unnoticed by {key}"
    if fault.startswith("merge_"):
        assert all(s is not None for _, s in changed), "a fault of the merge shows in K9s alone"


@pytest.mark.parametrize("fault", list(knn_ref.EQUIVALENT))
def test_the_equivalent_changes_change_no_output(fault):
    """if one of these ever changes an output its argument no longer holds: it is a fault then and needs its case"""
    for key in ("ins_fill", "ins_places", "keff", "tie_kth", "stale_lanes", "stale_i", "stale_blocks", "neg_t1", "nan_rows", "same_rows", "families"):
        assert not _faulty(key, fault), (fault, key)
    if fault == "no_reread":
        c = kc.CASES["stale_blocks"]
        sim, out = runs("stale_blocks")
        bad = knn_ref.stream_select(sim, c["cls"], 1, n_classes=c["C"], fault=fault)["arms"]
        good = out[1, None]["arms"]
        assert good["reread.refuses"] > 0 and bad["reread.refuses"] == 0
        assert bad["insert.refused_stale"] == good["insert.refused_stale"] + good["reread.refuses"]


def test_the_last_grid_row_gives_the_bits_it_gives_alone():
    c = kc.CASES["grid"]
    sim, out = runs("grid")
    q = len(c["queries"])
    assert q == 8 * kc.GRID_CPU_CU * kc.QT + 1 and out[1, None]["arms"]["grid.second_trip"] == 1
    alone = knn_ref.stream_select(sim[-1:], c["cls"], 1, n_classes=1)
    assert all(out[1, None][t][-1:].tobytes() == alone[t].tobytes() for t in TABLES)
    pat = expected(knn_ref.exact_similarities(c["store"], kc.grid_queries(kc.GRID_PERIOD)), c["cls"], 1, 1)
    assert all(out[1, None][t].tobytes() == pat[t][np.arange(q) % kc.GRID_PERIOD].tobytes() for t in TABLES), "row i is pattern i mod 5"


# ---- the pin to ml5 itself
FIXTURE = json.load(open(os.path.join(GOLDEN, "knn_exact_expected.json")))


def test_the_fixture_holds_every_ml5_case():
    assert sorted(FIXTURE["cases"]) == sorted(k for k, c in kc.CASES.items() if c["ml5"])


@pytest.mark.parametrize("key", [k for k, c in kc.CASES.items() if c["ml5"]])
def test_ml5_equals_the_exact_model(key):
    c, f = kc.CASES[key], FIXTURE["cases"][key]
    exact = knn_ref.exact_similarities(c["store"], c["queries"])
    q, n = exact.shape
    def table(b64, dtype, width):
        return np.frombuffer(zlib.decompress(base64.b64decode(b64)), dtype).reshape(q, width)
    assert table(f["sims_f32_zlib_b64"], "<f4", n).tobytes() == exact.tobytes(), "ml5's f32 matMul gives the integer formula's bits, +0 included"
    present = [int(x) for x in f["class_keys"]]                   # ml5 numbers a number label by itself and lists the classes it holds, ascending
    assert present == sorted(set(c["cls"].tolist()))
    for k in c["ks"]:
        want, got = knn_ref.select(exact, c["cls"], c["C"], k), f["results"][str(k)]
        assert np.array_equal(table(got["nbr_i16_zlib_b64"], "<i2", min(k, n)), want["nbr"]), (key, k)
        assert table(got["conf_f64_zlib_b64"], "<f8", len(present)).tobytes() == want["conf"][:, present].astype("<f8").tobytes(), (key, k)
        assert got["label"] == want["label"].tolist(), (key, k)

"""The arrangements of tests/stream_tracker_cases.py on the CPU, oracle only: that the step boundaries they lay over the hand-built tracker clips fall on every
kind of state the stream tracker (csrc/tracker_one.hpp track_stream) carries from one step to the next, and that a clip still does what it was built for when it
stands in a chain.  tests/test_gpu_stream_tracker.py runs the same arrangements on the device.

(a) Boundary classes, counted from the oracle's gate record (per frame: accumulate_fm called or not; per segment: its span [begin, end)) and its tracker table
record (pyoracle.run_backend(track=True)["track"]["frames"]: the table as the device holds it between two frames) over all arrangements of all families.  A
class has a floor above one where a single hit could be an accident of one clip; the classes that only one arrangement is built for (`cut`) have one.
(b) In `chained` every case meets, in every stream and on at least one of its passes, every arm of its `expect` (a pass: families of fewer frames than three
rings go round their cases again; under the automatic gate the gate's state is carried from pass to pass too, so only the first pass sees the floor the case
was built against).  The one exception is the second stream of the family `auto`, which starts with silence so that its only segment lies across the ring's
end and therefore files its start frame under the index the silence ran up: the unshifted chain stands next to it and is checked.

Counts as printed by this test (all arrangements, all families):
  live 6877   live_over_64 413   live_over_128 156   dead_in_table 4334   stale_set 6870   after_last_accumulate 3387   behind_finalize 266
  before_first_accumulate 1   step_closes_two 34   step_closes_and_starts 1029   closed_by_stop 1   gate_reset_in_step 29   zero_step_in_span 150
  ring_straddled 132   cut 1   finalize_nothing_accumulated 0 (unreachable, stream_tracker_cases.UNREACHABLE)"""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle
from tests import stream_tracker_cases as sc
from tests import tracker_rule_cases as rc

# class -> the least number of boundaries (or steps) over all arrangements
FLOORS = {
    "live": 100, "live_over_64": 10, "live_over_128": 10,          # the restore / save loops' first, second and third pass of 64 entries
    "dead_in_table": 10, "stale_set": 10,
    "after_last_accumulate": 10, "behind_finalize": 10,
    "before_first_accumulate": 1,                                    # only a cut (or STOP) leaves a span open without an accumulate call: the `cut` arrangement
    "step_closes_two": 3, "step_closes_and_starts": 10,
    "closed_by_stop": 1, "cut": 1,                                   # the `cut` arrangement's one stream
    "gate_reset_in_step": 4,                                         # the four crowded clips of the automatic gate
    "zero_step_in_span": 10, "ring_straddled": 10,
}


@pytest.fixture(scope="module")
def all_arrangements():
    return {fam: sc.arrangements(fam) for fam in sc.FAMILY_NAMES}


def test_arrangements_hold_the_clips_unchanged(all_arrangements):
    for fam, arrs in all_arrangements.items():
        cases = sc.family(fam)["cases"]
        assert 1 <= len(cases) <= 41 and all(0 < len(c["spectra"]) <= 64 for c in cases), fam
        names = [a["name"] for a in arrs]
        assert names[:7] == ["alone-1", "alone-2", "alone-3", "alone-7", "alone-64", "ragged", "chained"] and (names[7:] == ["cut"]) == (fam == "f1")
        for a in arrs:
            for s in a["streams"]:
                assert sum(s["counts"]) == len(s["frames"]) and all(0 <= c <= a["F"] for c in s["counts"]) and s["counts"][-1] > 0
            if a["kind"] == "alone":
                assert len(a["streams"]) == len(cases) and all(np.array_equal(s["frames"], c["spectra"]) for s, c in zip(a["streams"], cases))
            if a["name"] == "alone-64":
                assert sc.n_steps(a) == 1
            if a["name"] == "alone-1":
                assert all(set(s["counts"]) == {1} for s in a["streams"])
            if a["name"] == "ragged":
                assert all(0 in s["counts"] for s in a["streams"]) and a["F"] == sc.RAGGED_F
            if a["name"] in ("chained", "cut"):
                assert a["ring"] == sc.CHAIN_RING == sc.stream_ring_frames(a["F"], sc.CHAIN_MAX_SPAN)      # the smallest ring there is
                for s in a["streams"]:                       # a chain is its cases' frames in order, nothing else (bar closing zeros dropped and leading ones)
                    for name, lo, hi in s["where"]:
                        src = next(c["spectra"] for c in cases if c["name"] == name)
                        assert np.array_equal(s["frames"][lo:hi], src[:hi - lo]) and not src[hi - lo:].any(), (fam, a["name"], name)
                    assert not s["frames"][:s["where"][0][1]].any()


def test_every_boundary_class_occurs(all_arrangements):
    total = dict.fromkeys(sc.CLASSES, 0)
    for fam, arrs in all_arrangements.items():
        for a in arrs:
            n = sc.boundary_classes(a)
            print("%-8s %-8s %2d streams %3d steps %s" % (fam, a["name"], len(a["streams"]), sc.n_steps(a), {k: v for k, v in n.items() if v}))
            for k, v in n.items():
                total[k] += v
    print("boundary classes over all arrangements:", total)
    assert set(FLOORS) | set(sc.UNREACHABLE) == set(sc.CLASSES)
    for k, floor in FLOORS.items():
        assert total[k] >= floor, (k, total[k], floor)
    for k in sc.UNREACHABLE:
        assert total[k] == 0, (k, "reached after all: give it a floor")


def test_the_table_passes_64_and_128_entries_in_alone_and_in_chained_streams(all_arrangements):
    """entries 64 .. 127 and 128 .. of the saved table cross a boundary in more than one kind of arrangement (not only where a whole clip is one step)"""
    for fam in ("lim-low", "lim-high"):
        for a in all_arrangements[fam]:
            if a["name"] in ("alone-1", "alone-7", "ragged", "chained"):
                n = sc.boundary_classes(a)
                assert n["live_over_64"] >= 2 and n["live_over_128"] >= 2, (fam, a["name"], n)


@pytest.mark.parametrize("fam", sc.FAMILY_NAMES)
def test_chained_every_case_straddles_the_ring_in_some_stream(fam):
    a = sc.chained(fam)
    names = {c["name"] for c in sc.family(fam)["cases"]}
    got = [sc._straddlers(fam, s) for s in a["streams"]]
    assert set().union(*got) == names, (fam, sorted(names - set().union(*got)))
    covered = set()
    for s, g in zip(a["streams"], got):                      # greedy: no stream that adds nothing (bar the unshifted chain next to a shifted one)
        assert g - covered or (not s.get("shifted") and any(x.get("shifted") for x in a["streams"])), fam
        covered |= g
    assert len(a["streams"]) <= len(names) + (1 if any(x.get("shifted") for x in a["streams"]) else 0)


@pytest.mark.parametrize("fam", list(rc.FAMILIES))
def test_chained_cases_still_reach_their_arms(fam):
    L = pyoracle.lib()
    names = pyoracle.track_arm_names()
    expect = {c["name"]: c["expect"] for c in sc.family(fam)["cases"]}
    for i, s in enumerate(sc.chained(fam)["streams"]):
        if s.get("shifted"):
            assert fam == "auto" and i > 0                   # the stream that is there for the ring alone (stream_tracker_cases.chained); the chain before it is checked
            continue
        c = sc.cfg(fam, 10)
        h = L.wsa_or_seg_new(ctypes.byref(c))
        count = lambda: np.array([L.wsa_or_track_arm_count(h, k) for k in range(len(names))])
        met = dict.fromkeys(expect, False)
        try:
            at = 0
            for name, lo, hi in s["where"]:
                for f in range(at, lo):
                    L.wsa_or_seg_push(h, np.ascontiguousarray(s["frames"][f]).ctypes.data)
                before = count()
                for f in range(lo, hi):
                    L.wsa_or_seg_push(h, np.ascontiguousarray(s["frames"][f]).ctypes.data)
                at = hi
                d = dict(zip(names, count() - before))
                met[name] = met[name] or all(d[k] >= v for k, v in expect[name].items())
        finally:
            L.wsa_or_seg_free(h)
        assert all(met.values()), (fam, i, [k for k, v in met.items() if not v])


def test_the_cut_arrangement_meets_what_it_was_searched_for():
    a = sc.cut()
    n = sc.boundary_classes(a, only=[0])
    assert n["cut"] >= 1 and n["before_first_accumulate"] >= 1 and n["closed_by_stop"] >= 1, n
    other = sc.boundary_classes(a, only=[1])
    assert other["cut"] == 0 and other["closed_by_stop"] == 0 and other["live"] > 50, other      # the neighbour is an ordinary chain
    g = sc.reference(a, 0, 10, gate=True)["gate"]
    assert max(fe - fb for _, _, fb, fe, *_ in g["segments"]) + a["F"] > a["ring"] - a["F"]          # its longest span is what the ring just held

"""The hand-built frames of tests/peak_cases.py against the REFERENCE's own frame loop (tests/golden/peaks_expected.json, made by
tests/golden/gen/make_peaks_golden.py): the oracle's scan equals the reference's candidate lists and n, p, h, d, g exactly, the plain restatement
tests/peak_ref.py equals the oracle's scan — candidates, sums and arm counts — on every case and on the random frames of the older unit test, every
case takes the arms it was built for, all cases together take every arm but the provably shut ones, the geometry model finds every edge of the
kernels' rounds, ring, list and words, and every modelled fault of the restatement changes the record of the case that aims at it.  No GPU: a case
that misses its arm fails here, before tests/test_gpu_peaks.py compares the kernels with the restatement."""
import json
import os

import numpy as np
import pytest

from oracle import pyoracle
from tests import peak_cases as pc
from tests import peak_ref
from tests.test_gpu_units import _peak_frames
from tests.util import GOLDEN

RANDOM_BANDS = (128, 96, 33, 1, 2, 3, 4, 31, 32, 64, 65, 127, 200, 256)          # the band counts of test_peak_scan_kernels_equal_the_reference_scan
SAME = ("cands", "p_i", "p_s", "n", "p", "h", "d", "g", "largest", "arms")

# the modelled faults (peak_ref.MUTANTS) and the case that aims at each
MUTANT_CASES = {
    "c_cleared_at_rise": "flat-counter-carried",
    "shrink_le": "shrink-threshold",
    "thr_floored": "shrink-threshold",
    "eos_in_largest": "end-of-spectrum",
    "tie_to_later": "largest",
    "R_no_a3": "predicates-at-word-edges",
    "F_no_a3": "predicates-at-word-edges",
    "creep_ge": "creep",
    "timeout_gt3": "flat-timeout-then-fall",
    "ps_high_early": "prefix-crossings",
    "g_with_e0": "prefix-crossings",
    "l_not_forced": "end-of-spectrum",
}


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "peaks_expected.json")))


def _floor(dB):
    return pyoracle.lib().wsa_or_pow(10.0, dB / 20)          # as the segmenter computes the fixed floor (ref @B25471)


@pytest.fixture(scope="module")
def scans():
    """{case: [restatement's scan of each frame at v = None]}"""
    return {c["name"]: [peak_ref.scan(f) for f in c["frames"]] for c in pc.CASES}


def _runs():
    return [(c, None) for c in pc.CASES] + [(pc.by_name(n), dB) for n, dBs in pc.FLOOR_RUNS.items() for dB in dBs]


def test_the_cases_are_the_ones_the_reference_was_run_on(golden):
    assert [(r["name"], r["voiced_min_dB"]) for r in golden["runs"]] == [(c["name"], -20.0 if dB is None else dB) for c, dB in _runs()]
    for (c, _), r in zip(_runs(), golden["runs"]):
        assert pc.digest(c) == r["digest"], c["name"]
    assert 200 <= sum(len(c["frames"]) for c in pc.CASES) <= 600


def test_oracle_scan_equals_the_reference(golden):
    frames = cands = 0
    for (c, dB), r in zip(_runs(), golden["runs"]):
        v = _floor(r["voiced_min_dB"])
        tri = bytes.fromhex(r["triples"])
        at = 0
        for k, f in enumerate(c["frames"]):
            n = r["counts"][k]
            ref = [tuple(tri[at + 3 * j:at + 3 * j + 3]) for j in range(n)]
            at += 3 * n
            got = pyoracle.scan_frame(f, v)
            assert [t[:3] for t in got["cands"]] == ref, (c["name"], k, dB)
            assert [got["n"], got["p"], got["h"], got["d"], got["g"]] == [float(x) for x in r["nphdg"][k]], (c["name"], k, dB)
            if dB is None:
                # the floor of 0.1 drops nothing but an end-of-spectrum candidate of amplitude 0: with every candidate kept the table is the same otherwise
                every = pyoracle.scan_frame(f, None)
                if (c["name"], k) in pc.REF_DROPS_ZERO:
                    assert every["cands"][:-1] == got["cands"] and every["cands"][-1][3] == 1 and f[every["cands"][-1][2]] == 0
                else:
                    assert every["cands"] == got["cands"], (c["name"], k)
            frames += 1; cands += n
        assert at == len(tri)
    assert frames > 300 and cands > 1000


def _same(a, b, where):
    for k in SAME:
        assert a[k] == b[k], where + (k, {x: (a[k][x], b[k][x]) for x in a[k] if a[k][x] != b[k][x]} if k == "arms" else (a[k], b[k]))


def test_the_restatement_equals_the_oracle_on_every_case(scans):
    assert pyoracle.peak_arm_names() == list(peak_ref.ARMS)
    for c in pc.CASES:
        for k, f in enumerate(c["frames"]):
            _same(scans[c["name"]][k], pyoracle.scan_frame(f, None), (c["name"], k))
    for name, dBs in pc.FLOOR_RUNS.items():
        for dB in dBs:
            for k, f in enumerate(pc.by_name(name)["frames"]):
                _same(peak_ref.scan(f, _floor(dB)), pyoracle.scan_frame(f, _floor(dB)), (name, k, dB))


@pytest.mark.parametrize("bands", RANDOM_BANDS)
def test_the_restatement_equals_the_oracle_on_the_random_frames(bands):
    spec = _peak_frames(np.random.default_rng(100 + bands), 64 * 5 + 17, bands)
    for k, f in enumerate(spec):
        _same(peak_ref.scan(f), pyoracle.scan_frame(f, None), (bands, k))
        if k % 8 == 0:
            _same(peak_ref.scan(f, 1000.0), pyoracle.scan_frame(f, 1000.0), (bands, k, "floor"))


def _case_arms(c, scans):
    arms = dict.fromkeys(peak_ref.ARMS, 0)
    for r in scans[c["name"]]:
        for k, v in r["arms"].items():
            arms[k] += v
    return arms


def test_every_case_takes_the_arms_it_was_built_for(scans):
    for c in pc.CASES:
        arms = _case_arms(c, scans)
        short = {k: (arms[k], v) for k, v in c["expect"].items() if arms[k] < v}
        assert not short, f"{c['name']}: arm: (taken, wanted) {short}"


def test_no_arm_is_left_out(scans):
    total = dict.fromkeys(peak_ref.ARMS, 0)
    for c in pc.CASES:
        for k, v in _case_arms(c, scans).items():
            total[k] += v
    for name, dBs in pc.FLOOR_RUNS.items():
        for dB in dBs:
            for f in pc.by_name(name)["frames"]:
                for k, v in peak_ref.scan(f, _floor(dB))["arms"].items():
                    total[k] += v
    assert set(peak_ref.UNREACHABLE) <= set(total)
    never = sorted(k for k, v in total.items() if v == 0)
    assert never == sorted(peak_ref.UNREACHABLE), never


def test_the_floor_runs_sit_on_the_floor(golden):
    """voiced_min_dB 20 and 40 are floors of exactly 10 and 100: candidates of amplitude v (refused), v + 1 (kept), 2 v (kept, not the largest), 2 v + 1"""
    c = pc.by_name("floor-edges")
    for dB, v in ((20.0, 10.0), (40.0, 100.0)):
        assert _floor(dB) == v
        arms = dict.fromkeys(peak_ref.ARMS, 0)
        for f in c["frames"]:
            r = peak_ref.scan(f, v)
            for k, x in r["arms"].items():
                arms[k] += x
            amps = [int(f[l]) for _, _, l, _ in r["cands"]]
            assert int(v) not in amps and int(v) + 1 in amps and 2 * int(v) in amps
        assert arms["floor_equal_refused"] >= 1 and arms["floor_below_refused"] >= 1 and arms["h_2v_not_above"] >= 1


def test_the_model_finds_every_geometry_arm():
    total = dict.fromkeys(pc.GEO_ARMS, 0)
    for c in pc.CASES:
        g = pc.case_geometry(c)
        short = [k for k in c["geo"] if not g[k]]
        assert not short, f"{c['name']}: geometry arms not taken: {short}"
        for k, v in g.items():
            total[k] += v
    assert not [k for k, v in total.items() if v == 0]


def test_every_modelled_fault_changes_the_record_of_its_case(scans):
    assert set(MUTANT_CASES) == set(peak_ref.MUTANTS)
    for m, name in MUTANT_CASES.items():
        c = pc.by_name(name)
        changed = [k for k, f in enumerate(c["frames"]) if peak_ref.record(peak_ref.scan(f, mutant=m)) != peak_ref.record(scans[name][k])]
        assert changed, f"fault {m} goes unnoticed by {name}"

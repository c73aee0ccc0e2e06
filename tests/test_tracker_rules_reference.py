"""The hand-built clips of tests/tracker_rule_cases.py against the REFERENCE's own accumulate_fm and finalize (tests/golden/tracker_rules_expected.json, made
by tests/golden/gen/make_tracker_rules_golden.py): the oracle's level-3 ranked tracks and its level-10 frames and syllables equal the reference's bit for bit,
every case takes the arms it was built for, all cases together take every arm the oracle counts but the ones argued unreachable, and every case stays inside
the limits of all the device tracker's tiers.  No GPU: a case that misses its arm fails here, before tests/test_gpu_tracker_rules.py compares the kernels
with the oracle."""
import json
import os
import struct

import pytest

from oracle import pyoracle
from tests import tracker_cases as tc
from tests import tracker_rule_cases as rc
from tests.util import GOLDEN, callbacks_equal


def decode(x, table):
    if isinstance(x, list):
        return [decode(y, table) for y in x]
    if isinstance(x, dict):
        return x["s"]
    return None if x is None else table[x]


@pytest.fixture(scope="module")
def golden():
    g = json.load(open(os.path.join(GOLDEN, "tracker_rules_expected.json")))
    g["table"] = [struct.unpack(">d", bytes.fromhex(h))[0] for h in g["values"]]
    return g


@pytest.fixture(scope="module")
def runs():
    return {c["name"]: {3: pyoracle.run_backend(rc.spectra(c), rc.cfg(c, 3)), 10: pyoracle.run_backend(rc.spectra(c), rc.cfg(c, 10), track=True)} for c in rc.CASES}


def test_the_table_keeps_its_form():
    assert len(rc.CASES) <= rc.MAX_CASES and len({c["name"] for c in rc.CASES}) == len(rc.CASES)
    for c in rc.CASES:
        s = rc.spectra(c)
        assert 0 < len(s) <= rc.MAX_FRAMES and s.dtype.name == "uint32" and s.shape[1] == c["bands"], c["name"]
        assert c["expect"] and all(isinstance(v, int) and v >= 1 for v in c["expect"].values()), c["name"]


def test_the_cases_are_the_ones_the_reference_was_run_on(golden):
    assert [c["name"] for c in golden["cases"]] == [c["name"] for c in rc.CASES]
    for c, g in zip(rc.CASES, golden["cases"]):
        assert rc.digest(c) == g["digest"], c["name"]


def test_oracle_tracks_frames_and_syllables_equal_the_reference(golden, runs):
    tracks = rows = 0
    for c, g in zip(rc.CASES, golden["cases"]):
        for level in (3, 10):
            r = runs[c["name"]][level]
            assert r["segments_ci"] == g["segments_ci"], (c["name"], level)
            ref = decode(g["callbacks_%d" % level], golden["table"])
            ok, why = callbacks_equal(level, ref, r["callbacks"], exact=True)
            assert ok, f"{c['name']} level {level}: {why}"
            if level == 3:
                tracks += sum(len(cb[2]) for cb in ref)
            else:
                rows += sum(len(f) for cb in ref for f in cb[3])
        assert runs[c["name"]][10]["syllables_ci"] == g["syllables_ci"], c["name"]
        assert len(g["segments_ci"]) >= 1, c["name"]
    assert tracks >= 4 * len(rc.CASES) and rows >= 5 * len(rc.CASES), (tracks, rows)      # (every case has a segment of five frames or more, hence a syllable)


def test_every_case_takes_the_arms_it_was_built_for(runs):
    for c in rc.CASES:
        arms = runs[c["name"]][10]["track"]["arms"]
        short = {k: (arms[k], v) for k, v in c["expect"].items() if arms[k] < v}
        assert not short, f"{c['name']}: arm: (taken, wanted) {short}"


def test_no_arm_is_left_out(runs):
    total = {k: 0 for k in pyoracle.track_arm_names()}
    for r in runs.values():
        for k, v in r[10]["track"]["arms"].items():
            total[k] += v
    assert set(rc.UNREACHABLE) <= set(total)
    never = sorted(k for k, v in total.items() if v == 0)
    assert never == sorted(rc.UNREACHABLE), never


def test_every_case_stays_inside_the_tiers_limits(runs):
    """at most 16 peaks a frame and 38 live tracks (four spans per wave) — 32 and 64 in the cases built to hold more than 16 or 32 live tracks, which must do so:
    no span of these cases goes on the redo list or makes the back end run again (those paths belong to tests/test_gpu_tracker_limits.py)"""
    for c in rc.CASES:
        load = runs[c["name"]][10]["load"]
        assert load == runs[c["name"]][3]["load"] and len(load) >= 1
        peaks, live = max(p for p, _ in load), max(l for _, l in load)
        if c["crowd"] is None:
            assert peaks <= tc.QUAD[0] and live <= tc.QUAD[1], (c["name"], load)
        else:
            assert peaks <= tc.PAIR[0] and c["crowd"] < live <= tc.PAIR[1], (c["name"], load)

"""The hand-built frames of tests/gate_cases.py against the REFERENCE's own frame loop (tests/golden/gate_expected.json, made by
tests/golden/gen/make_gate_golden.py): the oracle's segments and per-frame state equal the reference's bit for bit, every case takes the arms it
was built for, and all cases together take every arm the oracle counts.  No GPU: a case that misses its arm fails here, before
tests/test_gpu_gate.py compares the kernels with the oracle's record."""
import json
import os
import struct

import numpy as np
import pytest

from oracle import pyoracle
from tests import gate_cases as gc
from tests.util import GOLDEN


@pytest.fixture(scope="module")
def golden():
    g = json.load(open(os.path.join(GOLDEN, "gate_expected.json")))
    g["table"] = np.array([struct.unpack(">d", bytes.fromhex(h))[0] for h in g["values"]], np.float64)
    return g


@pytest.fixture(scope="module")
def runs():
    return {c["name"]: pyoracle.run_backend(gc.spectra(c), pyoracle.default_cfg(level=5, bands=c["bands"], **c["settings"]), trace=True, gate=True)
            for c in gc.CASES}


def test_the_cases_are_the_ones_the_reference_was_run_on(golden):
    assert [c["name"] for c in golden["cases"]] == [c["name"] for c in gc.CASES]
    for c, g in zip(gc.CASES, golden["cases"]):
        assert gc.digest(c) == g["digest"], c["name"]


def test_oracle_trace_and_segments_equal_the_reference(golden, runs):
    frames = 0
    for c, g in zip(gc.CASES, golden["cases"]):
        r = runs[c["name"]]
        assert r["segments_ci"] == g["segments_ci"], c["name"]
        ref = golden["table"][np.array(g["trace"], np.int64)].reshape(-1, 10)
        got = r["trace"]
        assert ref.shape == got.shape, c["name"]
        bad = np.argwhere(ref.view(np.uint64) != np.ascontiguousarray(got).view(np.uint64))
        assert len(bad) == 0, f"{c['name']}: first differing (frame, column) {bad[:3].tolist()}: reference {ref[bad[0][0]]} oracle {got[bad[0][0]]}"
        frames += len(ref)
    assert frames > 3000


def test_every_case_takes_the_arms_it_was_built_for(runs):
    for c in gc.CASES:
        arms = runs[c["name"]]["gate"]["arms"]
        short = {k: (arms[k], v) for k, v in c["expect"].items() if arms[k] < v}
        assert not short, f"{c['name']}: arm: (taken, wanted) {short}"


def test_no_arm_is_left_out(runs):
    total = {k: 0 for k in pyoracle.gate_arm_names()}
    for r in runs.values():
        for k, v in r["gate"]["arms"].items():
            total[k] += v
    assert set(gc.UNREACHABLE) <= set(total)
    never = sorted(k for k, v in total.items() if v == 0)
    assert never == sorted(gc.UNREACHABLE), never


def test_the_record_agrees_with_the_trace(runs):
    """the per-frame record and the segment spans are what the trace says: a frame's call files under c_ci before the frame unless a reset came first,
    v is the floor the frame before left, fl the floor of the trace row; a span ends where its segment was finalized and holds the segment's frames"""
    for c in gc.CASES:
        r = runs[c["name"]]
        g, tr = r["gate"], r["trace"]
        n = len(tr)
        assert len(g["called"]) == n
        if n == 0:
            continue
        assert np.array_equal(g["fl"], tr[:, 4])
        assert np.array_equal(g["v"][1:], tr[:-1, 4])
        for f in np.flatnonzero(g["called"]):
            assert tr[f, 0] == (0 if g["stale"][f] else g["t"][f])            # (a reset in front of the call leaves c_ci 0, the call files under the old one)
        for seg, ci in zip(g["segments"], r["segments_ci"]):
            start, ln, fb, fe, cci, ctx, fl = seg
            assert [start, ln] == ci and fb <= start + ln <= fe <= n and fb <= fe - ln


def test_densest_segmentation_stays_inside_the_segment_table(runs):
    """host_plan.hpp sizes a clip's segment table as frames / period + 2 with period = min_frames + 1 + floor(breaker)"""
    for name, s in gc.DENSE_SETTINGS.items():
        n = len(gc.spectra(gc.by_name(name)))
        breaker = s["pause_length"] / s["window_step"]
        period = int(s["min_seg_length"] // s["window_step"]) + 1 + int(breaker)
        nseg = len(runs[name]["segments_ci"])
        assert nseg == 24 and nseg <= n // period + 2, (name, nseg, n, period)

"""The cases of tests/tracker_cases.py, from the oracle alone (CPU): every case meets the condition its name states — read off the oracle's
per-segment load counters (oracle/backend.c, wsa_or_segment_load) —, gives exactly one segment and finite features at every level the GPU test
compares.  What tests/test_gpu_tracker_limits.py expects of the device (which tier declines which span, which batch reruns) are conditions on these
counters, never on the device's output."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import tracker_cases as tc


@pytest.fixture(scope="module")
def runs():
    out = {}
    for key, c in tc.CASES.items():
        spec = tc.case_clip(key)
        out[key] = (spec, {level: pyoracle.run_backend(spec, pyoracle.default_cfg(level=level, **tc.settings(c["family"]))) for level in (3, 10, 5, 13)})
    return out


def test_the_table_covers_both_sides_of_every_limit():
    keys = set(tc.CASES)
    assert {f"low-{t}" for t in tc.TARGETS} <= keys
    assert {f"high-{t}" for t in tc.HIGH_TARGETS} <= keys and {"live64", "live65", "live140", "live141", "peaks63"} <= set(tc.HIGH_TARGETS)
    assert {f"auto-{t}" for t in tc.AUTO_TARGETS} <= keys and {"live38", "live39", "live64", "live65"} <= set(tc.AUTO_TARGETS)
    # the edges are the device's: QUAD_AC / PAIR_AC / AC_FAST and the 16 / 32 lanes of a group (csrc/tracker.hip)
    assert tc.QUAD == (16, 38) and tc.PAIR == (32, 64) and tc.AC_FAST == 140 and tc.K_MAX == 63
    for lo, hi in (("live38", "live39"), ("peaks16", "peaks17"), ("live64", "live65"), ("peaks32", "peaks33"), ("live140", "live141")):
        which = 1 if lo.startswith("live") else 0
        (op_lo, x_lo), (op_hi, x_hi) = tc.TARGETS[lo][which], tc.TARGETS[hi][which]
        assert op_lo == op_hi == "==" and x_hi == x_lo + 1 and x_lo in tc.QUAD + tc.PAIR + (tc.AC_FAST,)


@pytest.mark.parametrize("key", list(tc.CASES))
def test_case_meets_its_condition_with_one_segment_and_finite_features(runs, key):
    c = tc.CASES[key]
    spec, by_level = runs[key]
    assert spec.dtype == np.uint32 and spec.shape == (1 + len(c["Ks"]) + tc.TAIL, tc.BANDS) and spec.shape[0] <= 60
    cond_peaks, cond_live = tc.TARGETS[c["target"]]
    for level, r in by_level.items():
        assert len(r["segments_ci"]) == 1 and r["flags"][0] >= 0, (key, level)
        peaks, live = r["load"][0]
        assert (peaks, live) == (c["peaks"], c["live"]), (key, level, peaks, live)          # the load does not depend on the level
        assert tc.meets(cond_peaks, peaks) and tc.meets(cond_live, live), (key, peaks, live)
        assert len(r["callbacks"]) == 1, (key, level)
    assert np.isfinite(by_level[5]["features"][0]).all()
    assert len(by_level[13]["features"][0]) >= 1 and all(np.isfinite(f).all() for f in by_level[13]["features"][0])
    assert len(by_level[10]["syllables_ci"][0]) >= 1 and np.isfinite(by_level[10]["formants"][0]).all()
    assert len(by_level[3]["tracks"][0]) >= 1
    if c["family"] == "high":
        assert int(spec.max()) >= 2 ** 31
        assert max(max(t[11]) for t in by_level[3]["tracks"][0]) >= 2 ** 31              # a ranked track carries such an amplitude
    if c["family"] == "auto":
        # the mid-span reset: the segment's span (what the counters cover) starts behind the first crowded frame
        tr = pyoracle.run_backend(spec, pyoracle.default_cfg(level=5, **tc.settings("auto")), trace=True)["trace"]
        assert tr[2, 1] == 1 and tr[1, 1] == 2 and tr[2, 4] > 1e4                         # c_started back to 0 -> 1 on the third frame, the floor lifted


def test_partner_clips_are_light_and_one_segment_long():
    for fam in tc.FAMILIES:
        for n in (8, 17, 39):
            spec = tc.partner(fam, n, n)
            assert spec.shape == (1 + n + tc.TAIL, tc.BANDS)
            r = pyoracle.run_backend(spec, pyoracle.default_cfg(level=5, **tc.settings(fam)))
            assert len(r["segments_ci"]) == 1 and r["load"][0][0] <= 6 and r["load"][0][1] <= tc.QUAD[1] // 2, (fam, n, r["load"])
            assert np.isfinite(r["features"][0]).all()


def test_the_counters_count_what_the_device_compares():
    """Spans whose load can be told without the counters: the start frame (6 peaks, 6 tracks at bins 21, 33 .. 81) and three crowded frames of the
    three levels.  Peaks of different levels cannot match (1000 x apart); a top of the first / second crowded frame (600, 1.0e6: within 1000 x of the
    start frame's 2000 and 40000) could continue a start-frame track, but only from less than 4 / 6 bins away (gap 1 / 2), and the seeds here are the
    first whose frames keep that distance; the third (1.7e9) is out of their reach.  So every accepted peak opens a
    track, level 3 has no track of two points to hand out, and after the fourth frame every track is less than 4 frames old:
    live = all accepted peaks, peaks = the largest accepted count of the trace."""
    cfg = tc.settings("low")
    for Ks in ([4, 4, 63], [5, 4, 30], [4, 5, 11]):
        for seed in range(2000):
            spec = tc.clip("low", seed, Ks)
            tops = [np.flatnonzero(spec[f][1::2] > spec[f][0::2]) * 2 + 1 for f in (1, 2)]
            if all(np.abs(t[:, None] - np.arange(21, 82, 12)[None, :]).min() >= w for t, w in zip(tops, (4, 6))):
                break
        else:
            raise AssertionError("no seed keeps the first two crowded frames clear of the start frame's tracks")
        r = pyoracle.run_backend(spec, pyoracle.default_cfg(level=5, **cfg), trace=True)
        n = r["trace"][:4, 5].astype(int)                        # accepted peaks per frame
        assert n[0] == 6 and all(K - 1 <= m <= K for m, K in zip(n[1:], Ks))          # (a frame's last top is accepted only on bin 127)
        assert pyoracle.run_backend(spec, pyoracle.default_cfg(level=3, **cfg))["tracks"][0] == []
        assert r["load"] == [[int(n.max()), int(n.sum())]], (Ks, seed, r["load"], n)

"""CPU: the dispatcher's restatement (tests/dispatch_ref.py) that K3's GPU test (tests/test_gpu_dispatch.py) compares the kernels with is itself
held to the reference here — (a) against the oracle's dispatcher pyoracle.callbacks() on every hand-built batch case, through the host's own
formatting (capi.rows_to_callbacks); (b) against what the reference recorded for the fixture clips that hold a dropped segment; (c) against the new
fixture tests/golden/dispatch_expected.json (make_dispatch_golden.py: clips with two drops, a drop first, a drop with two results behind it, found by a
seed search bounded at 20 000 seeds that stopped after 7 600, run through the reference under Node at levels 5, 13 and 11); (d) the cases notice every modelled one-line fault; (e) they reach
every arm.  The streams' ring form equals the launch-long lists everywhere but in the time columns of results whose entry the ring has lost: only in
the stream-lost-* cases, under 5 % of their rows."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import pyoracle
from tests import dispatch_cases as dc
from tests import dispatch_ref as dr
from tests.util import GOLDEN, callbacks_equal, load_backend_golden
from webspeechanalyzer_amd import capi

STREAMS = dc.stream_cases()
BATCHES = dict(dc.BATCH, **dc.TWINS, everything=dc.EVERYTHING, generated=dc.generated(129, 7))
for _clips in BATCHES.values():
    dc.tables([_clips], "shuffled")              # the rows get their place in a pool that is not in segment order (the `pool-order` fault reads it)


def _callbacks_of(rows, level, step, feats=None):
    """one clip's restated rows through the host's formatting"""
    meta = np.array([r[0] for r in rows], np.int32).reshape(-1, 8)
    feat = [(feats[r[1]] if feats is not None else dc.feature_bits(r[1]).view(np.float64)) for r in rows]
    payload = (lambda m, f: np.zeros((int(m[3]), 9))) if level == 10 else (lambda m, f: f)
    return capi.rows_to_callbacks(level, step, meta, feat, payload)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("name", list(BATCHES))
def test_batch_cases_equal_the_oracles_dispatcher(name):
    """(a) callback index, time pairs (numbers at 5 / 4, the reference's toFixed(3) strings at 13 / 10) and the order of the feature rows"""
    clips = BATCHES[name]
    checked = {13: 0, 10: 0, 5: 0, 4: 0}
    results = sum(1 for c in clips for sg in c if sg["flag"] >= 0)
    for level in (13, 10, 5, 4):
        cfg = pyoracle.default_cfg(level=level)
        ref = dr.batch(clips, level)
        for c, segs in enumerate(clips):
            if level in (5, 4) and any(sg["flag"] >= 0 and len(sg["rows"]) != 1 for sg in segs):
                assert name not in dc.TWINS                            # a level-5 / level-4 result is one row: the one-row twin of the case is compared
                continue
            out = dc.oracle_out(segs, level)
            if level in (10, 4):
                out["formants"] = [None if sg["flag"] < 0 else np.zeros((80, 9)) for sg in segs]
            want = pyoracle.callbacks(out, cfg)
            got = _callbacks_of(ref["rows"][c], level, cfg.window_step / 1e3)
            assert [w[0] for w in want] == [g[0] for g in got], (name, level, c)
            for w, g in zip(want, got):
                if level in (13, 10):
                    assert [list(x) for x in w[2]] == [list(x) for x in g[2]], (name, level, c, w[0])
                    assert len(w[3]) == len(g[3])
                else:
                    assert _same_bits(w[2], g[2]), (name, level, c, w[0])
                if level == 13:
                    assert all(_same_bits(a, b) for a, b in zip(w[3], g[3])), (name, level, c, w[0])
                if level == 5:
                    assert _same_bits(w[3], g[3]), (name, level, c, w[0])
            checked[level] += len(want)
    if name in dc.TWINS:                                                # the segment form: every result of the case against the oracle at 5 and 4
        assert checked[5] == checked[4] == checked[13] == results > 0, (name, checked, results)
    with_rows = sum(1 for c in clips for sg in c if sg["flag"] >= 0 and sg["rows"])
    assert checked[13] == checked[10] == with_rows, (name, checked, with_rows)


def _segments_of(out, level):
    """the oracle's run of a clip as a restatement case + the rows' feature vectors by id"""
    segs, feats = [], {}
    for i, (u, f) in enumerate(zip(out["segments_ci"], out["flags"])):
        rows = []
        if f >= 0:
            if level == 5:
                rows = [dict(id=len(feats), w=(0, 0, 0, 0, 0), pos=-1)]
                feats[len(feats)] = out["features"][i]
            else:
                for ci, ft in zip(out["syllables_ci"][i], out["features"][i]):
                    rows.append(dict(id=len(feats), w=(ci[0], ci[1], 0, 0, 0), pos=-1))
                    feats[len(feats)] = ft
        segs.append(dict(start=u[0], len=u[1], flag=f, rows=rows))
    return segs, feats


def _restated_callbacks(spec, cfg, level):
    out = pyoracle.run_backend(spec, cfg)
    segs, feats = _segments_of(out, level)
    return out, _callbacks_of(dr.batch([segs], level)["rows"][0], level, cfg.window_step / 1e3, feats)


def test_fixture_clips_with_a_drop_equal_the_recorded_callbacks():
    """(b) backend_expected.json and fuzz_expected.json: wherever a clip holds a dropped segment, the restatement gives the reference's callbacks"""
    spectra, cases = load_backend_golden()
    fuzz = json.load(open(os.path.join(GOLDEN, "fuzz_expected.json")))
    spectra.update(np.load(os.path.join(GOLDEN, "fuzz_spectra.npz")))
    seen = {5: 0, 13: 0}
    for case in cases + [dict(c, settings=fuzz["settings"]) for c in fuzz["cases"]]:
        if case["level"] not in (5, 13):
            continue
        s = case["settings"]
        cfg = pyoracle.default_cfg(level=case["level"], bands=int(spectra[case["key"]].shape[1]), window_step=s["window_step"], pause_length=s["pause_length"],
                                   min_seg_length=s["min_seg_length"], auto_noise_gate=s["auto_noise_gate"], voiced_max_dB=s["voiced_max_dB"], voiced_min_dB=s["voiced_min_dB"])
        out, got = _restated_callbacks(spectra[case["key"]], cfg, case["level"])
        if not any(f < 0 for f in out["flags"]):
            continue
        ok, why = callbacks_equal(case["level"], case["callbacks"], got, exact=True)
        assert ok, (case["key"], case["level"], why)
        seen[case["level"]] += 1
    assert seen == SEEN_WITH_A_DROP, seen


# what the two fixture files hold today: one clip (s8_f400) with a dropped segment, at either level; at 13 its two results have no syllables
SEEN_WITH_A_DROP = {5: 1, 13: 1}


def _kinds(flags):
    drops = [i for i, f in enumerate(flags) if f < 0]
    k = set()
    if len(drops) >= 2:
        k.add("two-drops")
    if drops and drops[0] == 0 and len(flags) > len(drops):
        k.add("drop-first")
    if drops and sum(1 for f in flags[drops[0] + 1:] if f >= 0) >= 2:
        k.add("drop-two-results")
    return k


def test_more_than_one_drop_against_the_reference_fixture():
    """(c) the clips make_dispatch_golden.py's search found (bounded at 20 000 seeds of 400 frames; it stopped after 7 600, the set complete): two drops in one clip, a drop as the first segment,
    a drop with two results behind it — the oracle AND the restatement against what the reference returned, bit for bit"""
    spectra = np.load(os.path.join(GOLDEN, "dispatch_spectra.npz"))
    d = json.load(open(os.path.join(GOLDEN, "dispatch_expected.json")))
    assert d["search"]["seeds"] == [0, 20000] and d["search"]["frames"] == 400 and d["search"]["looked"] == 7600
    assert set(d["search"]["found"]) == {"two-drops", "drop-first", "drop-two-results"}
    kinds = set()
    for c in d["cases"]:
        cfg = pyoracle.default_cfg(level=c["level"])
        out = pyoracle.run_backend(spectra[c["key"]], cfg)
        assert out["segments_ci"] == c["segments_ci"], c["key"]
        assert set(c["kinds"]) <= _kinds(out["flags"]), (c["key"], out["flags"])
        kinds |= set(c["kinds"])
        ok, why = callbacks_equal(c["level"], c["callbacks"], out["callbacks"], exact=True)
        assert ok, (c["key"], c["level"], why)
        if c["level"] in (5, 13):
            _, got = _restated_callbacks(spectra[c["key"]], cfg, c["level"])
            ok, why = callbacks_equal(c["level"], c["callbacks"], got, exact=True)
            assert ok, (c["key"], c["level"], why)
            assert len(c["callbacks"]) < len(c["segments_ci"])
    assert kinds == {"two-drops", "drop-first", "drop-two-results"}
    assert sorted({c["level"] for c in d["cases"]}) == [5, 11, 13]


def _strip(steps, lost_columns):
    """step tables for comparison: the time columns of lost rows blanked where the rule allows leaving them out"""
    out = []
    for t in steps:
        rows = [[(m[:2] + (None, None) + m[4:] if lost_columns and (s, i) in t["lost"] else m, rid) for i, (m, rid, _) in enumerate(clip)] for s, clip in enumerate(t["rows"])]
        out.append(dict(rows=rows, row_off=t["row_off"], seg_off=t["seg_off"], seg_out=t["seg_out"], totals=t["totals"], lost=t["lost"], lost_flag=t["lost_flag"], carry=t["carry"]))
    return out


@pytest.mark.parametrize("level", dc.LEVELS)
def test_the_ring_form_equals_the_launch_long_lists(level):
    """the lost rows' time columns are the one thing left out: only in stream-lost-*, under 5 % of those cases' rows, nothing anywhere else"""
    left_out = rows_there = 0
    cases = dict(STREAMS, counts65=dc.stream_counts_case(65, 3))
    for name, c in cases.items():
        a, b = dr.streams(c["steps"], c["n"], level), dr.streams_carry(c["steps"], c["n"], level)
        assert _strip(a, True) == _strip(b, True), name
        lost = sum(len(t["lost"]) for t in a)
        if not name.startswith("stream-lost-"):
            assert lost == 0 and _strip(a, False) == _strip(b, False), name
        else:
            left_out += lost
            rows_there += sum(len(clip) for t in a for clip in t["rows"])
    flags = {name: [t["lost_flag"] for t in dr.streams(c["steps"], c["n"], level)] for name, c in STREAMS.items() if name.startswith("stream-lost-")}
    assert flags == {"stream-lost-32": [False, False], "stream-lost-33": [False, True], "stream-lost-34": [False, True], "stream-lost-33-empty": [False, True]}
    empty = STREAMS["stream-lost-33-empty"]                              # a lost result without rows: nothing left out, the flag comes all the same, in both forms
    assert [len(t["lost"]) for t in dr.streams(empty["steps"], empty["n"], level)] == [0, 0]
    assert [t["lost_flag"] for t in dr.streams_carry(empty["steps"], empty["n"], level)] == [False, True]
    assert 0 < left_out and left_out / rows_there < 0.05, (left_out, rows_there)


def _concat(steps, stream=0):
    rows = [(m[1:], rid) for t in steps for (m, rid, _) in t["rows"][stream]]
    segs = [s[1:] for t in steps for s in t["seg_out"] if s[0] == stream]
    return rows, segs


@pytest.mark.parametrize("level", dc.LEVELS)
def test_one_launch_dealt_four_ways_gives_the_batch_tables(level):
    b = dc.Builder()
    want = dr.batch([b.finish(dc.LAUNCH)], level)
    want = ([(m[1:], rid) for (m, rid, _) in want["rows"][0]], [s[1:] for s in want["seg_out"]])
    for how in ("all", "each", "gappy", "halves"):
        c = STREAMS["deal-" + how]
        assert _concat(dr.streams(c["steps"], 1, level)) == want, how
        assert _concat(dr.streams_carry(c["steps"], 1, level)) == want, how
    assert max(len(t["segs"][0]) for t in STREAMS["deal-all"]["steps"]) > dr.CARRY_HIST


def test_the_cases_notice_every_modelled_fault():
    """(d) each one-line fault of the restatement changes what some named case expects"""
    noticed = {}
    for fault in dr.LIST_FAULTS:
        for level in dc.LEVELS:
            for name, clips in BATCHES.items():
                if dr.batch(clips, level, fault) != dr.batch(clips, level):
                    noticed.setdefault("list:" + fault, f"{name} L{level}")
            for name, c in STREAMS.items():
                if dr.streams(c["steps"], c["n"], level, fault) != dr.streams(c["steps"], c["n"], level):
                    noticed.setdefault("list:" + fault, f"{name} L{level}")
    for fault in dr.CARRY_FAULTS:
        for name, c in STREAMS.items():
            if dr.streams_carry(c["steps"], c["n"], 13, fault) != dr.streams_carry(c["steps"], c["n"], 13):
                noticed.setdefault("ring:" + fault, name)
    assert set(noticed) == {"list:" + f for f in dr.LIST_FAULTS} | {"ring:" + f for f in dr.CARRY_FAULTS}, noticed
    # the faults the issue names, by the case that is there for them
    by = lambda fault, level, name: dr.batch(BATCHES[name], level, fault) != dr.batch(BATCHES[name], level)
    assert by("own-entry", 5, "drop-first") and by("own-entry", 5, "two-adjacent-drops") and not by("own-entry", 5, "all-reported")
    assert by("si-skips-empty", 13, "zero-row-before-drop") and by("si-skips-empty", 13, "zero-row-alone") is False
    assert by("dropped-rows-counted", 5, "dropped-with-rows") and by("syllable-no-start", 13, "all-reported") and not by("syllable-no-start", 5, "all-reported")
    ring = lambda fault, name: dr.streams_carry(STREAMS[name]["steps"], STREAMS[name]["n"], 13, fault) != dr.streams_carry(STREAMS[name]["steps"], STREAMS[name]["n"], 13)
    assert ring("mod-31", "wrapped-slot") and ring("history-always", "straddle") and ring("carry-across-start", "restart")
    assert ring("lost-ge", "stream-lost-32")                  # 32 outstanding drops: the oldest entry is still the history's last


def test_every_arm_is_counted_on_both_sides():
    """(e)"""
    dr.ARMS.clear()
    for level in dc.LEVELS:
        for clips in BATCHES.values():
            dr.batch(clips, level)
        for c in STREAMS.values():
            dr.streams(c["steps"], c["n"], level)
    zero = [a for a in dr.ARM_NAMES if dr.ARMS[a] == 0]
    assert not zero, zero
    assert set(dr.ARMS) <= set(dr.ARM_NAMES)


def test_the_long_clips_spans_sit_on_the_bucket_clamp():
    """the span order's clips (tests/test_gpu_dispatch.py) are cut from designed_clip("long_voiced", n): by the oracle's own span record — frames between
    the resets that bound the span, SEG_FEND - SEG_FBEGIN — they are 2046, 2047, 2048 and 2580 frames, one either side of the last bucket and two in it"""
    sys.path.insert(0, os.path.join(GOLDEN, "gen"))
    from synth_spectra import designed_clip
    from tests import gate_cases as gc
    st = gc.by_name("densest-int")["settings"]
    for span, n in dc.LONG_FRAMES.items():
        out = pyoracle.run_backend(designed_clip("long_voiced", n), pyoracle.default_cfg(level=5, **st), gate=True)
        segs = out["gate"]["segments"]
        assert len(segs) == 1 and segs[0][3] - segs[0][2] == span, (n, segs)
    assert sorted(dc.LONG_FRAMES) == [2046, 2047, 2048, 2580]

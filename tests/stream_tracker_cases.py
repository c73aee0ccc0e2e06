"""Arrangements of the hand-built tracker clips as lock-step streams (test helper): no new spectra, only where the step boundaries fall.  The clips are those of
tests/tracker_rule_cases.py (seven settings families, every rule of accumulate_fm and finalize on its boundary) and tests/tracker_cases.py (crowded spans: up
to 63 peaks per frame and 177 live tracks); an arrangement hands them to the stream form of the tracker (csrc/tracker.hip stream_body, csrc/tracker_one.hpp
track_stream) through the test entry wsa_debug_stream_step_backend, which feeds a step's u32 frames past the front end.

Families: the rule families under their own names (f1, f10, f100, frac, f1e8, auto, b200) and the crowded ones as lim-low, lim-high, lim-auto.

An arrangement is a list of streams of one stream object; a stream is its frames, the frames it gets in each step (`counts`; the stream is active from step 0
to its last count, START on the first step, STOP on the last, inactive afterwards) and where its cases lie in it:
  alone-F   F in 1, 2, 3, 7, 64: every case of the family a stream, F frames per step (F = 1: a boundary behind every frame; F = 64: a whole clip in one step)
  ragged    the same streams, per-step counts drawn from a seeded generator in 0 .. 5, zeros included
  chained   the family's cases one after the other as one long clip per stream (every clip ends in a pause that finalizes and resets, so the concatenation is
            a valid clip; a closing run of zeros longer than the pause is shortened to it, so that every case starts under the filing index 0 it was built
            for), 7 frames per step, max_span_frames 66: the smallest ring stream_ring_frames gives (128).  Stream s starts with another case; the
            rotations are chosen (greedily, as few as cover) so that every case has a span that straddles the ring's end in some stream.  A family whose
            cases are shorter in all than three rings goes round them again.
  cut       (f1) two streams of 5 frames per step and a ring of 128: a chained stream whose closing pauses are shortened to two frames, so that its segments
            run on for more than the ring holds and gate.hip cuts one (modelled by pyoracle.run_backend(cuts=...) as tests/test_gpu_gate.py does), and whose
            last pause is dropped: STOP closes its last segment; next to it an ordinary chained stream, which must not notice.  Step size, pause and rotation
            were searched (search_cut) so that the cut falls right before a lone unvoiced frame: the cut-off span's successor gets its first accumulate
            call only behind a step boundary.

boundary_classes() counts, from the oracle's gate record and tracker table record alone, how often the step boundaries of an arrangement fall on each kind of
carried state (tests/test_stream_tracker_reference.py asserts every class occurs)."""
import ctypes

import numpy as np

from oracle import pyoracle
from tests import tracker_cases as tc
from tests import tracker_rule_cases as rc

ALONE_F = (1, 2, 3, 7, 64)
RAGGED_F, RAGGED_SEED = 5, 20
CHAIN_F, CHAIN_MAX_SPAN, CHAIN_RING = 7, 66, 128
ACTIVE, START, STOP = 1, 2, 4                     # include/wsa.h WSA_STREAM_*

FAMILY_NAMES = list(rc.FAMILIES) + ["lim-" + f for f in tc.FAMILIES]

# the boundary class no arrangement can reach, with its reason (as tracker_rule_cases.UNREACHABLE)
UNREACHABLE = {
    "finalize_nothing_accumulated": "finalize needs c_started >= 2 (oracle/backend.c finalize(), ref @B27190); every reset leaves c_started at -1, 0 or 1 and only a frame "
                                    "that calls accumulate_fm raises it, so a finalized span holds an accumulate call behind its reset: track_stream's "
                                    "`SEG_FBEGIN != my_span` before a finalize is a guard the gate cannot trigger",
}


def stream_ring_frames(F, max_span):
    """csrc/host_plan.hpp stream_ring_frames"""
    want = max_span if max_span else 1024
    want = max(want, 2 * F + 64)
    ring = 64
    while ring < want + F:
        ring <<= 1
    return ring


_FAM = {}


def family(name):
    """dict(settings, bands, cases [dict(name, spectra, expect)]) — expect: the oracle arm counters a rule case aims at (None for the crowded ones)"""
    if name not in _FAM:
        if name.startswith("lim-"):
            fam = name[4:]
            cases = [dict(name=k, spectra=tc.case_clip(k), expect=None) for k, c in tc.CASES.items() if c["family"] == fam]
            _FAM[name] = dict(settings=tc.settings(fam), bands=tc.BANDS, cases=cases)
        else:
            cs = [c for c in rc.CASES if c["family"] == name]
            _FAM[name] = dict(settings=dict(rc.FAMILIES[name]["settings"]), bands=rc.FAMILIES[name]["bands"],
                              cases=[dict(name=c["name"], spectra=rc.spectra(c), expect=c["expect"]) for c in cs])
    return _FAM[name]


def cfg(fam, level):
    f = family(fam)
    return pyoracle.default_cfg(level=level, bands=f["bands"], **f["settings"])


def _counts_fixed(n, F):
    return [F] * (n // F) + ([n % F] if n % F else [])


def _counts_ragged(n, F, rng):
    while True:                                              # (drawn again until the stream has a step of no frames)
        out, left = [], n
        while left:
            c = min(int(rng.integers(0, F + 1)), left)
            out.append(c)
            left -= c
        if 0 in out or n < 2:
            return out                                               # (ends on a step with frames: STOP goes with the stream's last frames)


def _stream(cases, counts_of, pause=None, drop_last_pause=False):
    """the cases' frames one after the other; pause: every clip's closing run of zero frames shortened to that many (where it is longer)"""
    parts, where, at = [], [], 0
    for k, c in enumerate(cases):
        s = c["spectra"]
        if pause is not None:
            tail = 0
            while tail < len(s) and not s[len(s) - 1 - tail].any():
                tail += 1
            s = s[:len(s) - tail + (0 if drop_last_pause and k == len(cases) - 1 else min(pause, tail))]
        parts.append(s)
        where.append((c["name"], at, at + len(s)))
        at += len(s)
    frames = np.concatenate(parts, axis=0)
    return dict(frames=frames, counts=counts_of(len(frames)), where=where)


def _arrangement(name, fam, F, max_span, streams, kind):
    f = family(fam)
    assert all(sum(s["counts"]) == len(s["frames"]) and max(s["counts"]) <= F for s in streams)
    return dict(name=name, family=fam, F=F, max_span=max_span, ring=stream_ring_frames(F, max_span), settings=f["settings"], bands=f["bands"], streams=streams, kind=kind)


def alone(fam, F):
    return _arrangement("alone-%d" % F, fam, F, 1024, [_stream([c], lambda n: _counts_fixed(n, F)) for c in family(fam)["cases"]], "alone")


def ragged(fam):
    rng = np.random.default_rng(RAGGED_SEED)
    return _arrangement("ragged", fam, RAGGED_F, 1024, [_stream([c], lambda n: _counts_ragged(n, RAGGED_F, rng)) for c in family(fam)["cases"]], "alone")


def _rotated(cases, r, min_frames):
    order = cases[r:] + cases[:r]
    out, n = [], 0
    while not out or n < min_frames:
        out += order
        n += sum(len(c["spectra"]) for c in order)
    return out


def oracle_run(fam, stream, level=10, cut_F=None, ring=None, **kw):
    """the oracle's run of a stream's frames; cut_F / ring: cut where gate.hip's stream kernel does (tests/test_gpu_gate.py _oracle_with_ring_cuts)"""
    cuts = ()
    if cut_F is not None:
        cuts = stream.get("cuts")
        if cuts is None:
            L = pyoracle.lib()
            c = cfg(fam, 10)
            h = L.wsa_or_seg_new(ctypes.byref(c))
            st = (ctypes.c_double * 12)()
            cuts = []
            try:
                for f, e in enumerate(stream["frames"]):
                    L.wsa_or_seg_push(h, np.ascontiguousarray(e).ctypes.data)
                    L.wsa_or_gate_state(h, st)
                    if st[3] >= 0 and f + 1 - st[11] + cut_F > ring:
                        L.wsa_or_seg_cut(h)
                        cuts.append(f)
            finally:
                L.wsa_or_seg_free(h)
            stream["cuts"] = cuts
    return pyoracle.run_backend(stream["frames"], cfg(fam, level), cuts=cuts, **kw)


def _straddlers(fam, stream):
    """names of the cases one of whose spans holds a frame f > its first with f & (ring - 1) == 0"""
    g = oracle_run(fam, stream, gate=True)["gate"]
    out = set()
    for seg in g["segments"]:
        fb, fe = seg[2], seg[3]
        if (fe - 1) // CHAIN_RING > fb // CHAIN_RING:
            out |= {name for name, lo, hi in stream["where"] if lo <= fb < hi}
    return out


_CHAINED = {}


def chained(fam):
    if fam in _CHAINED:
        return _CHAINED[fam]
    cases = family(fam)["cases"]
    names = {c["name"] for c in cases}
    cand = []
    for r in range(len(cases)):
        s = _stream(_rotated(cases, r, 3 * CHAIN_RING), lambda n: _counts_fixed(n, CHAIN_F), pause=rc.PAUSE)
        cand.append((r, s, _straddlers(fam, s)))
    # where no rotation puts a case across the ring's end (one short case going round: every pass but the first meets the automatic gate's carried state and
    # starts no segment) the chain is shifted by leading frames of silence, an idle stretch before the first case.  That stream (`shifted`) is there for the
    # ring alone: its first case starts under the filing index the silence ran up, not the 0 it was built for, so the unshifted chain stays next to it.
    shift = 0
    while set().union(*[c[2] for c in cand]) != names and shift < CHAIN_RING:
        shift += 1
        for r in range(len(cases)):
            s = _stream(_rotated(cases, r, 3 * CHAIN_RING), lambda n: _counts_fixed(n, CHAIN_F), pause=rc.PAUSE)
            s["frames"] = np.concatenate([np.zeros((shift, s["frames"].shape[1]), np.uint32), s["frames"]], axis=0)
            s["where"] = [(nm, lo + shift, hi + shift) for nm, lo, hi in s["where"]]
            s["counts"] = _counts_fixed(len(s["frames"]), CHAIN_F)
            s["shifted"] = shift
            cand.append((r, s, _straddlers(fam, s)))
    assert set().union(*[c[2] for c in cand]) == names, (fam, sorted(names - set().union(*[c[2] for c in cand])))
    chosen, covered = [], set()
    if shift:
        chosen.append(cand[0][1])                           # the unshifted chain: every case under the filing index it was built for
        covered |= cand[0][2]
    while covered != names:                                 # greedy cover, the lowest rotation first on ties
        r, s, got = max(cand, key=lambda c: len(c[2] - covered))
        chosen.append(s)
        covered |= got
    _CHAINED[fam] = _arrangement("chained", fam, CHAIN_F, CHAIN_MAX_SPAN, chosen, "chained")
    assert _CHAINED[fam]["ring"] == CHAIN_RING
    return _CHAINED[fam]


def _cut_arrangement(fam, F, pause, r):
    cases = family(fam)["cases"]
    long_ = _stream(_rotated(cases, r, 0), lambda n: _counts_fixed(n, F), pause=pause, drop_last_pause=True)
    neighbour = _stream(_rotated(cases, 1, 0), lambda n: _counts_fixed(n, F), pause=rc.PAUSE)
    a = _arrangement("cut", fam, F, CHAIN_MAX_SPAN, [long_, neighbour], "cut")
    a["cut_streams"] = [0]
    assert a["ring"] == CHAIN_RING
    return a


def _cut_meets(a):
    n = boundary_classes(a, only=[0])
    return n["cut"] >= 1 and n["before_first_accumulate"] >= 1 and n["closed_by_stop"] >= 1


def search_cut(fam="f1"):
    """the search that found CUT: the first (frames per step, pause, rotation) whose cut falls right before a lone unvoiced frame, so that the new span's
    first accumulate call comes a step boundary later (the cut falls behind frame f when f + 1 - span begin + F > ring: F moves it frame by frame)"""
    for F in (7, 6, 5, 4, 3, 2, 1, 8, 9, 10, 11, 12, 13):
        for pause in (1, 2, 3):
            for r in range(len(family(fam)["cases"])):
                if _cut_meets(_cut_arrangement(fam, F, pause, r)):
                    return dict(F=F, pause=pause, rotation=r)
    return None


CUT = dict(F=5, pause=2, rotation=19)              # search_cut("f1"), hard-coded; tests/test_stream_tracker_reference.py asserts that it still meets its conditions
_CUT = {}


def cut(fam="f1"):
    if fam not in _CUT:
        _CUT[fam] = _cut_arrangement(fam, CUT["F"], CUT["pause"], CUT["rotation"])
    return _CUT[fam]


def arrangements(fam):
    out = [alone(fam, F) for F in ALONE_F] + [ragged(fam), chained(fam)]
    if fam == "f1":
        out.append(cut(fam))
    return out


def n_steps(arr):
    return max(len(s["counts"]) for s in arr["streams"])


def steps(arr):
    """per step (n_frames [n] u32, ctl [n] u8, frames [n, F, bands] u32)"""
    n, F = len(arr["streams"]), arr["F"]
    at = [0] * n
    for k in range(n_steps(arr)):
        nfr, ctl, fr = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros((n, F, arr["bands"]), np.uint32)
        for i, s in enumerate(arr["streams"]):
            if k >= len(s["counts"]):
                continue
            c = s["counts"][k]
            nfr[i] = c
            ctl[i] = ACTIVE | (START if k == 0 else 0) | (STOP if k == len(s["counts"]) - 1 else 0)
            fr[i, :c] = s["frames"][at[i]:at[i] + c]
            at[i] += c
        yield nfr, ctl, fr


def reference(arr, i, level, **kw):
    """the oracle's run of stream i of the arrangement (with the ring's cuts where the arrangement has them)"""
    if i in arr.get("cut_streams", ()):
        return oracle_run(arr["family"], arr["streams"][i], level, cut_F=arr["F"], ring=arr["ring"], **kw)
    return oracle_run(arr["family"], arr["streams"][i], level, **kw)


CLASSES = ("live", "live_over_64", "live_over_128", "dead_in_table", "stale_set", "after_last_accumulate", "behind_finalize", "before_first_accumulate",
           "step_closes_two", "step_closes_and_starts", "closed_by_stop", "finalize_nothing_accumulated", "gate_reset_in_step", "zero_step_in_span",
           "ring_straddled", "cut")


def boundary_classes(arr, only=None):
    """how often the arrangement's step boundaries (and steps) fall into each class, from the oracle alone (only: these streams)"""
    n = dict.fromkeys(CLASSES, 0)
    for i, s in enumerate(arr["streams"]):
        if only is not None and i not in only:
            continue
        r = reference(arr, i, 10, trace=True, gate=True, track=True)
        g, T, cci = r["gate"], r["track"]["frames"], r["trace"][:, 0]
        N = len(s["frames"])
        segs = [(seg[2], seg[3]) for seg in g["segments"]]              # spans [fb, fe): finalized right behind frame fe - 1
        called = g["called"]
        first = {fb: next((f for f in range(fb, fe) if called[f]), None) for fb, fe in segs}
        last = {fb: next((f for f in range(fe - 1, fb - 1, -1) if called[f]), None) for fb, fe in segs}
        n["finalize_nothing_accumulated"] += sum(1 for fb, _ in segs if first[fb] is None)
        n["closed_by_stop"] += g["arms"]["fin_truncate_open"]
        n["cut"] += g["arms"]["ring_cut"]
        n["gate_reset_in_step"] += int(T[:, 4].sum())
        if arr["kind"] != "alone":
            n["ring_straddled"] += sum(1 for fb, fe in segs if (fe - 1) // arr["ring"] > fb // arr["ring"])
        ends = np.cumsum(s["counts"])
        lo = 0
        for k, b in enumerate(ends):                                    # step k holds the frames [lo, b); the boundary behind it is b
            closed = [sg for sg in segs if lo < sg[1] <= b]
            n["step_closes_two"] += len(closed) >= 2
            n["step_closes_and_starts"] += any(any(fb2 >= fe and fb2 < b for fb2, _ in segs) for _, fe in closed)
            lo = b
            if b == 0 or b >= N:
                continue                                                # nothing is carried out of the last step, or before the first frame
            t = T[b - 1]
            n["live"] += t[0] > 0
            n["live_over_64"] += t[0] > 64
            n["live_over_128"] += t[0] > 128
            n["dead_in_table"] += t[0] > 0 and cci[b - 1] + 1 - t[1] >= 4
            n["stale_set"] += t[2] == 1
            n["after_last_accumulate"] += any(last[fb] is not None and last[fb] < b < fe for fb, fe in segs)
            n["behind_finalize"] += any(fe == b for _, fe in segs)
            n["before_first_accumulate"] += any(first[fb] is not None and fb < b <= first[fb] for fb, fe in segs)
            n["zero_step_in_span"] += s["counts"][k] == 0 and t[0] > 0
    return {k: int(v) for k, v in n.items()}


if __name__ == "__main__":
    print("CUT =", search_cut("f1"))
    for fam in FAMILY_NAMES:
        for a in arrangements(fam):
            print("%-8s %-8s %2d streams %3d steps %s" % (fam, a["name"], len(a["streams"]), n_steps(a), {k: v for k, v in boundary_classes(a).items() if v}))

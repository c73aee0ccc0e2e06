"""Hand-built u32 frames for the peak scan (csrc/peaks.hip, K1b: peaks_kernel<32>, peaks_kernel<16>, peaks_wave_kernel) (test helper): every case
aims one rule of the reference's scan, or one edge of the kernels' geometry, at its boundary and says so as arm counters that must be non-zero
(`expect`).  Scan arms are counted by tests/peak_ref.py and, under the same names, by the oracle (oracle/backend.c PEAK_ARMS); geometry arms by
geometry() below, a model that works from the restatement's candidates and the kernels' documented constants alone — rounds of PK_W = 32 or 16 bins,
an LDS ring of 2 PK_W bins, a candidate list of 8 PK_W entries, the wave kernel's two 64-bit words — and from no output of any kernel.

The bytes come from integer arithmetic only (digest(), pinned in tests/golden/peaks_expected.json next to what the REFERENCE made of them).

Frames are built from
  hump()   a baseline, a strictly rising left shoulder, the top, a strictly falling right shoulder and three flat bins that close the candidate;
  quad()   four values e[a - 3 .. a] on a flat background: one rising / falling test at bin a with chosen predecessors;
  cross()  e[0] chosen so that the prefix sum reaches 2^32 exactly on a chosen bin (e[0] is compared with e[1 .. 3] only; it is kept at or above them,
           so bin 1 .. 3 at most fall while idle).
All band counts are accepted by the reference's configure (it refuses only 0), so every case is pinned through the reference; frames whose end-of-
spectrum candidate has amplitude 0 are the one place where the reference's list at a floor of 0.1 is shorter than the device's table (REF_DROPS_ZERO)."""
import hashlib

import numpy as np

from tests import peak_ref

U32 = 4294967295
W_LANE = (32, 16)                 # PK_W of peaks_kernel<32> / <16>; ring = 2 W bins, list = 8 W entries
EDGES = (16, 32, 64, 96)          # first bins of a round: of both lane kernels (32, 64, 96), of <16> alone (16), of the wave kernel's second word (64)
CARRY_BINS = (16, 32, 33, 34, 64, 65, 66)

CASES = []


def case(name, bands, expect, geo=()):
    def deco(fn):
        fr = [np.asarray(f, np.int64) for f in fn()]
        assert fr and all(f.shape == (bands,) and f.min() >= 0 and f.max() <= U32 for f in fr), name
        CASES.append(dict(name=name, bands=bands, expect=dict(expect), geo=tuple(geo), frames=np.stack(fr).astype(np.uint32)))
        return fn
    return deco


def digest(c):
    return hashlib.sha256(repr((c["name"], c["bands"], c["frames"].shape)).encode() + c["frames"].tobytes()).hexdigest()


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def groups():
    """{bands: [(case name, frame index, frame)]} in the order of CASES"""
    out = {}
    for c in CASES:
        out.setdefault(c["bands"], []).extend((c["name"], k, f) for k, f in enumerate(c["frames"]))
    return out


# ------------------------------------------------------------------------------------------------------------------ builders
def flat(bands, base=0):
    return np.full(bands, base, np.int64)


def hump(e, at, left, top, right, tail=3):
    """left shoulder from bin `at` (strictly rising, above the background), the top, the right shoulder (strictly falling), `tail` bins equal to the last"""
    vals = list(left) + [top] + list(right)
    assert all(x < y for x, y in zip(left, list(left[1:]) + [top])) and all(x > y for x, y in zip([top] + list(right), right)), vals
    vals += [vals[-1]] * tail
    assert at + len(vals) <= len(e)
    e[at:at + len(vals)] = vals
    return at + len(left)                                  # the top's bin


def quad(bands, a, q):
    """background q[0] up to bin a - 3, q[1], q[2], q[3] on bins a - 2 .. a, q[3] from there on"""
    e = flat(bands, q[3])
    e[:a - 2] = q[0]
    e[a - 2], e[a - 1], e[a] = q[1], q[2], q[3]
    return e


def cross(e, t, k=1):
    """choose e[0] so that P[t] == k 2^32 exactly: the sum passes the multiple on bin t"""
    rest = int(e[1:t + 1].sum())
    e0 = (k << 32) - rest
    assert 0 <= e0 <= U32 and e0 >= max(int(x) for x in e[1:4]) and e[t] >= 1, (t, e0)
    e[0] = e0
    return e


def dense(bands):
    """tops rising on the odd bins, valleys falling on the even ones: a candidate on every odd bin"""
    e = np.zeros(bands, np.int64)
    a = np.arange(bands)
    e[1::2] = 1000 + a[1::2]
    e[0::2] = 2 * bands - a[0::2] // 2
    return e


def humps(bands, k):
    """speech-like: a few triangular humps of different width over a small ripple"""
    a = np.arange(bands, dtype=np.int64)
    e = 3 + (a * 7 + k) % 5
    for j in range(1 + (k + bands) % 4 + bands // 40):
        c = (17 * j + 11 * k + 5) % max(bands, 1)
        A = 400 * (j + 1) * (k + 2) + 37 * j
        w = 2 + (3 * j + k) % 7
        e = np.maximum(e, A - (A // w) * np.abs(a - c))
    return e


# ------------------------------------------------------------------------------------------------------------------ the geometry model
GEO_ARMS = (["round_edge_%s_%d" % (k, t) for k in ("rise", "fall", "timeout_1_2", "timeout_2_1", "creep") for t in EDGES]
            + ["carry_%s_%d" % (k, a) for k in ("R_true", "F_true", "R_a3_refuses", "F_a3_refuses") for a in CARRY_BINS]
            + ["%s_W%d_%s" % (k, W, hi) for W in W_LANE for hi in ("lo", "hi") for k in ("ring_path_at_limit", "global_path_just_past_qi_in", "global_path_just_past_qi_below")]
            + ["global_path_W%d_%s" % (W, k) for W in W_LANE for k in ("qs_in", "qs_below")]
            + ["hi_at_round_start_W%d" % W for W in W_LANE] + ["hi_at_round_end_W%d" % W for W in W_LANE] + ["hi_two_crossings_in_round_W%d" % W for W in W_LANE]
            + ["hi_one_frame_only"]
            + ["list_partial_flush_%s_W%d" % (k, W) for W in W_LANE for k in ("once", "twice")] + ["list_partial_flush_rest_W%d" % W for W in W_LANE]
            + ["partial_tile_W32", "partial_tile_W16", "non_vector_rows", "bands_1", "bands_2"])


def geometry(e, r=None):
    """geometry arms of ONE frame: where its events and candidates fall in the kernels' rounds, ring and words.  r = peak_ref.scan(e)."""
    B = len(e)
    r = r or peak_ref.scan(e)
    ev = [int(x) for x in e]
    P = r["P"]
    g = dict.fromkeys(GEO_ARMS, 0)
    what = {}
    for a, k in r["events"]:
        what.setdefault(k, []).append(a)
    for t in EDGES:
        if t in what.get("rise_from_idle", []) + what.get("rise_closes", []):
            g["round_edge_rise_%d" % t] += 1                               # i = t - 1: the last bin of the round before
        if t in what.get("fall_from_rising", []):
            g["round_edge_fall_%d" % t] += 1
        if t in what.get("creep", []):
            g["round_edge_creep_%d" % t] += 1
    # the three flat bins of a timeout: the bins that counted c to 1, 2, 3 (the last one is the emission bin)
    flats = [(a, int(k[5:])) for a, k in r["events"] if k.startswith("flat_")]
    for j, (a, k) in enumerate(flats):
        if k == 3 and j >= 2 and flats[j - 1][1] == 2 and flats[j - 2][1] == 1:
            b1, b2, b3 = flats[j - 2][0], flats[j - 1][0], a
            for t in EDGES:
                if b1 < t <= b2:
                    g["round_edge_timeout_1_2_%d" % t] += 1
                if b2 < t <= b3:
                    g["round_edge_timeout_2_1_%d" % t] += 1
    for a in CARRY_BINS:
        if a < B and a >= 3:
            x, p1, p2, p3 = ev[a], ev[a - 1], ev[a - 2], ev[a - 3]
            if x > p1 and x > p2:
                g["carry_R_true_%d" % a if x > p3 else "carry_R_a3_refuses_%d" % a] += 1
            if x < p1 and x < p2:
                g["carry_F_true_%d" % a if x < p3 else "carry_F_a3_refuses_%d" % a] += 1
    for W in W_LANE:
        for (ci, cs, cl, a), (qi, qs, _, last) in zip(r["raw"], r["cands"]):
            t0 = a // W * W                                                # the round that emits: the one that holds the closing rise / third flat bin / last bin
            lo_valid = max(0, t0 - W)
            hi = "hi" if P[min(t0 + W, B) - 1] >> 32 else "lo"             # any_hi of a wave of such frames at that round
            first = max(ci - 1, 0)
            if lo_valid > 0 and first == lo_valid:
                g["ring_path_at_limit_W%d_%s" % (W, hi)] += 1
            if lo_valid > 0 and first == lo_valid - 1:
                g["global_path_just_past_qi_%s_W%d_%s" % ("in" if qi - 1 >= lo_valid else "below", W, hi)] += 1
            if first < lo_valid:
                g["global_path_W%d_%s" % (W, "qs_in" if qs >= lo_valid else "qs_below")] += 1
        crossings = [a for a in range(1, B) if P[a] >> 32 != P[a - 1] >> 32]
        if any(a % W == 0 for a in crossings):
            g["hi_at_round_start_W%d" % W] += 1
        if any(a % W == W - 1 for a in crossings):
            g["hi_at_round_end_W%d" % W] += 1
        if r["cands"] and any(sum(1 for a in crossings if a // W == q) >= 2 for q in range((B + W - 1) // W)):
            g["hi_two_crossings_in_round_W%d" % W] += 1
        # a wave of 64 such frames (arrangement b) appends 64 entries per candidate; the list holds 8 W and is emptied at the end of every round, so a round
        # with more than 8 W entries was flushed in its middle at least once, with more than 16 W at least twice (a flush works off at most the whole list)
        per_round = {}
        for (_, _, _, a) in r["raw"][:64]:
            per_round[a // W] = per_round.get(a // W, 0) + 64
        if any(v > 8 * W for v in per_round.values()):
            g["list_partial_flush_once_W%d" % W] += 1
        if any(v > 16 * W for v in per_round.values()):
            g["list_partial_flush_twice_W%d" % W] += 1
        if B % W and B > 1:
            g["partial_tile_W%d" % W] += 1
    if B % 4:
        g["non_vector_rows"] += 1                                          # rows are no multiple of 16 bytes: the staging takes its scalar form
    if B <= 2:
        g["bands_%d" % B] += 1
    return g


def case_geometry(c):
    tot = dict.fromkeys(GEO_ARMS, 0)
    for f in c["frames"]:
        for k, v in geometry(f).items():
            tot[k] += v
    # one frame of the wave above 2^32 while the others hold zeros: a property of the case, whose frames stand together in arrangement (a) and whose
    # loud frame has 63 silent ones on either side, so that any wave that holds it holds nothing else
    fr = c["frames"].astype(np.int64)
    loud = [k for k, f in enumerate(fr) if int(f.sum()) >> 32]
    if len(loud) == 1 and loud[0] >= 63 and len(fr) - loud[0] > 63 and not fr[:loud[0]].any() and not fr[loud[0] + 1:].any():
        tot["hi_one_frame_only"] += 1
    # the case as a launch of its own, fewer than 64 frames (one wave): a step of the state machine appends at most one entry per frame, so the list grows
    # by less than 64 at a time; with more than 8 W entries in a round it is flushed in mid-round at a length strictly between 8 W - 64 and 8 W, which
    # is no multiple of 64: the flush works off whole groups of 64 and moves a rest to the front
    if len(fr) < 64:
        for W in W_LANE:
            per_round = {}
            for f in fr:
                for (_, _, _, a) in peak_ref.scan(f)["raw"][:64]:
                    per_round[a // W] = per_round.get(a // W, 0) + 1
            if any(v > 8 * W for v in per_round.values()):
                tot["list_partial_flush_rest_W%d" % W] += 1
    return tot


# ------------------------------------------------------------------------------------------------------------------ ordinary frames
for _B in (128, 127, 96, 64, 65, 33, 17, 200, 256):
    case("humps-%d" % _B, _B, dict(rise_from_idle=1, fall_from_rising=1, flat_timeout=1),
         geo=[k for k, on in (("partial_tile_W32", _B % 32), ("partial_tile_W16", _B % 16), ("non_vector_rows", _B % 4)) if on])(
        lambda _B=_B: [humps(_B, k) for k in range(4)])


@case("silence-and-constants", 128, dict(largest_none=3, R_eq_1=127, F_eq_1=127, idle_neither=127))
def _():
    return [flat(128), flat(128, 1), flat(128, U32)]


# ------------------------------------------------------------------------------------------------------------------ the six comparisons
QUADS = {"R_true": (1, 2, 3, 9), "R_eq_2": (1, 5, 3, 5), "R_eq_3": (5, 1, 2, 5), "R_wrong_2": (1, 9, 3, 5), "R_wrong_3": (9, 1, 2, 5),
         "F_true": (9, 8, 7, 1), "F_eq_2": (9, 5, 7, 5), "F_eq_3": (5, 9, 8, 5), "F_wrong_2": (9, 1, 7, 5), "F_wrong_3": (1, 9, 8, 5)}


@case("predicates-first-bins", 128, dict(R_true_a1=1, R_true_a2=1, R_true_a3plus=1, F_true_a1=1, F_true_a2=1, F_true_a3plus=1, R_eq_2_alone=1, F_eq_2_alone=1,
                                         fall_while_idle=3, rise_while_rising=2))
def _():
    up, dn = flat(128, 9), flat(128, 1)
    up[:4] = (1, 2, 3, 4); up[4:] = 4                     # rises at a = 1, 2, 3
    dn[:4] = (9, 8, 7, 6); dn[4:] = 6                     # falls at a = 1, 2, 3 (idle: nothing happens)
    a2r, a2f = flat(128, 5), flat(128, 5)
    a2r[:3] = (5, 3, 5)                                   # a = 2: above e[1], equal to e[0]: the `a < 3` side of the third test
    a2f[:3] = (5, 7, 5)
    return [up, dn, a2r, a2f]


@case("predicates-at-word-edges", 128, dict(R_true_a3plus=8, F_true_a3plus=8, R_eq_2_alone=8, R_eq_3_alone=8, R_wrong_2=8, R_wrong_3=8,
                                            F_eq_2_alone=8, F_eq_3_alone=8, F_wrong_2=8, F_wrong_3=8),
      geo=["carry_%s_%d" % (k, a) for k in ("R_true", "F_true", "R_a3_refuses", "F_a3_refuses") for a in CARRY_BINS])
def _():
    # every quad with its tested bin at 8 and at 16, 32, 33, 34, 64, 65, 66: the three bins before it lie in the round / the 64-bit word before
    return [quad(128, a, q) for q in QUADS.values() for a in (8,) + CARRY_BINS]


# ------------------------------------------------------------------------------------------------------------------ the state machine
@case("flat-counter-carried", 128, dict(rise_leaves_c_1=1, rise_leaves_c_2=1, flat_timeout_carried_1=1, flat_timeout_carried_2=1, flat_counts_1=2, flat_counts_2=2,
                                        rise_closes_candidate=2, fall_while_idle=2))
def _():
    # the reference does not clear c when a rise closes a falling stretch: the next stretch times out after two flat bins (one), and the fall behind
    # the early timeout meets an idle scan.  35 >= 300 / 10 keeps the shrink away from it.
    one, two = flat(128, 100), flat(128, 100)
    one[3:12] = (200, 50, 50, 300, 40, 40, 40, 35, 35)     # fall, flat (c = 1), rise; fall, flat, flat: timeout at the second; 35 falls while idle
    one[12:] = 35
    two[3:12] = (200, 50, 50, 50, 300, 40, 40, 35, 35)     # fall, flat, flat (c = 2), rise; fall, flat: timeout at the first
    two[12:] = 35
    return [one, two]


@case("flat-timeout-then-fall", 128, dict(flat_timeout=1, fall_while_idle=1, flat_counts_1=1, flat_counts_2=1))
def _():
    e = flat(128, 100)
    e[3:10] = (200, 50, 50, 50, 50, 45, 45)                # the third flat bin ends the stretch; the fall behind it moves nothing
    e[10:] = 45
    return [e]


@case("creep", 128, dict(creep_below_kept=1, creep_moves_l=1, creep_equal_kept=1, fall_from_rising=1, R_wrong_2=1))
def _():
    e = flat(128, 100)
    e[3:9] = (200, 150, 160, 160, 20, 20)                  # 150: below, not a fall; 160: above its predecessor, l moves off the higher bin; 160: equal
    e[9:] = 20
    return [e]


@case("falls-move-s", 128, dict(fall_moves_s=4, shrink_right_0=1))
def _():
    e = flat(128, 0)
    hump(e, 10, [260, 300], 900, [250, 240, 230, 220, 210])
    return [e]


@case("end-of-spectrum", 128, dict(eos_emit=3, eos_after_creep=1, eos_while_falling=1, eos_rise_on_last_bin=1, largest_eos_excluded=2))
def _():
    rising, crept, falling, lastbin, zero = (flat(128, 100) for _ in range(5))
    hump(rising, 20, [150], 300, [50])
    rising[120:] = 100 + 10 * np.arange(1, 9)              # still rising at bin 127, higher than the candidate before it
    crept[125:] = (200, 150, 150)                          # the rise at 125 is the highest bin; l is forced to 127: amplitude and threshold are e[127]'s
    falling[125:] = (100, 200, 50)                         # a candidate is pending at the last bin: dropped
    hump(lastbin, 20, [150], 180, [50])
    lastbin[127] = 200                                     # the rise sits on the last bin
    zero[:] = 0
    zero[125] = 5                                          # rising at 125, then 0, 0: neither a fall nor a creep; the forced l has amplitude 0
    return [rising, crept, falling, lastbin, zero]


REF_DROPS_ZERO = {("end-of-spectrum", 4)}                  # (case, frame): the reference's `e[l] > 0.1` drops the candidate of amplitude 0, the device keeps it


@case("largest", 128, dict(largest_tie_first_kept=2, largest_eos_excluded=1, largest_none=1))
def _():
    tie, eos_only = flat(128, 10), flat(128, 10)
    for at, top in ((10, 500), (30, 900), (50, 900), (70, 900), (90, 600)):
        hump(tie, at, [100], top, [50])
        tie[at + 3:at + 6] = 10
    eos_only[127] = 50                                     # the only candidate is the end-of-spectrum emission: the header says (0, 0)
    return [tie, eos_only]


# ------------------------------------------------------------------------------------------------------------------ the shrink
@case("shrink-counts", 128, dict(shrink_left_0=1, shrink_left_1=1, shrink_left_2=1, shrink_left_3=1, shrink_left_4=1, shrink_left_5plus=1, shrink_left_to_l=1,
                                 shrink_right_0=1, shrink_right_1=1, shrink_right_2=1, shrink_right_3=1, shrink_right_4=1, shrink_right_5plus=1, shrink_right_to_l=1,
                                 shrink_left_outlasts_right=1, shrink_right_outlasts_left=1))
def _():
    out = []
    for k in range(7):                                     # k bins of either shoulder lie below a tenth of the top; 6: the walk ends on l itself
        L = flat(128, 200 if k == 0 else 0)               # the background bin i = a - 1 is the first below, k - 1 bins of the shoulder follow it
        hump(L, 20, [1 + j for j in range(k - 1 if k < 6 else 5)] + ([300, 400] if k < 6 else []), 2000, [100])
        Rr = flat(128, 0)
        hump(Rr, 20, [900], 2000, ([400, 300] if k < 6 else []) + [9 - j for j in range(k)])
        out += [L, Rr]
    return out


@case("shrink-threshold", 128, dict(shrink_equal_stops=2, shrink_10k1_floor_goes_on=2, shrink_10k1_ceil_stops=2, shrink_10k9_floor_goes_on=2, shrink_10k9_ceil_stops=2))
def _():
    out = []
    for top in (1000, 1001, 1009):                         # 10 e[x] against e[l] = 10 k, 10 k + 1, 10 k + 9 at e[x] = k - 1, k, k + 1
        e = flat(128, 0)
        hump(e, 20, [98, 99, 100, 101, 102], top, [102, 101, 100, 99, 98])
        out.append(e)
    return out


@case("shrink-u32", 128, dict(shrink_big=2, g_above_2_32=1))
def _():
    # the top 2^32 - 1: a tenth of it is 429496729.5; 10 e[x] of the bins that stop the walk does not fit a u32
    e = flat(128, 0)
    hump(e, 20, [429496728, 429496729, 429496730, 429496731], U32, [429496730, 429496729, 429496728, 429496727])
    return [e]


# ------------------------------------------------------------------------------------------------------------------ amounts
@case("prefix-crossings", 128, dict(p_cross_at_i_minus_1=1, p_cross_at_s=1, p_cross_inside_shoulder=3, g_above_2_32=1),
      geo=["hi_at_round_start_W32", "hi_at_round_start_W16", "hi_at_round_end_W32", "hi_at_round_end_W16", "hi_two_crossings_in_round_W32", "hi_two_crossings_in_round_W16"])
def _():
    out = []
    for t in (31, 32, 15, 16, 63, 64, 95, 96):             # the sum reaches 2^32 on the candidate's bin i - 1 and, in a second frame, on its bin s
        for which in (0, 1):
            e = flat(128, 100)
            top = hump(e, t + 2 if which == 0 else t - 3, [150, 160], 300, [90])       # i - 1 = t  /  s = t
            assert (top - 4 if which == 0 else top + 1) == t
            out.append(cross(e, t))
    e = flat(128, 100)
    e[40:44] = U32                                         # the sum passes a multiple of 2^32 on four bins running, inside one candidate
    e[44:] = 50
    out.append(e)
    return out


@case("saturated-256", 256, dict(p_high_byte_255=1, eos_rise_on_last_bin=1, g_above_2_32=2, shrink_big=1), geo=["hi_two_crossings_in_round_W32"])
def _():
    e = flat(256, U32 - 1)
    e[255] = U32                                           # P[255] = 2^40 - 511: the high byte of the last candidate's P[s] is 255
    f = flat(256, U32 - 7)
    for at in range(5, 250, 9):
        hump(f, at, [U32 - 5], U32, [U32 - 9])
    return [e, f]


@case("one-loud-frame", 128, dict(g_above_2_32=1, p_cross_inside_shoulder=1), geo=["hi_one_frame_only"])
def _():
    e = flat(128, 0)
    hump(e, 60, [1 << 30, 1 << 31], U32, [1 << 31, 1 << 30])
    hump(e, 100, [500], 1000, [400])
    z = flat(128, 0)
    return [z] * 63 + [e] + [z] * 63


# ------------------------------------------------------------------------------------------------------------------ rounds and words
def _edge_frames(t):
    rise, fall, t12, t21, creep = (flat(128, 100) for _ in range(5))
    rise[t:t + 2] = (300, 50); rise[t + 2:] = 50                                   # the rise on the round's first bin: i = t - 1
    fall[t - 1:t + 1] = (300, 50); fall[t + 1:] = 50                                 # ... the fall on it
    t12[t - 3:t - 1] = (300, 50); t12[t - 1:] = 50                                   # fall at t - 2, flat bins t - 1 | t, t + 1
    t21[t - 4:t - 2] = (300, 50); t21[t - 2:] = 50                                   # fall at t - 3, flat bins t - 2, t - 1 | t
    creep[t - 2:t + 2] = (300, 150, 160, 20); creep[t + 2:] = 20                      # l moves to the round's first bin by a creep
    return [rise, fall, t12, t21, creep]


@case("round-edges", 128, dict(rise_from_idle=20, flat_timeout=20, creep_moves_l=4),
      geo=["round_edge_%s_%d" % (k, t) for k in ("rise", "fall", "timeout_1_2", "timeout_2_1", "creep") for t in EDGES])
def _():
    return [f for t in EDGES for f in _edge_frames(t)]


def _long_rise(bands, r, top_at, loud, shrink):
    """a candidate that rises from bin r to top_at, falls once and is closed by the third flat bin at top_at + 4.  shrink: bins of the left shoulder below a
    tenth of the top.  loud: the sum is above 2^32 from bin 1 on."""
    e = flat(bands, 0)
    n = top_at - r
    top = 1000 * n
    left = [(1 + j) if j < shrink - 1 else 100 * n + j for j in range(n)]           # the background bin i = r - 1 (0) is always the first below
    if shrink == 0:
        e[:r] = 100 * n
        left = [100 * n + 1 + j for j in range(n)]
    hump(e, r, left, top, [50 * n])
    if loud:
        e[0] = U32
        e[1:3] = max(int(e[1]), 1)
        assert int(e[:2].sum()) >> 32
    return e


@case("ring-and-global-path", 128, dict(rise_while_rising=30),
      geo=["%s_W%d_%s" % (k, W, hi) for W in W_LANE for hi in ("lo", "hi") for k in ("ring_path_at_limit", "global_path_just_past_qi_in", "global_path_just_past_qi_below")]
          + ["global_path_W%d_%s" % (W, k) for W in W_LANE for k in ("qs_in", "qs_below")])
def _():
    out = []
    for W in W_LANE:
        # emitted at bin 74 (round t0 = 64): lo_valid = 64 - W; max(i - 1, 0) = r - 2 equal to it (the ring's last bin) and one below (the frame's row)
        lo = 64 - W
        for loud in (False, True):
            out.append(_long_rise(128, lo + 2, 70, loud, 0))                          # ring path at its limit
            out.append(_long_rise(128, lo + 2, 70, loud, 3))
            out.append(_long_rise(128, lo + 1, 70, loud, 0))                          # global path, the shrunk i - 1 stays below the ring
            out.append(_long_rise(128, lo + 1, 70, loud, 1))                          # ... ends on the ring's first bin
            out.append(_long_rise(128, lo + 1, 70, loud, 4))                          # ... inside it
            out.append(_long_rise(128, lo - 7, 70, loud, 2))                          # further below
    for loud in (False, True):
        # a top at bin 10 and a long fall: closed in round 64; the right shoulder shrinks back to the top, below both rings
        e = flat(128, 0)
        hump(e, 8, [500000, 700000], 1000000, [2000 - j for j in range(60)])
        if loud:
            e[0] = U32; e[1:3] = 1
        out.append(e)
        # the same fall, kept: s stays inside the ring
        e = flat(128, 0)
        hump(e, 8, [5000, 7000], 10000, [2000 - j for j in range(60)])
        if loud:
            e[0] = U32; e[1:3] = 1
        out.append(e)
    return out


# ------------------------------------------------------------------------------------------------------------------ crowded frames, the list
@case("dense-128", 128, dict(cand_64=1, rise_closes_candidate=63, eos_emit=1),
      geo=["list_partial_flush_once_W32", "list_partial_flush_twice_W32", "list_partial_flush_once_W16", "list_partial_flush_twice_W16"])
def _():
    e = dense(128)
    assert len(peak_ref.scan(e)["cands"]) == 64
    return [e]


@case("dense-200", 200, dict(cand_65=1), geo=["list_partial_flush_twice_W32", "partial_tile_W32", "partial_tile_W16"])
def _():
    return [dense(200)]


@case("dense-mixed-lanes", 128, dict(rise_closes_candidate=600), geo=["list_partial_flush_rest_W32", "list_partial_flush_rest_W16"])
def _():
    # neighbours that differ, fewer than a wave: the dense frame cut off at rising bins (flat behind); run as a launch of its own, the list grows by
    # fewer than 64 entries a step and a flush in mid-round leaves a rest (case_geometry)
    out = []
    for k in range(24):
        e = dense(128)
        cut = 9 + 5 * k
        e[cut:] = e[cut - 1] if cut % 2 == 0 else e[cut - 2]
        out.append(e)
    return out


# ------------------------------------------------------------------------------------------------------------------ small and odd band counts
@case("bands-1", 1, dict(largest_none=3), geo=["bands_1"])
def _():
    return [flat(1), flat(1, 7), flat(1, U32)]


@case("bands-2", 2, dict(eos_rise_on_last_bin=2, R_true_a1=2, F_true_a1=1, R_eq_1=1, eos_emit=2), geo=["bands_2"])
def _():
    return [np.array(x, np.int64) for x in ((0, 0), (0, 1), (5, 1), (1, U32), (U32, U32))]


@case("one-bin-tiles", 33, dict(eos_rise_on_last_bin=1, eos_while_falling=1, eos_emit=2), geo=["partial_tile_W32", "partial_tile_W16"])
def _():
    a, b, c = flat(33, 100), flat(33, 100), flat(33, 100)
    a[32] = 300                                            # the last round holds one bin, and it rises
    b[31:] = (300, 50)                                     # ... falls
    c[30:] = (300, 150, 160)                               # ... creeps
    return [a, b, c]


@case("one-bin-tiles-17", 17, dict(eos_rise_on_last_bin=1, eos_while_falling=1, eos_emit=2), geo=["partial_tile_W16", "non_vector_rows"])
def _():
    a, b, c = flat(17, 100), flat(17, 100), flat(17, 100)
    a[16] = 300
    b[15:] = (300, 50)
    c[14:] = (300, 150, 160)
    return [a, b, c]


@case("rows-of-127", 127, dict(rise_closes_candidate=60), geo=["non_vector_rows", "partial_tile_W32", "list_partial_flush_once_W32"])
def _():
    e = dense(127)
    return [e] + [f[:127] for t in (32, 64, 96) for f in _edge_frames(t)]


# the floors a case is run at a second time (tests/golden/gen/make_peaks_golden.py: the fixed gate's voiced_min_dB 20 and 40): e[l] > v at equality, h from 2 v
FLOOR_RUNS = {"floor-edges": (20.0, 40.0)}


@case("floor-edges", 128, dict())
def _():
    e = flat(128, 1)
    for at, top in ((10, 9), (20, 10), (30, 11), (40, 20), (50, 21), (60, 100), (70, 101), (80, 200), (90, 201), (100, 99)):
        hump(e, at, [3], top, [2])
        e[at + 2:at + 6] = (2, 2, 2, 1)
    f = e.copy()
    f[60:63] = (3, 21, 2)                                   # at a floor of 10 nothing is above 2 v but by one
    return [e, f]


if __name__ == "__main__":
    tot, geo = dict.fromkeys(peak_ref.ARMS, 0), dict.fromkeys(GEO_ARMS, 0)
    for c in CASES:
        for f in c["frames"]:
            for k, v in peak_ref.scan(f)["arms"].items():
                tot[k] += v
        for k, v in case_geometry(c).items():
            geo[k] += v
        print("%-28s %3d bands %4d frames" % (c["name"], c["bands"], len(c["frames"])))
    print("frames in all:", sum(len(c["frames"]) for c in CASES))
    print("scan arms never taken:", [k for k, v in tot.items() if not v])
    print("geometry arms never taken:", [k for k, v in geo.items() if not v])

"""The peak scan of one u32 frame by the letter of the reference's frame loop D() (ref dist/main.js:2 @B25717, scan @B25827; DESIGN.md K1b,
SURVEY.md appendix A) (test helper): the one plain restatement that tests/test_gpu_units.py, tests/gate_cases.py and tests/peak_cases.py share, with an
arm counter on each side of every comparison (the same names as PEAK_ARMS in oracle/backend.c, which tests/test_peaks_reference.py holds it against)
and a table of one-line faults (`mutant=`) that the hand-built cases must notice.

scan(e, v) -> dict:
  cands    [(i, s, l, last)] after the /10 shoulder shrink; last = 1 for the end-of-spectrum emission
  p_i, p_s exact prefix sums P[i - 1] (0 for i = 0) and P[s], P[x] = e[0] + .. + e[x], one pair per candidate
  n, p, h, d, g   what the frame loop hands to the gate: accepted candidates, bin and amplitude of the largest, sum of amplitudes, sum e[1 ..]
  largest  (amplitude, bin) as the device's frame header stores it: first among equals, the end-of-spectrum emission left out, (0, 0) without one
  arms     {name: count}
  raw      [(i, s, l, a)] the same candidates before the shrink, with the bin a at which the loop emitted them; events [(bin, what)]; P the prefix sums
           (what the geometry model of tests/peak_cases.py works from)
v is the noise floor: a candidate is kept when e[l] > v, and h starts from 2 v.  v = None keeps every candidate and starts h from 0: the device's table
(csrc/peaks.hip emits all of them, the gate applies the floor later)."""

U32 = 4294967295
BIG = (1 << 32) // 10 + 1          # the least e[x] whose tenfold does not fit a u32

_PRED = ["true_a1", "true_a2", "true_a3plus", "eq_1", "eq_2_alone", "eq_3_alone", "wrong_2", "wrong_3"]
ARMS = (["R_" + k for k in _PRED] + ["F_" + k for k in _PRED] + [
    "rise_from_idle", "rise_closes_candidate", "rise_leaves_c_1", "rise_leaves_c_2", "rise_while_rising", "close_guard_fails",
    "fall_from_rising", "fall_moves_s", "fall_while_idle",
    "flat_counts_1", "flat_counts_2", "flat_timeout", "flat_timeout_carried_1", "flat_timeout_carried_2",
    "creep_moves_l", "creep_equal_kept", "creep_below_kept", "idle_neither",
    "eos_emit", "eos_after_creep", "eos_while_falling", "eos_rise_on_last_bin", "eos_guard_fails",
    "floor_equal_refused", "floor_below_refused", "h_2v_not_above"]
    + ["shrink_%s_%s" % (sd, k) for sd in ("left", "right") for k in ("0", "1", "2", "3", "4", "5plus", "to_l")] + [
    "shrink_equal_stops", "shrink_10k1_floor_goes_on", "shrink_10k1_ceil_stops", "shrink_10k9_floor_goes_on", "shrink_10k9_ceil_stops", "shrink_big",
    "shrink_left_outlasts_right", "shrink_right_outlasts_left",
    "largest_tie_first_kept", "largest_eos_excluded", "largest_none",
    "g_above_2_32", "p_cross_inside_shoulder", "p_cross_at_i_minus_1", "p_cross_at_s", "p_high_byte_255", "cand_64", "cand_65"])

# the arms the loop's own invariants keep shut, each with its reason (tests/test_peaks_reference.py exempts exactly these)
UNREACHABLE = {
    "close_guard_fails": "`i <= l && l < s` is asked only while u == -1, which only a fall out of u == 1 sets: the rise before it left i = l - 1 or less and "
                         "the fall put s past l; an emission shrinks i and s no further than l and is followed by u = 0 or a new [i, l]",
    "eos_guard_fails": "`i < l` at the end of the spectrum is asked only while u == 1: the last rise out of idle or falling set i = a - 1, l = a, and while "
                       "rising l only grows",
}

MUTANTS = ("c_cleared_at_rise", "shrink_le", "thr_floored", "eos_in_largest", "tie_to_later", "R_no_a3", "F_no_a3", "creep_ge", "timeout_gt3",
           "ps_high_early", "g_with_e0", "l_not_forced")


def scan(e, v=None, mutant=None):
    assert mutant is None or mutant in MUTANTS, mutant
    B = len(e)
    e = [int(x) for x in e]
    arms = dict.fromkeys(ARMS, 0)
    P, t = [], 0
    for x in e:
        t += x
        P.append(t)
    every = v is None
    n = p = 0
    d = 0
    h = 0 if every else 2 * v
    cands, p_i, p_s, raw, events = [], [], [], [], []
    i = l = s = c = u = c0 = 0

    def pred(a, X, above, drop3):
        """the rising (above) / falling test of bin a against the three bins before it"""
        ea = e[a]
        cmp = (lambda x, y: x > y) if above else (lambda x, y: x < y)
        if ea == e[a - 1]:
            arms[X + "eq_1"] += 1
            return False
        if not cmp(ea, e[a - 1]):
            return False
        ok2 = a < 2 or cmp(ea, e[a - 2])
        ok3 = a < 3 or cmp(ea, e[a - 3]) or drop3
        if a >= 2 and not ok2:
            if ea != e[a - 2]:
                arms[X + "wrong_2"] += 1
            elif ok3:
                arms[X + "eq_2_alone"] += 1
        if ok2 and not ok3:
            arms[X + ("eq_3_alone" if ea == e[a - 3] else "wrong_3")] += 1
        if ok2 and ok3:
            arms[X + ("true_a1" if a == 1 else "true_a2" if a == 2 else "true_a3plus")] += 1
        return ok2 and ok3

    def emit(last):
        nonlocal i, s, n, p, h, d
        el = e[l]
        if not every and not el > v:
            arms["floor_equal_refused" if el == v else "floor_below_refused"] += 1
            return
        if last and mutant != "eos_in_largest":
            if el > h:
                arms["largest_eos_excluded"] += 1
        else:
            if p > 0 and el == h:
                arms["largest_tie_first_kept"] += 1
            if not every and p == 0 and not el > h:
                arms["h_2v_not_above"] += 1
            if el > h or (mutant == "tie_to_later" and p > 0 and el == h):
                h, p = el, l
        raw.append((i, s, l, a))
        k, m = divmod(el, 10)

        def goes(x):
            ex = e[x]
            if ex >= BIG:
                arms["shrink_big"] += 1
            if m == 0 and ex == k:
                arms["shrink_equal_stops"] += 1
            if m in (1, 9) and ex in (k, k + 1):
                arms["shrink_10k%d_%s" % (m, "floor_goes_on" if ex == k else "ceil_stops")] += 1
            if mutant == "shrink_le":
                return 10 * ex <= el
            if mutant == "thr_floored":
                return ex < k
            return 10 * ex < el                    # e[x] < e[l] / 10

        nl = nr = 0
        while i < l and goes(i):
            i += 1; nl += 1
        while s > l and goes(s):
            s -= 1; nr += 1
        for sd, q, at_l in (("left", nl, i == l), ("right", nr, s == l)):
            arms["shrink_%s_%s" % (sd, q if q < 5 else "5plus")] += 1
            if at_l:
                arms["shrink_%s_to_l" % sd] += 1
        if nl > nr:
            arms["shrink_left_outlasts_right"] += 1
        if nr > nl:
            arms["shrink_right_outlasts_left"] += 1
        pi = P[i - 1] if i > 0 else 0
        ps = P[s]
        if ps >> 32 != pi >> 32:
            arms["p_cross_inside_shoulder"] += 1
        if i > 0 and pi >> 32 != (P[i - 2] if i > 1 else 0) >> 32:
            arms["p_cross_at_i_minus_1"] += 1
        if ps >> 32 != P[s - 1] >> 32:
            arms["p_cross_at_s"] += 1
        if ps >> 32 == 255:
            arms["p_high_byte_255"] += 1
        if mutant == "ps_high_early":
            ps = (P[s - 1] >> 32 << 32) | (ps & U32)
        cands.append((i, s, l, last)); p_i.append(pi); p_s.append(ps)
        n += 1; d += el

    g = e[0] if mutant == "g_with_e0" and B else 0
    for a in range(1, B):
        g += e[a]
        R = pred(a, "R_", True, mutant == "R_no_a3")
        F = (not R) and pred(a, "F_", False, mutant == "F_no_a3")
        if R:
            if a == B - 1:
                arms["eos_rise_on_last_bin"] += 1
            if u in (-1, 0):
                if u == -1:
                    if i <= l and l < s:
                        arms["rise_closes_candidate"] += 1
                        events.append((a, "rise_closes"))
                        if c in (1, 2):
                            arms["rise_leaves_c_%d" % c] += 1
                        emit(0)
                    else:
                        arms["close_guard_fails"] += 1
                    if mutant == "c_cleared_at_rise":
                        c = 0
                else:
                    arms["rise_from_idle"] += 1
                    events.append((a, "rise_from_idle"))
                i = a - 1; l = a
            else:
                arms["rise_while_rising"] += 1
                l = a
            u = 1
        elif F:
            if u == 1:
                arms["fall_from_rising"] += 1
                events.append((a, "fall_from_rising"))
                c0 = c
            if u == -1:
                arms["fall_moves_s"] += 1
            if u == 0:
                arms["fall_while_idle"] += 1
            if u in (1, -1):
                s = a; u = -1
        elif u == -1:
            c += 1
            if c < 3:
                arms["flat_counts_%d" % c] += 1
            events.append((a, "flat_%d" % c))
            if c > (3 if mutant == "timeout_gt3" else 2):
                c = 0
                if i <= l and l < s:
                    arms["flat_timeout"] += 1
                    if c0 in (1, 2):
                        arms["flat_timeout_carried_%d" % c0] += 1
                    emit(0)
                else:
                    arms["close_guard_fails"] += 1
                u = 0
        elif u == 1:
            if e[a] > e[a - 1] or (mutant == "creep_ge" and e[a] == e[a - 1]):
                if e[a] > e[a - 1]:
                    arms["creep_moves_l"] += 1
                    events.append((a, "creep"))
                l = a
            if e[a] == e[a - 1]:
                arms["creep_equal_kept"] += 1
            if e[a] < e[a - 1]:
                arms["creep_below_kept"] += 1
        else:
            arms["idle_neither"] += 1
        if a == B - 1 and u == -1:
            arms["eos_while_falling"] += 1
        if a == B - 1 and u == 1:
            crept = l != a and e[l] > e[a]
            s = a
            if mutant != "l_not_forced":
                l = a
            if i < l and l <= s:
                arms["eos_emit"] += 1
                if crept:
                    arms["eos_after_creep"] += 1
                emit(1)
            else:
                arms["eos_guard_fails"] += 1
    if g >> 32:
        arms["g_above_2_32"] += 1
    if p == 0:
        arms["largest_none"] += 1
    if n == 64:
        arms["cand_64"] += 1
    if n > 64:
        arms["cand_65"] += 1
    return dict(cands=cands, p_i=p_i, p_s=p_s, raw=raw, events=events, P=P, n=n, p=p, h=h, d=d, g=g, largest=(h, p) if p > 0 else (0, 0), arms=arms)


def record(r):
    """what a fault must change to be noticed: everything a frame's device record holds"""
    return (r["cands"], r["p_i"], r["p_s"], r["g"], r["largest"])

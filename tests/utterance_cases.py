"""Hand-built results for output level 11's utterance histograms (csrc/utterance.hip, K4) (test helper): the deterministic table of cases, a traced
twin of the fifteen `bump` arguments (domain assertion, path counts), and the layouts that put the cases into the tables of the test entry
wsa_debug_utterance — whole clips in the batch geometry, steps of streams (with a host model of compact_gather_kernel's carry) in the streams'.

A case is what one launch of the reference accumulates: `segs` = segments_ci with a flag, [(start, len, flag)] (flag < 0: the straighten step threw,
the entry stays in segments_ci but no result follows), and per result (one per entry with flag >= 0, in order) `syl` = [(first frame, length)] inside
the result's own frames and `frames` [n, 9] float32 = [bin, energy, width] x 3.  The frames around every syllable hold other valid points (FILL), so a
kernel that reads a frame too many or too few changes a bin.  Energies are integer-valued floats as the straighten step produces them (sums of u32
amplitudes), except in the cases of family `fractional`; family `synthetic` holds values the tracker cannot produce at all (negative or NaN widths,
a syllable of no frames) that single out one histogram.

The kernel's documented domain (utterance.hip's header): parseInt(x) is truncation because no finite argument of `bump` has a magnitude inside
(0, 1e-6) or at or above 1e21 — outside it parseInt reads the exponent notation of the Number's string.  check_domain() asserts that for every
argument of every case; NaN and +-Infinity (0 / 0, log10(0), n / 0) are no Numbers with digits and poison in the reference as in the kernel.

What a single histogram can NOT be made to do, and therefore no case does: `u` / `f` poisoned alone (a bin must be > 0 to count, so the mean bin is
NaN only together with the mean energy and width: u, d, p and f, h, m go together), `c`, `g`, `y` poisoned other than by a syllable of no frames,
`g` / `y` beyond one past their last bin (10 (e - c) / e <= 10), `i` and `o` poisoned at all (a length and a count are never negative)."""
import collections
import hashlib
import math

import numpy as np

SIZES = dict(i=10, o=10, l=10, s=10, c=20, u=40, f=40, d=24, h=24, p=8, m=8, g=10, y=10, v=20, x=20)
ORDER = "iolscufdhpmgyvx"                     # output order of the fifteen histograms
OFF = dict(zip(ORDER, np.concatenate([[0], np.cumsum([SIZES[k] for k in ORDER])]).tolist()))
NBINS = 264
LO_CLAMPED = "svx"
SEGMENT_LEVEL = "iols"
FLT_MAX = float(np.finfo(np.float32).max)
CARRY_HIST, CARRY_WORDS, UTT_STATE_WORDS = 32, 66, 288      # csrc/wsa_internal.hpp
LENS = (2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 300, 1)
COUNTS = (0, 1, 63, 64, 65, 128, 129)
FILL = np.array([31, 70000, 9, 77, 30000, 5, 140, 900, 3], np.float32)      # the frames between syllables: valid points of their own


# ---- syllables, results, cases -------------------------------------------------------------------------------------------------------------------

def syl(sl, b1=60, b2=120, e1=1000.0, e2=500.0, w1=4.0, w2=6.0):
    """[sl, 9] float32: every argument one value or sl of them; a bin of 0 is a frame without that formant (its energy and width stay)."""
    fr = np.zeros((sl, 9), np.float32)
    for col, v in zip((0, 3, 1, 4, 2, 5), (b1, b2, e1, e2, w1, w2)):
        fr[:, col] = np.broadcast_to(np.asarray(v, np.float32), (sl,))
    fr[:, 6:] = (200, 300, 3)
    return fr


def varied(sl, salt=0):
    """A syllable whose every frame differs: one frame more or fewer moves the means, the counts and the net bin movement."""
    o = np.arange(sl) + salt
    return syl(sl, 4 + (5 * o) % 70, 78 - (3 * o) % 66, 100.0 * 3 ** (o % 6), 50.0 * 2 ** (o % 9), 2 + o % 7, 3 + (3 * o) % 11)


def result(syls, lead=1, gap=(1,), tail=1):
    """A result: the syllables with `lead` FILL frames in front, gap[k % len] between them (0: back to back), `tail` behind."""
    parts, ci, pos = [np.tile(FILL, (lead, 1))], [], lead
    for k, s in enumerate(syls):
        if k:
            parts.append(np.tile(FILL, (gap[k % len(gap)], 1)))
            pos += gap[k % len(gap)]
        ci.append((pos, len(s)))
        parts.append(s)
        pos += len(s)
    parts.append(np.tile(FILL, (tail, 1)))
    return dict(syl=ci, frames=np.ascontiguousarray(np.concatenate(parts), np.float32))


def chain(items, start=40):
    """segments_ci from [(kind, len, gap)] in time order: kind 'r' a result's entry, 'd' a dropped one; gap = distance from the entry before (its end)."""
    segs, t = [], start
    for n, (kind, ln, gap) in enumerate(items):
        t += gap
        segs.append((t, ln, (n % 3 if kind == "r" else -1 - n % 2)))
        t += ln
    return segs


def _case(name, fam, segs, results):
    assert sum(f >= 0 for _, _, f in segs) == len(results), name
    return dict(name=name, fam=frozenset(fam), segs=[tuple(int(v) for v in s) for s in segs], results=results)


def N(k):
    """an ordinary syllable"""
    return varied(5 + k % 4, 3 * k)


def _plain(results, gap=20):
    return chain([("r", len(r["frames"]), gap) for r in results])


def _build():
    out = []
    add = lambda *a: out.append(_case(*a))
    # ---- per syllable-level histogram: the last bin reached unclamped, one past it, far past it, then an ordinary result
    tops = dict(c=[varied(38), varied(40), varied(300)],
                u=[syl(4, b1=78), syl(4, b1=80), syl(4, b1=255)], f=[syl(4, b2=79), syl(4, b2=81), syl(4, b2=255)],
                d=[syl(3, e1=5e7), syl(3, e1=1e8), syl(3, e1=FLT_MAX)], h=[syl(3, e2=6e5), syl(3, e2=1e6), syl(3, e2=FLT_MAX)],
                p=[syl(3, w1=15), syl(3, w1=16), syl(3, w1=200)], m=[syl(3, w2=14), syl(3, w2=17), syl(3, w2=200)],
                g=[syl(10, b1=[0] * 9 + [50]), syl(10, b1=0)], y=[syl(10, b2=[44] + [0] * 9), syl(10, b2=0)],
                v=[syl(2, b1=[10, 57]), syl(2, b1=[10, 60]), syl(2, b1=[3, 253])], x=[syl(2, b2=[10, 59]), syl(2, b2=[10, 60]), syl(3, b2=[3, 100, 253])])
    for k, special in tops.items():
        res = [result([N(0), s, N(1)]) for s in special] + [result([N(2), N(3)])]
        add(f"top-{k}", {"top"}, _plain(res), res)
    # ---- the low clamp of v and x: inside (-1, 0) (truncates to -0: bin 0 without the clamp), at -1, far below
    for k, col in (("v", "b1"), ("x", "b2")):
        res = [result([N(4), syl(2, **{col: pair})]) for pair in ([62, 10], [65, 10], [250, 5])] + [result([N(5)])]
        add(f"low-{k}", {"low"}, _plain(res), res)
    # ---- poison: exactly one histogram (or one formant's three) handed out as raw counts, still growing in a later result
    poison = {"d-zero": (syl(3, e1=0.0), set()), "h-zero": (syl(3, e2=0.0), set()),
              "d-quarter": (syl(3, e1=0.25), {"fractional"}), "h-quarter": (syl(3, e2=0.25), {"fractional"}),
              "d-tiny": (syl(3, e1=1e-44), {"fractional"}), "h-tiny": (syl(3, e2=1e-44), {"fractional"}),
              "p-negative": (syl(3, w1=-4), {"synthetic"}), "m-negative": (syl(3, w2=-9), {"synthetic"}),
              "p-nan": (syl(3, w1=float("nan")), {"synthetic"}), "m-nan": (syl(3, w2=float("nan")), {"synthetic"}),
              "udp": (syl(4, b1=0), set()), "fhm": (syl(4, b2=0), set()), "no-frames": (syl(0), {"synthetic"})}
    for name, (s, fam) in poison.items():
        res = [result([N(6), N(7)]), result([N(8), s]), result([N(9)]), result([s, N(10), s])]
        add(f"poison-{name}", {"poison"} | fam, _plain(res), res)
    # ---- below 1 but not poisoned: 3 log10(0.5) and 4 log10(0.75) truncate to -0; a fractional mean energy above 1
    res = [result([N(11), syl(3, e1=0.5, e2=0.75)]), result([syl(2, e1=[1.5, 2.25], e2=[7.75, 1.0]), N(12)])]
    add("below-one", {"fractional"}, _plain(res), res)
    # ---- syllable lengths: every tail of the four-frame trips, alone and with invalid frames at the edges and inside
    def holes(sl, salt):
        s = varied(sl, salt)
        s[3::4, 0] = 0                       # formant 1 missing on the last frame of every trip: the next trip's first frame jumps from 0
        s[1::3, 3] = 0
        return s

    def edge(sl, salt, at):
        s = varied(sl, salt)
        s[at, 0] = s[at, 3] = 0
        return s
    for name, make in (("plain", varied), ("first-invalid", lambda sl, k: edge(sl, k, 0)), ("last-invalid", lambda sl, k: edge(sl, k, -1)), ("holes", holes)):
        res = [result([make(sl, 2 * k), N(13 + k)], lead=k % 2, tail=1 + k % 2) for k, sl in enumerate(LENS)]
        add(f"lengths-{name}", {"lengths"}, _plain(res), res)
    # ---- syllables per result: the 64-lane trips of the syllable loop; the later trips' syllables are longer, so osum and s depend on them
    def many(n, salt):
        return [varied((1 + j % 3) if j < 64 else ((4 + j % 2) if j < 128 else 7), salt + j) for j in range(n)]
    res = [result(many(n, 5 * k), gap=(1, 0, 2), lead=1 if n else 4) for k, n in enumerate(COUNTS)]
    add("counts", {"counts"}, _plain(res), res)
    res = [result(many(n, n), gap=(1,)) for n in (9, 10, 11, 2)]
    add("top-o", {"top"}, _plain(res), res)
    # ---- segment-level histograms through their own entries (frames stay small: length and gap are the entry's)
    R = lambda k: result([N(k), N(k + 1)])
    res = [R(0), R(1), R(2), R(3), R(4)]
    add("top-i", {"top"}, chain([("r", 140, 20), ("r", 150, 20), ("r", 3000, 20), ("r", 149, 20), ("r", 20, 20)]), res)
    add("top-l", {"top"}, chain([("r", 50, 0), ("r", 50, 140), ("r", 50, 150), ("r", 50, 5000), ("r", 50, 149)]), res)
    res = [result([varied(n)]) for n in (39, 42, 100, 40)] + [R(5)]
    add("top-s", {"top"}, chain([("r", 50, 20), ("r", 50, 20), ("r", 10, 20), ("r", 50, 20), ("r", 30, 20)]), res)
    res = [result([varied(n)]) for n in (14, 10, 5)] + [R(6)]
    add("low-s", {"low"}, chain([("r", 50, 20)] * 3 + [("r", 30, 20)]), res)
    # ---- a result without syllables: o takes bin 0, s is clamped up from -6
    res = [R(7), result([], lead=5, tail=0), R(8), result([], lead=0, tail=0)]
    add("no-syllables", {"empty"}, chain([("r", 30, 20), ("r", 45, 20), ("r", 30, 20), ("r", 60, 20)]), res)
    # ---- dropped segments: segments_ci is indexed with the RESULT index behind them
    drops = {"first": "drrr", "middle": "rdrr", "last": "rrrd", "two": "rddrr", "alternating": "drdrdr"}
    lens = (30, 75, 120, 140, 45, 95)
    for name, kinds in drops.items():
        res = [R(9 + k) for k in range(kinds.count("r"))]
        add(f"drop-{name}", {"drop"}, chain([(kd, lens[n], 25 + 40 * n) for n, kd in enumerate(kinds)]), res)
    res = [R(20), R(21), R(22)]
    add("drop-length-0", {"drop"}, chain([("r", 30, 20), ("d", 0, 20), ("r", 75, 20), ("r", 120, 20)]), res)       # result 1 reads the entry of length 0: i bin 0, osum / 0
    add("drop-negative-gap", {"drop"}, chain([("r", 100, 20), ("d", 10, -30), ("r", 75, 40), ("r", 120, 20)]), res)  # result 1: gap -30 -> index -2
    add("drop-small-negative-gap", {"drop"}, chain([("r", 100, 20), ("d", 10, -10), ("r", 75, 40), ("r", 120, 20)]), res)   # gap -10 -> -0: bin 0
    # ---- more results than the streams' history holds entries; an entry that has left the history when its result comes
    res = [result([varied(2 + r % 4, r)]) for r in range(36)]
    add("many-results", {"history"}, chain([("r", 20 + 7 * (r % 11), 10 + 9 * (r % 5)) for r in range(36)]), res)
    res = [R(23), R(24)]
    add("late-entry", {"history", "drop"}, chain([("d", 10 + n, 5) for n in range(33)] + [("r", 30, 20), ("r", 44, 20)]), res)
    res = [R(25), R(26), R(27)]
    add("late-entry-after-results", {"history", "drop"}, chain([("r", 30, 20)] + [("d", 10 + n, 5) for n in range(33)] + [("r", 30, 20), ("r", 44, 20)]), res)
    assert len({c["name"] for c in out}) == len(out)
    return out


CASES = _build()
INDEX = {c["name"]: i for i, c in enumerate(CASES)}
FAMILIES = ("top", "low", "poison", "fractional", "synthetic", "lengths", "counts", "empty", "drop", "history")


def digest(c):
    h = hashlib.sha256(c["name"].encode() + b"\0" + np.array(c["segs"], np.int32).tobytes())
    for r in c["results"]:
        h.update(np.array(r["syl"], np.int32).reshape(-1, 2).tobytes() + b"\1" + r["frames"].tobytes())
    return h.hexdigest()[:16]


def load_golden(path):
    """tests/golden/utterance_expected.json -> ({case name: [results, 264] f64, row k = the reference after results 0 .. k}, {case name: digest})"""
    import json
    import struct
    d = json.load(open(path))
    values = np.array([struct.unpack(">d", bytes.fromhex(h))[0] for h in d["values"]])
    rows, digests = {}, {}
    for g in d["cases"]:
        a = np.zeros((len(g["rows"]), NBINS))
        for k, flat in enumerate(g["rows"]):
            a[k, flat[0::2]] = values[flat[1::2]]
        rows[g["name"]], digests[g["name"]] = a, g["digest"]
    return rows, digests


def result_segment(c, k):
    """index in segs of result k's own entry"""
    return [n for n, s in enumerate(c["segs"]) if s[2] >= 0][k]


def expected_meta(c, k):
    """Y()'s ingredients as K4 leaves them in utt_meta[2:4]: the first entry's start, the lengths summed up to result k's own entry."""
    return c["segs"][0][0], sum(s[1] for s in c["segs"][:result_segment(c, k) + 1])


def oracle_rows(c):
    """[results, 264] from pyoracle.utterance_features, one row per result prefix."""
    from oracle import pyoracle
    segs = [[s[0], s[1]] for s in c["segs"]]
    syl_ci, frames = [r["syl"] for r in c["results"]], [r["frames"] for r in c["results"]]
    return np.array([pyoracle.utterance_features(segs, syl_ci[:k + 1], frames[:k + 1]) for k in range(len(c["results"]))]).reshape(-1, NBINS)


# ---- the fifteen bump arguments of every result, traced (the arithmetic of the reference's b() and _(), in doubles) -------------------------------

def _div(a, b):
    if b == 0:
        return float("nan") if a == 0 or a != a else math.copysign(float("inf"), a)
    return a / b


def bumps(c):
    """per result: [(histogram, argument of parseInt, syllable length | None)] in the kernel's order."""
    from oracle import pyoracle
    L = pyoracle.lib()
    log10 = lambda x: L.wsa_or_log10(float(x)) if x == x else float("nan")
    out = []
    prev_end = c["segs"][0][0]
    for r, res in enumerate(c["results"]):
        seg_start, seg_len, _ = c["segs"][r]                     # the RESULT index
        row, osum = [], 0
        for st, sl in res["syl"]:
            fr = res["frames"][st:st + sl].astype(np.float64)
            a = e1 = w1 = dl1 = c1 = u = e2 = w2 = dl2 = c2 = 0.0
            for o in range(sl):
                F = fr[o]
                if F[0] > 0:
                    c1 += 1; a += F[0]; e1 += F[1]; w1 += F[2]
                    if o > 0:
                        dl1 += F[0] - fr[o - 1][0]
                if F[3] > 0:
                    c2 += 1; u += F[3]; e2 += F[4]; w2 += F[5]
                    if o > 0:
                        dl2 += F[3] - fr[o - 1][3]
            a, e1, w1, u, e2, w2 = _div(a, c1), _div(e1, c1), _div(w1, c1), _div(u, c2), _div(e2, c2), _div(w2, c2)
            e = float(sl)
            for k, x in (("c", e / 2), ("u", a / 2), ("f", u / 2), ("d", 3 * log10(e1)), ("h", 4 * log10(e2)), ("p", w1 / 2), ("m", w2 / 2),
                         ("g", _div(10 * (e - c1), e)), ("y", _div(10 * (e - c2), e)), ("v", 20 * (dl1 + 50) / 100), ("x", 20 * (dl2 + 50) / 100)):
                row.append((k, x, sl))
            osum += sl
        row += [("i", 10 * seg_len / 150, None), ("o", float(len(res["syl"])), None), ("l", 10 * (seg_start - prev_end) / 150, None),
                ("s", 2 * (_div(osum, seg_len) - .3) * 10, None)]
        prev_end = seg_start + seg_len
        out.append(row)
    return out


def check_domain(c):
    """the kernel's documented domain: no finite argument of bump with a magnitude inside (0, 1e-6) or at or above 1e21"""
    for r, row in enumerate(bumps(c)):
        for k, x, _ in row:
            if x == x and abs(x) != float("inf"):
                assert abs(x) == 0 or 1e-6 <= abs(x) < 1e21, (c["name"], r, k, x)


def classify(k, x):
    """what bump does with argument x of histogram k: 'nan' | 'negative' (poison), 'top-1' (one past the last bin) | 'top-far' | 'last' (reached
    unclamped), 'minus-zero' ((-1, 0): bin 0 with or without a clamp), 'low-1' | 'low-far' (clamped up to bin 0), 'inside'"""
    n = SIZES[k]
    if x != x or abs(x) == float("inf"):
        return "nan"
    t = math.trunc(x)
    if t >= n:
        return "top-1" if t == n else "top-far"
    if t == n - 1:
        return "last"
    if t == 0 and (x < 0 or math.copysign(1.0, x) < 0):
        return "minus-zero"
    if t <= -1:
        return ("low-1" if t == -1 else "low-far") if k in LO_CLAMPED else "negative"
    return "inside"


# the paths a case edited later must not silently stop reaching: (histogram, class) -> results at least (tests/test_utterance_reference.py counts them)
MINIMUMS = {(k, cl): 1 for k in ORDER for cl in ("last", "top-1")}
MINIMUMS.update({(k, "top-far"): 1 for k in ORDER if k not in "gy"})
MINIMUMS.update({(k, cl): 1 for k in LO_CLAMPED for cl in ("minus-zero", "low-1", "low-far")})
MINIMUMS.update({(k, "nan"): 2 for k in "ufdhpmgy"})
MINIMUMS.update({(k, "negative"): 2 for k in "dhpm"})
MINIMUMS.update({("s", "nan"): 1, ("l", "negative"): 1})      # the zero-length and negative-gap index shifts
MINIMUMS.update({("d", "minus-zero"): 1, ("h", "minus-zero"): 1, ("l", "minus-zero"): 1})


def path_stats():
    """Counter over all cases: (histogram, class) -> results; ('trips', n) -> results whose syllables take n 64-lane trips; ('sl%4', r) -> syllables;
    ('shifted',) -> results whose entry is not their own; ('raw+normalised',) -> rows with a raw and a normalised histogram side by side;
    ('only', k) -> rows where histogram k alone is raw."""
    st = collections.Counter()
    for c in CASES:
        poisoned = set()
        for r, row in enumerate(bumps(c)):
            seen = set()
            for k, x, sl in row:
                cl = classify(k, x)
                seen.add((k, cl))
                if cl in ("nan", "negative"):
                    poisoned.add(k)
                if k == "c":
                    st[("sl%4", sl % 4)] += 1
            for key in seen:
                st[key] += 1
            st[("trips", (len(c["results"][r]["syl"]) + 63) // 64)] += 1
            st[("shifted",)] += result_segment(c, r) != r
            st[("raw+normalised",)] += 0 < len(poisoned) < len(ORDER)
            if len(poisoned) == 1:
                st[("only", next(iter(poisoned)))] += 1
    return st


# ---- layouts: where the cases sit in the tables of one launch -----------------------------------------------------------------------------------
# Batch: dict(name, geometry "batch", clips [(what, pad)]): what = a case index, None (a clip without segments) or "dropped" (segments, all of them
# dropped: no result), pad = FILL frames in front of the clip's first result.  Stream: dict(name, geometry "stream", ring, streams [script]),
# a script = one entry per step: None (no segment, no START) or (case index, START?, [indices into the case's segs]).

def _interleaved(order):
    clips = []
    for n, ci in enumerate(order):
        if n % 5 == 1:
            clips.append((None, 0))
        if n % 7 == 3:
            clips.append(("dropped", 3))
        clips.append((ci, (0, 2, 5, 1)[n % 4]))
    return clips


def _padded(n_clips, ci):
    """the interleaved launch's head, empty clips up to n_clips, the last one holding case ci"""
    head = _interleaved(list(range(len(CASES))))[:max(0, min(n_clips - 1, 24))]
    return head + [(None, 0)] * (n_clips - 1 - len(head)) + [(ci, 4)]


def splits(c):
    """name -> steps, each a list of indices into the case's segs"""
    n = len(c["segs"])
    each = [[g] for g in range(n)]
    gappy, g, k = [], 0, 0
    while g < n:
        take = (0, 1, 2, 0, 0, 3, 1)[k % 7]
        gappy.append(list(range(g, min(n, g + take))))
        g += take
        k += 1
    return {"each": each, "all": [list(range(n))], "gappy": gappy}


def script(ci, split, delay=0):
    steps = splits(CASES[ci])[split]
    return [None] * delay + [(ci, k == 0, s) for k, s in enumerate(steps)]


def _step_frames(ci, seg_ids):
    c = CASES[ci]
    own = [n for n, s in enumerate(c["segs"]) if s[2] >= 0]
    return sum(len(c["results"][own.index(g)]["frames"]) for g in seg_ids if c["segs"][g][2] >= 0)


def _stream_layout(name, scripts):
    need = max([_step_frames(st[0], st[2]) for sc in scripts for st in sc if st] + [1])
    ring = 64
    while ring < need:
        ring *= 2
    return dict(name=name, geometry="stream", ring=ring, streams=scripts)


SMALL = [i for i, c in enumerate(CASES) if max(len(r["frames"]) for r in c["results"]) <= 64 and c["name"] != "late-entry"]
LOSERS = ("late-entry", "late-entry-after-results")       # their entry has left the 32-deep history when its result comes
ONE_STEP_LOSERS = ("many-results",)                       # more than 32 segments in ONE step: the first results' entries are overwritten before K4 runs


def layouts():
    I = INDEX
    out = [dict(name="batch-one-per-clip", geometry="batch", clips=[(ci, 0) for ci in range(len(CASES))]),
           dict(name="batch-interleaved", geometry="batch", clips=_interleaved(list(reversed(range(len(CASES))))))]
    for n, nm in ((1, "top-d"), (255, "poison-udp"), (256, "drop-two"), (257, "lengths-holes"), (513, "drop-length-0")):
        out.append(dict(name=f"batch-{n}-clips", geometry="batch", clips=_padded(n, I[nm])))
    quiet = [i for i in SMALL if CASES[i]["name"] not in LOSERS]
    # one segment per step (a dropped segment is then a step of its own), ring 64: syllables wrap; an idle stream beside the busy ones
    out.append(_stream_layout("stream-each", [script(ci, "each", delay=n % 3) for n, ci in enumerate(quiet)] + [[None]]))
    # steps of 0 .. 3 segments
    out.append(_stream_layout("stream-gappy", [[None]] + [script(ci, "gappy") for ci in range(len(CASES)) if CASES[ci]["name"] not in LOSERS + ("counts",)]))
    # everything in one step
    out.append(_stream_layout("stream-all", [script(ci, "all", delay=n % 2) for n, ci in enumerate(range(len(CASES))) if CASES[ci]["name"] not in LOSERS + ONE_STEP_LOSERS + ("counts",)]))
    # the longest tables: 129 syllables in a step's result
    out.append(_stream_layout("stream-counts", [script(I["counts"], "each"), [None], script(I["counts"], "gappy")]))
    # START in mid-life: a stream that has run part of one case (or all of it) starts another, which must come out as on a fresh stream
    out.append(_stream_layout("stream-restart", [script(I["poison-udp"], "each")[:3] + script(I["top-l"], "each"),
                                                 script(I["drop-two"], "all") + script(I["poison-d-zero"], "gappy"),
                                                 script(I["many-results"], "gappy")[:20] + [None, None] + script(I["drop-negative-gap"], "each"), [None],
                                                 script(I["top-u"], "each")[:2] + [(I["top-u"], True, [])] + [None] + script(I["no-syllables"], "each")]))
    # entries that have left the history: bit 0 of totals[2]; the other streams of the launch are unharmed
    out.append(_stream_layout("stream-lost", [script(I["late-entry"], "each"), script(I["drop-middle"], "each"), script(I["late-entry-after-results"], "gappy"),
                                              script(I["late-entry"], "all", delay=2), script(I["top-i"], "gappy"), script(I["many-results"], "all", delay=1)]))
    return out


def tables(lay):
    """Batch: one dict(segments, clip_seg_off, row_meta, clip_row_off, formants, frame_off, n_clips, rows_cap, expect [(clip, case index, k)]).
    Stream: a list of such dicts, one per step, with carry [n, CARRY_WORDS], ctl [n] and `lost` (streams whose entry has left the history) besides —
    the state is the caller's to thread through — and `expect` holding that step's rows."""
    if lay["geometry"] == "batch":
        return _batch_tables(lay)
    return _stream_tables(lay)


def _rows_of(c, k, clip, base, seg_index):
    return [(clip, k, st, sl, seg_index, j, base + st, sl) for j, (st, sl) in enumerate(c["results"][k]["syl"])]


def _finish(segs, seg_off, rows, row_off, frames, frame_off, expect, extra):
    t = dict(segments=np.array(segs, np.int32).reshape(-1, 4), clip_seg_off=np.array(seg_off, np.uint32), row_meta=np.array(rows, np.int32).reshape(-1, 8),
             clip_row_off=np.array(row_off, np.uint32), formants=np.ascontiguousarray(np.concatenate(frames + [np.zeros((0, 9), np.float32)]), np.float32),
             frame_off=np.array(frame_off, np.uint32), n_clips=len(seg_off) - 1, rows_cap=len(expect) + extra, expect=expect)
    return t


def _batch_tables(lay):
    segs, rows, frames, expect = [], [], [], []
    seg_off, row_off, frame_off = [0], [0], [0]
    for clip, (what, pad) in enumerate(lay["clips"]):
        nfr = 0
        if what == "dropped":
            segs += [(clip, 10, 30, -1), (clip, 70, 20, -2)]
            frames.append(np.tile(FILL, (pad, 1)))
            nfr = pad
        elif what is not None:
            c = CASES[what]
            frames.append(np.tile(FILL, (pad, 1)))
            nfr, k = pad, 0
            for n, (s, l, f) in enumerate(c["segs"]):
                segs.append((clip, s, l, f))
                if f >= 0:
                    rows += _rows_of(c, k, clip, nfr, n)
                    frames.append(c["results"][k]["frames"])
                    nfr += len(c["results"][k]["frames"])
                    expect.append((clip, what, k))
                    k += 1
        seg_off.append(len(segs)); row_off.append(len(rows)); frame_off.append(frame_off[-1] + nfr)
    return _finish(segs, seg_off, rows, row_off, frames, frame_off, expect, 5)


def _stream_tables(lay):
    ring, n = lay["ring"], len(lay["streams"])
    carry = np.zeros((n, CARRY_WORDS), np.int32)
    rings = [np.tile(FILL, (ring, 1)) for _ in range(n)]
    cursor = [ring * (3 + s) - 7 - 5 * s for s in range(n)]           # a stream's first syllables wrap its ring's end
    kres = [0] * n
    out = []
    for step in range(max(len(sc) for sc in lay["streams"])):
        segs, rows, expect, lost = [], [], [], []
        seg_off, row_off = [0], [0]
        ctl = np.zeros(n, np.uint32)
        for s, sc in enumerate(lay["streams"]):
            st = sc[step] if step < len(sc) else None
            if st:
                ci, start, ids = st
                c = CASES[ci]
                own = [g for g, e in enumerate(c["segs"]) if e[2] >= 0]
                if start:                                             # the gate clears a fresh stream's carry, K4 its state
                    ctl[s] = 1
                    carry[s] = 0
                    kres[s] = 0
                assert _step_frames(ci, ids) <= ring
                before = int(carry[s, 0])
                assert ids == list(range(before, before + len(ids))), (lay["name"], s, step)
                for g in ids:                                         # compact_gather_kernel: the history first, then the counts
                    carry[s, 2 + 2 * (g % CARRY_HIST)], carry[s, 3 + 2 * (g % CARRY_HIST)] = c["segs"][g][0], c["segs"][g][1]
                carry[s, 0] = before + len(ids)
                for g in ids:
                    segs.append((s, ) + c["segs"][g])
                    if c["segs"][g][2] >= 0:
                        k = own.index(g)
                        assert k == kres[s]
                        fr = c["results"][k]["frames"]
                        rings[s][(cursor[s] + np.arange(len(fr))) % ring] = fr
                        rows += _rows_of(c, k, s, cursor[s], g)
                        cursor[s] += len(fr)
                        expect.append((s, ci, k))
                        if int(carry[s, 0]) - k > CARRY_HIST:
                            lost.append(s)
                        kres[s] += 1
                carry[s, 1] = kres[s]
            seg_off.append(len(segs)); row_off.append(len(rows))
        t = _finish(segs, seg_off, rows, row_off, [r.copy() for r in rings], [ring * s for s in range(n + 1)], expect, 3)
        t.update(carry=carry.copy(), ctl=ctl, lost=sorted(set(lost)), ring_mask=ring - 1)
        out.append(t)
    return out


def carry_entry(carry_row, k):
    """[start, len] of segments_ci entry k as a stream's history holds it, None where it has left the history"""
    if int(carry_row[0]) - k > CARRY_HIST:
        return None
    return int(carry_row[2 + 2 * (k % CARRY_HIST)]), int(carry_row[3 + 2 * (k % CARRY_HIST)])

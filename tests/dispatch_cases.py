"""Hand-built segment tables and row pools for K3 (csrc/tracker.hip compact_*), shared by tests/test_dispatch_reference.py (CPU) and
tests/test_gpu_dispatch.py.  A case is a list of clips, a clip a list of segments S(start, len, flag, rows); streams are scripts of steps.  Starts and
lengths are all different, so a timestamp taken from the wrong entry shows; every row carries 53 feature words of its own (NaNs with distinct
payloads, -0.0, denormals among them) and five words that K3 copies through."""
import numpy as np

from tests import dispatch_ref as dr

NFEAT = 53
SEG_START, SEG_LEN, SEG_FBEGIN, SEG_FEND, SEG_CCI, SEG_FLAG, SEG_NROWS, SEG_ROW0 = range(8)
POISON = -77
LEVELS = (5, 13, 10, 4, 3)


def S(start, length, flag=None, rows=1):
    """a segment: flag None = 1 with rows, 0 without (a zero-row result); flag -1 = dropped"""
    return dict(start=start, len=length, flag=(1 if rows else 0) if flag is None else flag, nrows=rows)


def D(start, length, rows=0):
    """a dropped segment; rows > 0: its table entry names pool rows all the same (K3 goes by the flag)"""
    return S(start, length, -1, rows)


def feature_bits(row_id):
    """the 53 u64 words of row `row_id`: every word differs from every other row's"""
    j = np.arange(NFEAT, dtype=np.uint64)
    tag = (np.uint64(row_id) << np.uint64(8)) | j
    kind = row_id % 5
    if kind == 0:
        w = np.uint64(0x7ff8000000000000) | tag                                  # quiet NaNs, payload = the row and the slot
    elif kind == 1:
        w = np.uint64(0xfff0000000000000) | (tag + np.uint64(1))                 # signalling NaNs, negative
    elif kind == 2:
        w = tag + np.uint64(1)                                                   # denormals
    else:
        w = (tag * np.uint64(0x9e3779b97f4a7c15)) ^ np.uint64(0x3ff0000000000000)
    w = w.copy()
    w[3] = np.uint64(0x8000000000000000) if row_id % 2 else w[3]                 # -0.0
    return w


class Builder:
    """numbers the rows of the cases it finishes: ids are unique inside one builder"""
    def __init__(self):
        self.next_id = 0

    def finish(self, segs):
        """segments S(..) -> the segments tests/dispatch_ref.py takes (rows numbered; pos filled in by tables())"""
        out = []
        for sg in segs:
            rows = []
            for j in range(sg["nrows"]):
                i = self.next_id
                self.next_id += 1
                rows.append(dict(id=i, w=((i * 7) % 50, (i * 3) % 20 + 1, j, 1000 + i, (i * 3) % 20 + 1), pos=-1))
            out.append(dict(start=sg["start"], len=sg["len"], flag=sg["flag"], rows=rows))
        return out


def _numbered(clips):
    b = Builder()
    return [b.finish(c) for c in clips]


def _segs(n, base, drops=(), empty=(), rows=1):
    """n segments with starts base + 40 k and lengths 11 + k: those in `drops` dropped, those in `empty` zero-row results"""
    return [D(base + 40 * k, 11 + k) if k in drops else S(base + 40 * k, 11 + k, rows=0 if k in empty else rows) for k in range(n)]


BATCH = {
    "all-reported": [[S(10, 30), S(50, 21, rows=2), S(90, 15)]],
    "drop-first": [[D(3, 9), S(20, 31), S(60, 17, rows=2)], [S(7, 8)]],
    "drop-middle": [[S(4, 12), D(30, 13), S(55, 14, rows=3), S(80, 16)]],
    "drop-last": [[S(5, 19), S(31, 18), D(70, 22)], [S(9, 6, rows=2)]],
    "two-adjacent-drops": [[S(6, 10), D(25, 11), D(44, 12), S(63, 13), S(82, 14, rows=2)]],
    "two-separate-drops": [[D(2, 5), S(15, 6), D(28, 7), S(41, 8), S(54, 9)]],
    "every-segment-dropped": [[S(1, 2)], [D(8, 20), D(40, 21), D(70, 23)], [S(3, 4, rows=2)]],
    "dropped-with-rows": [[S(8, 9), D(30, 10, rows=2), S(50, 11, rows=2), S(70, 12)]],
    "zero-row-alone": [[S(5, 9, rows=0)]],
    "zero-row-before-drop": [[S(5, 9, rows=0), D(20, 10), S(35, 11), S(50, 12, rows=2)]],
    "zero-row-after-drop": [[D(5, 9), S(20, 10, rows=0), S(35, 11), S(50, 12, rows=2)]],
    "zero-rows-only-beside-a-drop": [[S(5, 9, rows=0), D(20, 10), S(35, 11, rows=0)], [S(2, 3)]],
    "empty-clip-between": [[S(10, 30, rows=2)], [], [S(50, 21)], [], []],
    "rows-per-segment": [[S(10, 30, rows=1), S(50, 21, rows=63), D(90, 15), S(130, 16, rows=64), S(170, 17, rows=65), S(210, 18, rows=130)], [S(1, 2, rows=65)]],
    "segments-63": [_segs(63, 5, drops=(0, 31, 62), empty=(1, 40))],
    "segments-64": [_segs(64, 6, drops=(63,), empty=(62,)), [S(9, 9)]],
    "segments-65": [[S(4, 4)], _segs(65, 7, drops=(1, 2, 64), empty=(0, 63))],
    "segments-130": [_segs(130, 8, drops=(5, 64, 65, 128), empty=(66, 129), rows=2), [D(1, 2)], [S(3, 3)]],
}
# every case again with ONE row per result, as levels 5 and 4 have it (a result there is one row; a zero-row result does not occur)
TWINS = {k + "-one-row": _numbered([[dict(sg, nrows=1 if sg["flag"] >= 0 else sg["nrows"]) for sg in clip] for clip in v]) for k, v in BATCH.items() if k != "rows-per-segment"}
BATCH = {k: _numbered(v) for k, v in BATCH.items()}
POOL_ORDERS = ("segment", "reversed", "shuffled")
# the composite case for the permuted pools (the tracker finishes spans longest first: the pool is never in segment order)
EVERYTHING = _numbered([c for name in ("drop-first", "two-adjacent-drops", "zero-row-before-drop", "empty-clip-between", "dropped-with-rows", "segments-65")
                        for c in [[dict(sg, nrows=len(sg["rows"])) for sg in clip] for clip in BATCH[name]]])

# span (SEG_FEND - SEG_FBEGIN, by the oracle's record under gate_cases' common settings) -> frames of designed_clip("long_voiced", frames) that give it
LONG_FRAMES = {2046: 2058, 2047: 2059, 2048: 2060, 2580: 2592}
CLIP_COUNTS = (1, 2, 63, 64, 65, 128, 129, 1023, 1024, 1025, 2048, 2049, 4096, 4097)


def generated(n, seed):
    """n clips of 0 .. 2 segments of 0 .. 3 rows, one segment in six dropped; the last clips are never empty (the scan's last threads have work)"""
    rng = np.random.default_rng(seed)
    clips = []
    for c in range(n):
        ns = int(rng.integers(0, 3)) if c < n - 2 else 2
        segs = []
        for k in range(ns):
            start, length = int(rng.integers(0, 5000)), int(rng.integers(1, 400))
            if rng.integers(0, 6) == 0:
                segs.append(D(start, length, rows=int(rng.integers(0, 2))))
            else:
                segs.append(S(start, length, rows=int(rng.integers(0, 4))))
        clips.append(segs)
    return _numbered(clips)


def tables(clips_per_step, pool_order="shuffled", seg_cap=None, seed=1):
    """clips_per_step: [per step [per clip its (numbered) segments]] (a batch: one step).  Lays the rows out in ONE pool — segments in `pool_order`, a
    poisoned row between some — fills in every row's pos, and returns dict(seg_i [steps, n, seg_cap, 8], seg_count [steps, n], meta_in [pool, 8],
    feat_in [pool, 53] u64, clip_rows [steps, n]).  Table slots past a clip's count hold POISON."""
    steps, n = len(clips_per_step), len(clips_per_step[0])
    cap = seg_cap or max(1, max(len(c) for st in clips_per_step for c in st)) + 1
    order = [(t, c, k) for t, st in enumerate(clips_per_step) for c, clip in enumerate(st) for k in range(len(clip))]
    if pool_order == "reversed":
        order.reverse()
    elif pool_order == "shuffled":
        order = [order[i] for i in np.random.default_rng(seed).permutation(len(order))]
    else:
        assert pool_order == "segment"
    seg_i = np.full((steps, n, cap, 8), POISON, np.int32)
    seg_count = np.zeros((steps, n), np.uint32)
    clip_rows = np.zeros((steps, n), np.uint32)
    meta, feat = [], []
    poison_meta, poison_feat = np.full(8, POISON, np.int32), np.full(NFEAT, 0xdeadbeefdeadbeef, np.uint64)
    for q, (t, c, k) in enumerate(order):
        sg = clips_per_step[t][c][k]
        if q % 3 == 1:
            meta.append(poison_meta); feat.append(poison_feat)
        seg_i[t, c, k] = [sg["start"], sg["len"], POISON, POISON, POISON, sg["flag"], len(sg["rows"]), len(meta)]
        for r in sg["rows"]:
            r["pos"] = len(meta)
            a, b, w5, w6, w7 = r["w"]
            meta.append(np.array([c, POISON, a, b, k, w5, w6, w7], np.int32))
            feat.append(feature_bits(r["id"]))
    for t, st in enumerate(clips_per_step):
        for c, clip in enumerate(st):
            seg_count[t, c] = len(clip)
            clip_rows[t, c] = sum(len(sg["rows"]) for sg in clip if sg["flag"] >= 0)
    return dict(seg_i=seg_i, seg_count=seg_count, meta_in=np.array(meta, np.int32).reshape(-1, 8), feat_in=np.array(feat, np.uint64).reshape(-1, NFEAT),
                clip_rows=clip_rows)


def expected_arrays(ref_tables, rows_cap=None):
    """a step's tables of dispatch_ref as arrays: meta [rows, 8], feat [rows, 53] u64, seg [segs, 4], row_off, seg_off"""
    rows = [r for clip in ref_tables["rows"] for r in clip]
    meta = np.array([r[0] for r in rows], np.int32).reshape(-1, 8)
    feat = np.array([feature_bits(r[1]) for r in rows], np.uint64).reshape(-1, NFEAT)
    return dict(meta=meta, feat=feat, seg=np.array(ref_tables["seg_out"], np.int32).reshape(-1, 4),
                row_off=np.array(ref_tables["row_off"], np.uint32), seg_off=np.array(ref_tables["seg_off"], np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------------ streams
# one launch's segment list: drops early, in a pair, and late; zero-row results; 40 segments, so a deal into one step holds more than 32
LAUNCH = [D(3, 7) if k in (1, 7, 8, 30) else S(3 + 50 * k, 7 + k, rows=0 if k in (2, 9, 31) else 1 + k % 3) for k in range(40)]


def deal(segs, how):
    """a (numbered) segment list as a stream's script of steps (None: an idle step)"""
    n = len(segs)
    if how == "all":
        return [segs]
    if how == "each":
        return [[sg] for sg in segs]
    if how == "gappy":                              # steps of 0 .. 3 segments, idle ones between
        out, k, q = [], 0, 0
        while k < n:
            take = (0, 3, 1, 0, 0, 2)[q % 6]
            out.append(segs[k:k + take] or None)
            k += take; q += 1
        return out
    if how == "halves":                             # 35 segments, then the rest: the second step's results straddle seg_before
        return [segs[:35], segs[35:]]
    raise ValueError(how)


def script_steps(scripts, starts=None):
    """scripts: per stream its steps ([segments] or None); START with the first step (or where `starts` says: {(stream, step)}).  -> the steps
    dispatch_ref.streams() takes"""
    n, n_steps = len(scripts), max(len(s) for s in scripts)
    steps = []
    for t in range(n_steps):
        segs = [(sc[t] if t < len(sc) and sc[t] else []) for sc in scripts]
        ctl = [1 if (t == 0 or (starts and (s, t) in starts)) else 0 for s in range(n)]
        steps.append(dict(segs=segs, ctl=ctl))
    return steps


def _lost_script(b, drops, results=40, lost_rows=1):
    """`drops` dropped segments in the first step, `results` results in the second: the first drops - CARRY_HIST of them have lost their entry, the
    next ones read the history, the last ones straddle into the step's own table.  The lost ones have `lost_rows` rows (0: a lost result
    that shows in the flag alone), the others two."""
    first = b.finish([D(10 + 13 * k, 3 + k) for k in range(drops)])
    gone = max(drops - dr.CARRY_HIST, 0)
    second = b.finish([S(2000 + 17 * k, 90 + k, rows=lost_rows if k < gone else 2) for k in range(results)])
    return [first, second]


def stream_cases():
    """name -> dict(steps, n): the steps of dispatch_ref.streams()"""
    out = {}
    for how in ("all", "each", "gappy", "halves"):                      # the same launch dealt four ways
        b = Builder()
        out["deal-" + how] = dict(steps=script_steps([deal(b.finish(LAUNCH), how)]), n=1)
    b = Builder()
    # a drop in step 1, later results straddling seg_before inside one step: timestamps from the history and from the step's own table
    out["straddle"] = dict(steps=script_steps([[b.finish([S(5, 6), D(30, 7), S(60, 8)]), b.finish([S(100, 9, rows=2), S(140, 10), D(180, 11), S(220, 12)]),
                                                None, b.finish([S(300, 13), S(340, 14, rows=0), S(380, 15)])],
                                               [None, b.finish([S(1, 1)])]]), n=2)
    # more than 32 segments after an early drop: the slot read has wrapped
    b = Builder()
    wrap = b.finish([D(9, 4)] + [S(20 + 30 * k, 5 + k) for k in range(70)])
    out["wrapped-slot"] = dict(steps=script_steps([deal(wrap, "gappy"), deal(b.finish([D(9, 4)] + [S(21 + 30 * k, 6 + k) for k in range(70)]), "each")]), n=2)
    # START in mid-life, STOP (bit 1: K3 does not look at it), streams that idle throughout
    b = Builder()
    a, c = b.finish([S(5, 6), D(30, 7), S(60, 8), S(90, 9)]), b.finish([D(7, 3), S(40, 4), S(80, 5, rows=2)])
    st = script_steps([[a[:2], a[2:], c[:1], c[1:]], [None], [c[:2], None, None, a]], starts={(0, 2), (2, 3)})
    st[3]["ctl"][0] |= 2
    out["restart"] = dict(steps=st, n=3)
    out["idle-throughout"] = dict(steps=[dict(segs=[[], []], ctl=[1, 0]), dict(segs=[[], []], ctl=[0, 0]), dict(segs=[[], []], ctl=[2, 1])], n=2)
    for drops in (32, 33, 34):                                           # 32: the oldest entry is the history's last; 33, 34: one, two results lost
        b = Builder()
        quiet = b.finish(_segs(20, 700, drops=(3,), rows=2))
        out[f"stream-lost-{drops}"] = dict(steps=script_steps([_lost_script(b, drops), deal(quiet, "all") + [None], [None, deal(quiet, "all")[0]]]), n=3)
    b = Builder()                                                        # the one lost result has no rows: nothing is left out, the flag must still come
    out["stream-lost-33-empty"] = dict(steps=script_steps([_lost_script(b, 33, lost_rows=0), [None, b.finish(_segs(6, 900, drops=(2,)))]]), n=2)
    return out


def stream_counts_case(n, seed):
    """n streams, three steps of generated segments with a START in mid-life for every fifth stream"""
    per_step = [generated(n, seed + t) for t in range(3)]
    b = Builder()
    steps = []
    for t, clips in enumerate(per_step):
        segs = [b.finish([dict(sg, nrows=len(sg["rows"])) for sg in clip]) for clip in clips]
        steps.append(dict(segs=segs, ctl=[1 if (t == 0 or (t == 2 and s % 5 == 0)) else 0 for s in range(n)]))
    return dict(steps=steps, n=n)


def oracle_out(segs, level):
    """a clip's segments as the `out` dict pyoracle.callbacks() takes; the feature rows are the rows' 53 words"""
    out = dict(segments_ci=[[sg["start"], sg["len"]] for sg in segs], flags=[sg["flag"] for sg in segs], syllables_ci=[], features=[], formants=[])
    for sg in segs:
        if sg["flag"] < 0:
            out["syllables_ci"].append(None); out["features"].append(None); out["formants"].append(None)
            continue
        out["syllables_ci"].append([[r["w"][0], r["w"][1]] for r in sg["rows"]])
        ft = [feature_bits(r["id"]).view(np.float64) for r in sg["rows"]]
        out["features"].append(ft if level == 13 else (ft[0] if ft else None))
        out["formants"].append(None)
    return out

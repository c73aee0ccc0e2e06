"""The dispatcher's bookkeeping, restated from the reference's text — NOT from csrc/tracker.hip — for K3's tests (tests/test_dispatch_reference.py,
tests/test_gpu_dispatch.py).

The reference keeps, per launch, the list u of segments_ci entries [start, len] and one list of results (d at level 5, p at 13, h at 10, c at 4,
s at 3).  A segment is pushed to u BEFORE its straighten step runs (@B27240), so a segment whose straighten step throws stays in u without a result.
The dispatcher P() (dist/main.js:2 @B28869) walks the RESULT list: `e = callbacks_processed - 1` is the result index, zero-length results advance it
without a callback, and the timestamps come from u[e] — V(e) = [u[e][0] * step, (u[e][1] + 1) * step] (@B31504) for the segment form, j(e) =
[(u[e][0] + syl[r][0]) * step, (syl[r][1] + 1) * step] per syllable (@B31114) for levels 10 / 12 / 13 (@B29138 / @B29622).  After a dropped segment
u[e] is an EARLIER segment's entry than the result's own: reproduced, not repaired.

Here the integers only: per clip (or stream) the rows of the compacted table [clip, e, t_start, t_len, segment index, ...copied words], the segment
table, the offsets and totals.  Two forms for streams:

  streams()        the launch-long lists u and the result count, cut into steps: START empties them, an idle step leaves them alone, a result whose
                   entry u[e] lies more than CARRY_HIST segments behind the step's first segment is `lost` (a 32-deep history cannot hold it)
  streams_carry()  the same bookkeeping on a CARRY_HIST-deep ring [segments so far, results so far, CARRY_HIST x (start, len)], the form a device
                   has to keep; tests/test_dispatch_reference.py shows it equal to streams() and takes the modelled faults

A segment here is dict(start, len, flag, rows=[dict(id, w=(a, b, w5, w6, w7), pos)]): flag < 0 = dropped; a row's a / b are the syllable's start
and length inside its segment (ignored by the segment form), w5 .. w7 words that are copied through, id names its 53 feature words, pos its place in
the row pool (only the `pool-order` fault looks at it).  Every comparison counts its arm in ARMS."""
from collections import Counter

CARRY_HIST = 32
CARRY_WORDS = 2 + 2 * CARRY_HIST
SYLLABLE_LEVELS = (10, 13)

ARM_NAMES = ["flag.dropped", "flag.reported", "rows.none", "rows.some", "entry.own", "entry.earlier", "form.syllable", "form.segment",
             "clip.empty", "clip.segments", "start.yes", "start.no", "step.idle", "step.busy", "where.step", "where.history", "where.lost"]
ARMS = Counter()

# one-line faults the cases must notice (tests/test_dispatch_reference.py test_the_cases_notice_every_modelled_fault)
LIST_FAULTS = ["own-entry", "si-skips-empty", "dropped-rows-counted", "syllable-no-start", "pool-order", "carry-across-start"]
CARRY_FAULTS = ["mod-31", "history-always", "lost-ge", "carry-across-start"]


def _rows_of(clip, e, entry, seg_index, sg, level, fault):
    out = []
    syl = level in SYLLABLE_LEVELS
    ARMS["form.syllable" if syl else "form.segment"] += 1
    for r in sg["rows"]:
        a, b, w5, w6, w7 = r["w"]
        if syl:
            t0, t1 = (entry[0] if fault != "syllable-no-start" else 0) + a, b          # j(e) @B31114
        else:
            t0, t1 = entry[0], entry[1]                                                 # V(e) @B31504
        out.append(((clip, e, t0, t1, seg_index, w5, w6, w7), r["id"], r["pos"]))
    return out


def _walk(clip, u, nres, segs, level, fault):
    """one clip's / one step's segments: u (the launch's entries so far) grows by them, returns (rows, results after, rows the offsets count,
    results [(result index, its rows)] in the order of the walk, zero-row results included)"""
    first = len(u)
    for sg in segs:
        u.append((sg["start"], sg["len"]))
    rows, counted, results = [], 0, []
    for k, sg in enumerate(segs):
        if sg["flag"] < 0:
            ARMS["flag.dropped"] += 1
            if fault == "dropped-rows-counted":
                counted += len(sg["rows"])
            continue
        ARMS["flag.reported"] += 1
        ARMS["rows.some" if sg["rows"] else "rows.none"] += 1
        if fault == "si-skips-empty" and not sg["rows"]:
            continue
        e = nres                                                                        # callbacks_processed - 1
        ARMS["entry.own" if e == first + k else "entry.earlier"] += 1
        entry = u[e] if fault != "own-entry" else u[first + k]
        rows += _rows_of(clip, e, entry, first + k, sg, level, fault)
        results.append((e, len(sg["rows"])))
        counted += len(sg["rows"])
        nres += 1
    if fault == "pool-order":
        rows.sort(key=lambda r: r[2])
    return rows, nres, counted, results


def _tables(per_clip_rows, per_clip_counted, per_clip_segs):
    row_off, seg_off, seg_out, rows = [0], [0], [], []
    for c, (r, n, segs) in enumerate(zip(per_clip_rows, per_clip_counted, per_clip_segs)):
        rows.append(r)
        row_off.append(row_off[-1] + n)
        seg_off.append(seg_off[-1] + len(segs))
        seg_out += [(c, sg["start"], sg["len"], sg["flag"]) for sg in segs]
    return dict(rows=rows, row_off=row_off, seg_off=seg_off, seg_out=seg_out, totals=(row_off[-1], seg_off[-1]))


def batch(clips, level, fault=None):
    """clips: per clip its segments.  dict(rows [per clip [(meta8, id, pos)]] — clip c's rows sit from row_off[c] on —, row_off, seg_off [n + 1],
    seg_out [(clip, start, len, flag)], totals (rows, segments))"""
    per_rows, per_counted = [], []
    for c, segs in enumerate(clips):
        ARMS["clip.segments" if segs else "clip.empty"] += 1
        rows, _, counted, _ = _walk(c, [], 0, segs, level, fault)
        per_rows.append(rows); per_counted.append(counted)
    return _tables(per_rows, per_counted, clips)


def _ring_of(u):
    ring = [0] * (2 * CARRY_HIST)
    for g, (s, l) in enumerate(u):
        ring[2 * (g % CARRY_HIST)], ring[2 * (g % CARRY_HIST) + 1] = s, l
    return ring


def streams(steps, n, level, fault=None):
    """steps: [dict(segs [per stream its segments of the step], ctl [per stream, bit 0 START])].  Per step the tables of batch() (row meta's segment
    index counts from the launch's first segment), lost = {(stream, index among the stream's rows of the step)}, lost_flag, carry [n][CARRY_WORDS]"""
    u = [[] for _ in range(n)]
    nres = [0] * n
    out = []
    for st in steps:
        per_rows, per_counted, lost, lost_flag = [], [], set(), False
        for s in range(n):
            start = bool(st["ctl"][s] & 1)
            ARMS["start.yes" if start else "start.no"] += 1
            if start and fault != "carry-across-start":
                u[s], nres[s] = [], 0
            segs = st["segs"][s]
            ARMS["step.busy" if segs else "step.idle"] += 1
            before = len(u[s])
            rows, nres[s], counted, results = _walk(s, u[s], nres[s], segs, level, fault)
            i = 0
            for e, nr in results:                                       # per RESULT: one without rows whose entry is gone raises the flag all the same
                where = "where.step" if e >= before else ("where.lost" if before - e > CARRY_HIST else "where.history")
                ARMS[where] += 1
                if where == "where.lost":
                    lost_flag = True
                    lost.update((s, i + q) for q in range(nr))
                i += nr
            per_rows.append(rows); per_counted.append(counted)
        t = _tables(per_rows, per_counted, st["segs"])
        t.update(lost=lost, lost_flag=lost_flag, carry=[[len(u[s]), nres[s]] + _ring_of(u[s]) for s in range(n)])
        out.append(t)
    return out


def streams_carry(steps, n, level, fault=None, carry_in=None):
    """streams() on the ring a device keeps: cy = [segments so far, results so far, CARRY_HIST x (start, len)] per stream.  A lost result's time
    columns hold whatever the ring holds in its slot."""
    cy = [list(carry_in[s]) if carry_in is not None else [0] * CARRY_WORDS for s in range(n)]
    out = []
    for st in steps:
        per_rows, per_counted, lost = [], [], set()
        for s in range(n):
            if (st["ctl"][s] & 1) and fault != "carry-across-start":
                cy[s] = [0] * CARRY_WORDS
            segs = st["segs"][s]
            seg_before, res_before = cy[s][0], cy[s][1]
            rows, si = [], 0
            for k, sg in enumerate(segs):
                if sg["flag"] < 0:
                    continue
                e = res_before + si
                if e >= seg_before and fault != "history-always":
                    entry = (segs[e - seg_before]["start"], segs[e - seg_before]["len"])
                else:
                    gone = seg_before - e >= CARRY_HIST if fault == "lost-ge" else seg_before - e > CARRY_HIST
                    slot = e % (CARRY_HIST - 1) if fault == "mod-31" else e % CARRY_HIST
                    entry = (cy[s][2 + 2 * slot], cy[s][3 + 2 * slot])
                    if gone:
                        lost.update((s, len(rows) + i) for i in range(len(sg["rows"])))
                        if not sg["rows"]:
                            lost.add((s, -1 - k))                       # a lost result without rows still raises the flag
                rows += _rows_of(s, e, entry, seg_before + k, sg, level, None)
                si += 1
            for k, sg in enumerate(segs):
                g = seg_before + k
                cy[s][2 + 2 * (g % CARRY_HIST)], cy[s][3 + 2 * (g % CARRY_HIST)] = sg["start"], sg["len"]
            cy[s][0], cy[s][1] = seg_before + len(segs), res_before + si
            per_rows.append(rows); per_counted.append(len(rows))
        t = _tables(per_rows, per_counted, st["segs"])
        t.update(lost={x for x in lost if x[1] >= 0}, lost_flag=bool(lost), carry=[list(c) for c in cy])
        out.append(t)
    return out

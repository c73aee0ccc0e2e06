"""Hand-built steps for the stream step's feature-DB kernels (specification FD-2; csrc/stream_featdb.hip), each on one
edge: row counts around the wave tile and the 1024-row walk, level-12 marks on both sides of those seams, the capacity decision, and
level 11's one-row-per-launch rule.  A case is dict(level, capacity, start, n_streams, steps); a step is dict(meta, feat, utt_off,
bits, flags).  `start` rows are in the DB before the first step (initial() makes them and the pattern the rest of the DB holds, so
that a stray write shows).  Everything is generated from small integers; nothing is recorded from a run."""
import numpy as np

from tests import featdb_cases as fc

START, STOP, ACTIVE = 1, 2, 4                            # the device control word's bits
ROW_COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025)


def _step(meta=None, feat=None, utt_off=None, bits=None, flags=0):
    return dict(meta=meta, feat=feat, utt_off=None if utt_off is None else np.array(utt_off, np.uint32),
                bits=None if bits is None else np.array(bits, np.uint32), flags=flags)


def _case(level, capacity, steps, start=0, n_streams=0):
    return dict(level=level, capacity=capacity, start=start, n_streams=n_streams, steps=steps)


def initial(case):
    """(pattern [capacity][width] the DB holds before anything, head [start][width] = its first rows before the first step)"""
    width = {5: 53, 13: 53, 11: 264, 12: 23}[case["level"]]
    return fc.feature_table(case["capacity"], width, 90), fc.feature_table(case["start"], width, 91)


def l12_table(n, run, marks, seed=11, stream_of=lambda cb: cb // 7):
    """n rows in callbacks of `run` rows each, (stream, si) = (cb // 7, cb % 7) by default, slot 23 = the entries of marks {row: value}, 0 elsewhere"""
    keys = [(stream_of(r // run), (r // run) % 7) for r in range(n)]
    feat = fc.feature_table(n, 53, seed) if n else np.zeros((0, 53))
    if n:
        feat[:, 23] = 0.0
    for r, v in marks.items():
        feat[r, 23] = v
    return fc.meta_table(keys), feat


def rows_case(level, n, spare=2, start=3):
    """one step of n rows into a DB with `spare` rows more room than it needs; level 12: callbacks of five rows, every 13th marked on its
    second row, so that fewer rows are kept than walked"""
    if level == 12:
        meta, feat = l12_table(n, 5, {r: 1.0 for r in range(1, n, 65)})
    else:
        meta, feat = fc.meta_table([(r // 9, r % 9 // 3) for r in range(n)]), (fc.feature_table(n, 53, 12) if n else np.zeros((0, 53)))
    return _case(level, start + n + spare, [_step(meta, feat)], start=start)


def all_kept_case(n, start=1):
    """level 12, n rows none marked: the copy kernel moves exactly n rows through a list"""
    meta, feat = l12_table(n, 3, {})
    return _case(12, start + n + 1, [_step(meta, feat)], start=start)


def _l12_small(name):
    meta, feat = fc.l12_small(name)
    return _case(12, 9, [_step(meta, feat)], start=1)


def _two_steps(level, n1, n2, capacity, flags2=0, start=0):
    mk = (lambda n, s: l12_table(n, 4, {2: 1.0} if n > 2 else {}, seed=s)) if level == 12 else \
         (lambda n, s: (fc.meta_table([(r // 4, 0) for r in range(n)]), fc.feature_table(n, 53, s)))
    (m1, f1), (m2, f2), (m3, f3) = mk(n1, 21), mk(n2, 22), mk(1, 23)
    return _case(level, capacity, [_step(m1, f1), _step(m2, f2, flags=flags2), _step(m3, f3)], start=start)


def _utt(n, seed):
    return fc.feature_table(n, 264, seed) if n else np.zeros((0, 264))


def _l11(capacity, steps, n_streams, start=0):
    """steps: [(counts per stream, bits per stream, flags)]"""
    out = []
    for k, (counts, bits, flags) in enumerate(steps):
        off = np.concatenate([[0], np.cumsum(counts)])
        out.append(_step(None, _utt(int(off[-1]), 30 + k), off, bits, flags))
    return _case(11, capacity, out, start=start, n_streams=n_streams)


A, SA, PA = ACTIVE, START | ACTIVE, STOP | ACTIVE


def _l11_many(n_streams):
    """more streams than one step of the plan kernel's walk: results in a fixed cycle, a second step that replaces, restarts and adds"""
    c1 = [(0, 1, 2, 1, 0, 3)[i % 6] for i in range(n_streams)]
    c2 = [(1, 0, 1, 2, 0, 1, 1)[i % 7] for i in range(n_streams)]
    b1 = [SA] * n_streams
    b2 = [SA if i % 5 == 0 else (0 if i % 7 == 4 else A) for i in range(n_streams)]
    new2 = sum(1 for i in range(n_streams) if c2[i] and (i % 5 == 0 or not c1[i]))
    return _l11(2 + sum(1 for c in c1 if c) + new2 + 1, [(c1, b1, 0), (c2, b2, 0)], n_streams, start=2)


CASES = {}
for _n in ROW_COUNTS:
    CASES[f"rows13_{_n}"] = (lambda n=_n: rows_case(13, n))
    CASES[f"rows12_{_n}"] = (lambda n=_n: rows_case(12, n))
CASES.update({
    "rows5_65": lambda: rows_case(5, 65),
    # level-12 marks.  Callbacks of five rows: rows 60 .. 64 and 1020 .. 1024 lie across the seams
    "l12_mark_last_row_of_wave": lambda: _case(12, 140, [_step(*l12_table(130, 5, {63: 1.0}))]),                   # drops 63 and, through the wave's carry, 64
    "l12_mark_first_row_of_next_wave": lambda: _case(12, 140, [_step(*l12_table(130, 5, {64: 2.0}))]),             # drops 64 only
    "l12_mark_first_row_of_wave_and_callback": lambda: _case(12, 140, [_step(*l12_table(130, 4, {64: 1.0}))]),     # rows 64 .. 67 are one callback: all dropped
    "l12_mark_before_walk_seam": lambda: _case(12, 1040, [_step(*l12_table(1030, 5, {1023: 1.0}))], start=2),      # drops 1023 and, through the walk's carry, 1024
    "l12_mark_behind_walk_seam": lambda: _case(12, 1040, [_step(*l12_table(1030, 5, {1024: 1.0}))]),
    "l12_mark_first_row_behind_walk_seam": lambda: _case(12, 1040, [_step(*l12_table(1030, 4, {1024: 1.0}))]),     # rows 1024 .. 1027 all dropped
    "l12_mark_carried_over_two_waves": lambda: _case(12, 300, [_step(*l12_table(256, 200, {10: 1.0}))]),           # one callback of 200 rows marked early, then one of 56
    "l12_marked_first_row_of_callback": lambda: _l12_small("mark_first"),
    "l12_nan_and_minus_zero": lambda: _l12_small("nan_marks"),
    "l12_all_marked": lambda: _l12_small("all_marked"),
    "l12_same_si_two_streams": lambda: _l12_small("same_si_two_clips"),
    # the capacity decision: three steps each — the second is the one on the edge, the third (one row) shows what came of it
    "fit_exact_13": lambda: _two_steps(13, 5, 7, 12),
    "fit_one_too_many_13": lambda: _two_steps(13, 5, 7, 11),
    "capacity_flag_13": lambda: _two_steps(13, 5, 7, 20, flags2=1),
    "fit_exact_12": lambda: _two_steps(12, 6, 70, 2 + 4 + 68, start=2),      # (each table loses the two rows from its mark on)
    "fit_one_too_many_12": lambda: _two_steps(12, 6, 70, 2 + 4 + 67, start=2),
    "capacity_flag_12": lambda: _two_steps(12, 6, 70, 100, flags2=1),
    "fit_flags_other_bits_13": lambda: _two_steps(13, 5, 7, 20, flags2=8),                                          # a flags word without bit 0 stores
    # level 11
    "l11_first_result": lambda: _l11(4, [([1, 0, 0], [SA, SA, SA], 0)], 3, start=1),
    "l11_two_results_last_wins": lambda: _l11(4, [([2, 0, 1], [SA, SA, SA], 0), ([3, 0, 0], [A, A, A], 0)], 3),
    "l11_result_on_start_step": lambda: _l11(4, [([1, 0, 0], [SA, SA, SA], 0), ([1, 0, 0], [SA, A, A], 0)], 3),
    "l11_stop_then_start": lambda: _l11(5, [([1, 1], [SA, SA], 0), ([1, 0], [PA, A], 0), ([0, 1], [0, A], 0), ([1, 0], [SA, A], 0), ([1, 1], [A, A], 0)], 2),
    "l11_start_without_result": lambda: _l11(4, [([1, 1], [SA, SA], 0), ([0, 1], [SA, A], 0), ([1, 0], [A, A], 0)], 2),
    "l11_idle_between_active": lambda: _l11(4, [([1, 0, 2], [SA, 0, SA], 0), ([1, 0, 1], [A, 0, A], 0), ([0, 1, 0], [A, SA, A], 0)], 3),
    "l11_exact_fit": lambda: _l11(3, [([1, 1, 0], [SA, SA, SA], 0), ([0, 0, 1], [A, A, A], 0), ([1, 1, 1], [A, A, A], 0)], 3),
    "l11_no_room_for_one_new_row": lambda: _l11(2, [([1, 1, 0], [SA, SA, SA], 0), ([1, 1, 1], [A, A, A], 0), ([2, 1, 0], [A, A, A], 0)], 3),
    "l11_full_step_start_still_forgets": lambda: _l11(2, [([1, 1], [SA, SA], 0), ([1, 1], [SA, A], 0), ([0, 1], [A, A], 0)], 2),
    "l11_capacity_flag": lambda: _l11(4, [([1, 1], [SA, SA], 0), ([1, 1], [SA, A], 1), ([1, 1], [A, A], 0)], 2),
    "l11_63_streams": lambda: _l11_many(63),
    "l11_65_streams": lambda: _l11_many(65),
    "l11_1025_streams": lambda: _l11_many(1025),
})

# every arm of tests/stream_featdb_ref.py that some case above must take
ARMS = ["all_rows", "capacity_flag", "fits", "fits_exactly", "full", "full_with_replacements", "nothing_to_store",
        "l12_mark", "l12_mark_nan", "l12_minus_zero", "l12_mark_on_first_row", "l12_mark_later", "l12_dropped",
        "l11_start_with_row", "l11_start_without_row", "l11_idle_stream", "l11_several_results", "l11_new_row", "l11_replaced"]

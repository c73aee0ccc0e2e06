"""The class fold K6b / K6b-e (csrc/classify_fold.hpp) on its own, through the test entry wsa_debug_class_fold (csrc/debug_fold.hip): the
hand-built cases of tests/fold_cases.py straight into the product's fold launches — fold_kernel<float> and <double> with
fold_compact_kernel, fold_group_kernel with fold_compact_group_kernel, and on streams stream_classes_kernel, stream_knn_kernel and
stream_fold_group_kernel with stream_decide_kernel — against the float64 restatements (tests/classify_ref.py, tests/ensemble_ref.py, pinned
to the reference's prediction.js by tests/test_fold_reference.py) fed the same confidences.  NO tolerance: labels, callback records, counts
and min_entropy_db as integers, every double by its bits, NaNs included.  Also: a case gives the same bits at any clip index, clip count,
row offset and split into steps; slots beyond the callback count keep the caller's sentinel; a member's figures inside a group equal its
single-model run; what would index outside the tables is refused.

Counts: 33 cases of tests/fold_cases.py (27 named, 6 of sizes: callbacks of 1, 2, 63, 64, 65 and 130 rows; 1, 2, 63 and 64 classes) in 125
tests.  Batch layouts: six clips per case (a filler, a clip without rows, the case twice, a filler, no rows) and 1, 3, 4, 5, 1023, 1024, 1025 and
2049 clips (the largest about 2 500 rows) per family; stream layouts: three streams, the case dealt into 1, 2 and K steps (one launch per step),
0 / 63 / 64 / 65 / 130 rows in front of a stream, D2H windows of 0, 1, 4, 5 and 64 callbacks.  About 450 calls of the entry and 1 500 kernel
launches (counted without the refusal test); the file takes under 4 s on an MI355X (the slowest test 0.2 s, the first one 1.5 s to load the library).

Mutation table: each row is a scratch build of csrc/classify_fold.hpp with ONE value changed (never an index or a bound), run once through
this file on an MI355X (the counts are of the 123 tests the file had before sum-ties-strings-two-singles came, the stamp row of all 125);
"before" is the library as it stood before this file (NaN rows ranked all 0, array indices parsed up to 2^31 - 1).

    build                                               fails   which
    before (both divergences unfixed)                      10   case_in_a_batch / case_on_streams [present-nan, all-nan-row-single(-index), all-nan-row-ensemble,
                                                                index-2-31, index-2-31-ensemble]  (all-nan-row-single: on streams only, see below)
    `pj == pf && j < lane` -> `j > lane`                   76   the rank-ties, all-nan and sum-ties cases, and every layout test (their fillers hold no tie: present-zero does)
    `acc_seg != 0.0 &&` dropped                             0   EQUIVALENT: a present 0 is +0 (a product of non-negative factors), and 0 + w == w bit for bit for every
    `a.acc_all != 0.0 &&` dropped                           0   w, NaN included; assignment and addition cannot differ.  The arm is still counted (FOLD_ARMS seg.zero, all.zero)
    `acc_seg == acc_seg` dropped                            2   present-nan (batch, streams)
    `a.acc_all == a.acc_all` dropped                       10   present-nan and the four all-nan-row cases (batch, streams)
    `nsyl > 1 ||` dropped                                 115   everything with a callback of several syllables
    `a.first = a.stamp` without `+ rank`                   14   fixed3-ties-0.1ms, sum-ties-strings, index-2-31-ensemble, ensemble-identical, long-callbacks, classes-63,
                                                                idle_start_in_mid_life_and_stop[float, double]
    `a.stamp += C` inside `if (add)`                        3   sum-ties-strings-two-singles (batch, streams: the case added for this mutant, which only
                                                                fixed3-ties-0.1ms on streams caught before), fixed3-ties-0.1ms on streams
    fixed3's correction loop removed                        2   fixed3-ties-0.1ms (95 and 115 steps of 0.1 ms: 1000 x rounds onto the tie from below)
    `f.seg > best` -> `>=`                                 40   every group test that holds a callback without a winner or a tie between members
    `am > max_inv` -> `>=`                                 35   the same for min_entropy_db
    all_sum added in lane order                            13   entropy-order, sum-ties-index, rank-ties-reversed-keys, index-2-31-ensemble, ensemble-identical, ...
    compact_offsets' `- v` dropped                         86   every batch test with more than one clip (the stream kernels have no compaction)

With the unfixed library all-nan-row-single passes in the batch layout: a NaN under a key is overwritten like an absent key, so the three extra
keys the old ranking inserted leave the clip's final sums and (here) the labels as they were; they show in a stream's sums after the step, and in
all-nan-row-single-index, whose last callback is NaN again."""
import numpy as np
import pytest

from tests import fold_cases as F
from webspeechanalyzer_amd import capi

pytestmark = pytest.mark.gpu

ACTIVE, START, STOP = capi.ACTIVE, capi.START, capi.STOP
SENT = -7
ALL = F.CASES + F.SIZE_CASES
FAMILIES = ("float", "double", "group")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _conf_as_sent(conf, family):
    """the confidences as the family's kernels read them, as doubles"""
    return [np.asarray(c, np.float64) if family == "double" else np.asarray(c, np.float32).astype(np.float64) for c in conf]


def _call(meta, row_off, step_s, legends, conf, family, **kw):
    return capi.debug_class_fold(meta, row_off, step_s, legends, conf, single=family != "group", f64=family == "double", sentinel=SENT, **kw)


def _families(case):
    if len(case["legends"]) > 1:
        return ("group",)
    return ("double",) if case["dtype"] == "f64" else FAMILIES


def _check_rows(out, rows, lo, M, group, where=""):
    """the device's callback tables [lo, lo + len(rows)) against the restatement's rows, bit for bit"""
    hi = lo + len(rows)
    assert [tuple(r) for r in out["cb"][lo:hi]] == [r["cb"] for r in rows], where
    for d in range(M):
        assert list(out["cb_label"][d][lo:hi]) == [r["label"][d] for r in rows], (where, d)
        assert np.array_equal(_bits(out["cb_conf"][d][lo:hi]), _bits([r["conf"][d] for r in rows])), (where, d)
        if group:
            assert np.array_equal(_bits(out["cb_all_max"][d][lo:hi]), _bits([r["all_max"][d] for r in rows])), (where, d)
    if group:
        for key, name in (("cb_db", "db"), ("cb_top_label", "top_label"), ("cb_min_db", "min_db")):
            assert list(out[key][lo:hi]) == [r[name] for r in rows], (where, key)
        for key, name in (("cb_top_conf", "top_conf"), ("cb_entropy", "entropy")):
            assert np.array_equal(_bits(out[key][lo:hi]), _bits([r[name] for r in rows])), (where, key)


def _check_sentinel(out, n, M, group, prefix=""):
    """slots beyond the n callbacks written keep the caller's sentinel"""
    assert (out[prefix + "cb"].reshape(-1, 4)[n:] == SENT).all()
    for d in range(M):
        assert (out[prefix + "cb_label"][d].reshape(-1)[n:] == SENT).all() and (out[prefix + "cb_conf"][d].reshape(-1)[n:] == SENT).all()
        if group:
            assert (out[prefix + "cb_all_max"][d].reshape(-1)[n:] == SENT).all()
    if group:
        for key in ("cb_db", "cb_top_label", "cb_top_conf", "cb_min_db", "cb_entropy"):
            assert (out[prefix + key].reshape(-1)[n:] == SENT).all(), key


def _run_batch(launches, family):
    """a batch of launches (None: a clip without rows) through the family's kernels, checked against the restatement; returns (out, R)"""
    first = next(l for l in launches if l is not None)
    legends, M, group = first["legends"], len(first["legends"]), family == "group"
    meta, row_off, conf, _ = F.batch_tables(launches)
    out = _call(meta, row_off, first["step_s"], legends, conf, family)
    R = F.restate_batch(meta, row_off, _conf_as_sent(conf, family), legends, first["step_s"])
    assert out["n_cb"] == len(R.rows)
    _check_rows(out, R.rows, 0, M, group)
    _check_sentinel(out, len(R.rows), M, group)
    for d in range(M):
        assert np.array_equal(_bits(out["run_conf"][d]), _bits(R.sums(d))), d
    if group:
        assert list(out["run_min_db"]) == list(R.min_db())
    return out, R


def _clip_slice(out, R, clip, M, group):
    """what a clip's callbacks hold, without the clip index and the row offset"""
    idx = [i for i, r in enumerate(R.rows) if r["cb"][0] == clip]
    first_row = R.rows[idx[0]]["cb"][2] if idx else 0
    cb = [(int(out["cb"][i][1]), int(out["cb"][i][2]) - first_row, int(out["cb"][i][3])) for i in idx]
    cols = [out["cb_label"][d][idx] for d in range(M)] + [_bits(out["cb_conf"][d][idx]) for d in range(M)]
    cols += [_bits(out["run_conf"][d][clip]) for d in range(M)]
    if group:
        cols += [_bits(out["cb_all_max"][d][idx]) for d in range(M)]
        cols += [out[k][idx] for k in ("cb_db", "cb_top_label", "cb_min_db")] + [_bits(out[k][idx]) for k in ("cb_top_conf", "cb_entropy")]
        cols.append(out["run_min_db"][clip:clip + 1])
    return cb, [np.asarray(c).tolist() for c in cols]


def test_entry_is_exported_but_no_part_of_the_abi():
    assert hasattr(capi.lib(), "wsa_debug_class_fold") and "wsa_debug_class_fold" not in capi.ABI_SYMBOLS


@pytest.mark.parametrize("name", [c["name"] for c in ALL])
def test_case_in_a_batch(name):
    """every case in every kernel family it applies to, between a filler clip, a clip without rows and a second copy of itself: the two
    copies hold the same bits.  A member of an ensemble case folds alone (single-model kernels) to the figures it has inside the group."""
    case = F.BY_NAME[name]
    M = len(case["legends"])
    for family in _families(case):
        launches = [F.filler_case(case, 0), None, case, F.filler_case(case, 1), case, None]
        out, R = _run_batch(launches, family)
        assert _clip_slice(out, R, 2, M, family == "group") == _clip_slice(out, R, 4, M, family == "group")
        if M > 1:
            for d in range(M):
                o1, _ = _run_batch([None if l is None else F.member_case(l, d) for l in launches], "float")
                assert list(o1["cb_label"][0][:o1["n_cb"]]) == list(out["cb_label"][d][:out["n_cb"]])
                assert np.array_equal(_bits(o1["cb_conf"][0][:o1["n_cb"]]), _bits(out["cb_conf"][d][:out["n_cb"]]))
                assert np.array_equal(_bits(o1["run_conf"][0]), _bits(out["run_conf"][d]))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n_clips", [1, 3, 4, 5, 1023, 1024, 1025, 2049])
def test_clip_counts(n_clips, family):
    """clip counts around fold_kernel's four clips per workgroup and compact_offsets' 1024 per scan pass; clips without rows at the front, in
    the middle and at the end; most clips hold one one-row callback, a few the named cases (the largest layout: 2049 clips, about 2500 rows)"""
    base = F.BY_NAME["all-zero-row" if family == "group" else "present-zero"]
    long = F.BY_NAME["long-callbacks"]
    launches = [F.filler_case(base, i) for i in range(n_clips)]
    spots = sorted({0, n_clips // 2, n_clips - 1})
    for i in spots:
        launches[i] = base
    if n_clips >= 5:
        launches[0] = launches[n_clips // 2 + 1] = launches[n_clips - 1] = None
        launches[1] = launches[n_clips - 2] = base
        if family != "group" and n_clips > 1000:
            launches[n_clips // 3] = long
            launches[1022 if n_clips > 1023 else 7] = base
    out, R = _run_batch(launches, family)
    M, group = len(base["legends"]), family == "group"
    holders = [i for i, l in enumerate(launches) if l is base]
    ref = _clip_slice(out, R, holders[0], M, group)
    for i in holders[1:]:
        assert _clip_slice(out, R, i, M, group) == ref, i


# ---- streams
def _run_steps(launches, plan, family, cap=0):
    """launches dealt into steps by plan through the family's step kernels, every step checked against the restatement; returns (out, steps)"""
    first = next(l for l in launches if l is not None)
    legends, M, group = first["legends"], len(first["legends"]), family == "group"
    meta, row_off, ctl, conf = F.deal_steps(launches, plan)
    out = _call(meta, row_off, first["step_s"], legends, conf, family, ctl=ctl, cap=cap)
    steps = F.restate_steps(meta, row_off, ctl, _conf_as_sent(conf, family), legends, first["step_s"])
    lo, W = 0, max(cap, 1)
    for k, st in enumerate(steps):
        n = len(st["rows"])
        assert out["n_cb"][k] == n, k
        _check_rows(out, st["rows"], lo, M, group, f"step {k}")
        for d in range(M):
            assert np.array_equal(_bits(out["run_conf"][d][k]), _bits(st["sums"][d])), (k, d)
        if group:
            assert list(out["run_min_db"][k]) == list(st["min_db"]), k
        # the D2H window: the step's first `cap` callbacks, nothing else
        below = min(n, cap)
        h = {key[2:]: ([a[k] for a in v] if isinstance(v, list) else v[k]) for key, v in out.items() if key.startswith("h_")}
        _check_rows(h, st["rows"][:below], 0, M, group, f"step {k} window")
        _check_sentinel(h, below, M, group)
        lo += n
    _check_sentinel(out, lo, M, group)
    return out, steps


def _flat(out, steps, M, group, s):
    """stream s's callbacks over all steps, without row offsets, and its sums after the last step"""
    idx, lo = [], 0
    for st in steps:
        idx += [lo + i for i, r in enumerate(st["rows"]) if r["cb"][0] == s]
        lo += len(st["rows"])
    cols = [[(int(out["cb"][i][1]), int(out["cb"][i][3])) for i in idx]]
    cols += [out["cb_label"][d][idx].tolist() for d in range(M)] + [_bits(out["cb_conf"][d][idx]).tolist() for d in range(M)]
    cols += [_bits(out["run_conf"][d][-1][s]).tolist() for d in range(M)]
    if group:
        cols += [_bits(out["cb_all_max"][d][idx]).tolist() for d in range(M)]
        cols += [out[k][idx].tolist() for k in ("cb_db", "cb_top_label", "cb_min_db")] + [_bits(out[k][idx]).tolist() for k in ("cb_top_conf", "cb_entropy")]
        cols.append(int(out["run_min_db"][-1][s]))
    return cols


def _deal(n_cb, n_steps):
    """n_cb callbacks over n_steps steps, as evenly as they go"""
    return [n_cb // n_steps + (1 if k < n_cb % n_steps else 0) for k in range(n_steps)]


@pytest.mark.parametrize("name", [c["name"] for c in ALL])
def test_case_on_streams(name):
    """every case on streams in every family: its callbacks in one step, in two and one per step give the same bits and leave the same
    carried sums, the ones the batch kernels give; a filler stream in front, a copy of the case behind it that starts a step late"""
    case = F.BY_NAME[name]
    M, K = len(case["legends"]), len(case["callbacks"])
    fill = dict(F.filler_case(case, 2), callbacks=[F.filler_case(case, i)["callbacks"][0] for i in range(K + 1)])
    for family in _families(case):
        group = family == "group"
        flats = []
        for n_steps in sorted({1, min(2, K), K}):
            take = _deal(K, n_steps)
            plan = []
            for k in range(n_steps + 1):
                a = take[k] if k < n_steps else 0
                b = take[k - 1] if k >= 1 else 0
                plan.append([(1, ACTIVE | (START if k == 0 else 0)), (a, ACTIVE | (START if k == 0 else 0) | (STOP if k == n_steps - 1 else 0)),
                             (b, (ACTIVE if b else 0) | (START if k == 1 else 0))])
            out, steps = _run_steps([fill, case, case], plan, family, cap=3)
            flats.append((_flat(out, steps, M, group, 1), _flat(out, steps, M, group, 2)))
            assert flats[-1][0] == flats[-1][1]
        assert all(f == flats[0] for f in flats)
        ob, Rb = _run_batch([case], family)
        n = ob["n_cb"]
        assert flats[0][0][1:1 + M] == [ob["cb_label"][d][:n].tolist() for d in range(M)]
        assert flats[0][0][1 + M:1 + 2 * M] == [_bits(ob["cb_conf"][d][:n]).tolist() for d in range(M)]
        assert flats[0][0][1 + 2 * M:1 + 3 * M] == [_bits(ob["run_conf"][d][0]).tolist() for d in range(M)]


# (the many-row callbacks are a one-model case; the group's callback_starts is the same function)
@pytest.mark.parametrize("front,family", [(fr, fam) for fam in FAMILIES for fr in (0, 63, 64, 65, 130, "long") if (fr, fam) != ("long", "group")])
def test_rows_in_front_of_a_stream(front, family):
    """callback_starts' ballot loop: 0, 63, 64, 65 and 130 one-row callbacks in front of the stream within the step, and callbacks of up to
    130 rows there (starts are fewer than rows)"""
    case = F.BY_NAME["all-zero-row" if family == "group" else "present-zero"]
    if front == "long":
        ahead, n_front = F.BY_NAME["long-callbacks"], len(F.BY_NAME["long-callbacks"]["callbacks"])
    else:
        n_front = front
        ahead = dict(F.filler_case(case, 0), callbacks=[F.filler_case(case, i)["callbacks"][0] for i in range(max(front, 1))])
    K = len(case["callbacks"])
    plan = [[(n_front, ACTIVE | START), (2, ACTIVE | START), (1, ACTIVE | START)],
            [(0, 0), (K - 2, ACTIVE), (K - 1, ACTIVE | STOP)]]
    out, steps = _run_steps([ahead, case, case], plan, family, cap=n_front + 1)
    M = len(case["legends"])
    assert _flat(out, steps, M, family == "group", 1) == _flat(out, steps, M, family == "group", 2)


@pytest.mark.parametrize("family", FAMILIES)
def test_idle_start_in_mid_life_and_stop(family):
    """a stream that is never started, START in mid-life (every member's sums and the group's max_inv / min_entropy_db begin again), STOP,
    and steps in which nothing arrives"""
    case = F.BY_NAME["ensemble-allmax-tie" if family == "group" else "sum-ties-strings-earlier-single"]
    other = F.BY_NAME["ensemble-seg-tie-cb3" if family == "group" else "sum-ties-strings"]
    assert case["legends"] == other["legends"]
    plan = [[(2, ACTIVE | START), (0, 0), (0, 0)],
            [(1, ACTIVE), (1, ACTIVE | START), (0, 0)],
            [(0, 0), (0, ACTIVE), (0, 0)],
            [(2, ACTIVE | START), (1, ACTIVE | STOP), (0, 0)],
            [(0, START), (0, 0), (0, 0)],
            [(1, ACTIVE), (0, 0), (0, STOP)]]
    out, steps = _run_steps([case, other, case], plan, family, cap=2)
    M = len(case["legends"])
    for d in range(M):
        assert not out["run_conf"][d][:, 2].any()                       # the stream that never ran: zero sums throughout
        assert not out["run_conf"][d][4, 0].any()                       # START without rows forgets the launch
    if family == "group":
        assert (out["run_min_db"][:, 2] == -1).all() and out["run_min_db"][4, 0] == -1 and out["run_min_db"][3, 0] >= 0


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("cap", [0, 1, 4, 5, 64])
def test_d2h_window(cap, family):
    """the D2H window at 0, inside a step (inside a stream's callbacks and between two streams), at the step's count and above it"""
    case = F.BY_NAME["all-zero-row" if family == "group" else "present-zero"]
    K = len(case["callbacks"])
    plan = [[(K, ACTIVE | START), (K, ACTIVE | START)], [(1, ACTIVE | START), (K, ACTIVE | START | STOP)]]
    _run_steps([case, case], plan, family, cap=cap)


def test_refusals():
    """whatever would make a kernel read or write outside the tables is refused before anything runs"""
    case = F.BY_NAME["present-zero"]
    meta, row_off, conf, _ = F.batch_tables([case, F.filler_case(case, 0)])
    args = dict(step_s=case["step_s"], legends=case["legends"], conf=conf, family="float")
    _call(meta, row_off, **args)

    def refused(m=meta, off=row_off, **kw):
        with pytest.raises(capi.WsaError):
            _call(m, off, **{**args, **kw})
    bad = row_off.copy(); bad[1] = row_off[2] + 1
    refused(off=bad)                                                    # offsets out of order
    bad = row_off.copy(); bad[2] -= 1
    refused(off=bad)                                                    # rows beyond the last offset
    for slot, v in ((0, 1), (3, -1), (3, 0x7fffffff), (1, -1)):         # a row of another clip; t_len negative or INT32_MAX; si negative
        m = meta.copy(); m[0, slot] = v
        refused(m=m)
    refused(cb_cap=len(case["callbacks"]))                              # more callbacks than the tables hold
    refused(legends=[[str(i) for i in range(65)]], conf=[np.zeros((len(meta), 65))])           # more than 64 classes
    refused(legends=case["legends"] * 2, conf=conf * 2)                 # the single-model kernels take one member
    refused(legends=case["legends"] * 9, conf=conf * 9, family="group")
    with pytest.raises(capi.WsaError):                                   # double confidences are the single fold's
        capi.debug_class_fold(meta, row_off, case["step_s"], case["legends"], conf, single=False, f64=True)
    # streams: a callback whose rows are split across two steps
    m2, off2, ctl2, conf2 = F.deal_steps([case], [[(1, ACTIVE | START)], [(1, ACTIVE)]])
    first = int(off2[0][1])
    off_split = np.array([[0, first - 1], [0, int(off2[1][1]) + 1]], np.uint32)
    with pytest.raises(capi.WsaError):
        capi.debug_class_fold(m2, off_split, case["step_s"], case["legends"], conf2, single=True, ctl=ctl2, cap=4)
    capi.debug_class_fold(m2, off2, case["step_s"], case["legends"], conf2, single=True, ctl=ctl2, cap=4)

"""K3 (csrc/tracker.hip compact_count_kernel, compact_scan_kernel<COUNT>, compact_gather_kernel<FUSED>, launch_compact) and the span order
(span_order_kernel + the gate's counting, GateParams::span_hist / span_key) on their own (-m gpu): the hand-built tables of tests/dispatch_cases.py
through the test entries wsa_debug_compact (csrc/debug_rows.hip) / wsa_debug_span_order (csrc/debug_gate.hip) against the dispatcher's restatement tests/dispatch_ref.py, which
tests/test_dispatch_reference.py holds to the reference.  Integers and bit copies: every comparison is on bits, nothing has a tolerance.  The one thing
left out: columns 2 and 3 of rows whose segments_ci entry has left the streams' 32-deep history, in the stream-lost-* cases of tests/dispatch_cases.py only
(the stream layouts of tests/utterance_cases.py are held to the ring form of the restatement, every word).

Kernel mutations, each built once into a scratch copy of the library and run against this file (no mutated code is kept); the named test is one that fails:

    mutation (csrc/tracker.hip unless said otherwise)                                   a test that fails
    ts / tl from entry k instead of the result index gsi                                test_batch_cases[drop-first-fused]
    si++ moved inside `nr > 0`                                                          test_batch_cases[zero-row-before-drop-fused]
    the fused prefix sum starts at lane 1 (i = lane + 1)                                test_batch_cases[drop-first-fused]
    `per` rounded down in compact_scan_kernel                                           test_clip_counts[1025-unfused]
    `n_clips <= 2 * CSCAN_T` -> `<`                                                     test_clip_counts[2048-unfused]
    the read slot `gsi % CARRY_HIST` -> `gsi % (CARRY_HIST - 1)`                        test_stream_cases[wrapped-slot]
    `seg_before - gsi > CARRY_HIST` -> `>=`                                             test_stream_cases[stream-lost-32]
    the bucket clamp SPAN_BUCKETS - 1 -> SPAN_BUCKETS - 2 (csrc/gate.hip, both kernels) test_span_order[257-integer-runs]
    `order[offs[e.x] + e.y]` without `+ e.y`                                            test_span_order[257-integer-runs]
"""
import os
import sys

import numpy as np
import pytest

from tests import dispatch_cases as dc
from tests import dispatch_ref as dr
from tests import gate_cases as gc
from tests import utterance_cases as uc
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = -7
SENT_U = np.uint32(SENT & 0xffffffff)
SENT_64 = np.uint64((int(SENT_U) << 32) | int(SENT_U))
BATCHES = dict(dc.BATCH, **dc.TWINS)
STREAMS = dc.stream_cases()


@pytest.fixture(scope="module")
def wsa():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import webspeechanalyzer_amd as w
    return w


@pytest.fixture(scope="module")
def capi(wsa):
    from webspeechanalyzer_amd import capi
    return capi


def _expected_path(capi, n, fused, carry=False):
    if fused and not carry and n <= 4096:
        return capi.COMPACT_FUSED
    return capi.COMPACT_SCAN if n <= 2048 else capi.COMPACT_COUNT_SCAN


def _check_tables(what, got_meta, got_feat, got_seg, got_row_off, got_seg_off, ref, lost=()):
    """one step's (or a batch's) tables against the restatement's, the untouched rest against the sentinel"""
    e = dc.expected_arrays(ref)
    nr, ns = len(e["meta"]), len(e["seg"])
    assert np.array_equal(got_row_off, e["row_off"]), f"{what}: clip_row_off"
    assert np.array_equal(got_seg_off, e["seg_off"]), f"{what}: clip_seg_off"
    assert np.array_equal(got_seg[:ns], e["seg"]) and np.all(got_seg[ns:] == SENT), f"{what}: segments"
    meta, want = got_meta[:nr].copy(), e["meta"].copy()
    if lost:
        base = {s: int(ref["row_off"][s]) for s, _ in lost}
        for s, i in lost:
            meta[base[s] + i, 2:4] = 0; want[base[s] + i, 2:4] = 0
    bad = np.argwhere(meta != want)
    assert len(bad) == 0, f"{what}: row meta differs first at (row, word) {bad[:4].tolist()}: got {meta[bad[0][0]].tolist()} want {want[bad[0][0]].tolist()}"
    assert np.all(got_meta[nr:] == SENT), f"{what}: a row past the table was written"
    bad = np.argwhere(got_feat[:nr] != e["feat"])
    assert len(bad) == 0, f"{what}: feature words differ first at (row, word) {bad[:4].tolist()}"
    assert np.all(got_feat[nr:] == SENT_64), f"{what}: feature words past the table were written"
    return nr, ns


def _run_batch(capi, clips, level, fused, pool_order="shuffled", **kw):
    t = dc.tables([clips], pool_order)
    out = capi.debug_compact(t["seg_i"][0], t["seg_count"][0], t["meta_in"], t["feat_in"], level, fused=fused, clip_rows=t["clip_rows"][0], sentinel=SENT, **kw)
    return out


def _check_batch(capi, what, out, clips, level, fused, cleared=False):
    assert out["path"] == _expected_path(capi, len(clips), fused), f"{what}: path {out['path']}"
    ref = dr.batch(clips, level)
    nr, ns = _check_tables(what, out["row_meta_out"], out["row_feat_out"], out["seg_out"], out["clip_row_off"], out["clip_seg_off"], ref)
    assert (nr, ns) == ref["totals"]
    if not cleared:
        assert out["totals"][:2].tolist() == [nr, ns], f"{what}: totals {out['totals']}"
    return nr, ns


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_batch_cases(capi, name, fused):
    clips = BATCHES[name]
    for level in dc.LEVELS:
        out = _run_batch(capi, clips, level, fused)
        _check_batch(capi, f"{name} L{level}", out, clips, level, fused)
        assert out["totals"][2:].tolist() == [0, SENT_U] and np.all(out["counters"] == SENT_U) and np.all(out["hist"] == SENT_U) and np.all(out["host4"] == SENT_U)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("order", dc.POOL_ORDERS)
def test_a_pool_filled_in_another_order_than_the_segments(capi, order, fused):
    for level in (5, 13):
        out = _run_batch(capi, dc.EVERYTHING, level, fused, pool_order=order)
        _check_batch(capi, f"everything {order} L{level}", out, dc.EVERYTHING, level, fused)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("n", dc.CLIP_COUNTS)
def test_clip_counts(capi, n, fused):
    """the path launch_compact takes is asserted at every count (fused up to 4096 clips, the counting scan up to 2048, count + scan above), and every
    path gives the restatement's tables"""
    clips = dc.generated(n, 100 + n)
    for level in (5, 13):
        out = _run_batch(capi, clips, level, fused)
        nr, ns = _check_batch(capi, f"{n} clips L{level}", out, clips, level, fused)
        assert n < 3 or (nr > 0 and ns > nr // 3)


@pytest.mark.parametrize("mode", ["clr+host", "host", "clr", "neither", "unfused"])
def test_the_fused_forms_extras(capi, mode):
    """the four host words = {rows, segments, flag word, totals[3]}; with clr_counters the seeded counters, totals and histogram read zero afterwards, without
    they read as seeded; the unfused paths touch none of them"""
    clips = dc.EVERYTHING
    counters = (np.arange(16, dtype=np.uint32) + 1) * np.uint32(0x01010101)
    totals = np.array([0xa1, 0xa2, 0xa3, 0xa4], np.uint32)
    hist = (np.arange(capi.SPAN_BUCKETS, dtype=np.uint32) * np.uint32(2654435761)) | np.uint32(1)
    fused, clr, host = mode != "unfused", mode in ("clr+host", "clr"), mode in ("clr+host", "host")
    for n_clips in (len(clips), 1):
        cl = clips[:n_clips]
        out = _run_batch(capi, cl, 13, fused, counters=counters, totals=totals, hist=hist, give_clr=clr or not fused, give_host=host or not fused)
        nr, ns = _check_batch(capi, mode, out, cl, 13, fused, cleared=fused and clr)
        if fused and host:
            assert out["host4"].tolist() == [nr, ns, int(counters[1]), 0xa4], out["host4"]
        else:
            assert np.all(out["host4"] == SENT_U)
        if fused and clr:
            assert not out["counters"].any() and not out["totals"].any() and not out["hist"].any()
        else:
            assert np.array_equal(out["counters"], counters) and np.array_equal(out["hist"], hist) and out["totals"].tolist() == [nr, ns, 0xa3, 0xa4]


# ---------------------------------------------------------------------------------------------------------------------------------- streams
def _run_streams(capi, case, level, carry_in=None):
    t = dc.tables([st["segs"] for st in case["steps"]])
    ctl = np.array([st["ctl"] for st in case["steps"]], np.uint32)
    return capi.debug_compact(t["seg_i"], t["seg_count"], t["meta_in"], t["feat_in"], level, ctl=ctl, carry_in=carry_in, sentinel=SENT)


def _check_streams(capi, name, out, case, level, may_lose=False, ring=False):
    """against the launch-long lists (dr.streams): the time columns of lost rows left out, which only a case named for it may have (may_lose).
    ring: against the ring form (dr.streams_carry), where a lost row's time columns are the slot's contents — every word compared"""
    lists = dr.streams(case["steps"], case["n"], level)
    ref = dr.streams_carry(case["steps"], case["n"], level) if ring else lists
    for k, r in enumerate(ref):
        what = f"{name} L{level} step {k}"
        assert out["path"][k] == _expected_path(capi, case["n"], True, carry=True), what
        assert (may_lose or not r["lost"]) and r["lost"] == lists[k]["lost"] and r["lost_flag"] == lists[k]["lost_flag"], what
        nr, ns = _check_tables(what, out["row_meta_out"][k], out["row_feat_out"][k], out["seg_out"][k], out["clip_row_off"][k], out["clip_seg_off"][k], r,
                               lost=() if ring else sorted(r["lost"]))
        assert out["totals"][k].tolist() == [nr, ns, 1 if r["lost_flag"] else 0, SENT_U], f"{what}: totals {out['totals'][k]}"
        assert np.array_equal(out["carry"][k], np.array(r["carry"], np.int32)), f"{what}: carry"
    assert np.all(out["counters"] == SENT_U) and np.all(out["hist"] == SENT_U) and np.all(out["host4"] == SENT_U)
    return ref


@pytest.mark.parametrize("name", list(STREAMS))
def test_stream_cases(capi, name):
    """per step the tables, the lost flag (totals[2] & 1, in exactly the steps the restatement says) and the carry words"""
    case = STREAMS[name]
    for level in (5, 13, 10):
        _check_streams(capi, name, _run_streams(capi, case, level), case, level, may_lose=name.startswith("stream-lost-"))


def _stream_concat(out, n_steps):
    meta, feat, seg = [], [], []
    for k in range(n_steps):
        nr, ns = int(out["clip_row_off"][k][-1]), int(out["clip_seg_off"][k][-1])
        meta.append(out["row_meta_out"][k][:nr]); feat.append(out["row_feat_out"][k][:nr]); seg.append(out["seg_out"][k][:ns])
    return np.concatenate(meta), np.concatenate(feat), np.concatenate(seg)


@pytest.mark.parametrize("level", [5, 13])
def test_one_launch_dealt_four_ways(capi, level):
    """the concatenated step outputs are equal for every deal, and equal the batch tables of the same list (apart from the offsets)"""
    b = dc.Builder()
    clips = [b.finish(dc.LAUNCH)]
    bo = _run_batch(capi, clips, level, True)
    nr, ns = _check_batch(capi, "the launch as a batch", bo, clips, level, True)
    for how in ("all", "each", "gappy", "halves"):
        case = STREAMS["deal-" + how]
        meta, feat, seg = _stream_concat(_run_streams(capi, case, level), len(case["steps"]))
        assert np.array_equal(meta, bo["row_meta_out"][:nr]) and np.array_equal(feat, bo["row_feat_out"][:nr]) and np.array_equal(seg, bo["seg_out"][:ns]), how


@pytest.mark.parametrize("n", [1, 65, 2049])
def test_stream_counts(capi, n):
    """2049 streams: compact_count_kernel + compact_scan_kernel<false> with the carry"""
    case = dc.stream_counts_case(n, 40 + n)
    _check_streams(capi, f"{n} streams", _run_streams(capi, case, 13), case, 13)


def _uc_case(steps):
    """the stream tables of tests/utterance_cases.py (K3's OUTPUT as a host model writes it) turned back into K3's input"""
    b = dc.Builder()
    n = steps[0]["n_clips"]
    out = []
    for t in steps:
        segs = []
        for s in range(n):
            a, e = int(t["clip_seg_off"][s]), int(t["clip_seg_off"][s + 1])
            before = int(t["carry"][s, 0]) - (e - a)
            rows = t["row_meta"][int(t["clip_row_off"][s]):int(t["clip_row_off"][s + 1])]
            mine = []
            for k in range(e - a):
                _, start, length, flag = (int(x) for x in t["segments"][a + k])
                r = [m for m in rows if int(m[4]) == before + k]
                sg = b.finish([dc.S(start, length, flag=flag, rows=len(r))])[0]
                for row, m in zip(sg["rows"], r):
                    row["w"] = (int(m[2]), int(m[3]), int(m[5]), int(m[6]), int(m[7]))
                mine.append(sg)
            segs.append(mine)
        out.append(dict(segs=segs, ctl=[int(x) for x in t["ctl"]]))
    return dict(steps=out, n=n)


def test_the_utterance_cases_host_model_of_the_carry(capi):
    """every stream layout of tests/utterance_cases.py through K3: the carry words its host model hands K4 equal the kernel's after every step.
    Nothing is left out here: the rows are compared with the ring form, lost results' time columns included (only the layout `stream-lost` has any)"""
    ran = lost = 0
    for lay in uc.layouts():
        if lay["geometry"] != "stream":
            continue
        steps = uc.tables(lay)
        case = _uc_case(steps)
        out = _run_streams(capi, case, 10)
        ref = _check_streams(capi, lay["name"], out, case, 10, may_lose=lay["name"] == "stream-lost", ring=True)
        lost += sum(len(r["lost"]) for r in ref)
        for k, t in enumerate(steps):
            assert np.array_equal(out["carry"][k], t["carry"]), f"{lay['name']} step {k}: the host model's carry differs from the kernel's"
        ran += 1
    assert ran >= 6 and lost > 0


# ---------------------------------------------------------------------------------------------------------------------------------- span order
VARIANTS = {"integer-runs": 0, "integer-general": 1, "f64": 2}
_CLIPS = {}


def _span_clips(n):
    """the gate cases that share the common settings, densest-int first, cyclically; the long_voiced cuts at clips 0, 2, 5, 9 where the batch has them"""
    if n not in _CLIPS:
        sys.path.insert(0, os.path.join(GOLDEN, "gen"))
        from synth_spectra import designed_clip
        st = gc.by_name("densest-int")["settings"]
        group = [c for c in gc.CASES if c["settings"] == st and c["bands"] == 128]
        group.sort(key=lambda c: c["name"] != "densest-int")
        small = [gc.spectra(c) for c in group]
        longs = dict(zip((0, 2, 5, 9), [designed_clip("long_voiced", f) for f in dc.LONG_FRAMES.values()]))
        _CLIPS[n] = ([longs[i] if i in longs else small[i % len(small)] for i in range(n)], st)
    return _CLIPS[n]


def _check_span_order(capi, out, n, what):
    """the checks every span-order run must pass; returns {(clip, segment): span}"""
    cnt, cap, B = out["seg_count"].astype(np.int64), out["seg_cap"], capi.SPAN_BUCKETS
    total = int(cnt.sum())
    assert np.all(cnt <= cap), what
    assert int(out["counters"][1]) == int(out["hist"].sum()) == total, f"{what}: counters[1] {out['counters'][1]}, hist {out['hist'].sum()}, segments {total}"
    pairs = [(c, k) for c in range(n) for k in range(int(cnt[c]))]
    span = np.array([int(out["seg_i"][c, k, dc.SEG_FEND]) - int(out["seg_i"][c, k, dc.SEG_FBEGIN]) for c, k in pairs], np.int64)
    key = np.array([out["key"][c, k] for c, k in pairs], np.int64).reshape(-1, 2)
    assert np.array_equal(key[:, 0], B - 1 - np.minimum(span, B - 1)), f"{what}: a key's bucket is not that of its own segment record"
    assert np.array_equal(np.bincount(key[:, 0], minlength=B), out["hist"]), what
    for b in np.flatnonzero(out["hist"]):
        assert sorted(key[key[:, 0] == b, 1].tolist()) == list(range(int(out["hist"][b]))), f"{what}: the ranks of bucket {b} are no permutation"
    offs = np.concatenate([[0], np.cumsum(out["hist"].astype(np.int64))])[:-1]
    want = np.full_like(out["order"], 0xfffffff9)
    want[offs[key[:, 0]] + key[:, 1]] = np.array(pairs, np.uint32).reshape(-1, 2)
    assert np.array_equal(out["order"], want), f"{what}: order is not the counting sort of key"
    assert sorted(map(tuple, out["order"][:total].tolist())) == pairs, f"{what}: a (clip, segment) pair is missing or listed twice"
    by = {p: int(s) for p, s in zip(pairs, span)}
    along = np.array([min(by[tuple(p)], B - 1) for p in out["order"][:total].tolist()], np.int64)
    assert np.all(np.diff(along) <= 0), f"{what}: the clamped span lengths increase along the order"
    mask = np.ones(out["key"].shape[:2], bool)
    for c, k in pairs:
        mask[c, k] = False
    assert np.all(out["key"][mask] == 0xfffffff9), f"{what}: a key slot without a segment was written"
    return by


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513, 1025])
def test_span_order(capi, n, variant):
    clips, st = _span_clips(n)
    for blocks in ((0,) if n == 1 else (0, max(1, n // 3))):
        out = capi.debug_span_order(VARIANTS[variant], clips, st, blocks=blocks)
        what = f"{n} clips {variant} blocks={blocks}"
        by = _check_span_order(capi, out, n, what)
        assert len(by) > 0
        longs = [c for c in (0, 2, 5, 9) if c < n]                    # the long_voiced cuts: one segment each, 2046 | 2047, 2048, 2580 frames
        assert [by[(c, 0)] for c in longs] == [2046, 2047, 2048, 2580][:len(longs)], what
        assert [int(out["key"][c, 0, 0]) for c in longs] == [1, 0, 0, 0][:len(longs)], f"{what}: the clamp at SPAN_BUCKETS - 1 frames"
        assert int(out["hist"][0]) == max(len(longs) - 1, 0) and int(out["hist"][1]) == 1, what


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n", [1, 257])
def test_span_order_runs_the_gate_as_the_gate_entry_does(capi, n, variant):
    """the two entries share one gate set-up (csrc/debug_gate.hip): with the span counting on the gate kernels only add the span_key / span_hist writes, and
    span_order_kernel reads seg_count and writes only order and counters — so both leave the same segment tables, over the whole zero-filled tables"""
    clips, st = _span_clips(n)
    span = capi.debug_span_order(VARIANTS[variant], clips, st, blocks=0)
    gate = capi.debug_gate(VARIANTS[variant], clips, st, blocks=0)
    assert span["seg_cap"] == gate["seg_cap"], f"{n} clips {variant}"
    assert np.array_equal(span["seg_count"], gate["seg_count"]), f"{n} clips {variant}: seg_count"
    assert span["seg_i"].shape == gate["seg_i"].shape and np.array_equal(span["seg_i"], gate["seg_i"]), f"{n} clips {variant}: seg_i"


def _other_groups():
    """the gate cases under every OTHER settings vector or band count (the entry takes one per call): the three remaining densest-* cases among them"""
    st = gc.by_name("densest-int")["settings"]
    groups = {}
    for c in gc.CASES:
        if c["settings"] != st or c["bands"] != 128:
            groups.setdefault((tuple(sorted(c["settings"].items())), c["bands"]), []).append(c)
    return {g[0]["name"] if len(g) == 1 else "+".join(c["name"] for c in g): g for g in groups.values()}


OTHER = _other_groups()


def test_every_densest_case_reaches_the_span_order():
    there = {c["name"] for g in OTHER.values() for c in g} | {"densest-int"}
    assert {c["name"] for c in gc.CASES if c["name"].startswith("densest-")} <= there and len(there) == len(gc.CASES) - 34


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("group", list(OTHER))
def test_span_order_under_the_other_settings(capi, group, variant):
    """257 clips (two workgroups of the scatter, one of them one clip long) of each other settings group, its densest case first"""
    cases = sorted(OTHER[group], key=lambda c: not c["name"].startswith("densest-"))
    st = cases[0]["settings"]
    if not st["auto_noise_gate"] and variant != "f64":
        with pytest.raises(capi.WsaError):                              # the integer kernel is the auto gate's
            capi.debug_span_order(VARIANTS[variant], [gc.spectra(cases[0])], st)
        return
    small = [gc.spectra(c) for c in cases]
    n = 257
    clips = [small[i % len(small)] for i in range(n)]
    for blocks in (0, 85):
        out = capi.debug_span_order(VARIANTS[variant], clips, st, blocks=blocks)
        by = _check_span_order(capi, out, n, f"{group} {variant} blocks={blocks}")
        if any(c["name"].startswith("densest-") for c in cases):
            per_clip = sum(1 for p in by if p[0] == 0)
            assert per_clip >= 20 and len(by) >= per_clip * (n // len(small)), (group, per_clip)


# ---------------------------------------------------------------------------------------------------------------------------------- the whole path
def _batch_rows(wsa, spectra_list, level, env):
    old = {k: os.environ.get(k) for k in ("WSA_NO_FUSE", "WSA_DBG")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        an = wsa.Analyzer(wsa.Config(output_level=level))
        g = an.geometry(16000)
        b = an.batch([g["win"] + (len(s) - 1) * g["hop"] for s in spectra_list], 16000)
        d = torch.from_numpy(np.ascontiguousarray(np.concatenate(spectra_list, axis=0)).view(np.int32)).cuda()
        s = torch.cuda.current_stream().cuda_stream
        b.run_backend(d.data_ptr(), s)
        first = b.rows(s)
        b.run_backend(d.data_ptr(), s)                   # a second run finds what the first one's self-clear left
        second = b.rows(s)
        b.close(); an.close()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    for k in first:
        assert np.array_equal(first[k].view(np.uint8), second[k].view(np.uint8)), (env, k)
    return first


@pytest.mark.parametrize("level", [5, 13])
def test_the_whole_path_three_ways(wsa, level):
    """fixture clips with a dropped segment and a small synthetic batch through Batch by default, under WSA_NO_FUSE=1 (the scan kernels) and under
    WSA_DBG=8192 (spans in (clip, segment) order, no span order): meta, features, segments and offsets bit-identical"""
    sys.path.insert(0, os.path.join(GOLDEN, "gen"))
    from synth_spectra import synth_clip
    d = np.load(os.path.join(GOLDEN, "dispatch_spectra.npz"))
    clips = [d[k] for k in sorted(d.files)] + [synth_clip(9000 + i, 120 + 37 * i) for i in range(5)]
    want = _batch_rows(wsa, clips, level, {})
    assert len(want["meta"]) > 5 and int((want["segments"][:, 3] < 0).sum()) >= 3
    for env in ({"WSA_NO_FUSE": "1"}, {"WSA_DBG": "8192"}):
        got = _batch_rows(wsa, clips, level, env)
        for k in want:
            assert want[k].shape == got[k].shape and np.array_equal(want[k].view(np.uint8), got[k].view(np.uint8)), (env, k)


# ---------------------------------------------------------------------------------------------------------------------------------- refusals
def _untouched(out):
    ints = all(np.all(out[k] == SENT) for k in ("seg_out", "row_meta_out"))
    words = all(np.all(out[k] == SENT_U) for k in ("clip_row_off", "clip_seg_off", "host4", "counters", "hist"))
    return ints and words and np.all(out["row_feat_out"] == SENT_64) and np.all(out["path"] == -9)


def test_compact_refuses_what_would_index_outside_its_tables(capi):
    clips = BATCHES["drop-middle"]
    t = dc.tables([clips])
    run = lambda seg_i, cnt, **kw: capi.debug_compact(seg_i, cnt, t["meta_in"], t["feat_in"], 5, sentinel=SENT, **kw)
    good = run(t["seg_i"][0], t["seg_count"][0], clip_rows=t["clip_rows"][0])
    assert good["path"] == capi.COMPACT_FUSED
    pool = len(t["meta_in"])
    bad = []
    a = t["seg_count"][0].copy(); a[0] = t["seg_i"].shape[2] + 1
    bad.append(dict(seg_i=t["seg_i"][0], cnt=a))                                             # seg_count > seg_cap
    s = t["seg_i"][0].copy(); s[0, 0, dc.SEG_ROW0] = pool - 0; s[0, 0, dc.SEG_NROWS] = 1
    bad.append(dict(seg_i=s, cnt=t["seg_count"][0]))                                          # SEG_ROW0 + SEG_NROWS past the pool
    s = t["seg_i"][0].copy(); s[0, 1, dc.SEG_ROW0] = pool                                     # ... for a dropped segment too
    s[0, 1, dc.SEG_NROWS] = 2
    bad.append(dict(seg_i=s, cnt=t["seg_count"][0]))
    s = t["seg_i"][0].copy(); s[0, 2, dc.SEG_NROWS] = -1
    bad.append(dict(seg_i=s, cnt=t["seg_count"][0]))                                          # negative SEG_NROWS
    s = t["seg_i"][0].copy(); s[0, 0, dc.SEG_ROW0] = -1
    bad.append(dict(seg_i=s, cnt=t["seg_count"][0]))
    bad.append(dict(seg_i=t["seg_i"][0], cnt=t["seg_count"][0], clip_rows=t["clip_rows"][0] + 1))   # row counters that differ from the rows reported
    bad.append(dict(seg_i=t["seg_i"][0], cnt=t["seg_count"][0], rows_cap=2))                  # more rows than the output table holds
    for kw in bad:
        with pytest.raises(capi.WsaError) as e:
            run(kw.pop("seg_i"), kw.pop("cnt"), **kw)
        assert _untouched(e.value.out), kw
    # streams: a carry that has counted more results than segments (the result index would run ahead of the step's table), negative counts
    ctl = np.zeros((1, len(clips)), np.uint32)
    for c0, c1 in ((3, 4), (-1, 0), (2, -1)):
        cy = np.zeros((len(clips), capi.CARRY_WORDS), np.int32); cy[0, :2] = (c0, c1)
        with pytest.raises(capi.WsaError) as e:
            capi.debug_compact(t["seg_i"], t["seg_count"], t["meta_in"], t["feat_in"], 5, ctl=ctl, carry_in=cy, sentinel=SENT)
        assert _untouched(e.value.out) and np.all(e.value.out["carry"] == SENT)
    cy = np.zeros((len(clips), capi.CARRY_WORDS), np.int32); cy[0, :2] = (4, 4)             # as many results as segments: allowed
    ok = capi.debug_compact(t["seg_i"], t["seg_count"], t["meta_in"], t["feat_in"], 5, ctl=ctl, carry_in=cy, sentinel=SENT)
    assert ok["carry"][0, 0, :2].tolist() == [4 + len(clips[0]), 4 + sum(1 for sg in clips[0] if sg["flag"] >= 0)]
    with pytest.raises(capi.WsaError):
        run(t["seg_i"][0], t["seg_count"][0], clip_rows=t["clip_rows"][0], pool=pool - 1)       # the pool shorter than ROW0 + NROWS of its last segment


def test_span_order_refuses_as_the_gate_entry_does(capi):
    c = gc.by_name("fixed-start-edges")
    for v in (0, 1):
        with pytest.raises(capi.WsaError):                                                      # the integer kernel under a fixed gate
            capi.debug_span_order(v, [gc.spectra(c)], c["settings"])
    c = gc.by_name("densest-int")
    good = capi.debug_span_order(0, [gc.spectra(c)], c["settings"])
    with pytest.raises(capi.WsaError) as e:                                                     # a table size the entry did not hand out
        capi.debug_span_order(0, [gc.spectra(c)], c["settings"], seg_cap=good["seg_cap"] + 1)
    o = e.value.out
    assert np.all(o["key"] == 0xfffffff9) and np.all(o["order"] == 0xfffffff9) and np.all(o["hist"] == 0xfffffff9) and np.all(o["counters"] == 0xfffffff9)
    assert np.all(o["seg_count"] == 0xffffffff)

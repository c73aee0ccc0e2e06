"""Live streams collect into the device feature DB inside the step (specification FD-2; csrc/stream_featdb.hip,
wsa_stream_set_featdb / wsa_stream_db_rows).  Every comparison is bit for bit against tests/stream_featdb_ref.py: the hand-built steps
of tests/stream_featdb_cases.py through the debug entry, with the DB compared over its whole capacity, and synthetic speech fed step
by step at levels 5, 13, 12 and 11 with the graph on and off."""
import numpy as np
import pytest

from tests import featdb_cases as fc
from tests import stream_featdb_cases as sc
from tests import stream_featdb_ref as ref
from tests.test_gpu_featdb import _spec, _state
from webspeechanalyzer_amd import capi, featdb, train

pytestmark = pytest.mark.gpu
LEVELS = [5, 13, 12, 11]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def an():
    a = capi.Analyzer(capi.Config(output_level=13), device=0)
    yield a
    a.close()


def _s(torch):
    return torch.cuda.current_stream().cuda_stream


def _sizes():
    wave, wg, tile, grid = capi.Streams.featdb_tile_info()
    assert (wave, wg) == (64, 1024) and tile > 0 and grid > 0
    return wave, wg, tile, grid


def _fresh_db(an, case):
    """a DB whose whole table holds the case's pattern, with its `start` head rows counted"""
    pattern, head = sc.initial(case)
    db = an.device_db(ref.WIDTH[case["level"]], case["capacity"])
    db.append_host(pattern)
    db.clear()
    if len(head):
        db.append_host(head)
    st = ref.State(case["level"], case["capacity"], case["n_streams"], fill=pattern)
    st.db[:case["start"]] = head
    st.count = case["start"]
    return db, st


def _same_outcome(got, want, name):
    for k in ("first_row", "n_added", "n_replaced", "not_fitted"):
        assert got[k] == want[k], (name, k, got[k], want[k])
    assert np.array_equal(got["kept"], want["kept"]), name
    if want["replaced"] is not None:
        assert np.array_equal(got["replaced"], want["replaced"]), name


def _run_case(torch, an, case, name):
    db, st = _fresh_db(an, case)
    slot = st.slot.copy()
    for k, s in enumerate(case["steps"]):
        want = ref.step(st, **s)
        got = capi.debug_stream_featdb_step(db, case["level"], s["meta"], s["feat"], flags=s["flags"], utt_off=s["utt_off"], bits=s["bits"],
                                            slot=slot if case["level"] == 11 else None, stream=_s(torch))
        _same_outcome(got, want, (name, k))
        if case["level"] == 11:
            slot = got["slot"]
            assert np.array_equal(slot, st.slot), (name, k)
        assert db.count == st.count
        assert ref.same_bits(capi.debug_featdb_copy_capacity(db), st.db), (name, k)      # the whole table: a stray write shows
    db.close()


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_hand_built_steps(torch, an, name):
    _run_case(torch, an, sc.CASES[name](), name)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_row_counts_at_the_copy_grids_edge(torch, an, delta):
    _, _, tile, grid = _sizes()
    n = grid * tile + delta
    for level in (13, 12):
        _run_case(torch, an, sc.rows_case(level, n), (level, n))
    _run_case(torch, an, sc.all_kept_case(n), ("all kept", n))       # level 12 counts KEPT rows at the copy kernel's edge: exactly n of them


def test_a_row_count_word_beyond_the_table_is_clamped(torch, an):
    case = sc.rows_case(13, 5)
    db, st = _fresh_db(an, case)
    s = case["steps"][0]
    got = capi.debug_stream_featdb_step(db, 13, s["meta"], s["feat"], n_rows=4000, stream=_s(torch))
    _same_outcome(got, ref.step(st, **s), "clamped")
    assert ref.same_bits(capi.debug_featdb_copy_capacity(db), st.db)
    db.close()


# ---- end to end: synthetic speech with pauses, three streams, 8 frames per step
FS, F, SECONDS = 16000, 8, 4


def _ctl_plan(nsteps):
    """stream 0 has idle steps, stream 1 starts at step 5, stream 2 is stopped and started again in the middle; all stop at the end"""
    A, S, P = capi.ACTIVE, capi.START, capi.STOP
    plan = np.zeros((nsteps, 3), np.uint8)
    for k in range(nsteps):
        plan[k, 0] = 0 if k % 7 == 3 else A
        plan[k, 1] = A if k >= 5 else 0
        plan[k, 2] = A
    plan[0, 0] |= S; plan[5, 1] |= S; plan[0, 2] |= S
    plan[nsteps // 2, 2] |= P; plan[nsteps // 2 + 1, 2] |= S
    plan[nsteps - 1] |= P
    return plan


def _ref_step(st, level, r, ctl):
    if level == 11:
        counts = np.bincount(r["utt_meta"][:, 0], minlength=3) if len(r["utt_meta"]) else np.zeros(3, np.int64)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
        bits = np.array([1 if int(c) & capi.START else 0 for c in ctl], np.uint32)
        return ref.step(st, feat=r["utt_feat"], utt_off=off, bits=bits, flags=r["flags"] & 1)
    return ref.step(st, meta=r["meta"], feat=r["feat"], flags=r["flags"] & 1)


_PCM = {}


def _pcm(torch):
    if "x" not in _PCM:
        from webspeechanalyzer_amd.synth import synth_clips
        _PCM["x"] = synth_clips(3, SECONDS * FS, fs=FS, seed=23, device="cuda")
    return _PCM["x"]


def _e2e(torch, level, graph, capacity, collect_every=1):
    """Feeds the clips step by step with a DB attached; after every collected step the DB, over its whole capacity, and the step's
    outcome must equal the restatement applied to the collected host rows.  Returns (final whole table, count, per-step outcomes, names)."""
    pcm = _pcm(torch)
    a = capi.Analyzer(capi.Config(output_level=level), device=0)
    st = a.streams(3, FS, frames_per_step=F)
    st.enable_graph(graph)
    db = featdb.DeviceDB(a, level, capacity)
    pattern = fc.feature_table(capacity, db.width, 77)
    db.append_host(pattern)
    db.clear()
    db.attach(st, ["mic0", "mic1", "mic2"])
    state = ref.State(level, capacity, 3, fill=pattern)
    sps = st.samples_per_step
    nsteps = pcm.shape[1] // sps
    plan = _ctl_plan(nsteps)
    buf = torch.zeros((3, sps), device="cuda", dtype=torch.float32)
    outs, pending = [], []
    for k in range(nsteps):
        if k == nsteps // 2 + 1:
            db.rename(2, "mic2 again")                   # the name of the launch that stream 2's START begins in this step
        buf.copy_(pcm[:, k * sps:(k + 1) * sps])
        st.step(buf.data_ptr(), buf.stride(0), plan[k], _s(torch))
        if (k + 1) % collect_every and k + 1 < nsteps:
            continue                                     # no collect: the next step reads this one's outcome itself
        r = st.collect(_s(torch))
        if collect_every == 1:
            want = _ref_step(state, level, r, plan[k])
            got = st.db_rows()
            _same_outcome(got, want, (level, graph, k))
            assert (r["flags"] & ref.FLAG_DB_FULL) == (want["flags"] & ref.FLAG_DB_FULL), k
            assert db.count == state.count
            assert ref.same_bits(capi.debug_featdb_copy_capacity(db), state.db), (level, graph, k)
            new = db.append_step(r, plan[k])
            assert len(new) == got["n_added"] + got["n_replaced"]
            outs.append(want)
    table, count, records = capi.debug_featdb_copy_capacity(db), db.count, [dict(x) for x in db.records]
    db.detach()
    db.close(); st.close(); a.close()
    return table, count, outs, records


_RUNS = {}


def _full_run(torch, level, graph):
    if (level, graph) not in _RUNS:
        _RUNS[level, graph] = _e2e(torch, level, graph, 400)
    return _RUNS[level, graph]


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "no_graph"])
@pytest.mark.parametrize("level", LEVELS)
def test_streams_fill_the_db_step_by_step(torch, level, graph):
    table, count, outs, records = _full_run(torch, level, graph)
    adding = [k for k, o in enumerate(outs) if o["n_added"]]
    assert len(adding) >= 2 and count == sum(o["n_added"] for o in outs) > 0      # an empty run cannot pass
    assert all(o["not_fitted"] == 0 for o in outs)
    if level == 11:
        assert sum(o["n_replaced"] for o in outs) >= 1                            # a later result of a launch replaced an earlier one
        assert any(r["file"] == "mic2 again" for r in records)                    # ... and a second launch took a row of its own
    # the host records: one per DB row, in DB order, named after the stream's launch
    assert [r["row"] for r in records] == list(range(count))
    assert {r["file"] for r in records} <= {"mic0", "mic1", "mic2", "mic2 again"} and len({r["file"] for r in records}) >= 2


@pytest.mark.parametrize("level", LEVELS)
def test_graph_on_equals_graph_off(torch, level):
    a, b = _full_run(torch, level, True), _full_run(torch, level, False)
    assert a[1] == b[1] and ref.same_bits(a[0], b[0])
    assert [(o["first_row"], o["n_added"], o["n_replaced"]) for o in a[2]] == [(o["first_row"], o["n_added"], o["n_replaced"]) for o in b[2]]


@pytest.mark.parametrize("level", LEVELS)
def test_one_row_short_the_step_that_does_not_fit_stores_nothing(torch, level):
    _, need, full, _ = _full_run(torch, level, True)
    table, count, outs, _ = _e2e(torch, level, True, need - 1)       # (every step is checked against the restatement inside, whole table included)
    missed = [k for k, o in enumerate(outs) if o["not_fitted"]]
    last_adding = max(k for k, o in enumerate(full) if o["n_added"])
    # (level 11: the launch that found no room asks again with its every later result, and is turned away again)
    assert missed[0] == last_adding and (level == 11 or missed == [last_adding]) and outs[last_adding]["not_fitted"] == full[last_adding]["n_added"]
    assert outs[last_adding]["flags"] & ref.FLAG_DB_FULL and (outs[last_adding]["n_added"], outs[last_adding]["n_replaced"]) == (0, 0)
    assert count == need - full[last_adding]["n_added"]


def test_steps_without_a_collect_between_them(torch):
    want = _full_run(torch, 13, True)
    table, count, _, _ = _e2e(torch, 13, True, 400, collect_every=2)
    assert count == want[1] and ref.same_bits(table, want[0])


def test_refusals(torch, an):
    other = capi.Analyzer(capi.Config(output_level=13), device=0)
    st = an.streams(2, FS, frames_per_step=F)
    with pytest.raises(capi.WsaError, match="no feature DB attached to these streams"):
        st.db_rows()
    db_other = other.device_db(53, 8)
    with pytest.raises(capi.WsaError, match="created on another context"):
        st.set_featdb(db_other)
    db23 = an.device_db(23, 8)
    with pytest.raises(capi.WsaError, match="output_level 13 do not feed a feature DB of 23 features"):
        st.set_featdb(db23)
    a4 = capi.Analyzer(capi.Config(output_level=4), device=0)
    st4 = a4.streams(1, FS, frames_per_step=F)
    db4 = a4.device_db(53, 8)
    with pytest.raises(capi.WsaError, match="output_level 4 do not feed a feature DB of 53 features.*levels 3, 4 and 10 store nothing"):
        st4.set_featdb(db4)
    db = an.device_db(53, 64)
    st.set_featdb(db)
    st2 = an.streams(3, FS, frames_per_step=F)
    with pytest.raises(capi.WsaError, match=r"0 of 64 rows\) is already attached to another stream set of 2 streams"):
        st2.set_featdb(db)
    with pytest.raises(capi.WsaError, match="wsa_featdb_clear on a feature DB that is attached to a stream set .0 rows.: detach"):
        db.clear()
    # between a step and its collect the host's count is behind the device: whatever reads or moves it is refused
    buf = torch.zeros((2, st.samples_per_step), device="cuda", dtype=torch.float32)
    st.step(buf.data_ptr(), buf.stride(0), None, _s(torch))
    feat = np.nan_to_num(fc.feature_table(12, 53, 3), nan=0.5, posinf=7.0)
    spec = _spec([53, 4, 2], ["relu", "softmax"], feat.min(axis=0), feat.max(axis=0), ["a", "b"])
    for call in (lambda: db.copy_rows(), lambda: db.append_host(feat), lambda: db.ranges(), lambda: db.trainer(spec, [0] * 12, [0, 1] * 6, 2, 4, 0.1),
                 lambda: an.feature_db(db, np.ones(0), (), 0)):
        with pytest.raises(capi.WsaError, match=r"\(0 rows before it\) has not been collected yet: call wsa_stream_collect first"):
            call()
    st.collect(_s(torch))
    db.append_host(feat)                                 # ... and legal again between the collect and the next step
    assert db.count == 12 and st.db_rows()["first_row"] == 0
    st.step(buf.data_ptr(), buf.stride(0), None, _s(torch))
    st.collect(_s(torch))
    assert st.db_rows()["first_row"] == 12               # the step was handed the count the host append left
    st.set_featdb(None)
    db.clear()                                           # detached: legal
    st2.set_featdb(db)                                   # ... and free for another set
    with pytest.raises(capi.WsaError, match="no feature DB attached"):
        st.db_rows()
    for x in (st, st2, st4, db, db23, db4, db_other):
        x.close()
    other.close(); a4.close()


def test_the_db_stands_beside_a_knn_store(torch, an):
    """attaching a DB neither detaches a KNN store nor is detached by one"""
    rows = np.nan_to_num(fc.feature_table(70, 53, 5), nan=0.5, posinf=7.0)
    store = an.knn_store(53, 2, 70)
    f = torch.from_numpy(rows).cuda()
    c = torch.from_numpy((np.arange(70) % 2).astype(np.int32)).cuda()
    store.add(f.data_ptr(), c.data_ptr(), 70, _s(torch))
    torch.cuda.synchronize()
    st = an.streams(2, FS, frames_per_step=F)
    db = an.device_db(53, 16)
    st.set_knn(store, 3)
    st.set_featdb(db)
    st.set_knn(store, 3)
    buf = torch.zeros((2, st.samples_per_step), device="cuda", dtype=torch.float32)
    st.step(buf.data_ptr(), buf.stride(0), None, _s(torch))
    st.collect(_s(torch))
    assert st.db_rows()["n_added"] == 0 and st.knn_classes()["label"].shape == (0,)
    st.close(); db.close(); store.close()


def test_a_trainer_from_the_streamed_db_equals_the_host_trainer(torch):
    """the rows the streams left in the DB, read in place by wsa_trainer_create_db, against the host trainer on the host copy of the same rows"""
    a = capi.Analyzer(capi.Config(output_level=13), device=0)
    st = a.streams(3, FS, frames_per_step=F)
    db = featdb.DeviceDB(a, 13, 400)
    db.attach(st, ["a", "b", "c"])
    pcm = _pcm(torch)
    sps = st.samples_per_step
    buf = torch.zeros((3, sps), device="cuda", dtype=torch.float32)
    host = []
    for k in range(pcm.shape[1] // sps):
        buf.copy_(pcm[:, k * sps:(k + 1) * sps])
        st.step(buf.data_ptr(), buf.stride(0), None, _s(torch))
        host.append(st.collect(_s(torch))["feat"])
    host = np.concatenate(host)
    n = db.count
    assert n == len(host) >= 12 and ref.same_bits(db.copy_rows(), host)
    rows = [(i * 7) % n for i in range(37)]
    y = np.array([i % 3 for i in range(37)], np.int32)
    in_min, in_max = db.ranges(rows)
    spec = _spec([53, 8, 3], ["relu", "softmax"], in_min, in_max, ["x", "y", "z"])
    ta, tb = db.trainer(spec, rows, y, 4, 32, 0.2), a.trainer(spec, host[rows], y, 4, 32, 0.2)
    assert _state(ta) == _state(tb)
    order = train.epoch_orders(33, 1, 3)[0]
    ta.epoch(order); tb.epoch(order)
    assert _state(ta) == _state(tb) and np.isfinite(ta.stats()["loss"])
    ta.close(); tb.close(); db.detach(); db.close(); st.close(); a.close()

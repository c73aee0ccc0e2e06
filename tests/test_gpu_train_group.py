"""Training groups (K7g, specification TG-1) on the GPU: a group epoch is wsa_trainer_epoch on every member, bit for bit.  The reference
is the solo trainer (device_run of tests/test_gpu_train_shapes.py and, for the 264- and 23-wide members, of tests/test_gpu_wide.py); the
comparison is same_bits: byte equality of every layer's kernel and bias after every epoch and equality of loss, acc, val_loss, val_acc
and epochs_done.  No tolerance anywhere: members share no buffer and every sum keeps its one owner and order."""
import numpy as np
import pytest

from tests import train_cases as tc
from tests import wide_cases as wc
from tests.test_gpu_train_shapes import device_run, same_bits, spec_of
from tests.test_gpu_wide import device_run as wide_device_run
from tests.test_gpu_wide import spec_of as wide_spec_of
from tests.test_train_group_host import formula
from webspeechanalyzer_amd import capi, train

pytestmark = pytest.mark.gpu

ALL = list(tc.CASES)
LRS_32 = [0.01 * (k + 1) for k in range(16)]                       # n = 32: last_of_1 and r_one_layer alternating, 16 learning rates


@pytest.fixture(scope="module")
def an():
    a = capi.Analyzer(capi.Config(output_level=13), device=0)
    yield a
    a.close()


@pytest.fixture(scope="module")
def solo(an):
    """the solo run of (key, lr), made when first asked for and shared: read-only"""
    done = {}

    def get(key, lr=None):
        if (key, lr) not in done:
            if key in wc.CASES:
                import torch
                done[key, lr] = wide_device_run(torch, an, key)[0]
            else:
                done[key, lr] = device_run(an, key, lr)[0]
        return done[key, lr]
    return get


def table(key):
    return (wc if key in wc.CASES else tc)


def make(an, key, lr=None):
    """the trainer device_run makes for the case"""
    c, i = table(key).CASES[key], table(key).inputs(key)
    spec = (wide_spec_of if key in wc.CASES else spec_of)(key)
    lr = c["lr"] if lr is None else lr
    if c["regression"]:
        return an.regress_trainer(spec, i["feat"], i["values"], c["n_val"], c["batch"], lr)
    return an.trainer(spec, i["feat"], i["labels"], c["n_val"], c["batch"], lr)


def snapshot(tr, st):
    k, b = tr.weights()
    return dict(st, kernels=k, biases=b)


def group_run(an, members, check_launches=True):
    """members: [(key, lr or None)] stepped as one group over their cases' epochs (a member whose case has fewer epochs leaves: the
    group is re-formed from the rest, as train.train_many does); per member what device_run returns"""
    trs = [make(an, k, lr) for k, lr in members]
    epochs = [table(k).CASES[k]["epochs"] for k, _ in members]
    orders = [table(k).inputs(k)["orders"] for k, _ in members]
    out = [[] for _ in members]
    try:
        for e in range(max(epochs)):
            live = [m for m in range(len(members)) if epochs[m] > e]
            g = an.train_group([trs[m] for m in live])
            try:
                if check_launches:
                    shapes = [(len(trs[m].spec.units) - 1, trs[m].n_train, table(members[m][0]).CASES[members[m][0]]["batch"], trs[m].n_val) for m in live]
                    assert g.launches() == formula(shapes)
                g.epoch([orders[m][e] for m in live])
                for m, st in zip(live, g.stats()):
                    out[m].append(snapshot(trs[m], st))
            finally:
                g.close()
    finally:
        for t in trs:
            t.close()
    return out


def assert_members_equal_solo(got, members, solo):
    for (key, lr), run in zip(members, got):
        want = solo(key, lr)
        assert len(run) == len(want), key
        assert same_bits(run, want), f"member {key} (lr {lr}) differs from its solo run"


@pytest.fixture(scope="module")
def all_cases_run(an):
    return group_run(an, [(k, None) for k in ALL])


def test_all_cases_as_one_group(all_cases_run, solo):
    """1-layer and 8-layer members, 53-1024-64, SGD and Adam, n_val of 0 and n_val > batch, 3-step members beside the 300-step one, steps of
    1 100 rows beside steps of 1 row, widths of exactly 16, 17, 15 and 1"""
    assert_members_equal_solo(all_cases_run, [(k, None) for k in ALL], solo)


def test_all_cases_in_reverse_order(an, solo):
    """the prefix and the owner of every workgroup change, the bits do not"""
    members = [(k, None) for k in ALL[::-1]]
    assert_members_equal_solo(group_run(an, members), members, solo)


def test_two_runs_of_the_same_group_are_bit_identical(an, all_cases_run):
    again = group_run(an, [(k, None) for k in ALL])
    assert all(same_bits(a, b) for a, b in zip(again, all_cases_run))


def test_group_of_one_equals_solo(an, solo):
    for key in ("width_edges", "r_width_edges"):
        assert_members_equal_solo(group_run(an, [(key, None)]), [(key, None)], solo)


def test_group_of_32_with_16_learning_rates(an, solo):
    members = [(("last_of_1", "r_one_layer")[m % 2], LRS_32[m // 2]) for m in range(32)]
    assert len(set(members)) == 32
    got = group_run(an, members)
    assert_members_equal_solo(got, members, solo)
    assert not same_bits(got[0], got[2])                           # the learning rates do reach the members


@pytest.mark.parametrize("keys", [("one_layer", "width_edges", "last_of_1"), ("r_one_layer", "r_width_edges", "classes_33")])
def test_partial_workgroup_in_the_middle_of_the_group(an, solo, keys):
    """the middle member (widths 16, 17, 15, 1 behind steps of 17 rows) has launches whose tile count is no multiple of TR_WAVES: its last
    workgroup has idle waves, and the member behind it starts at the next workgroup, not at the next wave"""
    c = tc.CASES[keys[1]]
    tiles = [(-(-c["batch"] // 16)) * (-(-u // 16)) for u in c["units"][1:]]
    assert any(t % 4 for t in tiles)
    members = [(k, None) for k in keys]
    assert_members_equal_solo(group_run(an, members), members, solo)


def test_one_member_of_each_width(an, solo):
    members = [("w264_stack", None), ("last_of_1", None), ("r_w23", None), ("r_w264", None), ("w23_stack", None)]
    assert sorted({table(k).CASES[k]["units"][0] for k, _ in members}) == [23, 53, 264]
    assert_members_equal_solo(group_run(an, members), members, solo)


def test_solo_epochs_between_group_epochs(an):
    """two group epochs, a solo epoch of ONE member, a group epoch: that member equals its four solo epochs, the others their three"""
    keys = ["r_relu_out", "classes_33", "one_layer"]
    mixed = 1

    def order(key, e):
        n_train = tc.CASES[key]["n"] - tc.CASES[key]["n_val"]
        return None if e % 2 else tc.permutation(n_train, 40 + e)

    def run(grouped):
        trs = [make(an, k) for k in keys]
        g = an.train_group(trs) if grouped else None
        count = [0] * len(keys)
        out = [[] for _ in keys]

        def all_of_them():
            if grouped:
                g.epoch([order(k, count[m]) for m, k in enumerate(keys)])
                sts = g.stats()
            else:
                for m, k in enumerate(keys):
                    trs[m].epoch(order(k, count[m]))
                sts = [t.stats() for t in trs]
            for m in range(len(keys)):
                count[m] += 1
                out[m].append(snapshot(trs[m], sts[m]))
        try:
            all_of_them(); all_of_them()
            trs[mixed].epoch(order(keys[mixed], count[mixed]))                 # wsa_trainer_epoch on a member of a living group
            count[mixed] += 1
            out[mixed].append(snapshot(trs[mixed], trs[mixed].stats()))
            all_of_them()
        finally:
            if g is not None:
                g.close()
            for t in trs:
                t.close()
        return out

    got, want = run(True), run(False)
    assert [len(r) for r in got] == [3, 4, 3] and got[mixed][-1]["epochs_done"] == 4
    for a, b in zip(got, want):
        assert same_bits(a, b)


def _prepared():
    feat, lab = tc.cluster_rows(120, 3, 21)
    data = train.prepare(feat, [str(v) for v in lab], ["0", "1", "2"])
    rfeat, values = tc.smooth_rows(90, 22)
    rdata = train.prepare_ordinal(rfeat, [float(v) for v in np.clip(values, 0.0, 1.0)])
    return data, rdata


def test_train_many_against_the_one_by_one_functions(an):
    data, rdata = _prepared()
    seen = {0: [], 1: []}
    jobs = [dict(data=data, epochs=3, seed=5, batch_size=16, learning_rate=0.1, on_epoch=lambda e, st: seen[0].append((e, st))),
            dict(data=rdata, epochs=2, seed=6, layers=[{"type": "dense", "units": 12, "activation": "tanh"}, {"type": "dense", "activation": "sigmoid"}],
                 learning_rate=0.01, validation_split=0.2)]
    got = train.train_many(an, jobs)
    want_seen = []
    want = [train.train(an, data, epochs=3, seed=5, batch_size=16, learning_rate=0.1, on_epoch=lambda e, st: want_seen.append((e, st))),
            train.train_regression(an, rdata, epochs=2, seed=6, layers=jobs[1]["layers"], learning_rate=0.01, validation_split=0.2)]
    assert len(got) == 2 and seen[0] == want_seen and len(want_seen) == 3
    for (gs, gh), (ws, wh) in zip(got, want):
        assert gh == wh
        assert gs.units == ws.units and gs.activations == ws.activations and gs.labels == ws.labels
        assert np.array_equal(gs.in_min, ws.in_min) and np.array_equal(gs.in_max, ws.in_max)
        assert (gs.out_min, gs.out_max) == (ws.out_min, ws.out_max)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(gs.kernels + gs.biases, ws.kernels + ws.biases))
    assert len(got[0][1]) == 3 and len(got[1][1]) == 1 and got[1][1][0]["epochs_done"] == 2


def test_refusals(an):
    trs = [make(an, "last_of_1"), make(an, "r_one_layer")]
    other = capi.Analyzer(capi.Config(output_level=13), device=0)
    foreign = make(other, "one_layer")
    try:
        with pytest.raises(capi.WsaError, match=r"1 \.\. 32 members, got 0"):
            an.train_group([])
        many = [make(an, "r_one_layer") for _ in range(33)]
        try:
            with pytest.raises(capi.WsaError, match=r"1 \.\. 32 members, got 33"):
                an.train_group(many)
        finally:
            for t in many:
                t.close()
        with pytest.raises(capi.WsaError, match="member 1 belongs to another context"):
            an.train_group([trs[0], foreign])
        with pytest.raises(capi.WsaError, match="member 2 is the same trainer as member 0"):
            an.train_group([trs[0], trs[1], trs[0]])
        import ctypes
        hs, h = (ctypes.c_void_p * 2)(trs[0].h, None), ctypes.c_void_p()
        assert an.L.wsa_train_group_create(an.h, ctypes.cast(hs, ctypes.c_void_p), 2, ctypes.byref(h)) != 0 and not h
        assert "member 1 is NULL" in an.L.wsa_last_error(an.h).decode()
        g = an.train_group(trs)
        try:
            free = make(an, "one_layer")
            try:
                with pytest.raises(capi.WsaError, match="member 1 is already in a living group"):
                    an.train_group([free, trs[1]])
            finally:
                free.close()
            before = [t.weights() for t in trs]
            n1 = trs[1].n_train
            bad = np.arange(n1, dtype=np.uint32)
            bad[7] = n1
            with pytest.raises(capi.WsaError, match=rf"member 1: order\[7\] = {n1} is outside 0 \.\. {n1 - 1}"):
                g.epoch([tc.permutation(trs[0].n_train, 3), bad])
            after = [t.weights() for t in trs]
            for (k0, b0), (k1, b1) in zip(before, after):
                assert all(x.tobytes() == y.tobytes() for x, y in zip(k0 + b0, k1 + b1))
            assert [t.stats()["epochs_done"] for t in trs] == [0, 0]
        finally:
            g.close()
        g = an.train_group(trs[::-1])                                  # a destroyed group has released its members
        g.close()
    finally:
        foreign.close()
        other.close()
        for t in trs:
            t.close()

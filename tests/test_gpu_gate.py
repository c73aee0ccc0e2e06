"""K2a (csrc/gate.hip) on its own (-m gpu): the hand-built frames of tests/gate_cases.py through the test entry wsa_debug_gate (csrc/debug_gate.hip) — the
peak scan, then ONE of the gate's four forms — against the oracle's record of what the gate decided (pyoracle.run_backend(gate=True), pinned to the
reference by tests/test_gate_reference.py): per frame whether accumulate_fm is called, its filing index, the stale bit and both floors; per segment
start, length, the span that owns its tracks, c_ci, ctx_max and the floor; the counts and the overflow flag.  Integers and doubles, compared bit
for bit: nothing here has a tolerance but the end-to-end test, which keeps the project's 1e-4 contract and its 1e-12 canary."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

from oracle import pyoracle
from tests import gate_cases as gc
from tests.util import GOLDEN, callbacks_equal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VARIANTS = {"integer-runs": 0, "integer-general": 1, "f64": 2}


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


def _cfg(c, level=5):
    return pyoracle.default_cfg(level=level, bands=c["bands"], **c["settings"])


@pytest.fixture(scope="module")
def oracle():
    """the oracle's run of every case, computed once and left alone"""
    return {c["name"]: pyoracle.run_backend(gc.spectra(c), _cfg(c), trace=True, gate=True) for c in gc.CASES}


def _groups():
    """cases that can share a launch: same settings, same band count"""
    g = {}
    for c in gc.CASES:
        g.setdefault((json.dumps(c["settings"], sort_keys=True), c["bands"]), []).append(c)
    return list(g.values())


def _check_frames(name, got_info, got_v, got_fl, ref, what):
    n = len(ref["called"])
    assert len(got_info) == n, (what, name)
    info = np.asarray(got_info)
    called = info != -1
    bad = np.flatnonzero(called != (ref["called"] != 0))
    assert len(bad) == 0, f"{what} {name}: accumulate_fm called / not called differs first at frame {bad[:3].tolist()}"
    idx = np.flatnonzero(called)
    assert np.all(info[idx] >= 0), (what, name)
    bad = idx[(info[idx] & 0x3fffffff) != ref["t"][idx]]
    assert len(bad) == 0, f"{what} {name}: filing index differs first at frame {bad[:3].tolist()}: {(info[bad[:3]] & 0x3fffffff).tolist()} oracle {ref['t'][bad[:3]].tolist()}"
    bad = idx[((info[idx] >> 30) & 1) != ref["stale"][idx]]
    assert len(bad) == 0, f"{what} {name}: stale bit differs first at frame {bad[:3].tolist()}"
    for k, got in (("v", got_v), ("fl", got_fl)):
        bad = np.flatnonzero(np.asarray(got) != ref[k])
        assert len(bad) == 0, f"{what} {name}: {k} differs first at frame {bad[:3].tolist()}: {np.asarray(got)[bad[:3]].tolist()} oracle {ref[k][bad[:3]].tolist()}"


def _segment_rows(seg_i, seg_d, count):
    return [[int(x) for x in seg_i[s, :5]] + [float(seg_d[s, 0]), float(seg_d[s, 1])] for s in range(count)]


def _check_batch(out, cases, oracle, what):
    assert out["flags"] == 0, what
    for i, c in enumerate(cases):
        ref = oracle[c["name"]]["gate"]
        _check_frames(c["name"], out["fr_info"][i], out["fr_v"][i], out["fr_fl"][i], ref, what)
        cnt = int(out["seg_count"][i])
        assert cnt == len(ref["segments"]) and cnt <= out["seg_cap"], f"{what} {c['name']}: {cnt} segments, oracle {len(ref['segments'])}, table {out['seg_cap']}"
        assert _segment_rows(out["seg_i"][i], out["seg_d"][i], cnt) == ref["segments"], f"{what} {c['name']}"
    assert out["counter0"] == max(len(oracle[c["name"]]["gate"]["segments"]) for c in cases), what


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_batch_variants_equal_the_oracles_record(capi, oracle, variant):
    ran = 0
    for cases in _groups():
        auto = bool(cases[0]["settings"]["auto_noise_gate"])
        if not auto and variant != "f64":
            continue                                                     # the integer kernel is the auto gate's; a fixed gate runs the f64 kernel
        for c in cases:                                                  # every case alone: its segment table is sized from its own length
            out = capi.debug_gate(VARIANTS[variant], [gc.spectra(c)], c["settings"])
            _check_batch(out, [c], oracle, variant)
            ran += 1
    assert ran == (len(gc.CASES) if variant == "f64" else sum(1 for c in gc.CASES if c["settings"]["auto_noise_gate"]))


def test_the_integer_kernel_refuses_a_fixed_gate(capi):
    c = gc.by_name("fixed-start-edges")
    for v in (0, 1):
        with pytest.raises(capi.WsaError):
            capi.debug_gate(v, [gc.spectra(c)], c["settings"])


def _run_backend_on(wsa, spectra_list, settings, level, bands, trace=False):
    cfg = wsa.Config(output_level=level, N_mel_bins=bands, window_step=settings["window_step"], window_width=settings["window_step"],
                     pause_length=settings["pause_length"], min_seg_length=settings["min_seg_length"], auto_noise_gate=int(settings["auto_noise_gate"]),
                     voiced_max_dB=settings["voiced_max_dB"], voiced_min_dB=settings["voiced_min_dB"])
    an = wsa.Analyzer(cfg)
    g = an.geometry(16000)
    ns = [g["win"] + (len(s) - 1) * g["hop"] if len(s) else 0 for s in spectra_list]
    b = an.batch(ns, 16000)
    flat = np.concatenate([s for s in spectra_list if len(s)], axis=0)
    d = torch.from_numpy(np.ascontiguousarray(flat).view(np.int32)).cuda()
    if trace:
        b.enable_trace(True)
    s = torch.cuda.current_stream().cuda_stream
    b.run_backend(d.data_ptr(), s)
    out = b.callbacks(s)
    if trace:
        tr = b.trace(s)
        off = np.concatenate([[0], np.cumsum([len(x) for x in spectra_list])])
        for i, o in enumerate(out):
            o["trace"] = tr[off[i]:off[i + 1]]
    b.close(); an.close()
    return out


def test_general_path_trace_equals_the_reference(wsa):
    """the trace of the batch API (enable_trace: every frame through the general path; the f64 kernel under a fixed gate) equals the golden the reference wrote"""
    g = json.load(open(os.path.join(GOLDEN, "gate_expected.json")))
    table = np.array([struct.unpack(">d", bytes.fromhex(h))[0] for h in g["values"]], np.float64)
    gold = {c["name"]: c for c in g["cases"]}
    frames = 0
    for cases in _groups():
        got = _run_backend_on(wsa, [gc.spectra(c) for c in cases], cases[0]["settings"], 5, cases[0]["bands"], trace=True)
        for c, o in zip(cases, got):
            ref = table[np.array(gold[c["name"]]["trace"], np.int64)].reshape(-1, 10)
            tr = np.ascontiguousarray(o["trace"][:, :10])
            assert ref.shape == tr.shape, c["name"]
            bad = np.argwhere(ref.view(np.uint64) != tr.view(np.uint64))
            assert len(bad) == 0, f"{c['name']}: first differing (frame, column) {bad[:3].tolist()}: reference {ref[bad[0][0]]} device {tr[bad[0][0]]}"
            assert o["segments_ci"] == gold[c["name"]]["segments_ci"], c["name"]
            frames += len(ref)
    assert frames > 3000


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_many_clips_per_launch_in_two_orders(capi, oracle, variant):
    """all cases of a group as one batch, three workgroups walking them (the kernels loop over clips per workgroup), forwards and shuffled: a clip's result
    depends neither on its neighbours nor on what the clip before it left in LDS or registers"""
    big = max(_groups(), key=len)
    assert len(big) > 30 and big[0]["settings"]["auto_noise_gate"]
    rng = np.random.default_rng(5)
    for order in (list(range(len(big))), list(rng.permutation(len(big)))):
        cases = [big[i] for i in order]
        out = capi.debug_gate(VARIANTS[variant], [gc.spectra(c) for c in cases], cases[0]["settings"], blocks=3)
        _check_batch(out, cases, oracle, f"{variant} blocks=3")


# ---------------------------------------------------------------------------------------------------------------------------------- streams
def _schedule(lengths, F, idle_tail=0):
    """every clip in steps of F frames from step 0: START with its first step, STOP with its last; afterwards idle"""
    steps = max(1, max((n + F - 1) // F for n in lengths)) + idle_tail
    nfr = np.zeros((steps, len(lengths)), np.uint32)
    ctl = np.zeros((steps, len(lengths)), np.uint32)
    for i, n in enumerate(lengths):
        k_last = max((n + F - 1) // F - 1, 0)
        for k in range(k_last + 1):
            nfr[k, i] = min(F, n - k * F)
        ctl[0, i] |= 1
        ctl[k_last, i] |= 2
    return nfr, ctl


def _stream_segments(out, i):
    rows = []
    for k in range(out["seg_count"].shape[0]):
        rows += _segment_rows(out["seg_i"][k, i], out["seg_d"][k, i], int(out["seg_count"][k, i]))
    return rows


def _check_spans(name, fr_info, fr_span, segments):
    for seg in segments:
        fb, fe = seg[2], seg[3]
        called = np.asarray(fr_info[fb:fe]) != -1
        assert np.all(np.asarray(fr_span[fb:fe])[called] == fb), f"{name}: a frame of span [{fb}, {fe}) names another span"


@pytest.mark.parametrize("F", [1, 3, 64, 65])
def test_streams_equal_the_batch_oracle(capi, oracle, F):
    for cases in _groups():
        lengths = [len(gc.spectra(c)) for c in cases]
        nfr, ctl = _schedule(lengths, F)
        out = capi.debug_gate(capi.GATE_STREAM, [gc.spectra(c) for c in cases], cases[0]["settings"], F=F, max_span=1024, step_nfr=nfr, step_ctl=ctl,
                              blocks=0 if F != 3 else 2)
        assert out["flags"] == 0 and out["ring"] >= 1024 + F
        for i, c in enumerate(cases):
            ref = oracle[c["name"]]["gate"]
            _check_frames(c["name"], out["fr_info"][i], out["fr_v"][i], out["fr_fl"][i], ref, f"stream F={F}")
            assert _stream_segments(out, i) == ref["segments"], f"stream F={F} {c['name']}"
            _check_spans(c["name"], out["fr_info"][i], out["fr_span"][i], ref["segments"])
            st = out["state"][-1, i]
            assert list(st[:12]) == ref["state"] and st[12] == 0, f"stream F={F} {c['name']}: state {list(st[:13])} oracle {ref['state']}"


def _oracle_with_ring_cuts(spec, cfg, F, ring):
    """drive the oracle frame by frame and cut where gate.hip's stream kernel does: behind frame f when c_started >= 0 and f + 1 - span_begin + F > ring"""
    L = pyoracle.lib()
    h = L.wsa_or_seg_new(ctypes.byref(cfg))
    st = (ctypes.c_double * 12)()
    cuts = []
    try:
        for f in range(len(spec)):
            L.wsa_or_seg_push(h, np.ascontiguousarray(spec[f]).ctypes.data)
            L.wsa_or_gate_state(h, st)
            if st[3] >= 0 and f + 1 - st[11] + F > ring:
                L.wsa_or_seg_cut(h)
                cuts.append(f)
    finally:
        L.wsa_or_seg_free(h)
    return cuts, pyoracle.run_backend(spec, cfg, gate=True, cuts=cuts)


@pytest.mark.parametrize("name", ["slow-decay-zero-step", "slow-decay"])
def test_a_small_ring_cuts_a_long_span_where_the_rule_says(capi, name):
    c = gc.by_name(name)
    F, spec = 16, gc.spectra(c)
    nfr, ctl = _schedule([len(spec)], F)
    out = capi.debug_gate(capi.GATE_STREAM, [spec], c["settings"], F=F, max_span=64, step_nfr=nfr, step_ctl=ctl)
    ring = out["ring"]
    assert ring == 128
    cuts, ref = _oracle_with_ring_cuts(spec, _cfg(c), F, ring)
    assert len(cuts) >= 1 and ref["gate"]["arms"]["ring_cut"] == len(cuts)
    g = ref["gate"]
    _check_frames(name, out["fr_info"][0], out["fr_v"][0], out["fr_fl"][0], g, "small ring")
    assert _stream_segments(out, 0) == g["segments"], (cuts, _stream_segments(out, 0), g["segments"])
    assert out["state"][-1, 0, 12] == len(cuts) and list(out["state"][-1, 0, :12]) == g["state"]
    assert out["flags"] == 0


def test_a_start_after_idle_steps_gives_the_launch_state_again(capi, oracle):
    c = gc.by_name("gate-w-and-decay")
    spec = gc.spectra(c)
    n, F = len(spec), 16
    one_n, one_c = _schedule([n], F)
    idle = np.zeros((3, 1), np.uint32)
    nfr = np.concatenate([one_n, idle, one_n])
    ctl = np.concatenate([one_c, idle, one_c])
    out = capi.debug_gate(capi.GATE_STREAM, [np.concatenate([spec, spec])], c["settings"], F=F, max_span=1024, step_nfr=nfr, step_ctl=ctl)
    ref = oracle[c["name"]]["gate"]
    k1 = len(one_n)
    for half, k0 in ((0, 0), (1, k1 + 3)):
        sl = slice(half * n, (half + 1) * n)
        _check_frames(c["name"], out["fr_info"][0][sl], out["fr_v"][0][sl], out["fr_fl"][0][sl], ref, f"pass {half}")
        rows = []
        for k in range(k0, k0 + k1):
            rows += _segment_rows(out["seg_i"][k, 0], out["seg_d"][k, 0], int(out["seg_count"][k, 0]))
        assert rows == ref["segments"], f"pass {half}"
    assert np.array_equal(out["state"][:k1, 0], out["state"][k1 + 3:, 0])            # step for step the same state
    for k in range(k1, k1 + 3):                                                       # idle steps: no segments, the state stands
        assert out["seg_count"][k, 0] == 0 and np.array_equal(out["state"][k, 0], out["state"][k1 - 1, 0])


# ---------------------------------------------------------------------------------------------------------------------------------- end to end
def test_the_cases_survive_the_tracker(wsa, oracle):
    """the same frames through wsa_batch_run_backend at level 5: segments and callbacks equal the oracle's (1e-4 is the contract, 1e-12 the project's canary
    for a change of arithmetic).  A segment whose straighten step throws in the reference is reported as the oracle reports it (pyoracle.callbacks)."""
    rows = 0
    for cases in _groups():
        got = _run_backend_on(wsa, [gc.spectra(c) for c in cases], cases[0]["settings"], 5, cases[0]["bands"])
        for c, o in zip(cases, got):
            r = oracle[c["name"]]
            assert o["segments_ci"] == r["segments_ci"], c["name"]
            for tol in (1e-4, 1e-12):
                ok, why = callbacks_equal(5, r["callbacks"], o["callbacks"], exact=False, tol=tol)
                assert ok, f"{c['name']} (tol {tol}): {why}"
            rows += len(r["callbacks"])
    assert rows > 100

"""Streams of different rates converted inside the step (wsa_stream_create_mixed): K0s gives bit for bit the samples oracle/resample.c
gives for the whole signal however the signal is cut into steps; the rows collected over the steps are the rows of a mixed-rate batch on
the whole signals and of the oracle chain resample -> front end -> back end; rows arrive in the step whose frames close their segment; a
set whose streams all sit at the analysis rate is a plain set; restart, idle and STOP behave per stream; the classifier inside the step
sees the features of the converted signal."""
import json
import os

import numpy as np
import pytest

from tests import stream_resample_model as M
from tests.test_gpu_stream import _per_stream_callbacks
from tests.util import callbacks_equal

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def wsa():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import webspeechanalyzer_amd as w
    return w


def _signals(fs_out, seconds=6.0):
    """One signal of `seconds` per rate of the list, each at its own rate, plus one at fs_out (the copied stream)."""
    from webspeechanalyzer_amd.synth import synth_clips
    rates = [float(r) for r in M.RATES if r != fs_out] + [float(fs_out)]
    return rates, [synth_clips(1, int(seconds * r), fs=int(r), seed=300 + k, device="cpu")[0].numpy().copy() for k, r in enumerate(rates)]


def _drive(wsa, an, sigs, rates, fs_out, F, feed, graph, host_in, seed=5, model=None, plan=None):
    """Feeds every signal to its stream of a mixed set in the steps `feed` gives ('paced' / 'capacity' / 'random'; plan: explicit per-stream
    lists of (step, count, control) instead).  Every step's counts are checked against the Python restatement of the host bookkeeping.
    -> dict(rows per step, conv per stream, frames [step][stream], outs [step][stream], books, none_steps, classes per step)"""
    n = len(sigs)
    st = an.streams(n, rates, frames_per_step=F, resample_to=fs_out)
    st.enable_graph(graph)
    if model is not None:
        st.set_model(model)
    g = an.geometry(fs_out)
    books = [M.Book(r, fs_out, F, g["win"], g["hop"]) for r in rates]
    assert [int(c) for c in st.input_capacity] == [b.cap for b in books]
    assert st.samples_per_step == F * g["hop"] and st.input_stride >= max(b.cap for b in books)
    min_ratio = min([b.ratio for b in books if b.fs_in != b.fs_out] or [0.0])
    assert st.frame_capacity == int(an.L.wsa_stream_frames_bound(F, g["hop"], min_ratio))
    rng = np.random.default_rng(seed)
    if plan is None:
        plan = []
        for b, x in zip(books, sigs):
            cnt = M.feed_counts(feed, b, len(x), rng)
            plan.append([(k, c, wsa.ACTIVE | (wsa.START if k == 0 else 0) | (wsa.STOP if k == len(cnt) - 1 else 0)) for k, c in enumerate(cnt)])
    sched = [{k: (c, ctl) for k, c, ctl in p} for p in plan]
    nsteps = max(max(s) for s in sched) + 1
    pos = [0] * n
    dev = torch.zeros((n, st.input_stride), device="cuda", dtype=torch.float32)
    stage = np.zeros((n, st.input_stride), np.float32)
    out = dict(rows=[], conv=[[] for _ in range(n)], frames=[], outs=[], ctl=[], books=books, none_steps=0, classes=[])
    for k in range(nsteps):
        ctl, n_in, paced_ok = np.zeros(n, np.uint8), np.zeros(n, np.uint32), True
        for i in range(n):
            if k in sched[i]:
                c, cb = sched[i][k]
                if cb & wsa.START:
                    books[i].N = books[i].Y = books[i].K = books[i].S = 0
                ctl[i], n_in[i] = cb, c
                stage[i, :c] = sigs[i][pos[i]:pos[i] + c]
                pos[i] += c
                paced_ok = paced_ok and c == books[i].paced()
        use_none = feed == "paced" and paced_ok            # n_in = NULL: the library paces (every step but the signals' cut last ones)
        out["none_steps"] += use_none
        if use_none:
            assert all(int(p) == books[i].paced() for i, p in enumerate(st.paced_input()) if k in sched[i] and not (ctl[i] & wsa.START))
        if host_in:
            st.host_input()[:] = stage
            st.step_host(ctl, _stream(), n_in=None if use_none else n_in)
        else:
            dev.copy_(torch.from_numpy(stage))
            st.step(dev.data_ptr(), dev.stride(0), ctl, _stream(), n_in=None if use_none else n_in)
        r = st.collect(_stream())
        conv = st.converted()
        fr, ou = [], []
        for i in range(n):
            o, f = books[i].step(int(n_in[i]), stop=bool(ctl[i] & wsa.STOP)) if ctl[i] & wsa.ACTIVE else (0, 0)
            assert len(conv[i]) == o, (k, i, len(conv[i]), o)
            assert f <= st.frame_capacity
            out["conv"][i].append(conv[i]); fr.append(f); ou.append(o)
        out["rows"].append(r); out["frames"].append(fr); out["outs"].append(ou); out["ctl"].append(ctl.copy())
        if model is not None:
            out["classes"].append(st.classes())
        assert not r["cuts"].any(), (k, r["cuts"])
    st.close()
    return out


def _batch(wsa, an, sigs, rates, fs_out):
    stride = max(len(x) for x in sigs) + 8
    pcm = torch.zeros((len(sigs), stride), dtype=torch.float32)
    for c, x in enumerate(sigs):
        pcm[c, :len(x)] = torch.from_numpy(x)
    pcm = pcm.cuda().contiguous()
    b = an.batch([len(x) for x in sigs], rates, resample_to=fs_out)
    b.run(pcm.data_ptr(), pcm.stride(0), _stream())
    return b


def _stream_rows(run, n):
    acc = [dict(meta=[], feat=[], segs=[], step=[]) for _ in range(n)]
    for k, r in enumerate(run["rows"]):
        for m, f in zip(r["meta"], r["feat"]):
            acc[int(m[0])]["meta"].append(m[1:].copy()); acc[int(m[0])]["feat"].append(f.copy())
        for sg in r["segments"]:
            acc[int(sg[0])]["segs"].append([int(sg[1]), int(sg[2])]); acc[int(sg[0])]["step"].append(k)
    return acc


def _check_k0s(run, sigs, rates, fs_out, tag):
    from oracle import pyoracle
    refs = []
    for i, (x, r) in enumerate(zip(sigs, rates)):
        ref = x.copy() if r == fs_out else pyoracle.resample(x, r, fs_out)
        got = np.concatenate(run["conv"][i]) if run["conv"][i] else np.zeros(0, np.float32)
        assert len(got) == len(ref), (tag, i, r, len(got), len(ref))
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{tag} stream {i} ({r} Hz): converted samples differ from oracle/resample.c"
        refs.append(ref)
    return refs


CASES = [  # fs_out, frames_per_step, feed, graph, pinned host input, level, compare with the oracle chain
    (48000, 1, "paced", True, False, 5, True),
    (48000, 5, "capacity", True, True, 13, True),
    (16000, 1, "random", False, True, 5, True),
    (16000, 5, "paced", True, False, 13, True),
    (48000, 1, "capacity", False, False, 4, False),
    (48000, 5, "random", True, True, 10, False),
    (16000, 5, "capacity", True, False, 11, False),
    (48000, 5, "paced", True, True, 12, False),
    (16000, 1, "random", True, False, 3, False),
]


@pytest.mark.parametrize("fs_out,F,feed,graph,host_in,level,oracle", CASES)
def test_stream_k0s_bit_exact_and_rows_equal_the_mixed_batch(wsa, fs_out, F, feed, graph, host_in, level, oracle):
    from oracle import pyoracle
    rates, sigs = _signals(fs_out)
    n = len(sigs)
    an = wsa.Analyzer(wsa.Config(output_level=level))
    run = _drive(wsa, an, sigs, rates, fs_out, F, feed, graph, host_in, seed=7 + F)
    tag = f"{fs_out} F{F} {feed} level {level}"
    # K0s bit for bit, whatever the cut into steps
    refs = _check_k0s(run, sigs, rates, fs_out, tag)
    most = max(f for fr, ctl in zip(run["frames"], run["ctl"]) for f, c in zip(fr, ctl) if not c & wsa.STOP)      # (a STOP step adds the tail's frames)
    if feed == "paced":
        assert run["none_steps"] > len(run["rows"]) // 2 and most <= F
    if feed == "capacity" and fs_out == 48000 and F == 5:
        assert most == F + 1, most                          # a step fed its capacity analysed frames_per_step + 1 frames
    if feed == "random":
        assert any(o == 0 for ou in run["outs"] for o in ou)
    # the whole path = the mixed batch on the whole signals
    b = _batch(wsa, an, sigs, rates, fs_out)
    ref = b.callbacks(_stream())
    rows = b.rows(_stream())
    got = _stream_rows(run, n)
    step_s = float(an.config["window_step"]) / 1e3
    cbs = _per_stream_callbacks(run["rows"], n, level, step_s)
    for i in range(n):
        assert len(ref[i]["segments_ci"]) >= 2, (tag, i)     # 6 s of synthetic speech: several segments
        assert got[i]["segs"] == ref[i]["segments_ci"], (tag, i)
        a, e = int(rows["row_off"][i]), int(rows["row_off"][i + 1])
        assert len(got[i]["meta"]) == e - a, (tag, i)
        if e > a and level in (5, 13):
            assert np.array_equal(np.array(got[i]["meta"]), rows["meta"][a:e, 1:]), (tag, i)
            assert np.allclose(np.array(got[i]["feat"]), rows["feat"][a:e], rtol=1e-9, atol=1e-12, equal_nan=True), (tag, i)
        ok, why = callbacks_equal(level, ref[i]["callbacks"], cbs[i], exact=False, tol=1e-9)
        assert ok, (tag, i, why)
    if oracle:
        fe = pyoracle.FrontEnd(pyoracle.fe_cfg(fs=float(fs_out)))
        for i in range(n):
            want = pyoracle.run_backend(fe.run(refs[i]), pyoracle.default_cfg(level=level, bands=fe.bands))
            assert want["segments_ci"] == got[i]["segs"], (tag, i)
            ok, why = callbacks_equal(level, want["callbacks"], cbs[i], exact=False, tol=1e-4)
            assert ok, (tag, i, why)
    b.close(); an.close()


@pytest.mark.parametrize("F", [1, 5])
def test_paced_rows_arrive_in_the_step_that_closes_their_segment(wsa, F):
    """The frame whose analysis reports a segment is taken from a plain one-frame-per-step set fed the batch's converted signals (step k of
    it analyses frame k); the bookkeeping tells in which step of the mixed set that frame is analysed: the segment must arrive right there."""
    fs_out = 48000
    rates, sigs = _signals(fs_out, seconds=4.0)
    n = len(sigs)
    an = wsa.Analyzer(wsa.Config(output_level=5))
    run = _drive(wsa, an, sigs, rates, fs_out, F, "paced", True, True)
    got = _stream_rows(run, n)
    b = _batch(wsa, an, sigs, rates, fs_out)
    ref = b.callbacks(_stream())
    conv = b.converted_pcm(_stream())
    lens = [int(v) for v in b.n_samples]
    hop = an.geometry(fs_out)["hop"]
    plain = an.streams(n, fs_out, frames_per_step=1)
    closing = [dict() for _ in range(n)]
    nfr = [l // hop for l in lens]
    buf = torch.zeros((n, hop), device="cuda", dtype=torch.float32)
    for k in range(max(nfr)):
        ctl = np.array([(wsa.ACTIVE | (wsa.START if k == 0 else 0) | (wsa.STOP if k == nfr[i] - 1 else 0)) if k < nfr[i] else 0 for i in range(n)], np.uint8)
        buf.copy_(torch.from_numpy(np.ascontiguousarray(conv[:, k * hop:(k + 1) * hop])))
        plain.step(buf.data_ptr(), buf.stride(0), ctl, _stream())
        for sg in plain.collect(_stream())["segments"]:
            closing[int(sg[0])][(int(sg[1]), int(sg[2]))] = k
    plain.close()
    checked = 0
    for i in range(n):
        assert got[i]["segs"] == ref[i]["segments_ci"]
        first = np.cumsum([0] + [fr[i] for fr in run["frames"]])          # frames analysed before step k
        for (start, ln), k_got in zip(got[i]["segs"], got[i]["step"]):
            frame = closing[i][(start, ln)]
            k_want = int(np.searchsorted(first, frame, side="right")) - 1
            assert first[k_want] <= frame < first[k_want + 1]
            assert k_got == k_want, (i, start, ln, frame, k_got, k_want)
            checked += 1
    assert checked >= 2 * n
    b.close(); an.close()


@pytest.mark.parametrize("kw", [{}, dict(window_width=25.0, window_step=15.0)])
def test_a_mixed_set_at_the_analysis_rate_is_a_plain_set(wsa, kw):
    from webspeechanalyzer_amd.synth import synth_clips
    fs, n, F = 16000, 6, 3
    pcm = synth_clips(n, 4 * fs, fs=fs, seed=33, device="cuda")
    outs = []
    for mixed in (False, True):
        an = wsa.Analyzer(wsa.Config(output_level=13, **kw))
        st = an.streams(n, [fs] * n, frames_per_step=F, resample_to=fs) if mixed else an.streams(n, fs, frames_per_step=F)
        st.enable_graph(True)
        sps = st.samples_per_step
        assert st.input_stride == sps and list(st.input_capacity) == [sps] * n and st.frame_capacity == F
        nsteps = pcm.shape[1] // sps
        steps = []
        for k in range(nsteps):
            ctl = np.full(n, wsa.ACTIVE | (wsa.START if k == 0 else 0) | (wsa.STOP if k == nsteps - 1 else 0), np.uint8)
            buf = pcm[:, k * sps:(k + 1) * sps].contiguous()
            st.step(buf.data_ptr(), buf.stride(0), ctl, _stream(), n_in=np.full(n, sps, np.uint32) if k % 2 else None)
            steps.append(st.collect(_stream()))
        st.close(); an.close()
        outs.append(steps)
    assert sum(len(r["meta"]) for r in outs[0]) > 10
    for k, (a, b) in enumerate(zip(*outs)):
        assert np.array_equal(a["meta"], b["meta"]), k
        assert np.array_equal(a["feat"].view(np.uint64), b["feat"].view(np.uint64)), k
        assert np.array_equal(a["segments"], b["segments"]), k


def test_restart_idle_stop_with_samples_and_start_in_mid_life(wsa):
    """Stream 0 plays its signal twice (STOP with samples in the step, three idle steps, START again); stream 1 idles through the first
    round; stream 2 gets a START in mid-life without a STOP; stream 3 (at the analysis rate) as stream 0.  Every sub-signal since a START
    equals its own batch clip: converted samples bit for bit, segments and rows."""
    fs_out, F = 48000, 4
    from webspeechanalyzer_amd.synth import synth_clips
    rates = [44100.0, 16000.0, 22050.0, 48000.0]
    sigs1 = [synth_clips(1, int(3.5 * r), fs=int(r), seed=81 + k, device="cpu")[0].numpy().copy() for k, r in enumerate(rates)]
    an = wsa.Analyzer(wsa.Config(output_level=5))
    g = an.geometry(fs_out)
    counts = [M.feed_counts("paced", M.Book(r, fs_out, F, g["win"], g["hop"]), len(x)) for r, x in zip(rates, sigs1)]
    A, S, T = wsa.ACTIVE, wsa.START, wsa.STOP
    round2 = max(len(c) for c in counts) + 3
    plan, sigs, subs = [], [], []
    for i, (cnt, x) in enumerate(zip(counts, sigs1)):
        one = [(k, c, A | (S if k == 0 else 0) | (T if k == len(cnt) - 1 else 0)) for k, c in enumerate(cnt)]
        two = [(round2 + k, c, ctl) for k, c, ctl in one]
        if i == 1:
            plan.append(two); sigs.append(x); subs.append([x])
        elif i == 2:                                        # START again after a third of the signal, no STOP in front of it
            k3 = len(cnt) // 3
            cut = sum(cnt[:k3])
            plan.append([(k, c, ctl | (S if k == k3 else 0)) for k, c, ctl in one]); sigs.append(x); subs.append([x[cut:]])
        else:
            plan.append(one + two); sigs.append(np.concatenate([x, x])); subs.append([x, x])
    run = _drive(wsa, an, sigs, rates, fs_out, F, "paced", True, False, plan=plan)
    assert run["none_steps"] > 0
    n = len(rates)
    # rows per (stream, sub-signal): a START sets the callback index back to 0
    per = [[] for _ in range(n)]
    for k, r in enumerate(run["rows"]):
        for i in range(n):
            if k in {p[0] for p in plan[i] if p[2] & S}:
                per[i].append(dict(meta=[], feat=[], segs=[], conv=[]))
            if per[i]:
                per[i][-1]["conv"].append(run["conv"][i][k])
        for m, f in zip(r["meta"], r["feat"]):
            per[int(m[0])][-1]["meta"].append(m[1:].copy()); per[int(m[0])][-1]["feat"].append(f.copy())
        for sg in r["segments"]:
            per[int(sg[0])][-1]["segs"].append([int(sg[1]), int(sg[2])])
    from oracle import pyoracle
    for i in range(n):
        runs = per[i][1:] if i == 2 else per[i]              # stream 2's first START covers the part that was abandoned
        assert len(runs) == len(subs[i]), i
        for got, x in zip(runs, subs[i]):
            b = _batch(wsa, an, [x], [rates[i]], fs_out)
            ref, rows = b.callbacks(_stream())[0], b.rows(_stream())
            want = x if rates[i] == fs_out else pyoracle.resample(x, rates[i], fs_out)
            conv = np.concatenate(got["conv"])
            assert len(conv) == len(want) and np.array_equal(conv.view(np.uint32), want.view(np.uint32)), i
            assert got["segs"] == ref["segments_ci"] and len(got["segs"]) >= 1, i
            assert np.array_equal(np.array(got["meta"]), rows["meta"][:, 1:]), i
            assert np.allclose(np.array(got["feat"]), rows["feat"], rtol=1e-9, atol=1e-12, equal_nan=True), i
            b.close()
    an.close()


def test_classifier_on_the_44k_excerpt_fed_directly(wsa):
    """The committed 44.1 kHz excerpt goes into a mixed level-13 set as it is, paced, with the fixture's settings (25 ms windows every 15 ms):
    segments and timestamps are the reference back end's, features within the contract, and the classifier inside the step gives what
    wsa_batch_classify gives for the excerpt converted by the batch."""
    from webspeechanalyzer_amd import nnmodel
    exc = np.load(os.path.join(GOLD, "config1_excerpt.npz"))
    EXP = json.load(open(os.path.join(GOLD, "config1_expected.json")))
    S = EXP["settings"]
    x = (exc["pcm_i16"].astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    fs, fs_out = float(exc["fs"]), float(S["fs_context"])
    cfg = wsa.Config(output_level=13, window_step=S["window_step"], pause_length=S["pause_length"], min_seg_length=S["min_seg_length"])
    an = wsa.Analyzer(cfg)
    assert an.geometry(fs_out)["hop"] == 720 and an.geometry(fs_out)["win"] == 1200
    spec = nnmodel.load_dir(os.path.join(GOLD, "nn", "1/cats_emotion"))
    m = an.load_model(spec)
    run = _drive(wsa, an, [x], [fs], fs_out, 1, "paced", True, True, model=m)
    assert run["none_steps"] >= len(run["rows"]) - 1
    got = _stream_rows(run, 1)[0]
    ref = EXP["excerpt"]["level13"]
    assert got["segs"] == ref["segments_ci"]
    cbs = _per_stream_callbacks(run["rows"], 1, 13, S["window_step"] / 1e3)[0]
    ok, why = callbacks_equal(13, ref["callbacks"], cbs, exact=False, tol=1e-4)
    assert ok, why
    b = _batch(wsa, an, [x], [fs], fs_out)
    b.classify(m, _stream())
    want, rows = b.classes(_stream()), b.rows(_stream())
    assert len(want["cb"]) > 0
    assert np.array_equal(np.array(got["meta"]), rows["meta"][:, 1:])
    assert np.array_equal(np.array(got["feat"]), rows["feat"], equal_nan=True)
    prob = np.concatenate([c["prob"] for c in run["classes"] if len(c["prob"])])
    assert np.array_equal(prob, want["prob"])                # bit for bit, as between a plain stream set and the batch
    scb = [(int(e[1]), int(e[3]), int(c["cb_label"][q]), float(c["cb_conf"][q])) for c in run["classes"] for q, e in enumerate(c["cb"])]
    wcb = [(int(e[1]), int(e[3]), int(want["cb_label"][k]), float(want["cb_conf"][k])) for k, e in enumerate(want["cb"])]
    assert scb == wcb
    assert np.array_equal(run["classes"][-1]["stream_conf"][0], want["clip_conf"][0])
    b.close(); m.close(); an.close()


def test_refusals_name_the_stream(wsa):
    an = wsa.Analyzer(wsa.Config(output_level=5))
    for bad in (0.0, -16000.0, 2000.0, 800000.0):
        with pytest.raises(wsa.WsaError, match=r"sample rates.*stream 1"):
            an.streams(3, [16000.0, bad, 44100.0], resample_to=48000)
    with pytest.raises(wsa.WsaError, match="one rate per stream"):
        an.streams(2, [16000.0, 44100.0])
    st = an.streams(3, [16000.0, 44100.0, 48000.0], frames_per_step=2, resample_to=48000)
    cap = st.input_capacity
    assert list(cap) == [800, 2205, 2400]
    n_in = cap.copy(); n_in[1] += 1
    with pytest.raises(wsa.WsaError, match=r"stream 1.*capacity"):
        st.step_host(None, _stream(), n_in=n_in)
    st.step_host(None, _stream(), n_in=cap)                  # the refusal counted nothing: the capacity itself goes through
    st.collect(_stream())
    assert [len(c) for c in st.converted()] == [M.ready(800, 16000.0, 48000.0), M.ready(2205, 44100.0, 48000.0), 2400]
    st.close()
    plain = an.streams(3, 48000, frames_per_step=2)
    wrong = np.array([2400, 2400, 2399], np.uint32)
    with pytest.raises(wsa.WsaError, match=r"stream 2.*exactly 2400"):
        plain.step_host(None, _stream(), n_in=wrong)
    plain.step_host(None, _stream(), n_in=np.full(3, 2400, np.uint32))
    plain.collect(_stream())
    with pytest.raises(wsa.WsaError, match="wsa_stream_create_mixed"):
        plain.converted()
    plain.close(); an.close()

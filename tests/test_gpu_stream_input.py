"""The input half of a plain stream set's step on the hand-built stream sets of tests/stream_input_cases.py (-m gpu): plan_plain_step, the history
shuffle stream_stage_kernel, the float pull stream_pull_kernel and the packed pull, and the front end as a step launches it (n_frames and pcm_off per
stream from the control words, one chunk per stream up to F = 100 and two from 101 on).  Every (geometry, F) set steps through Streams.step / step_host
and collect; after EVERY step
  * the control words on the device (test entry wsa_debug_stream_ctl) equal the model's (nfr, off, bits);
  * slots 0 .. nfr - 1 of every stream in d_spec (wsa_debug_stream_spectra) equal the oracle FE-1's frames of the launch clip at the model's indices:
    u32, bit for bit, no tolerance, no case left out;
  * slots nfr .. F - 1 hold what the step before left there (an all-idle first step and a read-back seed them).
Arrangements, all against the same expected frames: graph off and on (captured on the set's second step, which is the schedule's first; F, stride and
pointer stay put, so it is replayed), device floats at row stride samples_per_step and samples_per_step + 37 (NaN in the padding), the pinned host
input, and at 16k-25-10 and 22k05-25-20 WSA_PCM_I16 from the pinned packed buffer (expected frames from the host's decode of the codes).
One end-to-end check per geometry at level 5, on synthetic speech: the rows of launch B in each restart schedule equal, meta and features bit for bit,
the rows of a fresh stream set fed launch B alone.

Figures (an MI355X; this file's output, `pytest -s`): 39 tests in 5 s, the slowest 0.4 s (16k-25-10 at F = 101: 8 arrangements of 13 steps, 7 351
expected frames).  31 stream sets (geometry x F), 6 arrangements each and 8 at the two 16-bit geometries: 204 sets stepped, 2 838 steps (each set's all-idle first step among them), every
one compared in full; 22 571 expected frames per pass of the float arrangements.  The end-to-end check compares 4 or 5 rows of launch B per geometry (every
restart schedule closes at least one row; an empty comparison fails).
  geometry      instantiation (wsa_debug_fe_choice)   frames per step
  16k-25-10     fe_kernel_r8<4,5,8,true,4,3>          1, 2, 3, 5, 100, 101
  16k-30-10     fe_kernel_r8<4,5,8,true,4,3>          1, 2, 3, 5
  22k05-25-20   fe_kernel_r3<4,5,14,3>                1, 2, 5
  48k-60-10     fe_kernel_r3<8,24,14>                 1, 2, 5, 6, 4
  16k-16-1      fe_kernel_r8<2,9,12,false>            1, 2, 15, 16, 5
  8k-16-1       fe_kernel_rx<4,2,12>                  1, 2, 15, 16, 5
  16k-10-25     fe_kernel_r8<2,9,12,false>            1, 2, 5
No fault found: plan_plain_step, the stage, the pulls and the front end's chunks passed every case as they were.

Mutation check (scratch builds of libwsa, nothing committed; changes that keep every address inside the stage row or the caller's row; each ran once
with -x; all failures were comparisons, none faulted).  Every one failed in the first test, 16k-25-10 F = 1, device floats, graph off:
  fault                change                                                     first failure
  warm = q             plan_plain_step: START sets warm = q                       step 2: control words nfr 0, off 160 where the model has nfr 1, off 0 (every
                                                                                  stream whose warm-up ends there)
  off = 0              plan_plain_step: off = 0                                   step 0: control words off 0, model 160
  shuffle stores 0     stream_stage_kernel: st[i] = 0.0f in place of s_hist[i]    step 2, stream 0 (plain), slot 0, band 0: device 361, oracle 9046
                                                                                  (launch 0 frame 0); 4 slots differ
  idle test removed    stream_stage_kernel without its `return` for idle streams  step 4, stream 6 (pause), slot 0, band 0: device 0, oracle 12303
                                                                                  (launch 0 frame 1: the idle row's NaN went into the history)
  START keeps warm     plan_plain_step: the START line removed                    step 0: control words nfr 1, off 0, model nfr 0, off 160
Faults that would move an address (st[step_samples + i] -> st[i], off in frames, warm = q - 2 reading in front of the first step's samples) are shown
on the CPU restatement only (tests/test_stream_input_reference.py).
"""
import numpy as np
import pytest

from tests import stream_input_cases as sc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def wsa():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import webspeechanalyzer_amd as w
    return w


class _Feeder:
    """hands a step's rows to a stream set in one arrangement, the input pointer and stride the same in every step"""

    def __init__(self, st, case, how):
        self.st, self.how, self.sps = st, how, case.sps
        if how == "i16":
            st.set_input_format("i16")
            self.buf = st.host_input_packed()
            assert self.buf.dtype == np.int16 and self.buf.shape[1] >= case.sps
            self.buf[:] = 32767
        elif how == "host":
            self.buf = st.host_input()
            assert self.buf.shape == (sc.N_STREAMS, case.sps)
        else:
            self.stride = case.sps + (37 if how == "dev+37" else 0)
            self.host = np.full((sc.N_STREAMS, self.stride), np.nan, np.float32)
            self.dev = torch.full((sc.N_STREAMS, self.stride), float("nan"), dtype=torch.float32, device="cuda")

    def step(self, rows, ctl):
        if self.how in ("i16", "host"):
            self.buf[:, :self.sps] = rows
            self.st.step_host(ctl, _stream())
        else:
            self.host[:, :self.sps] = rows
            self.dev.copy_(torch.from_numpy(self.host))
            self.st.step(self.dev.data_ptr(), self.dev.stride(0), ctl, _stream())
        return self.st.collect(_stream())


def _idle_rows(case, how):
    return np.full((sc.N_STREAMS, case.sps), 32767, np.int16) if how == "i16" else np.full((sc.N_STREAMS, case.sps), np.nan, np.float32)


def _check_set(wsa, an, case, how, graph):
    from webspeechanalyzer_amd import capi
    g, F, n = case.geometry, case.F, sc.N_STREAMS
    fmt = "i16" if how == "i16" else "f32"
    want = case.expected(fmt)
    st = an.streams(n, g.fs, frames_per_step=F)
    try:
        st.enable_graph(graph)
        assert st.samples_per_step == case.sps and st.frame_capacity == F
        feed = _Feeder(st, case, how)
        feed.step(_idle_rows(case, how), np.zeros(n, np.uint8))
        bands = g.oracle().bands
        prev = capi.debug_stream_spectra(st, bands)
        assert not capi.debug_stream_ctl(st).any()
        for k in range(case.steps):
            feed.step(case.rows(k, fmt), case.ctl[k])
            words, spec = capi.debug_stream_ctl(st), capi.debug_stream_spectra(st, bands)
            what = f"{case.name} {how} graph {graph} step {k}"
            model = np.array([[case.plan[s][k][i] for s in range(n)] for i in range(3)], np.uint32)
            assert np.array_equal(words, model), f"{what}: control words (nfr, off, bits) {words.tolist()}, model {model.tolist()}"
            expect = prev.copy()
            for s in range(n):
                for j, (w, fr) in enumerate(case.plan[s][k][3]):
                    expect[s, j] = want[s][w][fr]
            if not np.array_equal(spec, expect):
                s, j, m = (int(x) for x in np.argwhere(spec != expect)[0])
                nfr = case.plan[s][k][0]
                where = f"launch {case.plan[s][k][3][j][0]} frame {case.plan[s][k][3][j][1]}" if j < nfr else f"behind nfr = {nfr}: the step before left {expect[s, j, m]}"
                raise AssertionError(f"{what}: stream {s} ({sc.SCHEDULES[s]}) slot {j} band {m}: device {spec[s, j, m]}, oracle {expect[s, j, m]} ({where}); "
                                     f"{int((spec != expect).any(axis=2).sum())} slots differ")
            prev = spec
    finally:
        st.close()
    return case.steps + 1


@pytest.mark.parametrize("gname,F", [(g.name, F) for g in sc.GEOMETRIES for F in g.frames_per_step])
def test_every_step_delivers_the_models_frames_in_every_arrangement(wsa, gname, F):
    from webspeechanalyzer_amd import capi
    g, case = sc.BY_NAME[gname], sc.case(gname, F)
    an = wsa.Analyzer(wsa.Config(output_level=5, **g.config_kw))
    try:
        geo = an.geometry(g.fs)
        assert (geo["win"], geo["hop"]) == (g.win, g.hop) and g.q == -(-geo["win"] // geo["hop"]) and g.hist == (g.q - 1) * geo["hop"]
        assert geo["bands"] == g.oracle().bands
        hows = ("dev", "dev+37", "host") + (("i16",) if gname in sc.I16_GEOMETRIES else ())
        steps = sum(_check_set(wsa, an, case, how, graph) for how in hows for graph in (False, True))
        inst = capi.debug_fe_choice(an, g.fs)
        print(f"\n{case.name}: {inst}, {len(hows) * 2} arrangements, {steps} steps, {sum(len(x) for per in case.expected() for x in per)} expected frames")
        assert inst == g.inst
    finally:
        an.close()


def test_the_test_entry_refuses_a_mixed_set(wsa):
    from webspeechanalyzer_amd import capi
    an = wsa.Analyzer(wsa.Config(output_level=5))
    st = an.streams(2, [8000.0, 16000.0], frames_per_step=1, resample_to=16000.0)
    with pytest.raises(wsa.WsaError, match="wsa_debug_stream_ctl: error 1"):
        capi.debug_stream_ctl(st)
    st.close(); an.close()


def _rows_of(case, an, picks, max_span):
    """Step a fresh 7-stream set: picks[s] = the schedule steps stream s lives through, in order (None: all of them).  -> per stream the rows
    (meta bytes, feat bytes) of every step, as [(step index within picks, meta, feat)]"""
    g, n = case.geometry, sc.N_STREAMS
    st = an.streams(n, g.fs, frames_per_step=case.F, max_span_frames=max_span)
    st.enable_graph(True)
    feed = _Feeder(st, case, "dev")
    out = [[] for _ in range(n)]
    total = max(len(p) for p in picks)
    for t in range(total):
        rows, ctl = _idle_rows(case, "dev"), np.zeros(n, np.uint8)
        for s in range(n):
            if t < len(picks[s]):
                k = picks[s][t]
                rows[s], ctl[s] = case.rows(k)[s], case.ctl[k, s]
        r = feed.step(rows, ctl)
        assert not r["cuts"].any() and not (r["flags"] & 1)
        for m, f in zip(r["meta"], r["feat"]):
            out[int(m[0])].append((t, m.tobytes(), f.tobytes()))
    st.close()
    return out


@pytest.mark.parametrize("gname", [g.name for g in sc.GEOMETRIES])
def test_a_restarted_launch_gives_the_rows_of_a_fresh_one(wsa, gname):
    """Carried input state is one way to break this, carried back-end state another."""
    g, case = sc.BY_NAME[gname], sc.speech_case(gname)
    an = wsa.Analyzer(wsa.Config(output_level=5, **g.config_kw))
    try:
        every = [list(range(case.steps))] * sc.N_STREAMS
        whole = _rows_of(case, an, every, 2048)
        b_steps = [[k for k in range(case.steps) if case.launch[s][k] == 1] if name in sc.RESTARTS else [] for s, name in enumerate(sc.SCHEDULES)]
        alone = _rows_of(case, an, b_steps, 2048)
        n_rows = 0
        for s, name in enumerate(sc.SCHEDULES):
            if name not in sc.RESTARTS:
                assert alone[s] == []
                continue
            first = b_steps[s][0]
            got = [(t - first, m, f) for t, m, f in whole[s] if t >= first]
            assert got == alone[s], f"{case.name} stream {s} ({name}): {len(got)} rows of launch B behind launch A, {len(alone[s])} from a fresh set"
            assert len(got) > 0, f"{case.name} stream {s} ({name}): launch B closes no row, the check is empty"
            n_rows += len(got)
        print(f"\n{case.name}: {n_rows} rows of launch B in {len(sc.RESTARTS)} restart schedules")
    finally:
        an.close()

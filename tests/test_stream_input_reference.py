"""The input half of a plain stream set's step, restated in numpy and held against the model of tests/stream_input_cases.py on every case.  No GPU.

The restatement (device_run) follows the device forms line for line: plan_plain_step's warm-up counter (`warm = q - 1` at START, `skip = min(warm, F)`,
`nfr = F - skip`, `off = skip hop`), stream_stage_kernel's row [hist | step_samples] with the history taken out of stage[step_samples .. step_samples +
hist) and no shuffle for an idle stream, and the front end's frame j at stage[off + j hop .. + win) (hist == 0: at the caller's row).  The stage starts as
NaN here, not as the zeros the device allocates: the faultless restatement then proves that no delivered frame reads what no step wrote.  Every window
it extracts must equal the launch clip's samples [k hop, k hop + win) under the model's (launch, k), NaN equal to NaN, and its control words the model's.

The faults are one-line changes of the restatement, one per arm.  Each must change the u32 FRAMES of the case named for its arm (FAULTS below): the
faulty windows go through the oracle FE-1 and are compared as tests/test_gpu_stream_input.py compares a step - slots 0 .. nfr - 1 against the launch's
frames, the slots behind them against what the step before left, the control words against the model's.  Samples alone do not count: a Hann window gives
a window's first sample the weight 0.

Analyzer.geometry needs a device, so q and hist are asserted here from the oracle's win and hop, and from Analyzer.geometry in the GPU file.

Measured (this file's output, `pytest -s`): 31 stream sets over 7 geometries; all 22 571 frames the oracle makes of the launches' clips are delivered,
and every fault changes its named case (step, stream; with the control words compared / with the u32 frames alone):
  fault                 named case                        words and frames                           frames alone
  hist_zeros            16k-25-10-F1 plain                step 2, slot 0: launch 0 frame 0           the same
  hist_from_stage_0     48k-60-10-F1 plain                step 5, slot 0: launch 0 frame 0           the same
  warm_q                16k-25-10-F1 plain                step 2: words (0, 160, 4), model (1, 0, 4) step 2, slot 0: launch 0 frame 0
  warm_q_minus_2        16k-30-10-F2 plain                step 0: words (1, 160, 5), model (0, 320, 5) step 0: a slot behind nfr = 0 was written
  off_in_frames         16k-25-10-F5 plain                step 0: words (3, 2, 5), model (3, 320, 5) step 0, slot 0: launch 0 frame 0
  off_zero              16k-25-10-F5 plain                step 0: words (3, 0, 5), model (3, 320, 5) step 0, slot 0: launch 0 frame 0
  warm_not_reset        16k-25-10-F2 restart-in-warm-up   step 6: words (2, 0, 5), model (0, 320, 5) step 6: a slot behind nfr = 0 was written
  idle_shuffled         48k-60-10-F1 pause                step 8, slot 0: launch 0 frame 0           the same
  idle_row_copied       16k-25-10-F2 pause                step 4, slot 0: launch 0 frame 4           the same
  start_keeps_history   16k-30-10-F3 restart-live         step 0: words (3, 0, 5), model (1, 320, 5) step 0, slot 0: launch 0 frame 0
"""
import numpy as np
import pytest

from tests import stream_input_cases as sc

# fault -> (geometry, F, schedule) of the case named for its arm
FAULTS = {
    "hist_zeros": ("16k-25-10", 1, "plain"),                       # history written as zeros
    "hist_from_stage_0": ("48k-60-10", 1, "plain"),                # history taken from stage[0 ...)
    "warm_q": ("16k-25-10", 1, "plain"),
    "warm_q_minus_2": ("16k-30-10", 2, "plain"),
    "off_in_frames": ("16k-25-10", 5, "plain"),                    # off in frames instead of samples
    "off_zero": ("16k-25-10", 5, "plain"),
    # only a stream's first START sets the counter.  (Not a poisoned schedule: there launch A's last frames are zeros, the frames launch B wrongly
    # delivers out of the poisoned history are zeros too, and with the control words left out the slots look untouched.)
    "warm_not_reset": ("16k-25-10", 2, "restart-in-warm-up"),
    "idle_shuffled": ("48k-60-10", 1, "pause"),                    # an idle stream's history shuffled (its row not copied)
    "idle_row_copied": ("16k-25-10", 2, "pause"),                  # the idle test removed: shuffle and copy
    "start_keeps_history": ("16k-30-10", 3, "restart-live"),       # START trusting a step of F >= q - 1 frames to need no warm-up
}

# Faults that no case can show at the level of frames, with the argument.  None of the ten is equivalent everywhere; one is on a part of the cases:
#   idle_shuffled with F >= q - 1 (hist <= step_samples): the shuffle reads stage[step_samples .. step_samples + hist), which lies wholly in the part of
#   the row the shuffle does not write, so shuffling an idle stream any number of times leaves [H | new] with the same H the next active step takes from
#   the same place.  test_idle_shuffle_shows_only_where_history_exceeds_the_step asserts both halves.
EQUIVALENT = {}


def device_run(case, fault=None, fmt="f32"):
    """-> per step: (words [3, n] = nfr, off, bits; windows [n][nfr] float32 arrays of win samples)"""
    g, F, n = case.geometry, case.F, sc.N_STREAMS
    q, hop, win, hist, sps = g.q, g.hop, g.win, g.hist, case.sps
    stage = np.full((n, hist + sps), np.nan, np.float32)
    warm = [0] * n
    started = [False] * n
    out = []
    for k in range(case.steps):
        rows = case.rows(k, fmt)
        if fmt != "f32":
            from webspeechanalyzer_amd import capi
            rows = np.stack([capi.pcm_decode("i16", r) for r in rows])
        words = np.zeros((3, n), np.uint32)
        windows = []
        for s in range(n):
            cb = int(case.ctl[k, s])
            nfr = off = 0
            if cb & sc.START:
                if not (fault == "warm_not_reset" and started[s]) and not (fault == "start_keeps_history" and F >= q - 1):
                    warm[s] = q if fault == "warm_q" else max(q - 2, 0) if fault == "warm_q_minus_2" else q - 1
                started[s] = True
            if cb & sc.ACTIVE:
                skip = min(warm[s], F)
                warm[s] -= skip
                nfr = F - skip
                off = skip if fault == "off_in_frames" else 0 if fault == "off_zero" else skip * hop
            words[:, s] = nfr, off, sc.device_bits(cb)
            src = rows[s]
            if hist:
                active = bool(cb & sc.ACTIVE)
                if active or fault in ("idle_shuffled", "idle_row_copied"):
                    st = stage[s]
                    if fault == "hist_zeros":
                        st[:hist] = 0.0
                    elif fault != "hist_from_stage_0":
                        st[:hist] = st[sps:sps + hist].copy()
                    if active or fault == "idle_row_copied":
                        st[hist:] = rows[s]
                src = stage[s]
            windows.append([src[off + j * hop:off + j * hop + win].copy() for j in range(nfr)])
        out.append((words, windows))
    return out


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _model_words(case, k):
    return np.array([[case.plan[s][k][i] for s in range(sc.N_STREAMS)] for i in range(3)], np.uint32)


@pytest.mark.parametrize("gname", [g.name for g in sc.GEOMETRIES])
def test_geometry_is_the_tables(gname):
    g = sc.BY_NAME[gname]
    fe = g.oracle()
    assert (fe.win, fe.hop) == (g.win, g.hop)
    assert g.q == -(-fe.win // fe.hop) and g.hist == (g.q - 1) * fe.hop
    assert len(g.frames_per_step) == len(set(g.frames_per_step)) and 0 not in g.frames_per_step


def test_schedules_hold_what_their_names_say():
    for case in sc.all_cases():
        g, F = case.geometry, case.F
        by = dict(zip(sc.SCHEDULES, range(sc.N_STREAMS)))
        assert case.steps == max(12, sc.warm_steps(g.q, F) + 8)
        ctl = case.ctl
        for name, s in by.items():
            c = [int(x) for x in ctl[:, s]]
            starts = [k for k, x in enumerate(c) if x & sc.START]
            assert len(starts) == (2 if name in sc.RESTARTS else 1), (case.name, name)
            assert c[-1] & sc.STOP and all(x & sc.ACTIVE for x in c if x & (sc.START | sc.STOP))
            if name == "late-start":
                assert starts == [3] and c[:3] == [0, 0, 0]
            if name == "restart-after-stop":
                assert c[starts[1] - 1] & sc.STOP
            if name == "restart-after-idle":
                assert c[starts[1] - 1] == 0 and c[starts[1] - 2] == 0 and c[starts[1] - 3] & sc.STOP
            if name == "restart-live":
                assert c[starts[1] - 1] == sc.ACTIVE or starts[1] - 1 == 0
            if name == "restart-in-warm-up" and F < g.q - 1:
                assert starts[1] * F < g.q - 1                     # the first launch's warm-up counter is still above 0
            if name == "pause":
                runs, k = [], 0
                while k < len(c):
                    if c[k] == 0:
                        j = k
                        while c[j] == 0:
                            j += 1
                        runs.append(j - k); k = j
                    else:
                        k += 1
                assert runs[:2] == [1, 2] and len(runs) == 3 and (runs[2] == g.q or 3 <= runs[2] < g.q), (case.name, runs)
            # every launch that the model lets deliver frames delivers some; launch B always does
            delivered = {}
            for step in case.plan[s]:
                for (w, _) in step[3]:
                    delivered[w] = delivered.get(w, 0) + 1
            assert delivered.get(len(case.clips[s]) - 1, 0) >= 1, (case.name, name)
        # a step holds streams with nfr = 0, partial and F side by side (partial needs 0 < (q - 1) mod F or F > q - 1 > 0)
        kinds = set()
        for k in range(case.steps):
            here = {case.plan[s][k][0] for s in range(sc.N_STREAMS)}
            if 0 in here and F in here:
                kinds.add("zero-and-full")
            if any(0 < x < F for x in here) and (0 in here or F in here):
                kinds.add("partial")
        assert "zero-and-full" in kinds, case.name
        if (g.q - 1) % F:
            assert "partial" in kinds, case.name


def test_the_restatement_delivers_the_models_frames_on_every_case():
    n_sets = n_frames = 0
    for case in sc.all_cases():
        g = case.geometry
        for fmt in ("f32",) + (("i16",) if g.name in sc.I16_GEOMETRIES and case.F <= 5 else ()):
            for k, (words, windows) in enumerate(device_run(case, None, fmt)):
                assert np.array_equal(words, _model_words(case, k)), (case.name, k, words, _model_words(case, k))
                for s in range(sc.N_STREAMS):
                    slots = case.plan[s][k][3]
                    assert len(windows[s]) == len(slots)
                    for x, (w, fr) in zip(windows[s], slots):
                        assert _same_bits(x, case.clip(s, w, fmt)[fr * g.hop:fr * g.hop + g.win]), (case.name, fmt, k, s, w, fr)
                        n_frames += fmt == "f32"
        n_sets += 1
    total = sum(len(x) for case in sc.all_cases() for per in case.expected() for x in per)
    print(f"\n{n_sets} stream sets over {len(sc.GEOMETRIES)} geometries, {n_frames} delivered frames of {total} expected")
    # every frame the oracle makes of a launch's clip is delivered: a clip of T F hop samples holds T F - q + 1 frames, and frame T F - q is the last
    # whose (k + q) hop samples have arrived
    assert n_frames == total


def frames_under(case, fault, words_too=True, only=None):
    """The first difference a GPU-style comparison of the (faulty) restatement finds, or None: (step, stream, what).  only: a stream index."""
    g, fe = case.geometry, case.geometry.oracle()
    want = case.expected()
    spec = np.full((sc.N_STREAMS, case.F, fe.bands), 0xDEADBEEF, np.uint32)       # what an all-idle first step would leave
    for k, (words, windows) in enumerate(device_run(case, fault)):
        prev = spec.copy()
        for s in range(sc.N_STREAMS):
            for j, x in enumerate(windows[s]):
                spec[s, j] = fe.run(x)[0]
        for s in range(sc.N_STREAMS) if only is None else (only,):
            nfr, off, bits, slots = case.plan[s][k]
            if words_too and tuple(int(x) for x in words[:, s]) != (nfr, off, bits):
                return k, s, f"words {tuple(int(x) for x in words[:, s])}, model {(nfr, off, bits)}"
            for j, (w, fr) in enumerate(slots):
                if not np.array_equal(spec[s, j], want[s][w][fr]):
                    return k, s, f"slot {j}: launch {w} frame {fr}"
            if not np.array_equal(spec[s, nfr:], prev[s, nfr:]):
                return k, s, f"a slot behind nfr = {nfr} was written"
    return None


@pytest.mark.parametrize("words_too", [True, False])
def test_every_fault_changes_frames(words_too):
    """words_too False: the u32 frames alone, the control words not looked at"""
    assert set(FAULTS) | set(EQUIVALENT) == set(FAULTS) and not EQUIVALENT
    print()
    for fault, (gname, F, name) in FAULTS.items():
        case = sc.case(gname, F)
        s = sc.SCHEDULES.index(name)
        assert frames_under(case, None, words_too, only=s) is None
        hit = frames_under(case, fault, words_too, only=s)
        print(f"{fault:24s}{case.name} {name}: {hit}")
        assert hit is not None, (fault, case.name, name)


def test_idle_shuffle_shows_only_where_history_exceeds_the_step():
    for case in sc.all_cases():
        g = case.geometry
        if not g.hist or case.F > 16:
            continue
        hit = frames_under(case, "idle_shuffled", only=sc.SCHEDULES.index("pause"))
        if case.F >= g.q - 1:
            assert hit is None, (case.name, hit)                   # the argument at EQUIVALENT
        else:
            assert hit is not None, case.name


def test_conditions_on_the_inputs():
    for case in sc.all_cases():
        g, fe = case.geometry, case.geometry.oracle()
        want = case.expected()
        for s, name in enumerate(sc.SCHEDULES):
            for w, fr in enumerate(want[s]):
                bad = case.poisoned_frames(s, w)
                assert bool(bad) == (w == 0 and name in sc.POISONED and g.hist > 0 and len(fr) > 0), (case.name, name, w)
                for k in range(len(fr)):
                    if k in bad:
                        assert not fr[k].any(), (case.name, name, w, k)                    # F8: a NaN sample in the window, zeros out
                    else:
                        assert fr[k].any(), (case.name, name, w, k)                        # no other frame is all zero
                    if k and not (k in bad and k - 1 in bad):
                        assert not np.array_equal(fr[k], fr[k - 1]), (case.name, name, w, k)    # consecutive frames differ
            if name in sc.RESTARTS and g.hist:
                # launch B behind launch A's history is not launch B: every frame that reaches into the history differs, with the history as the
                # device holds it (NaN where poisoned) and with the samples launch A would have had there
                a, b = case.clips[s][0], case.clips[s][1]
                tail = a[-g.hist:] if len(a) >= g.hist else np.concatenate([np.zeros(g.hist - len(a), np.float32), a])
                clean = np.where(np.isnan(tail), sc._noise(g, s, 0, max(len(a), g.hist))[-g.hist:], tail)
                for hist in (tail, clean):
                    mixed = fe.run(np.concatenate([hist, b]))
                    for k in range(min(g.q - 1, len(want[s][1]))):
                        assert not np.array_equal(mixed[k], want[s][1][k]), (case.name, name, k)
                    assert np.array_equal(mixed[g.q - 1:], want[s][1][:len(mixed) - g.q + 1])

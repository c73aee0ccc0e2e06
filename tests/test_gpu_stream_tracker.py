"""The stream form of the formant tracker (csrc/tracker.hip stream_body, csrc/tracker_one.hpp track_stream; tracker_kernel_stream / _stream_raw) on the
hand-built clips of tests/tracker_rule_cases.py and tests/tracker_cases.py, cut at every step boundary: the arrangements of tests/stream_tracker_cases.py
(alone-1 / 2 / 3 / 7 / 64, ragged, chained over the smallest ring, and a span the ring cuts) go through the test entry wsa_debug_stream_step_backend —
a step's u32 frames past the front end, then the product's own launches from the peak scan down — and wsa_stream_collect.
tests/test_stream_tracker_reference.py shows from the oracle alone which carried state the boundaries fall on: live tracks in the first, second and third
pass of 64 of the saved table, dead entries, a set stale filing index, between a span's last accumulate and its finalize, right behind a finalize, steps that
close two segments or close one and start the next, STOP, the automatic gate's reset, steps of no frames, spans across the ring's end, a cut.

Per family and level (3, 10, 5, 13):
  against the batch    per stream the collected segments, row meta (time columns included), features, level-10 frames and level-3 ranked raw tracks equal BIT
                       FOR BIT what wsa_batch_run_backend gives for the same frames as one clip — the batch under the default variant and under WSA_FULL_TABLE,
                       the streams under either (the stream kernels have one table, the full one)
  against the oracle   indices, timestamps, level-3 and level-10 contents exact; features within the contract (1e-4) and the canary of
                       test_gpu_tracker_limits.py (1e-12, or eight times the oracle's own distance from the long-double sums)
  across arrangements  all alone-F and ragged arrangements give every case the same rows, bit for bit
  flags                no overflow flag, no WSA_FLAG_STREAM_CUT and no stream_cuts anywhere but in `cut`; there the cut stream equals the oracle with the cut
                       (pyoracle.run_backend(cuts=...)), counts one cut, and its neighbour equals the batch and the oracle as everywhere else
The graph: test_the_graphed_product_step_equals_the_debug_entry runs synthetic speech through wsa_stream_step with the graph on, seven frames per step, and
the u32 frames of the same audio through the debug entry: the same rows step by step, bit for bit (the split of the step into its input and its back-end half
moved the launches, nothing else; the existing stream tests are the assertion proper).

Measured on an MI355X, worst relative error of a feature against the oracle over all arrangements and both variants (canary 1e-12, in lim-low 5.7e-08 for
the streams that hold low-max: the oracle's own distance; everything else is exact, and every stream equalled its batch clip bit for bit):
  f1        41 cases   chained 10 streams x 151 steps, cut 2 x 212   level 5 2.24e-15   level 13 5.22e-16
  f10        1 case    chained  1 x 56                               level 5 0          level 13 0
  f100       1 case    chained  1 x 56                               level 5 0          level 13 0
  frac       1 case    chained  1 x 56                               level 5 0          level 13 0
  f1e8       1 case    chained  1 x 56                               level 5 0          level 13 0
  auto       1 case    chained  2 x 73                               level 5 1.23e-16   level 13 0
  b200       3 cases   chained  1 x 56                               level 5 0          level 13 0      (a stream set takes 200 bands: the family runs)
  lim-low   12 cases   chained  5 x 55                               level 5 7.72e-16   level 13 7.68e-16
  lim-high   6 cases   chained  3 x 67                               level 5 5.97e-16   level 13 6.12e-16
  lim-auto   4 cases   chained  5 x 66                               level 5 3.61e-15   level 13 2.34e-15
The whole file takes 14 seconds (42 tests; the largest, a level-3 family with all its arrangements under both variants, under two seconds).  No test
exposed a fault of the kernel.

Mutation check (scratch builds of libwsa.so with one line of track_stream changed, nothing committed; the main test run once per build with -x, the first
failing run and the cases it names).  Values only: no address, index, loop bound or count was changed.
  `accG = std_[0] + std_[1]` -> `std_[0]`                       f1 alone-1 level 5: the features of all 41 cases (levels 3 and 10 pass: the sums feed features only)
  `accL` restored on every lane                                  f1 alone-1 level 5: all 41 cases
  `g_vel` restored as 0                                          f1 alone-1 level 3: pairs-split, velocity-decides, velocity-t-negative, velocity-third-decides
  `g_sumE` and `g_sumEbin` swapped at the restore                f1 alone-1 level 3: all 41 cases (`callback count 2 != 0`: no segment reports tracks)
  `g_amp` restored as 0                                          f1 alone-1 level 3: all 41 cases (`callback count 2 != 0`)
  `g_bins` restored with its two history bytes cleared           f1 alone-1 level 3: 23 cases, window-gap1 first (`ranked tracks differ`)
  `std_[0] = accS` saved as `accC`                               f1 alone-1 level 5: all 41 cases"""
import numpy as np
import pytest

from tests import stream_tracker_cases as sc
from tests import test_gpu_tracker_limits as tl
from tests.test_gpu_tracker_rules import _bits
from tests.util import rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LEVELS = tl.LEVELS
ENVS = {"default": {}, "full_table": {"WSA_FULL_TABLE": "1"}}
FLAG_STREAM_CUT = 8


@pytest.fixture(scope="module")
def wsa():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import webspeechanalyzer_amd as w
    return w


def _set_env(monkeypatch, env):
    for k in tl.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _config(wsa, arr, level):
    st = arr["settings"]
    return wsa.Config(output_level=level, N_mel_bins=arr["bands"], window_step=st["window_step"], window_width=st["window_step"], pause_length=st["pause_length"],
                      min_seg_length=st["min_seg_length"], auto_noise_gate=int(st["auto_noise_gate"]), voiced_max_dB=st["voiced_max_dB"], voiced_min_dB=st["voiced_min_dB"])


def _run_streams(wsa, monkeypatch, arr, level, env):
    """-> per stream dict(callbacks, segments_ci, flags, meta) in the shape of Batch.callbacks(), the flags of every step or-ed, the cut counters at the end"""
    from tests.test_gpu_stream import _per_stream_callbacks
    from webspeechanalyzer_amd import capi
    _set_env(monkeypatch, env)
    n = len(arr["streams"])
    an = wsa.Analyzer(_config(wsa, arr, level))
    st = an.streams(n, 16000, frames_per_step=arr["F"], max_span_frames=arr["max_span"])
    rows, flags, cuts, cut_steps = [], 0, np.zeros(n, np.uint32), 0
    for nfr, ctl, frames in sc.steps(arr):
        capi.debug_stream_step_backend(st, nfr, ctl, frames, tl._stream())
        r = st.collect(tl._stream())
        rows.append(r)
        flags |= r["flags"]
        cut_steps += 1 if r["flags"] & FLAG_STREAM_CUT else 0
        cuts = r["cuts"]
    st.close(); an.close()
    _set_env(monkeypatch, {})
    cbs = _per_stream_callbacks(rows, n, level, arr["settings"]["window_step"] / 1e3)
    out = []
    for i in range(n):
        segs = [sg for r in rows for sg in r["segments"] if sg[0] == i]
        meta = [r["meta"][r["meta"][:, 0] == i] for r in rows if len(r["meta"])]
        out.append(dict(callbacks=cbs[i], segments_ci=[[int(s[1]), int(s[2])] for s in segs], flags=[int(s[3]) for s in segs],
                        meta=np.concatenate(meta, axis=0) if meta else np.zeros((0, 8), np.int32)))
    return out, flags, cuts, cut_steps


def _run_batch(wsa, monkeypatch, arr, level, env):
    _set_env(monkeypatch, env)
    an = wsa.Analyzer(_config(wsa, arr, level))
    g = an.geometry(16000)
    clips = [s["frames"] for s in arr["streams"]]
    b = an.batch([g["win"] + (len(c) - 1) * g["hop"] for c in clips], 16000)
    d = torch.from_numpy(np.concatenate(clips, axis=0).view(np.int32)).cuda()
    b.run_backend(d.data_ptr(), tl._stream())
    out = b.callbacks(tl._stream())
    b.close(); an.close()
    _set_env(monkeypatch, {})
    return out


_REF = {}


def _reference(arr):
    """per stream the oracle's runs at every level and the feature canaries; the alone-F and ragged arrangements of a family share theirs"""
    key = (arr["family"], arr["kind"])
    if key in _REF:
        return _REF[key]
    from oracle import pyoracle
    from tests.test_gpu_units import _feat_exact
    log10 = pyoracle.lib().wsa_or_log10
    runs = {level: [sc.reference(arr, i, level, gate=(level == 5)) for i in range(len(arr["streams"]))] for level in LEVELS}
    canary = {5: [], 13: []}
    for i in range(len(arr["streams"])):
        d5 = d13 = 0.0
        for s, seg in enumerate(runs[5][i]["gate"]["segments"]):
            ctx_max, fr = seg[5], runs[5][i]["formants"][s]
            if fr is None:
                continue
            d5 = max(d5, rel_err(runs[5][i]["features"][s][5:].reshape(3, 16), _feat_exact(fr, ctx_max, log10)))
            for (a, n), f in zip(runs[13][i]["syllables_ci"][s], runs[13][i]["features"][s]):
                d13 = max(d13, rel_err(f[5:].reshape(3, 16), _feat_exact(fr[a:a + n], ctx_max, log10)))
        assert d5 <= 1e-7 and d13 <= 1e-7, (key, i, d5, d13)          # the oracle's own distance is held to what test_gpu_units.py holds it to
        canary[5].append(max(1e-12, 8 * d5)); canary[13].append(max(1e-12, 8 * d13))
    load = [(max([p for p, _ in r["load"]], default=0), max([l for _, l in r["load"]], default=0)) for r in runs[5]]
    _REF[key] = dict(runs=runs, canary=canary, load=load)
    return _REF[key]


def _names(arr):
    return [s["where"][0][0] if arr["kind"] == "alone" else "%s[%d]" % (arr["name"], i) for i, s in enumerate(arr["streams"])]


def _check(arr, level, got, batches, worst):
    """one stream run against the oracle and, bit for bit, against the batch runs"""
    ref, names = _reference(arr), _names(arr)
    fails = {}
    for i, o in enumerate(got):
        one = dict(runs={level: [ref["runs"][level][i]]}, load=[ref["load"][i]], canary={k: [v[i]] for k, v in ref["canary"].items()})
        try:
            err = tl._check_against_oracle(names[i], one, level, arr["name"], dict(callbacks=[o]))[0]
            assert [f < 0 for f in o["flags"]] == [f < 0 for f in ref["runs"][level][i]["flags"]], "the segments without a result entry are not the oracle's"
            if level in worst:
                worst[level] = max(worst[level], err)
            if i in arr.get("cut_streams", ()):
                continue                                         # (a batch has no ring: the cut stream is held by the oracle with the cut alone)
            for variant, b in batches.items():
                assert _bits(o) == _bits(b[i]), f"differs from the batch run ({variant}): " + next(k for k in o if _bits(o[k]) != _bits(b[i][k]))
        except AssertionError as e:
            fails.setdefault(names[i], str(e).splitlines()[0][:200])
    assert not fails, f"{(arr['family'], arr['name'], level)}: {len(fails)} streams fail, first {next(iter(fails.items()))}; all: {sorted(fails)}"


def _can_make_streams(wsa, fam):
    """(True, None), or (False, the refusal's text) where a stream object cannot be made with the family's band count"""
    arr = sc.alone(fam, 7)
    an = wsa.Analyzer(_config(wsa, arr, 5))
    try:
        st = an.streams(1, 16000, frames_per_step=7)
    except wsa.WsaError as e:
        an.close()
        return False, str(e)
    st.close(); an.close()
    return True, None


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("fam", sc.FAMILY_NAMES)
def test_stream_steps_equal_the_batch_bit_for_bit_and_the_oracle(wsa, monkeypatch, fam, level):
    ok, why = _can_make_streams(wsa, fam)
    if not ok:                                                   # (DESIGN.md §4 records the limit)
        assert fam == "b200" and "band" in why, why
        return
    worst = {5: 0.0, 13: 0.0}
    same = None
    for arr in sc.arrangements(fam):
        batches = {v: _run_batch(wsa, monkeypatch, arr, level, env) for v, env in ENVS.items()} if arr["name"] in ("alone-1", "chained", "cut") else batches
        for variant, env in ENVS.items():
            got, flags, cuts, cut_steps = _run_streams(wsa, monkeypatch, arr, level, env)
            tag = (fam, arr["name"], level, variant)
            _check(arr, level, got, batches, worst)
            if arr["kind"] == "cut":
                want = [len(arr["streams"][i].get("cuts", ())) if i in arr["cut_streams"] else 0 for i in range(len(arr["streams"]))]
                assert sum(want) >= 1 and list(cuts) == want and cut_steps == sum(want) and flags == FLAG_STREAM_CUT, (tag, flags, list(cuts), want, cut_steps)
            else:
                assert flags == 0 and not cuts.any(), (tag, flags, list(cuts))
            if arr["kind"] == "alone":                           # every arrangement of the single clips: the same rows for a case
                bits = [_bits(o) for o in got]
                assert same is None or bits == same, (tag, "rows differ from alone-1's", [n for n, a, b in zip(_names(arr), bits, same) if a != b])
                same = bits
    print(f"stream tracker {fam:8s} level {level:2d}: worst feature rel err against the oracle, level 5 {worst[5]:.2e}, level 13 {worst[13]:.2e}")


def test_the_debug_entry_refuses_what_it_cannot_step(wsa):
    from webspeechanalyzer_amd import capi
    an = wsa.Analyzer(wsa.Config(output_level=5))
    st = an.streams(3, 16000, frames_per_step=4)
    fr, nfr, ctl = np.zeros((3, 4, 128), np.uint32), np.array([4, 4, 4], np.uint32), np.full(3, wsa.ACTIVE | wsa.START, np.uint8)
    with pytest.raises(wsa.WsaError, match=r"stream 1: 5 frames in one step, frames_per_step is 4"):
        capi.debug_stream_step_backend(st, [4, 5, 4], ctl, fr)
    with pytest.raises(wsa.WsaError, match=r"frames of 64 bands, streams 0 \.\. 2 analyse 128"):
        capi.debug_stream_step_backend(st, nfr, ctl, fr, bands=64)
    for args, what in (((None, ctl, fr), "frame counts"), ((nfr, None, fr), "control bytes"), ((nfr, ctl, None), "frames")):
        with pytest.raises(wsa.WsaError, match=rf"null {what} for streams 0 \.\. 2"):
            capi.debug_stream_step_backend(st, *args, bands=128)
    with pytest.raises(wsa.WsaError, match="no step on this stream object yet"):
        st.collect()                                             # a refused step is no step
    capi.debug_stream_step_backend(st, nfr, ctl, fr)
    assert st.collect()["flags"] == 0
    st.close()
    mixed = an.streams(2, [8000.0, 16000.0], frames_per_step=4, resample_to=16000.0)
    with pytest.raises(wsa.WsaError, match=r"mixed-rate stream set .*streams 0 \.\. 1"):
        capi.debug_stream_step_backend(mixed, [1, 1], [3, 3], np.zeros((2, mixed.frame_capacity, 128), np.uint32))
    mixed.close(); an.close()


def test_the_graphed_product_step_equals_the_debug_entry(wsa):
    """Synthetic speech through the product's wsa_stream_step (graph on, 7 frames per step) and the u32 frames of the same audio through the debug entry: the
    rows of every step bit for bit.  (Windows as long as their step: no warm-up frames, a step's frames are the batch's frames 7 k .. 7 k + 6.)"""
    from webspeechanalyzer_amd import capi
    from webspeechanalyzer_amd.synth import synth_clips
    fs, n, F = 16000, 6, 7
    for level in (5, 3):
        an = wsa.Analyzer(wsa.Config(output_level=level))
        st = an.streams(n, fs, frames_per_step=F)
        st.enable_graph(True)
        sps = st.samples_per_step
        steps = (5 * fs) // sps
        pcm = synth_clips(n, steps * sps, fs=fs, seed=61, device="cuda")
        b = an.batch([steps * sps] * n, fs)
        b.run(pcm.data_ptr(), pcm.stride(0), tl._stream())
        spec, foff = b.spectra(tl._stream())
        b.close()
        assert all(int(foff[c + 1] - foff[c]) == steps * F for c in range(n)) and spec.shape[1] == 128
        dbg = an.streams(n, fs, frames_per_step=F)
        rows = 0
        for k in range(steps):
            ctl = np.full(n, wsa.ACTIVE | (wsa.START if k == 0 else 0) | (wsa.STOP if k == steps - 1 else 0), np.uint8)
            chunk = pcm[:, k * sps:(k + 1) * sps].contiguous()
            st.step(chunk.data_ptr(), chunk.stride(0), ctl, tl._stream())
            a = st.collect(tl._stream())
            frames = np.stack([spec[int(foff[c]) + k * F:int(foff[c]) + (k + 1) * F] for c in range(n)])
            capi.debug_stream_step_backend(dbg, np.full(n, F, np.uint32), ctl, frames, tl._stream())
            d = dbg.collect(tl._stream())
            assert a.keys() == d.keys() and all(_bits(a[key]) == _bits(d[key]) for key in a if key != "tracks"), (level, k, [key for key in a if key != "tracks" and _bits(a[key]) != _bits(d[key])])
            rows += len(a["meta"]) + len(a["segments"])
        assert rows > 10
        st.close(); dbg.close(); an.close()

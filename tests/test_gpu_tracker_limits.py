"""The formant tracker (csrc/tracker.hip) at the true limits of its tiers: the crowded spans of tests/tracker_cases.py — both sides of 16 / 32 peaks
per frame, of 38 / 64 / 140 live tracks, all 63 peaks in a frame, up to 177 live tracks, amplitudes at and above 2^31, the automatic gate with its
mid-span reset — straight into the back end (wsa_batch_run_backend), every crowded clip next to a light partner clip of the same length (the span
order is sorted by length: a declined span shares its wave with one that stays).  No debug switch shrinks a table here.

Against the oracle on the same spectra, at levels 3, 10, 5 and 13 and under every tracker variant: segments, syllables, level-3 ranked tracks and
level-10 fp32 frames exact; the 53 features within the contract (1e-4 relative, floor 1e-6) and within the canary of
test_backend_matches_reference_fixtures, 1e-12 — per case the larger of that and eight times the ORACLE's own distance from the same formulas summed in
long double (tests/test_gpu_units.py _feat_exact, on the oracle's frames): never a figure of the device's.

Which tier did the work is asserted from the oracle's load counters alone (tests/test_tracker_limits_reference.py shows every case to meet its
condition): the redo count of a run (Batch.tiers(), read before the first fetch) equals the number of spans over the variant's limits, (16, 38)
for four spans per wave, (32, 64) for two, none where no paired kernel runs; the back end is rerun with the full table exactly where a span has more
than 140 live tracks and the variant's table holds 140.  Rows are bit-identical between the variants; where the full table ran (WSA_FULL_TABLE=1 or
a rerun) meta is exact and the features agree to rtol 1e-9, atol 1e-12 (another finalize path).

Measured on an MI355X, worst relative error of a feature against the oracle over all variants (canary 1e-12 unless noted; everything else is exact):
  low-live38    peaks 14  live  38   level 5 7.68e-16   level 13 7.68e-16   partner 3.36e-16
  low-live39    peaks 14  live  39   level 5 3.22e-16   level 13 3.10e-16   partner 2.72e-16
  low-peaks16   peaks 16  live  30   level 5 2.99e-16   level 13 2.17e-16   partner 2.36e-16
  low-peaks17   peaks 17  live  32   level 5 6.26e-16   level 13 6.25e-16   partner 3.56e-16
  low-live64    peaks 24  live  64   level 5 7.40e-16   level 13 5.52e-16   partner 2.98e-16
  low-live65    peaks 24  live  65   level 5 3.51e-16   level 13 3.37e-16   partner 1.59e-16
  low-peaks32   peaks 32  live  58   level 5 3.76e-16   level 13 3.75e-16   partner 3.19e-16
  low-peaks33   peaks 33  live  50   level 5 7.72e-16   level 13 3.07e-16   partner 3.76e-16
  low-live140   peaks 51  live 140   level 5 4.73e-16   level 13 4.63e-16   partner 2.59e-16
  low-peaks63   peaks 63  live  66   level 5 4.57e-16   level 13 4.57e-16   partner 2.46e-16
  low-live141   peaks 52  live 141   level 5 3.04e-16   level 13 2.89e-16   partner 4.13e-16
  low-max       peaks 63  live 176   level 5 4.55e-16   level 13 4.68e-16   partner 3.99e-16   (canary 5.7e-08: the oracle's own distance)
  high-live64   peaks 28  live  64   level 5 3.07e-16   level 13 2.97e-16   partner 3.74e-16
  high-live65   peaks 24  live  65   level 5 5.97e-16   level 13 6.12e-16   partner 3.11e-16
  high-live140  peaks 60  live 140   level 5 4.08e-16   level 13 3.27e-16   partner 2.23e-16
  high-peaks63  peaks 63  live  68   level 5 2.19e-16   level 13 5.10e-16   partner 2.46e-16
  high-live141  peaks 52  live 141   level 5 3.72e-16   level 13 5.12e-16   partner 2.44e-16
  high-max      peaks 63  live 177   level 5 4.44e-16   level 13 5.63e-16   partner 0.00e+00
  auto-live38   peaks 15  live  38   level 5 2.06e-16   level 13 4.39e-16   partner 2.07e-16
  auto-live39   peaks 16  live  39   level 5 2.52e-16   level 13 2.52e-16   partner 1.48e-16
  auto-live64   peaks 29  live  64   level 5 3.61e-15   level 13 2.34e-15   partner 8.82e-16
  auto-live65   peaks 31  live  65   level 5 1.43e-15   level 13 1.14e-15   partner 0.00e+00
Every redo count and rerun equalled the oracle's prediction: in the batch "low" 4 spans on the redo list with two spans per wave (live 65, peaks 33,
live 140, peaks 63) and 8 with four (also live 39, peaks 17, live 64, peaks 32), none for live 38 / peaks 16 (quad) and live 64 / peaks 32 (pair);
reruns 0 with 140 live tracks, 1 with 141 and with 176 / 177, 0 under WSA_FULL_TABLE=1 and at level 3.  The rows of all variants were bit-identical,
the full table's and the reruns' included (the tolerance above was not needed).  The largest table load reached is 177 of AC_MAX = 320.
Mutation check (scratch builds, not committed): QUAD_AC 37, PAIR_AC 63, `>=` in each of the three comparisons — each fails this file
(AC_FAST itself cannot move by one: its LDS layout asserts a multiple of 4)."""
import numpy as np
import pytest

from tests import tracker_cases as tc
from tests.util import callbacks_equal, rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LEVELS = (3, 10, 5, 13)
ENV_KEYS = ("WSA_QUAD", "WSA_NO_QUAD", "WSA_NO_PAIR", "WSA_NO_SPLIT", "WSA_FULL_TABLE", "WSA_DBG")
# variant -> (environment, the (peaks, live) a span may reach before the paired kernel hands it on (None: no paired kernel), table of 140 entries)
VARIANTS = {
    "default": ({}, tc.PAIR, True),                         # a small batch tracks two spans per wave
    "quad": ({"WSA_QUAD": "1"}, tc.QUAD, True),
    "no_quad": ({"WSA_NO_QUAD": "1"}, tc.PAIR, True),
    "no_pair": ({"WSA_NO_PAIR": "1"}, None, True),
    "no_split": ({"WSA_NO_SPLIT": "1"}, tc.PAIR, True),
    "full_table": ({"WSA_FULL_TABLE": "1"}, None, False),
}
# the live-140 and live-141 cases sit in batches of their own kind: each side of that edge is asserted by itself
BATCHES = {
    "low": ["low-live38", "low-live39", "low-peaks16", "low-peaks17", "low-live64", "low-live65", "low-peaks32", "low-peaks33", "low-live140", "low-peaks63"],
    "low-141": ["low-live141", "low-live39", "low-live65"],
    "low-max": ["low-max", "low-peaks17", "low-peaks33"],
    "high": ["high-live64", "high-live65", "high-live140", "high-peaks63"],
    "high-141": ["high-live141"],
    "high-max": ["high-max"],
    "auto": ["auto-live38", "auto-live39", "auto-live64", "auto-live65"],
}


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def wsa():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import webspeechanalyzer_amd as w
    return w


def _clips(name):
    """The batch's clips: every case followed by its partner."""
    out = []
    for key in BATCHES[name]:
        c = tc.CASES[key]
        out += [tc.case_clip(key), tc.partner(c["family"], c["seed"], len(c["Ks"]))]
    return out


_REF = {}


def _reference(name):
    """The oracle's runs of the batch's clips at every level, the per-clip load and feature canaries; computed once."""
    if name in _REF:
        return _REF[name]
    from oracle import pyoracle
    from tests.test_gpu_units import _feat_exact
    fam = tc.CASES[BATCHES[name][0]]["family"]
    st = tc.settings(fam)
    clips = _clips(name)
    runs = {level: [pyoracle.run_backend(sp, pyoracle.default_cfg(level=level, **st), trace=(level == 5)) for sp in clips] for level in LEVELS}
    load = [tuple(r["load"][0]) for r in runs[5]]
    assert all(len(r["segments_ci"]) == 1 for r in runs[5]) and all([tuple(r["load"][0]) for r in runs[level]] == load for level in LEVELS)
    log10 = pyoracle.lib().wsa_or_log10
    canary = {5: [], 13: []}
    for i in range(len(clips)):
        ctx_max = float(runs[5][i]["trace"][-1, 3])            # (the gate does not move it behind the segment's end)
        fr = runs[5][i]["formants"][0]
        d5 = rel_err(runs[5][i]["features"][0][5:].reshape(3, 16), _feat_exact(fr, ctx_max, log10))
        d13 = max(rel_err(f[5:].reshape(3, 16), _feat_exact(fr[a:a + n], ctx_max, log10)) for (a, n), f in zip(runs[13][i]["syllables_ci"][0], runs[13][i]["features"][0]))
        assert d5 <= 1e-7 and d13 <= 1e-7, (name, i, d5, d13)    # the oracle's own distance is held to what test_gpu_units.py holds it to
        canary[5].append(max(1e-12, 8 * d5)); canary[13].append(max(1e-12, 8 * d13))
    _REF[name] = dict(clips=clips, settings=st, runs=runs, load=load, canary=canary)
    return _REF[name]


def _run(wsa, monkeypatch, ref, level, variant):
    """One run of the batch under a variant: the tiers as the run left them, the reruns, rows (+ level 10's frames) and callbacks."""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in VARIANTS[variant][0].items():
        monkeypatch.setenv(k, v)
    st = ref["settings"]
    cfg = wsa.Config(output_level=level, N_mel_bins=tc.BANDS, window_step=st["window_step"], window_width=st["window_step"], pause_length=st["pause_length"],
                     min_seg_length=st["min_seg_length"], auto_noise_gate=int(st["auto_noise_gate"]), voiced_max_dB=st["voiced_max_dB"], voiced_min_dB=st["voiced_min_dB"])
    an = wsa.Analyzer(cfg)
    g = an.geometry(16000)
    clips = ref["clips"]
    b = an.batch([g["win"] + (len(s) - 1) * g["hop"] for s in clips], 16000)
    b.keep_counters()
    d = torch.from_numpy(np.concatenate(clips, axis=0).view(np.int32)).cuda()
    b.run_backend(d.data_ptr(), _stream())
    tiers = b.tiers(_stream())                  # before the first fetch: a fetch that finds the table overflowed reruns the back end
    out = dict(tiers=tiers, callbacks=b.callbacks(_stream()), rows=b.rows(_stream()), reruns=b.backend_reruns())
    if level == 10:
        out["rows"]["formants"] = b.formants(_stream())
    b.close(); an.close()
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    return out


def _feature_error(level, ref_cbs, got_cbs):
    if level == 5:
        return max([rel_err(o[3], r[3]) for r, o in zip(ref_cbs, got_cbs)], default=0.0)
    return max([rel_err(b, a) for r, o in zip(ref_cbs, got_cbs) for a, b in zip(r[3], o[3])], default=0.0)


def _check_against_oracle(name, ref, level, variant, got):
    """-> the feature error of every clip (0 at the levels that are compared exactly)"""
    errs = []
    for i, (r, o) in enumerate(zip(ref["runs"][level], got["callbacks"])):
        tag = (name, variant, level, i, ref["load"][i])
        assert o["segments_ci"] == r["segments_ci"], tag
        if level in (3, 10):
            ok, why = callbacks_equal(level, r["callbacks"], o["callbacks"])                 # ranked tracks / fp32 frames and syllable indices: exact
            assert ok, f"{tag}: {why}"
            errs.append(0.0)
            continue
        ok, why = callbacks_equal(level, r["callbacks"], o["callbacks"], exact=False, tol=1e-4)      # the contract (indices and times exact)
        assert ok, f"{tag}: {why}"
        err = _feature_error(level, r["callbacks"], o["callbacks"])
        errs.append(err)
        assert err <= ref["canary"][level][i], f"{tag}: canary {ref['canary'][level][i]:.3g}, rel err {err:.3g}"
    return errs


def _same_rows(a, b, exact, tag, clips):
    assert set(a) == set(b), tag
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (tag, k)
        if k == "formants":                                      # only the frames of segments are written
            foff = np.concatenate([[0], np.cumsum([len(c) for c in clips])])
            for m in a["meta"]:
                lo = int(foff[int(m[0])]) + int(m[6]); hi = lo + int(m[7])
                assert (x[lo:hi].view(np.uint32) == y[lo:hi].view(np.uint32)).all(), (tag, k)
        elif x.dtype.kind == "f" and exact:
            assert (x.view(np.uint64) == y.view(np.uint64)).all(), (tag, k)
        elif x.dtype.kind == "f":
            assert np.allclose(x, y, rtol=1e-9, atol=1e-12, equal_nan=True), (tag, k)
        else:
            assert np.array_equal(x, y), (tag, k)


@pytest.mark.parametrize("name", list(BATCHES))
def test_crowded_spans_at_the_table_limits(wsa, monkeypatch, name):
    ref = _reference(name)
    load, clips = ref["load"], ref["clips"]
    assert len(clips) <= 64 and max(len(c) for c in clips) <= 60
    top = max(live for _, live in load)
    over_140 = top > tc.AC_FAST
    # each side of the 140 edge by itself: a batch stops at exactly 140, has exactly 141, or is as crowded as the generator gets
    if name.endswith("-141"):
        assert top == tc.AC_FAST + 1
    elif name.endswith("-max"):
        assert top >= 170
    else:
        assert top == tc.AC_FAST or (name == "auto" and top == tc.PAIR[1] + 1)
    worst = {5: [0.0] * len(clips), 13: [0.0] * len(clips)}
    for level in LEVELS:
        runs = {}
        for variant, (_, limits, table_140) in VARIANTS.items():
            if level == 3 and variant != "default":
                continue                                         # level 3 has one kernel (the full table, raw tracks): the switches do not reach it
            got = runs[variant] = _run(wsa, monkeypatch, ref, level, variant)
            tag = (name, level, variant)
            want_redo = 0 if limits is None or level == 3 else sum(1 for p, l in load if p > limits[0] or l > limits[1])
            want_rerun = 1 if over_140 and table_140 and level != 3 else 0
            tiers = got["tiers"]
            print(f"tracker limits {name:9s} level {level:2d} {variant:10s} spans {tiers['spans']:3d} redo {tiers['redo']:2d} (oracle {want_redo:2d})"
                  f" reruns {got['reruns']} (oracle {want_rerun}) flags {tiers['flags']}")
            errs = _check_against_oracle(name, ref, level, variant, got)
            if level in worst:
                worst[level] = [max(a, b) for a, b in zip(worst[level], errs)]
            assert tiers["spans"] == len(load), tag
            assert tiers["redo"] == want_redo, tag
            assert tiers["flags"] == (2 if want_rerun else 0), tag
            assert got["reruns"] == want_rerun, tag
        if level == 3:
            continue
        base = runs["no_pair"]["rows"]
        assert len(base["meta"]) >= len(clips)
        for variant, got in runs.items():
            # bit for bit, except where the full table ran — on one side only, or through a rerun: another finalize path
            _same_rows(base, got["rows"], variant != "full_table" and not over_140, (name, level, variant), clips)
    for k, key in enumerate(BATCHES[name]):
        print(f"tracker limits {name:9s} {key:13s} peaks {load[2 * k][0]:2d} live {load[2 * k][1]:3d}: worst feature rel err, level 5 {worst[5][2 * k]:.2e} (canary {ref['canary'][5][2 * k]:.1e}),"
              f" level 13 {worst[13][2 * k]:.2e} (canary {ref['canary'][13][2 * k]:.1e}); partner {max(worst[5][2 * k + 1], worst[13][2 * k + 1]):.2e}")

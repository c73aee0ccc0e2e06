"""The formant tracker's accumulate and finalize rules (csrc/tracker_one.hpp, tracker_group.hpp, tracker_finalize.hpp; K2b / K3) on the hand-built clips of
tests/tracker_rule_cases.py: every comparison of the reference's accumulate_fm and finalize with a case on each side of its boundary (search windows per gap
and across the bit map's words, negative gaps, gap 0 and its infinite score, dead tracks still in the table, ties inside and across chunks of the table,
pair lists split over passes, the first-peak amplitude, the three velocity forms, the floor at equality, rank filter, slot steps, straighten's fp32
threshold, the syllable split's thresholds), straight into the back end (wsa_batch_run_backend) as tests/test_gpu_tracker_limits.py does.

One batch per settings family, in two arrangements: every case once (neighbours in the length-sorted span list are different cases sharing a wave in lock
step) and every case seven times in a row (equal lengths sit next to each other; seven consecutive entries cover every half and quarter of a wave).  Under
every tracker variant of test_gpu_tracker_limits.VARIANTS and, on the default variant, with the generic (HBM) finalize, straighten's selection loop and the
third LDS form switched off (WSA_DBG 256, 32768, 262144).  Against the oracle (pinned to the reference by tests/test_tracker_rules_reference.py): level 3
ranked tracks exact, level 10 frames and syllable indices exact, levels 5 and 13 indices exact and features within the contract (1e-4) and the canary of
test_gpu_tracker_limits.py (1e-12, or eight times the oracle's own distance from the long-double sums).  Rows bit-identical between all variants, the seven
copies of a case bit-identical to each other and to the single one; no span on the redo list, no flag, no rerun.

Measured on an MI355X, worst relative error of a feature against the oracle over all variants, both arrangements alike (canary 1e-12 everywhere: the
oracle's own distance from the long-double sums is below 1.25e-13 on these clips; everything else is exact):
  f1     41 clips  72 spans   level 5 3.78e-16   level 13 2.15e-16
  f10     1 clip    2 spans   level 5 0          level 13 0
  f100    1 clip    2 spans   level 5 0          level 13 0
  frac    1 clip    2 spans   level 5 0          level 13 0
  f1e8    1 clip    1 span    level 5 0          level 13 0
  auto    1 clip    1 span    level 5 1.23e-16   level 13 0
  b200    3 clips   6 spans   level 5 0          level 13 0
The whole file takes under four seconds (the largest test, f1 seven times: 280 clips, 28 runs of the back end, 0.7 s).

Mutation check (scratch builds of libwsa.so, nothing committed; this file run once per build, the cases named are the ones the first failing run reports):
  tracker_group.hpp  `width = bin + win - lo` -> `+ 1`                 window-gap0 .. 3, window-cut-ends, mapword-<k>-gap<g> (all 15), pairs-split (level 10)
  tracker_group.hpp  `gap >= 0 &&` dropped                             stale-index, stale-index-amp, window-gap0 (level 5; the device's score takes a gap
                                                                       of - 1 .. - 3 for 10 / 3: a dormant track joins its peak)
  atomicMin(&...asg...) -> atomicMax, both accumulate forms            every case of every family (the sentinel 0x7fffffff wins every maximum: no peak is
                                                                       ever assigned).  With the sentinel turned round too (-1: the LATER track on ties):
                                                                       tie-earlier-track, tie-across-chunk-16, tie-across-chunk-32, length-10-11, pairs-split
                                                                       (level 3); in tracker_group.hpp alone: the same without tie-across-chunk-32 (level 10)
  tracker_group.hpp  `cs > best` -> `>=` (ties across chunks; added)   tie-across-chunk-32 (level 10, default: chunks of 32 entries)
  tracker_group.hpp  `ao > pb_amp` -> `>=`                             multi-peaks (level 10); the same in tracker_one.hpp: multi-peaks (level 3)
  `(double)a0 > fl` -> `>=`, both forms                                auto-floor-in-frame (level 3); in tracker_group.hpp alone: auto-floor-in-frame (level 10)
  tracker_finalize.hpp  `mb >= 7` -> `> 7`                             rank-filter (level 3)
  tracker_finalize.hpp  `> 20` -> `>= 20`                              slots, tie-across-chunk-32, floor-10, auto-floor-in-frame (level 10)
  tracker_finalize.hpp  `floor(floor_) + 1.0` -> `floor(floor_)`       floor-10, floor-100, floor-between-bins (level 10)
Level 3 runs the one-span kernel only, so the group kernels are seen through the straightened frames alone: a case that decides which of two tracks takes a
top puts the two into different slots, or leaves the loser one point long (dropped), so that the choice shows there (tracker_rule_cases.py says how)."""
import struct

import numpy as np
import pytest

from tests import test_gpu_tracker_limits as tl
from tests import tracker_rule_cases as rc
from tests.util import rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LEVELS = tl.LEVELS
# the default variant again with one finalize form forced or switched off (csrc/wsa_internal.hpp DBG_GENERIC_FINALIZE, DBG_SELECT_LOOP, DBG_NO_THIRD_FORM)
DBG_VARIANTS = {"generic_finalize": {"WSA_DBG": "256"}, "select_loop": {"WSA_DBG": "32768"}, "no_third_form": {"WSA_DBG": "262144"}}
ENVS = dict({k: v[0] for k, v in tl.VARIANTS.items()}, **DBG_VARIANTS)
COPIES = {"once": 1, "seven": 7}


@pytest.fixture(scope="module")
def wsa():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import webspeechanalyzer_amd as w
    return w


_REF = {}


def _reference(family):
    """The oracle's runs of the family's cases at every level, per-clip load and feature canaries (the same for every copy); computed once per module."""
    if family in _REF:
        return _REF[family]
    from oracle import pyoracle
    from tests.test_gpu_units import _feat_exact
    cases = [c for c in rc.CASES if c["family"] == family]
    runs = {level: [pyoracle.run_backend(rc.spectra(c), rc.cfg(c, level), gate=(level == 5)) for c in cases] for level in LEVELS}
    log10 = pyoracle.lib().wsa_or_log10
    canary = {5: [], 13: []}
    for i, c in enumerate(cases):
        d5 = d13 = 0.0
        for s, seg in enumerate(runs[5][i]["gate"]["segments"]):
            ctx_max, fr = seg[5], runs[5][i]["formants"][s]
            d5 = max(d5, rel_err(runs[5][i]["features"][s][5:].reshape(3, 16), _feat_exact(fr, ctx_max, log10)))
            for (a, n), f in zip(runs[13][i]["syllables_ci"][s], runs[13][i]["features"][s]):
                d13 = max(d13, rel_err(f[5:].reshape(3, 16), _feat_exact(fr[a:a + n], ctx_max, log10)))
        assert d5 <= 1e-7 and d13 <= 1e-7, (c["name"], d5, d13)      # the oracle's own distance is held to what test_gpu_units.py holds it to
        canary[5].append(max(1e-12, 8 * d5)); canary[13].append(max(1e-12, 8 * d13))
    _REF[family] = dict(cases=cases, runs=runs, canary=canary, segments=[len(r["segments_ci"]) for r in runs[5]],
                        load=[(max(p for p, _ in r["load"]), max(l for _, l in r["load"])) for r in runs[5]])
    return _REF[family]


def _arranged(ref, copies):
    """the reference in the shape test_gpu_tracker_limits._check_against_oracle reads, every case `copies` times in a row"""
    rep = lambda xs: [x for x in xs for _ in range(copies)]
    return dict(clips=rep([rc.spectra(c) for c in ref["cases"]]), settings=ref["cases"][0]["settings"], bands=ref["cases"][0]["bands"],
                runs={level: rep(r) for level, r in ref["runs"].items()}, load=rep(ref["load"]), canary={k: rep(v) for k, v in ref["canary"].items()})


def _run(wsa, monkeypatch, ref, level, env):
    for k in tl.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    st = ref["settings"]
    cfg = wsa.Config(output_level=level, N_mel_bins=ref["bands"], window_step=st["window_step"], window_width=st["window_step"], pause_length=st["pause_length"],
                     min_seg_length=st["min_seg_length"], auto_noise_gate=int(st["auto_noise_gate"]), voiced_max_dB=st["voiced_max_dB"], voiced_min_dB=st["voiced_min_dB"])
    an = wsa.Analyzer(cfg)
    g = an.geometry(16000)
    clips = ref["clips"]
    b = an.batch([g["win"] + (len(s) - 1) * g["hop"] for s in clips], 16000)
    b.keep_counters()
    d = torch.from_numpy(np.concatenate(clips, axis=0).view(np.int32)).cuda()
    b.run_backend(d.data_ptr(), tl._stream())
    tiers = b.tiers(tl._stream())                 # before the first fetch
    out = dict(tiers=tiers, callbacks=b.callbacks(tl._stream()), rows=b.rows(tl._stream()), reruns=b.backend_reruns())
    if level == 10:
        out["rows"]["formants"] = b.formants(tl._stream())
    b.close(); an.close()
    for k in tl.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    return out


def _bits(x):
    """a clip's callbacks as something `==` compares bit for bit"""
    if isinstance(x, dict):                                     # (a row's meta starts with the index of its clip: left out)
        return {k: _bits(np.asarray(v)[:, 1:] if k == "meta" and len(v) else v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_bits(v) for v in x]
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, (float, np.floating)):
        return struct.pack("<d", float(x))
    return x


FAMILY_NAMES = list(rc.FAMILIES)


@pytest.mark.parametrize("copies", list(COPIES))
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_rule_cases_equal_the_oracle_under_every_variant(wsa, monkeypatch, family, copies):
    base = _reference(family)
    n = COPIES[copies]
    ref = _arranged(base, n)
    clips = ref["clips"]
    assert len(base["cases"]) >= 1 and len(clips) <= rc.MAX_CASES * 7 and max(len(c) for c in clips) <= rc.MAX_FRAMES
    spans = n * sum(base["segments"])
    worst = {5: 0.0, 13: 0.0}
    single = {}
    for level in LEVELS:
        runs = {}
        for variant, env in ENVS.items():
            if level == 3 and variant != "default":
                continue                                         # level 3 has one kernel (the full table, raw tracks): the switches do not reach it
            got = runs[variant] = _run(wsa, monkeypatch, ref, level, env)
            tag = (family, copies, level, variant)
            assert len(got["callbacks"]) == len(clips), tag
            fails = {}
            for i, o in enumerate(got["callbacks"]):             # clip by clip, so that a failure names its case (and every failing case is named)
                name = base["cases"][i // n]["name"]
                one = dict(runs={level: [ref["runs"][level][i]]}, load=[ref["load"][i]], canary={k: [v[i]] for k, v in ref["canary"].items()})
                try:
                    err = tl._check_against_oracle(name, one, level, variant, dict(callbacks=[o]))[0]
                except AssertionError as e:
                    fails.setdefault(name, str(e).splitlines()[0][:160])
                    continue
                if level in worst:
                    worst[level] = max(worst[level], err)
            assert not fails, f"{tag}: differs from the oracle in {sorted(fails)}: {fails}"
            tiers = got["tiers"]
            assert tiers["spans"] == spans and tiers["redo"] == 0 and tiers["flags"] == 0 and got["reruns"] == 0, (tag, tiers, got["reruns"])
            cbs = [_bits(o) for o in got["callbacks"]]
            for i in range(0, len(cbs), n):                      # the copies of a case: bit-identical to each other
                assert all(cbs[i + k] == cbs[i] for k in range(1, n)), (tag, base["cases"][i // n]["name"])
            single[(level, variant)] = cbs[::n]
        first = next(iter(runs))
        for variant, got in runs.items():                        # rows bit for bit between all variants
            tl._same_rows(runs[first]["rows"], got["rows"], True, (family, copies, level, variant), clips)
    _SEEN.setdefault(family, {})[copies] = single
    other = _SEEN[family].get("seven" if copies == "once" else "once")
    if other is not None:                                        # ... and between the arrangements: a case alone equals each of its seven copies
        assert other.keys() == single.keys() and all(other[k] == single[k] for k in single), (family, "arrangements differ")
    print(f"tracker rules {family:5s} {copies:5s} clips {len(clips):3d} spans {spans:3d}: worst feature rel err, level 5 {worst[5]:.2e} (canary {max(ref['canary'][5]):.1e}),"
          f" level 13 {worst[13]:.2e} (canary {max(ref['canary'][13]):.1e})")


_SEEN = {}

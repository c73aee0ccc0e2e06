"""K1b (csrc/peaks.hip) on its own (-m gpu): the hand-built frames of tests/peak_cases.py through the test entry wsa_debug_peaks (capi.debug_peaks),
modes 4, 3 and 2 — peaks_kernel<32>, peaks_kernel<16>, peaks_wave_kernel (up to 128 bands) — against the plain restatement tests/peak_ref.py, which
tests/test_peaks_reference.py pins to the oracle's scan and to the reference's own run.  Every field of a frame's record: the header's 40-bit g, n,
largest amplitude and bin, table base and spare bits; per candidate i, s, l, last, the amplitude and both 40-bit prefix sums; the slots behind the
last candidate (zero-filled, and to stay so); the flag word.  Exact integers, no tolerance.

Each group of cases (same band count) runs in three arrangements, and a frame's record must be the same bits in all of them:
  (a) the frames one after another: neighbours in a wave are unrelated (the whole group in one launch, and every case as a launch of its own);
  (b) every frame 64 times: a whole wave does the same thing, which is what fills the candidate list (dense-128: 1024 entries in a round of 32 bins);
  (c) every frame alone in a launch (63 dead lanes) and as the last frame of a launch of 65.
A frame with more than 64 candidates (dense-200) raises the flag and keeps its first 64.

Run time on an MI355X: about 3 s for the file's 32 tests (0.4 s for the 340 frames of 128 bands in mode 4, the slowest; some 2500 launches in all).

Mutation check (scratch builds of libwsa, nothing committed; only changes that cannot move an address or a loop bound; each ran once):
  changed rule (lane kernels / wave kernel)                                     first failure (mode 4, 128 bands, one after another)
  tie key `63 - ord` -> `ord` / largest by `>=`                                largest, frame 0: largest bin 71, not 31
  the `last` bit no longer kept out of the largest                             predicates-first-bins, frame 0: largest amplitude 4, not 0
  threshold `e[l] / 10` floored, not ceiled                                    shrink-threshold, frame 1 (e[l] = 1001): i = 22, not 23
  c cleared when a rise closes the falling stretch                             flat-counter-carried, frame 0: s = 10, not 7
  creep by `>=`                                                                shrink-counts, frame 12: largest amplitude 100, not 2000
  shrink by `<=` against the ceiled threshold                                  predicates-first-bins, frame 0: i = 1, not 0
  rising test by `>=`                                                          silence-and-constants, frame 0: n = 1, not 0
All seven failed as comparisons, none faulted.  (The faults that would move an address — the high byte of P[s] a bin early, g with e[0], l not forced to
B - 1, the a - 3 test dropped — are modelled on the restatement alone: tests/test_peaks_reference.py MUTANT_CASES.)
"""
import numpy as np
import pytest

from oracle import pyoracle
from tests import peak_cases as pc
from tests import peak_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CAP = 64
FIELDS = ("g", "n", "largest_amp", "largest_bin", "hdr_top", "i", "s", "l", "last", "amp", "p_i", "p_s", "ent_top")
GROUPS = pc.groups()
PARAMS = [(b, m) for b in GROUPS for m in (4, 3, 2) if m != 2 or b <= 128]


@pytest.fixture(scope="module")
def capi():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from webspeechanalyzer_amd import capi
    return capi


@pytest.fixture(scope="module")
def expected():
    """{bands: (labels, frames [N, bands], {field: array})} from the restatement (held against the oracle here once more), computed once and left alone"""
    out = {}
    for bands, items in GROUPS.items():
        N = len(items)
        E = {k: np.zeros(N, np.uint64) for k in ("g", "n", "largest_amp", "largest_bin", "hdr_top")}
        E.update({k: np.zeros((N, CAP), np.uint64) for k in ("i", "s", "l", "last", "amp", "p_i", "p_s", "ent_top")})
        over = np.zeros(N, bool)
        for f, (_, _, row) in enumerate(items):
            r = peak_ref.scan(row)
            o = pyoracle.scan_frame(row, None)
            assert (r["cands"], r["p_i"], r["p_s"], r["g"], r["largest"]) == (o["cands"], o["p_i"], o["p_s"], int(o["g"]), o["largest"])
            over[f] = len(r["cands"]) > CAP
            best = (0, 0)
            for k, (qi, qs, l, last) in enumerate(r["cands"][:CAP]):
                a = int(row[l])
                for key, v in (("i", qi), ("s", qs), ("l", l), ("last", last), ("amp", a), ("p_i", r["p_i"][k]), ("p_s", r["p_s"][k])):
                    E[key][f, k] = v
                if not last and a > best[0]:
                    best = (a, l)
            assert over[f] or best == r["largest"]
            E["g"][f], E["n"][f], E["largest_amp"][f], E["largest_bin"][f] = r["g"], min(len(r["cands"]), CAP), best[0], best[1]
        E["over"] = over
        out[bands] = ([(n, k) for n, k, _ in items], np.stack([row for _, _, row in items]), E)
    return out


def _check(rec, idx, labels, E, what):
    """the launch's records against the expected ones of the group's frames idx"""
    assert np.array_equal(rec["base"], np.arange(len(idx), dtype=np.uint32) * CAP), what
    assert rec["flags"] == (1 if E["over"][idx].any() else 0), (what, rec["flags"])
    for k in FIELDS:
        got, want = np.asarray(rec[k]).astype(np.uint64), E[k][idx]
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)[0]
            f = int(bad[0])
            slot = int(bad[1]) if len(bad) > 1 else None
            raise AssertionError(f"{what}: case {labels[idx[f]][0]} frame {labels[idx[f]][1]} (launch row {f}) field {k} slot {slot}: "
                                 f"device {int(got[tuple(bad)])} restatement {int(want[tuple(bad)])}; its n: device {int(rec['n'][f])} restatement {int(E['n'][idx[f]])}")


def _bits(rec, rows):
    return rec["hdr"][rows, :3].copy(), rec["amp"][rows].copy(), rec["ent"][rows].copy()


def _same_bits(a, b, what):
    for x, y, part in zip(a, b, ("header", "amplitudes", "entries")):
        assert np.array_equal(x, y), (what, part, np.argwhere(x != y)[0].tolist())


@pytest.mark.parametrize("bands,mode", PARAMS)
def test_peak_scan_records_of_the_hand_built_frames(capi, expected, bands, mode):
    labels, frames, E = expected[bands]
    N = len(frames)
    all_rows = np.arange(N)
    # (a) one after another
    rec = capi.debug_peaks(frames, mode)
    _check(rec, all_rows, labels, E, f"mode {mode}, {bands} bands, one after another")
    bits = _bits(rec, all_rows)
    # ... and every case as a launch of its own: its first frame is lane 0 of a wave (peak_cases.case_geometry counts on that)
    for name in dict.fromkeys(n for n, _ in labels):
        idx = np.array([f for f, (n, _) in enumerate(labels) if n == name])
        rec = capi.debug_peaks(frames[idx], mode)
        _check(rec, idx, labels, E, f"mode {mode}, {bands} bands, case {name} alone")
        _same_bits(tuple(x[idx] for x in bits), _bits(rec, np.arange(len(idx))), f"mode {mode}, {bands} bands: case {name} alone against one after another")
    # (b) every frame 64 times
    idx = np.repeat(all_rows, 64)
    rec = capi.debug_peaks(frames[idx], mode)
    _check(rec, idx, labels, E, f"mode {mode}, {bands} bands, every frame 64 times")
    for lane in (0, 31, 63):
        _same_bits(bits, _bits(rec, all_rows * 64 + lane), f"mode {mode}, {bands} bands: 64 times, lane {lane}, against one after another")
    # (c) alone, and as the last frame of 65 (behind the 64 frames that precede it in the group, cyclically)
    for f in range(N):
        one = np.array([f])
        rec = capi.debug_peaks(frames[one], mode)
        _check(rec, one, labels, E, f"mode {mode}, {bands} bands, alone")
        _same_bits(tuple(x[one] for x in bits), _bits(rec, np.array([0])), f"mode {mode}, {bands} bands: alone against one after another, {labels[f]}")
        idx = np.concatenate([(f - 64 + np.arange(64)) % N, one])
        rec = capi.debug_peaks(frames[idx], mode)
        _check(rec, idx, labels, E, f"mode {mode}, {bands} bands, last of 65")
        _same_bits(tuple(x[one] for x in bits), _bits(rec, np.array([64])), f"mode {mode}, {bands} bands: last of 65 against one after another, {labels[f]}")


def test_the_modes_are_the_three_kernels(capi):
    """the numbers this file passes as `mode` are the ones csrc/peaks.hip launch_peaks_mode reads, and the wave kernel stops at 128 bands"""
    assert (capi.PEAKS_LANES_32, capi.PEAKS_LANES_16, capi.PEAKS_WAVE) == (4, 3, 2) and capi.CAND_CAP == CAP
    assert max(b for b, m in PARAMS if m == 2) == 128 and {200, 256} <= {b for b, m in PARAMS if m == 4}

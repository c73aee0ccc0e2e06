"""The results of tests/utterance_cases.py, from the oracle alone (CPU): pyoracle.utterance_features equals, bit for bit, what the reference's own
get_utterance_features returned for every result prefix of every case (tests/golden/utterance_expected.json, tests/golden/gen/make_utterance_golden.py),
every argument of `bump` stays inside the kernel's documented domain, and the cases reach the places of csrc/utterance.hip that
tests/test_gpu_utterance.py is there for — counted here from the traced arguments (utterance_cases.bumps), so that a case edited later cannot
silently stop reaching its edge: per histogram the last bin unclamped, one past it and far past it, the low clamp's three sides, poison by NaN and
by a negative index, one / two / three trips of the syllable loop, every syllable length modulo four, results whose segments_ci entry is not their
own, rows with raw and normalised histograms side by side.  The host model of the streams' steps is checked against itself: the carry it builds
holds segments_ci entry k for result k wherever the lag is within the history's 32 entries."""
import os

import numpy as np
import pytest

from tests import utterance_cases as uc
from tests.util import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return uc.load_golden(os.path.join(GOLDEN, "utterance_expected.json"))


@pytest.fixture(scope="module")
def stats():
    return uc.path_stats()


def test_cases_are_results_as_the_dispatcher_pushes_them(golden):
    rows, digests = golden
    assert [c["name"] for c in uc.CASES] == list(rows) and 30 <= len(uc.CASES) <= 100
    fams = set()
    for c in uc.CASES:
        assert digests[c["name"]] == uc.digest(c), c["name"]                       # the fixture is of these very bytes
        assert len(rows[c["name"]]) == len(c["results"]) == sum(s[2] >= 0 for s in c["segs"]) >= 1
        assert all(s[1] >= 0 for s in c["segs"]) and c["fam"] <= set(uc.FAMILIES) and c["fam"]
        fams |= c["fam"]
        for r in c["results"]:
            fr = r["frames"]
            assert fr.dtype == np.float32 and fr.ndim == 2 and fr.shape[1] == 9
            bins = fr[:, 0::3]
            assert (bins == np.floor(bins)).all() and bins.min(initial=0) >= 0 and bins.max(initial=0) <= 255
            en = fr[:, 1::3]
            if "fractional" not in c["fam"]:
                assert (en == np.floor(en)).all() and (en >= 0).all(), c["name"]  # sums of u32 amplitudes
            if "synthetic" not in c["fam"]:
                assert np.isfinite(fr).all() and (fr >= 0).all() and all(sl >= 1 for _, sl in r["syl"]), c["name"]
            cells = set()
            for st, sl in r["syl"]:                                                # the syllables lie inside the result's frames and do not overlap
                assert 0 <= st and st + sl <= len(fr) and not (cells & set(range(st, st + sl)))
                cells |= set(range(st, st + sl))
    assert fams == set(uc.FAMILIES)


def test_oracle_equals_the_reference_bit_for_bit(golden):
    rows, _ = golden
    n = raw = 0
    for c in uc.CASES:
        got, want = uc.oracle_rows(c), rows[c["name"]]
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        assert len(bad) == 0, (c["name"], bad[:5].tolist())
        n += len(got)
        raw += int((got.max(axis=1) > 1).sum())
    print(f"\n{len(uc.CASES)} cases, {n} rows equal the reference; {raw} rows hold a raw count above 1")
    assert n >= 200 and raw >= 30


def test_every_bump_argument_is_inside_the_documented_domain():
    for c in uc.CASES:
        uc.check_domain(c)
    # the assertion bites: a mean energy one ulp above 1 gives 3 log10 of about 8e-8, where parseInt reads the exponent notation
    c = dict(name="outside", segs=[(0, 9, 0)], results=[uc.result([uc.syl(2, e1=[1.0, float(np.nextafter(np.float32(1), np.float32(2)))])])])
    with pytest.raises(AssertionError):
        uc.check_domain(c)


def test_the_cases_reach_the_paths(stats):
    for key in sorted(stats, key=str):
        print(key, stats[key])
    short = {k: (stats[k], v) for k, v in uc.MINIMUMS.items() if stats[k] < v}
    assert not short, short
    assert all(stats[("trips", n)] >= 1 for n in (0, 1, 2, 3))
    assert all(stats[("sl%4", r)] >= 20 for r in range(4))
    assert stats[("shifted",)] >= 10 and stats[("raw+normalised",)] >= 30
    # exactly one histogram raw beside fourteen normalised ones — each that can be singled out (the cases module's docstring says which cannot)
    assert all(stats[("only", k)] >= 2 for k in "dhpmls"), {k: stats[("only", k)] for k in "dhpmls"}
    # the poison of a histogram never comes from a clamped one
    assert not any(stats[(k, "negative")] for k in uc.LO_CLAMPED) and not any(stats[(k, cl)] for k in "iocgy" for cl in ("negative",))


def test_the_cases_sit_where_their_names_say():
    by = {c["name"]: c for c in uc.CASES}
    lens = lambda c: [c["results"][k]["syl"][0][1] for k in range(len(c["results"]))]
    for name in ("lengths-plain", "lengths-first-invalid", "lengths-last-invalid", "lengths-holes"):
        assert set(lens(by[name])) >= {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17} and max(lens(by[name])) >= 200, name
    first = lambda r, col: r["frames"][r["syl"][0][0], col]
    last = lambda r, col: r["frames"][r["syl"][0][0] + r["syl"][0][1] - 1, col]
    assert all(first(r, 0) == 0 == first(r, 3) for r in by["lengths-first-invalid"]["results"])
    assert all(last(r, 0) == 0 == last(r, 3) for r in by["lengths-last-invalid"]["results"])
    # a valid frame behind an invalid one, also across the four-frame trips (frame 3 invalid, frame 4 valid)
    r = by["lengths-holes"]["results"][uc.LENS.index(9)]
    s = r["frames"][r["syl"][0][0]:][:9]
    assert s[3, 0] == 0 and s[4, 0] > 0 and s[1, 3] == 0 and s[2, 3] > 0
    assert [len(r["syl"]) for r in by["counts"]["results"]] == list(uc.COUNTS) == [0, 1, 63, 64, 65, 128, 129]
    for r in by["counts"]["results"]:                                  # the later trips' syllables are longer than any of the first trip's
        sl = [n for _, n in r["syl"]]
        assert not sl[64:] or min(sl[64:]) > max(sl[:64])
    # every syllable has other valid points in front of it and behind it, or the result's edge
    for c in uc.CASES:
        for r in c["results"]:
            for st, sl in r["syl"]:
                for at in (st - 1, st + sl):
                    assert not 0 <= at < len(r["frames"]) or (r["frames"][at, 0] > 0 and r["frames"][at, 3] > 0), c["name"]
    flags = lambda name: "".join("r" if s[2] >= 0 else "d" for s in by[name]["segs"])
    assert flags("drop-first")[0] == "d" and flags("drop-last")[-1] == "d" and "rdr" in flags("drop-middle") and "dd" in flags("drop-two")
    assert by["drop-length-0"]["segs"][1][1] == 0 and by["drop-length-0"]["segs"][1][2] < 0
    assert flags("late-entry").startswith("d" * 33 + "r") and len(by["many-results"]["results"]) > uc.CARRY_HIST
    # Y()'s ingredients
    assert uc.expected_meta(by["drop-first"], 0) == (by["drop-first"]["segs"][0][0], by["drop-first"]["segs"][0][1] + by["drop-first"]["segs"][1][1])


def test_layouts_cover_the_geometries():
    lays = {l["name"]: l for l in uc.layouts()}
    batch = {n: uc.tables(l) for n, l in lays.items() if l["geometry"] == "batch"}
    assert {t["n_clips"] for t in batch.values()} >= {1, 255, 256, 257, 513}
    every = set(range(len(uc.CASES)))
    assert {ci for _, ci, _ in batch["batch-one-per-clip"]["expect"]} == every == {ci for _, ci, _ in batch["batch-interleaved"]["expect"]}
    kinds = [w for w, _ in lays["batch-interleaved"]["clips"]]
    assert None in kinds and "dropped" in kinds
    for n, t in batch.items():
        assert t["rows_cap"] > len(t["expect"])                                    # rows past the result count keep the sentinel
        if t["n_clips"] > 1:
            assert lays[n]["clips"][-1][0] not in (None, "dropped")                # the last clip (the count kernel's last range) holds a case
    # a case at different frame offsets and clip indices
    where = lambda t, ci: next((c, int(t["frame_off"][c])) for c, i, k in t["expect"] if i == ci and k == 0)
    assert sum(where(batch["batch-one-per-clip"], ci) != where(batch["batch-interleaved"], ci) for ci in every) >= len(every) - 1
    streams = {n: (l, uc.tables(l)) for n, l in lays.items() if l["geometry"] == "stream"}
    wraps = idle = lone_drop = empty_steps = restarts = 0
    for n, (l, steps) in streams.items():
        assert l["ring"] & (l["ring"] - 1) == 0
        idle += any(all(s is None for s in sc) for sc in l["streams"])
        for sc in l["streams"]:
            lone_drop += any(s and len(s[2]) == 1 and uc.CASES[s[0]]["segs"][s[2][0]][2] < 0 for s in sc)
            started = [k for k, s in enumerate(sc) if s and s[1]]
            restarts += len(started) > 1
            empty_steps += any(s is None or not s[2] for s in sc[started[0]:]) if started else 0
        for t in steps:
            m = t["row_meta"]
            wraps += int(((m[:, 6] % l["ring"]) + m[:, 7] > l["ring"]).sum())
    assert streams["stream-each"][0]["ring"] == 64 and wraps >= 20 and idle >= 3 and lone_drop >= 5 and empty_steps >= 5 and restarts >= 4
    assert all(len(s) <= 1 for sc in lays["stream-each"]["streams"] for st in sc if st for s in [st[2]])
    assert all(len(sc) - sc.count(None) == 1 for sc in lays["stream-all"]["streams"])
    lost = {n: sorted({s for t in steps for s in t["lost"]}) for n, (l, steps) in streams.items()}
    assert lost.pop("stream-lost") and not any(lost.values()), lost
    many = uc.INDEX["many-results"]
    assert any(st and st[0] == many for sc in lays["stream-gappy"]["streams"] for st in sc)       # the history index wraps without losing an entry


def test_the_step_model_against_itself():
    """for every split of every case the carry holds, behind each step, entry k = segments_ci[k] for every result k of the step whose lag is within 32
    — and says so itself (carry_entry) where it is not"""
    checked = lost = 0
    for lay in uc.layouts():
        if lay["geometry"] != "stream":
            continue
        for t in uc.tables(lay):
            for s, ci, k in t["expect"]:
                c = uc.CASES[ci]
                got = uc.carry_entry(t["carry"][s], k)
                if got is None:
                    assert s in t["lost"]
                    lost += 1
                else:
                    assert s not in t["lost"] or any(uc.carry_entry(t["carry"][s], k2) is None for s2, _, k2 in t["expect"] if s2 == s)
                    assert got == c["segs"][k][:2], (lay["name"], s, k)
                    checked += 1
            assert (t["carry"][:, 0] >= np.diff(t["clip_seg_off"].astype(np.int64))).all()
    print(f"\n{checked} history entries equal segments_ci, {lost} had left the history")
    assert checked >= 400 and lost >= 4
    for c in uc.CASES:                                                                        # the splits are partitions of the segments, in order
        for name, steps in uc.splits(c).items():
            assert [g for s in steps for g in s] == list(range(len(c["segs"]))), (c["name"], name)

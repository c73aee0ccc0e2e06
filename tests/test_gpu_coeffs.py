"""K5 (csrc/coeffs.hip) on its own: the hand-built syllables of tests/coeffs_cases.py through the test entry wsa_debug_coeffs (csrc/debug_rows.hip) — one
launch_coeffs per layout, in the batch geometry (several clips, syllables back to back inside a clip and across a clip boundary, at frame 0 and on a
clip's last frame, 1 / 15 / 16 / 17 / 33 rows and the whole table with rows_cap far above the row count) and in the streams' (ring 64, scratch stride
128: syllables that wrap the ring's end on either storage path, one that starts on the ring's last row, one of 63 frames and one that fills the ring).
The frames around the syllables hold other points, so a fit that reads a frame too many changes.

Level 12's contract is bit for bit, so nothing here has a tolerance: slots 0 .. 22 of a row equal what the REFERENCE's make_coeffs returned for the
syllable (tests/golden/coeffs_expected.json; tests/test_coeffs_reference.py shows the oracle to equal it and counts the paths the cases take: the
h / 16 retries, throws, iterations, halvings of coeffs_cases.RECORDED), slot 23 is 0 and slots 24 .. 52 are 0.  Where numeric threw, slot 23 is 1.0,
the failing fit's order + 3 slots are NaN and the other fits hold the oracle's values for those fits alone.  Rows past n_rows keep the sentinel.
A case gives the same bits wherever it sits — any layout, wave, frame offset, ring position — and a twin (frames without points appended until the
syllable takes the scratch path) gives its original's.

On an MI355X every row of every layout equalled the reference bit for bit (158 cases, 632 fits, 18 throwing rows; ten layouts, 0.17 s for their launches, the
file in 2.4 s).  Mutation check (scratch builds of coeffs.hip, arithmetic only, not committed): the retry dividing h by 8, -ffp-contract=fast,
dot_r's length-4 sum associated the other way, cost_pm's abscissa without `- first` — each fails this file, the retry's divisor in five layouts."""
import collections
import ctypes
import json
import os
import struct
import time

import numpy as np
import pytest

from tests import coeffs_cases as cc
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = -7.25e77
WSA_OK, WSA_ERR_INVALID = 0, 1
LAYOUTS = {l["name"]: l for l in cc.layouts()}


def _lib():
    from webspeechanalyzer_amd import capi
    L = capi.lib()
    return L


def _call(fr, sm, off, meta, rows_cap, ring_mask, scratch_stride, n_rows=None, fill=SENTINEL):
    """(status, out [rows_cap, 53]); out starts as `fill + 1` on the host, so an entry that returns without running leaves it."""
    fr, sm = np.ascontiguousarray(fr, np.float32), np.ascontiguousarray(sm, np.float32)
    off, meta = np.ascontiguousarray(off, np.uint32), np.ascontiguousarray(meta, np.int32)
    out = np.full((rows_cap, cc.NFEAT), fill + 1)
    rc = _lib().wsa_debug_coeffs(0, fr.ctypes.data, sm.ctypes.data, off.ctypes.data, len(off) - 1, meta.ctypes.data, len(meta) if n_rows is None else n_rows,
                                 rows_cap, ring_mask, scratch_stride, fill, out.ctypes.data)
    return rc, out


@pytest.fixture(scope="module")
def golden():
    d = json.load(open(os.path.join(GOLDEN, "coeffs_expected.json")))
    out = {}
    for g in d["cases"]:
        out[g["name"]] = None if g["row"] is None else np.array([struct.unpack(">d", bytes.fromhex(h))[0] for h in g["row"]])
        assert g["digest"] == cc.digest(cc.CASES[cc.INDEX[g["name"]]])
    assert list(out) == [c["name"] for c in cc.CASES]
    return out


@pytest.fixture(scope="module")
def thrower_fits(golden):
    """per throwing case: the four fits on their own from the oracle (short syllables, three points in the failing column: milliseconds), None = threw"""
    out = {}
    for c in cc.CASES:
        if golden[c["name"]] is None:
            fits = []
            for q in range(4):
                try:
                    fits.append(np.array(cc.polyfit(c, q)))
                except ValueError:
                    fits.append(None)
            assert sum(f is None for f in fits) == 1
            out[c["name"]] = fits
    return out


@pytest.fixture(scope="module")
def device():
    """every layout once: name -> (out, seconds)"""
    assert torch.cuda.is_available(), "needs a GPU"
    res = {}
    for name, lay in LAYOUTS.items():
        fr, sm, off, meta = cc.tables(lay)
        t0 = time.perf_counter()
        rc, out = _call(fr, sm, off, meta, lay["rows_cap"], lay["ring_mask"], lay["scratch_stride"])
        assert rc == WSA_OK, (name, rc)
        res[name] = (out, time.perf_counter() - t0)
    return res


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_rows_equal_the_reference_bit_for_bit(name, device, golden, thrower_fits):
    lay = LAYOUTS[name]
    out, secs = device[name]
    n = len(lay["rows"])
    seen = collections.Counter()
    for k, (ci, clip, st) in enumerate(lay["rows"]):
        c = cc.CASES[ci]
        row, want = out[k], golden[c["name"]]
        where = (name, k, c["name"], clip, st)
        seen["lds rows" if c["sl"] <= cc.COEF_LDS_PTS else "scratch rows"] += 1
        for f in c["fam"]:
            seen[f] += 1
        assert np.array_equal(_bits(row[24:]), _bits(np.zeros(cc.NFEAT - 24))), where
        if want is not None:
            bad = np.flatnonzero(_bits(row[:cc.NCOEF]) != _bits(want))
            assert len(bad) == 0, (where, "slots", bad.tolist(), row[bad].tolist(), want[bad].tolist())
            assert _bits(row[23:24])[0] == 0, where
        else:
            seen["throwing rows"] += 1
            assert row[23] == 1.0, where
            for q, fit in enumerate(thrower_fits[c["name"]]):
                sl_ = slice(cc.FIT_OFF[q], cc.FIT_OFF[q] + cc.FIT_ORDER[q] + 3)
                if fit is None:
                    assert np.isnan(row[sl_]).all(), (where, q, row[sl_])
                else:
                    assert np.array_equal(_bits(row[sl_]), _bits(fit)), (where, q, row[sl_].tolist(), fit.tolist())
    # rows past n_rows: untouched
    assert np.array_equal(_bits(out[n:]), _bits(np.full((lay["rows_cap"] - n, cc.NFEAT), SENTINEL))), name
    waves = [lay["rows"][w:w + 16] for w in range(0, n, 16)]
    mixed = sum(1 for w in waves if len({cc.CASES[ci]["sl"] <= cc.COEF_LDS_PTS for ci, _, _ in w}) == 2)
    print(f"\n{name}: {lay['geometry']}, {n} rows in {len(waves)} waves ({mixed} with both storage paths), rows_cap {lay['rows_cap']}, {len(lay['clips'])} clips / streams, "
          f"{secs * 1e3:.1f} ms; {dict(seen)}")


def test_a_case_gives_the_same_bits_wherever_it_sits(device, golden):
    """over all layouts: a case's rows are identical — other frame offsets, clips, waves, lanes, the ring's wrap — and a twin's equal its original's"""
    rows = collections.defaultdict(list)
    for name, lay in LAYOUTS.items():
        for k, (ci, clip, st) in enumerate(lay["rows"]):
            rows[ci].append((name, k, device[name][0][k]))
    placed_twice = in_ring = 0
    for ci, lst in rows.items():
        for name, k, r in lst[1:]:
            assert np.array_equal(_bits(r), _bits(lst[0][2])), (cc.CASES[ci]["name"], lst[0][:2], (name, k))
        placed_twice += len(lst) > 1
        in_ring += any(LAYOUTS[name]["geometry"] == "stream" for name, _, _ in lst) and len({name for name, _, _ in lst}) > 1
    twins = 0
    for ci, c in enumerate(cc.CASES):
        if c["twin_of"]:
            a, b = rows[ci][0][2], rows[cc.INDEX[c["twin_of"]]][0][2]
            assert np.array_equal(_bits(a), _bits(b)), (c["name"], a.tolist(), b.tolist())
            twins += 1
    assert len(rows) == len(cc.CASES) and placed_twice >= 20 and in_ring >= 8 and twins >= 10
    print(f"\n{placed_twice} cases sit in more than one place, {in_ring} of them also in a ring, {twins} twins across the storage paths")
    print("paths the cases take in the oracle (tests/test_coeffs_reference.py):", cc.RECORDED, "; never reached:", cc.NOT_FOUND)
    print("wall time of the launches: %.1f ms" % (1e3 * sum(s for _, s in device.values())))


def test_the_entry_refuses_what_would_leave_its_tables():
    assert torch.cuda.is_available(), "needs a GPU"
    I = cc.INDEX
    lay = dict(name="one", geometry="batch", clips=[50, 45], rows=[(I["counts-sl9-3"], 0, 41), (I["twin-counts-sl9-3"], 1, 5)], rows_cap=2,
               ring_mask=0xFFFFFFFF, scratch_stride=0)
    fr, sm, off, meta = cc.tables(lay)
    untouched = lambda out: np.array_equal(_bits(out), _bits(np.full(out.shape, SENTINEL + 1)))
    rc, out = _call(fr, sm, off, meta, 2, 0xFFFFFFFF, 0)
    assert rc == WSA_OK and not untouched(out)                               # the valid call, then one thing wrong at a time
    bad = []
    m = meta.copy(); m[0, 6] = 42; bad.append(("a syllable past its clip's last frame", (fr, sm, off, m, 2, 0xFFFFFFFF, 0)))
    m = meta.copy(); m[1, 7] = 41; bad.append(("a syllable past the last clip's last frame", (fr, sm, off, m, 2, 0xFFFFFFFF, 0)))
    m = meta.copy(); m[1, 6] = -1; bad.append(("a negative start", (fr, sm, off, m, 2, 0xFFFFFFFF, 0)))
    m = meta.copy(); m[1, 0] = 2; bad.append(("a clip that does not exist", (fr, sm, off, m, 2, 0xFFFFFFFF, 0)))
    bad.append(("rows_cap below the row count", (fr, sm, off, meta, 1, 0xFFFFFFFF, 0)))
    bad.append(("a ring in the batch geometry", (fr, sm, off, meta, 2, 31, 0)))
    slay = dict(name="s", geometry="stream", clips=[64, 64], rows=[(I["twin-counts-sl9-3"], 0, 64 * 3 + 50), (I["counts-sl9-3"], 1, 7)], rows_cap=2,
                ring_mask=63, scratch_stride=128)
    sfr, ssm, soff, smeta = cc.tables(slay)
    rc, out = _call(sfr, ssm, soff, smeta, 2, 63, 128)
    assert rc == WSA_OK and not untouched(out)
    rc, out = _call(sfr, ssm, soff, smeta, 2, 63, 103)                        # 63 + 40 rows: the smallest stride that holds the 40-frame syllable
    assert rc == WSA_OK and not untouched(out)
    bad.append(("a scratch stride one row short of ring_mask + the longest syllable", (sfr, ssm, soff, smeta, 2, 63, 102)))
    bad.append(("ring_mask + 1 = 63, no power of two", (sfr, ssm, soff, smeta, 2, 62, 128)))
    bad.append(("ring_mask + 1 = 48, no power of two", (sfr, ssm, soff, smeta, 2, 47, 128)))
    bad.append(("a ring larger than a stream's frames", (sfr, ssm, soff, smeta, 2, 127, 256)))
    m = smeta.copy(); m[0, 7] = 65; bad.append(("a syllable longer than the ring", (sfr, ssm, soff, m, 2, 63, 128)))
    for what, args in bad:
        rc, out = _call(*args)
        assert rc == WSA_ERR_INVALID and untouched(out), what
    print(f"\n{len(bad)} refusals")

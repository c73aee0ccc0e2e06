"""Hand-built tables for the device feature DB (specification FD-1; kernels K10, csrc/featdb.hip): row metadata, feature
rows whose bits are awkward on purpose (NaN payloads, -0, denormals), the slot-23 marks of level 12 and the utterance offsets of level 11.
Everything is generated here from small integers; nothing is recorded from a run."""
import numpy as np

NFEAT, NUTT, NCOEF, MARK = 53, 264, 23, 23

# ---- level 12, small: (clip, si) per row, slot 23 per row, the rows FD-1 keeps (written out by hand)
_N = float("nan")
L12_SMALL = {
    # a mark on a callback's first row drops the whole callback
    "mark_first": dict(keys=[(0, 0)] * 3 + [(0, 1)] * 2, slot=[1, 0, 0, 0, 0], kept=[3, 4]),
    # a mark on its last row drops only that row
    "mark_last": dict(keys=[(0, 0)] * 3 + [(0, 1)] * 2, slot=[0, 0, 1, 0, 0], kept=[0, 1, 3, 4]),
    # a mark in one si does not reach the next si of the same clip
    "next_si_clean": dict(keys=[(0, 0)] * 3 + [(0, 1)] * 3, slot=[0, 1, 0, 0, 0, 0], kept=[0, 3, 4, 5]),
    # the same si in two clips are two callbacks
    "same_si_two_clips": dict(keys=[(0, 2)] * 2 + [(1, 2)] * 3, slot=[1, 0, 0, 0, 1], kept=[2, 3]),
    # NaN in slot 23 counts as marked (the JS `!== 0`); -0 does not
    "nan_marks": dict(keys=[(0, 0)] * 4 + [(1, 0)] * 2, slot=[0, -0.0, _N, 0, -0.0, 0], kept=[0, 1, 4, 5]),
    "all_marked": dict(keys=[(0, 0), (0, 1), (1, 0)], slot=[1, 1, 2], kept=[]),
    "none_marked": dict(keys=[(0, 0), (0, 0), (0, 1), (1, 0)], slot=[0, 0, 0, 0], kept=[0, 1, 2, 3]),
}

# ---- level 11: utterance-row offsets per clip, the utterance rows FD-1 keeps: clips with 0, 1 and 3 rows
L11_SMALL = {
    "zero_one_three": dict(off=[0, 0, 1, 4], kept=[0, 3]),
    "three_zero_one": dict(off=[0, 3, 3, 4], kept=[2, 3]),
    "all_empty": dict(off=[0, 0, 0], kept=[]),
}


def feature_table(n, stride, seed):
    """[n][stride] f64 whose bits are a hash of (seed, row, column): ordinary numbers, and in fixed places NaNs with payloads, -0, +0,
    infinities and denormals.  Slot 23 is left to the caller at level 12."""
    r = np.arange(n, dtype=np.uint64)[:, None]
    k = np.arange(stride, dtype=np.uint64)[None, :]
    h = (r * np.uint64(0x9E3779B97F4A7C15) + k * np.uint64(0xC2B2AE3D27D4EB4F) + np.uint64((int(seed) * 0x165667B19E3779F9) & 0xFFFFFFFFFFFFFFFF))
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    x = ((h >> np.uint64(11)).astype(np.float64) / float(1 << 53) - 0.5) * 200.0
    bits = x.view(np.uint64).copy()
    special = h % np.uint64(37)
    bits[special == 0] = np.uint64(0x7FF8000000000000) | (h[special == 0] & np.uint64(0xFFFF))        # quiet NaNs with payloads
    bits[special == 1] = np.uint64(0x8000000000000000)                                                 # -0
    bits[special == 2] = np.uint64(0)                                                                  # +0
    bits[special == 3] = np.uint64(0xFFF4000000000001)                                                 # a signalling NaN, sign set
    bits[special == 4] = np.uint64(0x7FF0000000000000)                                                 # +Infinity
    bits[special == 5] = np.uint64(0x0000000000000123)                                                 # a denormal
    return bits.view(np.float64)


def meta_table(keys):
    """[n][8] i32 with (clip, si) in columns 0 and 1; the other columns are filler that must not matter"""
    n = len(keys)
    meta = np.zeros((n, 8), np.int32)
    if n:
        meta[:, 0] = [k[0] for k in keys]
        meta[:, 1] = [k[1] for k in keys]
        meta[:, 2] = np.arange(n) * 3 + 1
        meta[:, 3] = np.arange(n) % 7 + 2
        meta[:, 5] = np.arange(n) % 5
    return meta


def l12_small(name, seed=1):
    """(meta, feat [n][53]) of a small level-12 case"""
    c = L12_SMALL[name]
    feat = feature_table(len(c["keys"]), NFEAT, seed)
    feat[:, MARK] = c["slot"]
    return meta_table(c["keys"]), feat


def l12_seam_table(n, seams, seed=2):
    """A level-12 table of n rows made to cross the kernel's seams.  Callbacks are runs of 1 .. 6 rows (a fixed cycle), except that at
    every seam s in `seams` (0 < s < n) one callback is made to lie ACROSS the seam: rows s - 2 .. s + 2, marked on row s - 1 (the last
    row before the seam), so that the rows s - 1 .. s + 2 — three of them behind the seam — are dropped through the carry.  Seams lie
    at least six rows apart.  Every 11th other callback is marked on its second row.  Returns (meta, feat [n][53])."""
    keys, slot = [], np.zeros(n)
    cross = {s for s in seams if 2 <= s <= n - 3}
    r, cb = 0, 0
    while r < n:
        length = (1, 4, 2, 6, 3, 5)[cb % 6]
        for s in cross:                                  # do not run into a crossing callback's rows
            if r < s - 2 < r + length:
                length = s - 2 - r
        if r + 2 in cross:
            length = 5
            slot[r + 1] = 1.0                            # row s - 1
        elif length >= 2 and cb % 11 == 3:
            slot[r + 1] = 2.0
        length = min(length, n - r)
        keys += [(cb // 9, cb % 9)] * length
        r += length
        cb += 1
    feat = feature_table(n, NFEAT, seed)
    feat[:, MARK] = slot
    return meta_table(keys), feat


def l11_table(n_clips, seed=3):
    """(off [n_clips + 1] u32, feat [n][264]): clips with 0 .. 3 utterance rows in a fixed cycle"""
    counts = [(0, 1, 3, 2, 0, 1)[c % 6] for c in range(n_clips)]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    return off, feature_table(int(off[-1]), NUTT, seed)


# ---- the label-only selection of train.select / select_ordinal: labels, the class list, and what comes out (written out by hand)
SELECT_TOPPED = dict(
    labels=["A", "B", "C", None, "B", "C", "A", "C", "zzz", "B", "C", "A", "B", "C"], classes=["A", "B", "C"],
    rows=[0, 1, 2, 4, 5, 6, 7, 9, 10, 11, 12, 13, 1], y=[0, 1, 2, 1, 2, 0, 2, 1, 2, 0, 1, 2, 1], legend=["A", "B", "C"], counts=[3, 5, 5])
SELECT_TIED = dict(
    labels=["x", "y"] * 5 + [None], classes=["y", "x"],
    rows=list(range(10)), y=[0, 1] * 5, legend=["x", "y"], counts=[5, 5])
SELECT_ORDINAL = dict(
    values=[0.25, 0.5, 0.1, 0.3, 1.5, None, 0.6, 0.9, 0.25, 0.5, 0.2, 0.26, 0.8, 0.22, 1.0],
    rows=[0, 1, 2, 3, 6, 7, 8, 9, 10, 11, 12, 13, 14, 1], counts=[5, 5, 1, 3])

# ---- part tags and times: metadata rows {clip, si, t_start, t_len, ...} at a 12.5 ms step, what the app would store for them.
# 5 x 0.0125 = 0.0625 is exact in binary: toFixed(3) rounds the tie up to "0.063" where "%.3f" gives 0.062
RECORD_STEP = 0.0125
RECORD_META = [(0, 2, 5, 4), (0, 2, 8, 0), (1, 0, 0, 7), (1, 0, 1, 1), (1, 0, 2, 2), (1, 0, 40, 79)]
RECORD_FILES = ["a.wav", "b.wav"]
RECORDS_13 = [("a.wav", "2", ["0.063", "0.063"]), ("a.wav", "2.01", ["0.100", "0.013"]), ("b.wav", "0", ["0.000", "0.100"]),
              ("b.wav", "0.01", ["0.013", "0.025"]), ("b.wav", "0.02", ["0.025", "0.038"]), ("b.wav", "0.03", ["0.500", "1.000"])]
RECORDS_5 = [("a.wav", "2", [0.0625, 0.0625]), ("a.wav", "2", [0.1, 0.0125]), ("b.wav", "0", [0.0, 0.1]),
             ("b.wav", "0", [0.0125, 0.025]), ("b.wav", "0", [0.025, 0.037500000000000006]), ("b.wav", "0", [0.5, 1.0])]     # 3 * 0.0125 in IEEE doubles, as JS computes it

"""The hand-built cases of specification CV-1 (K6f, webspeechanalyzer_amd.crossval): members with hand-made weights at every row-block
factor, fold columns whose lists have the lengths at which a tile can go wrong, the 60-row DB of the leakage checks and the small DB
of the end-to-end run."""
import copy

import numpy as np

COUNT_ROWS = (0, 1, 15, 16, 17, 63, 64, 65)           # wsa_crossval_tiles: around a tile of 16, and of 64


def tile_rows(units):
    """tests/test_gpu_wide.py's rule (csrc/classify.hip wsa_model_create): the rows of one K6 tile, 16 rb"""
    S = ((max((u + 15) & ~15 for u in units) + 63) & ~63) + 4
    rb = 4
    while rb > 1 and 2 * 16 * rb * S * 4 > 160 * 1024:
        rb >>= 1
    return 16 * rb


def tiles(rows_per_fold, rb):
    """wsa_crossval_tiles restated: the (member, tile) pairs of one K6f launch"""
    return sum((int(n) + 16 * int(b) - 1) // (16 * int(b)) for n, b in zip(rows_per_fold, rb))


def list_lengths(tile):
    """the held-out counts of one member: no row, one, a tile less one, a tile, a tile and one, two tiles and one"""
    return [0, 1, tile - 1, tile, tile + 1, 2 * tile + 1]


def member_spec(units, salt, regression=False, labels=None):
    """Hand-made weights: every layer a seeded normal kernel scaled by 1 / sqrt(fan_in) and a small bias; relu inside, softmax (or, for
    a regression member, one sigmoid unit with its own output range) at the end.  Input ranges differ per member, so a member that read
    another member's ranges or rows would not reproduce its own K6 run."""
    from webspeechanalyzer_amd import nnmodel
    rng = np.random.default_rng(1000 + salt)
    ks = [(rng.standard_normal((a, b)) / np.sqrt(a)).astype(np.float32) for a, b in zip(units[:-1], units[1:])]
    bs = [(0.1 * rng.standard_normal(b)).astype(np.float32) for b in units[1:]]
    acts = ["relu"] * (len(units) - 2) + ["sigmoid" if regression else "softmax"]
    in_min, in_max = -0.1 * rng.random(units[0]), 1.0 + 0.2 * rng.random(units[0])
    if regression:
        return nnmodel.ModelSpec(list(units), acts, ks, bs, in_min, in_max, [], 0.5 + 0.01 * salt, 4.0 + 0.25 * salt)
    return nnmodel.ModelSpec(list(units), acts, ks, bs, in_min, in_max, list(labels) if labels is not None else [f"c{c}" for c in range(units[-1])])


def fold_column(lengths, n_blank, seed):
    """fold_of_row [sum(lengths) + n_blank] i32: fold k has lengths[k] rows, n_blank rows have no fold (-1), all interleaved by a seeded
    permutation, so every list is scattered over the DB with rows of other folds and of no fold between its rows"""
    col = np.concatenate([np.full(n, k, np.int32) for k, n in enumerate(lengths)] + [np.full(n_blank, -1, np.int32)])
    return col[np.random.default_rng(seed).permutation(len(col))]


def dense_rows(n, width, seed):
    return np.random.default_rng(seed).random((n, width))


# ---- the leakage DB: 60 rows, 6 files of 10, unbalanced classes so that select's top-up loop runs
LEAK_CLASSES = ["N", "A", "S"]
EXTREME = 1.0e6


def leak_db():
    """(db_rows, labels).  Files f0 .. f5, ten rows each; K = 3 puts files (0, 3), (1, 4), (2, 5) in folds 0, 1, 2.  Class N has 34
    rows, A 18 and S 8 — S only in files 1 and 4, so fold 1's training set has no S at all while the common legend keeps it — and A
    and S are topped up in the other folds.  Row 37 (file 3, fold 0) carries EXTREME in feature 5: it must not show in fold 0's ranges
    and must show in the others'."""
    rng = np.random.default_rng(77)
    per_file = {0: "NNNNNNAAAA", 1: "NNNNSSSSAA", 2: "NNNNNNAAAA", 3: "NNNNNNAAAA", 4: "NNNNSSSSAA", 5: "NNNNNNAANN"}
    rows, labels = [], []
    for f in range(6):
        for j, c in enumerate(per_file[f]):
            feat = rng.random(53)
            rows.append(dict(file=f"f{f}.wav", seg=str(j // 2), time=["0.000", "0.250"], features=[float(x) for x in feat],
                             true=[{"emotion": c}, {"V": float(np.round(0.05 + 0.9 * rng.random(), 3))}], pred=None))
            labels.append(c)
    rows[37]["features"][5] = EXTREME
    return rows, labels


# ---- the end-to-end DB: about 90 rows, 9 files, 3 classes, one ordinal head
E2E_CLASS_LABELS = [{"emotion": ["low", "mid", "high"]}]
E2E_ORDINALS = ["V"]


def e2e_db(seed=5):
    """90 rows in 9 files of 10 (speakers s0 .. s2, three files each), callbacks of two syllables (part tags si and si + 0.01, so that (file, part) is a key), durations in whole milliseconds; the
    class shows in the features so that two epochs already predict something; two rows without a file sit between the files."""
    rng = np.random.default_rng(seed)
    names = ["low", "mid", "high"]
    rows = []
    for f in range(9):
        if f in (3, 6):
            rows.append(dict(file=None, seg=str(f), time=["0.000", "0.100"], features=[float(x) for x in rng.random(53)],
                             true=[{"emotion": names[f % 3]}, {"V": 0.5}], pred=None))
        for j in range(10):
            c = (f + j // 4) % 3
            feat = rng.random(53) * 0.5
            feat[c * 5:c * 5 + 5] += 0.5
            v = float(np.round(np.clip(0.2 + 0.3 * c + 0.05 * rng.standard_normal(), 0.01, 1.0), 3))
            rows.append(dict(file=f"s{f % 3}_take{f // 3}.wav", seg=str(j // 2) + (".01" if j % 2 else ""), time=["0.000", f"{0.1 + 0.01 * int(rng.integers(0, 40)):.3f}"],
                             features=[float(x) for x in feat], true=[{"emotion": names[c]}, {"V": v}], pred=None))
    return rows


def clone(rows):
    return copy.deepcopy(rows)

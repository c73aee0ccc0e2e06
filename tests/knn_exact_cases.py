"""Hand-built rows for the KNN kernels (K9, K9s; csrc/knn.hip) whose similarities are EXACT (test helper): every entry of a row is 0 or
+-2^e, at exactly 1, 4, 16, 64 or 256 places.  The sum of squares is then a power of 4, sqrtf and the division are exact, a unit row holds 0
and +-2^-m, and every dot product is a sum of multiples of 2^-(m1 + m2) bounded by 1: exact in f32 in any order, fused or not, in one
accumulator or two.  So the device's similarity must equal overlap / 2^(m1 + m2) (knn_ref.exact_similarities) bit for bit, and so must ml5's.

Integer arithmetic only (np.ldexp for the powers of two), as tests/knn_cases.py.  Where a case says which tile, block, lane or arrival order
it sits on, that follows from the kernel's constants: T = QT = 64, blocks of 16 store rows, store row r in tile r // 64, block (r % 64) // 16,
column r % 16; query row q in wave (q % 64) // 16, at i = q % 4; a block's passing candidates arrive in the order i, then lane
(= 16 ((q % 16) // 4) + r % 16), so the candidates of ONE query arrive by store row ascending.  knn_ref.stream_select replays exactly that and
counts the arm; `expect` below is what each case was built to reach (checked by tests/test_knn_exact_reference.py, never read from a kernel).

The ladder: the focus query Q0 is 16-hot on features 0 .. 15; a 16-hot store row sharing j of them has similarity j / 16 (`lad(j)`), the
negated query -j / 16; a `dull` query (1-hot on feature 52, which no ladder row uses) has similarity +0 with every row, so its list is the
first k rows in rank order and every later candidate ties with its k-th.

case             what it sits on
  fmap<W>          store e_0 .. e_{W-1}, queries e_0 .. e_{W-1}, scaled by powers of two from 2^-20 to 2^20 (one row times 1 + 2^-30): with
                   k = 64 neighbour 0 of query j is row j at 1.0f, the other 63 are +0 in rank order: the k permutation 8 jj + 2 (lane >> 4)
                   + m on both operands, the pad columns, every (query lane, tile row, tile) position
  fmap<W>_s<c>     the same queries against rows 64 c .. 64 c + 63 with k = n: the full matrix is read
  mix<W>           16-hot (at 264 also 64- and 256-hot) rows spread over even and odd 8-feature steps with mixed signs: both accumulators
  ins_fill         list not yet full, the insert that fills it, a stale candidate of the same block, an insert in the middle (thr = up)
  ins_places       a full list with an insert at place 0, in the middle (thr = up), at the last place (thr = ck); equal to the k-th behind it
  keff             k_eff 1 (the __shfl index 0 arm), 2, 63, 64 on 70 rows of 17 levels, for Q0 and -Q0 side by side in one wave
  tie_kth          equal to the k-th: higher rank refused, lower rank displaces; the lower rank first, and in a later tile
  stale_lanes      two candidates of one block: the first raises the threshold, the second is refused inside knn_insert (same i, other lane)
  stale_i          the same for five queries at i = 0 .. 3 in one block
  stale_blocks     the same with the candidates in different blocks: the re-read threshold refuses in the pass test
  skip_blocks      blocks in which nothing passes; a tile where only the last block passes
  neg_t1           every similarity negative, n = T + 1, k = 64: the 63 padding rows' +0 would beat every real row of a full list (cv); the
                   store's last row is the only real row of its tile
  neg_40           the same at n = 40, k = 40: padding rows while the list fills, and after
  nan_rows         a zero row in the first tile arrives while the list fills and is pushed out later; a zero query; sim written as NaN
  nan_last_slice   a zero row alone in the last slice, with the lower rank of two NaN rows
  vote_tie         a vote tie that goes to the lower class when the top neighbour belongs to the other; a three-way tie
  class63          class 63 wins at C = 64; 64 classes inside one chunk
  c1 / k_gt_n      C = 1; k > n: -1 and NaN behind k_eff, confidences multiples of 1 / k_eff
  families         450 rows added in calls of 1, 63, 64, 65, 257; nine one-hot families, so each query lists its family in rank order
  same_rows        every row the same up to scale: every similarity 1.0f, nbr IS the grouped-rank order; a class straddling rows 63 | 64 of
                   a chunk and two add calls
  classes64        64 classes inside one chunk, one row each
  late_class       a class first seen in the last call: every rank moves
  bad_class        a class index of -1 and one of C: stored as class 0, wsa_knn_count names the row
  q63 / q64 / q65  query counts at the tile edge against a three-row store
  grid             8 n_cu 64 + 1 query rows (n_cu = 2 on the CPU, the device's on the GPU) against a three-row store, C = 1, k = 1: the last
                   row sits in the tile a workgroup takes on its second trip through `qt += gridDim.x`
"""
import numpy as np

T, QT, BLOCK = 64, 64, 16
SLICES = (1, 2, 3, 7)                      # K9s slice counts of every case with at least two store tiles; 7 leaves empty slices up to 6 tiles
#                                            (a store of 7 tiles or more also runs at tiles + 1 slices)
CASES = {}


def hot(width, places, e=0, signs=None):
    """a row of +-2^e at `places`, 0 elsewhere"""
    row = np.zeros(width)
    places = [int(p) for p in places]
    assert len(set(places)) == len(places) and len(places) in (0, 1, 4, 16, 64, 256)
    row[places] = np.ldexp(1.0, e) * (np.ones(len(places)) if signs is None else np.asarray(signs, np.float64))
    return row


def lad(j, width=53, e=0, sign=1):
    """a 16-hot row sharing the first j of Q0's features 0 .. 15; the other 16 - j lie on 16 .. 51"""
    assert 0 <= j <= 16 and 16 + (16 - j) <= min(width, 52)
    return hot(width, list(range(j)) + list(range(16, 32 - j)), e, [sign] * 16)


def q0(width=53, e=0, sign=1):
    return hot(width, range(16), e, [sign] * 16)


def dull(width=53, e=0):
    return hot(width, [52], e)


def scale_of(i):
    """a power of two between 2^-20 and 2^20"""
    return (i * 7) % 41 - 20


def _case(key, store, cls, queries, ks, C=None, adds=None, expect=(), ml5=True):
    """store [n, width], class index per row, queries, the ks to run; adds: rows per add call (None: one call); expect: the arms of
    knn_ref.KNN_ARM_NAMES the case was built to reach; ml5: whether tests/golden/knn_exact_expected.json records ml5's figures for it"""
    store, queries = np.asarray(store, np.float64), np.asarray(queries, np.float64)
    cls = np.asarray(cls, np.int64)
    n = len(store)
    tiles = (n + T - 1) // T
    slices = (SLICES + ((tiles + 1,) if tiles >= 7 else ())) if tiles >= 2 else ()
    CASES[key] = dict(key=key, width=store.shape[1], store=store, cls=cls, C=int(C if C is not None else cls.max() + 1), queries=queries,
                      ks=tuple(ks), adds=[n] if adds is None else list(adds), slices=slices, expect=tuple(expect), ml5=ml5)


def ladder(key, n, js, ks, default=0, cls=None, queries=None, **kw):
    """a store of n ladder rows, row r at level js.get(r, default), scaled by scale_of(r); queries default to (Q0, dull)"""
    store = [lad(js.get(r, default) if isinstance(js, dict) else js(r), e=scale_of(r)) for r in range(n)]
    _case(key, store, np.zeros(n, np.int64) if cls is None else cls, [q0(e=3), dull(e=-2)] if queries is None else queries, ks, **kw)


# ---- the feature map
def _fmap(width):
    store = np.stack([hot(width, [c], scale_of(c)) for c in range(width)])
    store[width // 2] *= 1.0 + 2.0 ** -30                       # rounds to the same f32
    queries = np.stack([hot(width, [c], scale_of(3 * c + 11)) for c in range(width)])
    cls = (np.arange(width) * 5) % 4
    _case(f"fmap{width}", store, cls, queries, (64, 1) if width < 64 else (64,),
          expect=("tile.partial", "qtile.partial", "tie.behind") + (("insert.full_first", "qtile.full", "tile.full") if width > 64 else ()))
    for c in range((width + 63) // 64):
        _case(f"fmap{width}_s{c}", store[64 * c:64 * c + 64], cls[64 * c:64 * c + 64], queries, (len(store[64 * c:64 * c + 64]),), C=4)


def _mix(width, stride, hots):
    """rows of h non-zeros at (p + stride t) mod width, t < h: they spread over every 8-feature step, with signs from the indices"""
    def row(p, h, e):
        return hot(width, [(p + stride * t) % width for t in range(h)], e, [1 - 2 * (((p + 1) * (t + 3) // 3) % 2) for t in range(h)])
    store = np.stack([row(3 * r, hots[r % len(hots)], scale_of(r)) for r in range(24)])
    queries = np.stack([row(2 * r + 1, hots[(r + 1) % len(hots)], scale_of(5 * r + 2)) for r in range(10)])
    _case(f"mix{width}", store, np.arange(24) % 3, queries, (24, 5), expect=("pass.above", "tie.behind"))


for _w in (53, 23, 264):
    _fmap(_w)
_mix(53, 3, (16, 16, 4))
_mix(23, 3, (16, 4, 16, 1))
_mix(264, 5, (16, 64, 256))

# ---- knn_insert
ladder("ins_fill", 6, dict(enumerate([2, 5, 3, 7, 1, 6])), (4, 6, 8),
       expect=("insert.filling", "insert.fills", "insert.refused_stale", "insert.full_middle", "thr.up", "clamp.k_above_n"))
# k = 3: rows 0 .. 2 fill [6, 5, 4]; row 16 (block 1) 9 at place 0, thr = up = 5; row 32 (block 2) 7 in the middle, thr = up = 6; row 48
# (block 3) 6 equals the k-th behind it; row 64 (tile 1) 7 at the last place behind row 32's 7, thr = ck = 7
ladder("ins_places", 70, {0: 4, 1: 5, 2: 6, 16: 9, 32: 7, 48: 6, 64: 7}, (3,), queries=[q0(e=3)],
       expect=("insert.full_first", "insert.full_middle", "insert.full_last", "insert.refused_equal", "pass.equal", "thr.ck", "thr.up", "tie.behind"))
ladder("keff", 70, lambda r: (r * 7) % 17, (1, 2, 63, 64), cls=(np.arange(70) * 3) % 5, queries=[q0(e=1), q0(e=-4, sign=-1), dull()],
       expect=("keff.1", "keff.2", "keff.63", "keff.64", "up.index_0", "up.index_k_minus_2", "insert.full_last", "kth.displaced_equal"))
# classes give rows 3 and 100 (class 1) higher ranks than rows 5, 70, 129 (class 0).  k = 2: [8 (3), 6 (5)]; row 70 (tile 1) 8 with the
# lower rank goes ahead of its equal; row 100 equals the k-th (row 3) with the higher rank: refused; row 129 (tile 2) equals the k-th
# with the lower rank: displaces it
_cls = np.zeros(130, np.int64)
_cls[[3, 100]] = 1
ladder("tie_kth", 130, {3: 8, 5: 6, 70: 8, 100: 8, 129: 8}, (1, 2, 3), cls=_cls, queries=[q0()],
       expect=("tie.ahead", "tie.behind", "insert.refused_equal", "kth.displaced_equal", "pass.equal", "merge.tie_ahead", "merge.tie_behind", "slice.short"))
ladder("stale_lanes", 20, {0: 3, 1: 9, 2: 5}, (1, 2), queries=[q0()], expect=("insert.refused_stale", "block.one_i"))
ladder("stale_i", 20, {0: 3, 1: 9, 2: 5}, (1,), queries=[q0(e=i) for i in range(4)] + [dull(), q0(sign=-1)],
       expect=("insert.refused_stale", "block.several_i"))
ladder("stale_blocks", 40, {0: 3, 17: 9, 33: 5}, (1, 2), queries=[q0()], expect=("reread.refuses",))
ladder("skip_blocks", 128, {0: 10, 127: 12}, (1,), default=2, queries=[q0()], expect=("block.skipped", "tile.only_last_block"))

# ---- cv: every similarity negative, so a padding row's +0 would beat every real row
ladder("neg_t1", T + 1, lambda r: 1 + (r * 5) % 16, (64,), cls=np.arange(T + 1) % 2, queries=[q0(sign=-1), q0(e=5, sign=-1)],
       expect=("cv.refuses_full", "tile.one_row"))
ladder("neg_40", 40, lambda r: 1 + (r * 5) % 16, (40,), cls=np.arange(40) % 2, queries=[q0(sign=-1)], expect=("cv.refuses_filling", "cv.refuses_full"))

# ---- NaN: a row of zeros has no unit row (the model only: ml5 is not pinned there)
_store = np.stack([lad((r * 7) % 17, e=scale_of(r)) for r in range(70)])
_store[[2, 69]] = 0.0
_case("nan_rows", _store, np.arange(70) % 3, [q0(), np.zeros(53), dull()], (3, 64), ml5=False,
      expect=("key.nan", "nan.pushed_out", "sim.nan", "merge.nan"))
_store = np.stack([lad((r * 7) % 17, e=scale_of(r)) for r in range(65)])
_store[[10, 64]] = 0.0
_cls = np.ones(65, np.int64)
_cls[64] = 0                                                   # the last slice's NaN row has the lower rank of the two
_case("nan_last_slice", _store, _cls, [q0(), dull()], (64,), ml5=False, expect=("merge.nan", "merge.tie_ahead", "sim.nan", "slice.short"))

# ---- the epilogue
ladder("vote_tie", 10, lambda r: {0: 12, 1: 11, 2: 10}.get(r, r % 5), (2, 3), cls=np.array([2, 1, 0, 0, 1, 2, 0, 1, 2, 0]),
       expect=("vote.tie_not_top", "vote.tie_three"))
ladder("class63", 130, lambda r: {63: 16, 127: 15}.get(r, r % 7), (1, 3), cls=np.arange(130) % 64, C=64, expect=("label.class_63",))
ladder("c1", 5, lambda r: r, (3,), C=1, expect=("classes.one",))
ladder("k_gt_n", 3, lambda r: 2 * r, (5, 64), cls=np.array([1, 0, 1]), expect=("clamp.k_above_n",))

# ---- store bookkeeping
ADDS = [1, 63, 64, 65, 257]
_n = sum(ADDS)
_case("families", [hot(53, [r % 9], scale_of(r)) for r in range(_n)], (np.arange(_n) ** 2 + np.arange(_n) // 3) % 7,
      [hot(53, [f], scale_of(f + 4)) for f in range(9)], (64,), adds=ADDS,
      expect=("within.first", "within.call_carry", "within.chunk_carry", "rank.some_moved"))
_cls = np.ones(130, np.int64)
_cls[[62, 63, 64, 65, 99, 100, 101]] = 0                       # class 0 straddles rows 63 | 64 of the first call's chunks and the two calls
_case("same_rows", [lad(16, e=scale_of(r)) for r in range(130)], _cls, [q0(e=7), q0(e=-9)], (64,), adds=[100, 30],
      expect=("within.chunk_carry", "within.call_carry", "tie.ahead"))
_case("classes64", [lad(16, e=scale_of(r)) for r in range(64)], (np.arange(64) * 37) % 64, [q0()], (64,), C=64, expect=("within.first", "vote.tie_three"))
_case("late_class", [lad(16, e=scale_of(r)) for r in range(45)], np.array([1 + r % 2 for r in range(40)] + [0] * 5), [q0()], (45,), adds=[40, 5],
      expect=("rank.all_moved",))
_cls = np.arange(12) % 3
_cls[4], _cls[9] = -1, 3
_case("bad_class", [lad(r % 5 + 10, e=scale_of(r)) for r in range(12)], _cls, [q0(), dull()], (4, 12), C=3, adds=[6, 6], ml5=False,
      expect=("add.class_below", "add.class_above"))
BAD_ROW = 4                                                    # the call-local row wsa_knn_count names: max(4, 9 - 6)

# ---- the query grid
_three = [hot(53, [0], 3), hot(53, [0, 1, 2, 3], -2), hot(53, range(16), 0)]
GRID_PERIOD = 5


def grid_queries(q):
    """q query rows cycling through five patterns (so the expectation of row i is that of pattern i mod 5)"""
    pats = np.stack([hot(53, [0], 0), hot(53, [1], 5), hot(53, [0, 1, 2, 3], -1, [1, -1, 1, 1]), hot(53, range(16), 2, [-1] * 16), hot(53, [40], 0)])
    return pats[np.arange(q) % GRID_PERIOD]


for _q in (63, 64, 65):
    _case(f"q{_q}", _three, np.array([1, 0, 1]), grid_queries(_q), (1, 3), expect=("qtile.full",) if _q >= 64 else ("qtile.partial",))
GRID_CPU_CU = 2
_case("grid", _three, np.zeros(3, np.int64), grid_queries(8 * GRID_CPU_CU * QT + 1), (1,), C=1, ml5=False, expect=("grid.second_trip", "classes.one"))
GRID = {"grid": 8 * GRID_CPU_CU}                               # workgroups of the K9 launch: min(query tiles, 8 n_cu)


def grid_case(n_cu):
    """the `grid` case at a device's CU count: (store, cls, queries)"""
    return np.stack(_three), np.zeros(3, np.int64), grid_queries(8 * n_cu * QT + 1)


# fault (knn_ref.FAULTS) -> the case named for its arm, which must notice it
FAULT_CASES = {
    "pass_gt": "tie_kth", "merge_pass_gt": "tie_kth", "rank_gt": "tie_kth", "thr_ck_always": "ins_places", "shift_le": "keff",
    "cv_dropped": "neg_t1", "nan_pos_inf": "nan_rows", "sim_nan_dropped": "nan_rows", "vote_key_lane": "vote_tie", "conf_over_k": "k_gt_n",
    "within_no_carry": "same_rows", "rank_no_soff": "families", "merge_reads_empty": "tie_kth", "no_list_reset": "grid",
}

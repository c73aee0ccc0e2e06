"""Crowded spans with a known load for the formant tracker (csrc/tracker.hip, K2b / K3) (test helper): a seeded generator of u32 spectra of
128 bands and the table of cases that sit on both sides of every table limit of the tracker's tiers.

The load of a span is what the device compares with its limits and what oracle/backend.c counts per segment (pyoracle.run_backend(...)["load"]):
  peaks   the most accepted peaks accumulate_fm got in one frame          device: `n > GW`, GW = 16 (quad) / 32 (pair) lanes per span
  live    the most tracks with frame - last_frame < 4 after a frame,     device: `g_nact + nnew > ACG`, ACG = QUAD_AC 38 / PAIR_AC 64, and
          the frame's new tracks included                                         `n_act + nnew > AC`, AC = AC_FAST 140 (one span per wave)
A span over a limit of the quad / pair tier goes on the redo list (tracker_kernel_fast takes it); over 140 live tracks the fast kernel raises flag
bit 1 and the host reruns the back end with tracker_kernel_full (AC_MAX = 320).

A clip = one start frame (six tops of 2000 at bins 21, 33 .. 81 on a ramp falling from 60 to 5, the one at bin 45 raised to 40000: the start test's
h (n - 1) / (d - h) > 4), one crowded frame per entry K of `Ks`, twelve frames of zeros (the pause that finalizes the segment).  A crowded frame
at level L: valleys linspace(0.30, 0.05, 128) L (strictly falling: the scan needs a falling edge behind every top), tops on K odd bins — always
bin 87 at 1.04 L (the frame's arg-max, below max_voiced_bin = 89), the others a random subset of the odd bins below 87 and from 91 up, strictly
rising inside each of the two runs (0.80 L .. 1.00 L and 0.80 L .. 0.97 L: the scan compares a top with the top two bins before it).  That is at
most 63 accepted peaks (K of them, or K - 1: the scan hands a top over at the next rise, so a frame's last top counts only on bin 127).  Crowded frame f has level LEVELS[f % len(LEVELS)]; the levels are more than 1000 x apart, so a peak scores 0 against the
tracks of the other levels' frames (`s < .001`) and opens a track of its own until the frame of its own level comes round: live tops out near
len(LEVELS) x K.  Three levels are what a u32 has room for.

Families:
  low    fixed gate (auto_noise_gate 0, voiced_min_dB 0: floor 1, voiced_max_dB 190), LEVELS 600, 1.0e6, 1.7e9
  high   the same gate, LEVELS 2200, 2.9e6, 4.0e9: tops up to 4.16e9, at and above 2^31 (the level-3 export stores `(int)a0`)
  auto   the app's default settings (automatic gate), LEVELS 1.0e6, 1.7e9 alternating: the second crowded frame lifts the floor to 88 400 and
         resets the tracker in mid-span (T / k < 30 v), so the span of the segment starts there, and every later frame goes through the integer gate

Every case's seed and Ks were found by search() below (seeded, CPU, oracle only: `python -m tests.tracker_cases` prints the table again) and are
hard-coded; tests/test_tracker_limits_reference.py asserts from the oracle's counters that every case still meets its condition.  The largest
live count the generator reaches is 176 / 177 (`low-max` / `high-max`), far from AC_MAX = 320: that the full table cannot overflow (<= 5 x 63) stays an
argument, unmeasured.

A partner clip (partner()) is the same start frame and frame count with K = 3 .. 5 tops per frame: a light span of the same length, which the
length-sorted span order puts into the same wave as the crowded one."""
import numpy as np

BANDS = 128
TAIL = 12
SETTINGS_FIXED = dict(window_step=25.0, pause_length=200.0, min_seg_length=50.0, auto_noise_gate=0, voiced_max_dB=190.0, voiced_min_dB=0.0)
SETTINGS_AUTO = dict(window_step=25.0, pause_length=200.0, min_seg_length=50.0, auto_noise_gate=1, voiced_max_dB=100.0, voiced_min_dB=10.0)
FAMILIES = {
    "low": dict(levels=(600.0, 1.0e6, 1.7e9), settings=SETTINGS_FIXED),
    "high": dict(levels=(2200.0, 2.9e6, 4.0e9), settings=SETTINGS_FIXED),
    "auto": dict(levels=(1.0e6, 1.7e9), settings=SETTINGS_AUTO),
}
RIDGE = 87
_RUN_A = np.arange(1, RIDGE, 2)              # 43 odd bins below the ridge
_RUN_B = np.arange(RIDGE + 4, BANDS, 2)      # 19 odd bins from 91 up (a top at 89 would have to beat the ridge two bins before it)
K_MAX = 1 + len(_RUN_A) + len(_RUN_B)        # 63

# the tiers' limits: (peaks per frame, live tracks) a span may reach without being handed on
QUAD = (16, 38)
PAIR = (32, 64)
AC_FAST = 140


def start_frame():
    e = np.linspace(60.0, 5.0, BANDS)
    e[21:82:12] = 2000.0
    e[45] = 40000.0
    return e.astype(np.uint32)


def _rising(lo, hi, n):
    """n integers rising strictly from about lo to about hi."""
    v = np.floor(np.linspace(lo, hi, n)) if n > 1 else np.array([np.floor(hi)])
    return np.maximum.accumulate(v + np.arange(n)) if n else v          # (+ index: strict also where the floor ties)


def crowded_frame(rng, K, L):
    assert 1 <= K <= K_MAX
    e = np.floor(np.linspace(0.30, 0.05, BANDS) * L)
    rest = np.sort(rng.choice(np.concatenate([_RUN_A, _RUN_B]), K - 1, replace=False))
    a, b = rest[rest < RIDGE], rest[rest > RIDGE]
    e[a] = _rising(0.80 * L, 1.00 * L, len(a)) if len(a) else 0
    e[b] = _rising(0.80 * L, 0.97 * L, len(b)) if len(b) else 0
    e[RIDGE] = np.floor(1.04 * L)
    assert e.max() < 2.0 ** 32
    return e.astype(np.uint32)


def clip(family, seed, Ks):
    """(1 + len(Ks) + TAIL, 128) uint32."""
    rng = np.random.default_rng(seed)
    levels = FAMILIES[family]["levels"]
    rows = [start_frame()] + [crowded_frame(rng, int(K), levels[f % len(levels)]) for f, K in enumerate(Ks)]
    return np.stack(rows + [np.zeros(BANDS, np.uint32)] * TAIL)


def partner(family, seed, n_crowded):
    """The light clip that shares a wave with a crowded one: the same frame count, 3 .. 5 tops per frame."""
    rng = np.random.default_rng(100000 + seed)
    return clip(family, 200000 + seed, rng.integers(3, 6, n_crowded).tolist())


def settings(family):
    return dict(FAMILIES[family]["settings"])


def load(family, spec):
    """(peaks, live) of the clip's only segment, from the oracle; None when the clip does not give exactly one segment."""
    from oracle import pyoracle
    r = pyoracle.run_backend(spec, pyoracle.default_cfg(level=5, **settings(family)))
    return tuple(r["load"][0]) if len(r["segments_ci"]) == 1 else None


# what a case must meet: name -> (condition on peaks, condition on live), each ("==", x) | ("<=", x) | (">=", x) | None
TARGETS = {
    "live38": (("<=", 16), ("==", 38)), "live39": (("<=", 16), ("==", 39)),
    "peaks16": (("==", 16), ("<=", 38)), "peaks17": (("==", 17), ("<=", 38)),
    "live64": (("<=", 32), ("==", 64)), "live65": (("<=", 32), ("==", 65)),
    "peaks32": (("==", 32), ("<=", 64)), "peaks33": (("==", 33), ("<=", 64)),
    "live140": (None, ("==", 140)), "live141": (None, ("==", 141)),
    "peaks63": (("==", 63), None), "max": (None, (">=", 170)),
}
# the automatic gate's family: both sides of 38 and of 64 (its two levels reach live 126 at most)
AUTO_TARGETS = ("live38", "live39", "live64", "live65")
HIGH_TARGETS = ("live64", "live65", "live140", "live141", "peaks63", "max")


def meets(cond, x):
    return cond is None or {"==": x == cond[1], "<=": x <= cond[1], ">=": x >= cond[1]}[cond[0]]


def _case(family, target, seed, Ks, peaks, live):
    return dict(key=f"{family}-{target}", family=family, target=target, seed=seed, Ks=Ks, peaks=peaks, live=live)


# (family, target, seed, Ks, peaks, live): peaks / live are the oracle's counters, recorded by search()
CASES = {c["key"]: c for c in (
    _case("low", "live38", 619, [13, 12, 13, 14, 13, 12, 14, 13, 13, 11, 12, 12, 13, 11, 14, 12, 12, 14, 11], 14, 38),
    _case("low", "live39", 753, [12, 12, 14, 12, 12, 12, 15, 15, 12, 15, 14, 14, 15, 12, 13, 14, 15], 14, 39),
    _case("low", "peaks16", 250, [14, 13, 6, 5, 13, 7, 7, 5, 10, 15, 14, 7, 7, 11, 8, 15, 17, 6, 12, 8, 6], 16, 30),
    _case("low", "peaks17", 54, [9, 12, 12, 7, 17, 13, 15, 7, 13, 11, 9, 14, 11, 7, 15, 18, 17, 18], 17, 32),
    _case("low", "live64", 371, [22, 24, 22, 22, 24, 21, 21, 23, 21, 22, 22, 22, 21, 24, 22, 21, 24, 22, 23, 23, 24, 24, 22, 22, 24, 23, 24, 21, 24, 24, 22, 21, 24, 21, 22, 24, 23, 21, 22], 24, 64),
    _case("low", "live65", 265, [23, 21, 24, 24, 22, 23, 22, 24, 24, 21, 23, 21, 23, 22, 24, 22, 22, 21, 21, 24, 22, 22, 24, 22, 21, 21, 24, 22, 22, 21, 23, 22], 24, 65),
    _case("low", "peaks32", 38, [18, 16, 20, 28, 22, 26, 13, 33, 14, 11, 24, 31, 27, 22, 31, 21], 32, 58),
    _case("low", "peaks33", 630, [20, 12, 21, 14, 16, 32, 12, 34, 31, 27, 28, 27, 29, 28, 24, 22, 29, 24, 24], 33, 50),
    _case("low", "live140", 203, [51, 49, 51, 48, 49, 48, 50, 49, 48, 51, 51, 50, 51, 49, 48, 50, 51, 51], 51, 140),
    _case("low", "live141", 5, [49, 52, 50, 51, 51, 50, 52, 49, 50, 50, 51, 50, 49, 49, 49, 49, 49, 52, 49, 51, 52, 49, 50, 50, 50, 52, 49, 52, 52, 52], 52, 141),
    _case("low", "peaks63", 0, [28, 21, 22, 15, 16, 14, 19, 37, 32, 40, 28, 31, 42, 35, 32, 29, 30, 63, 22, 37, 33, 14, 25, 38, 30, 14, 36, 35, 38, 19, 16, 39, 14, 29, 16, 22], 63, 66),
    _case("high", "live64", 18, [13, 24, 27, 14, 16, 10, 29, 29, 23, 20, 20, 22, 24, 21, 25, 18, 16, 11, 25, 15, 22, 24, 23, 28, 23, 27, 24, 28, 19, 9, 21, 24, 12, 23, 25, 22, 13], 28, 64),
    _case("high", "live65", 265, [23, 21, 24, 24, 22, 23, 22, 24, 24, 21, 23, 21, 23, 22, 24, 22, 22, 21, 21, 24, 22, 22, 24, 22, 21, 21, 24, 22, 22, 21, 23, 22], 24, 65),
    _case("high", "live140", 4, [56, 40, 58, 60, 59, 23, 38, 44, 31, 35, 45, 52, 43, 27, 47, 55, 29, 42, 33, 56, 22, 39, 56, 37, 25, 52, 59, 60, 58, 35, 50], 60, 140),
    _case("high", "live141", 5, [49, 52, 50, 51, 51, 50, 52, 49, 50, 50, 51, 50, 49, 49, 49, 49, 49, 52, 49, 51, 52, 49, 50, 50, 50, 52, 49, 52, 52, 52], 52, 141),
    _case("high", "peaks63", 0, [28, 21, 22, 15, 16, 14, 19, 37, 32, 40, 28, 31, 42, 35, 32, 29, 30, 63, 22, 37, 33, 14, 25, 38, 30, 14, 36, 35, 38, 19, 16, 39, 14, 29, 16, 22], 63, 68),
    _case("auto", "live38", 116, [10, 14, 7, 15, 13, 15, 7, 10, 6, 11, 8, 8, 15, 11, 15], 15, 38),
    _case("auto", "live39", 348, [12, 14, 15, 11, 9, 14, 16, 15, 7, 6, 6, 13, 16, 16, 13, 10], 16, 39),
    _case("auto", "live64", 143, [28, 29, 26, 28, 28, 28, 29, 28, 26, 29, 26, 27, 27, 26, 26, 27, 29, 26, 27, 27, 29, 29, 27, 27, 27, 28, 29, 28, 26, 29, 26, 28, 29, 27, 27, 27, 27, 27], 29, 64),
    _case("auto", "live65", 211, [28, 29, 31, 28, 30, 30, 30, 29, 29, 31, 31, 31, 31], 31, 65),
    # as crowded as the generator gets: all 63 tops in every frame (set by hand, not searched)
    _case("low", "max", 1, [63] * 12, 63, 176),
    _case("high", "max", 1, [63] * 12, 63, 177),
)}


def case_clip(key):
    c = CASES[key]
    return clip(c["family"], c["seed"], c["Ks"])


def search(seeds=4000):
    """The seeded search that found CASES: random Ks lists of 8 .. 40 frames whose K are drawn below a random cap (every other seed close to it), the first seed that meets a
    target wins.  Prints the table rows."""
    wanted = [("low", t) for t in TARGETS] + [("high", t) for t in HIGH_TARGETS] + [("auto", t) for t in AUTO_TARGETS]
    wanted = [w for w in wanted if w[1] != "max"]              # (set by hand in CASES: every frame full)
    found = {}
    for seed in range(seeds):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(8, 41))
        cap = int(rng.integers(6, K_MAX + 1))
        Ks = rng.integers(max(3, cap - 3 if seed % 2 else cap // 3), cap + 1, n).tolist()      # odd seeds: a nearly level load
        if seed % 8 == 0:
            Ks[int(rng.integers(0, n))] = K_MAX
        for fam in FAMILIES:
            if all((f, t) in found for f, t in wanted if f == fam):
                continue
            ld = load(fam, clip(fam, seed, Ks))
            if ld is None:
                continue
            for f, t in wanted:
                if f == fam and (f, t) not in found and meets(TARGETS[t][0], ld[0]) and meets(TARGETS[t][1], ld[1]):
                    found[(f, t)] = (seed, Ks, ld)
        if len(found) == len(wanted):
            break
    for f, t in wanted:
        if (f, t) in found:
            seed, Ks, ld = found[(f, t)]
            print(f'    _case("{f}", "{t}", {seed}, {Ks}, {ld[0]}, {ld[1]}),')
        else:
            print(f"    # {f}-{t}: not found in {seeds} seeds")


if __name__ == "__main__":
    search()

"""Hand-built u32 clips for the formant tracker (csrc/tracker_one.hpp, tracker_group.hpp, tracker_finalize.hpp; K2b / K3) (test helper): every case aims
one rule of the reference's accumulate_fm or finalize at its boundary and says so as oracle arm counters that must be non-zero (`expect`;
oracle/backend.c TRACK_ARMS, pyoracle.run_backend(track=True)["track"]["arms"], counted in a level-10 run).  The frames come from tests/gate_cases.py:
sparse() (tops at least 6 bins apart on the ramp 1, 2, A) and dense() (tops two bins apart over a falling baseline), each checked by its scan().

A clip is a row of segments.  A segment is a start frame (five or more tops, the ridge RIDGE_AMP so far above the others that the start test's
h (n - 1) / (d - h) > 4 holds), the frames of the case, and eight frames of zeros (the pause that finalizes it).  Every top of the start frame above the
floor opens a track under the filing index the segmenter had when the frame came (0 in a fresh clip and after a pause; the stale index otherwise), so THE
START FRAME'S TRACKS ARE THE CASE'S TRACKS: no case here uses tracker_cases.start_frame(), each names its own tops, and the ridge is either one of the
tracks the case is about or sits more than 9 + 6 bins from every bin the case offers (said in each case's comment).  Later frames are voiced when their
largest top lies on a bin in 7 .. 88 and is above twice the floor; the `keep` top that makes them so is part of the frame lists below.

A clip is BUILT AGAINST THE ORACLE (Clip pushes into a live segmenter and reads state and arm counters back), its bytes are pinned by digest() in
tests/golden/tracker_rules_expected.json next to what the REFERENCE made of them at levels 3 and 10.

Settings families (one GPU batch each, tests/test_gpu_tracker_rules.py):
  f1     fixed gate, floor 10^0 = 1 (tracker_cases.SETTINGS_FIXED): the accumulate rules
  f10    fixed gate, voiced_min_dB 20: floor 10, a bin-valued integer: straighten's `cur > floor` at cur == 10 and 11
  f100   fixed gate, voiced_min_dB 40: floor 100, the same at cur == 100 and 101
  frac   fixed gate, voiced_min_dB 28: floor 25.118..., between the bins 25 and 26
  f1e8   fixed gate, voiced_min_dB 160: floor 10^8 (>= 256: no bin is above it; and a float: a band sum of 10^8 + 1 rounds to it, `sm[1] == floor`)
  auto   the automatic gate: a frame that raises ctx_max has v (the floor its peaks were accepted against) below fl (the floor its tracks are updated against)
  b200   fixed gate, floor 1, 200 bands: tracks on bins >= 128 (one span per wave only: api.hip `bands <= 128`)"""
import ctypes
import hashlib

import numpy as np

from oracle import pyoracle
from tests import gate_cases as gc
from tests import tracker_cases as tc
from tests.gate_cases import dense, scan, sparse  # noqa: F401  (scan: every frame built here went through it inside sparse / dense)

U32 = 4294967295
RIDGE_AMP = 40000


def _fixed(db):
    return dict(tc.SETTINGS_FIXED, voiced_min_dB=float(db))


FAMILIES = {
    "f1": dict(settings=dict(tc.SETTINGS_FIXED), bands=128),
    "f10": dict(settings=_fixed(20), bands=128),
    "f100": dict(settings=_fixed(40), bands=128),
    "frac": dict(settings=_fixed(28), bands=128),
    "f1e8": dict(settings=_fixed(160), bands=128),
    "auto": dict(settings=dict(tc.SETTINGS_AUTO), bands=128),
    "b200": dict(settings=dict(tc.SETTINGS_FIXED), bands=200),
}
# the arms no case can reach, each with its reason (tests/test_tracker_rules_reference.py exempts exactly these)
UNREACHABLE = {
    "acc_no_peak": "accumulate_fm is only called from a voiced frame, and a frame without an accepted peak (n == 0) is unvoiced (ref @B26646)",
    "score_pamp_le0": "the score's `pamp <= 0` return needs tamp < pamp <= 0, but a track's amplitude is an accepted peak's: amp > v >= 0",
    "score_le1": "a score in (0, 1]: at gap 0 a non-zero score is 300 s / dist with s > .1 and dist <= 2, at least 15; at gap 1 .. 3 it is 10 / gap (t t + i s) "
                 "with t >= 1, i >= 1 and s >= 1 after its rescaling, at least 20 / 3",
    "multi_st_lowered": "`st` starts at the first assigned peak's low edge and the peaks come in bin order: a later peak's low edge starts at the bin before its "
                        "rise (ref @B25827 `i = a - 1`), which is not below the earlier peak's top, and shrinking only raises it",
}
MAX_FRAMES, MAX_CASES = 64, 80
PAUSE = 8                                  # pause_length 200 / window_step 25


class Clip:
    """frames pushed into a live oracle segmenter (level 10) as they are built; .st() / .arm() are the state and the tracker arm counters so far"""

    def __init__(self, family):
        f = FAMILIES[family]
        self.settings, self.bands = dict(f["settings"]), f["bands"]
        self.L = pyoracle.lib()
        self.cfg = pyoracle.default_cfg(level=10, bands=self.bands, **self.settings)
        self.h = self.L.wsa_or_seg_new(ctypes.byref(self.cfg))
        self.names = pyoracle.track_arm_names()
        self.frames = []

    def __del__(self):
        if getattr(self, "h", None):
            self.L.wsa_or_seg_free(self.h)
            self.h = None

    def st(self):
        o = (ctypes.c_double * 12)()
        self.L.wsa_or_gate_state(self.h, o)
        return dict(zip(("cur_frame", "no_fm", "c_ci", "c_started", "ctx_max", "floor", "last_max", "last_floor", "w", "T", "k", "span_begin"), [float(x) for x in o]))

    def arm(self, name):
        return int(self.L.wsa_or_track_arm_count(self.h, self.names.index(name)))

    def push(self, e):
        e = np.ascontiguousarray(e, np.uint32)
        assert e.shape == (self.bands,)
        self.frames.append(e)
        self.L.wsa_or_seg_push(self.h, e.ctypes.data)
        return self

    # ---- phrases
    def quiet(self, times=1):
        for _ in range(times):
            self.push(np.zeros(self.bands, np.uint32))
        return self

    def start(self, tops):
        """a frame that passes the start test and is voiced: its tops open the segment's first tracks"""
        assert self.st()["c_started"] < 0
        self.push(sparse(sorted(tops), bands=self.bands))
        assert self.st()["c_started"] == 1, ("start frame did not start", tops)
        return self

    def voiced(self, tops, frame=None):
        """a voiced frame of a running segment: accumulate_fm is called with its accepted tops"""
        before = self.arm("acc_called")
        self.push(frame if frame is not None else sparse(sorted(tops), bands=self.bands))
        assert self.arm("acc_called") == before + 1 and self.st()["c_started"] >= 1, ("frame is not voiced", tops)
        return self

    def close(self):
        """the pause: eight frames of zeros finalize a started segment (and leave c_ci at 0 for the next start frame)"""
        self.quiet(PAUSE)
        assert self.st()["c_started"] == -1 and self.st()["c_ci"] == 0
        return self

    def spectra(self):
        return np.stack(self.frames) if self.frames else np.zeros((0, self.bands), np.uint32)


CASES = []


def case(name, expect, family="f1", crowd=None):
    """crowd: None, 16 or 32 — the case is built to hold more than that many live tracks (and then at most 32 peaks and 64 live tracks)"""
    def deco(fn):
        CASES.append(dict(name=name, expect=expect, family=family, settings=dict(FAMILIES[family]["settings"]), bands=FAMILIES[family]["bands"], crowd=crowd, build=fn))
        return fn
    return deco


def _built(c):
    if "spectra" not in c:
        clip = Clip(c["family"])
        c["build"](clip)
        c["spectra"] = clip.spectra()
        assert 0 < len(c["spectra"]) <= MAX_FRAMES, (c["name"], len(c["spectra"]))
    return c["spectra"]


def spectra(c):
    return _built(c)


def digest(c):
    s = _built(c)
    return hashlib.sha256(repr((c["name"], sorted(c["settings"].items()), c["bands"], s.shape)).encode() + s.tobytes()).hexdigest()


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def cfg(c, level):
    return pyoracle.default_cfg(level=level, bands=c["bands"], **c["settings"])


A = 2000                                   # the amplitude of an ordinary track and of the peaks offered to it (s = 1)
WIN = (3, 4, 6, 9)


def _tops(bins, amp=A, ridge=None):
    return [(b, RIDGE_AMP if b == ridge else amp) for b in bins]


# ------------------------------------------------------------------------------------------------------------------ search window, gaps 1 .. 3
def _window_segment(c, gap, tracks, offers, keep, stale=0, offer_amp=A):
    """tracks (bins, `keep` among them as the ridge) open at filing index 0; frames 1 .. gap - 1 hold `keep` alone; frame `gap` offers `offers`; the frames
    after it hold `keep` alone again.  A track that takes an offered top is two points long and shows in every level's output; a track that refuses it stays
    one point long and is dropped, as is the track the refused top opens: a top taken or refused wrongly changes what every level reports (were the frame
    repeated, the straightened frames would hide a wrongly taken top: the joined track and the new one share a slot).  stale: that many idle frames of
    zeros come first, so the start frame files its tracks under the stale index `stale` while the frames after it count from 1: they meet the tracks at gap < 0
    until frame `stale`, which meets them at gap 0 (pass gap = stale)"""
    c.quiet(stale)
    c.start(_tops(tracks, ridge=keep))
    assert c.st()["c_ci"] == 1
    for _ in range(gap - 1):
        c.voiced([(keep, RIDGE_AMP)])
    c.voiced(_tops(sorted(set(offers) | {keep}), amp=offer_amp, ridge=keep))
    for _ in range(max(1, 4 - gap)):           # (five frames or more: a segment of fewer has no syllable, its level-10 callback would be empty)
        c.voiced([(keep, RIDGE_AMP)])
    c.close()


def _both_sides(b, gap):
    """the two frames that put a peak on all four window edges of a track on bin b: (b - (w - 1) in, b + w out), (b - w out, b + w - 1 in)"""
    w = WIN[gap]
    return [b - (w - 1), b + w], [b - w, b + w - 1]


def _window_case(gap, keep_at=60):
    # tracks at 20 and 100; the ridge (bin 60) is 23 or more bins from every offered bin and keeps its own track going
    def build(c):
        for k in (0, 1):
            _window_segment(c, gap, [20, 40, keep_at, 80, 100], _both_sides(20, gap)[k] + _both_sides(100, gap)[1 - k], keep_at)
    return build


for _g in (1, 2, 3):
    case("window-gap%d" % _g, {"gap%d_in" % _g: 4, "win%d_lo_in" % _g: 2, "win%d_lo_out" % _g: 2, "win%d_hi_in" % _g: 2, "win%d_hi_out" % _g: 2})(_window_case(_g))


def _mapword_case(k, gap):
    # the windows of tracks on bins 30 + k, 62 + k and 94 + k straddle the bit map's words (bits 32, 64, 96); the ridge on bin 10 keeps its own track going
    # (gap 1, window 4) and is 11 or more bins below every offered bin
    def build(c):
        tr = [10, 30 + k, 62 + k, 94 + k, 120]
        for side in (0, 1):
            offers = [o for j, b in enumerate(tr[1:4]) for o in _both_sides(b, gap)[(side + j) % 2]]
            _window_segment(c, gap, tr, offers, 10)
    return build


for _k in range(5):
    for _g in (1, 2, 3):
        case("mapword-%d-gap%d" % (_k, _g), {"gap%d_in" % _g: 6, "win%d_lo_in" % _g: 3, "win%d_lo_out" % _g: 3, "win%d_hi_in" % _g: 3, "win%d_hi_out" % _g: 3})(_mapword_case(_k, _g))


@case("window-cut-ends", dict(gap3_in=2, gap1_in=2, win3_hi_in=1, win3_lo_in=1, win3_hi_out=1, win3_lo_out=1, win1_hi_in=1, win1_lo_in=1, win1_hi_out=1, win1_lo_out=1))
def _(c):
    # tracks on bins 2 and 122 (the last bin a closed top can sit on): bin < win and bin + win > 127, the windows are cut at both ends of the spectrum.
    # The ridge (bin 60) is out of reach.  The offered tops are twice as loud as the tracks (s = .5): a track on bin 2 that wrongly took the top on 11 would
    # have a mean bin of 8 and show (with equal weights 6.5 < 7 would hide it; the top on 6 at gap 1 cannot be made to show: any mean stays below 7).
    for gap, offers in ((3, [10, 114]), (1, [6, 118]), (3, [11, 113]), (1, [5, 119])):
        _window_segment(c, gap, [2, 30, 60, 90, 122], offers, 60, offer_amp=2 * A)


@case("window-cut-eos", dict(gap2_in=2, win2_hi_in=2))
def _(c):
    # the same tracks at gap 2: 2 is offered 7, 122 the end-of-spectrum candidate on bin 127 (dist 5, inside a window that ends past the spectrum)
    _window_segment(c, 2, [2, 30, 60, 90, 122], [7, 127], 60)


# ------------------------------------------------------------------------------------------------------------------ stale filing index: gap < 0, gap 0
def _stale_two_segments(amp_parallel, amp_revive):
    """two segments of one tracker_cases.start_frame() (tops of 2000 on 21, 33, 57, 69, 81 and the ridge 40000 on 45, all part of the case: only the ridge's
    track is offered anything), N frames of one top on bin 45, twelve frames of zeros: the pause ends the segment after eight, the other four leave c_ci at 4,
    and the second start frame files its tracks under that stale index.  Its ridge track lies dormant at the indices 1 .. 3 (gap < 0) while a parallel track
    opens on bin 45; at index 4 it meets the top at gap 0, dist 0: 300 s / 0 = Infinity when s > .1, else 0"""
    def build(c):
        for n_frames in (5, 12):
            c.push(tc.start_frame())
            assert c.st()["c_started"] == 1
            for k in range(n_frames):
                c.voiced([(45, amp_revive if k == 3 else amp_parallel)])
            c.quiet(12)
        assert c.st()["c_ci"] == 4
    return build


case("stale-index", dict(gap_neg=18, gap0_in=1, score_inf=1, score_below_best=1, rank_mb_tie=1, str_ref_f_eq=1))(_stale_two_segments(40000, 40000))
# the parallel track is opened and fed by tops of 20000; the top at index 4 (3000) is below a tenth of the revived track's 40000: score 0, the parallel track keeps it
case("stale-index-amp", dict(gap_neg=18, gap0_in=1, score_zero=1))(_stale_two_segments(20000, 3000))


@case("window-gap0", dict(gap_neg=15, gap0_in=6, win0_lo_in=2, win0_lo_out=2, win0_hi_in=2, win0_hi_out=2, score_inf=2))
def _(c):
    # the tracks on 20, 40, 80, 100 and the ridge's (bin 60, kept going by a parallel track while the stale one is dormant, and offered its own bin at gap 0:
    # dist 0) are filed under the stale index 4; frame 4 offers the window edges of gap 0 (dist 2 in, dist 3 out)
    _window_segment(c, 4, [20, 40, 60, 80, 100], [18, 37, 82, 103], 60, stale=4)
    c.quiet(4)
    _window_segment(c, 4, [20, 40, 60, 80, 100], [22, 43, 78, 97], 60, stale=0)      # (the four zeros before it are the stale index)


@case("dead-gap4", dict(gap4_in=3))
def _(c):
    # tracks born on the steps 1, 2, 3 of the span (bins 20, 40, 80; bin 100 on step 1) get a top on their bin again four filing indices later (bin 100:
    # five), on the steps 5, 6, 7 = 1, 2, 3 mod 4 (bin 100: step 6): dead for the reference, still in the group kernels' table.  The start frame's tracks
    # (8, 30, 90, 116 and the ridge 60, which every frame keeps going) are 10 or more bins from those bins.
    k = (60, RIDGE_AMP)
    c.start(_tops([8, 30, 60, 90, 116], ridge=60))
    # The tops are not repeated: the tracks they open stay one point long and are dropped, a dead track that took one would be two points long and show.
    for tops in ([20, 100], [40], [80], [], [20], [40, 100], [80], []):
        c.voiced(_tops(tops) + [k])
    c.close()


# ------------------------------------------------------------------------------------------------------------------ arg-max over the tracks
@case("tie-earlier-track", dict(score_tie_kept=1, score_replaces=1, score_below_best=1, gap2_in=6))
def _(c):
    # three pairs of tracks of the start frame, 6 bins apart, equal in length, amplitude and velocity, offered one top each at gap 2 (window 6): bin 23 between
    # 20 and 26 (equal scores: the earlier track keeps it), 54 (nearer to the later track 56), 82 (nearer to the earlier track 80).  The ridge (68) is 12 bins from both neighbours.
    c.start(_tops([20, 26, 50, 56, 68, 80, 86], ridge=68))
    c.voiced([(68, RIDGE_AMP)])
    for _ in range(4):
        c.voiced(_tops([23, 54, 68, 82], ridge=68))
    c.close()


LEVELS = (600, 3200000, 3300000000)       # more than 1000 x apart: a top scores 0 (`s < .001`) against the tracks of another level and opens its own
# twelve bins each; the tying tracks are the tops 3 | 4 (60, 66) and 7 | 8 (56, 62): the third group of the ranking and the last one that gets a slot (the next
# bin is more than 20 away: the fourth group, dropped), so nothing overwrites slot 2 and which of the two took the top shows in the straightened frames
GRID_16 = [8, 30, 36, 60, 66, 87, 93, 99, 105, 111, 117, 123]
GRID_32 = [8, 14, 20, 26, 32, 38, 44, 56, 62, 90, 96, 102]


def _level_frame(level, bins, ridge=None):
    return [(b, 5 * level if b == ridge else level) for b in bins]


def _chunk_tie(levels, grid):
    """twelve tracks per level, opened frame after frame on the same bins: the table's entries 12 q .. 12 q + 11 are level q's.  The last frames offer the
    last level one top midway between two of its tracks whose entries are 15 | 16 (two levels) or 31 | 32 (three): equal scores from tracks in different
    chunks of 16 (and of 32) lanes, the earlier one keeps the top and the later one stays one point long (dropped).  The ridge (5 x 600 on the second bin, the start
    test) is a track of level 0 like the others; every frame's first top (bin 8) is its largest, so the frames are voiced."""
    def build(c):
        c.start(_level_frame(LEVELS[0], grid, ridge=grid[1]))
        for q in range(1, levels):
            c.voiced(_level_frame(LEVELS[q], grid))
        k = (15 if levels == 2 else 31) - 12 * (levels - 1)             # the tying tracks are the last level's tops k and k + 1
        assert grid[k + 1] - grid[k] == 6 and grid[k + 2] - grid[k] > 20 + 6
        bins = grid[:k] + [grid[k] + 3] + grid[k + 2:]
        for _ in range(4):                                   # (the last level's tracks are five frames long: the earlier levels' are one frame long and dropped)
            c.voiced(_level_frame(LEVELS[levels - 1], bins))
        c.close()
    return build


case("tie-across-chunk-16", dict(score_tie_kept=1, score_zero=50), crowd=16)(_chunk_tie(2, GRID_16))
case("tie-across-chunk-32", dict(score_tie_kept=1, score_zero=100), crowd=32)(_chunk_tie(3, GRID_32))


@case("pairs-split", dict(gap3_in=40))
def _(c):
    # thirteen tracks 6 bins apart (the ridge, bin 44, among them and kept going alone for two frames), then at gap 3 (window 9) sixteen tops on the odd bins
    # 9 .. 39: 4 + 7 + 8 + 8 + 8 + 5 = 40 (track, peak) pairs, more than the 32 (16) a pass of the group kernels scores; every top has pairs in two passes
    c.start(_tops([8 + 6 * k for k in range(13)], ridge=44))
    c.voiced([(44, RIDGE_AMP)]); c.voiced([(44, RIDGE_AMP)])
    fr = dense([(9 + 2 * k, A + 10 * k) for k in range(16)])
    c.voiced(None, fr); c.voiced(None, fr)
    c.close()


# ------------------------------------------------------------------------------------------------------------------ several peaks to one track
@case("multi-peaks", dict(multi_en_raised=2, multi_pb_equal_kept=1, multi_pb_moved=1))
def _(c):
    # the track on 42 gets the tops 39 and 45 (dist 3, gap 1) with equal amplitudes: its bin becomes the first one's, 39; then 36 and 42 with the later one
    # larger by one: 42.  The ridge (70) is out of reach.
    c.start(_tops([12, 42, 70, 94, 110], ridge=70))
    c.voiced([(39, A), (45, A), (70, RIDGE_AMP)])
    c.voiced([(36, A), (42, A + 1), (70, RIDGE_AMP)])
    c.voiced([(42, A), (70, RIDGE_AMP)]); c.voiced([(42, A), (70, RIDGE_AMP)])
    c.close()


@case("first-amp-stored", dict(multi_pb_moved=1, score_zero=1))
def _(c):
    # the track on 42 gets the tops 39 (amplitude 3) and 45 (4000): its bin becomes 45, its amplitude stays the FIRST one's, 3 (quirk 3).  The next frame's top on
    # 45 (4000) therefore scores 0 (s = 3 / 4000 < .001) and opens a track; with the amplitude of bin 45 stored it would have been joined.
    c.start(_tops([12, 42, 70, 94, 110], ridge=70))
    # The top is not repeated: its track stays one point long and is dropped, so frame 2 shows bin 45 only if the track on 42 joined it.
    c.voiced([(39, 3), (45, 4000), (70, RIDGE_AMP)])
    c.voiced([(45, 4000), (70, RIDGE_AMP)])
    c.voiced([(70, RIDGE_AMP)]); c.voiced([(70, RIDGE_AMP)])
    c.close()


# ------------------------------------------------------------------------------------------------------------------ velocity, length
@case("velocity-decides", dict(vel_h1=1, vel_h2=1, vel_h3=1, score_replaces=1))
def _(c):
    # the track on 9 moves + 3, + 3, + 3 to 18: the reference's velocity is (3 - 3 - 3) / 3 = - 1.  Then ONE top on 21, dist 3 from it and from the standing
    # track on 24 (part of the case, as long as the mover): t = 10 - |3 + 1| = 6 against 10 - 3 = 7, the standing track takes it.  The mover ranks into slot 0
    # (mean bin <= 20), the standing track into slot 1: who took the top shows in the straightened frames.  The ridge (60) is out of reach.
    c.start(_tops([9, 24, 60, 90, 110], ridge=60))
    for b in (12, 15, 18):
        c.voiced([(b, A), (24, A), (60, RIDGE_AMP)])
    c.voiced([(21, A), (60, RIDGE_AMP)])
    c.voiced([(21, A), (60, RIDGE_AMP)])
    c.close()


@case("velocity-third-decides", dict(vel_h3=1, score_replaces=1))
def _(c):
    # the track on 25 stands for two frames and moves to 24: x = - 1, velocity - 1 / 3.  The top on 21 is 3 bins from it and from the EARLIER standing track on 18
    # (as long, as loud): t = 10 - |- 3 + 1 / 3| = 7.33 against 7, the later track takes it — with a velocity of 0 the scores would tie and the earlier one keep
    # it.  18 ranks into slot 0, the mover into slot 1.  The ridge (60) is out of reach.
    c.start(_tops([18, 25, 60, 90, 110], ridge=60))
    for b in (25, 25, 24):
        c.voiced([(18, A), (b, A), (60, RIDGE_AMP)])
    c.voiced([(21, A), (60, RIDGE_AMP)])
    c.voiced([(21, A), (60, RIDGE_AMP)])
    c.close()


@case("velocity-thirds", dict(vel_h3=9))
def _(c):
    # the ridge's own track wanders by + 1, + 1, + 3, - 3, + 3, + 2, - 1, - 3, + 3, 0, + 1 bins: the history sums x are 1, - 7, 3, 2, - 6, - 4, 7, 0, - 2 (x / 3 by
    # two FMAs on the device).  The other tracks of the start frame (60, 80, 100, 116) are never offered anything.
    c.start(_tops([30, 60, 80, 100, 116], ridge=30))
    b = 30
    for step in (1, 1, 3, -3, 3, 2, -1, -3, 3, 0, 1):
        b += step
        c.voiced([(b, RIDGE_AMP)])
    c.close()


@case("velocity-t-negative", dict(score_zero=1, vel_h1=1, gap3_in=1))
def _(c):
    # the track on 40 moves to 43 (velocity 3) and is offered 35 at gap 3: dist 8 is inside the window, but |35 - 43 - 3| = 11 > 10 makes t < 0: score 0,
    # the top opens a track.  The ridge (70) is out of reach.
    c.start(_tops([12, 40, 70, 94, 110], ridge=70))
    c.voiced([(43, A), (70, RIDGE_AMP)])
    c.voiced([(70, RIDGE_AMP)]); c.voiced([(70, RIDGE_AMP)])
    c.voiced([(35, A), (70, RIDGE_AMP)])               # (not repeated: the track it opens is dropped, frame 4 shows bin 35 only if the mover joined it)
    c.voiced([(70, RIDGE_AMP)])
    c.close()


@case("length-10-11", dict(score_tie_kept=1, score_replaces=1))
def _(c):
    # the track on 18 (start frame) misses two frames, the one on 24 (born a frame later) none: at the decision frame they are 10 and 11 points long, `i > 10`
    # caps both: equal scores for the top on 21, the EARLIER (shorter) track keeps it.  Second segment, a frame earlier: 9 against 10, the longer one wins.
    # 18 ranks into slot 0 (mean bin <= 20), 24 into slot 1: which track took the top shows in the straightened frames.  The ridge (70) and 50 are out of reach.
    for D in (12, 11):
        c.start(_tops([18, 50, 70, 94, 110], ridge=70))
        for t in range(1, D):
            c.voiced(([] if t in (3, 6) else [(18, A)]) + [(24, A), (70, RIDGE_AMP)])
        c.voiced([(21, A), (70, RIDGE_AMP)])
        c.voiced([(21, A), (70, RIDGE_AMP)])
        c.close()


# ------------------------------------------------------------------------------------------------------------------ band sums above 2^32
def _wide(tops, bands=128):
    """tops [(bin, amplitude near 2^32)], 12 or more bins apart: seven bins wide each (steps of 1000 down on both sides), zeros between"""
    e = np.zeros(bands, np.int64)
    for b, a in tops:
        e[b - 3:b + 4] = [a - 3000, a - 2000, a - 1000, a, a - 1000, a - 2000, a - 3000]
    assert [x[0] for x in scan(e)] == [b for b, _ in tops] and e.max() <= U32
    return e.astype(np.uint32)


@case("band-sums-2-40", dict(multi_en_raised=1, gap3_in=2))
def _(c):
    # tops seven bins wide with amplitudes just below 2^32 (they score 0 against the start frame's tracks of 2000 and open their own): a band sum is 3.0e10, and
    # at gap 3 the track on 42 gets the tops on 36 and 48: its band 33 .. 51 sums to 6.0e10 (the 40-bit prefix difference).  The largest top (64) keeps the frames voiced.
    c.start(_tops([12, 42, 64, 94, 110], ridge=64))
    c.voiced(None, _wide([(20, U32 - 20), (42, U32 - 10), (64, U32)]))
    c.voiced(None, _wide([(64, U32)])); c.voiced(None, _wide([(64, U32)]))
    for _ in range(2):
        c.voiced(None, _wide([(36, U32 - 10), (48, U32 - 5), (64, U32)]))
    c.close()


# ------------------------------------------------------------------------------------------------------------------ 200 bands: bins >= 128
def _b200_case(gap):
    # tracks on 130, 160 and 190 (the one-span kernels only); the ridge (bin 100 < max_voiced_bin 140) is out of reach
    def build(c):
        for k in (0, 1):
            _window_segment(c, gap, [20, 100, 130, 160, 190], _both_sides(130, gap)[k] + _both_sides(160, gap)[1 - k] + [190 - WIN[gap] + k], 100)
    return build


for _g in (1, 2, 3):
    case("bands200-gap%d" % _g, {"gap%d_in" % _g: 5, "win%d_lo_in" % _g: 2, "win%d_lo_out" % _g: 2, "win%d_hi_in" % _g: 1, "win%d_hi_out" % _g: 1}, family="b200")(_b200_case(_g))


# ------------------------------------------------------------------------------------------------------------------ automatic gate: v < fl inside a frame
@case("auto-floor-in-frame", dict(new_equal=1, new_below=1, new_above=4, upd_equal=1, upd_below=1, upd_quirk=1, upd_above=2), family="auto")
def _(c):
    # the start frame's ridge (1000 on bin 20, part of the case: every frame keeps it going) lifts the floor from 2 to law(1000) inside the frame: its tops were accepted
    # against 2 and open tracks against the new floor f0 — above it (30, 40, 52), equal (64), below (76).  The next frame's ridge (8000) lifts it to f1: the track on
    # 30 is offered f1 itself (no update, and the top opens no track), 40 a top below it, 52 the tops 49 (below f1, the first) and 55 (above: quirk 3, still no update)
    assert c.st()["floor"] == 2
    f0 = gc._law(1000)
    c.start([(20, 1000), (30, f0 + 1), (40, f0 + 2), (52, f0 + 2), (64, f0), (76, f0 - 5)])
    assert c.st()["floor"] == f0 and c.arm("new_equal") == 1 and c.arm("new_below") == 1
    f1 = gc._law(8000)
    assert f1 - 5 > f0
    fr = [(20, 8000), (30, f1), (40, f1 - 5), (49, f1 - 5), (55, f1 + 5)]
    c.voiced(fr)
    assert c.st()["floor"] == f1 and c.st()["c_started"] == 2 and c.arm("upd_equal") == 1 and c.arm("upd_quirk") == 1
    c.voiced(fr); c.voiced(fr); c.voiced(fr)
    c.close()



# ------------------------------------------------------------------------------------------------------------------ finalize: rank filter, slots
def _held(c, bins, ridge, frames=4):
    """a segment whose tracks all stand still: the start frame and `frames` repeats of it (every track reaches count 1 + frames, its mean bin is its bin)"""
    c.start(_tops(bins, ridge=ridge))
    for _ in range(frames):
        c.voiced(_tops(bins, ridge=ridge))
    c.close()


@case("rank-filter", dict(rank_count1=2, rank_count2=2, rank_mb_lt7=1, rank_mb_eq7=1))
def _(c):
    # standing tracks on bin 6 (mean bin < 7: dropped) and on bin 7 (== 7: kept), one frame long (dropped: 110, never repeated) and two (116, kept); the ridge (60) is a track like the others
    for low in (6, 7):
        c.start(_tops([low, 30, 60, 110, 116], ridge=60))
        c.voiced(_tops([low, 30, 60, 116], ridge=60))
        for _ in range(3):
            c.voiced(_tops([low, 30, 60], ridge=60))
        c.close()


@case("slots", dict(slot_first_le20=1, slot_first_gt20=1, slot_diff_eq20=2, slot_step=4, slot_fourth=2, str_ref_l2=1, str_twice=1))
def _(c):
    # standing tracks, all of them the case (the ridge is one): 20 (slot 0: |20 - 0| is not above 20), 40 (step), 60 (|60 - 40| == 20: no step), 81 (step: slot 2), 110 (fourth group: dropped);
    # 21 (slot 0 stays empty), 41 (== 20), 62 (slot 2), 90 (dropped), 116 (dropped behind it); 15, 40, then 65 and 71 both in slot 2: `l < 2` refuses the bump, 71 overwrites 65
    _held(c, [20, 40, 60, 81, 110], 60)
    _held(c, [21, 41, 62, 90, 116], 62)
    _held(c, [15, 40, 65, 71, 110], 40)


# ------------------------------------------------------------------------------------------------------------------ straighten's `cur > floor`
def _floor_case(bins_refused, bins_bumped, ridge):
    def build(c):
        _held(c, bins_refused, ridge)
        _held(c, bins_bumped, ridge)
    return build


# floor 10: the tracks on 10 and 16 share slot 0 (both within 20 of 0): cur == 10 == floor refuses the bump, 16 overwrites 10; 11 and 17: cur == floor + 1, 17 moves up a slot
case("floor-10", dict(str_ref_floor_eq=3, str_bump_int_above=3, str_twice=3), family="f10")(_floor_case([10, 16, 60, 90, 110], [11, 17, 60, 90, 110], 60))
# floor 100: the ridge (88) opens slot 1 and is overwritten by the track on 100 (cur == 88 <= floor); 106 meets cur == 100 == floor; in the second segment 107 meets cur == 101
case("floor-100", dict(str_ref_floor_eq=3, str_ref_floor=9, str_bump_int_above=3), family="f100")(_floor_case([88, 100, 106, 112, 118], [88, 101, 107, 113, 119], 88))
# floor 25.118...: 25 and 31 share slot 1: cur == 25 == floor(floor) refuses; 26 and 32: cur == floor(floor) + 1 bumps
case("floor-between-bins", dict(str_ref_frac_below=3, str_bump_frac_above=3), family="frac")(_floor_case([25, 31, 60, 90, 110], [26, 32, 60, 90, 110], 60))


@case("floor-1e8", dict(str_ref_floor_256=4, syl_sm_eq_floor=1), family="f1e8")
def _(c):
    # floor 10^8: no bin is above it, 36 always overwrites 30.  Frame 2 holds the track on 45 alone (amplitude and band sum 10^8 + 1, which the fp32 sums array
    # rounds to 10^8 == floor: the frame counts as silent) next to a top on 80 that makes the frame voiced, opens a track and is never seen again (count 1: dropped)
    assert c.st()["floor"] == 1e8
    a, r = 100000001, 4000000000
    fr = [(30, a), (36, a), (45, a), (60, r), (90, a)]
    c.start(fr)
    c.voiced(fr)
    c.voiced([(45, a), (80, r)])
    for _ in range(4):
        c.voiced(fr)
    c.close()


# ------------------------------------------------------------------------------------------------------------------ syllable split
def _run(c, pattern):
    """a segment from a string: S the start frame (tracks 20, 40, 60 = ridge, 80, 100, all the case's), V a frame that keeps the ridge's track going (sm[1] > floor),
    q a frame of zeros inside the segment (silent), then the pause"""
    for ch in pattern:
        if ch == "S":
            c.start(_tops([20, 40, 60, 80, 100], ridge=60))
        elif ch == "V":
            c.voiced([(60, RIDGE_AMP)])
        else:
            c.quiet()
            assert c.st()["c_started"] == 2
    c.close()


@case("syllables-u-20-10", dict(syl_a_u20=1, syl_a_u21=1, syl_b_u10=1, syl_b_u11=1))
def _(c):
    _run(c, "S" + "V" * 19 + "q" + "V" + "q" + "VVV")          # u == 20 with c == 1 (open), u == 21 with c == 1 (closes)
    _run(c, "S" + "V" * 9 + "qq" + "V" + "qq" + "VVV")          # u == 10 with c == 2 (open), u == 11 with c == 2 (closes)


@case("syllables-c-4-5", dict(syl_c_c4=2, syl_c_c5=2, syl_short=1, syl_d_u5=1))
def _(c):
    _run(c, "SVV" + "qqqq" + "V" + "qqqqq" + "VVV")             # c == 4 (open), c == 5 (closes)
    _run(c, "SV" + "qqqqq" + "VVV")                             # c == 5 closes with t - i == 1: not emitted, u runs on to 5 on the last frame


@case("syllables-end", dict(syl_d_u4=1, syl_d_u5=1))
def _(c):
    _run(c, "SVVVV")                                            # five frames: u == 5 on the last one closes
    _run(c, "SVVV")                                             # four: u == 4 does not



if __name__ == "__main__":
    tot = {}
    for c in CASES:
        r = pyoracle.run_backend(spectra(c), cfg(c, 10), track=True)
        short = {k: (r["track"]["arms"][k], v) for k, v in c["expect"].items() if r["track"]["arms"][k] < v}
        print("%-24s %-5s %3d frames %2d segments load %s %s" % (c["name"], c["family"], len(spectra(c)), len(r["segments_ci"]), r["load"], ("SHORT %s" % short) if short else ""))
        for k, v in r["track"]["arms"].items():
            tot[k] = tot.get(k, 0) + v
    print("cases:", len(CASES), "frames in all:", sum(len(spectra(c)) for c in CASES))
    print("arms never taken:", [k for k, v in tot.items() if not v])

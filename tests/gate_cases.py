"""Hand-built u32 frames for the gate (csrc/gate.hip, K2a) (test helper): every case aims one rule of the frame loop's state machine at its
boundary and says so as oracle arm counters that must be non-zero (`expect`; oracle/backend.c GATE_ARMS, pyoracle.run_backend(gate=True)).

Frames.  A candidate needs a shape the peak scan accepts (ref @B25827: a rise over the three bins before it, a fall below the three bins
before that, then three flat bins or the next rise):
  sparse()  zeros, and per candidate the ramp 1, 2, A on bins b - 2 .. b — candidates at least 6 bins apart, any A >= 3.  Bins 1 .. first - 6
            hold a non-rising shelf that brings g = sum e[1 ..] to the value asked for without adding a candidate (e[0] is not part of g).
            A candidate on the last bin is the end-of-spectrum emission, which the reference leaves out of h / p.
  dense()   a baseline falling by one per bin, tops on every second bin, rising inside a run of neighbours: up to 64 candidates at 128 bands.
Every frame built is run through scan() below, a restatement of the scan's geometry, and must give exactly the candidates asked for.

The floor moves under the frames, so a clip is BUILT AGAINST THE ORACLE: Clip pushes each frame into a live oracle segmenter and reads the
state back (ctx_max, floor, last_max, w, T, k) to place the next frame's amplitudes on the boundary it is after.  The bytes that come out are
fixed (digest(), pinned in tests/golden/gate_expected.json next to what the REFERENCE made of them), so the oracle cannot move a case without
the golden test noticing.

Left out: the `k >= 2^20` arm of the integer kernel's T / k test (f64 fallback) needs a clip of more than a million gate events; there is no
way to preset the counter and none is added.  "A decay of more than 64 steps" is read as a decaying steady state of more than 64 FRAMES: the law
itself ends a decay after 18 steps (floor - s trunc(floor / 20) > floor / 10), or never when the step is 0 — both are here, under a long pause
so that the unvoiced frames of the run do not finalize the segment."""
import ctypes
import hashlib

import numpy as np

from oracle import pyoracle
from tests import peak_ref

U32 = 4294967295
AUTO = dict(window_step=25.0, pause_length=200.0, min_seg_length=50.0, auto_noise_gate=1, voiced_max_dB=100.0, voiced_min_dB=10.0)
# the arms no case can reach, each with its reason (tests/test_gate_reference.py exempts exactly these)
UNREACHABLE = {
    "d_g_equals_d": "g == d needs every non-zero bin from 1 up to be an accepted top, but a top on a bin >= 3 only closes on a falling bin below the three "
                    "bins before it, which are then non-zero and not all tops; only the end-of-spectrum candidate does without, and it leaves p = 0",
    "ring_cut": "counted by wsa_or_seg_cut, which only the stream tests call (tests/test_gpu_gate.py)",
}


def scan(e):
    """the candidates of frame e by geometry alone (ref @B25827 without `e[l] > v`): [(l, is end-of-spectrum emission)]"""
    return [(l, bool(last)) for _, _, l, last in peak_ref.scan(e)["cands"]]


def _fill_g(e, g, last_free):
    """raise bins 1 .. last_free (a non-rising shelf in front of the first candidate) until sum e[1:] == g"""
    if g is None:
        return
    rest = int(g) - int(e[1:].sum())
    assert rest >= 0 and (rest == 0 or last_free >= 1), ("g below what the candidates weigh, or no room for a shelf", g, rest, last_free)
    if rest:
        q, r = divmod(rest, last_free)
        sh = np.full(last_free, q, np.int64)
        sh[:r] += 1
        assert sh[0] + e[1:last_free + 1].max() <= U32, "shelf does not fit a u32"
        e[1:last_free + 1] += sh
        e[0] = e[1]
    assert int(e[1:].sum()) == g


def sparse(cands, g=None, bands=128):
    """cands: [(bin, amplitude)], bins rising and >= 6 apart, the first >= 2; a bin == bands - 1 is the end-of-spectrum candidate."""
    e = np.zeros(bands, np.int64)
    prev = -4
    for b, a in cands:
        assert a >= 3 and b >= 2 and b - prev >= 6 and b < bands, (b, a)
        e[b - 2], e[b - 1], e[b] = 1, 2, a
        prev = b
    _fill_g(e, g, (cands[0][0] - 6) if cands else bands - 1)
    got = scan(e)
    assert [x[0] for x in got] == [b for b, _ in cands] and all(eos == (b == bands - 1) for b, eos in got), (cands, got)
    return e.astype(np.uint32)


def dense(tops, g=None, bands=128, base=None):
    """tops: [(bin, amplitude)] at least 2 bins apart over a baseline falling by one per bin from `base` (default bands); the last top sits on
    bands - 1 (end of spectrum) or at most on bands - 5 (the flat tail that closes it)."""
    base = bands if base is None else base
    e = base - np.arange(bands, dtype=np.int64)
    assert e.min() >= 1
    for b, a in tops:
        e[b] = a
    last = tops[-1][0]
    if last != bands - 1:
        assert last <= bands - 5
        e[last + 2:] = e[last + 1]
    _fill_g(e, g, tops[0][0] - 4)
    got = scan(e)
    assert [x[0] for x in got] == [b for b, _ in tops], (tops, got)
    return e.astype(np.uint32)


def silence(bands=128):
    return np.zeros(bands, np.uint32)


class Clip:
    """frames pushed into a live oracle segmenter as they are built; .st() is the state the next frame will meet"""

    def __init__(self, settings=AUTO, bands=128):
        self.settings, self.bands = dict(settings), bands
        self.L = pyoracle.lib()
        self.cfg = pyoracle.default_cfg(level=5, bands=bands, **settings)
        self.h = self.L.wsa_or_seg_new(ctypes.byref(self.cfg))
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
        return int(self.L.wsa_or_gate_arm_count(self.h, pyoracle.gate_arm_names().index(name)))

    def push(self, e, times=1):
        e = np.ascontiguousarray(e, np.uint32)
        assert e.shape == (self.bands,)
        for _ in range(times):
            self.frames.append(e)
            self.L.wsa_or_seg_push(self.h, e.ctypes.data)
        return self

    @property
    def n(self):
        return len(self.frames)

    # ---- phrases
    def one(self, amp, b=20, times=1, g=None):
        """a frame with one candidate"""
        return self.push(sparse([(b, int(amp))], g=g, bands=self.bands), times)

    def quiet(self, times=1):
        return self.push(silence(self.bands), times)

    def weak(self, times=1):
        """a candidate above the floor but not above twice the floor: n = 1, p = 0, h = 2 floor (unvoiced, and the gate's steady decay goes on)"""
        for _ in range(times):
            v = int(self.st()["floor"])
            assert 2 * v >= 3 and 2 * v > v
            self.one(2 * v)
        return self

    def start(self, H=1000, b=20, others=None):
        """a frame that passes the start test: the ridge H at bin b and four small tops behind it"""
        v = int(self.st()["floor"])
        others = others or [max(v + 1, 3)] * 4
        assert self.st()["c_started"] < 0
        self.push(sparse([(b, H)] + [(b + 6 * (k + 1), a) for k, a in enumerate(others)], bands=self.bands))
        assert self.st()["c_started"] >= 0, "start frame did not start"
        return self

    def open(self, H=1000, b=20):
        """start + two voiced frames: a running segment (c_started 2) whose ctx_max is H"""
        self.start(H, b)
        self.one(H, b, 2)
        assert self.st()["c_started"] == 2 and (self.st()["ctx_max"] == H or not self.settings["auto_noise_gate"])
        return self

    def close(self):
        """unvoiced frames until the pause finalizes the segment"""
        k = 0
        while self.st()["c_started"] >= 0:
            self.quiet()
            k += 1
            assert k < 1000
        return self

    def spectra(self):
        return np.stack(self.frames) if self.frames else np.zeros((0, self.bands), np.uint32)


CASES = []


def case(name, expect, settings=AUTO, bands=128):
    def deco(fn):
        CASES.append(dict(name=name, expect=expect, settings=dict(settings), bands=bands, build=fn))
        return fn
    return deco


def _built(c):
    if "spectra" not in c:
        clip = Clip(c["settings"], c["bands"])
        c["build"](clip)
        c["spectra"] = clip.spectra()
    return c["spectra"]


def spectra(c):
    return _built(c)


def digest(c):
    s = _built(c)
    return hashlib.sha256(repr((c["name"], sorted(c["settings"].items()), c["bands"], s.shape)).encode() + s.tobytes()).hexdigest()


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


# ------------------------------------------------------------------------------------------------------------------ start test
def _five(H, b, others, g=None, bands=128):
    """the ridge H at bin b and the other tops 6 bins apart behind it"""
    return sparse([(b, H)] + [(b + 6 * (k + 1), a) for k, a in enumerate(others)], g=g, bands=bands)


def _start_edges(c):
    """every clause of the start test failing alone (128 bands: max_voiced_bin 89)"""
    H = 1000
    c.push(_five(H, 20, [10] * 3))                                     # n = 4
    assert c.arm("start_n4") == 1
    c.push(_five(H, 7, [10] * 4))                                      # p = 7
    assert c.arm("start_p7") == 1
    c.push(_five(H, 89, [10] * 4))                                     # p = max_voiced_bin
    assert c.arm("start_pmax") == 1
    c.push(_five(H, 20, [H // 4] * 4))                                 # h (n - 1) == 4 (d - h)
    assert c.arm("start_r_equal") == 1 and c.st()["c_started"] < 0


@case("start-edges", dict(start_n4=1, start_p7=1, start_pmax=1, start_r_equal=1, start_r_above=1, start_pass=3, start_n5=1, start_p8=1, start_pmax_m1=1,
                          unvoiced_at_1=2, unvoiced_at_0=2, voiced_at_0=3))
def _(c):
    _start_edges(c)
    m = 52                                                                                               # h = 4 m + 1, n = 6: h (n - 1) = 4 (d - h) + 1
    c.push(_five(4 * m + 1, 20, [m, m, m, m, m + 1]))
    assert c.arm("start_r_above") == 1 and c.st()["c_started"] == 1
    c.quiet(2)                                                                                           # 1 -> 0 -> -1
    assert c.st()["c_started"] == -1
    v = int(c.st()["floor"])
    c.push(_five(100 * v + 1000, 8, [v + 1] * 4))                                                        # n = 5, p = 8
    assert c.arm("start_n5") == 1 and c.arm("start_p8") == 1
    c.quiet(2)
    v = int(c.st()["floor"])
    c.push(sparse([(52 + 6 * k, v + 1) for k in range(4)] + [(88, 100 * v + 1000)]))                     # p = max_voiced_bin - 1
    assert c.arm("start_pmax_m1") == 1
    c.one(int(c.st()["ctx_max"]), 88, 4)
    c.close()


@case("start-edges-33", dict(start_n4=1, start_p7=1, start_pmax=1, start_r_equal=1, start_pass=1), bands=33)
def _(c):
    # 33 bands: max_voiced_bin 23; candidates 6 bins apart leave room for five
    H = 1000
    c.push(sparse([(8, H), (14, 10), (20, 10), (26, 10)], bands=33))
    c.push(sparse([(7, H), (13, 10), (19, 10), (25, 10), (32, 10)], bands=33))
    c.push(sparse([(2, 10), (8, 10), (14, 10), (23, H), (29, 10)], bands=33))
    c.push(sparse([(2, 250), (8, 250), (14, H), (20, 250), (26, 250)], bands=33))
    assert c.st()["c_started"] < 0
    c.push(sparse([(2, 10), (8, 10), (14, 10), (22, H), (28, 10)], bands=33))
    assert c.st()["c_started"] == 1
    c.one(H, 22, 3)
    c.close()


@case("start-edges-256", dict(start_pmax=1, start_pmax_m1=1, voiced_pmax=1, voiced_pmax_m1=1), bands=256)
def _(c):
    # 256 bands: max_voiced_bin 179, bins past 127 in the header's bin byte
    H = 1000
    c.push(_five(H, 179, [10] * 4, bands=256))
    assert c.st()["c_started"] < 0
    c.push(_five(H, 178, [10] * 4, bands=256))
    c.one(H, 178, 3)
    c.one(H, 179)
    c.one(H, 178, 2)
    c.close()


# ------------------------------------------------------------------------------------------------------------------ voiced test
@case("voiced-edges", dict(voiced_n0=1, voiced_p0=1, voiced_p6=1, voiced_p7=1, voiced_pmax_m1=1, voiced_pmax=1, d_equal=1, d_below=1, d_n3=1,
                           mx_covers=1, mx_short_n3=1, mx_short_d_covers=1, unvoiced_at_2=1, voiced_at_1=1))
def _(c):
    H = 1000
    c.open(H)
    v = int(c.st()["floor"])
    c.quiet()
    c.one(2 * v)                                                       # above the floor, not above twice the floor: p = 0
    c.one(H, 6)
    c.one(H, 7)
    c.one(H, 88)
    c.one(H, 89)
    c.one(H)
    four = [(20, H), (26, 400), (32, 300), (38, 300)]                  # d = 2000, 11 mx = 11000
    c.push(sparse(four, g=22000))                                      # 11 d == g: voiced
    assert c.arm("d_equal") == 1 and c.st()["no_fm"] == 0
    c.push(sparse(four, g=22001))                                      # 11 d == g - 1: unvoiced
    assert c.arm("d_below") == 1 and c.st()["no_fm"] == 1
    c.push(sparse(four[:3], g=40000))                                  # n == 3: the clause is not asked
    assert c.arm("d_n3") == 1 and c.st()["no_fm"] == 0
    c.push(sparse(four, g=11000))                                      # 11 mx >= g at equality
    c.push(sparse(four, g=11001))                                      # 11 mx < g <= 11 d
    assert c.arm("mx_short_d_covers") >= 1 and c.st()["no_fm"] == 0
    c.one(H, times=2)
    c.close()


@case("unvoiced-start", dict(unvoiced_at_0=1, start_pass=2))
def _(c):
    # a frame that passes the start test and fails the voiced test's d clause: 0 -> -1 in the frame that started
    c.push(_five(1000, 20, [10] * 4, g=12000))
    assert c.st()["c_started"] == -1 and c.arm("start_pass") == 1
    c.open(1000)
    c.close()


@case("header-largest", dict(hdr_eos_largest=2, hdr_tie=2))
def _(c):
    H = 1000
    c.open(H)
    c.push(sparse([(20, H), (127, 5000)]))                             # the end-of-spectrum candidate is the largest: h, p stay the ridge's
    assert c.st()["ctx_max"] == H
    c.push(sparse([(127, 5000)]))                                      # ... and alone: n = 1, p = 0
    c.push(sparse([(20, H), (100, H)]))                                # tie: the first wins (bin 100 would be unvoiced)
    assert c.st()["no_fm"] == 0
    c.push(sparse([(14, 30), (100, H), (110, H)]))                     # a tie outside the voiced range
    c.one(H, times=2)
    c.close()


# ------------------------------------------------------------------------------------------------------------------ noise gate
@case("gate-w-and-decay", dict(gate_raise_above=1, gate_w40=1, gate_w41=1, gate_decay=1, gate_decay_edge=1, decay_first_w21=1, decay_stop=1,
                               gate_neither=3, gate_decay_refused_equal=1, gate_raise_equal_w=1, floor_t2=1))
def _(c):
    c.open(9999)                                                       # last_max = 9999 = 100 h - 1 for h = 100
    v = int(c.st()["floor"])
    assert 2 * v < 100
    while c.st()["w"] < 40:
        c.one(100)
    assert c.arm("gate_w40") == 1 and c.arm("gate_decay") == 0
    c.one(100)                                                         # w = 41: 100 h == last_max + 1, the decay arm
    assert c.arm("gate_decay_edge") == 1 and c.st()["w"] == 35
    H = int(c.st()["ctx_max"])
    c.one(10000)                                                       # raise: last_max = 10000
    while c.st()["w"] < 40:
        c.one(100)
    c.one(100)                                                         # 100 h == last_max: neither arm; from here on every frame recomputes the floor
    assert c.arm("gate_decay_refused_equal") == 1 and c.st()["ctx_max"] == 10000
    c.one(100, times=3)
    c.one(10000)                                                       # h == ctx_max through `w > 40`
    assert c.arm("gate_raise_equal_w") == 1 and H < 10000
    c.one(10000, times=2)
    c.close()


@case("floor-law-arms", dict(floor_t1=1, floor_one=1, floor_t2=1, floor_t4=1, floor_t6=1, floor_t7=1, tk_reset_voiced=2, gate_decay=10))
def _(c):
    # ctx_max starts at 50 and only the decay arm brings it down: h stays just above twice the floor until ctx_max rests at 7
    c.start(40, others=[3, 3, 3, 3])
    k = 0
    while True:
        s = c.st()
        h = max(2 * int(s["floor"]) + 1, 3)
        if not h < s["ctx_max"] or c.arm("floor_one") >= 3:
            break
        c.one(h)
        k += 1
        assert k < 400
    assert c.arm("floor_one") >= 1 and c.arm("floor_t1") >= 1
    for H in (1000, 200000, 2000000, 20000000, U32):
        c.one(H, times=2)
    assert c.st()["ctx_max"] == U32
    c.close()


@case("tk-reset", dict(tk_equal=1, tk_reset_voiced=1, tk_reset_unvoiced=1))
def _(c):
    c.open(360)
    c.one(2000)                                                        # T / k = 360 = 30 v(2000): no reset
    assert c.arm("tk_equal") == 1 and c.st()["floor"] == 12 and c.st()["c_started"] == 2
    c.one(2000, times=2)
    c.one(1000000)                                                     # T / k far below 30 v: reset in a voiced frame, the stale bit
    assert c.arm("tk_reset_voiced") == 1 and c.st()["c_started"] == 1
    c.one(1000000, times=3)
    c.one(4000000000, b=100)                                           # unvoiced (bin past the voiced range) and loud: reset, span begins at the next frame
    assert c.arm("tk_reset_unvoiced") == 1 and c.st()["c_started"] == 0 and c.st()["span_begin"] == c.n
    c.one(4000000000, times=4)
    c.close()


LONG_PAUSE = dict(AUTO, pause_length=5000.0)


@case("slow-decay", dict(decay_first_w21=1, decay_stop=40), settings=LONG_PAUSE)
def _(c):
    # under a 200-frame pause the unvoiced weak frames keep the gate in its steady decay: 18 steps down to last_floor / 10, then rest (> 64 frames)
    c.open(1000000)
    assert c.st()["floor"] == 5000
    c.weak(90)
    assert c.st()["floor"] == 500 and c.arm("decay_stop") > 40
    c.one(1000000, times=2)
    c.close()


@case("slow-decay-clamp", dict(decay_clamp10=1, decay_stop=10), settings=LONG_PAUSE)
def _(c):
    y = next(y for y in range(10001, 11000) if _law(y) == 51)          # floor 51: 49, 47 .. 11, then 9 -> the clamp to 10
    c.open(y)
    assert c.st()["floor"] == 51
    c.weak(50)
    assert c.st()["floor"] == 10
    c.one(y, times=2)
    c.close()


@case("slow-decay-zero-step", dict(decay_zero_step=64), settings=LONG_PAUSE)
def _(c):
    y = next(y for y in range(3375, 4096) if _law(y) == 15)            # floor 15: trunc(15 / 20) = 0, the floor never moves and the decay never ends
    c.open(y)
    c.weak(100)
    assert c.st()["floor"] == 15
    c.one(y, times=2)
    c.close()


def _law(y):
    L = pyoracle.lib()
    t = L.wsa_or_log10(float(y))
    if t > 7: return int(L.wsa_or_pow(10.0, t - 3) / 20)
    if t > 6: return int(L.wsa_or_pow(10.0, t - 3) / 2)
    if t > 4: return int(L.wsa_or_pow(10.0, t - 2) / 2)
    if t > 2: return int(L.wsa_or_pow(10.0, t / 3))
    if t > 1: return int(y / 10)
    return 1


# ------------------------------------------------------------------------------------------------------------------ pause, finalize
def _short_and_kept(c):
    c.start(1000); c.one(1000); c.close()                              # two voiced frames: len == min_frames, dropped
    c.open(1000); c.close()                                            # three: len == min_frames + 1, kept


@case("pause-integer", dict(pause_int=2, fin_len_min=1, fin_len_min1=1))
def _(c):
    _short_and_kept(c)


@case("pause-fraction", dict(pause_frac=2, fin_len_min=1, fin_len_min1=1), settings=dict(AUTO, pause_length=210.0))
def _(c):
    _short_and_kept(c)                                                 # breaker 8.4: the ninth unvoiced frame ends the segment


@case("pause-rule-250", dict(breaker_rule_250=1, pause_int=2), settings=dict(AUTO, pause_length=40.0))
def _(c):
    _short_and_kept(c)                                                 # pause_length <= 2 window_step: breaker = 250 / window_step = 10


@case("end-unstarted", dict(fin_end_unstarted=1, unvoiced_at_1=2))
def _(c):
    c.start(1000); c.quiet(); c.one(1000); c.quiet(); c.one(1000)      # c_started 1 0 1 0 1 at the end of input: long enough, never started


@case("end-open", dict(fin_truncate_open=1))
def _(c):
    c.open(1000); c.one(1000, times=5)


# ------------------------------------------------------------------------------------------------------------------ crowded frames
def _run(b0, amps):
    return [(b0 + 2 * k, int(a)) for k, a in enumerate(amps)]


def crowd_all(K):
    """K tops from bin 9 up, rising from 6000, the last one the ridge (20000): every one above a floor of 5000"""
    return dense(_run(9, [6000 + k for k in range(K - 1)] + [20000]))


def crowd_late_start():
    """21 tops: sixteen at 200 .. 215 (below a floor of 500 .. 5000), then 6000 .. 6003 and the ridge 1000000: n = 5, all behind the 16 staged ones"""
    return dense(_run(9, [200 + k for k in range(16)] + [6000, 6001, 6002, 6003, 1000000]))


def crowd_late_n3():
    """twenty tops, four accepted (all behind the 16th) and a shelf that makes 11 d < g"""
    amps = [200 + k for k in range(16)] + [6000, 6001, 6002, 20000]
    return dense(_run(9, amps), g=11 * 38003 + 1)


def crowd_late_d(extra=0):
    """twenty tops; accepted: the 16th (6000), 6001, 6002, 6003 and the ridge 20000: d = 44006, g = 11 d + extra — the first 16 alone would say 11 d < g"""
    amps = [200 + k for k in range(15)] + [6000, 6001, 6002, 6003, 20000]
    return dense(_run(9, amps), g=11 * 44006 + extra)


def crowd_64(lo):
    """a top on every odd bin, 64 of them, rising from lo: the largest but one sits on bin 125, the largest is the end-of-spectrum candidate"""
    return dense(_run(1, [lo + k for k in range(64)]))


def crowd_63_ridge(top):
    """63 tops just below `top` with the ridge `top` at bin 87 (voiced): 11 mx < g, so d — a sum of 63 amplitudes near `top` — decides"""
    a = [(1 + 2 * k, top - 100 + k) for k in range(43)] + [(87, top)] + [(91 + 2 * k, top - 100 + k) for k in range(19)]
    e = (top - 101) - np.arange(128, dtype=np.int64)
    for b, v in a:
        e[b] = v
    assert [x[0] for x in scan(e)] == [b for b, _ in a]
    return e.astype(np.uint32)


@case("crowded-frames", dict(cand_16=1, cand_17=1, cand_64=2, late_n4=1, late_n3=1, late_d=1, d_below=1, d_equal=1, hdr_eos_largest=1))
def _(c):
    c.open(1000000)
    assert c.st()["floor"] == 5000
    c.push(crowd_all(16))
    c.push(crowd_all(17))
    c.push(crowd_late_n3())
    assert c.arm("late_n3") == 1 and c.st()["no_fm"] == 1
    c.push(crowd_late_d())                                             # 11 d == g
    assert c.arm("late_d") == 1 and c.st()["no_fm"] == 0
    c.push(crowd_late_d(1))                                            # 11 d == g - 1
    assert c.st()["no_fm"] == 1
    c.push(crowd_64(20000))                                            # the end-of-spectrum candidate (20063) is the largest: h, p are bin 125's
    c.one(1000000, times=2)
    c.close()
    c.push(crowd_64(6000))                                             # idle: 64 accepted, the largest outside the start range
    c.push(crowd_late_start())
    assert c.arm("late_n4") == 1 and c.st()["c_started"] == 1
    c.one(1000000, times=3)
    c.close()


@case("u32-ends", dict(cand_64=2, floor_t7=1, mx_short_d_covers=1))
def _(c):
    c.open(U32)                                                        # a dominant candidate of 4294967295
    c.one(U32, times=2)
    c.push(crowd_64((1 << 26) - 32))                                   # 64 accepted near 2^32 / 64: d just past 2^32
    c.one(U32)
    c.push(crowd_63_ridge(U32))                                        # d near 2^38, g near 2^39
    assert c.st()["no_fm"] == 0
    e = (U32 - 64) - np.arange(128, dtype=np.int64)                    # every bin near 2^32 and 64 tops: g = 127 x 2^32 - ..., just below 2^39
    e[1::2] = U32 - 63 + np.arange(64)
    assert len(scan(e)) == 64 and e[1:].sum() > 0.99 * 2 ** 39
    c.push(e.astype(np.uint32))
    c.one(U32, times=2)
    c.close()


# ------------------------------------------------------------------------------------------------------------------ lengths, block edges
def _length_case(N):
    def build(c):
        if N == 0:
            return
        if N < 12:
            c.start(1000)
            while c.n < N:
                c.one(1000)
            return
        c.quiet(2)
        c.open(1000)
        while c.n < N - 8:
            c.one(1000)
        c.quiet(8)                                                     # the pause runs out on the clip's last frame
        assert c.n == N and c.st()["c_started"] == -1
    return build


for _N in (0, 1, 63, 64, 65, 128, 129):
    case("length-%d" % _N, {} if _N < 12 else dict(pause_int=1))(_length_case(_N))


def _idle(c, upto):
    """idle frames up to frame `upto` (exclusive): silence, and ridges in the start range that fail `n > 4`"""
    while c.n < upto:
        if c.n % 5 == 3:
            c.one(1000)
        else:
            c.quiet()
    assert c.st()["c_started"] == -1


def _event_start(P):
    def build(c):
        _idle(c, P)
        c.open(1000)
        assert c.st()["span_begin"] == P
        c.one(1000, times=70)                                          # a running span across the next block edge
        c.close()
    return build


def _event_tk(P):
    def build(c):
        c.open(360)
        while c.n < P:
            c.one(360)
        c.one(1000000)
        assert c.arm("tk_reset_voiced") == 1 and c.st()["span_begin"] == P
        c.one(1000000, times=4)
        c.close()
    return build


def _event_pause(P):
    def build(c):
        c.open(1000)
        while c.n < P - 7:
            c.one(1000)
        c.quiet(8)
        assert c.n == P + 1 and c.st()["c_started"] == -1 and c.arm("pause_int") == 1
        _idle(c, P + 6)
        c.open(1000)
        c.close()
    return build


def _event_crowd(P):
    def build(c):
        c.open(1000000)
        while c.n < P:
            c.one(20000)
        c.push(crowd_late_d())
        assert c.arm("late_d") == 1
        c.one(20000, times=3)
        c.close()
    return build


def _event_decay_end(P):
    def build(c):
        _idle(c, P - 38)
        c.open(1000000)                                                # the frame P - 38 raises ctx_max (w = 0): frame f meets w = f - (P - 38)
        while c.n <= P:
            c.one(20000)
        assert c.st()["floor"] == 500 and c.st()["w"] == 38 and c.arm("decay_stop") == 0
        c.one(20000, times=6)
        assert c.arm("decay_stop") >= 1
        c.close()
    return build


for _P in (63, 64, 65):
    case("start-at-%d" % _P, dict(start_pass=1))(_event_start(_P))
    case("tk-reset-at-%d" % _P, dict(tk_reset_voiced=1))(_event_tk(_P))
    case("pause-at-%d" % _P, dict(pause_int=2))(_event_pause(_P))
    case("crowd-at-%d" % _P, dict(late_d=1))(_event_crowd(_P))
    case("decay-end-at-%d" % _P, dict(decay_stop=1, decay_first_w21=1))(_event_decay_end(_P))


# ------------------------------------------------------------------------------------------------------------------ densest segmentation
def _densest(c, periods=24):
    """segments of min_frames + 1 frames (never fewer than the two that reach c_started 2), each followed by ceil(breaker) unvoiced frames"""
    mf = int(c.settings["min_seg_length"] // c.settings["window_step"])
    for _ in range(periods):
        c.start(1000)
        c.one(1000, times=max(mf, 1))
        c.close()


DENSE_SETTINGS = {"densest-int": dict(AUTO), "densest-frac": dict(AUTO, pause_length=210.0), "densest-int-min0": dict(AUTO, min_seg_length=10.0),
                  "densest-frac-min0": dict(AUTO, min_seg_length=10.0, pause_length=210.0)}
for _name, _s in DENSE_SETTINGS.items():
    case(_name, dict(start_pass=24, fin_len_min1=24) if _s["min_seg_length"] >= 25 else dict(start_pass=24), settings=_s)(_densest)


# ------------------------------------------------------------------------------------------------------------------ fixed gate (the f64 kernel)
FIXED = dict(AUTO, auto_noise_gate=0, voiced_min_dB=35.0)              # floor 10^1.75 = 56.23..., 2 floor = 112.46...: r keeps its division


@case("fixed-start-edges", dict(start_n4=1, start_p7=1, start_pmax=1, start_r_equal=1, start_r_above=1, start_pass=1), settings=FIXED)
def _(c):
    H = 1000
    c.push(sparse([(20, H), (26, 100), (32, 100), (38, 100)]))
    c.push(_five(H, 7, [100] * 4))
    c.push(_five(H, 89, [100] * 4))
    c.push(_five(H, 20, [250] * 4))
    c.push(_five(H, 20, [56] * 4))                                     # 56 is not above the floor: n = 1
    assert c.st()["c_started"] == -1 and c.arm("start_r_equal") == 1
    c.push(_five(401, 20, [100, 100, 100, 100, 101]))                  # h (n - 1) = 2005 = 4 (d - h) + 1
    assert c.arm("start_r_above") == 1
    c.one(H, times=3)
    c.close()


@case("fixed-voiced-edges", dict(voiced_n0=1, voiced_p0=2, voiced_p6=1, voiced_p7=1, voiced_pmax=1, voiced_pmax_m1=1, d_equal=1, d_below=1, d_n3=1,
                                 mx_short_d_covers=1), settings=FIXED)
def _(c):
    H = 1000
    c.open(H)
    c.one(57); c.one(112)                                              # above the floor, not above twice the floor
    c.one(113)                                                         # above twice the floor
    assert c.st()["no_fm"] == 0
    c.quiet()
    c.one(H, 6); c.one(H, 7); c.one(H, 88); c.one(H, 89); c.one(H)
    four = [(20, H), (26, 400), (32, 300), (38, 300)]
    c.push(sparse(four, g=22000))
    assert c.st()["no_fm"] == 0
    c.push(sparse(four, g=22001))
    assert c.st()["no_fm"] == 1
    c.push(sparse(four[:3], g=40000))
    c.push(sparse(four, g=11001))
    c.one(H, times=2)
    c.close()


if __name__ == "__main__":
    tot = {}
    for c in CASES:
        r = pyoracle.run_backend(spectra(c), pyoracle.default_cfg(level=5, bands=c["bands"], **c["settings"]), gate=True)
        print("%-22s %4d frames %2d segments" % (c["name"], len(spectra(c)), len(r["segments_ci"])))
        for k, v in r["gate"]["arms"].items():
            tot[k] = tot.get(k, 0) + v
    print("frames in all:", sum(len(spectra(c)) for c in CASES))
    print("arms never taken:", [k for k, v in tot.items() if not v])

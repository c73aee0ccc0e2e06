"""Hand-built stream sets for the input half of a plain stream set's step (csrc/stream_step.hip plan_plain_step, csrc/stream_input.hip
stream_stage_kernel / stream_pull_kernel, the front end as a step launches it): geometries, frames per step, schedules, signals and an integer model of
what every step must deliver.  Used by tests/test_stream_input_reference.py (a numpy restatement of the device forms against the model, the modelled
faults; no GPU) and tests/test_gpu_stream_input.py (the step itself against the oracle FE-1, bit for bit).

Geometries: the smallest at which each form exists.  `inst` is the K1 instantiation the GPU test asserts through wsa_debug_fe_choice.
  name          fs     width / step (ms)  win, hop, q, hist   what it reaches
  16k-25-10     16000  25 / 10            400, 160, 3, 320    win < q hop; the baseline r8 instantiation with pcm_off
  16k-30-10     16000  30 / 10            480, 160, 3, 320    win == q hop: the last frame ends on the stage's last sample
  22k05-25-20   22050  25 / 20            551, 441, 2, 441    odd window and odd hop: pcm_off and frame starts off the 8-byte grid, n in_stride no multiple of 4
  48k-60-10     48000  60 / 10            2880, 480, 6, 2400  hist > 256 (the shuffle's strided loops), hist > step_samples for F <= 4, radix-3 family
  16k-16-1      16000  16 / 1             256, 16, 16, 240    15 warm-up frames spread over many steps, step_samples < hist
  8k-16-1       8000   16 / 1             128, 8, 16, 120     the same in the rx family
  16k-10-25     16000  10 / 25            160, 400, 1, 0      step > width: no history and no stage, d_pcm goes straight to the front end
None was refused by the library.  16k-16-1 was meant to reach the rx family and does not: the FFT length follows the sample rate, not the window, and
16 kHz runs fe_kernel_r8<2,9,12,false> at any window up to 256 samples.  It stays, and 8k-16-1 (fe_kernel_rx<4,2,12>) has the same q, the same warm-up
and step_samples < hist in the rx family.

Frames per step: F = 1, 2, q - 1, q and 5 everywhere (duplicates and zeros dropped), 100 and 101 at 16k-25-10 (frames_per_wave = min(25, ceil(F / 4)):
one chunk per stream up to F = 100, two from 101 on), 4 at 48k-60-10.

Schedules: one set of 7 streams per (geometry, F), stream i on SCHEDULES[i], so that a step holds streams with nfr = 0, partial and F side by side;
12 steps, or W + 8 with W = ceil((q - 1) / F) warm-up steps if that is more.  A launch that is to show frames needs W + 1 steps, and two launches do not
both get them inside W + 8 steps when W is large: in the restart schedules launch B gets max(W + 3, steps / 2) steps and launch A the rest (at 16k-16-1
with F <= 2 launch A is restarted before it leaves its warm-up: its samples are in the history all the same).  `pause` idles for 1, then 2, then q steps
where q fits; where it does not (q = 6 and 16) the third pause is what leaves the launch W + 2 active steps and one in front of the first pause, at
least 3 steps.

Signals: integer-hash noise (knn_cases.mix: no random generator) scaled into +-0.5, another per stream and per launch.  NaN stands in the row of a stream
in every step in which it is idle, in the padding behind samples_per_step, and in launch A's final `hist` samples in the three restart schedules that let
A run (restart-after-stop, restart-after-idle, restart-live): the oracle then gives zeros for A's last frames (F8), and any frame of B that touches the
stale history shows.  For the 16-bit arrangement the same samples are rounded to int16 codes (NaN: 32767) and the expected frames come from the decoded
codes (capi.pcm_decode, as tests/test_gpu_stream_pcm.py decodes them).

The model.  plan(ctl, q, F) is written from include/wsa.h (wsa_stream_step) and DESIGN section 5 alone and sees no kernel output.  The rule: a launch's
clip is the concatenation of the samples the stream was handed in its ACTIVE steps since its START; an idle step is a step in which no time passes for
that stream.  Frame k of the launch covers samples [k hop, k hop + win) and is delivered in the step whose samples bring the clip to (k + q) hop samples:
the step that hands over its last sample, or the step after where win < q hop leaves it short of q hop.  The first delivered frame is frame 0.  The frames
an active step does not deliver are the first ones of its row: off = (F - nfr) hop samples.
"""
import functools

import numpy as np

from oracle import pyoracle
from tests.knn_cases import mix

ACTIVE, START, STOP = 1, 2, 4            # WSA_STREAM_* (include/wsa.h)
N_STREAMS = 7


class Geometry:
    def __init__(self, name, fs, width, step, win, hop, q, hist, inst, extra_F=()):
        self.name, self.fs, self.width, self.step = name, float(fs), float(width), float(step)
        self.win, self.hop, self.q, self.hist, self.inst, self.extra_F = win, hop, q, hist, inst, tuple(extra_F)

    @property
    def config_kw(self):
        return dict(window_width=self.width, window_step=self.step)

    @functools.lru_cache(maxsize=None)
    def oracle(self):
        return pyoracle.FrontEnd(pyoracle.fe_cfg(fs=self.fs, window_width=self.width, window_step=self.step))

    @property
    def frames_per_step(self):
        out = []
        for F in (1, 2, self.q - 1, self.q, 5) + self.extra_F:
            if F > 0 and F not in out:
                out.append(F)
        return out


GEOMETRIES = [
    Geometry("16k-25-10", 16000, 25, 10, 400, 160, 3, 320, "fe_kernel_r8<4,5,8,true,4,3>", extra_F=(100, 101)),
    Geometry("16k-30-10", 16000, 30, 10, 480, 160, 3, 320, "fe_kernel_r8<4,5,8,true,4,3>"),
    Geometry("22k05-25-20", 22050, 25, 20, 551, 441, 2, 441, "fe_kernel_r3<4,5,14,3>"),
    Geometry("48k-60-10", 48000, 60, 10, 2880, 480, 6, 2400, "fe_kernel_r3<8,24,14>", extra_F=(4,)),
    Geometry("16k-16-1", 16000, 16, 1, 256, 16, 16, 240, "fe_kernel_r8<2,9,12,false>"),
    Geometry("8k-16-1", 8000, 16, 1, 128, 8, 16, 120, "fe_kernel_rx<4,2,12>"),
    Geometry("16k-10-25", 16000, 10, 25, 160, 400, 1, 0, "fe_kernel_r8<2,9,12,false>"),
]
BY_NAME = {g.name: g for g in GEOMETRIES}
I16_GEOMETRIES = ("16k-25-10", "22k05-25-20")

SCHEDULES = ("plain", "late-start", "restart-after-stop", "restart-after-idle", "restart-live", "restart-in-warm-up", "pause")
POISONED = ("restart-after-stop", "restart-after-idle", "restart-live")           # launch A's final hist samples are NaN
RESTARTS = ("restart-after-stop", "restart-after-idle", "restart-live", "restart-in-warm-up")


def warm_steps(q, F):
    return -(-(q - 1) // F)


def n_steps(q, F):
    return max(12, warm_steps(q, F) + 8)


def schedule(name, q, F):
    """-> (ctl [steps] control bytes, launch [steps]: which launch's samples the step carries (0 = A, 1 = B, None = idle))"""
    T, W = n_steps(q, F), warm_steps(q, F)
    ctl, launch = [0] * T, [None] * T

    def run(first, last, which, stop):
        for k in range(first, last + 1):
            ctl[k] = ACTIVE | (START if k == first else 0) | (STOP if stop and k == last else 0)
            launch[k] = which

    b_len = max(W + 3, T // 2)
    if name == "plain":
        run(0, T - 1, 0, True)
    elif name == "late-start":
        run(3, T - 1, 0, True)
    elif name == "restart-after-stop":
        run(0, T - b_len - 1, 0, True); run(T - b_len, T - 1, 1, True)
    elif name == "restart-after-idle":
        run(0, T - b_len - 3, 0, True); run(T - b_len, T - 1, 1, True)
    elif name == "restart-live":
        run(0, T - b_len - 1, 0, False); run(T - b_len, T - 1, 1, True)
    elif name == "restart-in-warm-up":
        if F < q - 1:
            a = max(1, W // 2)                        # a F < q - 1: launch A's warm-up counter is still above 0 at the second START
            assert a * F < q - 1
            run(0, a - 1, 0, False); run(a, T - 1, 1, True)
        else:
            return schedule("restart-live", q, F)
    elif name == "pause":
        p3 = min(q, T - W - 5, T - 7)                 # W + 2 active steps at least, and one in front of the first pause
        assert p3 >= 3 or p3 == q
        idle = 3 + p3
        b0 = T - idle - 3
        assert b0 >= 1 and T - idle >= W + 2
        run(0, T - 1, 0, True)
        k = b0
        for p in (1, 2, p3):
            for _ in range(p):
                ctl[k], launch[k] = 0, None
                k += 1
            k += 1                                    # one active step between the pauses, and behind the last
        assert k == T
    else:
        raise KeyError(name)
    return ctl, launch


def device_bits(cb):
    """a control byte as the device control word: 1 START, 2 STOP, 4 active in this step"""
    return (1 if cb & START else 0) | (2 if cb & STOP else 0) | (4 if cb & ACTIVE else 0)


def plan(ctl, q, F, hop=1):
    """The model, for one stream: per step (nfr, off in samples, bits, [(launch, k) of slot 0 .. nfr - 1]).  Launches count from 0 at every START."""
    out, launch, have = [], -1, 0                     # have: hops of the current launch's clip handed over so far
    for cb in ctl:
        if cb & START:
            launch, have = launch + 1, 0
        slots = []
        if cb & ACTIVE:
            assert launch >= 0, "ACTIVE before the first START: outside the model"
            # frame k arrives when the clip reaches (k + q) hops: have < k + q <= have + F
            slots = [(launch, k) for k in range(max(have + 1 - q, 0), have + F - q + 1)]
            have += F
        nfr = len(slots)
        out.append((nfr, (F - nfr) * hop if cb & ACTIVE else 0, device_bits(cb), slots))
    return out


def _noise(geometry, stream, launch, n):
    h = mix(np.arange(n, dtype=np.uint64), np.uint64(8 * stream + launch), 0x51A7 + 977 * GEOMETRIES.index(geometry))
    return ((h.astype(np.float64) + 0.5) / 4294967296.0 - 0.5).astype(np.float32)


def _speech(geometry, stream, launch, n):
    """synthetic speech, for the end-to-end check alone: noise closes no segment, and a check of rows needs rows"""
    from webspeechanalyzer_amd.synth import synth_clips
    return synth_clips(1, n, fs=int(geometry.fs), seed=1000 + 8 * stream + launch, device="cpu")[0].numpy().copy()


def _to_i16(x):
    return np.where(np.isnan(x), 32767, np.clip(np.rint(np.nan_to_num(x).astype(np.float64) * 32767.0), -32768, 32767)).astype(np.int16)


class Case:
    """one stream set: a geometry, F, and the seven schedules"""

    def __init__(self, geometry, F, speech=False):
        g = self.geometry = geometry
        self.F, self.name = F, f"{geometry.name}-F{F}" + ("-speech" if speech else "")
        self.sps = F * g.hop
        self.steps = n_steps(g.q, F)
        both = [schedule(name, g.q, F) for name in SCHEDULES]
        self.ctl = np.array([c for c, _ in both], np.uint8).T.copy()                 # [steps, streams]
        self.launch = [l for _, l in both]                                           # [streams][steps]
        self.plan = [plan(c, g.q, F, g.hop) for c, _ in both]                        # [streams][steps]
        self.clips = []                                                              # [streams][launch] float32
        for s, name in enumerate(SCHEDULES):
            per = []
            for which in (0, 1):
                n = sum(1 for l in self.launch[s] if l == which) * self.sps
                if n == 0:
                    continue
                x = _speech(g, s, which, n) if speech else _noise(g, s, which, n)
                if which == 0 and name in POISONED and g.hist:
                    x[max(n - g.hist, 0):] = np.nan
                x.setflags(write=False)
                per.append(x)
            self.clips.append(per)

    def clip(self, s, which, fmt="f32"):
        """launch `which` of stream s as the front end sees it: the floats, or the decode of their 16-bit codes"""
        if fmt == "f32":
            return self.clips[s][which]
        from webspeechanalyzer_amd import capi
        return capi.pcm_decode("i16", _to_i16(self.clips[s][which]))

    def rows(self, k, fmt="f32"):
        """step k's input: [streams, samples_per_step]; float32 with NaN in the rows of idle streams, or int16 codes with 32767 there"""
        out = np.full((N_STREAMS, self.sps), np.nan, np.float32)
        for s in range(N_STREAMS):
            which = self.launch[s][k]
            if which is not None:
                done = sum(1 for l in self.launch[s][:k] if l == which)
                out[s] = self.clips[s][which][done * self.sps:(done + 1) * self.sps]
        return out if fmt == "f32" else _to_i16(out)

    @functools.lru_cache(maxsize=None)
    def expected(self, fmt="f32"):
        """[streams][launch] -> the oracle's u32 frames of the launch's clip"""
        fe = self.geometry.oracle()
        return [[fe.run(self.clip(s, w, fmt)) for w in range(len(self.clips[s]))] for s in range(N_STREAMS)]

    def poisoned_frames(self, s, which):
        """frames of the launch whose window holds a NaN sample"""
        g, x = self.geometry, self.clips[s][which]
        bad = np.flatnonzero(np.isnan(x))
        if not len(bad):
            return set()
        nf = g.oracle().n_frames(len(x))
        return {k for k in range(nf) if k * g.hop + g.win > bad[0] and k * g.hop <= bad[-1]}


@functools.lru_cache(maxsize=None)
def case(gname, F):
    return Case(BY_NAME[gname], F)


# the end-to-end check: synthetic speech, a quarter of a second per step, so that launch B (six steps) closes a segment
E2E_FRAMES = {"16k-25-10": 25, "16k-30-10": 25, "22k05-25-20": 12, "48k-60-10": 25, "16k-16-1": 100, "8k-16-1": 100, "16k-10-25": 10}


@functools.lru_cache(maxsize=None)
def speech_case(gname):
    return Case(BY_NAME[gname], E2E_FRAMES[gname], speech=True)


def all_cases():
    return [case(g.name, F) for g in GEOMETRIES for F in g.frames_per_step]

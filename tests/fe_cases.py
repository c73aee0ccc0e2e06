"""Hand-built geometries and frames for the front end K1 (csrc/fe_r8.hip, fe_rx.hip, fe_r3.hip): each geometry sits on one edge of the instantiation
table (az = ceil(win / 128) changing, win == 128 AF, odd windows, kmax == N2, three bands in a lane, triangles narrower than a bin, a band clamped at kmax,
a gap between frames), each frame on one rule of FE-1 or of a device form (tests/fe_ref.py).  Used by tests/test_fe_reference.py (oracle against the
float64 statement, the modelled faults) and tests/test_gpu_frontend.py (kernels against the oracle, bit for bit).

A clip is three frames long unless said otherwise: frames 0 and 2 are quiet noise, frame 1 carries the case, so a leak between neighbouring frames shows.
Everything that is searched for (amplitudes, gains) is searched on the CPU with the oracle and fe_ref, inside the condition written at the search, and
the condition is asserted: no case is ever skipped.
"""
import functools
import re
import zlib

import numpy as np

from oracle import pyoracle
from tests import fe_ref

QUIET = 1e-3


class Geometry:
    def __init__(self, name, fs, inst, **kw):
        self.name, self.fs, self.inst, self.kw = name, float(fs), inst, kw          # kw: settings as webspeechanalyzer_amd.Config names them

    def oracle_kw(self, gain=None, emph=None):
        k = {("n_" + a[2:] if a.startswith("N_") else a): v for a, v in self.kw.items() if a != "output_level"}
        if gain is not None:
            k["pre_norm_gain"] = gain
        if emph is not None:
            k["high_f_emph"] = emph
        return k

    def config_kw(self, gain=None, emph=None):
        k = dict(self.kw)
        if gain is not None:
            k["pre_norm_gain"] = gain
        if emph is not None:
            k["high_f_emph"] = emph
        return k

    @functools.lru_cache(maxsize=None)
    def oracle(self, gain=None, emph=None):
        return pyoracle.FrontEnd(pyoracle.fe_cfg(fs=self.fs, **self.oracle_kw(gain, emph)))

    @functools.lru_cache(maxsize=None)
    def ref(self, gain=None, emph=None):
        return fe_ref.FeRef(fs=self.fs, **self.oracle_kw(gain, emph))

    @functools.lru_cache(maxsize=None)
    def form(self):
        """what the instantiation's template arguments say: family, R8 = 8 R (lane 0's bins are its multiples), AF, and the band form with MW / MWL"""
        fam, args = re.match(r"fe_kernel_(r8|rx|r3)<(.*)>", self.inst).groups()
        a = [x for x in args.split(",")]
        fe = self.oracle()
        if fam == "r8":
            mw = int(a[2]); mwl = int(a[4]) if len(a) > 4 else mw; af = int(a[5]) if len(a) > 5 else 0; r = 8
        elif fam == "rx":
            mw = mwl = int(a[2]); af = 0; r = int(a[0])
        else:
            mw = mwl = int(a[2]); af = int(a[4]) if len(a) > 4 else 0; r = int(a[0])
        st = self.kw.get("spec_type", 1)
        two = False
        if st == 1 and fe.bands <= 128:
            cnt = self.ref().cnt
            two = bool(cnt[:64].max() <= mwl and (len(cnt) <= 64 or cnt[64:].max() <= mw))
        return dict(family=fam, R8=8 * r * (3 if fam == "r3" else 1), AF=af, two_band=two, MW=mw, MWL=mwl)


def _ms(win, fs):
    return win * 1000.0 / fs


GEOMETRIES = [
    # 16 kHz, 1024 points: az = ceil(win / 128) = 2 -> 3, the AF = 3 edge win >= 384, az = 4 -> 5
    Geometry("16k-win256", 16000, "fe_kernel_r8<2,9,12,false>", output_level=2, window_width=_ms(256, 16000), window_step=_ms(256, 16000)),
    Geometry("16k-win258", 16000, "fe_kernel_r8<4,5,8,true,4>", output_level=2, window_width=_ms(258, 16000), window_step=_ms(258, 16000)),
    Geometry("16k-win383", 16000, "fe_kernel_r8<4,5,8,true,4>", output_level=2, window_width=_ms(383, 16000), window_step=_ms(383, 16000)),
    Geometry("16k-win384", 16000, "fe_kernel_r8<4,5,8,true,4,3>", output_level=2, window_width=_ms(384, 16000), window_step=_ms(384, 16000)),
    Geometry("16k-default", 16000, "fe_kernel_r8<4,5,8,true,4,3>", output_level=2),
    Geometry("16k-win512", 16000, "fe_kernel_r8<4,5,8,true,4,3>", output_level=2, window_width=_ms(512, 16000), window_step=_ms(512, 16000)),
    Geometry("16k-win514", 16000, "fe_kernel_r8<8,9,12,false>", output_level=2, window_width=_ms(514, 16000), window_step=_ms(514, 16000)),
    # 48 kHz, 3072 points: the AF = 9 edge win >= 1152, the default, the last full block, az = 10 -> 11
    Geometry("48k-win1151", 48000, "fe_kernel_r3<8,10,14,2>", output_level=2, window_width=_ms(1151, 48000), window_step=_ms(1151, 48000)),
    Geometry("48k-win1152", 48000, "fe_kernel_r3<8,10,14,2,9>", output_level=2, window_width=_ms(1152, 48000), window_step=_ms(1152, 48000)),
    Geometry("48k-default", 48000, "fe_kernel_r3<8,10,14,2,9>", output_level=2),
    Geometry("48k-win1280", 48000, "fe_kernel_r3<8,10,14,2,9>", output_level=2, window_width=_ms(1280, 48000), window_step=_ms(1280, 48000)),
    Geometry("48k-win1282", 48000, "fe_kernel_r3<8,16,14>", output_level=2, window_width=_ms(1282, 48000), window_step=_ms(1282, 48000)),
    # odd windows
    Geometry("44k1-default", 44100, "fe_kernel_r3<8,10,14,2>", output_level=2),                     # win 1103
    Geometry("22k05-default", 22050, "fe_kernel_r3<4,5,14,3>", output_level=2),                     # win 551
    Geometry("8k-default", 8000, "fe_kernel_rx<4,2,12>", output_level=2),
    # kmax == N2: the P[N2] lane-0 arm.  With linear bins nobody reads P[N2] (bands <= 256 < N2 + 1 in every family); the mel geometry below has
    # triangles narrower than a bin up to f_max = fs / 2, and its top bands interpolate between the bins N2 - 1 and N2
    Geometry("8k-nyquist-linear", 8000, "fe_kernel_rx<4,2,12>", output_level=2, f_max=4000.0, N_fft_bins=256, spec_type=2),
    Geometry("8k-nyquist-narrow", 8000, "fe_kernel_rx<4,2,12>", output_level=2, f_min=3500.0, f_max=4000.0),
    Geometry("48k-sqrt", 48000, "fe_kernel_r3<8,10,14,2,9>", output_level=2, spec_type=3, high_f_emph=0.02),
    # three bands in a lane: fe_bands_general with mel taps
    Geometry("16k-mel160", 16000, "fe_kernel_r8<4,5,8,true,4>", output_level=2, N_mel_bins=160),
    # the lowest triangles narrower than a bin (256 bands: nine of the lowest 41), and the highest bands clamped at kmax (f_max is no multiple of the bin width)
    Geometry("16k-narrow-low", 16000, "fe_kernel_r8<4,5,8,true,4>", output_level=2, N_mel_bins=256),
    Geometry("16k-clamp-kmax", 16000, "fe_kernel_r8<4,5,8,true,4>", output_level=2, f_min=3000.0, f_max=3510.0, N_fft_bins=224),
    # a gap between frames
    Geometry("16k-gap", 16000, "fe_kernel_r8<4,5,8,true,4,3>", output_level=2, window_step=30.0),
]
BY_NAME = {g.name: g for g in GEOMETRIES}
DEFAULTS = ("16k-default", "48k-default")
OVERFLOW_GEOMETRIES = ("16k-default", "48k-default", "8k-default")


class Case:
    def __init__(self, geometry, name, clip, gain=None, emph=None, tail=None, same_as=None, model=False):
        self.geometry, self.name, self.gain, self.emph = geometry, name, gain, emph
        self.clip = np.ascontiguousarray(clip, np.float32)
        self.tail = np.zeros(0, np.float32) if tail is None else np.asarray(tail, np.float32)       # behind the clip's length, inside the row's stride
        self.same_as = same_as              # name of the case of this geometry whose frames these must equal
        self.model = model                  # the device-form model runs on this case (tests/test_fe_reference.py)

    @property
    def key(self):
        return (self.gain, self.emph)


def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


def _three(g, name, frame1):
    """quiet noise, the case in frame 1, quiet noise — noise in a gap too"""
    fe = g.oracle()
    x = (_rng(g.name, name).standard_normal(fe.win + 2 * fe.hop) * QUIET).astype(np.float32)
    x[fe.hop:fe.hop + fe.win] = frame1
    return x


def _tone(fe, k, amp):
    n = np.arange(fe.win)
    return (amp * np.sin(2 * np.pi * k * n / fe.nfft)).astype(np.float32)


def _nonfinite(P):
    return np.flatnonzero(~np.isfinite(P))


def overflow_sets(g, bad):
    """bands with a non-finite bin among the PADDED taps of their fixed-length chain (inside the tap window, outside the triangle), and bands with one
    among their own taps — from k0, cnt and the instantiation's MW / MWL"""
    r, f = g.ref(), g.form()
    padded, own = [], []
    for m in range(r.bands):
        L = fe_ref.taps_of(m, f["MW"], f["MWL"]) if f["two_band"] else int(r.cnt[m])
        taps = [min(int(r.k0[m]) + j, r.kmax) for j in range(L)]
        if any(k in bad for k in taps[:int(r.cnt[m])]):
            own.append(m)
        elif any(k in bad for k in taps[int(r.cnt[m]):]):
            padded.append(m)
    return padded, own


@functools.lru_cache(maxsize=None)
def overflow_search(gname):
    """A finite tone whose power overflows fp32 in 1 .. 9 bins, none NaN, with a band of each kind of overflow_sets, and in float64 no bin within
    5 % of the largest fp32 (fp32 rounding moves a bin by 1e-6 of it) (so fe_ref and the oracle agree on which bins are infinite).  Returns (frame, gain, bad bins, padded, own)."""
    g = BY_NAME[gname]
    fe, r = g.oracle(), g.ref()
    for k in range(8, fe.kmax - 8):
        # the bin-centred tone under the Hann window: 4 |X[k]|^2 = amp^2 win^2 / 4 at the centre, 0.82 of it in the two neighbours (the frame is
        # zero padded to NFFT = 2.56 win, so the main lobe is five bins wide): 1.12 of the largest fp32 puts the centre alone over the edge
        amp = float(np.sqrt(1.12 * fe_ref.FLT_MAX * 4.0) / fe.win)
        fr = _tone(fe, k, amp)
        P = fe.power4(fr)
        bad = _nonfinite(P)
        if not (1 <= len(bad) <= 9) or np.isnan(P).any():
            continue
        P64 = r.power4(fr)
        if set(np.flatnonzero(np.isinf(P64))) != set(bad):
            continue
        fin = P64[np.isfinite(P64)]
        raw = 4.0 * np.abs(np.fft.rfft(np.concatenate([fr.astype(np.float64) * r.window, np.zeros(fe.nfft - fe.win)]))[:fe.kmax + 1]) ** 2
        if fin.max() * 1.05 > fe_ref.FLT_MAX or raw[bad].min() < 1.05 * fe_ref.FLT_MAX:
            continue
        padded, own = overflow_sets(g, set(int(b) for b in bad))
        if padded and own:
            return fr, 1e-30, bad, padded, own
    raise AssertionError(f"{gname}: no tone overflows one bin with a band of each kind")


def device_frame(g, P, gain=None, emph=None, fault=None):
    """fe_ref.device_bands of one oracle power row under the geometry's instantiation"""
    fe, r, f = g.oracle(gain, emph), g.ref(gain, emph), g.form()
    tab = None
    if r.spec_type == 1:
        off = np.concatenate([[0], np.cumsum(r.cnt)[:-1]])
        tab = (r.k0, r.cnt, off, fe.table(4))
    return fe_ref.device_bands(P, tab, r.spec_type, r.emph.astype(np.float32), np.float32(r.gain), fe.kmax, f, fault)


@functools.lru_cache(maxsize=None)
def denormal_search(gname):
    """Noise so quiet that power bins are denormal fp32 values, under gain 1e38: at least 8 non-zero bands in the oracle's frame, at least 8 bins
    denormal and not zero, and flushing denormals changes the frame (fe_ref.device_bands).  The loudest such amplitude from 1e-19 downwards."""
    g = BY_NAME[gname]
    fe = g.oracle(1e38)
    base = _rng(gname, "denormal").standard_normal(fe.win)
    for amp in 1e-19 * 10.0 ** (-np.arange(0, 17) / 16.0):
        fr = (base * amp).astype(np.float32)
        P = fe.power4(fr)
        if int(((P > 0) & (P < fe_ref.FLT_MIN)).sum()) < 8:
            continue
        out = fe.run(fr)[0]
        if int((out > 0).sum()) >= 8 and not np.array_equal(device_frame(g, P, 1e38), device_frame(g, P, 1e38, fault="flush_denormals")):
            return fr, 1e38
    raise AssertionError(f"{gname}: no amplitude leaves 8 non-zero bands with denormal powers among their bins")


@functools.lru_cache(maxsize=None)
def f8_search(gname):
    """A tone and a gain whose oracle frame holds exactly 0xffffffff with the band below it under 2^32 and not zero, a value in [2^31, 2^32), and a band
    whose real value lies in (0, 1) and is written as 0."""
    g = BY_NAME[gname]
    fe0, r0 = g.oracle(), g.ref()
    fr = _tone(fe0, 64.37, 0.4)
    for gain in 1000.0 * 2.0 ** (np.arange(0, 160) / 8.0):
        fe, r = g.oracle(float(gain)), g.ref(float(gain))
        out = fe.run(fr)[0].astype(np.int64)
        E, _, _, _ = r.frame(fr, count=False)
        sat = np.flatnonzero(out == 0xFFFFFFFF)
        edge = any(m > 0 and 0 < out[m - 1] < 0xFFFFFFFF for m in sat)
        if edge and ((out >= 2 ** 31) & (out < 0xFFFFFFFF)).any() and ((E > 0) & (E < 1) & (out == 0)).any():
            return fr, float(gain)
    raise AssertionError(f"{gname}: no gain puts a frame on all three F8 edges")


def seam_clip(g, frames):
    """noise with a distinct impulse on the first and the last frame of every wave's share (25 frames per wave, 100 per chunk)"""
    fe = g.oracle()
    x = (_rng(g.name, "seam", frames).standard_normal(fe.win + (frames - 1) * fe.hop) * 0.05).astype(np.float32)
    for f in range(frames):
        if f % 25 in (0, 24) or f == frames - 1:
            x[f * fe.hop + (7 * f + 3) % fe.win] = 0.25 + 0.5 * (f % 7) / 7.0
    return x


SEAM_FRAMES = (24, 25, 26, 99, 100, 101, 201)


@functools.lru_cache(maxsize=None)
def cases(gname):
    g = BY_NAME[gname]
    fe, f = g.oracle(), g.form()
    win, hop = fe.win, fe.hop
    out = []
    zero = np.zeros(win, np.float32)
    # ---- impulses: one sample of 1.0 (pair index and the `odd` lane, block edges, the AF blocks' edge)
    for n in sorted({0, 1, 126, 127, 128, 129, 128 * f["AF"] - 1, 128 * f["AF"], win - 2, win - 1}):
        if 0 <= n < win:
            fr = zero.copy(); fr[n] = 1.0
            out.append(Case(g, f"impulse-{n}", _three(g, f"impulse-{n}", fr), model=n in (0, win - 1)))
    # ---- spectral edges
    out.append(Case(g, "dc", _three(g, "dc", zero + 0.3)))
    out.append(Case(g, "alternating", _three(g, "alternating", 0.5 * (1 - 2 * (np.arange(win) & 1)).astype(np.float32))))
    r8 = f["R8"]
    for k in sorted({1, r8, r8 * 7, fe.kmax - 1, fe.kmax}):
        if 0 < k <= fe.kmax and k < fe.nfft // 2:
            out.append(Case(g, f"tone-{k}", _three(g, f"tone-{k}", _tone(fe, k, 0.5)), model=k in (r8, fe.kmax)))
    if f["family"] == "r3":
        for k in (fe.kmax // 2 // 3 * 3 + d for d in (0, 1, 2)):
            out.append(Case(g, f"tone-mod3-{k % 3}", _three(g, f"tone-mod3-{k % 3}", _tone(fe, k, 0.5))))
    out.append(Case(g, "square", _three(g, "square", np.where((np.arange(win) // 8) & 1, -1.0, 1.0).astype(np.float32))))
    # ---- plain noise with emphasis (the emphasis index) and the row of -0.0
    out.append(Case(g, "noise-emphasis", _three(g, "noise-emphasis", (_rng(gname, "ne").standard_normal(win) * 0.1).astype(np.float32)),
                    emph=0.013 if "high_f_emph" not in g.kw else None, model=True))
    out.append(Case(g, "minus-zero", np.full(win + 2 * hop, -0.0, np.float32)))
    # ---- a NaN sample inside the window: its frame is zeros (F8), the frames beside it are untouched
    fr = (_rng(gname, "nan").standard_normal(win) * 0.1).astype(np.float32); fr[win // 3] = np.nan
    out.append(Case(g, "nan-in-window", _three(g, "nan-in-window", fr)))
    # ---- poison outside the window: behind the clip's length, inside the row's stride, both orders; each equals the same clip with zeros there
    base = _three(g, "poison", (_rng(gname, "poison").standard_normal(win) * 0.1).astype(np.float32))
    out.append(Case(g, "poison-none", base, tail=[0.0, 0.0], model=True))
    out.append(Case(g, "poison-nan-1e30", base, tail=[np.nan, 1e30], same_as="poison-none", model=True))
    out.append(Case(g, "poison-1e30-nan", base, tail=[1e30, np.nan], same_as="poison-none"))
    if hop > win:                            # the same in the gap between frames
        clean, dirty = base.copy(), base.copy()
        for fr_i in range(2):
            clean[fr_i * hop + win:(fr_i + 1) * hop] = 0.0
            dirty[fr_i * hop + win:(fr_i + 1) * hop] = np.where(np.arange(hop - win) & 1, np.float32(1e30), np.float32(np.nan))
        out.append(Case(g, "gap-zero", clean))
        out.append(Case(g, "gap-poison", dirty, same_as="gap-zero"))
    # ---- one bin overflows
    if gname in OVERFLOW_GEOMETRIES:
        fr, gain, _, _, _ = overflow_search(gname)
        out.append(Case(g, "overflow-one-bin", _three(g, "overflow-one-bin", fr), gain=gain, model=True))
    if gname in DEFAULTS:
        # ---- denormal intermediates
        fr, gain = denormal_search(gname)
        out.append(Case(g, "denormal", _three(g, "denormal", fr), gain=gain, model=True))
        # ---- F8 edges
        fr, gain = f8_search(gname)
        out.append(Case(g, "f8-edges", _three(g, "f8-edges", fr), gain=gain, model=True))
        # ---- wave and chunk seams
        for n in SEAM_FRAMES:
            out.append(Case(g, f"seam-{n}", seam_clip(g, n)))
    return out


def expected(case):
    """the oracle's u32 frames of the case"""
    return case.geometry.oracle(case.gain, case.emph).run(case.clip)

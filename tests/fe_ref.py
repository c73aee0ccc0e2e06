"""A plain float64 statement of the front-end specification FE-1, F1-F8, and a small model of the DEVICE FORMS of K1
(csrc/fe_r8.hip, fe_rx.hip, fe_r3.hip) with selectable one-line faults.

Part 1, `FeRef`, shares no structure with oracle/frontend.c: numpy.fft.rfft of the zero-padded frame under the fp32-rounded Hann window, the mel
triangles rebuilt from f_min, f_max, N_mel_bins and the DESIGN text (unit peak, the strict lo < f_k < hi rule, the narrower-than-a-bin rule with its
k0 >= kmax clamp and its fr == 0 arm), linear and square-root bins, emphasis fl32(1 + m high_f_emph), gain fl32(pre_norm_gain), and F8.  Every value
stays a real number except where FE-1 names a number format's RANGE: a power bin, a band sum or a product beyond the largest fp32 is +Inf, as the
fp32 operation gives it (the cases keep clear of that edge by a factor; fe_cases asserts it).  FE_ARMS counts each side of every comparison.

Part 2, `device_bands`, works on the ORACLE's own fp32 power rows (pyoracle.FrontEnd.power4) and restates what the kernels do differently from the
oracle's loop on the way from P to the u32 frame; `device_frame_input` restates what they do differently on the way from the clip to the windowed
frame (the caller feeds the result to the oracle's own transform); `split_partner_bins` with `FeRef.power4_split` restates the real split's pairing.
Each fault is one line.  The model takes no kernel output.
"""
import collections

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)

FE_ARMS = collections.Counter()
ARM_NAMES = (
    "tri_fk_gt_lo", "tri_fk_le_lo", "tri_fk_lt_hi", "tri_fk_ge_hi", "tri_up_lt_dn", "tri_up_ge_dn",          # F5 triangle: lo < f_k < hi, min(up, dn)
    "band_has_bins", "band_is_narrow", "narrow_clamped_at_kmax", "narrow_not_clamped", "narrow_fr_zero", "narrow_fr_positive",
    "spec_mel", "spec_linear", "spec_sqrt",
    "f8_not_positive", "f8_nan", "f8_saturate", "f8_truncate",
)
FAULTS = ("padded_tap_multiplies", "flush_denormals", "window_by_multiply", "odd_last_sample_dropped", "saturate_at_2_31", "emph_index_off_by_one",
          "taps_lo_3", "lane0_partner")


def geometry(fs, window_width=25.0, window_step=25.0, n_fft_bins=256, f_max=4000.0, **_):
    """F1, F2: win, hop, NFFT"""
    win = int(np.floor(fs * window_width / 1000.0 + 0.5))
    hop = int(np.floor(fs * window_step / 1000.0 + 0.5))
    need = max(win, int(np.ceil(fs * n_fft_bins / f_max)))
    n = 256
    while True:
        if n >= need:
            nfft = n
            break
        if n // 2 * 3 >= need:
            nfft = n // 2 * 3
            break
        n *= 2
    return win, hop, nfft


def _range32(x):
    """a real number as the fp32 RANGE holds it: beyond the largest finite value it is an infinity"""
    x = np.asarray(x, np.float64).copy()
    big = np.abs(x) > FLT_MAX
    x[big] = np.sign(x[big]) * np.inf
    return x


class FeRef:
    def __init__(self, fs=16000.0, spec_type=1, f_min=50.0, f_max=4000.0, n_fft_bins=256, n_mel_bins=128, window_width=25.0, window_step=25.0,
                 pre_norm_gain=1000.0, high_f_emph=0.0):
        self.fs, self.spec_type = float(fs), int(spec_type)
        self.win, self.hop, self.nfft = geometry(fs, window_width, window_step, n_fft_bins, f_max)
        self.n2 = self.nfft // 2
        self.kmax = min(int(np.floor(f_max * self.nfft / fs)), self.n2)
        self.bands = n_mel_bins if spec_type == 1 else n_fft_bins
        n = np.arange(self.win)
        self.window = (0.5 - 0.5 * np.cos(2 * np.pi * n / self.win)).astype(np.float32).astype(np.float64)                 # F3, rounded once
        self.emph = (1.0 + np.arange(self.bands) * float(high_f_emph)).astype(np.float32).astype(np.float64)                # F6
        self.gain = float(np.float32(pre_norm_gain))                                                                          # F7
        self.k0 = np.zeros(self.bands, np.int64)
        self.cnt = np.zeros(self.bands, np.int64)
        self.weights = []                                       # per band: the float64 weights of bins k0 .. k0 + cnt - 1, 0.25 folded in
        self.narrow = np.zeros(self.bands, bool)
        self.clamped = np.zeros(self.bands, bool)
        if self.spec_type == 1:
            self._triangles(float(f_min), float(f_max))
        else:
            for m in range(self.bands):
                self.k0[m], self.cnt[m] = m, 1
                self.weights.append(np.array([0.25]))

    def _triangles(self, f_min, f_max):
        """F5: HTK-mel triangles, unit peak, sampled at the bin centres f_k = k fs / NFFT, k = 0 .. kmax"""
        mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
        hz = lambda m: 700.0 * (np.power(10.0, m / 2595.0) - 1.0)
        M, df = self.bands, self.fs / self.nfft
        edges = hz(np.linspace(mel(f_min), mel(f_max), M + 2))
        fk = np.arange(self.kmax + 1) * df
        for m in range(M):
            lo, ce, hi = edges[m], edges[m + 1], edges[m + 2]
            w = np.zeros(self.kmax + 1)
            for k in range(self.kmax + 1):
                above = fk[k] > lo
                FE_ARMS["tri_fk_gt_lo" if above else "tri_fk_le_lo"] += 1
                if not above:
                    continue
                below = fk[k] < hi
                FE_ARMS["tri_fk_lt_hi" if below else "tri_fk_ge_hi"] += 1
                if not below:
                    continue
                up, dn = (fk[k] - lo) / (ce - lo), (hi - fk[k]) / (hi - ce)
                FE_ARMS["tri_up_lt_dn" if up < dn else "tri_up_ge_dn"] += 1
                w[k] = min(up, dn)
            inside = np.flatnonzero(w > 0)
            if len(inside):
                FE_ARMS["band_has_bins"] += 1
                self.k0[m], self.cnt[m] = inside[0], inside[-1] - inside[0] + 1
                self.weights.append(0.25 * w[inside[0]:inside[-1] + 1])
                continue
            FE_ARMS["band_is_narrow"] += 1                      # no bin centre strictly inside: the linearly interpolated power at the centre
            self.narrow[m] = True
            pos = ce / df
            k0 = int(np.floor(pos))
            fr = pos - k0
            if k0 >= self.kmax:
                FE_ARMS["narrow_clamped_at_kmax"] += 1
                self.clamped[m] = True
                k0, fr = self.kmax, 0.0
            else:
                FE_ARMS["narrow_not_clamped"] += 1
            FE_ARMS["narrow_fr_positive" if fr > 0 else "narrow_fr_zero"] += 1
            self.k0[m] = k0
            if fr > 0:
                self.cnt[m] = 2
                self.weights.append(0.25 * np.array([1.0 - fr, fr]))
            else:
                self.cnt[m] = 1
                self.weights.append(0.25 * np.array([1.0]))

    def n_frames(self, n):
        return 0 if n < self.win else (n - self.win) // self.hop + 1

    def power4(self, frame):
        """F1-F4: 4 |X[k]|^2, k = 0 .. kmax, of one frame (samples behind the window are not read)"""
        x = np.zeros(self.nfft)
        x[:self.win] = np.asarray(frame[:self.win], np.float64) * self.window
        with np.errstate(all="ignore"):
            X = np.fft.rfft(x)[:self.kmax + 1]
            return _range32(4.0 * (X.real * X.real + X.imag * X.imag))

    def power4_split(self, frame, partner):
        """the same through the packed transform the kernels run: z[n] = x[2n] + i x[2n + 1], Z = DFT_N2(z), 2 X[k] = (Z[k] + Z*[p]) - i W^k (Z[k] - Z*[p]) with
        p = partner[k] (N2 - k in FE-1: split_partner_bins)"""
        x = np.zeros(self.nfft)
        x[:self.win] = np.asarray(frame[:self.win], np.float64) * self.window
        with np.errstate(all="ignore"):
            Z = np.fft.fft(x[0::2] + 1j * x[1::2])
            k = np.arange(self.kmax + 1)
            za, zb = Z[k % self.n2], np.conj(Z[np.array([partner[i] for i in k])])
            X2 = (za + zb) - 1j * np.exp(-2j * np.pi * k / self.nfft) * (za - zb)
            return _range32(X2.real * X2.real + X2.imag * X2.imag)

    def frame_from_power(self, P):
        """F5-F8 on a float64 power row"""
        E, _ = self.band_sums(P)
        with np.errstate(all="ignore"):
            if self.spec_type == 3:
                E = np.sqrt(E)
            E = _range32(_range32(E * self.emph) * self.gain)
        return f8(E, count=False)

    def band_sums(self, P):
        """F5 for one power row: (sum_k w[m][k] P[k], sum_k w[m][k]) per band, the 0.25 inside w"""
        E, sw = np.zeros(self.bands), np.zeros(self.bands)
        with np.errstate(all="ignore"):
            for m in range(self.bands):
                w = self.weights[m]
                E[m] = float(np.sum(w * P[self.k0[m]:self.k0[m] + self.cnt[m]]))
                sw[m] = float(np.sum(w))
        return _range32(E), sw

    def frame(self, frame, count=True):
        """one frame: E64[m] (real valued; +Inf / NaN where FE-1's fp32 range gives them), the u32 FE-1 asks for, sum of weights, max P64"""
        P = self.power4(frame)
        E, sw = self.band_sums(P)
        with np.errstate(all="ignore"):
            if self.spec_type == 3:
                E = np.sqrt(E)
                if count:
                    FE_ARMS["spec_sqrt"] += self.bands
            elif count:
                FE_ARMS["spec_mel" if self.spec_type == 1 else "spec_linear"] += self.bands
            E = _range32(_range32(E * self.emph) * self.gain)
        return E, f8(E, count), sw, P

    def run(self, pcm):
        nf = self.n_frames(len(pcm))
        out = [self.frame(pcm[f * self.hop:f * self.hop + self.win]) for f in range(nf)]
        return out


def f8(E, count=True):
    """F8 on real values: !(x > 0) -> 0 (NaN among them), x >= 2^32 -> 0xffffffff, else truncate"""
    E = np.asarray(E, np.float64)
    out = np.zeros(E.shape, np.uint32)
    with np.errstate(all="ignore"):
        nan = np.isnan(E)
        notpos = ~(E > 0)
        sat = E >= 4294967296.0
    tr = ~notpos & ~sat
    out[sat] = 0xFFFFFFFF
    out[tr] = np.floor(E[tr]).astype(np.uint64).astype(np.uint32)
    if count:
        FE_ARMS["f8_nan"] += int(nan.sum())
        FE_ARMS["f8_not_positive"] += int((notpos & ~nan).sum())
        FE_ARMS["f8_saturate"] += int(sat.sum())
        FE_ARMS["f8_truncate"] += int(tr.sum())
    return out


# =====================================================================================================================================================
# Part 2: the device forms.

def fmaf32(a, b, c):
    """fl32(a b + c) for fp32 arrays, one rounding: the product of two fp32 values is exact in fp64; the sum is rounded to odd in fp64 (TwoSum gives the
    discarded part) and then once to fp32, which equals the single rounding because fp64 carries more than 2 * 24 + 2 bits"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def _ftz(x):
    x = np.asarray(x, np.float32).copy()
    x[np.abs(x) < np.float32(FLT_MIN)] = 0
    return x


def f8_device(e, fault=None):
    """v_cvt_u32_f32 on fp32 values: round toward zero, clamp to [0, 2^32 - 1], NaN -> 0"""
    e = np.asarray(e, np.float32).astype(np.float64)
    top = 2147483648.0 if fault == "saturate_at_2_31" else 4294967296.0
    out = np.zeros(e.shape, np.uint32)
    with np.errstate(all="ignore"):
        pos = e > 0
        sat = e >= top
    out[pos & ~sat] = np.floor(e[pos & ~sat]).astype(np.uint64).astype(np.uint32)
    out[sat] = 0xFFFFFFFF if fault != "saturate_at_2_31" else 0x7FFFFFFF
    return out


def taps_of(m, mw, mwl):
    """taps the two-band form multiplies for band m: MWL for a lane's lower band (m < 64) in the 1024-point kernels, MW otherwise"""
    return mwl if m < 64 else mw


def device_bands(P, tab, spec_type, emph, gain, kmax, form, fault=None):
    """One fp32 power row (the oracle's) -> u32 frame as a kernel forms it.  tab = (k0, cnt, off, w) the oracle's mel table (table(4) and fe_ref's k0 /
    cnt, which the CPU test holds equal to the oracle's); form = dict(two_band=bool, MW=int, MWL=int): the two-band form runs a chain of FIXED length
    over the band's taps — a tap j >= cnt is padding and must leave e alone whatever P holds —, the general form runs exactly cnt taps."""
    P = np.asarray(P, np.float32)
    if fault == "flush_denormals":
        P = _ftz(P)
    bands = len(emph)
    e = np.zeros(bands, np.float32)
    with np.errstate(all="ignore"):
        if spec_type == 1:
            k0, cnt, off, w = tab
            for m in range(bands):
                n = int(cnt[m])
                acc = np.float32(0)
                if form["two_band"]:
                    length = taps_of(m, form["MW"], form["MWL"])
                    if fault == "taps_lo_3" and m < 64:
                        length -= 1
                    for j in range(length):
                        wj = w[off[m] + j] if j < n else np.float32(0)
                        pj = P[min(k0[m] + j, kmax)]
                        if j < n or fault == "padded_tap_multiplies":
                            acc = fmaf32(wj, pj, acc)                      # padded_tap_multiplies: fmaf(0, P, e) is e only while P is finite
                else:
                    for j in range(n):
                        acc = fmaf32(w[off[m] + j], P[k0[m] + j], acc)
                e[m] = acc
        else:
            e = (np.float32(0.25) * P[:bands]).astype(np.float32)
            if spec_type == 3:
                e = np.sqrt(e).astype(np.float32)
        if fault == "flush_denormals":
            e = _ftz(e)
        em = np.asarray(emph, np.float32)
        if fault == "emph_index_off_by_one":
            em = np.concatenate([em[1:], em[-1:]])
        e = (e * em).astype(np.float32)
        if fault == "flush_denormals":
            e = _ftz(e)
        e = (e * np.float32(gain)).astype(np.float32)
        if fault == "flush_denormals":
            e = _ftz(e)
    return f8_device(e, fault)


def device_frame_input(row, start, win, fault=None):
    """What a kernel's lanes hand to the window multiply for the frame at `start` of the clip row.  Lanes read 8-byte PAIRS (n, n + 1), n even, the pair
    index clamped to win - 2, so no lane reads behind the window whatever the row holds there; samples at n >= win are replaced by 0 by a select; the
    lane that owns the last sample of an odd window (n = win - 1) finds it in the clamped pair's second half.  Returns (x[0 .. win - 1], behind): behind
    = what entered the transform at the two positions n >= win of the window's last pair(s) — zeros, unless a fault lets something through (a NaN there
    poisons every bin).  window_by_multiply: the clamped pair times the window's 0 instead of the select, which is 0 unless the pair holds an infinity."""
    row = np.asarray(row, np.float32)
    x = np.zeros(win + 3, np.float32)
    with np.errstate(all="ignore"):
        for n in range(0, win + 2, 2):
            idx = max(min(n, win - 2), 0)
            a, b = row[start + idx], row[start + idx + 1]
            odd = n == win - 1
            first = (np.float32(0) if fault == "odd_last_sample_dropped" else b) if odd else a
            if fault == "window_by_multiply":
                lo = first if n < win else first * np.float32(0)
                hi = b if n + 1 < win else b * np.float32(0)
            else:
                lo = first if n < win else np.float32(0)
                hi = b if n + 1 < win else np.float32(0)
            x[n], x[n + 1] = lo, hi
    return x[:win].copy(), x[win:win + 2].copy()


def device_frame_is_clean(behind):
    """the positions behind the window entered the transform as zeros"""
    return bool(np.all(behind == 0))


def split_partner_bins(kmax, n2, R8, fault=None):
    """For every bin k <= kmax the bin whose conjugate the real split pairs it with: N2 - k, and 0 with itself.  Lane 0 of the general families holds the
    bins k = 8R c; their partners sit in the lane's own registers ((8 - c) & 7), not in the partner lane's register 7 - c as for every other lane:
    lane0_partner pairs them as the other lanes are, i.e. k = 8R c with 8R (7 - c)."""
    out = {}
    for k in range(kmax + 1):
        pk = (n2 - k) % n2
        if fault == "lane0_partner" and k % R8 == 0 and k < n2:
            pk = R8 * (7 - k // R8)
        out[k] = pk
    return out

"""The host bookkeeping of a mixed stream set (include/wsa.h, wsa_stream_create_mixed) restated in plain Python, for the tests: which
outputs of RS-1 are ready after N input samples, what a step of a given input count produces, the paced counts, and the feeds the tests use.
Python floats are IEEE doubles, so `n * ratio` here is the product oracle/resample.c and the library form."""
import math

import numpy as np

RS_HALF = 16          # RS-1 reads 16 samples on either side of floor(pos)
RATES = [8000, 11025, 16000, 22050, 24414, 32000, 44100, 96000]


def resample_length(n_in, fs_in, fs_out):
    return int(n_in / (fs_in / fs_out))


def tap_ready(n, n_in, ratio):
    return math.floor(n * ratio) + RS_HALF <= n_in


def ready(n_in, fs_in, fs_out):
    """Outputs whose taps have all arrived, never more than the batch's length; n_in at equal rates."""
    if fs_in == fs_out:
        return n_in
    ratio = fs_in / fs_out
    if n_in < RS_HALF:
        return 0
    g = int((n_in - RS_HALF) / ratio)
    while g > 0 and not tap_ready(g - 1, n_in, ratio):
        g -= 1
    while tap_ready(g, n_in, ratio):
        g += 1
    return min(g, resample_length(n_in, fs_in, fs_out))


def capacity(fs_in, fs_out, frames_per_step, hop):
    return frames_per_step * hop if fs_in == fs_out else math.ceil(frames_per_step * hop * (fs_in / fs_out))


class Book:
    """One stream's counts since START: N inputs, Y outputs, K frames, S active steps."""

    def __init__(self, fs_in, fs_out, frames_per_step, win, hop):
        self.fs_in, self.fs_out, self.F, self.win, self.hop = float(fs_in), float(fs_out), frames_per_step, win, hop
        self.ratio = self.fs_in / self.fs_out
        self.cap = capacity(self.fs_in, self.fs_out, frames_per_step, hop)
        self.N = self.Y = self.K = self.S = 0
        self.max_history = 0

    def paced(self):
        b = self.F * self.hop
        if self.fs_in == self.fs_out:
            return b
        return math.floor((self.S + 1) * b * self.ratio) - math.floor(self.S * b * self.ratio)

    def step(self, count=None, stop=False):
        """-> (outputs, frames) of the step; count None = paced"""
        count = self.paced() if count is None else int(count)
        assert 0 <= count <= self.cap
        n0, y0, k0 = self.N, self.Y, self.K
        self.N += count
        self.Y = max(y0, resample_length(self.N, self.fs_in, self.fs_out) if stop else ready(self.N, self.fs_in, self.fs_out))
        if self.fs_in == self.fs_out:
            self.Y = self.N
        self.K = (self.Y - self.win) // self.hop + 1 if self.Y >= self.win else 0
        self.S += 1
        if self.Y > y0 and self.fs_in != self.fs_out:       # input history the step's oldest tap reaches back into
            self.max_history = max(self.max_history, n0 - (math.floor(y0 * self.ratio) - RS_HALF))
        return self.Y - y0, self.K - k0


def feed_counts(kind, book, total, rng=None):
    """The input counts of every step until `total` samples are delivered: 'paced', 'capacity' (the capacity every step) or 'random'
    (uniform in [0, capacity], zeros included).  The caller runs them through `book` (or a stream set) itself; the last count is cut to fit."""
    probe = Book(book.fs_in, book.fs_out, book.F, book.win, book.hop)
    left, out = int(total), []
    while left > 0:
        if kind == "paced":
            c = probe.paced()
        elif kind == "capacity":
            c = probe.cap
        else:
            c = int(rng.integers(0, probe.cap + 1))
            if len(out) % 7 == 3:
                c = 0
        c = min(c, left)
        probe.step(c)
        out.append(c)
        left -= c
    return out


def chunks(x, counts):
    pos, out = 0, []
    for c in counts:
        out.append(np.asarray(x[pos:pos + c]))
        pos += c
    return out

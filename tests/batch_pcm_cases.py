"""Spec PK-2's test inputs, shared by tests/test_batch_pcm_host.py and tests/test_gpu_batch_pcm.py: the edge values of every format, hashed
values, numpy's statement of each format's rule, a bit-for-bit comparison, and an encoder from float clips to each format's samples."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ["f32", "i16", "mulaw", "alaw", "u8", "i24", "i32", "f64"]
SAMPLE_BYTES = {"f32": 4, "i16": 2, "mulaw": 1, "alaw": 1, "u8": 1, "i24": 3, "i32": 4, "f64": 8}
DTYPE = {"f32": np.float32, "i16": np.int16, "mulaw": np.uint8, "alaw": np.uint8, "u8": np.uint8, "i24": np.uint8, "i32": np.int32, "f64": np.float64}


def hashed(n, seed):
    """n 32-bit values from an integer hash (lowbias32 over a counter)"""
    x = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)
    for shift, mul in ((16, 0x7FEB352D), (15, 0x846CA68B)):
        x ^= x >> np.uint64(shift)
        x = (x * np.uint64(mul)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def i24_bytes(values):
    v = np.asarray(values, np.int64) & 0xFFFFFF
    return np.stack([v & 0xFF, (v >> 8) & 0xFF, v >> 16], axis=1).astype(np.uint8).reshape(-1)


def i24_values():
    edge = np.array([0x000000, 0x000001, 0x7FFFFF, 0x800000, 0xFFFFFF, 0x800001], np.int64)
    return np.concatenate([edge, (hashed(4096, 24) >> np.uint32(8)).astype(np.int64)])


def i32_values():
    edge = [-2**31, 2**31 - 1, 2**24 + 1, -(2**24 + 1), 2**24 + 3, 2**25 + 2, 2**25 + 6, 2**31 - 64, 2**31 - 65, 2**31 - 128, 2**31 - 129, 0, 1, -1]
    return np.concatenate([np.array(edge, np.int64).astype(np.int32), hashed(4096, 32).view(np.int32)])


def f64_values(with_nan=True):
    edge = [1e-40, 1e-46, 3e38, 3.5e38, -0.0, 1 + 2.0**-24, 1 + 3 * 2.0**-24, np.inf, -np.inf] + ([np.nan] if with_nan else [])
    h = hashed(8192, 64).astype(np.float64)
    inside = (h[0::2] * 2.0**32 + h[1::2]) / 2.0**63 - 1.0            # (-1, 1), all 53 bits in use
    inside = inside[np.abs(inside) < 1.0]
    return np.concatenate([np.array(edge, np.float64), inside, inside[:512] * 1e-39, inside[:512] * 1e-44])


def reference(fmt, raw):
    """numpy's statement of the format's rule for mono samples, float32"""
    if fmt == "u8":
        return ((raw.astype(np.float64) - 128.0) / 128.0).astype(np.float32)
    if fmt == "i24":
        b = raw.reshape(-1, 3).astype(np.int64)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 0x800000, v - 0x1000000, v)
        return (v.astype(np.float64) / 2.0**23).astype(np.float32)
    if fmt == "i32":
        return (raw.astype(np.float64) / 2.0**31).astype(np.float32)
    if fmt == "f64":
        with np.errstate(over="ignore"):
            return raw.astype(np.float32)
    if fmt == "f32":
        return raw.copy()
    if fmt == "i16":
        return (raw.astype(np.float64) / 32768.0).astype(np.float32)
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "g711_expected.json")))
    return (np.asarray(gold[fmt], np.float64)[raw] / 32768.0).astype(np.float32)


def same_bits(got, want):
    """bit for bit, NaN compared as NaN (its payload is unspecified)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def samples(fmt, n, seed):
    """n samples of a format as the array pcm_decode takes (edge values first, tiled)"""
    if fmt == "u8" or fmt in ("mulaw", "alaw"):
        return np.resize(np.arange(256, dtype=np.uint8), n)
    if fmt == "i24":
        return i24_bytes(np.resize(i24_values(), n))
    if fmt == "i32":
        return np.resize(i32_values(), n)
    if fmt == "f64":
        return np.resize(f64_values(), n)
    if fmt == "i16":
        return np.resize(np.array([-32768, 32767, 0, 1, -1, 12345, -12345], np.int16), n)
    return np.resize(np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, 1e-40, np.inf], np.float32), hashed(64, seed).view(np.float32)]), n)


def _g711_encode(x, law):
    """the code whose table value is nearest to x * 32768"""
    table = np.asarray(json.load(open(os.path.join(ROOT, "tests", "golden", "g711_expected.json")))[law], np.float64)
    order = np.argsort(table, kind="stable")
    t = table[order]
    v = np.clip(np.asarray(x, np.float64) * 32768.0, t[0], t[-1])
    hi = np.clip(np.searchsorted(t, v), 1, len(t) - 1)
    pick = np.where(v - t[hi - 1] <= t[hi] - v, hi - 1, hi)
    return order[pick].astype(np.uint8)


def encode(x, fmt, channels, seed):
    """float clip x -> the interleaved samples a file of that encoding would hold (as pcm_decode takes them); channel 0 is x, the others noise"""
    x = np.clip(np.asarray(x, np.float64), -1.0, 1.0)
    rng = np.random.default_rng(seed)
    cols = [x] + [np.clip(x[::-1] * 0.5 + rng.uniform(-0.2, 0.2, len(x)), -1, 1) for _ in range(channels - 1)]
    enc = []
    for v in cols:
        if fmt == "f32":
            e = v.astype(np.float32).view(np.uint8)
        elif fmt == "i16":
            e = np.round(v * 32767).astype("<i2").view(np.uint8)
        elif fmt in ("mulaw", "alaw"):
            e = _g711_encode(v, fmt)
        elif fmt == "u8":
            e = np.round(v * 127 + 128).astype(np.uint8)
        elif fmt == "i24":
            q = np.round(v * 8388607).astype(np.int64) & 0xFFFFFF
            e = np.stack([q & 0xFF, (q >> 8) & 0xFF, q >> 16], axis=1).astype(np.uint8).reshape(-1)
        elif fmt == "i32":
            e = np.round(v * 2147483647).astype("<i4").view(np.uint8)
        else:
            e = (v * (1.0 + 2.0**-30)).astype("<f8").view(np.uint8)            # doubles that are no floats
        enc.append(e.reshape(len(x), SAMPLE_BYTES[fmt]))
    return np.stack(enc, axis=1).reshape(-1).view(DTYPE[fmt]).copy()

"""K6 (csrc/classify.hip classify_tile) restated literally on the CPU (test helper).

mfma_f32_16x16x4f32 is a k-ordered f32 fmaf chain with one rounding per product, and K6 feeds it K ascending from a zero accumulator, adds
the bias with a rounding of its own and then applies the activation.  So a network whose activations are linear or relu has exactly one
possible output, and `forward_bits` computes it: the normalisation in float64 rounded to f32, oracle/dense.c's wsa_or_dense_f32 over the
layers padded as wsa_model_create pads them, relu as `v < 0 ? 0 : v`, the padded columns of every layer but the last zeroed.
`forward64` is classify_ref.forward opened up (it can stop before an activation, start from given pre-activations, and run in numpy
float32 throughout: the twin whose distance D32 gives the tolerance cases their bound).  ARMS counts what the cases reach, FAULTS names
the wrong variants of this restatement that tests/test_k6_reference.py must be able to tell from the right one."""
import ctypes
from collections import Counter

import numpy as np

from oracle import pyoracle

ARM_NAMES = ("pad_k.input", "pad_col.nonzero_act", "row.past_n", "relu.negative", "relu.neg_zero", "relu.nan", "fmax.nan_skipped",
             "softmax.m_inf", "nan_slot.set", "nan_slot.clear", "range0.inf", "range0.nan", "wg.second_tile", "group.fell_through")
ARMS = Counter()

# the restatement's wrong variants (tests/test_k6_reference.py): what they change, in the kernel's words
FAULTS = ("k_block_short",        # the K loop ends one block of 16 early
          "col_block_skipped",    # a wave takes one column block only: blocks past the wave count (8) are never computed
          "pad_cols_kept",        # `if (col >= L.n && !last) v = 0` dropped
          "k_guard",              # `k < p.nin` dropped: a padded k reads on into the next row
          "row_guard",            # `row0 + r < n` -> `<=`
          "no_max",               # softmax without the max subtraction
          "fused_epilogue",       # unnormalise_value contracted into one fma
          "k_descending", "pairs", "bias_first",      # the chain's order (oracle/dense.c)
          "tile_kept")            # `tile -= t` dropped in K6e's walk
_ORDER = {"k_descending": 1, "pairs": 2, "bias_first": 3}
CLS_WAVES = 8
LDS_BUDGET = 160 * 1024
SEED_F32, SEED_F64 = np.uint32(0xffc0beef), np.uint64(0xfff8beef0000beef)      # capi.DEBUG_CLASSIFY_SEED_*
QNAN_F32, QNAN_F64 = np.uint32(0x7fc00000), np.uint64(0x7ff8000000000000)


def _lib():
    L = pyoracle.lib()
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    L.wsa_or_dense_f32_order.argtypes = [vp, vp, vp, u32, u32, u32, i32, vp]
    L.wsa_or_dense_f32_order.restype = None
    L.wsa_or_dense_f32.argtypes = [vp, vp, vp, u32, u32, u32, vp]
    L.wsa_or_dense_f32.restype = None
    L.wsa_or_unnormalise.argtypes = [ctypes.c_float, ctypes.c_double, ctypes.c_double, i32]
    L.wsa_or_unnormalise.restype = ctypes.c_double
    return L


def pad16(n):
    return (n + 15) & ~15


def row_blocks(units):
    """the row-block factor wsa_model_create gives the widths: S = pad64(widest padded layer) + 4 floats, two buffers of 16 RB rows"""
    S = ((max(pad16(u) for u in units) + 63) & ~63) + 4
    rb = 4
    while rb > 1 and 2 * 16 * rb * S * 4 > LDS_BUDGET:
        rb >>= 1
    return rb


def padded(spec):
    """[(w [kp, np], b [np])] zero padded to 16-column blocks, as wsa_model_create uploads them"""
    out = []
    for l, (k, b) in enumerate(zip(spec.kernels, spec.biases)):
        K, N = spec.units[l], spec.units[l + 1]
        w = np.zeros((pad16(K), pad16(N)), np.float32)
        w[:K, :N] = k
        bb = np.zeros(pad16(N), np.float32)
        bb[:N] = b
        out.append((w, bb))
    return out


def dense(a, w, b, order=0):
    a, w, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)
    out = np.empty((a.shape[0], w.shape[1]), np.float32)
    assert a.shape[1] == w.shape[0] and b.shape[0] == w.shape[1]
    if order == 0:
        _lib().wsa_or_dense_f32(a.ctypes.data, w.ctypes.data, b.ctypes.data, a.shape[0], w.shape[0], w.shape[1], out.ctypes.data)
    else:
        _lib().wsa_or_dense_f32_order(a.ctypes.data, w.ctypes.data, b.ctypes.data, a.shape[0], w.shape[0], w.shape[1], order, out.ctypes.data)
    return out


def normalise(spec, feat):
    """ml5 normalizeValue in double, then the f32 tensor: [rows, nin] f32 of feat [rows, stride >= nin]"""
    nin = spec.units[0]
    x = np.asarray(feat, np.float64)[:, :nin]
    lo, hi = np.asarray(spec.in_min, np.float64), np.asarray(spec.in_max, np.float64)
    with np.errstate(all="ignore"):
        v = ((x - lo) / (hi - lo)).astype(np.float32)
    flat = hi == lo
    if flat.any():
        ARMS["range0.inf"] += int(np.isinf(v[:, flat]).sum())
        ARMS["range0.nan"] += int(np.isnan(v[:, flat]).sum())
    return v


def _relu(v):
    ARMS["relu.negative"] += int((v < 0).sum())
    ARMS["relu.neg_zero"] += int(((v == 0) & np.signbit(v)).sum())
    ARMS["relu.nan"] += int(np.isnan(v).sum())
    return np.where(v < 0, np.float32(0), v)            # `v < 0.f ? 0.f : v`: -0 and NaN pass


def _act64(z, a, dtype):
    with np.errstate(all="ignore"):
        if a == "relu":
            return np.where(z < 0, dtype(0), z)
        if a == "sigmoid":
            return (dtype(1) / (dtype(1) + np.exp(-z))).astype(dtype)
        if a == "tanh":
            return np.tanh(z).astype(dtype)
        if a == "softmax":
            return softmax(z, dtype)
    return z


def softmax(x, dtype=np.float64, fault=None, count=False):
    """K6's softmax, step for step, in `dtype`: m = x[0], then fmaxf over the rest (fmaxf returns the other operand beside a NaN);
    exp(x - (m + log(sum exp(x - m))))"""
    x = np.asarray(x).astype(dtype)
    with np.errstate(all="ignore"):
        m = x[:, 0].copy()
        skipped = 0
        for c in range(1, x.shape[1]):
            skipped += int((np.isnan(m) != np.isnan(x[:, c])).sum())
            m = np.fmax(m, x[:, c])
        if count:
            ARMS["fmax.nan_skipped"] += skipped
            ARMS["softmax.m_inf"] += int((m == np.inf).sum())
        if fault == "no_max":
            m = np.zeros_like(m)
        s = np.zeros_like(m)
        for c in range(x.shape[1]):
            s = (s + np.exp(x[:, c] - m)).astype(dtype)
        lse = (m + np.log(s)).astype(dtype)
        return np.exp(x - lse[:, None]).astype(dtype)


def forward_bits(spec, feat, fault=None, upto=None):
    """The network as K6 computes it, every row of feat [rows, stride]: {"pre": the pre-activation f32 values [rows, np] of every layer (padded
    columns included, before they are zeroed), "out": the last layer's values [rows, C] after its activation — softmax excepted, whose
    logits these are}.  Exact for hidden and last activations relu / linear; anything else is refused.  upto: stop after that layer."""
    nin = spec.units[0]
    x = normalise(spec, feat)
    kp0 = pad16(nin)
    a = np.zeros((len(x), kp0), np.float32)
    a[:, :nin] = x
    ARMS["pad_k.input"] += (kp0 - nin) * len(x)
    if fault == "k_guard":                                # the padded k of row r: the doubles behind its nin features, converted with range 0 .. 1
        flat = np.concatenate([np.asarray(feat, np.float64).ravel(), np.zeros(kp0)])
        stride = np.asarray(feat).shape[1]
        with np.errstate(all="ignore"):
            for r in range(len(x)):
                a[r, nin:] = flat[r * stride + nin:r * stride + kp0].astype(np.float32)
    pre = []
    nl = len(spec.kernels)
    for l, (w, b) in enumerate(padded(spec)):
        act, last = spec.activations[l], l == nl - 1
        if act not in ("relu", "linear") and not (last and act == "softmax"):
            raise ValueError(f"forward_bits: layer {l} is {act}")
        aa, ww = a, w
        if fault == "k_block_short" and w.shape[0] > 16:
            aa, ww = a[:, :-16], w[:-16]
        z = dense(aa, ww, b, _ORDER.get(fault, 0))
        if fault == "col_block_skipped":
            z[:, 16 * CLS_WAVES:] = 0
        pre.append(z)
        v = _relu(z) if act == "relu" else z
        if not last and fault != "pad_cols_kept":
            v = v.copy()
            v[:, spec.units[l + 1]:] = 0
        a = v
        if upto == l:
            break
    return dict(pre=pre, out=a[:, :spec.units[len(pre)]])


def forward64(spec, feat, upto=None, dtype=np.float64, start=None):
    """classify_ref.forward opened up: the normalised f32 tensor, then act(x W + b) per layer in `dtype` (float64, or numpy float32
    arithmetic throughout: the twin) with the f32 weights.  upto = l: returns layer l's pre-activation values.  start = (l, z): begins
    with z as layer l's pre-activation values (the device's own).  Hidden sigmoid layers count their padded columns' arm."""
    x = None if start is not None else normalise(spec, feat).astype(dtype)
    for l, (k, b, a) in enumerate(zip(spec.kernels, spec.biases, spec.activations)):
        if start is not None and l < start[0]:
            continue
        if start is not None and l == start[0]:
            z = np.asarray(start[1]).astype(dtype)
        else:
            with np.errstate(all="ignore"):
                z = (x @ k.astype(dtype) + b.astype(dtype)).astype(dtype)
        if upto == l:
            return z
        if a == "sigmoid" and l < len(spec.kernels) - 1:
            ARMS["pad_col.nonzero_act"] += (pad16(spec.units[l + 1]) - spec.units[l + 1]) * len(z)
        x = _act64(z, a, dtype)
    return x


def unnormalise(p, out_min, out_max, fault=None):
    """K6's regression epilogue on the f32 outputs p [rows]: (double)p * (max - min), rounded, + min, rounded -> f64"""
    L = _lib()
    span = float(out_max) - float(out_min)
    return np.array([L.wsa_or_unnormalise(float(v), float(out_min), span, int(fault == "fused_epilogue")) for v in np.asarray(p, np.float32)], np.float64)


def output_table(values, n, rows, nan_rows=(), fault=None, f64=False):
    """What a launch over n rows leaves in a table of `rows` rows seeded with the pattern: values [>= n (+ 1), C] bits for the rows below n, K6's
    quiet NaN in the rows whose nan_slot is set, the seed past n."""
    v = np.asarray(values)
    bits = v.view(np.uint64 if f64 else np.uint32).reshape(len(v), -1)
    out = np.full((rows, bits.shape[1]), SEED_F64 if f64 else SEED_F32, bits.dtype)
    m = n + 1 if fault == "row_guard" and n < min(rows, len(bits)) else n
    out[:m] = bits[:m]
    for r in nan_rows:
        if r < m:
            out[r] = QNAN_F64 if f64 else QNAN_F32
            ARMS["nan_slot.set"] += 1
    if len(nan_rows):
        ARMS["nan_slot.clear"] += m - sum(1 for r in nan_rows if r < m)
    if n % 16:
        ARMS["row.past_n"] += 1
    return out


def group_order(units_list):
    """K6e's work list: the members by descending multiply-adds per tile, a stable sort"""
    cost = [sum(pad16(u[l]) * pad16(u[l + 1]) for l in range(len(u) - 1)) * 16 * row_blocks(u) for u in units_list]
    order = list(range(len(units_list)))
    for i in range(1, len(order)):
        j = i
        while j > 0 and cost[order[j]] > cost[order[j - 1]]:
            order[j], order[j - 1] = order[j - 1], order[j]
            j -= 1
    return order


def group_walk(n, rbs, grid, fault=None):
    """classify_group_kernel's walk over the (member, tile) pairs of n rows, rbs in work-list order, `grid` workgroups: per member (work-list
    position) the set of rows some workgroup computes"""
    tiles = [(n + 16 * rb - 1) // (16 * rb) for rb in rbs]
    total = sum(tiles)
    rows = [set() for _ in rbs]
    for b in range(grid):
        for trip, i in enumerate(range(b, total, grid)):
            d, tile = 0, i
            while d < len(rbs) - 1:
                if tile < tiles[d]:
                    break
                if fault != "tile_kept":
                    tile -= tiles[d]
                d += 1
            else:
                ARMS["group.fell_through"] += 1 if len(rbs) > 1 else 0
            ARMS["wg.second_tile"] += 1 if trip else 0
            tm = 16 * rbs[d]
            rows[d].update(range(tile * tm, min(n, (tile + 1) * tm)))
    return rows


def tile_walk(n, rb, grid):
    """classify_kernel's grid-stride walk: counts a workgroup's second tile; returns the tiles per workgroup"""
    tiles = (n + 16 * rb - 1) // (16 * rb)
    per = [len(range(b, tiles, grid)) for b in range(grid)]
    ARMS["wg.second_tile"] += sum(max(p - 1, 0) for p in per)
    return per


def distance(a, b):
    """max |a - b| over the finite entries; the NaN and Inf patterns must be the same (else inf)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fa, fb = np.isfinite(a), np.isfinite(b)
    if not np.array_equal(fa, fb) or not np.array_equal(np.isnan(a), np.isnan(b)) or not np.array_equal(a[~fa & ~np.isnan(a)], b[~fb & ~np.isnan(b)]):
        return float("inf")
    return float(np.max(np.abs(a[fa] - b[fb]))) if fa.any() else 0.0

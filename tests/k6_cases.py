"""Hand-built networks and rows for K6 / K6e (csrc/classify.hip; test helper): one table of cases, every number from integer hashes
(train_cases.mix; no random generator, no libm), which tests/test_k6_reference.py examines on the CPU and tests/test_gpu_k6.py runs.

kind      what the device must give
  int     exact-integer networks (in_min 0, in_max 1, features k / 2, integer weights, relu / linear): every sum is exact in any order, so
          the expected bits depend on no rounding at all — bit for bit k6_ref.forward_bits
  real    relu / linear networks with weights and features over several binades: bit for bit forward_bits (order and rounding); the softmax
          twin (same weights) within 4 x D32 of a float64 softmax of its linear twin's logits
  tol     tanh / sigmoid hidden layers: within 4 x D32 of float64 from the device's own first pre-activation values where a truncated twin
          (first layer, linear, at most 64 wide) can hand them out, else of forward64
  special non-finite, subnormal and signed-zero features beside ordinary rows; flat input ranges; extreme logits; the -0 no sum can reach
          but a product can

d32: D32 of the case, the distance between the float64 yardstick and its numpy-float32 twin, measured once on the CPU and recorded here
(tests/test_k6_reference.py measures it again); bound = 4 x D32, from the references alone.  device: the distance of K6 on an MI355X from
the float64 yardstick, measured once."""
import functools

import numpy as np

from tests import k6_ref
from tests.train_cases import mix, unit
from webspeechanalyzer_amd import nnmodel

C_EDGES = (1, 16, 17, 63, 64)


def _case(key, kind, units, acts, salt, wmax=1, d32=None, device=None, out_range=None, rows=None):
    return dict(key=key, kind=kind, units=units, acts=acts, salt=salt, wmax=wmax, d32=d32, device=device, out_range=out_range, rows=rows)


CASES = {c["key"]: c for c in (
    # ---- exact integers: widths 1, 15, 16, 17, 63, 64, 65, 255, 256 | 257 (RB 4 | 2), 576 | 577 (RB 2 | 1), 1024; 1 and 8 layers; every C edge; every input width
    _case("i_one_unit", "int", [53, 1], ["linear"], 11, 2),
    _case("i_15_16_17", "int", [264, 15, 16, 17], ["relu", "linear", "relu"], 12, 2),
    _case("i_63_64_65", "int", [23, 63, 64, 65, 16], ["relu", "relu", "linear", "linear"], 13, 1),
    _case("i_255_256", "int", [53, 255, 256, 63], ["relu", "relu", "linear"], 14, 1),
    _case("i_257", "int", [53, 257, 64], ["relu", "linear"], 15, 2),
    _case("i_576", "int", [53, 576, 17], ["relu", "relu"], 16, 2),
    _case("i_577", "int", [53, 577, 16], ["relu", "linear"], 17, 2),
    _case("i_1024", "int", [53, 1024, 64], ["relu", "linear"], 18, 1),
    _case("i_eight", "int", [53, 17, 16, 15, 65, 17, 64, 63, 1], ["relu", "linear", "relu", "relu", "linear", "relu", "relu", "linear"], 19, 1),
    _case("i_264_one", "int", [264, 64], ["linear"], 20, 2),
    _case("i_23_one", "int", [23, 16], ["relu"], 21, 2),
    # ---- real values: the app's stacks (53-512-512-8 classifiers, 53-64-16-1 regression) and the widest model
    _case("r_app_cls", "real", [53, 512, 512, 8], ["relu", "relu", "softmax"], 31, d32=8.69e-8, device=7.917e-8),
    _case("r_app_reg", "real", [53, 64, 16, 1], ["relu", "relu", "linear"], 32, out_range=(-3.7, 12.9)),
    _case("r_app_reg_b", "real", [53, 64, 16, 1], ["linear", "relu", "linear"], 33, out_range=(0.1, 0.8)),
    _case("r_widest", "real", [53, 1024, 64], ["relu", "softmax"], 34, d32=3.21e-8, device=5.061e-8, rows=4200),
    # ---- tanh / sigmoid
    _case("t_17_16", "tol", [53, 17, 16, 5], ["sigmoid", "tanh", "softmax"], 41, d32=1.32e-7, device=1.023e-7),
    _case("t_257", "tol", [53, 257, 3], ["sigmoid", "softmax"], 42, d32=1.18e-7, device=2.070e-7),
    _case("t_app_reg", "tol", [53, 64, 16, 1], ["sigmoid", "sigmoid", "sigmoid"], 43, d32=6.60e-7, device=6.022e-7, out_range=(-3.7, 12.9)),
    _case("t_tanh_out", "tol", [23, 40, 1], ["tanh", "tanh"], 44, d32=1.45e-7, device=1.516e-7),
    # ---- special values
    _case("s_relu", "special", [53, 17, 5], ["relu", "softmax"], 51, d32=5.81e-8, device=7.514e-8),
    _case("s_sigmoid", "special", [53, 17, 5], ["sigmoid", "softmax"], 52, d32=1.57e-7, device=1.665e-7),
    _case("s_flat_range", "special", [53, 17, 5], ["relu", "softmax"], 53),
    _case("s_logits", "special", [53, 5], ["softmax"], 54, d32=1.06e-4, device=1.061e-4),
    _case("s_one_class", "special", [53, 1], ["softmax"], 55),
    _case("s_neg_zero", "special", [53, 16, 16], ["linear", "relu"], 56),
)}
KEYS = list(CASES)
EXACT_KEYS = [k for k, c in CASES.items() if all(a in ("relu", "linear") for a in c["acts"][:-1])]     # the logits at least are bit-exact
D32_KEYS = [k for k, c in CASES.items() if c["d32"] is not None]


def bound(case):
    """4 x D32: from the references alone, never from the device"""
    return 4.0 * case["d32"]


def rb_of(case):
    return k6_ref.row_blocks(case["units"])


def row_counts(case):
    """the row counts every case runs at: 1, 15, 16, 17, TM - 1, TM, TM + 1 and 5 TM + 3 for its own row tile"""
    tm = 16 * rb_of(case)
    return sorted({1, 15, 16, 17, tm - 1, tm, tm + 1, 5 * tm + 3})


def n_rows(case):
    return case["rows"] or 5 * 16 * rb_of(case) + 3


def marked_rows(n, rb):
    """the rows of the strided form whose nan_slot is set: the first, the last, and one alone in its tile"""
    tm = 16 * rb
    return sorted({0, n - 1} | ({tm + 3} if n > tm + 3 else set()))


def _binade(h, lo, hi):
    """2^e, e in lo .. hi from the hash"""
    return np.ldexp(1.0, (h % np.uint64(hi - lo + 1)).astype(np.int64) + lo)


def _int_spec(c):
    units, salt, w = c["units"], c["salt"], c["wmax"]
    ks, bs = [], []
    for l in range(len(units) - 1):
        k, n = np.arange(units[l])[:, None], np.arange(units[l + 1])[None, :]
        ks.append(((mix(k, n, salt + 100 * l) % np.uint64(2 * w + 1)).astype(np.int64) - w).astype(np.float32))
        bs.append(((mix(n[0], 7, salt + 100 * l + 1) % np.uint64(5)).astype(np.int64) - 2).astype(np.float32))
    nin = units[0]
    return nnmodel.ModelSpec(units, list(c["acts"]), ks, bs, np.zeros(nin), np.ones(nin), [f"c{i}" for i in range(units[-1])])


def _int_rows(c, n):
    r, f = np.arange(n)[:, None], np.arange(c["units"][0])[None, :]
    return ((mix(r, f, c["salt"] + 5) % np.uint64(13)).astype(np.int64) - 6) / 2.0


def _real_spec(c, units=None, acts=None):
    units, acts, salt = units or c["units"], acts or c["acts"], c["salt"]
    ks, bs = [], []
    for l in range(len(units) - 1):
        k, n = np.arange(units[l])[:, None], np.arange(units[l + 1])[None, :]
        scale = 2.0 / np.sqrt(units[l])
        ks.append((unit(mix(k, n, salt + 100 * l)) * _binade(mix(k, n, salt + 100 * l + 1), -4, 1) * scale).astype(np.float32))
        bs.append((unit(mix(n[0], 7, salt + 100 * l + 2)) * _binade(mix(n[0], 9, salt + 100 * l + 3), -5, -1)).astype(np.float32))
    nin = units[0]
    f = np.arange(nin)
    in_min, in_max = -1.25 - 0.01 * (f % 7), 2.5 + 0.03 * (f % 11)
    out = c["out_range"] or (None, None)
    return nnmodel.ModelSpec(list(units), list(acts), ks, bs, in_min, in_max, [f"c{i}" for i in range(units[-1])], out[0], out[1])


def _real_rows(c, n):
    r, f = np.arange(n)[:, None], np.arange(c["units"][0])[None, :]
    return unit(mix(r, f, c["salt"] + 5)) * _binade(mix(r, f, c["salt"] + 6), -3, 1) + 0.5


# ---- the special cases' rows: 17 rows of one 16-row block and its neighbour, the poisoned features named here
S_ROWS = 17
POISON = {                    # row: (feature, value)            what it is
    1: (-1, float("nan")),    # the LAST feature of row r - 1 (r = 2): the double in front of row 2's first
    3: (0, float("nan")),     # feature 0 of row r + 1: the double behind row 2's last, where a padded k would read on
    5: (10, float("inf")),
    6: (11, float("-inf")),
    8: (3, 1e300),            # a finite double that is +Inf in the f32 tensor
    9: (4, 1e-41),            # (set after the range: a subnormal after normalisation)
    11: (6, -1e-60),          # in_min 0: -0 in the f32 tensor
    12: (6, -0.0),
    16: (52, float("inf")),   # the neighbour block's first row
}
FLAT = 7                      # s_flat_range: in_max == in_min == 0.25 at this input; rows 0, 4, 8, 12, 16 have x == min (NaN), the rest +-Inf


def _special(c):
    key = c["key"]
    if key == "s_logits":                    # logits: rows 0 .. 3 +-1e4 (feature 0 = 1), rows 4 .. 7 all equal (features 0), rows 8, 9 one +Inf (an f32 overflow), 10, 11 +Inf and NaNs, rest ordinary
        C = c["units"][-1]
        k = np.zeros((53, C), np.float32)
        k[0] = [1e4 if j % 2 == 0 else -1e4 for j in range(C)]
        k[1, 0] = 2.0
        k[2:] = _real_spec(c).kernels[0][2:]
        b = np.full(C, 0.5, np.float32)
        spec = nnmodel.ModelSpec([53, C], ["softmax"], [k], [b], np.zeros(53), np.ones(53), [f"c{i}" for i in range(C)])
        feat = _real_rows(c, S_ROWS)
        feat[:, 0:2] = 0.0
        feat[0:4, 2:] = 0.0; feat[0:4, 0] = [1.0, -1.0, 1.0, -1.0]
        feat[4:8] = 0.0
        feat[8:10, 1] = 3e38
        feat[10:12, 1] = 1e300                # +Inf in the tensor: +Inf in logit 0, Inf x 0 = NaN in the others, which fmaxf passes over
        return spec, feat
    if key == "s_one_class":
        spec = _real_spec(c)
        return spec, _real_rows(c, S_ROWS)
    if key == "s_neg_zero":                  # hidden unit 0 = 2^-100 (its bias), the rest +0; a negative weight on each: the first product
        k0 = np.zeros((53, 16), np.float32)  # underflows to -0, the other fifteen are +0 x negative = -0, the bias is -0: the only way to a -0 sum
        b0 = np.zeros(16, np.float32); b0[0] = np.float32(2.0 ** -100)
        k1 = np.full((16, 16), -1.0, np.float32); k1[0] = np.float32(-(2.0 ** -100))
        k1[:, 8:] = 1.0                      # columns 8 .. 15: +0 sums beside them
        b1 = np.zeros(16, np.float32); b1[:8] = np.float32(-0.0)
        spec = nnmodel.ModelSpec([53, 16, 16], ["linear", "relu"], [k0, k1], [b0, b1], np.zeros(53), np.ones(53), [f"c{i}" for i in range(16)])
        return spec, _real_rows(c, S_ROWS)
    spec = _real_spec(c)
    spec.in_min = np.array(spec.in_min); spec.in_max = np.array(spec.in_max)
    feat = _real_rows(c, S_ROWS)
    if key == "s_flat_range":
        spec.in_min[FLAT] = spec.in_max[FLAT] = 0.25
        feat[::4, FLAT] = 0.25
        spec.kernels[0][FLAT, 0] = 0.0       # an exact zero weight beside the Inf: NaN in one hidden unit, +-Inf in the others
        return spec, feat
    spec.in_min[6] = 0.0
    spec.kernels[0][52] = np.abs(spec.kernels[0][52])          # row 16's +Inf input: +Inf in every hidden unit, +Inf in logit 0 (sigmoid: 1 in every unit)
    spec.kernels[1][:, 0] = np.abs(spec.kernels[1][:, 0])
    for k in range(spec.units[1]):           # exact zero weights under the poisoned inputs, in some units only: Inf x 0 = NaN there
        if k % 3 == 0 and key == "s_relu":    # (s_sigmoid keeps every weight: an Inf input then gives 0 or 1 in every unit and finite probabilities, as in tfjs)
            spec.kernels[0][10, k] = spec.kernels[0][3, k] = 0.0
    for r, (f, v) in POISON.items():
        feat[r, f] = v
    feat[9, 4] = spec.in_min[4] + 1e-41 * (spec.in_max[4] - spec.in_min[4])
    return spec, feat


@functools.lru_cache(maxsize=None)
def build(key):
    """(spec, feat [rows, nin] f64) of the case, shared between the tests: treat as read-only"""
    c = CASES[key]
    if c["kind"] == "int":
        return _int_spec(c), _int_rows(c, n_rows(c))
    if c["kind"] == "special":
        return _special(c)
    return _real_spec(c), _real_rows(c, n_rows(c))


def clean_rows(key):
    """the special case's rows with every poisoned row made ordinary (what its neighbours are compared against)"""
    c = CASES[key]
    feat = build(key)[1].copy()
    plain = _real_rows(c, S_ROWS)
    for r in POISON:
        feat[r] = plain[r]
    return feat


def twin(spec, upto=None, last="linear"):
    """the same weights up to layer `upto` (default all) with the last activation replaced: hands out pre-activation values"""
    n = len(spec.kernels) if upto is None else upto + 1
    acts = list(spec.activations[:n - 1]) + [last]
    return nnmodel.ModelSpec(list(spec.units[:n + 1]), acts, spec.kernels[:n], spec.biases[:n], spec.in_min, spec.in_max, [f"c{i}" for i in range(spec.units[n])])


def yardstick(key, dtype=np.float64, pre0=None):
    """the tolerance yardstick of a case in `dtype`, for every row: [rows, C] (a regression: the f32 output, before the epilogue).
    Softmax over relu / linear layers: softmax of forward_bits' logits.  tanh / sigmoid: forward64 from the first layer's pre-activation
    values (pre0: the device's own; default forward_bits', which the device must equal) when the first layer is at most 64 wide, else
    forward64 from the features."""
    spec, feat = build(key)
    if key in EXACT_KEYS:
        logits = k6_ref.forward_bits(spec, feat)["out"]
        return k6_ref.softmax(logits, dtype) if spec.activations[-1] == "softmax" else logits.astype(dtype)
    if spec.units[1] <= 64:
        if pre0 is None:
            pre0 = k6_ref.forward_bits(twin(spec, 0), feat)["out"]
        y = k6_ref.forward64(spec, feat, dtype=dtype, start=(0, pre0))
    else:
        y = k6_ref.forward64(spec, feat, dtype=dtype)
    if CASES[key]["out_range"]:                         # a regression: the value, the epilogue in double on the output as `dtype` holds it
        lo, hi = CASES[key]["out_range"]
        y = y.astype(np.float64) * (hi - lo) + lo
    return y


def d32(key):
    """D32 of the case, computed fresh"""
    return k6_ref.distance(yardstick(key, np.float32), yardstick(key))


@functools.lru_cache(maxsize=None)
def expected(key):
    """What the device must give for every row of the case, computed once and shared (read-only):
    logits — f32, bit for bit (the linear twin's output; None where a tanh / sigmoid layer comes first);
    bits   — the case's own output as uint32 [rows, C] (uint64 [rows, 1] for a regression) where it is exact, else None;
    yard   — the float64 yardstick where it is not (bound(case) applies), else None;
    pre0   — the first layer's pre-activation values f32, bit for bit, where a truncated twin hands them out."""
    c = CASES[key]
    spec, feat = build(key)
    e = dict(logits=None, bits=None, yard=None, pre0=None)
    if key in EXACT_KEYS:
        e["logits"] = k6_ref.forward_bits(spec, feat)["out"]
        if spec.activations[-1] == "softmax":
            e["yard"] = k6_ref.softmax(e["logits"], np.float64, count=True)
            if spec.units[-1] == 1:                      # C = 1: exp(x - (x + log 1)) is exactly 1 for every finite logit
                e["bits"] = np.where(np.isfinite(e["logits"]), np.float32(1.0), np.float32("nan")).view(np.uint32)
        elif c["out_range"]:
            e["bits"] = k6_ref.unnormalise(e["logits"][:, 0], *c["out_range"]).view(np.uint64)[:, None]
        else:
            e["bits"] = e["logits"].view(np.uint32)
    else:
        if spec.units[1] <= 64:
            e["pre0"] = k6_ref.forward_bits(twin(spec, 0), feat)["out"]
        e["yard"] = yardstick(key)
    return e


# ---- the group: members with RB 4, 2 and 1 (hidden widths 64, 257, 577), one model twice
GROUP = ("g_64", "g_257", "g_577", "g_64")
GROUP_CASES = {
    "g_64": _case("g_64", "real", [53, 64, 17], ["relu", "linear"], 61),
    "g_257": _case("g_257", "real", [53, 257, 5], ["relu", "linear"], 62),
    "g_577": _case("g_577", "real", [53, 577, 64], ["relu", "linear"], 63),
}
GROUP_ROWS_CAP = 64           # the grid: 1 + 2 + 4 + 1 = 8 workgroups (16 with one_block), one per (member, tile) pair of 64 rows
GROUP_COUNTS = (0, 1, 17, 33, 65)            # 65: one row more than the grid holds, 2 + 3 + 5 + 2 = 12 pairs (20 with one_block): second trips


@functools.lru_cache(maxsize=None)
def group_build():
    specs = {k: _real_spec(c) for k, c in GROUP_CASES.items()}
    feat = _real_rows(GROUP_CASES["g_64"], max(GROUP_COUNTS))
    return specs, feat

"""Float64 references and per-element error bounds for the non-convolution kernels (csrc/pointwise.hip, csrc/head_ops.hip)
and MatMul's non-transposed GEMM.  The pattern of tests/ref64.py: a float64 reference from the operands exactly as the oracle
defines them, a tolerance per element, and `ref64.check` to compare.

Row kernels (softmax_kernel, reduce_rows_kernel, gap_kernel, gap_q4_kernel, instancenorm_kernel) run one wave64 per row: a
lane adds ceil(n/64) terms in sequence and a 6-level shuffle tree combines the lanes, so a sum of n terms carries

    g(n) = (ceil(n/64) + 6) * u,      u = 2^-24

and a rounded sum s differs from the exact one by at most lam * g(n) * sum|x|.  The bounds:

* ReduceSum: lam * g(n) * sum|x|;
* ReduceMean, GlobalAveragePool (NCHW and Q4: s * (1/n), two roundings): ReduceSum's bound / n + 2u |mean|;
* ReduceMax / Min, HardSigmoid: exact;
* LogSoftmax: t = (x - m) - log s is off by at most
      2u (|x - m| + |log s|) + ULP["log"] 2u |log s| + (lam g(n) + ULP["exp"] 2u)
  (the last term: the relative error of s, which log turns into an absolute one);
  Softmax: exp(t), relative error ULP["exp"] 2u + that bound on t;
* InstanceNormalization: the mean's error is carried through the two-pass variance, powf(., 0.5), k = s/dev and
  off = b - s mean/dev (see `instancenorm_bound`);
* upsample_linear (integer factors): exact on integer operands (the float16 weights of power-of-two factors are
  multiples of 2^-6); on float data lam u sum|w_i x_i| over the product + three fmas of the kernel;
* resize_linear (fractional factors, resize_planes_kernel): lam u sum|w_i x_i|, the weights being the float32 fractions of
  layer._linear_positions and their float32 complements, as the reference rounds them;
* Erf: exact (a table lookup);
* exp, log, tanh, sqrt, reciprocal, sigmoid, pow: ULP[f] units in the last place of the float64 result rounded to float32;
* the LSTM cell (pl_lstm_cell_f32): ULP["lstm"] units in the last place of each rounded term -- f * c_prev, i * tanh(g)
  and C for the cell state, h for the output -- plus C's bound carried into h (tanh is 1-Lipschitz, sigmoid(o) <= 1), and
  SIGMOID_FLOOR per gate;
* MatMul: ref64.bound with LAMBDA["direct"] -- the product is launched as the 1x1 conv it is.

Subnormal outputs: softmax and exp results below 2^-126 lose relative precision as their exponent runs out; their error is
a few units of 2^-149 however exact the computation, so those bounds get an absolute floor SUBNORMAL_FLOOR = 4 * 2^-149
(one rounding of the result and one of exp's argument, each up to 2^-149 there, doubled).

Each lam (LAM) is 4x the worst err / (bound at lam = 1) of a float32 emulation of the kernel's order of operations
(`emulate_*`) over `calibration_cases`, rounded up; tests/test_ops_ref64.py checks that every constant still covers it.
"""
import math

import numpy as np

from tests.ref64 import U, check, ratio  # noqa: F401  (re-exported for the tests)

F32 = np.float32
SUBNORMAL_FLOOR = 4 * 2.0 ** -149
# sigmoid as the reference writes it, 1 / (1 + exp(-v)), is 0 once exp(-v) overflows (v < -88.72), where the true value is
# below 2^-127: the LSTM cell's gates carry that much absolute error on top of their ulps
SIGMOID_FLOOR = 2.0 ** -126
# ulps of the float64 result, each at most 4 (see the module docstring)
ULP = {"exp": 2.0, "log": 2.0, "tanh": 2.0, "sqrt": 0.5, "reciprocal": 0.5, "sigmoid": 3.0, "pow": 2.0, "lstm": 4.0}
# worst emulated ratios (tests/test_ops_ref64.py): sum 0.251, mean 0.198, gap 0.325, softmax 0.783, logsoftmax 0.929,
# instancenorm 0.890, upsample_linear 2.94, resize_linear 2.67
LAM = {"sum": 1.5, "softmax": 3.5, "logsoftmax": 4.0, "instancenorm": 4.0, "upsample_linear": 12.0, "resize_linear": 11.0}


def g(n):
    return (math.ceil(n / 64) + 6) * U


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- references ---------------------------------------------------------------------------------------------------------
def reduce64(x, op):
    """Rows of x (rows, n) reduced in float64: 0 sum, 1 mean, 2 max, 3 min."""
    x = _f64(x)
    return [x.sum(-1), x.mean(-1), x.max(-1), x.min(-1)][op]


def softmax64(x, log=False):
    x = _f64(x)
    y = x - x.max(-1, keepdims=True)
    y = y - np.log(np.exp(y).sum(-1, keepdims=True))
    return y if log else np.exp(y)


def instancenorm64(x, s, b, eps=1e-5):
    """x (rows, n), s / b per row."""
    x = _f64(x)
    mean = x.mean(-1, keepdims=True)
    dev = np.sqrt(((x - mean) ** 2).mean(-1, keepdims=True) + _f64(F32(eps)))
    s, b = _f64(s).reshape(-1, 1), _f64(b).reshape(-1, 1)
    return (x - mean) * (s / dev) + b


# ---- bounds -------------------------------------------------------------------------------------------------------------
def sum_bound(x, lam=None):
    lam = LAM["sum"] if lam is None else lam
    x = _f64(x)
    return lam * g(x.shape[-1]) * np.abs(x).sum(-1)


def mean_bound(x, lam=None):
    x = _f64(x)
    return sum_bound(x, lam) / x.shape[-1] + 2 * U * np.abs(x.mean(-1))


def softmax_t_bound(x, lam=None):
    """Absolute bound on t = (x - m) - log s, per element of x (rows, n)."""
    lam = LAM["logsoftmax"] if lam is None else lam
    x = _f64(x)
    d = x - x.max(-1, keepdims=True)
    ls = np.log(np.exp(d).sum(-1, keepdims=True))
    return 2 * U * (np.abs(d) + np.abs(ls)) + ULP["log"] * 2 * U * np.abs(ls) + (lam * g(x.shape[-1]) + ULP["exp"] * 2 * U)


def softmax_bound(x, log=False, lam=None):
    tb = softmax_t_bound(x, LAM["logsoftmax" if log else "softmax"] if lam is None else lam)
    if log:
        return tb
    y = softmax64(x)
    return np.maximum(y * (np.expm1(ULP["exp"] * 2 * U + tb)), SUBNORMAL_FLOOR)


def instancenorm_bound(x, s, b, eps=1e-5, lam=None):
    lam = LAM["instancenorm"] if lam is None else lam
    x = _f64(x)
    n = x.shape[-1]
    s, b = _f64(s).reshape(-1, 1), _f64(b).reshape(-1, 1)
    mean = x.mean(-1, keepdims=True)
    d2 = ((x - mean) ** 2).sum(-1, keepdims=True)
    var = d2 / n + _f64(F32(eps))
    dev = np.sqrt(var)
    em = (g(n) * np.abs(x).sum(-1, keepdims=True)) / n + 2 * U * np.abs(mean)           # the mean
    ev = ((g(n) + 3 * U) * d2 + n * em * em) / n + 2 * U * var                             # variance + eps
    rdev = 0.5 * ev / var + ULP["pow"] * 2 * U                                             # powf(., 0.5)
    k = np.abs(s) / dev
    off = np.abs(b - s * mean / dev)
    y = np.abs((x - mean) * (s / dev) + b)
    return lam * (np.abs(x) * k * (rdev + 2 * U) + k * (em + np.abs(mean) * (rdev + 3 * U)) + U * off + U * y)


def ulp_bound(ref, name):
    """ULP[name] units in the last place of the float32 rounding of the float64 result ref."""
    r32 = np.abs(_f64(ref).astype(F32))
    sp = np.spacing(np.where(np.isfinite(r32), r32, F32(0))).astype(np.float64)
    return ULP[name] * sp


def ulps(y, ref):
    """|y - ref| in units of the float32 spacing at ref (0 where equal, NaN matching NaN)."""
    y, ref = _f64(y), _f64(ref)
    sp = np.spacing(np.abs(ref.astype(F32))).astype(np.float64)
    with np.errstate(invalid="ignore"):
        e = np.where((y == ref) | (np.isnan(y) & np.isnan(ref)), 0.0, np.abs(y - ref) / sp)
    return np.where(np.isnan(e), np.inf, e)


# ---- float32 emulations of the kernels' order of operations ---------------------------------------------------------------
def emulate_rowsum(x):
    """reduce_rows_kernel / gap_kernel / softmax_kernel's sum: lane l adds x[l], x[l + 64], ... in sequence, then the lanes
    pair up 32, 16, ..., 1 apart."""
    x = np.asarray(x, F32)
    rows, n = x.shape
    k = math.ceil(n / 64)
    p = np.zeros((rows, k * 64), F32)
    p[:, :n] = x
    p = p.reshape(rows, k, 64)
    acc = np.zeros((rows, 64), F32)
    for i in range(k):
        acc = (acc + p[:, i]).astype(F32)
    off = 32
    while off:
        acc = (acc[:, :off] + acc[:, off:2 * off]).astype(F32)
        off >>= 1
    return acc[:, 0]


def emulate_gap(x):
    n = x.shape[-1]
    return (emulate_rowsum(x) * (F32(1) / F32(n))).astype(F32)


def emulate_mean(x):
    return (emulate_rowsum(x) / F32(x.shape[-1])).astype(F32)


def _exp32(v):
    return np.exp(_f64(v)).astype(F32)          # a correctly rounded expf


def emulate_softmax(x, log=False, exp=_exp32):
    x = np.asarray(x, F32)
    m = x.max(-1, keepdims=True)
    d = (x - m).astype(F32)
    s = emulate_rowsum(exp(d))[:, None]
    ls = np.log(_f64(s)).astype(F32)
    t = (d - ls).astype(F32)
    return t if log else exp(t)


def emulate_instancenorm(x, s, b, eps=1e-5, two_pass=True):
    x = np.asarray(x, F32)
    n = x.shape[-1]
    mean = (emulate_rowsum(x) / F32(n)).astype(F32)[:, None]
    if two_pass:
        d = (x - mean).astype(F32)
        sq = emulate_rowsum((d * d).astype(F32))[:, None]
        var = (sq / F32(n)).astype(F32)
    else:                                       # the mutation: E[x^2] - mean^2
        ex2 = (emulate_rowsum((x * x).astype(F32)) / F32(n)).astype(F32)[:, None]
        var = np.maximum((ex2 - mean * mean).astype(F32), F32(0))
    dev = np.sqrt(_f64((var + F32(eps)).astype(F32))).astype(F32)
    s, b = np.asarray(s, F32).reshape(-1, 1), np.asarray(b, F32).reshape(-1, 1)
    k = (s / dev).astype(F32)
    off = (b - ((s * mean).astype(F32) / dev).astype(F32)).astype(F32)
    return ((x * k).astype(F32) + off).astype(F32)


# ---- interpolation and the LSTM cell ----------------------------------------------------------------------------------------
def _bilinear_blocks(x, fh, fw, combine):
    """The oracle's upsample_bilinear (oracle/planer_np.py) with the weighted sum of each neighbourhood done by
    `combine(corners (..., T), table (T, fh*fw) float64)`."""
    from oracle import planer_np as onp
    n, c, h, w = x.shape
    p = x
    if fh > 1:
        p = np.concatenate([p[:, :, :1], p, p[:, :, -1:]], axis=2)
    if fw > 1:
        p = np.concatenate([p[:, :, :, :1], p, p[:, :, :, -1:]], axis=3)
    if fh == 1:
        corners = [p[:, :, :, :-1], p[:, :, :, 1:]]
    elif fw == 1:
        corners = [p[:, :, :-1, :], p[:, :, 1:, :]]
    else:
        corners = [p[:, :, :-1, :-1], p[:, :, :-1, 1:], p[:, :, 1:, :-1], p[:, :, 1:, 1:]]
    field = np.stack(corners, axis=-1).reshape(-1, len(corners))
    blocks = combine(field, onp._bilinear_table(fh, fw).astype(np.float64))
    hh, ww = h + (fh > 1), w + (fw > 1)
    out = blocks.reshape(-1, ww, fh, fw).transpose(0, 2, 1, 3).reshape(n, c, hh * fh, ww * fw)
    return out[:, :, fh // 2:h * fh + fh // 2, fw // 2:w * fw + fw // 2]


def upsample_linear64(x, fh, fw):
    return _bilinear_blocks(_f64(x), fh, fw, lambda f, t: f @ t)


def upsample_linear_bound(x, fh, fw, lam=None):
    lam = LAM["upsample_linear"] if lam is None else lam
    return lam * U * upsample_linear64(np.abs(_f64(x)), fh, fw)        # the weights are >= 0


def emulate_upsample_linear(x, fh, fw, drop_last=False):
    """upsample_linear_kernel: v = fma(x0, w0, 0), then fma(x_t, w_t, v) per corner, each rounded once to float32.
    `drop_last`: the mutation that leaves the last corner out."""
    def fma_chain(f, t):
        v = np.zeros((f.shape[0], t.shape[1]), F32)
        for i in range(t.shape[0] - (1 if drop_last else 0)):
            v = (_f64(f[:, i])[:, None] * t[i][None, :] + _f64(v)).astype(F32)
        return v
    return _bilinear_blocks(np.asarray(x, F32), fh, fw, fma_chain)


def _resize_weights(h, w, oh, ow):
    from planer_amd.layer import _linear_positions
    ra, rs = _linear_positions(h, oh)
    ca, cs = _linear_positions(w, ow)
    return ra, rs, (F32(1) - rs).astype(F32), ca, cs, (F32(1) - cs).astype(F32)


def resize_linear64(x, oh, ow):
    """Columns then rows with the float32 fractions and complements the kernel (and the reference) use, in float64."""
    x = _f64(x)
    ra, rs, gr, ca, cs, gc = (_f64(a) if a.dtype != np.int32 else a for a in _resize_weights(*x.shape[-2:], oh, ow))
    cols = x[..., :, ca] * gc + x[..., :, ca + 1] * cs
    return cols[..., ra, :] * gr[:, None] + cols[..., ra + 1, :] * rs[:, None]


def resize_linear_bound(x, oh, ow, lam=None):
    lam = LAM["resize_linear"] if lam is None else lam
    return lam * U * resize_linear64(np.abs(_f64(x)), oh, ow)


def emulate_resize_linear(x, oh, ow):
    """resize_planes_kernel's float32 roundings (the reference's own)."""
    x = np.asarray(x, F32)
    ra, rs, gr, ca, cs, gc = _resize_weights(*x.shape[-2:], oh, ow)
    cols = (x[..., :, ca] * gc + x[..., :, ca + 1] * cs).astype(F32)
    return (cols[..., ra, :] * gr[:, None] + cols[..., ra + 1, :] * rs[:, None]).astype(F32)


def lstm_gates(gx, gh, b):
    """The four gate pre-activations, rounded to float32 after each add as the kernel and the reference do."""
    H = b.shape[-1] // 8
    return (((np.asarray(gx, F32) + np.asarray(gh, F32)).astype(F32) + np.asarray(b[:4 * H], F32)).astype(F32)
            + np.asarray(b[4 * H:], F32)).astype(F32)


def lstm_cell64(gx, gh, b, c_prev):
    """-> (h, C, f * c_prev, i * tanh(g)) in float64 from the float32 gates; gates in ONNX order i, o, f, c."""
    g = _f64(lstm_gates(gx, gh, b))
    H = g.shape[-1] // 4
    sig = lambda v: 1 / (1 + np.exp(-v))        # noqa: E731
    i, o, f, cg = sig(g[:, :H]), sig(g[:, H:2 * H]), sig(g[:, 2 * H:3 * H]), np.tanh(g[:, 3 * H:])
    fc, ic = f * _f64(c_prev), i * cg
    C = fc + ic
    return o * np.tanh(C), C, fc, ic, o


def _sp(v):
    return np.spacing(np.abs(_f64(v).astype(F32))).astype(np.float64)


def lstm_cell_bound(gx, gh, b, c_prev):
    """-> (tol_h, tol_c): ULP["lstm"] ulps of each rounded term, C's bound carried into h."""
    h, C, fc, ic, o = lstm_cell64(gx, gh, b, c_prev)
    g = _f64(lstm_gates(gx, gh, b))
    H = g.shape[-1] // 4
    tc = ULP["lstm"] * (_sp(fc) + _sp(ic) + _sp(C)) + SIGMOID_FLOOR * (np.abs(_f64(c_prev)) + np.abs(np.tanh(g[:, 3 * H:])))
    return ULP["lstm"] * _sp(h) + o * tc + SIGMOID_FLOOR, tc


def emulate_lstm_cell(gx, gh, b, c_prev, exp=None):
    """lstm_cell_kernel in float32 with correctly rounded expf / tanhf (`exp`: a replacement expf, for mutations)."""
    exp = exp or (lambda v: np.exp(_f64(v)).astype(F32))
    with np.errstate(over="ignore"):
        return _lstm_cell32(gx, gh, b, c_prev, exp)


def _lstm_cell32(gx, gh, b, c_prev, exp):
    g = lstm_gates(gx, gh, b)
    H = g.shape[-1] // 4
    sig = lambda v: (F32(1) / (exp(-v) + F32(1)).astype(F32)).astype(F32)       # noqa: E731
    th = lambda v: np.tanh(_f64(v)).astype(F32)                                 # noqa: E731
    i, o, f, cg = sig(g[:, :H]), sig(g[:, H:2 * H]), sig(g[:, 2 * H:3 * H]), th(g[:, 3 * H:])
    C = ((f * np.asarray(c_prev, F32)).astype(F32) + (i * cg).astype(F32)).astype(F32)
    return (o * th(C)).astype(F32), C


# ---- data -------------------------------------------------------------------------------------------------------------------
def skewed_rows(rng, rows, n, dc=0.0, lo=-10, hi=6):
    """Standard normal rows, each scaled by 2^U(lo, hi), plus a DC offset."""
    return (rng.standard_normal((rows, n)) * 2.0 ** rng.uniform(lo, hi, (rows, 1)) + dc).astype(F32)


def lstm_operands(rng, N, H, spread=4.0):
    gx = (rng.standard_normal((N, 4 * H)) * spread).astype(F32)
    gh = (rng.standard_normal((N, 4 * H)) * spread).astype(F32)
    b = rng.standard_normal(8 * H).astype(F32)
    cp = (rng.standard_normal((N, H)) * 2.0 ** rng.uniform(-10, 6, (N, 1))).astype(F32)
    return gx, gh, b, cp


def calibration_cases():
    rng = np.random.default_rng(7)
    for n in (1, 63, 64, 65, 1000, 4096, 50176):
        rows = max(2, min(64, 400000 // n))
        for dc in (0.0, 50.0):
            yield n, dc, skewed_rows(rng, rows, n, dc)

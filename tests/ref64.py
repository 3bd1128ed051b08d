"""Float64 reference and per-element error bounds for the convolution kernels.

`ref64` is the oracle's conv (oracle/planer_np.conv2d, which follows the dtype of its operands) on float64 copies, followed by
the fused tail in the order of apply_epilogue (csrc/device_utils.h): bias, scale, shift, residual before or after the
activation, then ReLU or leaky ReLU in the reference's form x * ((x > 0) * (1 - a) + a).

Two ways to use it:

* integer operands (`int_operands`): x and K in [-3, 3] with zero runs and zero channels, integer bias and residual, BN scales
  in {+-0.5, +-1, +-2, +-4}, shifts in multiples of 0.25, leaky alpha 0.125.  Every product and partial sum is then an exactly
  representable fp32 value whatever the summation order (`assert_exact` checks the magnitudes on the host), so a kernel must
  equal `ref64` bit for bit;
* float data: `bound` gives a per-element tolerance

      tol = lam * u * sqrt(Kred) * |scale_c| * sqrt(conv(x^2, K^2)) + 4u * (|scale_c| * (conv(|x|, |K|) + |B|) + |shift_c| + |res|)

  with u = 2^-24 and Kred = Cin/group * kh * kw, all in float64.  ReLU and leaky ReLU with alpha <= 1 are non-expansive, so
  the bound passes through the activation unchanged.  `check` compares element by element.

The lam of each family (LAMBDA) is fixed from the algorithm, not from the kernel under test: tests/test_conv_ref64.py measures
the worst err / (u * sqrt(Kred) * L2) of a float32 emulation of each algorithm over a case set (`calibration_cases`) and fails
if a constant here no longer covers 4x that ratio.
"""
import numpy as np

from oracle import planer_np as onp

U = 2.0 ** -24
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_RES_AFTER = 0, 1, 2, 16

# Per-family lam.  Direct families (an fmaf / MFMA chain or a blocked sum per output): 8 -- the float32 oracle (an sgemm; worst
# ratio 3.65 over calibration_cases) is checked against it on every case.  Each Winograd constant is 4x the worst
# err / (u sqrt(Kred) L2) of the float32 emulation `wino_emulate` of its transforms over `calibration_cases`, rounded up:
#   F(2x2,3x3) 2.75, F(4x4,3x3) 32.5, 1-D F(4,3) along W 7.94, mixed F(4,3) / F(3,3) segments 28.5
# (the worst case is the 5-channel skewed map for F(2x2) and the skewed batch of 32 for the others: the worst element grows
# with the number of elements drawn, so the calibration set holds one case of real layer size).
LAMBDA = {
    "direct": 8.0,
    "f2x2": 12.0,
    "f4x4": 132.0,
    "w1d4": 32.0,
    "wino43": 116.0,
}


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _chan(a):
    return None if a is None else _f64(a).reshape(1, -1, 1, 1)


def conv64(x, K, B=None, group=1, strides=(1, 1), dilations=(1, 1), pads=(0, 0, 0, 0)):
    """oracle conv2d in float64 (same pad rules and geometry)."""
    y = onp.conv2d(_f64(x), _f64(K), _f64(B), group=group, strides=strides, dilations=dilations, pads=pads)
    return np.ascontiguousarray(y)


def tail64(y, B=None, scale=None, shift=None, res=None, act=ACT_NONE, alpha=0.0):
    y = np.array(y, dtype=np.float64)
    if B is not None:
        y = y + _chan(B)
    if scale is not None:
        y = y * _chan(scale)
    if shift is not None:
        y = y + _chan(shift)
    post, kind = act & ACT_RES_AFTER, act & 15
    if res is not None and not post:
        y = y + _f64(res).reshape(y.shape)
    if kind == ACT_RELU:
        y = y * (y > 0)
    elif kind == ACT_LEAKY:
        y = y * ((y > 0) * (1.0 - alpha) + alpha)
    if res is not None and post:
        y = y + _f64(res).reshape(y.shape)
    return y


def ref64(x, K, B=None, scale=None, shift=None, res=None, act=ACT_NONE, alpha=0.0, **conv):
    """The conv plus fused tail in float64."""
    return tail64(conv64(x, K, **conv), B, scale, shift, res, act, alpha)


# ---- integer operands -------------------------------------------------------------------------------------------------
SCALES = np.array([-4.0, -2.0, -1.0, -0.5, 0.5, 1.0, 2.0, 4.0])
ALPHA = 0.125


def int_tensor(rng, shape, lo=-3, hi=3):
    """Integers in [lo, hi] with zero runs along W (post-ReLU-like) and, where there are several, a whole zero channel."""
    a = rng.integers(lo, hi + 1, shape).astype(np.float32)
    if len(shape) == 4 and shape[3] > 2:
        n, c, h, w = shape
        m = rng.random((n, c, h)) < 0.3
        start = rng.integers(0, w, (n, c, h))
        ln = rng.integers(1, max(2, w // 2) + 1, (n, c, h))
        cols = np.arange(w)
        run = m[..., None] & (cols >= start[..., None]) & (cols < (start + ln)[..., None])
        a[run] = 0
    if len(shape) == 4 and shape[1] > 2:
        a[:, int(rng.integers(0, shape[1]))] = 0
    return a


def int_tail(rng, cout, out_shape, bias=False, bn=False, res=False):
    """(B, scale, shift, res) of the integer form, None where the tail has no such term."""
    B = rng.integers(-8, 9, cout).astype(np.float32) if bias else None
    sc = rng.choice(SCALES, cout).astype(np.float32) if bn else None
    sh = (rng.integers(-16, 17, cout) * 0.25).astype(np.float32) if bn else None
    r = rng.integers(-8, 9, out_shape).astype(np.float32) if res else None
    return B, sc, sh, r


def int_operands(rng, xs, ks, bias=False, bn=False, res=False, **conv):
    """x, K and tail of the integer form for a conv of input xs and filter ks -> (x, K, B, scale, shift, res)."""
    x = int_tensor(rng, xs)
    K = int_tensor(rng, ks)
    out = conv64(np.zeros(xs, np.float32), np.zeros(ks, np.float32), **conv).shape
    return (x, K) + int_tail(rng, ks[0], out, bias, bn, res)


def assert_exact(x, K, B=None, scale=None, shift=None, res=None, gran=0.25, **conv):
    """Host precondition of the integer form: conv(|x|, |K|) + |B|, carried through the tail, stays below 2^22 units of the
    finest granularity `gran` -- so every partial sum is an exactly representable fp32 value."""
    a = conv64(np.abs(x), np.abs(K), **conv)
    if B is not None:
        a = a + np.abs(_chan(B))
    t = a * (np.abs(_chan(scale)) if scale is not None else 1.0)
    if shift is not None:
        t = t + np.abs(_chan(shift))
    if res is not None:
        t = t + np.abs(_f64(res)).reshape(t.shape)
    top = max(float(a.max(initial=0.0)), float(t.max(initial=0.0)))
    assert top / gran < 2.0 ** 22, "integer operands too large for exact fp32 sums: %g units of %g" % (top / gran, gran)


# ---- per-element bound for float data -----------------------------------------------------------------------------------
# How far, in output pixels along (H, W), a Winograd output's tile can reach: m - 1 for output segments of m.  The input and
# output transforms of a tile mix ALL its inputs, so the rounding error of an output is that of its tile's arithmetic, not of its
# own 3x3 receptive field: an output whose receptive field is all zeros (a ReLU map behind a nearest upsample: blocks of zeros
# over every channel) beside a large neighbour in the same tile gets that neighbour's error -- sqrt(conv(x^2, K^2)) at the
# element itself is 0 there, and the float32 emulation `wino_emulate` is outside the element's own bound (err / tol = inf on
# such maps, tests/test_plan_audit_q4ops.py).  `bound(reach=...)` therefore takes, for the lam term, the largest L2 among the
# outputs that can share a tile with the element, whatever the tiles' alignment: the window of +-(m - 1).  On maps without such
# holes it changes little (the calibration of LAMBDA, on dense maps, is untouched); the emulation stays below 0.12 of it on the
# sparse maps and on calibration_cases alike.
REACH = {"direct": (0, 0), "f2x2": (1, 1), "f4x4": (3, 3), "w1d4": (0, 3), "wino43": (3, 3)}


def _window_max(a, rh, rw, sh=1, sw=1):
    """max of a (N, C, H, W) over the elements up to rh rows and rw columns away from each element, in steps of (sh, sw)."""
    if not rh and not rw:
        return a
    h, w = a.shape[2:]
    p = np.pad(a, ((0, 0), (0, 0), (rh * sh, rh * sh), (rw * sw, rw * sw)))
    out = a
    for i in range(2 * rh + 1):
        for j in range(2 * rw + 1):
            out = np.maximum(out, p[:, :, i * sh:i * sh + h, j * sw:j * sw + w])
    return out


def bound(x, K, B=None, scale=None, shift=None, res=None, lam=LAMBDA["direct"], group=1, reach=(0, 0), **conv):
    """Per-element tolerance of a conv + fused tail whose sums are rounded to fp32 (see the module docstring).  `reach`: REACH of a
    Winograd family, where the element's tile neighbours count (above); (0, 0) is the element's own receptive field.  With
    dilations (d, d) -- a conv that runs by pixel phase on a Winograd kernel -- the neighbours are d pixels apart."""
    x, K = _f64(x), _f64(K)
    kred = K.shape[1] * K.shape[2] * K.shape[3]
    l2 = np.sqrt(_window_max(conv64(x * x, K * K, group=group, **conv), *reach, *[int(d) for d in conv.get("dilations", (1, 1))]))
    a = conv64(np.abs(x), np.abs(K), group=group, **conv)
    if B is not None:
        a = a + np.abs(_chan(B))
    s = np.abs(_chan(scale)) if scale is not None else 1.0
    lin = s * a
    if shift is not None:
        lin = lin + np.abs(_chan(shift))
    if res is not None:
        lin = lin + np.abs(_f64(res)).reshape(lin.shape)
    return lam * U * np.sqrt(kred) * s * l2 + 4 * U * lin


def ratio(y, ref, tol):
    """Element-wise err / tol (0 where both are 0; +-0 compare equal)."""
    y, ref, tol = _f64(y), _f64(ref), _f64(tol)
    err = np.abs(y - ref)
    err = np.where(np.isnan(y) & np.isnan(ref), 0.0, err)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / tol)
    return np.where(np.isnan(r), np.inf, r)


def check(y, ref, tol, what="", plan=""):
    """Fail unless |y - ref| <= tol everywhere; name the worst element as (n, c, y, x) with its err / tol.  -> worst ratio."""
    y = np.asarray(y)
    assert y.shape == ref.shape, "%s [%s]: shape %s != %s" % (what, plan, y.shape, ref.shape)
    if y.size == 0:
        return 0.0
    r = ratio(y, ref, np.broadcast_to(tol, ref.shape))
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    worst = float(r[i])
    assert worst <= 1.0, "%s [%s]: element %s = %r, want %r (err %.3g, tol %.3g, err/tol %.3g)" % (
        what, plan, tuple(int(v) for v in i), float(y[i]), float(ref[i]), abs(float(y[i]) - float(ref[i])),
        float(np.broadcast_to(tol, ref.shape)[i]), worst)
    return worst


def skewed_operands(rng, xs, ks, lo=-10, hi=6, dc=0.0):
    """Float operands whose channels differ in magnitude: per input channel, filter output channel and BN scale a factor
    2^U(lo, hi); `dc` adds a constant offset to the input (stresses the Winograd transforms)."""
    x = rng.standard_normal(xs) * 2.0 ** rng.uniform(lo, hi, (1, xs[1], 1, 1)) + dc
    K = rng.standard_normal(ks) * 2.0 ** rng.uniform(lo, hi, (ks[0], 1, 1, 1)) / np.sqrt(ks[1] * ks[2] * ks[3])
    sc = rng.choice([-1.0, 1.0], ks[0]) * 2.0 ** rng.uniform(lo, hi, ks[0])
    return x.astype(np.float32), K.astype(np.float32), sc.astype(np.float32)


# ---- Winograd emulations (float32, the transforms the kernels document) -------------------------------------------------
# F(m, 3) along one axis: y = A^T [(G g) * (B^T d)], d a segment of m + 2 inputs
_F = {
    # F(1,3): the direct 3-tap sum (a 1-D Winograd conv runs its other axis this way)
    1: (np.eye(3), np.eye(3), np.ones((1, 3))),
    # F(2,3): conv_winograd.hip (wino_filter_kernel)
    2: (np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], float),
        np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]),
        np.array([[1, 1, 1, 0], [0, 1, -1, -1]], float)),
    # F(3,3), points 0, +-1, 2, inf: wino43_kernels.h
    3: (np.array([[2, -1, -2, 1, 0], [0, -2, -1, 1, 0], [0, 2, -3, 1, 0], [0, -1, 0, 1, 0], [0, 2, -1, -2, 1]], float),
        np.array([[1 / 2, 0, 0], [-1 / 2, -1 / 2, -1 / 2], [-1 / 6, 1 / 6, -1 / 6], [1 / 6, 1 / 3, 2 / 3], [0, 0, 1]]),
        np.array([[1, 1, 1, 1, 0], [0, 1, -1, 2, 0], [0, 1, 1, 4, 1]], float)),
    # F(4,3), points 0, +-1, +-2, inf: conv_winograd.hip (F(4x4,3x3)), conv_w1d_kernel.h
    4: (np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                  [0, 4, 0, -5, 0, 1]], float),
        np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
                  [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]),
        np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], float)),
}

# segments of a side: F(2x2) / F(4x4) tiles run past the map's edge; wino43 cuts 7a into a segments of 4 and a of 3
SEGMENTS = {
    "f2x2": lambda n: [2] * -(-n // 2),
    "f4x4": lambda n: [4] * -(-n // 4),
    "wino43": lambda n: [4] * (n // 7) + [3] * (n // 7) if n % 7 == 0 else [4] * -(-n // 4),
}


def wino_emulate(x, K, rows, cols, dtype=np.float32, mats=_F):
    """3x3 / stride 1 / pad 1 conv as Winograd tiles: `rows` / `cols` list the output segment sizes m (keys of _F) along H / W.
    Transforms and the per-frequency channel sums run in `dtype` (float32: an emulation of a kernel's arithmetic; float64:
    the algorithm's exact value).  `mats` maps m to (B^T, G, A^T).  -> (N, Cout, H, W), no bias."""
    x, K = np.asarray(x, dtype), np.asarray(K, dtype)
    n, cin, h, w = x.shape
    cout = K.shape[0]
    H, W = sum(rows), sum(cols)
    xp = np.zeros((n, cin, H + 2, W + 2), dtype)
    xp[:, :, 1:1 + h, 1:1 + w] = x
    out = np.zeros((n, cout, H, W), dtype)
    oy = 0
    for mr in rows:
        BTr, Gr, ATr = (m.astype(dtype) for m in mats[mr])
        ox = 0
        for mc in cols:
            BTc, Gc, ATc = (m.astype(dtype) for m in mats[mc])
            d = xp[:, :, oy:oy + mr + 2, ox:ox + mc + 2]                           # (n, cin, ar, ac)
            V = np.matmul(np.matmul(BTr, d), BTc.T)                                 # (n, cin, fr, fc)
            Uf = np.matmul(np.matmul(Gr, K), Gc.T)                                  # (cout, cin, fr, fc)
            M = np.matmul(Uf.transpose(2, 3, 0, 1)[None], V.transpose(0, 2, 3, 1)[..., None])[..., 0]  # (n, fr, fc, cout)
            M = M.transpose(0, 3, 1, 2)                                             # (n, cout, fr, fc)
            out[:, :, oy:oy + mr, ox:ox + mc] = np.matmul(np.matmul(ATr, M), ATc.T)
            ox += mc
        oy += mr
    return out[:, :, :h, :w]


def wino4_input(x, bt=None):
    """B^T d B of every 6x6 tile of x (pad 1) in float64, in the layout of q4.Wino4In: [36][C/4][T][4], T = (n, tile row,
    tile column), channels zero padded to whole quads.  `bt` replaces B^T (|B^T| bounds the transform of |x|)."""
    bt = _F[4][0] if bt is None else bt
    n, c, h, w = x.shape
    th, tw, cq = -(-h // 4), -(-w // 4), -(-c // 4)
    xp = np.zeros((n, cq * 4, 4 * th + 2, 4 * tw + 2))
    xp[:, :c, 1:1 + h, 1:1 + w] = x
    v = np.zeros((6, 6, n, cq * 4, th, tw))
    for ty in range(th):
        for tx in range(tw):
            d = xp[:, :, 4 * ty:4 * ty + 6, 4 * tx:4 * tx + 6]
            v[:, :, :, :, ty, tx] = np.einsum("ai,ncij,bj->abnc", bt, d, bt)
    return v.reshape(36, n, cq, 4, th * tw).transpose(0, 2, 1, 4, 3).reshape(36, cq, n * th * tw, 4)


def wino_family(fam, h, w):
    """(rows, cols) segment lists of a family on an h x w map; w1d4 is F(1,3) along H and F(4,3) along W."""
    if fam == "w1d4":
        return [1] * h, SEGMENTS["f4x4"](w)
    return SEGMENTS[fam](h), SEGMENTS[fam](w)


def winograd_f2_assert_exact(x, K, B=None, scale=None, shift=None, res=None):
    """The exactness precondition of F(2x2,3x3) on integer operands, on the TRANSFORMED operands: G g G^T has granularity
    0.25 (G's halves), B^T d B is integer; |U| . |V| summed over channels and carried through |A^T| . |A| and the tail stays
    below 2^22 units of 0.25 (and of the tail's own granularity)."""
    rows, cols = wino_family("f2x2", x.shape[2], x.shape[3])
    a = wino_emulate_abs(np.abs(np.asarray(x, np.float64)), np.asarray(K, np.float64), rows, cols)
    if B is not None:
        a = a + np.abs(_chan(B))
    t = a * (np.abs(_chan(scale)) if scale is not None else 1.0)
    if shift is not None:
        t = t + np.abs(_chan(shift))
    if res is not None:
        t = t + np.abs(_f64(res)).reshape(t.shape)
    top = max(float(a.max(initial=0.0)), float(t.max(initial=0.0)))
    assert top / 0.25 < 2.0 ** 22, "F(2x2) transformed operands too large for exact fp32 sums"


def wino_emulate_abs(xabs, K, rows, cols):
    """wino_emulate with every matrix and operand replaced by its absolute value (a bound on every partial sum)."""
    mats = {m: tuple(np.abs(a) for a in f) for m, f in _F.items()}
    return wino_emulate(xabs, np.abs(K), rows, cols, np.float64, mats)


def calibration_cases():
    """(name, x, K) float cases for the lam of every family: N(0,1), per-channel skew 2^U(-10, 6), a DC offset of 50, and
    real channel counts on small maps."""
    rng = np.random.default_rng(2024)
    out = []
    for name, n, cin, h, w, cout, skew, dc in [("normal", 2, 16, 14, 14, 8, False, 0.0), ("skew", 2, 32, 14, 14, 8, True, 0.0),
                                               ("dc50", 2, 32, 14, 14, 8, False, 50.0), ("skew_dc50", 1, 64, 7, 7, 8, True, 50.0),
                                               ("c256", 1, 256, 14, 14, 4, False, 0.0), ("c512_dc", 1, 512, 7, 7, 4, False, 50.0),
                                               ("odd", 3, 5, 9, 13, 6, True, 0.0), ("skew_b32", 32, 32, 14, 14, 32, True, 0.0)]:
        if skew:
            x, K, _ = skewed_operands(rng, (n, cin, h, w), (cout, cin, 3, 3), dc=dc)
        else:
            x = (rng.standard_normal((n, cin, h, w)) + dc).astype(np.float32)
            K = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
        out.append((name, x, K))
    return out


def emulation_ratio(fam, x, K):
    """Worst err / (u sqrt(Kred) L2) of the float32 emulation of `fam` (or the float32 oracle for "direct") on one case."""
    conv = dict(pads=[1, 1, 1, 1])
    want = conv64(x, K, **conv)
    if fam == "direct":
        got = np.ascontiguousarray(onp.conv2d(x, K, **conv))
    else:
        got = wino_emulate(x, K, *wino_family(fam, x.shape[2], x.shape[3]))
    kred = K.shape[1] * 9
    l2 = np.sqrt(conv64(_f64(x) ** 2, _f64(K) ** 2, **conv))
    err = np.abs(_f64(got) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / (U * np.sqrt(kred) * l2))
    return float(r.max())


# ---- geometry sweep -------------------------------------------------------------------------------------------------------
def _conv(group=1, s=(1, 1), d=(1, 1), p=(0, 0)):
    return dict(group=group, strides=list(s), dilations=list(d), pads=[p[0], p[1], p[0], p[1]])


# (name, x shape, K shape, conv parameters): fixed cases where kernels go wrong
FIXED_GEOMETRIES = [
    ("k1x7_s1x2", (2, 6, 9, 17), (8, 6, 1, 7), _conv(s=(1, 2), p=(0, 3))),
    ("k7x1_d2x1", (1, 5, 19, 8), (7, 5, 7, 1), _conv(d=(2, 1), p=(6, 0))),
    ("k3x5_s2x1_d1x2", (3, 4, 11, 13), (9, 4, 3, 5), _conv(s=(2, 1), d=(1, 2), p=(1, 4))),
    ("k3x5_s3x2_d2x3", (1, 8, 16, 20), (5, 8, 3, 5), _conv(s=(3, 2), d=(2, 3), p=(2, 6))),
    ("pad_gt_half", (2, 3, 6, 7), (4, 3, 3, 3), _conv(p=(3, 2))),
    ("map_lt_filter", (1, 4, 2, 3), (6, 4, 5, 5), _conv(p=(2, 2))),
    ("k1_s2_p1", (2, 8, 9, 10), (12, 8, 1, 1), _conv(s=(2, 2), p=(1, 1))),
    ("k1_s3_p1", (1, 16, 11, 7), (20, 16, 1, 1), _conv(s=(3, 3), p=(1, 1))),
    ("g3_cin1_cout1", (2, 3, 8, 9), (3, 1, 3, 3), _conv(group=3, p=(1, 1))),
    ("g4_cin2_cout3", (1, 8, 10, 7), (12, 2, 3, 3), _conv(group=4, p=(1, 1))),
    ("g2_cin3_cout5", (2, 6, 9, 9), (10, 3, 3, 3), _conv(group=2, s=(2, 1), p=(1, 1))),
    ("g3_cin5_cout1", (1, 15, 7, 8), (3, 5, 1, 3), _conv(group=3, p=(0, 1))),
    ("dw_mult2", (2, 5, 9, 8), (10, 1, 3, 3), _conv(group=5, p=(1, 1))),
    ("dw_mult3", (1, 4, 7, 11), (12, 1, 3, 3), _conv(group=4, s=(2, 2), p=(1, 1))),
    ("dw_k3x5_s1x2", (2, 6, 12, 13), (6, 1, 3, 5), _conv(group=6, s=(1, 2), p=(1, 2))),
    ("dw_k7_d2", (1, 8, 15, 16), (8, 1, 7, 7), _conv(group=8, d=(2, 2), p=(6, 6))),
]


def drawn_geometries(count=24, seed=31337):
    """A seeded draw: kh != kw, sh != sw, dh != dw, pads above (k - 1) d / 2, grouped convs of any Cin / group, batch 1 and odd."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        kh, kw = (int(v) for v in rng.choice([1, 2, 3, 5, 7], 2))
        sh, sw = (int(v) for v in rng.choice([1, 1, 2, 3], 2))
        dh = int(rng.choice([1, 1, 2, 3])) if kh > 1 else 1
        dw = int(rng.choice([1, 1, 2, 3])) if kw > 1 else 1
        group = int(rng.choice([1, 1, 2, 3]))
        cin = group * int(rng.choice([1, 2, 3, 4, 5, 8]))
        cout = group * int(rng.choice([1, 3, 4, 5, 8]))
        ph = int(rng.integers(0, (kh - 1) * dh // 2 + 3))
        pw = int(rng.integers(0, (kw - 1) * dw // 2 + 3))
        h = max(int(rng.integers(1, 20)), (kh - 1) * dh + 1 - 2 * ph)
        w = max(int(rng.integers(1, 20)), (kw - 1) * dw + 1 - 2 * pw)
        n = int(rng.choice([1, 2, 3, 5]))
        out.append(("draw%d" % i, (n, cin, h, w), (cout, cin // group, kh, kw), _conv(group, (sh, sw), (dh, dw), (ph, pw))))
    return out


def geometries():
    return FIXED_GEOMETRIES + drawn_geometries()



# ---- operands on which the F(4,3) / F(3,3) Winograd pipelines are exact in fp32 -------------------------------------------------
# Filters whose nonzero taps are +-576 = +-24^2.  The filter kernels (wf4_filter_kernel, wino4_filter_q4_kernel, w43_g, the
# packer of conv_w1d_kernel.h) apply G in two stages with every product rounded on its own (no contraction), e.g.
#     g0 * (1.f/24.f) + g1 * (1.f/12.f) + g2 * (1.f/6.f)        -(g0 + g1 + g2) * (1.f/6.f)
# fl(1/6), fl(1/12), fl(1/24), fl(1/3), fl(2/3) share one mantissa (1.0101...b rounded up) with a relative error of exactly 2^-25,
# less than half an ulp of any product, so fl(c) * (24 m) rounds to the integer 24 m c: stage one leaves multiples of 24, stage
# two integers (1/4 and 1/2 are exact).  B^T and A^T are integer matrices, the inputs integers: where the pipeline with every
# matrix and operand replaced by its absolute value stays below 2^24, every partial sum in any order is an integer below 2^24 and
# so exact -- a kernel of these families must then equal `ref64` in every bit (tests/test_gpu_wino_exact.py).
WINO_TAP = 576.0
WINO_CAP = 2.0 ** 24
# (24 G) of _F[m], integer: U = (24 G) g (24 G)^T / 576 in exact float64 arithmetic
_G24 = {1: 24.0 * np.eye(3), 3: np.rint(24.0 * _F[3][1]), 4: np.rint(24.0 * _F[4][1])}
# the segment sizes (rows, columns) of a family's tiles
WINO_CLASSES = {"f4x4": [(4, 4)], "w1d4": [(1, 4)], "wino43": [(4, 4), (4, 3), (3, 4), (3, 3)]}


def _g_f32(m, g0, g1, g2):
    """G g along the leading axis for F(m, 3), in float32 the way the kernels write it: every product and sum rounded."""
    f = np.float32
    one = f(1.0)
    c2, c4, c6, c12, c24, c3, c23 = f(0.5), f(0.25), one / f(6), one / f(12), one / f(24), one / f(3), f(2) / f(3)
    if m == 1:
        return np.stack([g0, g1, g2])
    if m == 4:
        return np.stack([g0 * c4, -(g0 + g1 + g2) * c6, (-g0 + g1 - g2) * c6, g0 * c24 + g1 * c12 + g2 * c6,
                         g0 * c24 - g1 * c12 + g2 * c6, g2])
    assert m == 3, m
    return np.stack([g0 * c2, -(g0 + g1 + g2) * c2, (-g0 + g1 - g2) * c6, g0 * c6 + g1 * c3 + g2 * c23, g2])


def wino_filter_f32(K, fam):
    """G g G^T of the (Cout, Cin, 3, 3) filter K for every tile class of `fam`, evaluated the way the filter kernels write it:
    G along the filter's rows first, then along its columns, each stage in float32 with separate products.
    -> {(mr, mc): (Cout, Cin, mr + 2 | 3, mc + 2) float32} (a 1-D family keeps its other axis: 3 rows)."""
    K = np.asarray(K, np.float32)
    out = {}
    for mr, mc in WINO_CLASSES[fam]:
        t = _g_f32(mr, K[:, :, 0, :], K[:, :, 1, :], K[:, :, 2, :])                # (fr, co, c, 3)
        u = _g_f32(mc, t[..., 0], t[..., 1], t[..., 2])                            # (fc, fr, co, c)
        assert u.dtype == np.float32
        out[(mr, mc)] = np.ascontiguousarray(u.transpose(2, 3, 1, 0))
    return out


def wino_filter_f64(K, fam):
    """The same U in exact arithmetic: (24 G) g (24 G)^T / 576 on float64 integers -- every step exact where g is integer."""
    K = _f64(K)
    return {(mr, mc): np.einsum("ai,ocij,bj->ocab", _G24[mr], K, _G24[mc]) / 576.0 for mr, mc in WINO_CLASSES[fam]}


def _wino_tiles(xp, rows, cols, mr, mc):
    """The (mr + 2) x (mc + 2) input patches of the tiles of class (mr, mc) in the padded map xp -> (n, c, R, S, mr + 2, mc + 2),
    with the output offsets of the R tile rows and S tile columns."""
    ro = [o for o, m in zip(np.cumsum([0] + rows[:-1]), rows) if m == mr]
    co = [o for o, m in zip(np.cumsum([0] + cols[:-1]), cols) if m == mc]
    ar = 3 if mr == 1 else mr + 2
    iy = np.asarray(ro, int)[:, None] + np.arange(ar)[None]
    ix = np.asarray(co, int)[:, None] + np.arange(mc + 2)[None]
    return xp[:, :, iy[:, None, :, None], ix[None, :, None, :]], ro, co


def wino_pipeline(x, U, fam, dtype, mats=_F, order=None):
    """The tiled pipeline Y = A^T [sum_c U_c * (B^T d_c B)] A of `fam` with the transformed filters U (wino_filter_*) given, all in
    `dtype`, the channel sum as a running sum in `order` (default: ascending).  -> (y, top): y (N, Cout, H, W) without bias, and
    the largest magnitude among V, U, the running sums and y's tiles."""
    x = np.asarray(x, dtype)
    n, cin, h, w = x.shape
    rows, cols = wino_family(fam, h, w)
    H, W = sum(rows), sum(cols)
    xp = np.zeros((n, cin, H + 2, W + 2), dtype)
    xp[:, :, 1:1 + h, 1:1 + w] = x
    cout = next(iter(U.values())).shape[0]
    out = np.zeros((n, cout, H, W), dtype)
    top = 0.0
    for (mr, mc), u in U.items():
        d, ro, co = _wino_tiles(xp, rows, cols, mr, mc)
        if not ro or not co:
            continue
        BTr, _, ATr = (m.astype(dtype) for m in mats[mr])
        BTc, _, ATc = (m.astype(dtype) for m in mats[mc])
        u = np.asarray(u, dtype)
        V = np.einsum("ai,ncrsij,bj->ncrsab", BTr, d, BTc).astype(dtype)
        if order is None and dtype == np.float64:
            # the whole channel sum per frequency at once (a bound: the operands are non-negative, or the sums exact)
            M = np.empty((n, cout) + V.shape[2:], dtype)
            for a in range(V.shape[4]):
                for b in range(V.shape[5]):
                    M[..., a, b] = np.tensordot(V[..., a, b], u[:, :, a, b], axes=([1], [1])).transpose(0, 3, 1, 2)
            top = max(top, float(np.abs(M).max(initial=0.0)))
        else:
            M = np.zeros((n, cout) + V.shape[2:], dtype)
            for c in (range(cin) if order is None else order):
                M += u[None, :, c, None, None] * V[:, None, c]
                top = max(top, float(np.abs(M).max(initial=0.0)))
        assert M.dtype == dtype
        Y = np.einsum("ia,norsab,jb->norsij", ATr, M, ATc).astype(dtype)
        top = max(top, float(np.abs(V).max(initial=0.0)), float(np.abs(u).max(initial=0.0)), float(np.abs(Y).max(initial=0.0)))
        for r, oy in enumerate(ro):
            for s, ox in enumerate(co):
                out[:, :, oy:oy + mr, ox:ox + mc] = Y[:, :, r, s]
    return out[:, :, :h, :w], top


def wino_abs_top(fam, x, K):
    """The cap's left side: the pipeline of `fam` with every matrix and operand replaced by its absolute value (what
    wino_emulate_abs computes tile by tile, here per tile class at once) -> its largest value."""
    mats = {m: tuple(np.abs(a) for a in f) for m, f in _F.items()}
    uabs = {k: np.einsum("ai,ocij,bj->ocab", np.abs(_F[k[0]][1]), np.abs(_f64(K)), np.abs(_F[k[1]][1])) for k in WINO_CLASSES[fam]}
    return wino_pipeline(np.abs(_f64(x)), uabs, fam, np.float64, mats)[1]


def wino_exact_operands(rng, xs, cout, bias=False, bn=False, res=False):
    """Operands on which the F(4,3) / F(3,3) pipelines are exact (above) for a 3x3 / pad 1 conv of input xs -> (x, K, B, scale,
    shift, res).  Narrow recipe (Cin <= 20): per output channel min(Cin, 12) randomly chosen input channels carry two random taps
    of +-576 each, x in [-2, 2] ([-3, 3] for Cin <= 8).  Wide recipe (Cin above 20; meant for 64 .. 256): 24 input channels per
    output channel, one tap each, x in [-1, 1].  The live channels differ per output channel, so that no K chunk is idle."""
    n, cin, h, w = xs
    narrow = cin <= 20
    live, taps, xmax = (min(cin, 12), 2, 3 if cin <= 8 else 2) if narrow else (min(cin, 24), 1, 1)
    x = int_tensor(rng, xs, -xmax, xmax)
    K = np.zeros((cout, cin, 9), np.float32)
    for co in range(cout):
        for c in rng.choice(cin, live, replace=False):
            K[co, c, rng.choice(9, taps, replace=False)] = rng.choice([-WINO_TAP, WINO_TAP], taps)
    return (x, K.reshape(cout, cin, 3, 3)) + int_tail(rng, cout, (n, cout, h, w), bias, bn, res)


def wino_exact_assert(fam, x, K, B=None, scale=None, shift=None, res=None):
    """The precondition of bit-exactness for family `fam` in {"f4x4", "w1d4", "wino43"}: the filter transform as the kernels
    evaluate it (wino_filter_f32) equals the exact U and is integer; the pipeline in absolute values stays below 2^24; and the
    tail's absolute bound -- conv(|x|, |K|) + |B| through max(|scale|, 1), |shift| and |res|, which covers the tail with any of
    its terms left out -- stays below 2^24 units of 0.25 * ALPHA (the finest grain: a leaky value in quarters times 1/8)."""
    u32, u64 = wino_filter_f32(K, fam), wino_filter_f64(K, fam)
    for k in u64:
        assert u32[k].dtype == np.float32 and u32[k].shape == u64[k].shape, k
        np.testing.assert_array_equal(u32[k].astype(np.float64), u64[k], err_msg="%s filter transform, class %s" % (fam, k))
        assert np.all(u64[k] == np.rint(u64[k])), "%s: U is not integer" % fam
    assert np.all(_f64(x) == np.rint(_f64(x))), "x is not integer"
    top = wino_abs_top(fam, x, K)
    assert top < WINO_CAP, "%s: |pipeline| reaches %g = %.3f * 2^24" % (fam, top, top / WINO_CAP)
    t = conv64(np.abs(x), np.abs(K), pads=[1, 1, 1, 1])
    if B is not None:
        t = t + np.abs(_chan(B))
    if scale is not None:
        t = t * np.maximum(np.abs(_chan(scale)), 1.0)
    if shift is not None:
        t = t + np.abs(_chan(shift))
    if res is not None:
        t = t + np.abs(_f64(res)).reshape(t.shape)
    tail = float(t.max(initial=0.0)) / (0.25 * ALPHA)
    assert tail < WINO_CAP, "%s: the tail reaches %g units of 1/32" % (fam, tail)
    return top / WINO_CAP


def wino43_input(x, absolute=False):
    """B^T d B of every mixed tile of x (pad 1; sides 7, 14 or 21) in float64, in the layout of q4.Wino43In: [121][C/4][T][4] --
    frequency groups 0..35 the F(4)xF(4) tiles, 36..65 F(4) rows x F(3) columns, 66..95 F(3) x F(4), 96..120 F(3) x F(3), each
    a * nb + b; T = (n, tile row, tile column) of the class, H/7 x W/7 tiles an image; channels zero padded to whole quads.
    `absolute`: |B^T| in place of B^T (a bound on the transform of |x|)."""
    n, c, h, w = x.shape
    ar, ac, cq = h // 7, w // 7, -(-c // 4)
    xp = np.zeros((n, cq * 4, h + 2, w + 2))
    xp[:, :c, 1:1 + h, 1:1 + w] = x
    rows, cols = SEGMENTS["wino43"](h), SEGMENTS["wino43"](w)
    out = np.zeros((121, cq, n * ar * ac, 4))
    fb = {(4, 4): 0, (4, 3): 36, (3, 4): 66, (3, 3): 96}
    for (mr, mc), base in fb.items():
        d, ro, co = _wino_tiles(xp, rows, cols, mr, mc)                              # (n, C, ar, ac, mr + 2, mc + 2)
        btr, btc = _F[mr][0], _F[mc][0]
        if absolute:
            btr, btc = np.abs(btr), np.abs(btc)
        v = np.einsum("ai,ncrsij,bj->abncrs", btr, d, btc)
        v = v.reshape((mr + 2) * (mc + 2), n, cq, 4, ar * ac).transpose(0, 2, 1, 4, 3)
        out[base:base + (mr + 2) * (mc + 2)] = v.reshape(-1, cq, n * ar * ac, 4)
    return out

"""One non-finite value planted in otherwise valid conv operands: which outputs may change, which must, and how.

A plant is (tensor, index, value) with value in {NaN, +inf, -inf} and tensor one of x, K, B, scale, shift, res.  For a case of
`CASES` and its float64 reference (tests/ref64.py, or the reference of the family's own test file) three masks over every output:

* must  -- where the float64 reference of the poisoned operands is non-finite; `cls` is its IEEE class there;
* may   -- must for the direct families; for a Winograd family where `ref64.wino_emulate(..., dtype=float64)` with the family's
           segments (`ref64.wino_family`) is non-finite -- whole tiles, by construction of the transforms; for a conv folded by
           dilation (d, d) the same on each pixel phase; for the second conv of a chain the tiles that read a may element of the
           first; for the pooled stems the pooling windows that read a may element; for conv1x1 + Winograd-in every frequency of
           the 6x6 tiles that hold a may pixel (must: the frequencies whose B^T coefficients on that pixel are not 0 -- numpy's
           0 x NaN in `ref64.wino4_input` would claim the others too, and a kernel that adds and subtracts rows is not wrong);
* clean -- everything else.

The rules, for an output y against the SAME implementation's run y0 on the clean operands (`check`):

* R1 containment: y and y0 have the same bits on clean;
* R2 propagation: y is non-finite on must;
* R3 class: on the direct families y is NaN / +inf / -inf exactly as cls says (a single inf meets no opposite inf, so the class is
  determined through bias, BN, residual and both activations); on the Winograd families and behind the input transform of
  conv1x1 + Winograd-in a NaN plant gives NaN on must, an inf plant a non-finite value;
* R4 pooled stems: R2 on the pooling windows that read a NaN or a +inf BEFORE the activation -- the pool's maximum propagates a NaN
  and a +inf wins it, and both activations keep them, whichever side of the pool the activation runs on.  A -inf before the
  activation is free: it loses the max-pool to a finite neighbour, the pool's zero padding or its -1e4 start, and the stem kernels
  run the ReLU of a scale + shift + ReLU tail BEHIND the pool (csrc/conv_stem_pool_kernel.h: max and x (x > 0) commute on every
  value but -inf, which the reference turns into NaN first).  Its windows are in may, not in must;
* a filter plant K[co, ...] = NaN: may is channel co, must the outputs of channel co whose tap lies inside the image (the
  reference of a ones image under the one-hot filter); the outputs whose tap falls on padding are free (0 x NaN in the reference, and
  a kernel that skips padding taps is not wrong).

There is no constant here: every comparison is by bits or by class.  `sweep` asserts its own preconditions (no zero filter value,
scale or alpha; y0 finite; clean and must non-empty)."""
import collections

import numpy as np

from oracle import planer_np as onp
from tests import ref64 as R
from tests.ref64 import ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_RES_AFTER
from tests.test_gpu_conv_bounds import ALPHA, TAILS, _full, _operands

VALUES = collections.OrderedDict([("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)])
Plant = collections.namedtuple("Plant", "tensor index value")
TENSORS = ("x", "K", "B", "scale", "shift", "res")
POOL = dict(w=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2])
# tails of the entry points that take no residual (the pooled stems, conv1x1 + Winograd-in) or a bias alone (small-Cin, Dense),
# as tests/test_gpu_conv_bounds.py runs them
POOL_TAILS = [(False, True, False, ACT_RELU), (True, True, False, ACT_LEAKY), (True, False, False, ACT_NONE)]
C1W_TAILS = [(True, True, False, ACT_LEAKY), (False, True, False, ACT_RELU)]
BIAS_TAIL = [(True, False, False, ACT_NONE)]
PAIR1_TAIL, PAIR2_TAIL = (False, True, False, ACT_RELU), (True, True, False, ACT_NONE)


def classes(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    a = np.asarray(a)
    return np.where(np.isnan(a), 1, np.where(a == np.inf, 2, np.where(a == -np.inf, 3, 0))).astype(np.int8)


def poison(ops, plant):
    """A copy of the operand tuple (x, K, B, scale, shift, res, ...) with the plant's value at its index."""
    ops = list(ops)
    i = TENSORS.index(plant.tensor)
    a = np.array(ops[i], copy=True)
    a[plant.index] = VALUES[plant.value]
    ops[i] = a
    return tuple(ops)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
class Case:
    """kind: which reference (conv, convt, pool, c1w, pair, chain).  fam: "direct" or a Winograd family of ref64.SEGMENTS.  tails:
    the fused tails of the entry point; intails: the indices of those the input plants run under (the last takes the filter plants)."""

    def __init__(self, name, kind, xs, ks, conv=None, fam="direct", tails=TAILS, intails=(1, 2), **extra):
        self.name, self.kind, self.xs, self.ks, self.fam, self.tails, self.intails = name, kind, xs, ks, fam, tails, intails
        self.conv = _full(conv or {})
        self.extra = extra
        self.fold = extra.get("fold", 1)
        self._ops, self._masks = {}, {}

    def __repr__(self):
        return self.name

    def operands(self, t):
        """-> ((x, K, B, scale, shift, res, ...), act) of tail t, made once."""
        if t not in self._ops:
            self._ops[t] = _make_operands(self, self.tails[t])
        return self._ops[t]


def _stuffed_geometry(case):
    """ConvTranspose as the stride-1 conv of the zero-stuffed input (tests/test_gpu_convtranspose.py::stuffed)."""
    s, pads, op = case.extra["strides"], case.extra["pads"], case.extra["output_padding"]
    kh, kw = case.ks[2:]
    lo_h, hi_h = kh - 1 - pads[0], kh - 1 - pads[2] + op[0]
    lo_w, hi_w = kw - 1 - pads[1], kw - 1 - pads[3] + op[1]
    n, c, h, w = case.xs
    return (n, c, (h - 1) * s[0] + lo_h + hi_h + 1, (w - 1) * s[1] + lo_w + hi_w + 1), (lo_h, lo_w)


def _make_operands(case, tail):
    if case.kind == "convt":
        # the skewed operands of the equivalent stride-1 conv; x its samples at the stuffed positions, K the filter un-flipped
        bs, (lo_h, lo_w) = _stuffed_geometry(case)
        ci, co, kh, kw = case.ks
        (xb, Kt, B, sc, sh, r), act, _ = _operands(case.name, bs, (co, ci, kh, kw), tail)
        s, (n, c, h, w) = case.extra["strides"], case.xs
        x = np.ascontiguousarray(xb[:, :, lo_h::s[0], lo_w::s[1]][:, :, :h, :w])
        K = np.ascontiguousarray(Kt[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))
        return (x, K, B, sc, sh, r), act
    if case.kind == "pair":
        ops1, act1, _ = _operands(case.name + "1", case.xs, case.ks, PAIR1_TAIL, **case.conv)
        ops2, act2, _ = _operands(case.name + "2", case.xs, case.extra["ks2"], PAIR2_TAIL, **case.extra["conv2"])
        return ops1 + ops2[1:], (act1, act2)          # (x, K1, B1, s1, t1, r1, K2, B2, s2, t2, r2)
    ops, act, _ = _operands(case.name, case.xs, case.ks, tail, **case.conv)
    if case.kind == "chain":                          # + the second conv's filter, scale and shift (its tail: BN + ReLU)
        c = case.ks[0]
        rng = np.random.default_rng(c * 1000 + case.xs[2])
        K2 = (rng.standard_normal((c, c, 3, 3)) / np.sqrt(9 * c)).astype(np.float32)
        sc2 = (rng.choice([-1.0, 1.0], c) * 2.0 ** rng.uniform(-10, 6, c)).astype(np.float32)
        ops = ops + (K2, sc2, rng.standard_normal(c).astype(np.float32))
    return ops, act


def preconditions(case, ops, act):
    """No filter value, scale or alpha of the case is 0: otherwise `must` would depend on luck."""
    at = {"pair": (1, 3, 6, 8), "chain": (1, 3, 6, 7)}.get(case.kind, (1, 3))
    for i in at:
        assert ops[i] is None or np.all(np.asarray(ops[i]) != 0), "%s: operand %d holds a zero" % (case, i)
    assert ALPHA != 0


# ---- references and CPU implementations ------------------------------------------------------------------------------------------
def wino_conv(x, K, fam, dtype, d=1):
    """The family's tiling (ref64.wino_emulate) in `dtype`, by pixel phase for a conv folded by dilation (d, d)."""
    if d == 1:
        return R.wino_emulate(x, K, *R.wino_family(fam, *x.shape[2:]), dtype=dtype)
    out = np.zeros((x.shape[0], K.shape[0]) + x.shape[2:], dtype)
    for i in range(d):
        for j in range(d):
            p = np.ascontiguousarray(x[:, :, i::d, j::d])
            out[:, :, i::d, j::d] = R.wino_emulate(p, K, *R.wino_family(fam, *p.shape[2:]), dtype=dtype)
    return out


def tail_as(y, B, scale, shift, res, act, alpha, dtype):
    """ref64.tail64, in float32 where asked: the arithmetic of apply_epilogue."""
    if dtype == np.float64:
        return R.tail64(y, B, scale, shift, res, act, alpha)
    f = lambda a: None if a is None else np.asarray(a, dtype)
    ch = lambda a: None if a is None else f(a).reshape(1, -1, 1, 1)
    y = np.array(y, dtype=dtype)
    one, a = dtype(1.0), dtype(alpha)
    if B is not None:
        y = y + ch(B)
    if scale is not None:
        y = y * ch(scale)
    if shift is not None:
        y = y + ch(shift)
    post, kind = act & ACT_RES_AFTER, act & 15
    if res is not None and not post:
        y = y + f(res).reshape(y.shape)
    if kind == ACT_RELU:
        y = y * (y > 0).astype(dtype)
    elif kind == ACT_LEAKY:
        y = y * ((y > 0).astype(dtype) * (one - a) + a)
    if res is not None and post:
        y = y + f(res).reshape(y.shape)
    return y


_MEMO = collections.OrderedDict()


def raw_conv(case, x, K, dtype, wino, conv=None):
    """The conv alone in `dtype`: the oracle's conv (in float64: ref64.conv64), or with `wino` the family's tiling.  The last few
    results are kept by operand identity (a tail plant leaves x and K as they are)."""
    key = (case.name, id(x), id(K), np.dtype(dtype).str, bool(wino), conv is None)
    if key in _MEMO and _MEMO[key][0] is x and _MEMO[key][1] is K:
        return _MEMO[key][2]
    x0, K0 = x, K
    conv = case.conv if conv is None else conv
    if case.kind == "convt":
        from tests.test_gpu_convtranspose import stuffed
        x, K = stuffed(np.asarray(x), np.asarray(K), case.extra["strides"], case.extra["pads"], case.extra["output_padding"])
        conv = _full({})
    with np.errstate(invalid="ignore"):
        if wino and case.fam != "direct":
            y = wino_conv(x, K, case.fam, dtype, case.fold)
        else:
            y = np.ascontiguousarray(onp.conv2d(np.asarray(x, dtype), np.asarray(K, dtype), None, **conv))
    _MEMO[key] = (x0, K0, y)
    while len(_MEMO) > 8:
        _MEMO.popitem(last=False)
    return y


def stages(case, ops, act, dtype=np.float64, wino=False, raw=None):
    """Every conv + tail of the case as NCHW maps, before the max-pool or the input transform -> list of arrays.  dtype float64,
    wino False: the reference.  float32: an implementation that exists on the CPU (the float32 oracle conv, or with `wino` the float32
    Winograd emulation).  `raw` replaces raw_conv (the negative controls)."""
    raw = raw or raw_conv
    with np.errstate(invalid="ignore", over="ignore"):
        if case.kind == "pair":
            x, K1, B1, s1, t1, r1, K2, B2, s2, t2, r2 = ops
            return [tail_as(raw(case, x, K1, dtype, wino, None), B1, s1, t1, r1, act[0], ALPHA, dtype),
                    tail_as(raw(case, x, K2, dtype, wino, case.extra["conv2"]), B2, s2, t2, r2, act[1], ALPHA, dtype)]
        if case.kind == "chain":
            x, K, B, sc, sh, r, K2, sc2, sh2 = ops
            y1 = tail_as(raw(case, x, K, dtype, wino, None), B, sc, sh, r, act, ALPHA, dtype)
            return [y1, tail_as(raw(case, y1, K2, dtype, wino, None), None, sc2, sh2, None, ACT_RELU, ALPHA, dtype)]
        x, K, B, sc, sh, r = ops
        return [tail_as(raw(case, x, K, dtype, wino, None), B, sc, sh, r, act, ALPHA, dtype)]


def finish(case, ys):
    """The stage behind the conv: the 3x3 / s2 / p1 max-pool of the stems, B^T d B of conv1x1 + Winograd-in."""
    with np.errstate(invalid="ignore"):
        if case.kind == "pool":
            return [onp.maxpool(ys[0], **POOL)]
        if case.kind == "c1w":
            return [R.wino4_input(ys[0]).astype(ys[0].dtype)]
    return ys


def compute(case, ops, act, dtype=np.float64, wino=False, raw=None):
    return finish(case, stages(case, ops, act, dtype, wino, raw))


def _pool_reads(mask):
    """The pooling windows that read an element of the mask."""
    return onp.maxpool(mask.astype(np.float64), **POOL) > 0


def _behind(case, must, may, ref, pre=None):
    """Masks of a conv stage carried through the stage behind it -> (must, may, cls).  pre: the stage before its activation."""
    if case.kind == "pool":
        strong = np.isnan(pre) | (pre == np.inf)
        assert not (strong & ~must).any()
        return _pool_reads(strong), _pool_reads(may), None
    if case.kind == "c1w":
        reads = (R._F[4][0] != 0).astype(np.float64)
        return R.wino4_input(must.astype(np.float64), reads) > 0, R.wino4_input(may.astype(np.float64), np.ones((6, 6))) > 0, None
    return must, may, classes(ref)


def masks(case, t, plant):
    """-> (poisoned operands, [(must, may, cls)] per output) of a plant outside the filter; made once per (tail, plant)."""
    key = (t, plant)
    if key not in case._masks:
        ops, act = case.operands(t)
        bad = poison(ops, plant)
        ref = stages(case, bad, act)
        pre = stages(case, bad, ACT_NONE)[0] if case.kind == "pool" else None
        tiled = stages(case, bad, act, wino=True) if case.fam != "direct" and plant.tensor == "x" else None
        out = []
        for i, y in enumerate(ref):
            must = ~np.isfinite(y)
            may = must.copy()
            if tiled is not None:
                may |= ~np.isfinite(tiled[i])
            elif case.kind == "chain" and i == 1:
                # behind a tail plant of the first conv: the tiles of the second that read a non-finite element of the first
                may |= ~np.isfinite(wino_conv(np.where(out[0][1], np.nan, 0.0), np.ones(ops[6].shape), case.fam, np.float64))
            out.append(_behind(case, must, may, y, pre))
        case._masks[key] = (bad, out)
    return case._masks[key]


def filter_masks(case, ops, plant):
    """A NaN at K[index] of the (first) conv -> (must, may): may is channel co, must the outputs of channel co whose tap lies
    inside the image."""
    onehot = np.zeros(ops[1].shape)
    onehot[plant.index] = 1.0
    co = plant.index[1] if case.kind == "convt" else plant.index[0]
    reach = raw_conv(case, np.ones(case.xs), onehot, np.float64, False) != 0
    assert reach[:, co].any() and not np.delete(reach, co, axis=1).any()
    may = np.zeros(reach.shape, bool)
    may[:, co] = True
    return _behind(case, reach, may, reach.astype(np.float64), np.where(reach, np.nan, 0.0))[:2]


# ---- the plants ---------------------------------------------------------------------------------------------------------------------
def _read(axis, xs, ks, conv, tap=None):
    """The input rows (axis 0) or columns (axis 1) that some output of the conv reads (through filter row / column `tap` alone)."""
    size, k = xs[2 + axis], ks[2 + axis]
    s, d, lo, hi = conv["strides"][axis], conv["dilations"][axis], conv["pads"][axis], conv["pads"][2 + axis]
    outs = (size + lo + hi - d * (k - 1) - 1) // s + 1
    taps = range(k) if tap is None else (tap,)
    return sorted({o * s - lo + i * d for o in range(outs) for i in taps} & set(range(size)))


def input_plants(case):
    """(n, channel, h, w) of the planted pixels: the corners, one pixel on each side of the first tile boundary in both axes (both
    boundaries of the 4 + 3 segments; in a folded conv on its first pixel phase), the last pixel of the last (partial) tile, the last
    pixel of image 0 and the first of image 1; over channels 0, Cin - 1, 15 and 16 where Cin >= 32, and the two channels at a group
    boundary -- every pixel and every channel of these lists at least once."""
    n, c, h, w = case.xs
    edges = {"f2x2": (1, 2), "wino43": (3, 4, 6, 7)}.get(case.fam, (3, 4))
    pix = ([(0, 0, 0), (n - 1, h - 1, w - 1)] + [(0, e * case.fold, e * case.fold) for e in edges]
           + [(0, h - 1, w - 1), (min(1, n - 1), 0, 0)])
    pix = [p for p in pix if p[1] < h and p[2] < w]
    if case.kind != "convt":                # a strided conv skips pixels: the nearest one above / left of it that some output reads
        rows, cols = (set(_read(a, case.xs, case.ks, case.conv)) for a in (0, 1))
        if case.kind == "pair":             # (pixels that both siblings read)
            rows, cols = (v & set(_read(a, case.xs, case.extra["ks2"], case.extra["conv2"])) for a, v in ((0, rows), (1, cols)))
        pix = [(i, max(r for r in rows if r <= y), max(c for c in cols if c <= x)) for i, y, x in pix]
    pix = list(dict.fromkeys(pix))
    chans = [0, c - 1] + ([15, 16] if c >= 32 else [])
    g = case.conv["group"]
    if 1 < g < c:
        chans += [c // g - 1, c // g]
    chans = list(dict.fromkeys(ch for ch in chans if 0 <= ch < c))
    out = []
    for i in range(max(len(pix), len(chans))):
        nn, hh, ww = pix[i % len(pix)]
        out.append((nn, chans[i % len(chans)], hh, ww))
    return list(dict.fromkeys(out))


def tail_channels(cout):
    return list(dict.fromkeys([0, cout - 1] + ([63, 64] if cout > 64 else [])))


def filter_plants(case, K):
    """K[co, ci, i, j] = NaN for co in {0, Cout - 1, 63 and 64 where Cout > 64}: a corner tap of the last input channel and the
    centre tap of the first ([ci, co, i, j] in a transposed conv's filter).  Under a dilation wider than the map the corner tap
    never meets the image: the outermost tap that does."""
    convt = case.kind == "convt"
    cout, cin, kh, kw = K.shape[1 if convt else 0], K.shape[0 if convt else 1], K.shape[2], K.shape[3]
    corner = (0, 0) if convt else tuple(next(i for i in range(k) if _read(a, case.xs, case.ks, case.conv, i))
                                         for a, k in ((0, kh), (1, kw)))
    out = []
    for co in tail_channels(cout):
        for tap, ci in ((corner, cin - 1), ((kh // 2, kw // 2), 0)):
            out.append(Plant("K", ((ci, co) if convt else (co, ci)) + tap, "nan"))
    return list(dict.fromkeys(out))


def plants(case, t, ops, tensors=TENSORS):
    """Every plant of tail t: input pixels under the tails of `intails`, x every value; the filter plants under the last of them;
    B, scale and shift of the filter plants' channels and one residual element at the quad-padding boundary under every tail that
    has the term."""
    out = []
    if "x" in tensors and t in case.intails:
        out += [Plant("x", idx, v) for idx in input_plants(case) for v in VALUES]
    if "K" in tensors and t == case.intails[-1]:
        out += filter_plants(case, ops[1])
    cout = case.ks[1] if case.kind == "convt" else case.ks[0]
    for name in ("B", "scale", "shift"):
        if name in tensors and ops[TENSORS.index(name)] is not None:
            out += [Plant(name, (co,), v) for co in tail_channels(cout) for v in VALUES]
    if "res" in tensors and ops[5] is not None:
        n, c, h, w = ops[5].shape
        out += [Plant("res", (n - 1, c - 1, h // 2, w - 1), v) for v in VALUES]
    return out


# ---- the rules --------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _first(mask):
    return tuple(int(v) for v in np.argwhere(mask)[0])


def same_bits(y, y0, what):
    assert (_bits(y) == _bits(y0)).all(), "R1 %s: an output the plant cannot reach changed" % what


def check(y, y0, must, may, cls, value, what):
    """R1 - R3 for one output (R4: the pooled stems' must).  cls: the reference's classes for R3 by class, or None (a NaN plant:
    NaN on must; an inf: non-finite)."""
    y, y0 = np.asarray(y), np.asarray(y0)
    assert y.shape == y0.shape == must.shape == may.shape, (what, y.shape, y0.shape, must.shape, may.shape)
    assert y.dtype == y0.dtype and np.isfinite(y0).all(), "%s: the clean run is not finite" % what
    assert not (must & ~may).any(), "%s: must outside may" % what
    diff = (_bits(y) != _bits(y0)) & ~may
    assert not diff.any(), "R1 %s: %d clean elements changed, first at %s (%r -> %r)" % (
        what, diff.sum(), _first(diff), float(y0[_first(diff)]), float(y[_first(diff)]))
    got = classes(y)
    fin = must & (got == 0)
    assert not fin.any(), "R2 %s: %d finite values on must, first at %s" % (what, fin.sum(), _first(fin))
    if cls is not None:
        bad = must & (got != cls)
        assert not bad.any(), "R3 %s: %d of %d classes differ, first at %s: %r, reference class %d" % (
            what, bad.sum(), must.sum(), _first(bad), float(y[_first(bad)]), int(cls[_first(bad)]))
    elif value == "nan":
        assert (got[must] == 1).all(), "R3 %s: a NaN plant gave an inf on must" % what


def padding_lanes(raw_q4, chan, what):
    """The raw Q4 result (N, ceil(C/4), H, W, 4) -> NCHW; the lanes of a partial quad past `chan` are +0.0 bit for bit."""
    raw = np.asarray(raw_q4)
    n, cq, h, w, _ = raw.shape
    nchw = raw.transpose(0, 1, 4, 2, 3).reshape(n, cq * 4, h, w)
    assert not _bits(nchw[:, chan:]).any(), "%s: a padding lane of the last channel quad is not +0.0" % what
    return np.ascontiguousarray(nchw[:, :chan])


def sweep(case, run, tensors=TENSORS, label="", seen=None):
    """Every plant of the case through `run(ops, act, what) -> list of outputs` (on the clean operands first, then once per plant);
    asserts the preconditions and R1 - R4.  -> number of plants.  `seen`: a set that collects the planted tensors."""
    strict = case.fam == "direct" and case.kind not in ("pool", "c1w")
    count = 0
    for t in range(len(case.tails)):
        ops, act = case.operands(t)
        preconditions(case, ops, act)
        y0 = run(ops, act, "%s%s tail %d clean" % (label, case, t))
        for plant in plants(case, t, ops, tensors):
            what = "%s%s tail %d %s%s=%s" % (label, case, t, plant.tensor, list(plant.index), plant.value)
            if plant.tensor == "K":
                must, may = filter_masks(case, ops, plant)
                y = run(poison(ops, plant), act, what)
                assert must.any() and not may.all(), what
                check(y[0], y0[0], must, may, None, "nan", what)
                if case.kind == "pair":                 # the sibling keeps its bits (a chain's second conv reads channel co)
                    same_bits(y[1], y0[1], what + " out 1")
            else:
                bad, ms = masks(case, t, plant)
                y = run(bad, act, what)
                assert len(y) == len(ms), what
                # (a -inf before the activation can lose every max of the pooled stems: there R1 alone is left)
                assert ms[0][0].any() or (case.kind == "pool" and plant.value != "nan"), "%s: must is empty" % what
                for k, (must, may, cls) in enumerate(ms):
                    if plant.tensor == "res" and k == 0:
                        assert must.sum() == 1 and may.sum() == 1, what
                    if plant.tensor == "x" and case.kind != "pool":
                        assert must.any(), "%s: the plant does not reach output %d" % (what, k)
                    # (a tail plant of a chain's first conv reaches every tile of the second)
                    assert not may.all() or (case.kind == "chain" and k == 1), "%s: no clean element in output %d" % (what, k)
                    check(y[k], y0[k], must, may, cls if strict else None, plant.value, "%s out %d" % (what, k))
            count += 1
            if seen is not None:
                seen.add(plant.tensor)
    return count


# ---- the table: the smallest shapes at which every kernel path of tests/test_gpu_conv_nonfinite.py still exists -------------------
def _geom(name):
    return next(g for g in R.geometries() if g[0] == name)[1:]


P1 = dict(pads=[1, 1, 1, 1])
WINO_SHAPES = [((3, 16, 9, 13), 24, 1, ("f2x2", "f4x4", "w1d4")),                 # partial tiles on both axes
               ((2, 8, 14, 14), 8, 1, ("f2x2", "f4x4", "w1d4", "wino43")),        # the 4 + 3 segments
               ((1, 8, 21, 21), 8, 1, ("f2x2", "f4x4", "w1d4", "wino43")),
               ((2, 32, 28, 28), 32, 1, ("f2x2", "f4x4", "w1d4")),                # the fused kernel's multi-patch blocks
               ((2, 8, 12, 12), 8, 2, ("f2x2", "f4x4", "w1d4"))]                  # dilation 2, folded by pixel phase
CASES = collections.OrderedDict((c.name, c) for c in [
    # direct: partial quads in Cin and Cout; geometries of tests/test_gpu_conv_bounds.py; its strided 1x1 cut down
    Case("d_6to10", "conv", (2, 6, 9, 11), (10, 6, 3, 3), P1),
    Case("k3x5_s2x1_d1x2", "conv", *_geom("k3x5_s2x1_d1x2")),
    Case("k1x7_s1x2", "conv", *_geom("k1x7_s1x2")),
    Case("g2_cin3_cout5", "conv", *_geom("g2_cin3_cout5")),
    Case("c32_1x1_s2", "conv", (2, 32, 6, 6), (40, 32, 1, 1), dict(strides=[2, 2])),
    Case("cfg", "conv", (2, 32, 14, 14), (40, 32, 3, 3), P1),
    Case("hybrid", "conv", (3, 64, 28, 28), (128, 64, 3, 3), P1),
    Case("rowpack", "conv", (2, 3, 33, 35), (20, 3, 7, 7), dict(strides=[2, 2], pads=[3, 3, 3, 3])),
    Case("stem", "pool", (1, 3, 50, 36), (36, 3, 7, 7), dict(strides=[2, 2], pads=[3, 3, 3, 3]), tails=POOL_TAILS, intails=(2, 1)),
    Case("smallcin_2to70", "conv", (1, 2, 17, 44), (70, 2, 3, 3), P1, tails=BIAS_TAIL, intails=(0,)),
    Case("smallcin_1to20", "conv", (3, 1, 9, 16), (20, 1, 3, 3), P1, tails=BIAS_TAIL, intails=(0,)),
    Case("dw_7x7_d8", "conv", (3, 5, 17, 19), (5, 1, 7, 7), dict(group=5, dilations=[8, 8], pads=[24, 24, 24, 24])),
    Case("dw_3x5_s2x1_d1x2", "conv", (3, 36, 17, 19), (36, 1, 3, 5),
         dict(group=36, strides=[2, 1], dilations=[1, 2], pads=[1, 4, 1, 4])),
    Case("convt_k3_even", "convt", (3, 5, 5, 6), (5, 5, 3, 3), strides=(2, 2), pads=(1, 1, 1, 1), output_padding=(1, 1)),
    Case("convt_k3_odd", "convt", (1, 3, 4, 5), (3, 5, 3, 3), strides=(2, 2), pads=(1, 1, 1, 1), output_padding=(0, 0)),
    Case("pair", "pair", (2, 8, 9, 11), (12, 8, 3, 3), dict(strides=[2, 2], pads=[1, 1, 1, 1]), tails=[None], intails=(0,),
         ks2=(16, 8, 1, 1), conv2=_full(dict(strides=[2, 2]))),
    Case("dense_5x72x40", "conv", (5, 72, 1, 1), (40, 72, 1, 1), tails=BIAS_TAIL, intails=(0,)),
    Case("dense_65x96x255", "conv", (65, 96, 1, 1), (255, 96, 1, 1), tails=BIAS_TAIL, intails=(0,)),
    Case("c1w", "c1w", (3, 4, 9, 13), (12, 4, 1, 1), tails=C1W_TAILS, intails=(0, 1)),
] + [
    Case("%s_%s%s" % (fam, "x".join(map(str, xs)), "_d%d" % d if d > 1 else ""), "conv", xs, (co, xs[1], 3, 3),
         dict(pads=[d, d, d, d], dilations=[d, d]), fam=fam, fold=d)
    for xs, co, d, fams in WINO_SHAPES for fam in fams
] + [
    Case("chain_f4x4", "chain", (2, 8, 14, 14), (8, 8, 3, 3), P1, fam="f4x4"),
    Case("chain_wino43", "chain", (2, 8, 14, 14), (8, 8, 3, 3), P1, fam="wino43"),
])

"""NaN, +-inf, +-0, subnormals and +-1e4 (the max-pool's initial value) through every non-conv kernel, NCHW and Q4, against
the oracle (oracle/planer_np.py) bit for bit: outputs are compared as uint32 patterns, NaNs as a class.

Data: integer base values with special values sprinkled in.  Where an op sums (average pools, GAP, ReduceSum / Mean, linear
upsampling) the base stays integer and the specials exclude subnormals and the neighbours of +-1e4, so every finite partial sum
is exact whatever the order; transcendental ops get the special values alone, whose results every libm gets exactly.

Max and min (pools, ReduceMax / Min) follow IEEE 754-2019 maximum / minimum on the GPU: a NaN propagates like np.maximum,
and -0 < +0.  numpy's result for a +0 / -0 tie depends on the order it visits the operands (np.maximum returns its second
operand on a tie; np.max's vector loop its own way), so those ops are compared with `ieee_max_ref` -- the oracle run in
float64 with -0 mapped to -1e-300 -- and the one named divergence from numpy, ZERO_SIGN_TIE, is asserted to be all that
differs.

The last cases are the empty extents: numpy's answer (or its exception type) without a kernel launch.

The conv kernels are not here: test_stem_maxpool_nan_mask keeps its one NaN pixel, and tests/test_gpu_conv_nonfinite.py plants
NaN and +-inf in the input, the filter and the tail of every conv family (the stem + max-pool kernels among them) under the
contract of tests/nonfinite_ref.py.
"""
import zlib

import numpy as np
import pytest

from oracle import planer_np as onp

pytestmark = pytest.mark.gpu

F32 = np.float32
TINY = float(np.float32(2.0 ** -149))
SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, TINY, -TINY, 3 * TINY, 2.0 ** -127, -2.0 ** -127,
                    1e4, -1e4, np.nextafter(F32(1e4), F32(0)), np.nextafter(F32(1e4), F32(2e4)),
                    np.nextafter(F32(-1e4), F32(0)), np.nextafter(F32(-1e4), F32(-2e4))], F32)
# for ops that add: finite partial sums stay exact
SUM_SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e4, -1e4], F32)
# transcendental inputs with exact results in every libm
TRANS_SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e4, -1e4], F32)
ZERO_SIGN_TIE = "max / min of a +0 / -0 tie: the GPU gives IEEE maximum / minimum (-0 < +0), numpy the operand order's"


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def seeded(key, shape, specials=SPECIAL, frac=0.3, lo=-4, hi=4):
    """Integers in [lo, hi] with a fraction `frac` of the elements replaced by special values, every special present."""
    rng = _rng("seeded", key, shape)
    x = rng.integers(lo, hi + 1, shape).astype(F32)
    flat = x.reshape(-1)
    m = rng.random(flat.size) < frac
    flat[m] = rng.choice(specials, int(m.sum()))
    k = min(flat.size, specials.size)
    flat[rng.choice(flat.size, k, replace=False)] = specials[:k]
    return x


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def mismatch(y, ref):
    """Elements whose bit patterns differ, NaN matching NaN."""
    y, ref = np.asarray(y, F32), np.asarray(ref, F32)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    return (bits(y) != bits(ref)) & ~(np.isnan(y) & np.isnan(ref))


def assert_bits(y, ref, what):
    bad = mismatch(y, ref)
    if bad.any():
        i = np.argwhere(bad)[:5]
        yy, rr = np.asarray(y, F32), np.asarray(ref, F32)
        raise AssertionError("%s: %d of %d elements differ, e.g. %s" % (
            what, int(bad.sum()), bad.size, ", ".join("%s: %r (0x%08x) want %r (0x%08x)" % (
                tuple(int(v) for v in j), float(yy[tuple(j)]), int(bits(yy)[tuple(j)]), float(rr[tuple(j)]),
                int(bits(rr)[tuple(j)])) for j in i)))


def ieee_max_ref(f, x, *args, **kw):
    """`f` (an oracle max / min op) in float64 with -0 below +0: -0 becomes -1e-300, which no float32 operand can equal."""
    x64 = np.asarray(x, np.float64)
    x64 = np.where((x64 == 0) & np.signbit(x64), -1e-300, x64)
    r = np.asarray(f(x64, *args, **kw), np.float64)
    return np.where(r == -1e-300, -0.0, r).astype(F32)


def assert_max_family(y, x, f, what, *args, **kw):
    """Bit-exact against the IEEE-maximum reference; against numpy's own float32 result only ZERO_SIGN_TIE may differ."""
    assert_bits(y, ieee_max_ref(f, x, *args, **kw), what)
    with np.errstate(all="ignore"):
        ref = np.asarray(f(x.copy(), *args, **kw), F32)
    bad = mismatch(y, ref)
    assert not (bad & ~((np.asarray(y) == 0) & (ref == 0))).any(), what
    if bad.any():
        print("%s: %d elements, %s" % (what, int(bad.sum()), ZERO_SIGN_TIE))


def _q4(pa, x):
    from planer_amd import q4
    return q4.to_q4(pa.asarray(x))


def _nchw(pa, yq):
    from planer_amd import q4
    return q4.from_q4(yq).get()


# ---- elementwise ---------------------------------------------------------------------------------------------------------
# odd total (scalar tail of unary_vec4) and an unaligned view: d[1] of a (2, 1001) tensor starts 4004 bytes in
def _unary_inputs(pa, key, specials):
    x = seeded(key, (2, 1001), specials)
    d = pa.asarray(x)
    return [("vec4+tail", x[0], d[0]), ("unaligned", x[1], d[1])]


EXACT_UNARY = [
    ("relu", lambda L, d: L.ReLU(d), onp.relu),
    ("leakyrelu", lambda L, d: L.LeakyReLU(d, alpha=0.1), lambda x: onp.leakyrelu(x, 0.1)),
    ("sqrt", lambda L, d: L.Sqrt(d), np.sqrt),
    ("reciprocal", lambda L, d: L.Reciprocal(d), lambda x: 1 / x),
    ("hardsigmoid", lambda L, d: L.HardSigmoid(d, alpha=0.2, beta=0.5), lambda x: onp.hardsigmoid(x, 0.2, 0.5)),
    ("clip", lambda L, d: L.Clip(d, min=0.0, max=6.0), lambda x: onp.clip(x, 0.0, 6.0)),
    ("clip-neg", lambda L, d: L.Clip(d, min=-1.0, max=2.0), lambda x: onp.clip(x, -1.0, 2.0)),
]
TRANS_UNARY = [
    ("exp", lambda L, d: L.Exp(d), np.exp),
    ("log", lambda L, d: L.Log(d), np.log),
    ("tanh", lambda L, d: L.Tanh(d), np.tanh),
    ("sigmoid", lambda L, d: L.Sigmoid(d), onp.sigmoid),
]


@pytest.mark.parametrize("name,dev,ref", EXACT_UNARY + TRANS_UNARY, ids=[u[0] for u in EXACT_UNARY + TRANS_UNARY])
def test_unary(pa, name, dev, ref):
    trans = name in [u[0] for u in TRANS_UNARY]
    for path, x, d in _unary_inputs(pa, name, SPECIAL):
        if trans:
            x = np.resize(TRANS_SPECIAL, x.shape).astype(F32)
            d = pa.asarray(np.stack([x, x]))[0 if path == "vec4+tail" else 1]
        with np.errstate(all="ignore"):
            want = np.asarray(ref(x.copy()), F32)
        assert_bits(dev(pa.layer, d).get(), want, "%s %s" % (name, path))


def test_unary_q4(pa):
    from planer_amd import q4
    x = seeded("uq4", (2, 6, 5, 7))
    for name, f, ref in [("relu", q4.ReLUQ4, onp.relu), ("leakyrelu", lambda t: q4.LeakyReLUQ4(t, alpha=0.1),
                                                            lambda v: onp.leakyrelu(v, 0.1)),
                         ("clip", lambda t: q4.ClipQ4(t, min=0.0, max=6.0), lambda v: onp.clip(v, 0.0, 6.0))]:
        with np.errstate(all="ignore"):
            assert_bits(_nchw(pa, f(_q4(pa, x))), np.asarray(ref(x.copy()), F32), "%s q4" % name)
    xt = np.resize(TRANS_SPECIAL, (2, 6, 5, 7)).astype(F32)
    with np.errstate(all="ignore"):
        assert_bits(_nchw(pa, q4.SigmoidQ4(_q4(pa, xt))), onp.sigmoid(xt.copy()), "sigmoid q4")


BINARY = [("add", "Add", np.add), ("sub", "Sub", np.subtract), ("mul", "Mul", np.multiply), ("div", "Div", np.divide)]


@pytest.mark.parametrize("name,fn,ref", BINARY, ids=[b[0] for b in BINARY])
def test_binary_and_broadcast(pa, name, fn, ref):
    f = getattr(pa.layer, fn)
    a = seeded(name + "a", (2, 3, 4, 5))
    for bshape in [(2, 3, 4, 5), (1, 3, 1, 1), (1,), (4, 1), (5,), (2, 1, 4, 1)]:
        b = seeded((name, bshape), bshape)
        with np.errstate(all="ignore"):
            assert_bits(f(pa.asarray(a), pa.asarray(b)).get(), ref(a, b), "%s %s" % (name, bshape))
            assert_bits(f(pa.asarray(b), pa.asarray(a)).get(), ref(b, a), "%s %s reversed" % (name, bshape))


def test_add_vec4_and_q4(pa):
    from planer_amd import q4
    a, b = seeded("addv4a", (2, 5, 6, 7)), seeded("addv4b", (2, 5, 6, 7))
    assert_bits(pa.layer.Add(pa.asarray(a), pa.asarray(b)).get(), a + b, "add same shape")
    assert_bits(_nchw(pa, q4.AddQ4(_q4(pa, a), _q4(pa, b))), a + b, "add q4")


def test_pow_special_grid(pa):
    base = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 4.0, -4.0, 0.25], F32)      # exact powers only
    expo = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 2.0, 3.0, -1.0, -2.0, 0.5], F32)
    a, b = np.meshgrid(base, expo, indexing="ij")
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    with np.errstate(all="ignore"):
        want = np.power(a, b)
    assert_bits(pa.layer.Pow(pa.asarray(a), pa.asarray(b)).get(), want, "pow")


# ---- pools ------------------------------------------------------------------------------------------------------------------
POOLS = [  # (input shape, window, pads, strides): generic; 3x3 s2 p1 on an even map with Wo % 4 == 0 (the x4 kernel); odd map
    ((2, 3, 9, 11), (2, 2), (0, 0, 0, 0), (2, 2)),
    ((2, 3, 16, 16), (3, 3), (1, 1, 1, 1), (2, 2)),
    ((1, 5, 13, 9), (3, 3), (1, 1, 1, 1), (2, 2)),
    ((1, 2, 7, 8), (3, 3), (1, 1, 1, 1), (1, 1)),
]


@pytest.mark.parametrize("geom", POOLS, ids=["x".join(map(str, g[0])) + "k%d" % g[1][0] for g in POOLS])
def test_maxpool_nchw_and_q4(pa, geom):
    from planer_amd import q4
    xs, w, pads, strides = geom
    x = seeded(("maxpool", geom), xs)
    kw = dict(w=list(w), pads=list(pads), strides=list(strides))
    assert_max_family(pa.layer.Maxpool(pa.asarray(x), **kw).get(), x, onp.maxpool, "maxpool %s" % (geom,), **kw)
    assert_max_family(_nchw(pa, q4.MaxpoolQ4(_q4(pa, x), **kw)), x, onp.maxpool, "maxpool q4 %s" % (geom,), **kw)


def test_maxpool_q4_generic_3x3(pa, monkeypatch):
    from planer_amd import q4
    monkeypatch.setenv("PLANER_HIP_POOL_GENERIC", "1")
    x = seeded("maxpool-generic", (2, 6, 10, 12))
    kw = dict(w=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2])
    assert_max_family(_nchw(pa, q4.MaxpoolQ4(_q4(pa, x), **kw)), x, onp.maxpool, "maxpool q4 generic", **kw)


def test_maxpool_nan_in_every_tap_position(pa):
    """A lone NaN (or +inf) at each position of the map: every output window that covers it must show it."""
    from planer_amd import q4
    kw = dict(w=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2])
    for v in (np.nan, np.inf):
        x = np.full((16, 1, 8, 8), -3.0, F32)
        for i in range(16):
            x[i, 0, (i * 5) % 8, (i * 3) % 8] = v
        x = np.concatenate([x, x[::-1]], axis=1)
        want = onp.maxpool(x.copy(), **kw)
        assert_bits(pa.layer.Maxpool(pa.asarray(x), **kw).get(), want, "maxpool x4 lone %r" % v)
        assert_bits(_nchw(pa, q4.MaxpoolQ4(_q4(pa, x), **kw)), want, "maxpool q4 2x1 lone %r" % v)


@pytest.mark.parametrize("geom", POOLS, ids=["x".join(map(str, g[0])) + "k%d" % g[1][0] for g in POOLS])
def test_avgpool_nchw_and_q4(pa, geom):
    from planer_amd import q4
    xs, w, pads, strides = geom
    x = seeded(("avgpool", geom), xs, SUM_SPECIAL)
    kw = dict(w=list(w), pads=list(pads), strides=list(strides))
    with np.errstate(all="ignore"):
        want = onp.avgpool(x.copy(), **kw)
    assert_bits(pa.layer.AveragePool(pa.asarray(x), **kw).get(), want, "avgpool %s" % (geom,))
    assert_bits(_nchw(pa, q4.AveragePoolQ4(_q4(pa, x), **kw)), want, "avgpool q4 %s" % (geom,))


# ---- resampling --------------------------------------------------------------------------------------------------------------
def test_upsample_nearest_nchw_and_q4(pa):
    from planer_amd import q4
    x = seeded("upn", (2, 5, 4, 3))
    want = onp.upsample(x.copy(), [1, 1, 2, 3], "nearest")
    assert_bits(pa.layer.UpSample(pa.asarray(x), [1, 1, 2, 3], "nearest").get(), want, "upsample nearest")
    assert_bits(_nchw(pa, q4.UpSampleQ4(_q4(pa, x), [1, 1, 2, 3], "nearest")), want, "upsample nearest q4")


@pytest.mark.parametrize("k", [(2, 2), (4, 4), (1, 2), (2, 1)], ids=["2x2", "4x4", "1x2", "2x1"])
def test_upsample_linear(pa, k):
    """Integer data, power-of-two factors: the float16 weights are multiples of 2^-6, every finite sum is exact."""
    x = seeded(("upl", k), (2, 3, 5, 6), SUM_SPECIAL)
    with np.errstate(all="ignore"):
        want = np.asarray(onp.upsample(x.copy(), [1, 1, k[0], k[1]], "linear"), F32)
    assert_bits(pa.layer.UpSample(pa.asarray(x), [1, 1, k[0], k[1]], "linear").get(), want, "upsample linear %s" % (k,))
    z = np.full((1, 2, 3, 4), -0.0, F32)                    # an all -0 map: the oracle's matrix product gives +0
    assert_bits(pa.layer.UpSample(pa.asarray(z), [1, 1, k[0], k[1]], "linear").get(),
                np.asarray(onp.upsample(z.copy(), [1, 1, k[0], k[1]], "linear"), F32), "upsample linear -0 %s" % (k,))


def test_resize_linear_fractional(pa):
    """Fractional factors (resize_planes_kernel): the reference's own roundings, so bit-exact on any data."""
    for xs, k in [((2, 3, 5, 6), (1.5, 2.5)), ((1, 4, 7, 4), (0.75, 1.75))]:
        x = seeded(("resize", xs, k), xs)
        with np.errstate(all="ignore"):
            want = np.asarray(onp.upsample_to_size(x.copy(), (int(round(k[0] * xs[2])), int(round(k[1] * xs[3])))), F32)
        y = pa.layer.Resize(pa.asarray(x), None, np.array([1, 1, k[0], k[1]], F32), mode="linear").get()
        assert_bits(y, want, "resize %s %s" % (xs, k))


@pytest.mark.parametrize("xs", [(2, 3, 40, 40), (2, 5, 7, 7)], ids=["affine_plane", "affine_flat"])
def test_batchnorm_affine_paths(pa, xs):
    """BatchNorm's two kernels (one block row per plane for planes >= 1024 elements, flat otherwise) and the Q4 one:
    x * K then + B, two roundings like numpy."""
    from planer_amd import q4
    x = seeded(("bn", xs), xs)
    rng = _rng("bn", xs)
    K = np.concatenate([[np.nan, np.inf, -0.0], rng.standard_normal(xs[1] - 3)]).astype(F32)
    B = np.concatenate([[1.0, -np.inf, 0.0], rng.standard_normal(xs[1] - 3)]).astype(F32)
    with np.errstate(all="ignore"):
        want = onp.batchnorm(x.copy(), K.reshape(1, -1, 1, 1), B.reshape(1, -1, 1, 1))
    assert_bits(pa.layer.BatchNorm(pa.asarray(x), pa.asarray(K.reshape(1, -1, 1, 1)), pa.asarray(B.reshape(1, -1, 1, 1))).get(),
                want, "batchnorm %s" % (xs,))
    assert_bits(_nchw(pa, q4.BatchNormQ4(_q4(pa, x), pa.asarray(K.reshape(1, -1, 1, 1)), pa.asarray(B.reshape(1, -1, 1, 1)))),
                want, "batchnorm q4 %s" % (xs,))


def test_erf_lut(pa):
    """The table lookup on special values and floats of [-3, 3]: the entry and the clobbered x both equal the oracle's.
    NaN and +-inf index entry 0 (inf * 0 is NaN in the mask multiplications), as numpy's astype('int16') does."""
    rng = _rng("erf")
    x = np.concatenate([SPECIAL, rng.uniform(-3, 3, 2001), np.arange(-1030, 1031) / 256]).astype(F32)
    xr = x.copy()
    with np.errstate(all="ignore"):
        want = onp.erf(xr)
    d = pa.asarray(x)
    assert_bits(pa.layer.Erf(d).get(), want, "erf")
    assert_bits(d.get(), xr, "erf: x clobbered like the reference")


# ---- row kernels ----------------------------------------------------------------------------------------------------------
def test_gap_nchw_and_q4(pa):
    from planer_amd import q4
    for xs in [(2, 6, 4, 4), (1, 5, 8, 8), (3, 7, 2, 8)]:            # spatial sizes are powers of two: 1/n is exact
        x = seeded(("gap", xs), xs, SUM_SPECIAL)
        with np.errstate(all="ignore"):
            want = onp.gap(x.copy())
        assert_bits(pa.layer.GlobalAveragePool(pa.asarray(x)).get(), want, "gap %s" % (xs,))
        assert_bits(q4.GlobalAveragePoolQ4(_q4(pa, x)).get(), want, "gap q4 %s" % (xs,))


@pytest.mark.parametrize("axes", [[-1], [1], [0, 2]], ids=["last", "mid", "0+2"])
def test_reductions(pa, axes):
    xs = (3, 64, 16)
    x = seeded(("reduce", str(axes)), xs, SUM_SPECIAL, frac=0.02)
    xm = seeded(("reducem", str(axes)), xs, SPECIAL, frac=0.02)
    L = pa.layer
    with np.errstate(all="ignore"):
        assert_bits(L.ReduceSum(pa.asarray(x), axes=axes).get(), np.sum(x, axis=tuple(axes), keepdims=True), "sum %s" % axes)
        assert_bits(L.ReduceMean(pa.asarray(x), axes=axes).get(), np.mean(x, axis=tuple(axes), keepdims=True), "mean %s" % axes)
    for name, f, ref in [("max", L.ReduceMax, np.max), ("min", L.ReduceMin, np.min)]:
        assert_max_family(f(pa.asarray(xm), axes=axes).get(), xm, ref, "%s %s" % (name, axes), axis=tuple(axes), keepdims=True)


@pytest.mark.parametrize("log", [0, 1], ids=["softmax", "logsoftmax"])
def test_softmax_rows_with_specials(pa, log):
    """Rows with a NaN or +inf are NaN; -inf entries give exact 0 (or -inf); -1e4 beside 0 underflows to exact 0."""
    rng = _rng("softmax", log)
    x = rng.integers(-4, 5, (9, 70)).astype(F32)
    x[1, 5] = np.nan
    x[2, 69] = np.inf
    x[3, ::7] = -np.inf
    x[4, :] = -np.inf
    x[5, 3] = -1e4
    x[6, :] = -0.0
    x[7, 10] = 1e4
    x[8, :64] = TINY
    f, ref = (pa.layer.LogSoftmax, onp.logsoftmax) if log else (pa.layer.Softmax, onp.softmax)
    for axis in (-1, 0):
        xa = x if axis == -1 else np.ascontiguousarray(x.T)
        with np.errstate(all="ignore"):
            want = np.asarray(ref(xa.copy(), axis=axis), F32)
        y = f(pa.asarray(xa), axis=axis).get()
        cls = lambda a: np.stack([np.isnan(a), np.isposinf(a), np.isneginf(a), a == 0])   # noqa: E731
        assert (cls(y) == cls(want)).all(), "%s axis %d: NaN / inf / zero pattern differs" % (f.__name__, axis)
        fin = np.isfinite(want) & (want != 0)
        np.testing.assert_allclose(y[fin], want[fin], rtol=1e-5, atol=1e-6)


def test_stem_maxpool_nan_mask(pa):
    """One NaN input pixel through the fused stem + max-pool kernels (row-packed and NCHW): the output's NaN mask is the
    oracle's conv -> BN -> ReLU -> maxpool."""
    from planer_amd import q4
    rng = _rng("stem-nan")
    conv = dict(strides=[2, 2], pads=[3, 3, 3, 3], dilations=[1, 1], group=1)
    pool = dict(w=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2])
    x = rng.standard_normal((2, 3, 64, 64)).astype(F32)
    x[0, 1, 20, 33] = np.nan
    x[1, 2, 0, 63] = np.nan                                 # at a corner: the window touches the zero padding
    K = (rng.standard_normal((64, 3, 7, 7)) / 12).astype(F32)
    sc = rng.uniform(0.5, 2, 64).astype(F32)
    sh = rng.uniform(-1, 1, 64).astype(F32)
    with np.errstate(all="ignore"):
        want = onp.maxpool(onp.relu(onp.batchnorm(onp.conv2d(x, K, **conv), sc.reshape(1, -1, 1, 1), sh.reshape(1, -1, 1, 1))),
                           **pool)
    assert np.isnan(want).any() and not np.isnan(want).all()
    dx, dsc, dsh = pa.asarray(x), pa.asarray(sc), pa.asarray(sh)
    ctx = pa.hip.context()
    for label, Kq, extra in [("stem+maxpool ", q4.prepare_rowpack_weights(pa.asarray(K)), {}),
                             ("stem+maxpool(nchw)", q4.prepare_stem_nchw_weights(pa.asarray(K)), dict(w_layout=12))]:
        y = _nchw(pa, q4.ConvPoolQ4(dx, Kq, None, dsc, dsh, act=pa.layer.ACT_RELU, **conv, **extra))
        assert ctx.last_conv_plan().startswith(label), ctx.last_conv_plan()
        assert (np.isnan(y) == np.isnan(want)).all(), "%s: %d NaN outputs, oracle %d" % (
            label, int(np.isnan(y).sum()), int(np.isnan(want).sum()))
        fin = ~np.isnan(want)
        np.testing.assert_allclose(y[fin], want[fin], rtol=1e-4, atol=1e-4 * float(np.abs(want[fin]).max()))


# ---- empty extents: numpy's answer, no kernel launch ----------------------------------------------------------------------------
def _same(y, want, what):
    y = np.asarray(y)
    assert y.shape == want.shape, "%s: shape %s, numpy %s" % (what, y.shape, want.shape)
    assert_bits(y, want.astype(F32), what)


def test_empty_gap_and_instancenorm(pa):
    from planer_amd import q4
    for xs in [(2, 3, 0, 5), (2, 5, 4, 0)]:
        x = np.zeros(xs, F32)
        with np.errstate(all="ignore"), pytest.warns(RuntimeWarning):
            want = onp.gap(x.copy())
        _same(pa.layer.GlobalAveragePool(pa.asarray(x)).get(), want, "gap %s" % (xs,))
        _same(q4.GlobalAveragePoolQ4(_q4(pa, x)).get(), want, "gap q4 %s" % (xs,))
        s, b = np.ones(xs[1], F32), np.zeros(xs[1], F32)
        with np.errstate(all="ignore"):
            want = onp.instancenorm(x.copy(), s.copy(), b.copy())
        _same(pa.layer.InstanceNormalization(pa.asarray(x), pa.asarray(s), pa.asarray(b)).get(), want,
              "instancenorm %s" % (xs,))


@pytest.mark.parametrize("xs,axes", [((4, 0, 3), [1]), ((4, 0), [-1]), ((0, 5), [0]), ((2, 0, 3), [0, 1])],
                         ids=["mid", "last", "first", "two"])
def test_empty_reductions(pa, xs, axes):
    x = np.zeros(xs, F32)
    L = pa.layer
    for keep in (True, False):
        with np.errstate(all="ignore"):
            _same(L.ReduceSum(pa.asarray(x), axes=axes, keepdims=keep).get(), np.sum(x, axis=tuple(axes), keepdims=keep),
                  "sum %s %s" % (xs, axes))
            _same(L.ReduceMean(pa.asarray(x), axes=axes, keepdims=keep).get(), np.mean(x, axis=tuple(axes), keepdims=keep),
                  "mean %s %s" % (xs, axes))
        for f, ref in [(L.ReduceMax, np.max), (L.ReduceMin, np.min)]:
            with pytest.raises(ValueError):
                ref(x, axis=tuple(axes), keepdims=keep)
            with pytest.raises(ValueError):
                f(pa.asarray(x), axes=axes, keepdims=keep)


def test_empty_inner_dimension_matmul_and_dense(pa):
    L = pa.layer
    for xs, ys in [((3, 0), (0, 4)), ((2, 3, 0), (0, 4)), ((2, 3, 0), (2, 0, 4)), ((3, 0), (2, 0, 4)), ((1, 3, 0), (2, 0, 4))]:
        x, y = np.zeros(xs, F32), np.zeros(ys, F32)
        _same(L.MatMul(pa.asarray(x), pa.asarray(y)).get(), onp.matmul(x, y), "matmul %s @ %s" % (xs, ys))
    x, y = np.zeros((2, 3, 0), F32), np.zeros((5, 0, 4), F32)
    with pytest.raises(ValueError):
        onp.matmul(x, y)
    with pytest.raises(ValueError):
        L.MatMul(pa.asarray(x), pa.asarray(y))
    x, K, B = np.zeros((3, 0), F32), np.zeros((4, 0), F32), np.array([1.5, -2.0, np.nan, -0.0], F32)
    _same(L.Dense(pa.asarray(x), pa.asarray(K), pa.asarray(B)).get(), onp.dense(x, K, B), "dense K = 0")

"""Non-convolution kernels on float data against the float64 references of tests/ref64_ops.py, element by element, and on
integer operands bit for bit where every sum is exact.  Rows of 1 .. 65537 elements scaled per row by 2^U(-10, 6), DC offsets
0 and 50, more rows than the grid cap (cu_count * 8 blocks of 4 waves), Q4 GAP with C % 4 != 0, the transpose route of
softmax and reductions, linear upsampling, fractional resize, and the LSTM cell called through pl_lstm_cell_f32.  Each case prints its worst err / tol, and the transcendentals their worst ulps (run with -s)."""
import zlib

import numpy as np
import pytest

from tests import ref64 as R64
from tests import ref64_ops as R

pytestmark = pytest.mark.gpu

LENGTHS = [1, 63, 64, 65, 1000, 4096, 50176, 65537]


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _rows(n):
    return max(3, min(300, 600000 // n))


def _report(what, worst):
    print("%-40s worst err/tol %.3f" % (what, worst))


@pytest.mark.parametrize("dc", [0.0, 50.0], ids=["dc0", "dc50"])
def test_reductions_and_gap(pa, dc):
    L = pa.layer
    from planer_amd import q4
    for n in LENGTHS:
        x = R.skewed_rows(_rng("red", n, dc), _rows(n), n, dc)
        d = pa.asarray(x)
        w = [R.check(L.ReduceSum(d, axes=[-1], keepdims=False).get(), R.reduce64(x, 0), R.sum_bound(x), "sum n=%d" % n),
             R.check(L.ReduceMean(d, axes=[-1], keepdims=False).get(), R.reduce64(x, 1), R.mean_bound(x), "mean n=%d" % n)]
        for op, f in [(2, L.ReduceMax), (3, L.ReduceMin)]:
            assert (f(d, axes=[-1], keepdims=False).get() == R.reduce64(x, op)).all(), "max/min n=%d" % n
        x4 = x.reshape(1, x.shape[0], 1, n)
        w.append(R.check(L.GlobalAveragePool(pa.asarray(x4)).get().reshape(-1), R.reduce64(x, 1), R.mean_bound(x), "gap"))
        w.append(R.check(q4.GlobalAveragePoolQ4(q4.to_q4(pa.asarray(x4))).get().reshape(-1), R.reduce64(x, 1),
                         R.mean_bound(x), "gap q4 n=%d" % n))
        _report("reduce/gap n=%d dc=%g" % (n, dc), max(w))
    # the transpose route: a reduced axis that is not last
    x = R.skewed_rows(_rng("redmid", dc), 40, 3000, dc).reshape(8, 5, 3000).transpose(0, 2, 1).copy()
    xt = x.transpose(0, 2, 1).reshape(40, 3000)
    y = L.ReduceSum(pa.asarray(x), axes=[1], keepdims=False).get().reshape(-1)
    _report("reducesum mid axis", R.check(y, R.reduce64(xt, 0), R.sum_bound(xt), "sum mid axis"))


def test_gap_past_grid_cap_and_partial_quads(pa):
    from planer_amd import q4
    L = pa.layer
    for xs in [(32, 512, 7, 7), (40, 517, 7, 7), (3, 5, 13, 13), (2, 7, 224, 224), (32, 512, 8, 8), (40, 517, 4, 4)]:
        rng = _rng("gap", xs)
        x = (rng.standard_normal(xs) * 2.0 ** rng.uniform(-10, 6, (1, xs[1], 1, 1)) + 50 * (xs[0] % 2)).astype(np.float32)
        rows = x.reshape(xs[0] * xs[1], -1)
        ref, tol = R.reduce64(rows, 1).reshape(xs[0], xs[1], 1, 1), R.mean_bound(rows).reshape(xs[0], xs[1], 1, 1)
        w = max(R.check(L.GlobalAveragePool(pa.asarray(x)).get(), ref, tol, "gap %s" % (xs,)),
                R.check(q4.GlobalAveragePoolQ4(q4.to_q4(pa.asarray(x))).get(), ref, tol, "gap q4 %s" % (xs,)))
        _report("gap %s" % (xs,), w)
        xi = rng.integers(-64, 65, xs).astype(np.float32)                 # integer sums are exact; 1/49, 1/169 are not,
        if (xs[2] * xs[3]) & (xs[2] * xs[3] - 1) == 0:                    # so only power-of-two maps are bit-exact
            want = xi.astype(np.float64).mean(axis=(2, 3), keepdims=True)
            assert (L.GlobalAveragePool(pa.asarray(xi)).get() == want).all(), "integer gap %s" % (xs,)
            assert (q4.GlobalAveragePoolQ4(q4.to_q4(pa.asarray(xi))).get() == want).all(), "integer gap q4 %s" % (xs,)
        si = L.ReduceSum(pa.asarray(xi.reshape(xs[0] * xs[1], -1)), axes=[-1], keepdims=False).get()
        assert (si == xi.reshape(xs[0] * xs[1], -1).astype(np.int64).sum(-1)).all(), "integer reducesum %s" % (xs,)


@pytest.mark.parametrize("log", [0, 1], ids=["softmax", "logsoftmax"])
def test_softmax(pa, log):
    f = pa.layer.LogSoftmax if log else pa.layer.Softmax
    cases = [(n, _rows(n)) for n in LENGTHS if n > 1] + [(10, 20000)]
    for n, rows in cases:
        rng = _rng("softmax", n, log)
        x = (rng.standard_normal((rows, n)) * 2.0 ** rng.uniform(-10, 6, (rows, 1))).astype(np.float32)
        x[0] = rng.uniform(-120, 0, n)                                    # subnormal outputs
        _report("%s n=%d rows=%d" % (f.__name__, n, rows),
                R.check(f(pa.asarray(x)).get(), R.softmax64(x, log), R.softmax_bound(x, log), "%s n=%d" % (f.__name__, n)))
    x = (_rng("softmax-axis0", log).standard_normal((300, 7, 5)) * 8).astype(np.float32)
    xt = x.transpose(1, 2, 0).reshape(35, 300)
    y = f(pa.asarray(x), axis=0).get().transpose(1, 2, 0).reshape(35, 300)
    _report("%s axis 0" % f.__name__, R.check(y, R.softmax64(xt, log), R.softmax_bound(xt, log), "axis 0"))


@pytest.mark.parametrize("dc", [0.0, 50.0], ids=["dc0", "dc50"])
def test_instancenorm(pa, dc):
    for xs in [(2, 3, 1, 1), (2, 5, 7, 9), (4, 16, 32, 32), (1, 3, 224, 256), (3, 4, 1, 65537)]:
        rng = _rng("in", xs, dc)
        x = (rng.standard_normal(xs) * 2.0 ** rng.uniform(-10, 6, (xs[0], xs[1], 1, 1)) + dc).astype(np.float32)
        s = (rng.choice([-1, 1], xs[1]) * 2.0 ** rng.uniform(-10, 6, xs[1])).astype(np.float32)
        b = rng.standard_normal(xs[1]).astype(np.float32)
        rows = x.reshape(xs[0] * xs[1], -1)
        sr, br = np.tile(s, xs[0]), np.tile(b, xs[0])
        y = pa.layer.InstanceNormalization(pa.asarray(x), pa.asarray(s), pa.asarray(b)).get().reshape(rows.shape)
        _report("instancenorm %s dc=%g" % (xs, dc),
                R.check(y, R.instancenorm64(rows, sr, br), R.instancenorm_bound(rows, sr, br), "instancenorm %s" % (xs,)))


def test_transcendentals_ulps(pa):
    L = pa.layer
    x = np.concatenate([np.linspace(-87, 88, 400001), np.geomspace(1e-30, 80, 20001), -np.geomspace(1e-30, 80, 20001)])
    x = x.astype(np.float32)
    pos = np.abs(x[np.abs(x) > 0]).astype(np.float32)
    x64, p64 = x.astype(np.float64), pos.astype(np.float64)
    cases = [("exp", L.Exp, x, np.exp(x64)), ("log", L.Log, pos, np.log(p64)), ("tanh", L.Tanh, x, np.tanh(x64)),
             ("sqrt", L.Sqrt, pos, np.sqrt(p64)), ("reciprocal", L.Reciprocal, x[x != 0], 1 / x64[x != 0]),
             ("sigmoid", L.Sigmoid, x, 1 / (1 + np.exp(-x64)))]
    d = pa.asarray(x)
    dp = pa.asarray(pos)
    for name, f, inp, ref in cases:
        arg = d if inp is x else dp if inp is pos else pa.asarray(inp)
        y = f(arg).get()
        u = R.ulps(y, ref)
        i = int(np.argmax(u))
        print("%-10s worst %.3f ulp at x = %r" % (name, u[i], float(inp[i])))
        assert u[i] <= R.ULP[name], "%s: %.3f ulp at x = %r (allowance %g)" % (name, u[i], float(inp[i]), R.ULP[name])
    # pow with a float exponent
    a = np.geomspace(1e-3, 1e3, 4001).astype(np.float32)
    for p in (0.5, 2.0, 3.0, -1.5, 2.7):
        y = L.Pow(pa.asarray(a), pa.asarray(np.full(a.shape, p, np.float32))).get()
        u = R.ulps(y, np.power(a.astype(np.float64), np.float64(np.float32(p))))
        print("pow ^%-5g worst %.3f ulp" % (p, u.max()))
        assert u.max() <= R.ULP["pow"]


def test_hardsigmoid_exact(pa):
    x = np.concatenate([np.linspace(-4, 4, 100003), (np.arange(-4096, 4097) / 1024)]).astype(np.float32)
    want = np.clip(x * np.float32(0.2) + np.float32(0.5), 0, 1)
    assert (pa.layer.HardSigmoid(pa.asarray(x), alpha=0.2, beta=0.5).get() == want).all()


@pytest.mark.parametrize("dc", [0.0, 50.0], ids=["dc0", "dc50"])
def test_matmul(pa, dc):
    for xs, ys in [((64, 300), (300, 70)), ((3, 33, 129), (129, 17)), ((2, 40, 64), (2, 64, 50)), ((1, 1), (1, 1))]:
        rng = _rng("mm", xs, ys, dc)
        x = (rng.standard_normal(xs) * 2.0 ** rng.uniform(-10, 6, xs[:-1] + (1,)) + dc).astype(np.float32)
        y = (rng.standard_normal(ys) * 2.0 ** rng.uniform(-10, 6, (1,) * (len(ys) - 1) + (ys[-1],))).astype(np.float32)
        got = pa.layer.MatMul(pa.asarray(x), pa.asarray(y)).get()
        if len(ys) == 2:                                       # (..., m, k) @ (k, n): one GEMM over all rows
            pairs = [(x.reshape(-1, xs[-1]), y, got.reshape(-1, ys[-1]))]
        else:
            pairs = [(x[b], y[b], got[b]) for b in range(xs[0])]
        w = 0.0
        for xb, yb, g in pairs:
            m, k = xb.shape
            n = yb.shape[1]
            xc, kc = xb.reshape(m, k, 1, 1), yb.T.reshape(n, k, 1, 1)
            w = max(w, R64.check(g, R64.ref64(xc, kc).reshape(m, n), R64.bound(xc, kc).reshape(m, n),
                                 "matmul %s @ %s" % (xs, ys)))
        _report("matmul %s @ %s dc=%g" % (xs, ys, dc), w)
        xi = rng.integers(-8, 9, xs).astype(np.float32)
        yi = rng.integers(-8, 9, ys).astype(np.float32)
        assert (pa.layer.MatMul(pa.asarray(xi), pa.asarray(yi)).get() == np.matmul(xi.astype(np.int64), yi.astype(np.int64))).all()


@pytest.mark.parametrize("dc", [0.0, 50.0], ids=["dc0", "dc50"])
def test_upsample_linear_and_resize(pa, dc):
    L = pa.layer
    for fh, fw in [(2, 2), (4, 4), (3, 3), (1, 2), (2, 1), (8, 8), (3, 5)]:
        rng = _rng("upl", fh, fw, dc)
        x = (rng.standard_normal((2, 6, 9, 11)) * 2.0 ** rng.uniform(-10, 6, (1, 6, 1, 1)) + dc).astype(np.float32)
        y = L.UpSample(pa.asarray(x), [1, 1, fh, fw], "linear").get()
        _report("upsample_linear %dx%d dc=%g" % (fh, fw, dc), R.check(y, R.upsample_linear64(x, fh, fw),
                                                                   R.upsample_linear_bound(x, fh, fw), "upsample %dx%d" % (fh, fw)))
        if fh & (fh - 1) == 0 and fw & (fw - 1) == 0:          # integer operands, power-of-two factors: exact
            xi = rng.integers(-64, 65, x.shape).astype(np.float32)
            assert (L.UpSample(pa.asarray(xi), [1, 1, fh, fw], "linear").get() == R.upsample_linear64(xi, fh, fw)).all()
    for k in [(1.5, 1.5), (0.75, 2.5), (2.3, 1.7)]:
        rng = _rng("resize", k, dc)
        x = (rng.standard_normal((2, 6, 9, 11)) * 2.0 ** rng.uniform(-10, 6, (1, 6, 1, 1)) + dc).astype(np.float32)
        oh, ow = int(round(k[0] * 9)), int(round(k[1] * 11))
        y = L.Resize(pa.asarray(x), None, np.array([1, 1, k[0], k[1]], np.float32), mode="linear").get()
        _report("resize_linear %s dc=%g" % (k, dc), R.check(y, R.resize_linear64(x, oh, ow), R.resize_linear_bound(x, oh, ow),
                                                          "resize %s" % (k,)))


def test_lstm_cell(pa):
    """pl_lstm_cell_f32 called directly; gates spread so that sigmoid and tanh see their whole range."""
    from planer_amd import _lib
    ctx = pa.hip.context()
    worst = [0.0, 0.0]
    for N, H, spread in [(64, 256, 4.0), (32, 100, 30.0), (5, 7, 100.0)]:
        gx, gh, b, cp = R.lstm_operands(_rng("lstm", N, H, spread), N, H, spread)
        d = [pa.asarray(a) for a in (gx, gh, b, cp)]
        h, c = pa.hip.empty((N, H)), pa.hip.empty((N, H))
        _lib.call("pl_lstm_cell_f32", ctx.handle, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, h.ptr, c.ptr, N, H)
        h64, C64, *_ = R.lstm_cell64(gx, gh, b, cp)
        th, tc = R.lstm_cell_bound(gx, gh, b, cp)
        worst[0] = max(worst[0], R.check(h.get(), h64, th, "lstm h %s" % ((N, H, spread),)))
        worst[1] = max(worst[1], R.check(c.get(), C64, tc, "lstm c %s" % ((N, H, spread),)))
    _report("lstm cell h", worst[0])
    _report("lstm cell c", worst[1])

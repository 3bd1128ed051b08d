"""CPU checks of tests/ref64_ops.py: the float64 references equal numpy on integer data, every lam covers 4x its float32
emulation over the calibration set, and for each family a named mutation that the per-tensor check (conftest.assert_close)
lets through fails the per-element bound."""
import numpy as np
import pytest

from oracle import planer_np as onp
from tests import ref64_ops as R
from tests.conftest import RTOL, rel_err


def _ints(seed, shape):
    return np.random.default_rng(seed).integers(-8, 9, shape).astype(np.float32)


def test_references_equal_numpy_on_integer_data():
    x = _ints(1, (6, 257))
    for op, f in enumerate([np.sum, np.mean, np.max, np.min]):
        assert (R.reduce64(x, op) == f(x.astype(np.int64) if op != 1 else x.astype(np.float64), axis=-1)).all()
    xs = _ints(2, (5, 40)) / 4
    np.testing.assert_allclose(R.softmax64(xs), onp.softmax(xs.astype(np.float64)), rtol=1e-15)
    np.testing.assert_allclose(R.softmax64(xs, True), onp.logsoftmax(xs.astype(np.float64)), rtol=1e-15, atol=1e-15)
    x4 = _ints(3, (2, 3, 4, 5)).astype(np.float64)
    s, b = np.array([1.0, -2.0, 0.5]), np.array([0.0, 1.0, -3.0])
    want = onp.instancenorm(x4.copy(), s.copy(), b.copy(), epsilon=float(np.float32(1e-5)))
    got = R.instancenorm64(x4.reshape(6, 20), np.tile(s, 2), np.tile(b, 2)).reshape(x4.shape)
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=1e-14)
    xi = _ints(4, (2, 3, 5, 6))
    for fh, fw in [(2, 2), (4, 4), (1, 2), (2, 1)]:             # float16 weights of 2^k factors: multiples of 2^-6, exact
        assert (R.upsample_linear64(xi, fh, fw) == onp.upsample_bilinear(xi.astype(np.float64), fh, fw)).all()
        assert (R.emulate_upsample_linear(xi, fh, fw) == R.upsample_linear64(xi, fh, fw)).all()
    np.testing.assert_allclose(R.resize_linear64(xi, 9, 13), onp.upsample_to_size(xi, (9, 13)), rtol=1e-6, atol=1e-5)
    assert (R.emulate_resize_linear(xi, 9, 13) == onp.upsample_to_size(xi, (9, 13))).all()     # the reference's roundings
    gx, _, b, cp = R.lstm_operands(np.random.default_rng(4), 3, 5)
    gx, b = np.round(gx), np.round(b)                                 # integer gates: the float32 sums are exact
    Y, h, c = onp.lstm(gx[None].astype(np.float64), np.eye(20)[None], np.zeros((1, 20, 5)), B=b[None].astype(np.float64),
                       initial_h=np.zeros((1, 3, 5)), initial_c=cp[None].astype(np.float64))
    h64, C64, *_ = R.lstm_cell64(gx, np.zeros_like(gx), b, cp)
    np.testing.assert_allclose(h64, h, rtol=1e-14, atol=1e-300)
    np.testing.assert_allclose(C64, c[0], rtol=1e-14, atol=1e-300)


def test_lambdas_cover_their_float32_emulation():
    worst = {}
    for n, dc, x in R.calibration_cases():
        def upd(k, v):
            worst[k] = max(worst.get(k, 0.0), float(v))
        upd("sum", R.ratio(R.emulate_rowsum(x), R.reduce64(x, 0), R.sum_bound(x, 1.0)).max())
        upd("sum", R.ratio(R.emulate_mean(x), R.reduce64(x, 1), R.mean_bound(x, 1.0)).max())
        upd("sum", R.ratio(R.emulate_gap(x), R.reduce64(x, 1), R.mean_bound(x, 1.0)).max())
        if n > 1:
            xs = (x - dc) * 4
            for log, k in ((False, "softmax"), (True, "logsoftmax")):
                upd(k, R.ratio(R.emulate_softmax(xs, log), R.softmax64(xs, log), R.softmax_bound(xs, log, 1.0)).max())
            rng = np.random.default_rng(n)
            s = (rng.standard_normal(x.shape[0]) * 2.0 ** rng.uniform(-10, 6, x.shape[0])).astype(np.float32)
            b = rng.standard_normal(x.shape[0]).astype(np.float32)
            upd("instancenorm", R.ratio(R.emulate_instancenorm(x, s, b), R.instancenorm64(x, s, b),
                                        R.instancenorm_bound(x, s, b, lam=1.0)).max())
    rng = np.random.default_rng(3)
    for dc in (0.0, 50.0):
        for fh, fw in [(2, 2), (4, 4), (3, 3), (1, 2), (2, 1), (8, 8), (3, 5)]:
            x = (rng.standard_normal((2, 6, 9, 11)) * 2.0 ** rng.uniform(-10, 6, (1, 6, 1, 1)) + dc).astype(np.float32)
            worst["upsample_linear"] = max(worst.get("upsample_linear", 0.0), float(R.ratio(
                R.emulate_upsample_linear(x, fh, fw), R.upsample_linear64(x, fh, fw), R.upsample_linear_bound(x, fh, fw, 1.0)).max()))
        for oh, ow in [(13, 17), (5, 7), (20, 30), (9, 11)]:
            x = (rng.standard_normal((2, 6, 9, 11)) * 2.0 ** rng.uniform(-10, 6, (1, 6, 1, 1)) + dc).astype(np.float32)
            worst["resize_linear"] = max(worst.get("resize_linear", 0.0), float(R.ratio(
                R.emulate_resize_linear(x, oh, ow), R.resize_linear64(x, oh, ow), R.resize_linear_bound(x, oh, ow, 1.0)).max()))
    assert set(worst) == set(R.LAM)
    for k, v in worst.items():
        assert R.LAM[k] >= 4 * v, "%s: lam %g < 4 x %g" % (k, R.LAM[k], v)
    assert all(v <= 4 for v in R.ULP.values())


def _skewed(rng, rows, n):
    x = R.skewed_rows(rng, rows, n)
    x[0] *= 2.0 ** -10 / np.abs(x[0]).max()           # one row 2^-10 beside rows up to 2^6
    return x


def test_mutation_reduction_drops_last_lane():
    """Rows up to 2^6 with zero runs (post-ReLU) where lane 63 reads, beside one row of magnitude 2^-10."""
    x = _skewed(np.random.default_rng(5), 8, 4096)
    x[1:, 63::64] = 0
    bad = x.copy()
    bad[:, 63::64] = 0                                  # lane 63's partial sum never joins the tree
    y = R.emulate_rowsum(bad)
    ref = R.reduce64(x, 0)
    assert rel_err(y, ref) <= RTOL
    with pytest.raises(AssertionError):
        R.check(y, ref, R.sum_bound(x), "reducesum, lane 63 dropped")
    R.check(R.emulate_rowsum(x), ref, R.sum_bound(x), "reducesum")


def test_mutation_gap_q4_reads_neighbour_channel():
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((8, 49)) * 2.0 ** np.array([6, 3, 0, -2, 4, 1, -10, -10])[:, None]).astype(np.float32)
    bad = x.copy()
    bad[6, 5] = x[7, 5]                                 # channel 6 (2^-10) of a partial quad reads channel 7 in one lane
    y = R.emulate_gap(bad)
    ref = R.reduce64(x, 1)
    assert rel_err(y, ref) <= RTOL
    with pytest.raises(AssertionError):
        R.check(y, ref, R.mean_bound(x), "gap q4, neighbour channel")
    R.check(R.emulate_gap(x), ref, R.mean_bound(x), "gap")


def test_mutation_softmax_flushes_subnormals():
    """Logits spread over more than 87 units: some outputs are subnormal, and a kernel that flushed them would pass."""
    rng = np.random.default_rng(8)
    x = (rng.uniform(-100, 0, (16, 300))).astype(np.float32)
    y = R.emulate_softmax(x)
    ref = R.softmax64(x)
    assert ((ref > 0) & (ref < 2.0 ** -126)).any()
    R.check(y, ref, R.softmax_bound(x), "softmax")
    flushed = np.where(np.abs(y) < 2.0 ** -126, 0, y)
    assert rel_err(flushed, ref) <= RTOL
    with pytest.raises(AssertionError):
        R.check(flushed, ref, R.softmax_bound(x), "softmax, subnormals flushed")


def _fast_exp(v):
    """exp2f(x * log2e) with the product rounded to float32: an error that grows with |x|."""
    v = np.asarray(v, np.float32)
    return np.exp2((v * np.float32(np.log2(np.e))).astype(np.float32).astype(np.float64)).astype(np.float32)


def test_mutation_sigmoid_fast_math_exp():
    x = np.linspace(-87, 30, 20001).astype(np.float32)
    ref = 1 / (1 + np.exp(-x.astype(np.float64)))
    with np.errstate(over="ignore"):
        y = (np.float32(1) / (_fast_exp(-x) + np.float32(1))).astype(np.float32)
    assert rel_err(y, ref) <= RTOL
    assert R.ulps(y, ref).max() > R.ULP["sigmoid"]


def test_mutation_instancenorm_one_pass_variance():
    rng = np.random.default_rng(9)
    x = np.concatenate([(50 + 2.0 ** -4 * rng.standard_normal((1, 196))),
                        2.0 ** 6 * rng.standard_normal((3, 196))]).astype(np.float32)
    s = np.array([2.0 ** -10, 2.0 ** 6, 1.0, 4.0], np.float32)
    b = np.array([0.0, 1.0, -1.0, 0.5], np.float32)
    ref = R.instancenorm64(x, s, b)
    y = R.emulate_instancenorm(x, s, b, two_pass=False)
    assert rel_err(y, ref) <= RTOL
    with pytest.raises(AssertionError):
        R.check(y, ref, R.instancenorm_bound(x, s, b), "instancenorm, one-pass variance")
    R.check(R.emulate_instancenorm(x, s, b), ref, R.instancenorm_bound(x, s, b), "instancenorm")


def test_mutation_transcendental_fast_exp_exceeds_ulp_cap():
    x = np.linspace(-87, 88, 20001).astype(np.float32)
    ref = np.exp(x.astype(np.float64))
    fast = _fast_exp(x)
    assert rel_err(fast, ref) <= RTOL
    assert R.ulps(fast, ref).max() > R.ULP["exp"]
    assert R.ulps(ref.astype(np.float32), ref).max() <= 0.5


def test_mutation_mean_drops_last_lane():
    x = _skewed(np.random.default_rng(15), 8, 4096)
    x[1:, 63::64] = 0
    bad = x.copy()
    bad[:, 63::64] = 0
    ref = R.reduce64(x, 1)
    assert rel_err(R.emulate_mean(bad), ref) <= RTOL
    with pytest.raises(AssertionError):
        R.check(R.emulate_mean(bad), ref, R.mean_bound(x), "reducemean, lane 63 dropped")
    R.check(R.emulate_mean(x), ref, R.mean_bound(x), "reducemean")


def test_mutation_logsoftmax_subtracts_m_plus_log_s():
    """t = x - (m + log s): one rounding of m + log s at the size of m, which a DC offset makes large."""
    rng = np.random.default_rng(16)
    x = (rng.standard_normal((16, 300)) * 4 + 1000).astype(np.float32)
    m = x.max(-1, keepdims=True)
    s = R.emulate_rowsum(np.exp((x - m).astype(np.float64)).astype(np.float32))[:, None]
    bad = (x - (m + np.log(s.astype(np.float64)).astype(np.float32)).astype(np.float32)).astype(np.float32)
    ref = R.softmax64(x, True)
    assert rel_err(bad, ref) <= RTOL
    with pytest.raises(AssertionError):
        R.check(bad, ref, R.softmax_bound(x, True), "logsoftmax, x - (m + log s)")
    R.check(R.emulate_softmax(x, True), ref, R.softmax_bound(x, True), "logsoftmax")


def test_mutation_matmul_drops_last_k():
    from tests import ref64 as R64
    rng = np.random.default_rng(17)
    x = (rng.standard_normal((16, 300)) * 2.0 ** rng.uniform(0, 6, (16, 1))).astype(np.float32)
    x[0] *= 2.0 ** -16
    x[1:, -1] = 0
    y = rng.standard_normal((300, 40)).astype(np.float32)
    xc, kc = x.reshape(16, 300, 1, 1), y.T.reshape(40, 300, 1, 1)
    ref, tol = R64.ref64(xc, kc).reshape(16, 40), R64.bound(xc, kc).reshape(16, 40)
    bad = x[:, :-1] @ y[:-1]
    assert rel_err(bad, ref) <= RTOL
    with pytest.raises(AssertionError):
        R64.check(bad, ref, tol, "matmul, last k dropped")
    R64.check(x @ y, ref, tol, "matmul")


def test_mutation_hardsigmoid_fused_multiply_add():
    """x * alpha + beta contracted to one fma: off by an ulp where the two roundings differ."""
    x = np.linspace(-4, 4, 100003).astype(np.float32)
    a, b = np.float32(0.2), np.float32(0.5)
    want = np.clip(x * a + b, 0, 1)
    fused = np.clip((x.astype(np.float64) * a + b).astype(np.float32), 0, 1)
    assert rel_err(fused, want) <= RTOL
    assert (fused != want).any()


def test_mutation_upsample_linear_drops_a_corner():
    rng = np.random.default_rng(18)
    x = (rng.standard_normal((1, 4, 9, 11)) * 2.0 ** np.array([6, 3, 0, -10])[None, :, None, None]).astype(np.float32)
    bad = R.emulate_upsample_linear(x, 2, 2, drop_last=True)
    good = R.emulate_upsample_linear(x, 2, 2)
    bad = np.concatenate([good[:, :3], bad[:, 3:]], axis=1)       # only the 2^-10 plane is wrong
    ref = R.upsample_linear64(x, 2, 2)
    assert rel_err(bad, ref) <= RTOL
    with pytest.raises(AssertionError):
        R.check(bad, ref, R.upsample_linear_bound(x, 2, 2), "upsample_linear, last corner dropped")
    R.check(good, ref, R.upsample_linear_bound(x, 2, 2), "upsample_linear")


def test_mutation_resize_linear_uses_unrounded_complement():
    """1 - cs taken in float64 instead of rounded to float32 like the reference: within the bound but no longer
    the reference's roundings, so the bit-exact special-values check is what catches it; the bound still holds."""
    rng = np.random.default_rng(19)
    x = (rng.standard_normal((2, 3, 9, 11)) * 2.0 ** np.array([6, 0, -10])[None, :, None, None]).astype(np.float32)
    ref = R.resize_linear64(x, 13, 17)
    R.check(R.emulate_resize_linear(x, 13, 17), ref, R.resize_linear_bound(x, 13, 17), "resize_linear")
    bad = R.emulate_resize_linear(x, 13, 17).copy()
    bad[:, 2] = R.emulate_resize_linear(x[:, 2:] * np.float32(1 + 2.0 ** -20), 13, 17)[:, 0]   # a 16-ulp drift in one plane
    assert rel_err(bad, ref) <= RTOL
    with pytest.raises(AssertionError):
        R.check(bad, ref, R.resize_linear_bound(x, 13, 17), "resize_linear, drifted plane")


def test_mutation_erf_table_from_float_erff():
    """A table built with a float32 erff (up to 2 ulp) instead of the double erf rounded once: per-tensor it passes."""
    import math
    lut = np.array([math.erf(i / 256 - 2) for i in range(1025)], np.float32)
    bad = lut + np.where(np.arange(1025) % 3 == 0, 2, 0) * np.spacing(np.abs(lut))
    x = np.linspace(-3, 3, 4001).astype(np.float32)
    idx = ((np.clip(x.astype(np.float64), -2, 2) + 2) * 256).astype(int)
    assert rel_err(bad[idx], lut[idx]) <= RTOL
    assert (bad[idx] != lut[idx]).any()


def test_mutation_lstm_fast_math_exp():
    rng = np.random.default_rng(20)
    gx, gh, b, cp = R.lstm_operands(rng, 16, 64, spread=30.0)
    fast = lambda v: np.exp2((np.asarray(v, np.float32) * np.float32(np.log2(np.e))).astype(np.float32)   # noqa: E731
                             .astype(np.float64)).astype(np.float32)
    h64, C64, *_ = R.lstm_cell64(gx, gh, b, cp)
    th, tc = R.lstm_cell_bound(gx, gh, b, cp)
    with np.errstate(over="ignore"):
        h, C = R.emulate_lstm_cell(gx, gh, b, cp, exp=fast)
    assert rel_err(h, h64) <= RTOL and rel_err(C, C64) <= RTOL
    with pytest.raises(AssertionError):
        R.check(h, h64, th, "lstm h, fast-math exp")
    h, C = R.emulate_lstm_cell(gx, gh, b, cp)
    R.check(h, h64, th, "lstm h")
    R.check(C, C64, tc, "lstm c")

"""The float64 reference and the per-element bounds of tests/ref64.py, on the CPU (no GPU): ref64 against an int64 conv, the
float32 oracle inside bound(LAMBDA["direct"]), each Winograd LAMBDA against a float32 emulation of its transforms, and
mutations that the per-element check catches and the per-tensor assert_close (1e-4 of max|ref|) lets through."""
import zlib
from fractions import Fraction

import numpy as np
import pytest

from oracle import planer_np as onp
from tests import ref64 as R
from tests.conftest import RTOL, assert_close

GEOMS = R.geometries()
TAILS = [(False, False, False, R.ACT_NONE), (True, True, False, R.ACT_RELU), (False, True, True, R.ACT_LEAKY),
         (True, True, True, R.ACT_RELU | R.ACT_RES_AFTER), (True, False, True, R.ACT_LEAKY | R.ACT_RES_AFTER)]


def conv_int64(x, K, group=1, strides=(1, 1), dilations=(1, 1), pads=(0, 0, 0, 0)):
    """Direct conv in int64: one strided slice per tap, einsum over the group's channels."""
    x, K = x.astype(np.int64), K.astype(np.int64)
    n, cin, h, w = x.shape
    cout, cg, kh, kw = K.shape
    (sh, sw), (dh, dw), (ph, pw) = strides, dilations, pads[:2]
    ho = (h + 2 * ph - (kh - 1) * dh - 1) // sh + 1
    wo = (w + 2 * pw - (kw - 1) * dw - 1) // sw + 1
    xp = np.zeros((n, cin, h + 2 * ph, w + 2 * pw), np.int64)
    xp[:, :, ph:ph + h, pw:pw + w] = x
    xg = xp.reshape(n, group, cg, h + 2 * ph, w + 2 * pw)
    Kg = K.reshape(group, cout // group, cg, kh, kw)
    y = np.zeros((n, group, cout // group, ho, wo), np.int64)
    for a in range(kh):
        for b in range(kw):
            tap = xg[:, :, :, a * dh:a * dh + (ho - 1) * sh + 1:sh, b * dw:b * dw + (wo - 1) * sw + 1:sw]
            y += np.einsum("ngchw,goc->ngohw", tap, Kg[:, :, :, a, b])
    return y.reshape(n, cout, ho, wo)


@pytest.mark.parametrize("geom", GEOMS, ids=[g[0] for g in GEOMS])
def test_ref64_equals_an_int64_conv_on_integer_operands(geom):
    name, xs, ks, conv = geom
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    for i, (bias, bn, res, act) in enumerate(TAILS):
        x, K, B, sc, sh, r = R.int_operands(rng, xs, ks, bias, bn, res, **conv)
        R.assert_exact(x, K, B, sc, sh, r, **conv)
        y = R.ref64(x, K, B, sc, sh, r, act, R.ALPHA, **conv)
        want = conv_int64(x, K, **conv).astype(np.float64)
        if B is not None:
            want = want + B.reshape(1, -1, 1, 1)
        if sc is not None:
            want = want * sc.reshape(1, -1, 1, 1) + sh.reshape(1, -1, 1, 1)
        if r is not None and not act & R.ACT_RES_AFTER:
            want = want + r
        if act & 15 == R.ACT_RELU:
            want = np.maximum(want, 0.0)
        elif act & 15 == R.ACT_LEAKY:
            want = np.where(want > 0, want, want * R.ALPHA)
        if r is not None and act & R.ACT_RES_AFTER:
            want = want + r
        np.testing.assert_array_equal(y, want, err_msg="%s tail %d" % (name, i))
        # the operands round-trip through fp32 unchanged, and the fp32 result of ref64 is itself exact
        np.testing.assert_array_equal(y.astype(np.float32).astype(np.float64), y)


def test_integer_operands_have_the_promised_form():
    rng = np.random.default_rng(0)
    x, K, B, sc, sh, r = R.int_operands(rng, (2, 6, 9, 11), (8, 6, 3, 3), True, True, True, pads=[1, 1, 1, 1])
    assert x.min() >= -3 and x.max() <= 3 and np.all(x == np.round(x))
    assert np.any(np.all(x == 0, axis=(0, 2, 3)))                      # a whole zero channel
    assert np.mean(x == 0) > 0.2                                       # zero runs beside the zero channel
    assert set(np.abs(sc).tolist()) <= {0.5, 1.0, 2.0, 4.0}
    assert np.all(sh * 4 == np.round(sh * 4)) and np.all(B == np.round(B)) and np.all(r == np.round(r))
    with pytest.raises(AssertionError):                                # the host precondition is a real check
        R.assert_exact(np.full((1, 16384, 3, 3), 3.0), np.full((1, 16384, 3, 3), 3.0), pads=[1, 1, 1, 1])


@pytest.mark.parametrize("geom", GEOMS, ids=[g[0] for g in GEOMS])
def test_fp32_oracle_lies_within_the_direct_bound(geom):
    """The float32 oracle (an sgemm) inside bound(LAMBDA["direct"]) on skewed and DC-offset float operands: the direct bar
    is calibrated on the CPU."""
    name, xs, ks, conv = geom
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    for dc in (0.0, 50.0):
        x, K, sc = R.skewed_operands(rng, xs, ks, dc=dc)
        B = rng.standard_normal(ks[0]).astype(np.float32)
        sh = (rng.standard_normal(ks[0]) * 2.0 ** rng.uniform(-10, 6, ks[0])).astype(np.float32)
        want = R.ref64(x, K, B, sc, sh, None, R.ACT_RELU, **conv)
        y = onp.relu(onp.batchnorm(np.ascontiguousarray(onp.conv2d(x, K, B, **conv)), sc.reshape(1, -1, 1, 1),
                                   sh.reshape(1, -1, 1, 1)))
        R.check(y, want, R.bound(x, K, B, sc, sh, None, R.LAMBDA["direct"], **conv), "oracle fp32 %s dc %g" % (name, dc))


@pytest.mark.parametrize("fam", sorted(R.LAMBDA))
def test_each_lambda_covers_its_float32_emulation(fam):
    """LAMBDA[fam] >= 4x the worst err / (u sqrt(Kred) L2) of the family's float32 emulation (the oracle's sgemm for
    "direct", where the constant is the issue's starting value and must only cover the ratio itself)."""
    worst = 0.0
    for name, x, K in R.calibration_cases():
        if fam == "wino43" and (x.shape[2] % 7 or x.shape[3] % 7):
            continue
        worst = max(worst, R.emulation_ratio(fam, x, K))
    need = worst if fam == "direct" else 4 * worst
    assert 0 < need <= R.LAMBDA[fam], (fam, worst, R.LAMBDA[fam])


@pytest.mark.parametrize("fam", ["f2x2", "f4x4", "w1d4", "wino43"])
def test_winograd_emulations_compute_the_conv(fam):
    rng = np.random.default_rng(5)
    for h, w in [(7, 7), (14, 14), (9, 13), (1, 1), (5, 2)]:
        if fam == "wino43" and (h % 7 or w % 7):
            continue
        x = rng.standard_normal((2, 3, h, w))
        K = rng.standard_normal((4, 3, 3, 3))
        got = R.wino_emulate(x, K, *R.wino_family(fam, h, w), dtype=np.float64)
        np.testing.assert_allclose(got, R.conv64(x, K, pads=[1, 1, 1, 1]), rtol=0, atol=1e-11)


def test_f2x2_emulation_is_bit_exact_on_integer_operands():
    """The premise of the exact GPU tests of F(2x2,3x3): on integer operands every transform and sum is exact in fp32."""
    rng = np.random.default_rng(6)
    for n, c, h, w, co in [(2, 16, 14, 14, 8), (1, 64, 7, 7, 12), (3, 5, 9, 13, 6), (1, 256, 4, 4, 4)]:
        x, K, B, sc, sh, r = R.int_operands(rng, (n, c, h, w), (co, c, 3, 3), True, True, True, pads=[1, 1, 1, 1])
        R.winograd_f2_assert_exact(x, K, B, sc, sh, r)
        got = R.wino_emulate(x, K, *R.wino_family("f2x2", h, w))
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, R.conv64(x, K, pads=[1, 1, 1, 1]))


# ---- mutations: the per-element check fails them, the per-tensor criterion does not ------------------------------------
def _skewed_case(cout=6, cin=2):
    """Skewed float operands with low-magnitude output channels 4 and 5 (scales 2^-14, 10 % apart) in a partial quad and
    channel 0 scaled by 1e-3 beside channels scaled by 1e3; Cin 2 and 3x3 filters keep Kred small (18)."""
    rng = np.random.default_rng(77)
    xs, ks = (2, cin, 9, 11), (cout, cin, 3, 3)
    conv = dict(pads=[1, 1, 1, 1])
    x, K, sc = R.skewed_operands(rng, xs, ks, lo=-2, hi=2)
    sc = np.abs(sc) * 1e3
    sc[0] = 1e-3
    sc[4] = 2.0 ** -14
    sc[5] = sc[4] * 1.1
    sh = np.zeros(cout, np.float32)
    want = R.ref64(x, K, None, sc, sh, **conv)
    y32 = onp.batchnorm(np.ascontiguousarray(onp.conv2d(x, K, **conv)), sc.reshape(1, -1, 1, 1), sh.reshape(1, -1, 1, 1))
    tol = R.bound(x, K, None, sc, sh, None, R.LAMBDA["direct"], **conv)
    R.check(y32, want, tol, "unmutated")
    return x, K, sc, sh, conv, y32, want, tol


def _fails_check_passes_assert_close(y, y32, want, tol, what):
    with pytest.raises(AssertionError):
        R.check(y, want, tol, what)
    assert_close(y, y32, RTOL, what)                    # the old criterion: the same mutation passes
    assert_close(y, want, RTOL, what)


def test_mutation_drop_one_tap_at_a_border_pixel():
    x, K, sc, sh, conv, y32, want, tol = _skewed_case()
    c = 4
    # pixel (0, c, 0, 0): taps (ky, kx) >= (1, 1) land inside the map; drop the largest one
    contrib = [(abs(float(x[0, ci, ky - 1, kx - 1]) * float(K[c, ci, ky, kx])), ci, ky, kx)
               for ci in range(x.shape[1]) for ky in (1, 2) for kx in (1, 2)]
    _, ci, ky, kx = max(contrib)
    y = y32.copy()
    y[0, c, 0, 0] = np.float32(y[0, c, 0, 0] - np.float32(x[0, ci, ky - 1, kx - 1] * K[c, ci, ky, kx] * sc[c]))
    _fails_check_passes_assert_close(y, y32, want, tol, "dropped tap")


def test_mutation_neighbour_scale_in_one_lane_of_a_partial_quad():
    x, K, sc, sh, conv, y32, want, tol = _skewed_case()
    y = y32.copy()
    raw = np.ascontiguousarray(onp.conv2d(x, K, **conv))
    y[:, 4] = raw[:, 4] * sc[5] + sh[4]                 # lane 0 of the last quad (channels 4, 5) reads channel 5's scale
    _fails_check_passes_assert_close(y, y32, want, tol, "scale of c+1")


def test_mutation_64_ulp_in_a_channel_scaled_by_1e_minus_3():
    x, K, sc, sh, conv, y32, want, tol = _skewed_case()
    y = y32.copy()
    i = np.unravel_index(int(np.argmax(np.abs(y[:, 0]))), y[:, 0].shape)
    at = (i[0], 0, i[1], i[2])
    y[at] = y[at] + 64 * np.spacing(np.abs(y[at]))
    _fails_check_passes_assert_close(y, y32, want, tol, "64 ulp")


def test_check_reports_the_worst_element_and_treats_signed_zeros_as_equal():
    ref = np.zeros((1, 2, 3, 3))
    y = -np.zeros((1, 2, 3, 3), np.float32)
    assert R.check(y, ref, 0.0) == 0.0
    y[0, 1, 2, 1] = 1e-3
    with pytest.raises(AssertionError, match=r"element \(0, 1, 2, 1\).*err/tol inf"):
        R.check(y, ref, 0.0, "probe", "plan-x")
    with pytest.raises(AssertionError, match=r"probe \[plan-x\].*err/tol 2"):
        R.check(y, ref, np.full(ref.shape, 5e-4), "probe", "plan-x")


# ---- operands on which the F(4,3) / F(3,3) Winograd pipelines are exact (tests/test_gpu_wino_exact.py) -----------------------------
def _wino_exact_cases():
    from tests.test_gpu_wino_exact import FAMILIES
    return sorted(FAMILIES.items())


@pytest.mark.parametrize("shape,fams", _wino_exact_cases(), ids=["x".join(map(str, s)) for s, _ in _wino_exact_cases()])
def test_wino_exact_precondition_holds_on_every_gpu_shape(shape, fams):
    """For every shape the GPU module runs and every family it runs it on: the filter transform as the kernels write it is the
    exact integer U, the pipeline in absolute values stays below 2^24, the tail below 2^24 of its grain; and every input channel
    is live in some output channel's filter for Cin <= 128 (no idle K chunk)."""
    from tests.test_gpu_wino_exact import operands
    ops = operands(shape)
    x, K = ops[:2]
    assert set(np.unique(np.abs(K)).tolist()) <= {0.0, R.WINO_TAP} and np.all(x == np.round(x))
    for fam in sorted(fams):
        frac = R.wino_exact_assert(fam, *ops)
        assert 0.0 < frac < 1.0
    if shape[1] <= 128:
        assert (K != 0).any(axis=(0, 2, 3)).all(), "an input channel no filter reads"
    assert len({tuple(np.flatnonzero((K[co] != 0).any(axis=(1, 2)))) for co in range(shape[4])}) > (1 if shape[1] > 12 and shape[4] > 1 else 0)


def test_wino_exact_precondition_holds_on_the_phases_of_the_folded_convs():
    from tests.test_gpu_wino_exact import FOLD_SIDES, fold_phases, operands
    for side in FOLD_SIDES:
        shape = (2, 16, side, side, 16)
        _, K, _, sc, sh, _ = operands(shape)
        phases = list(fold_phases(shape))
        assert len(phases) == 4 and all(p.shape == (2, 16, -(-side // 2), -(-side // 2)) for p in phases)
        assert sum(float(np.abs(p).sum()) for p in phases) == float(np.abs(operands(shape)[0]).sum())
        for xph in phases:
            R.wino_exact_assert("f4x4", xph, K, None, sc, sh, xph)


def test_wino_exact_precondition_is_a_real_check():
    rng = np.random.default_rng(9)
    x, K, B, sc, sh, r = R.wino_exact_operands(rng, (1, 64, 8, 8), 4, True, True, True)
    R.wino_exact_assert("f4x4", x, K, B, sc, sh, r)
    dense = np.full((4, 64, 3, 3), R.WINO_TAP, np.float32)
    with pytest.raises(AssertionError, match="pipeline"):             # every tap live: the Winograd-domain sums pass 2^24
        R.wino_exact_assert("f4x4", np.full((1, 64, 8, 8), 3.0, np.float32), dense)
    for tap in (100.0, 577.0, 1.0):                                    # taps that are no multiple of 576: G g G^T is rounded
        Kbad = K.copy()
        Kbad[Kbad != 0] = tap
        with pytest.raises(AssertionError, match="filter transform"):
            R.wino_exact_assert("f4x4", x, Kbad)
    with pytest.raises(AssertionError, match="tail"):
        R.wino_exact_assert("f4x4", x, K, None, np.full(4, 2.0 ** 10, np.float32), sh, None)


def test_rounded_winograd_constants_times_multiples_of_24_are_exact():
    """fl(c) * (24 m) is the integer 24 m c for c in {1/6, 1/12, 1/24, 1/3, 2/3}, |m| <= 4096: each constant is off by exactly
    2^-25 of itself (one mantissa, 1.0101...b rounded up), less than half an ulp of the product."""
    f = np.float32
    m = np.arange(-4096, 4097)
    v = (24 * m).astype(np.float32)
    for num, den in ((1, 6), (1, 12), (1, 24), (1, 3), (2, 3)):
        c = f(num) / f(den)
        assert c.dtype == np.float32
        rel = (Fraction(float(c)) - Fraction(num, den)) / Fraction(num, den)          # exact rational arithmetic
        assert rel == Fraction(1, 2 ** 25), (num, den, rel)
        got = v * c
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.astype(np.int64), 24 * m * num // den, err_msg="%d/%d" % (num, den))
        assert np.all(got == np.round(got))


@pytest.mark.parametrize("fam", ["f4x4", "w1d4", "wino43"])
def test_float32_winograd_emulation_is_bit_exact_on_the_exact_operands(fam):
    """The premise of tests/test_gpu_wino_exact.py: with U from wino_filter_f32 (the kernels' two-stage float32 transform), a running
    channel sum and the integer B^T / A^T, all in float32, the pipeline gives the float64 conv in every bit, whatever the order of
    the channel sum (ascending, descending and shuffled)."""
    rng = np.random.default_rng(43)
    shapes = [(2, 4, 8, 8), (2, 20, 8, 8), (1, 8, 13, 17), (2, 16, 9, 10), (1, 64, 7, 7)]
    if fam == "wino43":
        shapes = [(1, 64, 7, 7), (2, 16, 14, 7), (1, 8, 21, 14)]
    for xs in shapes:
        x, K, B, sc, sh, r = R.wino_exact_operands(rng, xs, 8, True, True, True)
        R.wino_exact_assert(fam, x, K, B, sc, sh, r)
        want = R.conv64(x, K, pads=[1, 1, 1, 1])
        u = R.wino_filter_f32(K, fam)
        for order in (range(xs[1]), range(xs[1] - 1, -1, -1), rng.permutation(xs[1])):
            got, top = R.wino_pipeline(x, u, fam, np.float32, order=list(order))
            assert got.dtype == np.float32 and top < R.WINO_CAP
            np.testing.assert_array_equal(got.astype(np.float64), want, err_msg="%s %s" % (fam, xs))
        # and ref64.wino_emulate, whose U comes from a float32 matmul with the rounded G, is NOT this check: not asserted exact


@pytest.mark.parametrize("fam", ["f4x4", "w1d4", "wino43"])
def test_wino_abs_top_is_the_maximum_of_wino_emulate_abs(fam):
    """On maps of whole tiles the two agree; where tiles run past the map, wino_emulate_abs crops them and the cap counts them whole."""
    rng = np.random.default_rng(8)
    for xs, whole in [((2, 8, 14, 7), fam == "wino43"), ((1, 20, 8, 12), True), ((1, 8, 9, 10), False), ((2, 4, 5, 2), False)]:
        if fam == "wino43" and (xs[2] % 7 or xs[3] % 7):
            continue
        x, K = R.wino_exact_operands(rng, xs, 6)[:2]
        a = R.wino_emulate_abs(np.abs(x.astype(np.float64)), K.astype(np.float64), *R.wino_family(fam, xs[2], xs[3]))
        top = R.wino_abs_top(fam, x, K)
        assert top >= a.max() and (top == a.max() or not whole), (fam, xs, top, a.max())


def test_mixed_tile_input_reference_agrees_with_the_f4x4_one_on_its_shared_tiles():
    """wino43_input's F(4) x F(4) class on a 7 x 7 map is the first tile of wino4_input (same 6 x 6 patch, same B^T)."""
    rng = np.random.default_rng(12)
    x = rng.integers(-3, 4, (2, 6, 7, 7)).astype(np.float64)
    v43, v4 = R.wino43_input(x), R.wino4_input(x)
    assert v43.shape == (121, 2, 2, 4) and v4.shape == (36, 2, 8, 4)
    np.testing.assert_array_equal(v43[:36], v4[:, :, [0, 4], :])
    assert np.all(R.wino43_input(np.abs(x), True) >= np.abs(v43))

"""The polyphase F(4,4) form of the stem + max-pool kernel, without a device: the k order its filter pack and fragment reads share
(pl_conv2d_stem_wino_korder), and the float32 emulation of the whole form (tests/stem_wino_ref.py) against the float64 conv +
the oracle's pool within the bound the GPU tests use."""
import ctypes

import numpy as np
import pytest

from planer_amd import _lib
from tests import ref64 as R
from tests import stem_wino_ref as S
from tests.ref64 import ACT_NONE, ACT_RELU


def _korder():
    tab = (ctypes.c_int * 176)()
    _lib.call("pl_conv2d_stem_wino_korder", tab, 176)
    return np.array(tab[:], np.int64).reshape(44, 4)


def test_korder_holds_every_row_channel_phase_tap_once():
    t = _korder()
    real = t[t >= 0]
    assert sorted(real.tolist()) == list(range(147))                    # every tap of a [3][7][7] filter once
    k, a = np.nonzero(t >= 0)
    c, fr, kw = t[k, a] // 49, t[k, a] // 7 % 7, t[k, a] % 7
    assert (k == 6 * fr + 2 * c + (kw & 1)).all() and (a == kw // 2).all()  # k = (filter row, channel, phase), tap a = column 2 a + phase
    zeros = {(int(i), int(j)) for i, j in zip(*np.nonzero(t < 0))}
    assert zeros == {(k, 3) for k in range(1, 42, 2)} | {(k, a) for k in (42, 43) for a in range(4)}


def test_matrices_are_an_exact_f44():
    rng = np.random.default_rng(7)
    g, d = rng.integers(-4, 5, 4).astype(float), rng.integers(-4, 5, 7).astype(float)
    want = [sum(g[j] * d[i + j] for j in range(4)) for i in range(4)]
    np.testing.assert_allclose(S.AT @ ((S.G @ g) * (S.BT @ d)), want, rtol=0, atol=1e-12)


CASES = [((1, 3, 28, 32), 64, (False, False, False, ACT_NONE), 0.0), ((2, 3, 36, 40), 36, (False, True, False, ACT_RELU), 50.0),
         ((1, 3, 30, 64), 64, (True, False, False, ACT_NONE), 0.0)]


@pytest.mark.parametrize("xs,cout,tail,dc", CASES)
def test_float32_emulation_within_the_bound(xs, cout, tail, dc):
    from tests.test_gpu_conv_bounds import _operands
    (x, K, B, sc, sh, _), act, want = _operands("stem-wino", xs, (cout, 3, 7, 7), tail, dc, **S.CONV)
    y = S.emulate(x, K)
    chan = lambda a: a.reshape(1, -1, 1, 1)                            # noqa: E731
    if B is not None:
        y = y + chan(B)
    if sc is not None:
        y = y * chan(sc) + chan(sh)
    if act == ACT_RELU:
        y = y * (y > 0)
    assert y.dtype == np.float32
    worst = R.check(S.pooled(y), S.pooled(want), S.pooled(S.bound(x, K, B, sc, sh)), "emulation %s" % (xs,))
    print("emulation worst err / tol %.3g" % worst)


def test_lambda_is_four_times_the_emulations_worst_ratio():
    cases = list(S.calibration_cases())[1:]                             # (the full-size case is in the module docstring: 0.846)
    worst = max(S.emulation_ratio(x, K) for _, x, K in cases)
    print("emulation worst err / (u W) %.3g" % worst)
    assert 4 * worst <= S.LAMBDA and 4 * 0.846 <= S.LAMBDA < 4 * 0.846 + 0.5

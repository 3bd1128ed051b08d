"""The NCHW-reading stem + max-pool kernel (w_layout 12) with its packed k order: K = 148 (147 taps + one zero) instead of 176.
The k-order table the filter pack and the fragment reads share (sp_nchw_tap, read back through pl_conv2d_stem_nchw_korder) is
checked without a device; on the GPU the kernel equals the float64 reference bit for bit on integer operands at every pixel-block
count NB = 1..7 and on multi-chunk widths, stays within the direct-conv bound on float operands, and reports K = 148."""
import ctypes

import numpy as np
import pytest

from oracle import planer_np as onp
from planer_amd import _lib
from tests import ref64 as R
from tests.ref64 import ACT_LEAKY, ACT_NONE, ACT_RELU

CONV = dict(group=1, strides=[2, 2], dilations=[1, 1], pads=[3, 3, 3, 3])
POOL = dict(w=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2])
QUADS = 37


def _korder():
    tab = (ctypes.c_int * (4 * QUADS))()
    _lib.call("pl_conv2d_stem_nchw_korder", tab, 4 * QUADS)
    return np.array(tab[:], np.int64).reshape(QUADS, 4)


def test_korder_holds_every_tap_once_and_one_zero():
    t = _korder()
    assert (t >= 0).all()                                    # 148 slots: no slot without a tap or a zero
    rho, kw = t >> 3, (t & 7) - 1
    real = kw >= 0
    assert int((~real).sum()) == 1                           # the one zero: (kw -1) of row 20
    taps = sorted(zip(rho[real].tolist(), kw[real].tolist()))
    assert taps == [(r, k) for r in range(21) for k in range(7)]
    assert (rho < 21).all()


def test_korder_reads_are_aligned_and_half_waves_two_rows_apart():
    """Groups 0-8: elements (0, 1) are one 8-byte aligned pair of one row (a tap kw at float 2 l + kw + 1 of its row); groups
    0-6 also (2, 3).  The quarters a half-wave reads together (kk = 0, 1 and 2, 3) sit two rows apart (32 banks mod 64) in
    every b64 read except group 8's row-20 pairs."""
    t = _korder()
    rho, f = t >> 3, t & 7                                   # f = kw + 1: the float offset in the row
    q = t[:36].reshape(9, 4, 4)                              # [group][quarter][element]
    for u in range(9):
        pairs = [0, 2] if u < 7 else [0]
        for j in pairs:
            for kk in range(4):
                a, b = q[u, kk, j], q[u, kk, j + 1]
                assert a >> 3 == b >> 3 and (a & 7) % 2 == 0 and (b & 7) == (a & 7) + 1, (u, kk, j)
            if u != 8:
                for k0 in (0, 2):
                    assert (q[u, k0 + 1, j] >> 3) - (q[u, k0, j] >> 3) == 2, (u, k0, j)
                    assert q[u, k0 + 1, j] & 7 == q[u, k0, j] & 7
    singles = np.concatenate([q[7:9, :, 2:].ravel(), t[36]])  # the kw-0 taps read one float each
    assert ((singles & 7) == 1).all()
    assert (rho.max(), f.max()) == (20, 7)


# ---- on the GPU -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _run(pa, x, K, B, sc, sh, act, alpha, strip_rows=0):
    from planer_amd import q4
    from tests.test_gpu_conv_exact import _dev
    dx, dB, dsc, dsh = (_dev(pa, a) for a in (x, B, sc, sh))
    y = q4.ConvPoolQ4(dx, q4.prepare_stem_nchw_weights(_dev(pa, K)), dB, dsc, dsh, act=act, alpha=alpha, w_layout=12,
                      strip_rows=strip_rows, **CONV)
    ctx = pa.hip.context()
    plan = ctx.last_conv_plan()
    assert plan.startswith("stem+maxpool(nchw)"), plan
    return q4.from_q4(y).get(), plan, ctx.last_conv_extents()


# widths -> NB: W / 2 conv columns in blocks of 16, one chunk up to 112 columns; 300, 400: two chunks, 452: three
WIDTHS = [(8, 1), (56, 2), (88, 3), (120, 4), (152, 5), (184, 6), (224, 7), (300, 5), (400, 7), (452, 5)]


@pytest.mark.gpu
def test_packed_k_is_bit_exact_at_every_block_count(pa):
    from tests.test_gpu_conv_exact import _case, _exact
    tails = [(False, True, False, ACT_RELU), (True, False, False, ACT_NONE), (True, True, False, ACT_LEAKY)]
    for i, (w, nb) in enumerate(WIDTHS):
        n, h, cout = (2, 37, 12) if i % 2 else (1, 30, 36)
        tail = tails[i % len(tails)]
        (x, K, B, sc, sh, _), act, want = _case("stem-kpack", (n, 3, h, w), (cout, 3, 7, 7), tail, **CONV)
        want = onp.maxpool(want.astype(np.float32), **POOL)
        for strip_rows in (0, 14):
            y, plan, ext = _run(pa, x, K, B, sc, sh, act, R.ALPHA, strip_rows)
            assert " x %dpx," % (16 * nb) in plan, plan
            assert ext[3] == 148, ext
            _exact(y, want, "stem kpack %s strip_rows %d" % ((n, h, w, cout), strip_rows), plan)
    for n, h, w, cout in [(1, 50, 36, 36), (3, 30, 8, 8), (1, 33, 100, 12), (2, 64, 64, 64), (1, 21, 224, 128)]:
        (x, K, B, sc, sh, _), act, want = _case("stem-kpack", (n, 3, h, w), (cout, 3, 7, 7), tails[0], **CONV)
        y, plan, _ = _run(pa, x, K, B, sc, sh, act, R.ALPHA)
        _exact(y, onp.maxpool(want.astype(np.float32), **POOL), "stem kpack %s" % ((n, h, w, cout),), plan)


@pytest.mark.gpu
def test_packed_k_within_the_direct_conv_bound(pa):
    from tests.test_gpu_conv_bounds import _check, _operands
    for n, h, w, cout, dc in [(2, 64, 224, 64, 0.0), (1, 40, 300, 36, 50.0), (2, 33, 56, 12, 50.0)]:
        ops, act, want = _operands("stem-kpack", (n, 3, h, w), (cout, 3, 7, 7), (False, True, False, ACT_RELU), dc, **CONV)
        x, K, B, sc, sh, _ = ops
        tol = onp.maxpool(R.bound(*ops, lam=R.LAMBDA["direct"], **CONV), **POOL)
        y, _, ext = _run(pa, x, K, B, sc, sh, act, 0.1)
        assert ext[3] == 148, ext
        _check(pa, y, ops, onp.maxpool(want, **POOL), "direct", "%s dc %g" % ((n, h, w, cout), dc), "stem-kpack", tol)

"""The polyphase F(4,4) form of the stem + max-pool kernel (csrc/conv_stem_wino_kernel.h) on the GPU: its prepared filter against
G g in numpy, the kernel against the float64 conv + the oracle's pool under the per-element bound of tests/stem_wino_ref.py
(LAMBDA = 3.5, calibrated on the float32 emulation; a pooled value is checked against the largest bound in its window), and the
pick through Net.  Worst err / tol of the kernel over these cases, measured on an MI355X: 0.265 ((3, 56, 224); 0.228 - 0.255 on
the others), where the emulation reaches 0.25 by construction."""
import numpy as np
import pytest

from tests import ref64 as R
from tests import stem_wino_ref as S
from tests.ref64 import ACT_NONE, ACT_RELU

pytestmark = pytest.mark.gpu
TAILS = [(False, False, False, ACT_NONE), (False, True, False, ACT_RELU), (True, False, False, ACT_NONE)]
# one strip of 4 tiles; partial last strip, 5 tiles; odd conv-row count; full width, 28 tiles, two strips; two column chunks
SHAPES = [(1, 28, 32), (2, 36, 40), (1, 30, 64), (3, 56, 224), (1, 28, 300)]


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _dev(pa, a):
    return None if a is None else pa.asarray(np.ascontiguousarray(a))


def test_prepared_filter_is_g_g(pa):
    from planer_amd import q4
    rng = np.random.default_rng(11)
    for cout in (64, 36):
        K = (rng.standard_normal((cout, 3, 7, 7)) * 2.0 ** rng.uniform(-6, 6, (cout, 1, 1, 1))).astype(np.float32)
        Kq = q4.prepare_stem_wino_weights(pa.asarray(K))
        got = Kq._view((7 * 11 * cout * 4,)).get()                                     # (the array keeps K's logical shape)
        got = got.reshape(7, 11, cout, 4).transpose(2, 0, 1, 3).reshape(cout, 7, 44).astype(np.float64)
        want = S.filter_freq(K).transpose(0, 4, 2, 1, 3).reshape(cout, 7, 42)          # [o][f][k = (fr, c, phase)]
        tol = 8 * S.U * S.filter_freq(np.abs(K), mat=np.abs(S.G)).transpose(0, 4, 2, 1, 3).reshape(cout, 7, 42)
        assert (np.abs(got[..., :42] - want) <= tol).all()
        assert (got[..., 42:] == 0).all()


def _run(pa, x, K, B, sc, sh, act, strip_rows):
    from planer_amd import q4
    dx, dB, dsc, dsh = (_dev(pa, a) for a in (x, B, sc, sh))
    y = q4.ConvPoolQ4(dx, q4.prepare_stem_wino_weights(_dev(pa, K)), dB, dsc, dsh, act=act, alpha=0.1, w_layout=12, wino=44,
                      strip_rows=strip_rows, **S.CONV)
    ctx = pa.hip.context()
    plan = ctx.last_conv_plan()
    assert plan.startswith("stem+maxpool(nchw) F(4,4)"), plan
    return q4.from_q4(y).get(), plan, ctx.last_conv_extents()


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_kernel_within_the_bound(pa, shape):
    from tests.test_gpu_conv_bounds import _operands
    n, h, w = shape
    worst = 0.0
    for t, tail in enumerate(TAILS):
        # Cout 64, and 36: a partial 64-channel block (the kernel pads it with zero filters)
        for cout, dc in ((64, 0.0), (36, 50.0)) if t == 1 else ((64, 50.0 if n > 1 else 0.0),):
            (x, K, B, sc, sh, _), act, want = _operands("stem-wino", (n, 3, h, w), (cout, 3, 7, 7), tail, dc, **S.CONV)
            want, tol = S.pooled(want), S.pooled(S.bound(x, K, B, sc, sh))
            for strip_rows in (0, 14):
                y, plan, ext = _run(pa, x, K, B, sc, sh, act, strip_rows)
                assert ext[0] == 7 and ext[3] == 44, ext
                r = R.check(y, want, tol, "stem F(4,4) %s cout %d tail %d strip_rows %d" % (shape, cout, t, strip_rows), plan)
                worst = max(worst, r)
    print("ratio stem-wino %.3g %s" % (worst, shape))


def test_unsupported_width_is_refused(pa):
    from planer_amd import q4
    assert not q4.stem_pool_wino_eligible((1, 3, 28, 30), (64, 3, 7, 7), **S.CONV)       # W % 4 != 0: the direct forms take it
    assert q4.stem_pool_eligible((1, 3, 28, 30), (64, 3, 7, 7), **S.CONV)
    assert q4.stem_pool_wino_eligible((1, 3, 28, 300), (64, 3, 7, 7), **S.CONV)


def test_net_picks_the_form_and_the_switch_restores_the_direct_kernel(pa, monkeypatch):
    """ResNet-18 at batch 2 @224 against the oracle under the net tolerance, with the form and with stem_wino=0, which launches
    the direct kernel (the logits of two nets are not compared bit for bit here: at a batch the shipped database does not hold,
    the other convs' kernels are timed picks)."""
    from oracle import planer_np as onp
    from planer_amd.irgen import resnet18
    from tests.conftest import RTOL, assert_close
    g, b = resnet18.build()
    x = resnet18.make_input(2)
    ref = onp.OracleNet()
    ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
    ref.load_weights(b)
    want = ref(x.copy())
    outs = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("PLANER_HIP_EXPERIMENT", "stem_wino=" + flag)
        net = pa.from_graph(g, b)
        plan = net.compile(pa.asarray(x))
        stem = [a["plan"] for a in plan.algos if a["kind"] == "conv_pool_q4"]
        assert len(stem) == 1 and stem[0].startswith("stem+maxpool(nchw)") and ("F(4,4)" in stem[0]) == (flag == "1"), stem
        outs[flag] = net(x)
        assert_close(outs[flag], want, RTOL)

"""The woven K step of the fused Winograd F(4x4,3x3) kernel's 16-tile blocks (csrc/conv_wf4_kernel.h, WEAVE: every wave's
patch-transform item of chunk c + 1 rides behind the MFMAs of chunk c) on a real MI355X.

The woven step runs the operations of the phased step (PLANER_HIP_EXPERIMENT=wf4_weave=0: the item as a phase of its own in
front of the MFMAs) in the same order on the same operands, so the two are compared bit for bit; both are held to the oracle
(util.conv_for + layer.BatchNorm / Add / ReLU / LeakyReLU) at the bound of tests/test_gpu_wf4.py, 3e-5 of max|ref|."""
import numpy as np
import pytest

from tests.conftest import assert_close
from tests.test_gpu_wino_chain import _act, _operands, _oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


# (N, Cin, H, W, Cout) -> what of the K loop and the block geometry the shape reaches
SHAPES = [((2, 4, 8, 8, 64), "one chunk: prologue only, no woven step feeds a multiply"),
          ((2, 8, 8, 8, 64), "one woven step plus the last"),
          ((2, 12, 8, 8, 40), "odd chunk count (tail of the two-step unroll), partial output-channel block"),
          ((1, 8, 12, 20, 64), "tile rows and columns past the map edge"),
          ((2, 16, 28, 28, 128), "two-image blocks with the padding column, two output-channel blocks"),
          ((8, 8, 56, 56, 64), "packed blocks")]
# no tail; scale + shift + ReLU; the same with a residual (the two straight-line tails); bias + leaky (the general tail)
TAILS = [(), ("bn", "relu"), ("bn", "res", "relu"), ("b", "leaky")]


@pytest.mark.parametrize("shape", [s for s, _ in SHAPES], ids=["x".join(map(str, s)) for s, _ in SHAPES])
def test_woven_step_equals_phased_step_bit_for_bit_and_the_oracle(pa, shape, monkeypatch):
    from planer_amd import q4
    n, cin, h, w, cout = shape
    rng = np.random.default_rng(17 + sum(shape))
    ctx = pa.hip.context()
    for tail in TAILS:
        host, dev = _operands(pa, rng, n, cin, h, w, cout, tail)
        u = q4.prepare_wf4_q4_weights(dev["k"])
        kw = dict(pads=(1, 1, 1, 1), act=_act(tail), alpha=0.1, w_layout=9)
        monkeypatch.setenv("PLANER_HIP_EXPERIMENT", "wf4_weave=1")
        woven = q4.ConvQ4(dev["xq"], u, dev["b"], dev["scale"], dev["shift"], dev["resq"], **kw)
        plan1 = ctx.last_conv_plan()
        monkeypatch.setenv("PLANER_HIP_EXPERIMENT", "wf4_weave=0")
        phased = q4.ConvQ4(dev["xq"], u, dev["b"], dev["scale"], dev["shift"], dev["resq"], **kw)
        plan0 = ctx.last_conv_plan()
        assert "16tiles woven" in plan1 and "woven" not in plan0 and "16tiles" in plan0, (plan1, plan0)
        assert plan1.replace(" woven", "") == plan0, (plan1, plan0)          # same block geometry
        if shape == (8, 8, 56, 56, 64):
            assert "packed" in plan1, plan1
        if shape == (2, 16, 28, 28, 128):
            assert "(2x1x8)" in plan1 and "blocks=14" in plan1, plan1
        assert q4.logical_shape(woven) == (n, cout, h, w)
        np.testing.assert_array_equal(woven.get(), phased.get(), err_msg="%s %s [%s]" % (shape, tail, plan1))
        ref = _oracle(host, tail)
        assert_close(q4.from_q4(woven).get(), ref, 3e-5, "woven %s %s [%s]" % (shape, tail, plan1))
        assert_close(q4.from_q4(phased).get(), ref, 3e-5, "phased %s %s [%s]" % (shape, tail, plan0))


def test_woven_step_is_the_default_and_the_32_tile_block_has_none(pa, monkeypatch):
    from planer_amd import q4
    rng = np.random.default_rng(9)
    x = q4.to_q4(pa.asarray(rng.standard_normal((2, 8, 12, 12)).astype(np.float32)))
    u = q4.prepare_wf4_q4_weights(pa.asarray((rng.standard_normal((8, 8, 3, 3)) * 0.1).astype(np.float32)))
    monkeypatch.delenv("PLANER_HIP_EXPERIMENT", raising=False)
    q4.ConvQ4(x, u, pads=(1, 1, 1, 1), w_layout=9)
    assert "16tiles woven" in pa.hip.context().last_conv_plan(), pa.hip.context().last_conv_plan()
    monkeypatch.setenv("PLANER_HIP_EXPERIMENT", "wf4_half=0,wf4_weave=1")
    q4.ConvQ4(x, u, pads=(1, 1, 1, 1), w_layout=9)
    plan = pa.hip.context().last_conv_plan()
    assert "32tiles" in plan and "woven" not in plan, plan

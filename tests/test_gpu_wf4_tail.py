"""Head and tail of the fused Winograd F(4x4,3x3) kernel's 16-tile blocks (csrc/conv_wf4_kernel.h, HALF) on a real MI355X: the first
K step that multiplies into a literal zero instead of cleared accumulators, the column sums of A^T m A computed once and in
place, the store offsets computed once per block and stepped by the row pitch.

The 32-tile block (PLANER_HIP_EXPERIMENT=wf4_half=0) keeps the head and tail these replace.  The two forms are NOT equal bit for
bit, before this change or after it: the 32-tile block transforms patch rows 1-4 as c (d1 +- d2) + (d4 +- d3) (wf4_bt_row2), the
16-tile block as c1 d1 + (c2 d2 + (c3 d3 + d4)) (wf4_transform_2rows and the woven item), which rounds differently.  So both
forms are held to the oracle (util.conv_for + layer.BatchNorm / Add / ReLU / LeakyReLU) at the bound of tests/test_gpu_wf4.py,
3e-5 of max|ref|, on float data.  On operands where every sum is exact whatever its grouping, both forms -- and the phased and
the plain-block ones -- must equal float64, and so each other, in every bit: tests/test_gpu_wino_exact.py
(test_fused_kernel_every_form_and_tail) holds them to that on these shapes."""
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


# (N, Cin, H, W, Cout) -> what of the new head and tail the shape reaches
CHUNKS = [((2, 4, 8, 8, 64), "one chunk: the first K step is the last"),
          ((2, 8, 8, 8, 64), "two chunks: the peeled step and one odd step, no even step"),
          ((2, 12, 8, 8, 64), "three chunks: odd count, one whole turn of the loop"),
          ((2, 16, 8, 8, 64), "four chunks: a turn and a half"),
          ((2, 20, 8, 8, 64), "five chunks: odd count, two turns")]
PARTIAL = [((2, 8, 8, 8, 40), "partial channel block: cq0 + q < Coq in the once-computed offsets")]
# rows 1-3 of the last tile row and columns of the last tile fall off the map one at a time
EDGES = [((1, 8, h, w, 8), "map %d x %d" % (h, w)) for h in (5, 6, 7, 8) for w in (5, 6, 7, 8)]
LARGER = [((1, 8, 12, 20, 64), "larger map with tile rows and columns past the map edge"),
          ((2, 16, 28, 28, 128), "two-image blocks, two channel blocks"),
          ((8, 8, 56, 56, 64), "packed blocks")]
SHAPES = [s for s, _ in CHUNKS + PARTIAL + EDGES + LARGER]
# no tail; scale + shift + ReLU; the same with a residual (the two straight-line tails); bias + leaky (the general tail)
TAILS = [(), ("bn", "relu"), ("bn", "res", "relu"), ("b", "leaky")]


def _conv(pa, dev, tail, form, monkeypatch):
    from planer_amd import q4
    monkeypatch.setenv("PLANER_HIP_EXPERIMENT", form)
    u = q4.prepare_wf4_q4_weights(dev["k"])
    y = q4.ConvQ4(dev["xq"], u, dev["b"], dev["scale"], dev["shift"], dev["resq"], pads=(1, 1, 1, 1), act=_act(tail), alpha=0.1,
                  w_layout=9)
    return y, pa.hip.context().last_conv_plan()


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_16_tile_and_32_tile_blocks_against_the_oracle(pa, shape, monkeypatch):
    from planer_amd import q4
    n, cin, h, w, cout = shape
    rng = np.random.default_rng(23 + sum(shape))
    for tail in TAILS:
        host, dev = _operands(pa, rng, n, cin, h, w, cout, tail)
        y16, plan16 = _conv(pa, dev, tail, "wf4_half=1", monkeypatch)
        y32, plan32 = _conv(pa, dev, tail, "wf4_half=0", monkeypatch)
        assert "16tiles woven" in plan16 and "32tiles" in plan32, (plan16, plan32)
        if shape == (8, 8, 56, 56, 64):
            assert "packed" in plan16, plan16
        if shape == (2, 16, 28, 28, 128):
            assert "(2x1x8)" in plan16 and "blocks=14" in plan16, plan16
        assert q4.logical_shape(y16) == (n, cout, h, w)
        ref = _oracle(host, tail)
        print("%s %s: max|16 - 32| = %.3g, max|ref| = %.3g" % (shape, tail, np.abs(y16.get() - y32.get()).max(), np.abs(ref).max()))
        assert_close(q4.from_q4(y16).get(), ref, 3e-5, "16 tiles %s %s [%s]" % (shape, tail, plan16))
        assert_close(q4.from_q4(y32).get(), ref, 3e-5, "32 tiles %s %s [%s]" % (shape, tail, plan32))


def _planted(pa):
    """(2, 16, 12, 12, 64), scale + shift + residual + ReLU, with NaN, +inf and -inf in x, the filter and the residual at channels
    of the first K step (input channels 0-3) and of the last (12-15)"""
    from planer_amd import q4
    tail = ("bn", "res", "relu")
    rng = np.random.default_rng(5)
    n, cin, h, w, cout = 2, 16, 12, 12, 64
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    k = (rng.standard_normal((cout, cin, 3, 3)) * (2.0 / (9 * cin)) ** 0.5).astype(np.float32)
    res = rng.standard_normal((n, cout, h, w)).astype(np.float32)
    x[0, 1, 1, 2] = np.nan
    x[0, 13, 6, 9] = np.inf
    x[1, 2, 10, 1] = -np.inf
    x[1, 14, 5, 5] = np.nan
    x[1, 12, 0, 11] = np.inf
    k[3, 0, 1, 1] = np.inf
    k[21, 15, 0, 2] = np.nan
    k[40, 3, 2, 0] = -np.inf
    k[63, 12, 1, 0] = np.inf
    res[0, 7, 11, 11] = np.nan
    res[1, 30, 4, 0] = np.inf
    res[1, 50, 8, 3] = -np.inf
    host = {"x": x, "k": k, "b": None, "res": res, "scale": rng.uniform(0.5, 1.5, (1, cout, 1, 1)).astype(np.float32),
            "shift": (rng.standard_normal((1, cout, 1, 1)) * 0.1).astype(np.float32)}
    dev = {key: (None if v is None else pa.asarray(v)) for key, v in host.items()}
    dev["xq"], dev["resq"] = q4.to_q4(dev["x"]), q4.to_q4(dev["res"])
    return host, dev, tail


def test_nan_and_inf_in_the_first_and_the_last_k_step(pa, monkeypatch):
    """a first step that multiplies into a literal zero must do what the cleared accumulator did: fma(a, b, +0), NaN and inf too"""
    host, dev, tail = _planted(pa)
    y16, plan16 = _conv(pa, dev, tail, "wf4_half=1", monkeypatch)
    y32, plan32 = _conv(pa, dev, tail, "wf4_half=0", monkeypatch)
    assert "16tiles woven" in plan16 and "32tiles" in plan32, (plan16, plan32)
    a, b = y16.get(), y32.get()
    assert np.isnan(a).any() and np.isfinite(a).any()
    # the phased 16-tile step (its own copy of the peeled first step) runs the woven step's operations: exact, NaN positions included
    yph, planph = _conv(pa, dev, tail, "wf4_weave=0", monkeypatch)
    assert "16tiles" in planph and "woven" not in planph, planph
    np.testing.assert_array_equal(a, yph.get(), err_msg="[%s] [%s]" % (plan16, planph))
    # the same NaNs and the same infinities in the same places; the finite values differ by the two forms' rounding, each within
    # 3e-5 of max|ref| of the oracle, so within 6e-5 of each other
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg="[%s] [%s]" % (plan16, plan32))
    inf = np.isinf(a)
    np.testing.assert_array_equal(inf, np.isinf(b))
    np.testing.assert_array_equal(a[inf], b[inf])
    fin = np.isfinite(a)
    print("planted: %d NaN, %d inf of %d; max|16 - 32| over the finite values %.3g of %.3g"
          % (np.isnan(a).sum(), inf.sum(), a.size, np.abs(a[fin] - b[fin]).max(), np.abs(b[fin]).max()))
    assert_close(a[fin], b[fin], 6e-5, "finite values [%s] [%s]" % (plan16, plan32))

"""References for the uint8 image input (pl_image_u8_nchw_f32): y[n][c] = fl(fl(r * k[c]) + b[c]).

`resize32` restates the reference's util.resize (util.py:253-269) on a uint8 image in numpy float32 with exactly its roundings:
columns first, t = fl(fl(p[ca] (1 - cs)) + fl(p[ca + 1] cs)), then rows on t the same way, 1 - cs and 1 - rs in float32.  It is
bit-equal to the reference's own outputs stored in tests/golden/image_input.npz (tests/test_image_input.py).

`resize64` is the same sum in float64 with the SAME float32 weights (cs, 1 - cs, rs, 1 - rs as float32 computes them: the
weights are operands, what is bounded is the rounding of the products and sums).

Bound per element, U = 2^-24 the unit roundoff of float32, first order:
  resized:    |y - y64| <= 7 U 255 |k_c| + U |y64|   six roundings of magnitudes up to 255 in the two resize stages (two
                                                     products and a sum each), then the product by k, then the sum with b
  not resized: |y - y64| <= U 255 |k_c| + U |y64|    the product, then the sum
"""
import numpy as np

U = 2.0 ** -24


def axis_samples(n, size):
    """util.resize's sample positions along one axis (util.py:256-266): (integer part, float32 fraction)."""
    k = size / n
    pos = np.linspace(-0.5 + 0.5 / k, n - 0.5 - 0.5 / k, size, dtype=np.float32)
    pos = np.clip(pos, 0, n - 1, out=pos)
    lo = np.floor(np.clip(pos, 0, n - 1.001)).astype(int)
    pos -= lo
    return lo, pos


def _resize(img, size, dt):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    ra, rs = axis_samples(img.shape[0], size[0])
    ca, cs = axis_samples(img.shape[1], size[1])
    gr, gc = (np.float32(1) - rs), (np.float32(1) - cs)            # float32, as the reference's `1 - cs`
    assert gr.dtype == np.float32 and gc.dtype == np.float32
    p = img.astype(dt)
    cs, gc, rs, gr = (v.astype(dt) for v in (cs, gc, rs, gr))
    t = p[:, ca] * gc[None, :, None] + p[:, ca + 1] * cs[None, :, None]
    out = t[ra] * gr[:, None, None] + t[ra + 1] * rs[:, None, None]
    assert out.dtype == dt
    return out


def resize32(img, size):
    """(H, W, C) uint8 -> (OH, OW, C) float32, every product and sum rounded to float32 on its own."""
    return _resize(img, size, np.float32)


def resize64(img, size):
    return _resize(img, size, np.float64)


def pick(x, layout, order):
    """The (N, Co, H, W) uint8 planes a batch in `layout` hands to the output channels."""
    x = np.asarray(x)
    planes = x.transpose(0, 3, 1, 2) if layout == "nhwc" else x
    return planes if order is None else planes[:, list(order)]


def decode32(x, k, b, layout="nhwc", order=None, size=None):
    """The kernel's arithmetic restated: float32 (N, Co, OH, OW)."""
    k, b = np.asarray(k, np.float32), np.asarray(b, np.float32)
    if size is None:
        r = pick(x, layout, order).astype(np.float32)
    else:
        assert layout == "nhwc"
        r = pick(np.stack([resize32(im, size) for im in x]), "nhwc", order)
    y = r * k[None, :, None, None] + b[None, :, None, None]
    assert y.dtype == np.float32
    return y


def decode64(x, k, b, layout="nhwc", order=None, size=None):
    """(y64, bound): the float64 value of the same expression on the same float32 k, b and sampling weights, and the
    per-element bound of the module docstring."""
    k, b = np.asarray(k, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    if size is None:
        r = pick(x, layout, order).astype(np.float64)
    else:
        assert layout == "nhwc"
        r = pick(np.stack([resize64(im, size) for im in x]), "nhwc", order)
    y = r * k[None, :, None, None] + b[None, :, None, None]
    bound = (7 if size is not None else 1) * U * 255 * np.abs(k)[None, :, None, None] + U * np.abs(y)
    return y, bound


def stem_net(cout=16, seed=5):
    """conv 7x7 / stride 2 / pad 3 (3 -> cout) + batchnorm + relu, maxpool 3x3 / stride 2 / pad 1, conv 1x1 (cout -> 8): the
    smallest net whose plan runs the stem + max-pool kernel (at feed time where W % 4 == 0: `static.prefed`)."""
    from planer_amd.irgen.builder import GraphBuilder
    rng = np.random.default_rng(seed)
    g = GraphBuilder(["x"])
    g.init("K", (rng.standard_normal((cout, 3, 7, 7)) * 0.1).astype(np.float32))
    g.init("s", rng.uniform(0.5, 1.5, (1, cout, 1, 1)).astype(np.float32))
    g.init("t", (rng.standard_normal((1, cout, 1, 1)) * 0.1).astype(np.float32))
    g.init("K2", (rng.standard_normal((8, cout, 1, 1)) * 0.2).astype(np.float32))
    g.op("conv", ["x", "K"], "c", name="stem", group=1, strides=[2, 2], dilations=[1, 1], pads=[3, 3, 3, 3])
    g.op("batchnorm", ["c", "s", "t"], "n", name="bn")
    g.op("relu", "n", "r", name="relu")
    g.op("maxpool", "r", "p", name="pool", w=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2])
    g.op("conv", ["p", "K2"], "y", name="head", group=1, strides=[1, 1], dilations=[1, 1], pads=[0, 0, 0, 0])
    return g.finish(["y"])


def rgba_net(seed=6):
    """conv 3x3 / pad 1 on FOUR input channels + relu: takes neither feed-time route."""
    from planer_amd.irgen.builder import GraphBuilder
    rng = np.random.default_rng(seed)
    g = GraphBuilder(["x"])
    g.init("K", (rng.standard_normal((8, 4, 3, 3)) * 0.1).astype(np.float32))
    g.init("B", rng.standard_normal(8).astype(np.float32))
    g.op("conv", ["x", "K", "B"], "c", name="conv", group=1, strides=[1, 1], dilations=[1, 1], pads=[1, 1, 1, 1])
    g.op("relu", "c", "r", name="relu")
    return g.finish(["r"])


def worst(y, y64, bound):
    """max of |y - y64| / bound (0 / 0 counts as 0)."""
    err = np.abs(np.asarray(y, np.float64) - y64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(q.max()) if q.size else 0.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())

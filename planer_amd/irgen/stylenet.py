"""The image transformation network of fast neural style (Johnson et al. 2016, with instance normalisation after Ulyanov et al.
2016 and the upsample + conv up-steps of Odena et al. 2016) as planer IR with seeded weights: the ONNX model zoo's
fast-neural-style "TransformerNet".

Layout as read_onnx would emit it for a PyTorch export.  Every conv layer is `pad` (mode reflect, k // 2 pixels on each side of H
and W, pads as an int64 init in ONNX order) followed by `conv` with bias and pads 0; every norm is `instancenormalization` with a
per-channel scale and bias (eps 1e-5).

    conv 3 -> 32 k9, IN, relu;  conv 32 -> 64 k3 s2, IN, relu;  conv 64 -> 128 k3 s2, IN, relu
    5 x residual block at 128 channels: conv k3, IN, relu, conv k3, IN, add(block input)
    2 x up-step: upsample nearest x2, conv k3 (128 -> 64, 64 -> 32), IN, relu
    conv 32 -> 3 k9

16 conv layers, 15 norms, 1,679,235 parameters.
"""
import numpy as np

from .builder import GraphBuilder

RES_BLOCKS = 5
PARAMS = 1679235


def params():
    """Parameter count of build() (conv weights and biases, one scale and bias per normalised channel)."""
    def conv(ci, co, k):
        return ci * co * k * k + co
    n = conv(3, 32, 9) + conv(32, 64, 3) + conv(64, 128, 3) + 2 * (32 + 64 + 128)
    n += RES_BLOCKS * 2 * (conv(128, 128, 3) + 2 * 128)
    n += conv(128, 64, 3) + conv(64, 32, 3) + 2 * (64 + 32)
    return n + conv(32, 3, 9)


class _Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.g = GraphBuilder(["x"])
        self._pads = set()

    def conv(self, src, cin, cout, k, stride, tag, gain=2.0):
        rng, g = self.rng, self.g
        p = k // 2
        if p not in self._pads:
            self._pads.add(p)
            g.init("pads%d" % p, np.array([0, 0, p, p, 0, 0, p, p], np.int64))
        g.init(tag + "_w", (rng.standard_normal((cout, cin, k, k)) * np.sqrt(gain / (cin * k * k))).astype(np.float32))
        g.init(tag + "_b", (rng.standard_normal(cout) * 0.1).astype(np.float32))
        g.op("pad", [src, "pads%d" % p], tag + "_p", name=tag + "_pad", mode="reflect")
        return g.op("conv", [tag + "_p", tag + "_w", tag + "_b"], tag + "_c", name=tag + "_conv", group=1, strides=[stride, stride],
                    dilations=[1, 1], pads=[0, 0, 0, 0])

    def norm(self, src, c, tag, relu=True):
        rng, g = self.rng, self.g
        g.init(tag + "_s", rng.uniform(0.5, 1.5, c).astype(np.float32))
        g.init(tag + "_t", (rng.standard_normal(c) * 0.1).astype(np.float32))
        out = g.op("instancenormalization", [src, tag + "_s", tag + "_t"], tag + "_n", name=tag + "_in", epsilon=1e-5)
        return g.op("relu", out, tag + "_r", name=tag + "_relu") if relu else out

    def conv_norm(self, src, cin, cout, k, stride, tag, relu=True):
        return self.norm(self.conv(src, cin, cout, k, stride, tag), cout, tag, relu)


def build(seed=0):
    m = _Gen(seed)
    g = m.g
    y = m.conv_norm("x", 3, 32, 9, 1, "c1")
    y = m.conv_norm(y, 32, 64, 3, 2, "c2")
    y = m.conv_norm(y, 64, 128, 3, 2, "c3")
    for i in range(RES_BLOCKS):
        t = m.conv_norm(y, 128, 128, 3, 1, "r%da" % i)
        t = m.conv_norm(t, 128, 128, 3, 1, "r%db" % i, relu=False)
        y = g.op("add", [t, y], "r%d" % i, name="r%d_add" % i)
    g.init("scales", np.array([1, 1, 2, 2], np.float32))
    for i, (cin, cout) in enumerate(((128, 64), (64, 32))):
        y = g.op("upsample", [y, "scales"], "u%d_up" % i, name="u%d_up" % i, mode="nearest")
        y = m.conv_norm(y, cin, cout, 3, 1, "u%d" % i)
    y = m.conv(y, 32, 3, 9, 1, "out", gain=1.0)
    return g.finish([y])


def make_input(n, seed=1, size=224):
    return np.random.default_rng(seed).standard_normal((n, 3, size, size)).astype(np.float32)

"""The standard U-Net (Ronneberger et al. 2015, in its common padded form with BatchNorm) as planer IR with seeded weights.

Layout as read_onnx would emit it for a PyTorch export: every DoubleConv is conv 3x3 (pad 1, no bias) -> batchnorm (folded
K,B of shape (1,C,1,1), eps 1e-5, io.py:76-91) -> relu, twice; channels 64, 128, 256, 512, 1024 with a 2x2 / stride-2 max
pool before each of the four deeper levels.  Each of the four up-steps is a ConvTranspose2d(k=2, s=2) with bias that halves
the channels, a concat of [skip, up-sampled] along the channels, and a DoubleConv; a 1x1 conv with bias makes the class map.
With 3 input channels and 2 classes that is 31,037,698 parameters (BN as K/B pairs).

up="k3" swaps each up-step's transposed conv for ConvTranspose2d(k=3, s=2, p=1, output_padding=1) without bias, followed by
batchnorm -> relu: phases with unequal tap counts and a fused tail on the transposed conv.
"""
import numpy as np

from .builder import GraphBuilder

WIDTHS = [64, 128, 256, 512, 1024]
PARAMS = 31037698


def params(in_ch=3, classes=2, up="k2"):
    """Parameter count of build(in_ch, classes, up) (BN as K/B pairs)."""
    n, cin = 0, in_ch

    def dconv(ci, co):
        return ci * co * 9 + 2 * co + co * co * 9 + 2 * co
    for c in WIDTHS:
        n += dconv(cin, c)
        cin = c
    for c in WIDTHS[-2::-1]:
        n += cin * c * 4 + c if up == "k2" else cin * c * 9 + 2 * c
        n += dconv(2 * c, c)
        cin = c
    return n + cin * classes + classes


class _Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.g = GraphBuilder(["x"])

    def bn_relu(self, src, c, tag):
        rng, g = self.rng, self.g
        gamma = rng.uniform(0.5, 1.5, c)
        beta = rng.standard_normal(c) * 0.1
        mean = rng.standard_normal(c) * 0.1
        var = rng.uniform(0.5, 1.5, c)
        inv = gamma / np.sqrt(var + 1e-5)
        g.init(tag + "_invK", inv.reshape(1, -1, 1, 1).astype(np.float32))
        g.init(tag + "_invB", (beta - mean * inv).reshape(1, -1, 1, 1).astype(np.float32))
        out = g.op("batchnorm", [src, tag + "_invK", tag + "_invB"], tag + "_b", name=tag + "_bn")
        return g.op("relu", out, tag + "_r", name=tag + "_relu")

    def conv_bn_relu(self, src, cin, cout, tag):
        w = self.rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (cin * 9))
        self.g.init(tag + "_w", w.astype(np.float32))
        self.g.op("conv", [src, tag + "_w"], tag + "_c", name=tag + "_conv", group=1, strides=[1, 1], dilations=[1, 1],
                  pads=[1, 1, 1, 1])
        return self.bn_relu(tag + "_c", cout, tag)

    def double_conv(self, src, cin, cout, tag):
        return self.conv_bn_relu(self.conv_bn_relu(src, cin, cout, tag + "a"), cout, cout, tag + "b")

    def up(self, src, cin, cout, mode, tag):
        rng, g = self.rng, self.g
        k = 2 if mode == "k2" else 3
        w = rng.standard_normal((cin, cout, k, k)) * np.sqrt(1.0 / (cin * k * k / 4.0))
        g.init(tag + "_w", w.astype(np.float32))
        if mode == "k2":
            g.init(tag + "_bias", (rng.standard_normal(cout) * 0.1).astype(np.float32))
            return g.op("convtranspose", [src, tag + "_w", tag + "_bias"], tag + "_t", name=tag + "_convt", strides=[2, 2],
                        dilations=[1, 1], pads=[0, 0, 0, 0], output_padding=[0, 0], group=1)
        g.op("convtranspose", [src, tag + "_w"], tag + "_t", name=tag + "_convt", strides=[2, 2], dilations=[1, 1],
             pads=[1, 1, 1, 1], output_padding=[1, 1], group=1)
        return self.bn_relu(tag + "_t", cout, tag)


def build(seed=0, in_ch=3, classes=2, up="k2"):
    if up not in ("k2", "k3"):
        raise ValueError("up is 'k2' (ConvTranspose2d k=2 s=2 + bias) or 'k3' (k=3 s=2 p=1 output_padding=1 + BN + ReLU)")
    m = _Gen(seed)
    skips, y, cin = [], "x", in_ch
    for i, c in enumerate(WIDTHS):
        if i:
            y = m.g.op("maxpool", y, "pool%d" % i, name="pool%d" % i, w=[2, 2], strides=[2, 2], pads=[0, 0, 0, 0])
        y = m.double_conv(y, cin, c, "d%d" % i)
        skips.append(y)
        cin = c
    for i, c in enumerate(WIDTHS[-2::-1]):
        u = m.up(y, cin, c, up, "u%d" % i)
        cat = m.g.op("concat", [skips[-2 - i], u], "cat%d" % i, name="cat%d" % i, axis=1)
        y = m.double_conv(cat, 2 * c, c, "u%dc" % i)
        cin = c
    m.g.init("head_w", (m.rng.standard_normal((classes, cin, 1, 1)) * np.sqrt(1.0 / cin)).astype(np.float32))
    m.g.init("head_b", (m.rng.standard_normal(classes) * 0.1).astype(np.float32))
    y = m.g.op("conv", [y, "head_w", "head_b"], "logits", name="head", group=1, strides=[1, 1], dilations=[1, 1],
               pads=[0, 0, 0, 0])
    return m.g.finish([y])


def make_input(n, seed=1, size=256, in_ch=3):
    return np.random.default_rng(seed).standard_normal((n, in_ch, size, size)).astype(np.float32)

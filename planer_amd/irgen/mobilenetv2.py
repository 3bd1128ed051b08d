"""MobileNet-v2 (torchvision's, width 1.0) as planer IR with seeded weights.

Layout as read_onnx would emit it for a torchvision export: conv (no bias) -> batchnorm (folded K,B of shape (1,C,1,1),
eps 1e-5, io.py:76-91) -> clip(min=0, max=6) for ReLU6; a 3x3 / stride-2 stem; 17 inverted-residual blocks (1x1 expand,
3x3 depthwise conv with group == C, 1x1 linear projection, residual add where stride 1 keeps the width); a 1x1 conv to
1280 channels; gap, flatten, dense, return.  52 convs (17 depthwise), 52 batchnorms, 35 clips, 10 adds;
3,504,872 parameters (torchvision's count, BN as K/B pairs).
"""
import numpy as np

from .builder import GraphBuilder

# (expansion t, output channels c, repeats n, first stride s): torchvision's inverted_residual_setting
SETTING = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]
PARAMS = 3504872


class _Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.g = GraphBuilder(["x"])

    def conv_bn(self, src, cin, cout, k, s, group, relu6, tag):
        rng, g = self.rng, self.g
        cin_g = cin // group
        w = rng.standard_normal((cout, cin_g, k, k)) * np.sqrt(2.0 / (cin_g * k * k))
        gamma = rng.uniform(0.5, 1.5, cout)
        beta = rng.standard_normal(cout) * 0.1
        mean = rng.standard_normal(cout) * 0.1
        var = rng.uniform(0.5, 1.5, cout)
        inv = gamma / np.sqrt(var + 1e-5)
        g.init(tag + "_w", w.astype(np.float32))
        g.init(tag + "_invK", inv.reshape(1, -1, 1, 1).astype(np.float32))
        g.init(tag + "_invB", (beta - mean * inv).reshape(1, -1, 1, 1).astype(np.float32))
        p = (k - 1) // 2
        g.op("conv", [src, tag + "_w"], tag + "_c", name=tag + "_conv", group=group,
             strides=[s, s], dilations=[1, 1], pads=[p, p, p, p])
        out = g.op("batchnorm", [tag + "_c", tag + "_invK", tag + "_invB"], tag + "_b", name=tag + "_bn")
        if relu6:
            out = g.op("clip", out, tag + "_r", name=tag + "_clip", min=0.0, max=6.0)
        return out

    def block(self, src, cin, cout, stride, t, tag):
        hidden = cin * t
        y = src
        if t != 1:
            y = self.conv_bn(y, cin, hidden, 1, 1, 1, True, tag + "e")
        y = self.conv_bn(y, hidden, hidden, 3, stride, hidden, True, tag + "d")
        y = self.conv_bn(y, hidden, cout, 1, 1, 1, False, tag + "p")
        if stride == 1 and cin == cout:
            y = self.g.op("add", [y, src], tag + "_s", name=tag + "_add")
        return y


def build(seed=0, classes=1000):
    m = _Gen(seed)
    y = m.conv_bn("x", 3, 32, 3, 2, 1, True, "stem")
    cin, bi = 32, 0
    for t, c, n, s in SETTING:
        for i in range(n):
            y = m.block(y, cin, c, s if i == 0 else 1, t, "b%d" % bi)
            cin, bi = c, bi + 1
    y = m.conv_bn(y, cin, 1280, 1, 1, 1, True, "last")
    y = m.g.op("gap", y, "gap", name="gap")
    y = m.g.op("flatten", y, "flat", name="flatten")
    m.g.init("fc_w", (m.rng.standard_normal((classes, 1280)) * 0.03).astype(np.float32))
    m.g.init("fc_b", (m.rng.standard_normal(classes) * 0.1).astype(np.float32))
    y = m.g.op("dense", [y, "fc_w", "fc_b"], "logits", name="fc", shp=[1280, classes])
    return m.g.finish([y])


def make_input(n, seed=1, size=224):
    return np.random.default_rng(seed).standard_normal((n, 3, size, size)).astype(np.float32)

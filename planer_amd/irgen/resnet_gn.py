"""ResNet-18 with group normalisation (Wu & He 2018) as planer IR with seeded weights: torchvision's resnet18 built with
norm_layer = GroupNorm(groups, C) wherever it has BatchNorm.

Layout as read_onnx would emit it for a PyTorch export below opset 18, which has no GroupNormalization operator and writes every
norm as five steps:

    reshape(x, [0, G, -1]) -> instancenormalization(ones(G), zeros(G), eps 1e-5) -> reshape(., [0, C, H, W])
      -> mul(., gamma (C, 1, 1)) -> add(., beta (C, 1, 1))

The first reshape's shape and the instance norm's ones / zeros are one init each per net; the second reshape's shape is a constant
per (C, H, W), so a graph is built for one input size.  conv (no bias) -> norm -> relu; maxpool 3x3 s2 p1; 8 BasicBlocks with
add + relu; three 1x1 s2 downsample conv + norm; gap, flatten, dense, return.  plan.fuse_groupnorm finds the five steps again.

At the defaults (groups 32, width 64) the four stages have 2, 4, 8 and 16 channels per group; width 8 with groups 4 has the same
four in miniature.  20 conv layers, 20 norms, 11,689,512 parameters.
"""
import numpy as np

from .builder import GraphBuilder

STAGES = ((1, 1), (2, 2), (4, 2), (8, 2))        # (width multiple, stride of the first block)


def params(groups=32, width=64, classes=1000):
    """Parameter count of build(groups, width, classes): conv weights, gamma and beta per normalised channel, the classifier.  The
    instance norms' ones / zeros and the reshapes' shapes are not parameters."""
    def conv_norm(ci, co, k):
        return ci * co * k * k + 2 * co
    n, cin = conv_norm(3, width, 7), width
    for mult, stride in STAGES:
        cout = width * mult
        for bi in range(2):
            n += conv_norm(cin, cout, 3) + conv_norm(cout, cout, 3)
            if bi == 0 and (stride != 1 or cin != cout):
                n += conv_norm(cin, cout, 1)
            cin = cout
    return n + cin * classes + classes


class _Gen:
    def __init__(self, seed, groups):
        self.rng = np.random.default_rng(seed)
        self.g = GraphBuilder(["x"])
        self.groups = groups
        self._shapes = set()
        self.g.init("gn_split", np.array([0, groups, -1], np.int64))
        self.g.init("gn_ones", np.ones(groups, np.float32))
        self.g.init("gn_zeros", np.zeros(groups, np.float32))

    def conv_gn(self, src, cin, cout, k, s, p, hw, relu, tag):
        """-> (output key, output map size)"""
        rng, g = self.rng, self.g
        if cout % self.groups:
            raise ValueError("%d groups do not divide the %d channels of %s" % (self.groups, cout, tag))
        hw = (hw + 2 * p - k) // s + 1
        g.init(tag + "_w", (rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32))
        g.init(tag + "_gamma", rng.uniform(0.5, 1.5, (cout, 1, 1)).astype(np.float32))
        g.init(tag + "_beta", (rng.standard_normal((cout, 1, 1)) * 0.1).astype(np.float32))
        merge = "gn_merge_%dx%d" % (cout, hw)
        if merge not in self._shapes:
            self._shapes.add(merge)
            g.init(merge, np.array([0, cout, hw, hw], np.int64))
        y = g.op("conv", [src, tag + "_w"], tag + "_c", name=tag + "_conv", group=1, strides=[s, s], dilations=[1, 1], pads=[p, p, p, p])
        y = g.op("reshape", [y, "gn_split"], tag + "_g", name=tag + "_split")
        y = g.op("instancenormalization", [y, "gn_ones", "gn_zeros"], tag + "_n", name=tag + "_in", epsilon=1e-5)
        y = g.op("reshape", [y, merge], tag + "_m", name=tag + "_merge")
        y = g.op("mul", [y, tag + "_gamma"], tag + "_k", name=tag + "_mul")
        y = g.op("add", [y, tag + "_beta"], tag + "_b", name=tag + "_shift")
        if relu:
            y = g.op("relu", y, tag + "_r", name=tag + "_relu")
        return y, hw

    def block(self, src, cin, cout, stride, hw, tag):
        y, out_hw = self.conv_gn(src, cin, cout, 3, stride, 1, hw, True, tag + "a")
        y, _ = self.conv_gn(y, cout, cout, 3, 1, 1, out_hw, False, tag + "b")
        if stride != 1 or cin != cout:
            src, _ = self.conv_gn(src, cin, cout, 1, stride, 0, hw, False, tag + "d")
        s = self.g.op("add", [y, src], tag + "_s", name=tag + "_add")
        return self.g.op("relu", s, tag + "_o", name=tag + "_out"), out_hw


def build(seed=0, groups=32, width=64, classes=1000, size=224):
    m = _Gen(seed, groups)
    y, hw = m.conv_gn("x", 3, width, 7, 2, 3, size, True, "stem")
    y = m.g.op("maxpool", y, "pool", name="maxpool", w=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2])
    hw = (hw + 2 - 3) // 2 + 1
    cin = width
    for li, (mult, stride) in enumerate(STAGES, 1):
        for bi in range(2):
            y, hw = m.block(y, cin, width * mult, stride if bi == 0 else 1, hw, "l%d%d" % (li, bi))
            cin = width * mult
    y = m.g.op("gap", y, "gap", name="gap")
    y = m.g.op("flatten", y, "flat", name="flatten")
    m.g.init("fc_w", (m.rng.standard_normal((classes, cin)) * 0.03).astype(np.float32))
    m.g.init("fc_b", (m.rng.standard_normal(classes) * 0.1).astype(np.float32))
    y = m.g.op("dense", [y, "fc_w", "fc_b"], "logits", name="fc", shp=[cin, classes])
    return m.g.finish([y])


def make_input(n, seed=1, size=224):
    return np.random.default_rng(seed).standard_normal((n, 3, size, size)).astype(np.float32)

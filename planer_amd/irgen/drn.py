"""A dilated ResNet-18 (Yu, Koltun & Funkhouser 2017, "Dilated Residual Networks"; the backbone form of DeepLab) as planer IR
with seeded weights, written like irgen/resnet18.py.

Stem, max-pool, layer1 and layer2 are ResNet-18's.  layer3 and layer4 keep the 1/8 resolution of layer2 and dilate instead
of striding:

    layer3.0   conv a 3x3 s1 d1 p1; conv b 3x3 d2 p2; 1x1 s1 projection
    layer3.1   a, b 3x3 d2 p2
    layer4.0   a 3x3 d2 p2; b 3x3 d4 p4; 1x1 s1 projection
    layer4.1   a, b 3x3 d4 p4

Seven dilated convs.  The head is a 1x1 conv 512 -> classes with bias and a bilinear upsample by 8 back to the input size: the
output is (N, classes, size, size).  At 224 x 224 the seven dilated convs are 18 of the net's 21 GFLOP per image.
"""
import numpy as np

from .resnet18 import _Gen as _ResNetGen


class _Gen(_ResNetGen):
    def conv_bn(self, src, cin, cout, k, s, p, relu, tag, d=1):
        out = super().conv_bn(src, cin, cout, k, s, p, relu, tag)
        if d != 1:
            conv = next(e for e in self.g.layers if e[0] == tag + "_conv")
            conv[2]["dilations"] = [d, d]
        return out

    def dblock(self, src, cin, cout, da, db, tag):
        """BasicBlock at stride 1: conv a dilated by `da`, conv b by `db`, pads equal to the dilation."""
        y = self.conv_bn(src, cin, cout, 3, 1, da, True, tag + "a", d=da)
        y = self.conv_bn(y, cout, cout, 3, 1, db, False, tag + "b", d=db)
        if cin != cout:
            src = self.conv_bn(src, cin, cout, 1, 1, 0, False, tag + "d")
        s = self.g.op("add", [y, src], tag + "_s", name=tag + "_add")
        return self.g.op("relu", s, tag + "_o", name=tag + "_out")


def build(seed=0, classes=21):
    m = _Gen(seed)
    y = m.conv_bn("x", 3, 64, 7, 2, 3, True, "stem")
    y = m.g.op("maxpool", y, "pool", name="maxpool", w=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2])
    cin = 64
    for li, (cout, stride) in enumerate([(64, 1), (128, 2)], 1):
        for bi in range(2):
            y = m.block(y, cin, cout, stride if bi == 0 else 1, "l%d%d" % (li, bi))
            cin = cout
    y = m.dblock(y, 128, 256, 1, 2, "l30")
    y = m.dblock(y, 256, 256, 2, 2, "l31")
    y = m.dblock(y, 256, 512, 2, 4, "l40")
    y = m.dblock(y, 512, 512, 4, 4, "l41")
    m.g.init("head_w", (m.rng.standard_normal((classes, 512, 1, 1)) * 0.03).astype(np.float32))
    m.g.init("head_b", (m.rng.standard_normal(classes) * 0.1).astype(np.float32))
    y = m.g.op("conv", [y, "head_w", "head_b"], "head", name="head_conv", group=1, strides=[1, 1], dilations=[1, 1],
               pads=[0, 0, 0, 0])
    m.g.init("scales", np.array([1, 1, 8, 8], np.float32))
    y = m.g.op("upsample", [y, "scales"], "up", name="up8", mode="linear")
    return m.g.finish([y])


def make_input(n, seed=1, size=224):
    return np.random.default_rng(seed).standard_normal((n, 3, size, size)).astype(np.float32)

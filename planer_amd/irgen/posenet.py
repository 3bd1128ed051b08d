"""The "simple baselines" pose net (Xiao, Wu & Wei 2018, "Simple Baselines for Human Pose Estimation and Tracking") on the
ResNet-18 of irgen/resnet18.py, as planer IR with seeded weights, written like irgen/fpn.py.

    trunk         ResNet-18 without its pool and fc: 512 channels at 1/32 scale
    deconv        three times ConvTranspose2d(256, k=4, s=2, p=1) without bias + BN + ReLU: 1/16, 1/8, 1/4 scale
    output        1x1 conv 256 -> joints with bias: (N, joints, H / 4, W / 4) heat maps, one plane per joint

256 x 192 in, 64 x 48 heat maps out (17 COCO joints), stride 4: `net.keypoint_output(stride=STRIDE)` hands back input pixels.
"""
import numpy as np

from .resnet18 import _Gen as _ResNetGen

DECONV, JOINTS, STRIDE, SIZE = 256, 17, 4, (256, 192)


class _Gen(_ResNetGen):
    def deconv_bn_relu(self, src, cin, cout, tag):
        rng, g = self.rng, self.g
        g.init(tag + "_w", (rng.standard_normal((cin, cout, 4, 4)) * np.sqrt(2.0 / (cin * 4))).astype(np.float32))
        g.op("convtranspose", [src, tag + "_w"], tag + "_t", name=tag + "_convt", strides=[2, 2], dilations=[1, 1], pads=[1, 1, 1, 1],
             output_padding=[0, 0], group=1)
        gamma, beta = rng.uniform(0.5, 1.5, cout), rng.standard_normal(cout) * 0.1
        mean, var = rng.standard_normal(cout) * 0.1, rng.uniform(0.5, 1.5, cout)
        inv = gamma / np.sqrt(var + 1e-5)
        g.init(tag + "_invK", inv.reshape(1, -1, 1, 1).astype(np.float32))
        g.init(tag + "_invB", (beta - mean * inv).reshape(1, -1, 1, 1).astype(np.float32))
        out = g.op("batchnorm", [tag + "_t", tag + "_invK", tag + "_invB"], tag + "_b", name=tag + "_bn")
        return g.op("relu", out, tag + "_r", name=tag + "_relu")


def build(seed=0, joints=JOINTS):
    m = _Gen(seed)
    y = m.conv_bn("x", 3, 64, 7, 2, 3, True, "stem")
    y = m.g.op("maxpool", y, "pool", name="maxpool", w=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2])
    cin = 64
    for li, (cout, stride) in enumerate([(64, 1), (128, 2), (256, 2), (512, 2)], 1):
        for bi in range(2):
            y = m.block(y, cin, cout, stride if bi == 0 else 1, "l%d%d" % (li, bi))
            cin = cout
    for i in range(3):
        y = m.deconv_bn_relu(y, cin, DECONV, "up%d" % i)
        cin = DECONV
    m.g.init("heat_w", (m.rng.standard_normal((joints, cin, 1, 1)) * np.sqrt(1.0 / cin)).astype(np.float32))
    m.g.init("heat_bias", (m.rng.standard_normal(joints) * 0.1).astype(np.float32))
    y = m.g.op("conv", [y, "heat_w", "heat_bias"], "heat", name="heat_conv", group=1, strides=[1, 1], dilations=[1, 1], pads=[0, 0, 0, 0])
    return m.g.finish([y])


def make_input(n, seed=1, size=SIZE):
    return np.random.default_rng(seed).standard_normal((n, 3) + tuple(size)).astype(np.float32)

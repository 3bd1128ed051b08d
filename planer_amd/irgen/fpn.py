"""A Panoptic-FPN semantic-segmentation net (Kirillov, Girshick, He & Dollar 2019, "Panoptic Feature Pyramid Networks", the
semantic branch; Lin et al. 2017 for the pyramid) on the ResNet-18 of irgen/resnet18.py, as planer IR with seeded weights,
written like irgen/drn.py.  GroupNorm is left out: planer has no such kind.

    C2 .. C5      the outputs of ResNet-18's layer1 .. layer4: 64 / 128 / 256 / 512 channels at 1/4 .. 1/32 scale
    laterals      1x1 conv with bias to 128 channels on every C_l
    top-down      P5 = lateral5;  P_l = lateral_l + up2(P_{l+1}), bilinear
    smoothing     3x3 conv 128 -> 128 with bias on every P_l
    head          per level (3x3 conv 128 -> 64 + ReLU + bilinear x2) until 1/4 scale: 3, 2, 1 times for P5, P4, P3;
                  P2 gets the conv + ReLU alone
    sum           the four 64-channel maps at 1/4 scale
    output        1x1 conv 64 -> classes with bias, bilinear x4 back to the input size: (N, classes, size, size)

Nine bilinear x2 steps inside the net and one x4 at its end.  `via="upsample"` writes them as `upsample` steps;
`via="resize"` as `resize` steps that carry scales and an empty roi, the way an ONNX export of F.interpolate arrives.
"""
import numpy as np

from .resnet18 import _Gen as _ResNetGen

PYRAMID, HEAD = 128, 64


class _Gen(_ResNetGen):
    def __init__(self, seed, via):
        super().__init__(seed)
        if via not in ("upsample", "resize"):
            raise ValueError("via is 'upsample' or 'resize', got %r" % (via,))
        self.via = via
        self.g.init("scales2", np.array([1, 1, 2, 2], np.float32))
        self.g.init("scales4", np.array([1, 1, 4, 4], np.float32))
        if via == "resize":
            self.g.init("roi", np.zeros(0, np.float32))

    def conv_b(self, src, cin, cout, k, tag, relu=False):
        rng, g = self.rng, self.g
        g.init(tag + "_w", (rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32))
        g.init(tag + "_bias", (rng.standard_normal(cout) * 0.1).astype(np.float32))
        out = g.op("conv", [src, tag + "_w", tag + "_bias"], tag + "_c", name=tag + "_conv", group=1, strides=[1, 1],
                   dilations=[1, 1], pads=[k // 2] * 4)
        return g.op("relu", out, tag + "_r", name=tag + "_relu") if relu else out

    def up(self, src, f, tag):
        if self.via == "upsample":
            return self.g.op("upsample", [src, "scales%d" % f], tag, name=tag + "_up", mode="linear")
        return self.g.op("resize", [src, "roi", "scales%d" % f], tag, name=tag + "_up", mode="linear",
                         coordinate_transformation_mode="half_pixel", nearest_mode="round_prefer_floor")


def build(seed=0, classes=21, via="upsample"):
    m = _Gen(seed, via)
    y = m.conv_bn("x", 3, 64, 7, 2, 3, True, "stem")
    y = m.g.op("maxpool", y, "pool", name="maxpool", w=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2])
    cin, feats = 64, {}
    for li, (cout, stride) in enumerate([(64, 1), (128, 2), (256, 2), (512, 2)], 1):
        for bi in range(2):
            y = m.block(y, cin, cout, stride if bi == 0 else 1, "l%d%d" % (li, bi))
            cin = cout
        feats[li + 1] = (y, cout)                                  # C2 .. C5
    # top-down path
    p = {5: m.conv_b(feats[5][0], feats[5][1], PYRAMID, 1, "lat5")}
    for l in (4, 3, 2):
        lat = m.conv_b(feats[l][0], feats[l][1], PYRAMID, 1, "lat%d" % l)
        u = m.up(p[l + 1], 2, "td%d" % l)
        p[l] = m.g.op("add", [lat, u], "p%d" % l, name="p%d_add" % l)
    # smoothing and the per-level heads, finest first; each map joins the sum as soon as it exists
    total = None
    for l in (2, 3, 4, 5):
        y = m.conv_b(p[l], PYRAMID, PYRAMID, 3, "smooth%d" % l)
        cin = PYRAMID
        for r in range(max(l - 2, 1)):
            y = m.conv_b(y, cin, HEAD, 3, "head%d_%d" % (l, r), relu=True)
            cin = HEAD
            if l > 2:
                y = m.up(y, 2, "head%d_%d_u" % (l, r))
        total = y if total is None else m.g.op("add", [total, y], "sum%d" % l, name="sum%d_add" % l)
    y = total
    y = m.conv_b(y, HEAD, classes, 1, "logits")
    y = m.up(y, 4, "out")
    return m.g.finish([y])


def make_input(n, seed=1, size=224):
    return np.random.default_rng(seed).standard_normal((n, 3, size, size)).astype(np.float32)

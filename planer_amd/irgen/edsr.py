"""EDSR-baseline (Lim, Son, Kim, Nah & Lee 2017, "Enhanced Deep Residual Networks for Single Image Super-Resolution") as planer IR
with seeded weights, written from the paper's description like irgen/fpn.py.  The mean shift around the net is left out.

    head          3x3 conv 3 -> 64 with bias
    trunk         16 residual blocks (3x3 conv + ReLU + 3x3 conv, + the block's input; no BatchNorm, residual scale 1),
                  a 3x3 conv, + the head's output (the long skip)
    upsampler     sub-pixel convolutions (Shi et al. 2016): scale 2 is one (3x3 conv 64 -> 256, pixel shuffle 2), scale 4 two of
                  them, scale 3 one (3x3 conv 64 -> 576, pixel shuffle 3)
    tail          3x3 conv 64 -> 3

Every pixel shuffle is written the way torch.onnx exports nn.PixelShuffle -- reshape to (N, C, r, r, H, W), transpose by
[0, 1, 4, 2, 5, 3], reshape to (N, C, H r, W r) -- because planer has no depth-to-space kind; plan.fuse_pixel_shuffle finds the
three steps again.  The reshapes carry their shapes as constants with 0 for the batch axis, so a graph is built for one input
`size` and any batch.

    tail="shuffle"      the ESPCN ending instead of upsampler + tail: a 3x3 conv 64 -> 3 scale^2 and ONE pixel shuffle by `scale`
                        that ends the program
    unshuffle_in=True   a Real-ESRGAN-x2-style front: pixel unshuffle 2 of the image (3 -> 12 channels at half the size) ahead of
                        the head conv, so the result is (N, 3, size / 2 * scale, size / 2 * scale)
"""
import numpy as np

from .builder import GraphBuilder

CONV = dict(group=1, strides=[1, 1], dilations=[1, 1], pads=[1, 1, 1, 1])


class _Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.g = GraphBuilder(["x"])

    def conv(self, src, cin, cout, tag, gain=1.0):
        rng, g = self.rng, self.g
        g.init(tag + "_w", (rng.standard_normal((cout, cin, 3, 3)) * (gain * np.sqrt(2.0 / (cin * 9)))).astype(np.float32))
        g.init(tag + "_bias", (rng.standard_normal(cout) * 0.05).astype(np.float32))
        return g.op("conv", [src, tag + "_w", tag + "_bias"], tag + "_c", name=tag + "_conv", **CONV)

    def _trio(self, src, mid, axis, out, tag):
        g = self.g
        g.init(tag + "_s6", np.array(mid, np.int64))
        g.init(tag + "_s4", np.array(out, np.int64))
        y = g.op("reshape", [src, tag + "_s6"], tag + "_6", name=tag + "_split")
        y = g.op("transpose", [y], tag + "_t", name=tag + "_perm", axis=list(axis))
        return g.op("reshape", [y, tag + "_s4"], tag, name=tag + "_merge")

    def shuffle(self, src, c, h, w, r, tag):
        """(N, c r^2, h, w) -> (N, c, h r, w r), CRD order (nn.PixelShuffle)."""
        return self._trio(src, [0, c, r, r, h, w], [0, 1, 4, 2, 5, 3], [0, c, h * r, w * r], tag)

    def unshuffle(self, src, c, h, w, r, tag):
        """(N, c, h, w) -> (N, c r^2, h / r, w / r), CRD order (nn.PixelUnshuffle)."""
        return self._trio(src, [0, c, h // r, r, w // r, r], [0, 1, 3, 5, 2, 4], [0, c * r * r, h // r, w // r], tag)


def build(seed=0, scale=4, size=128, blocks=16, feats=64, tail="conv", unshuffle_in=False):
    if scale not in (2, 3, 4):
        raise ValueError("scale is 2, 3 or 4, got %r" % (scale,))
    if tail not in ("conv", "shuffle"):
        raise ValueError("tail is 'conv' or 'shuffle', got %r" % (tail,))
    m = _Gen(seed)
    y, cin, s = "x", 3, size
    if unshuffle_in:
        if size % 2:
            raise ValueError("unshuffle_in needs an even size, got %d" % size)
        y, cin, s = m.unshuffle(y, 3, size, size, 2, "front"), 12, size // 2
    head = y = m.conv(y, cin, feats, "head")
    for b in range(blocks):
        t = m.conv(y, feats, feats, "b%d_1" % b)
        t = m.g.op("relu", t, "b%d_r" % b, name="b%d_relu" % b)
        t = m.conv(t, feats, feats, "b%d_2" % b, gain=0.25)
        y = m.g.op("add", [t, y], "b%d" % b, name="b%d_add" % b)
    y = m.conv(y, feats, feats, "trunk", gain=0.25)
    y = m.g.op("add", [y, head], "skip", name="skip_add")
    if tail == "shuffle":
        y = m.conv(y, feats, 3 * scale * scale, "sub")
        y = m.shuffle(y, 3, s, s, scale, "out")
        return m.g.finish([y])
    for i, r in enumerate([2, 2] if scale == 4 else [scale]):
        y = m.conv(y, feats, feats * r * r, "up%d" % i)
        y = m.shuffle(y, feats, s, s, r, "up%d_ps" % i)
        s *= r
    y = m.conv(y, feats, 3, "tail")
    return m.g.finish([y])


def make_input(n, seed=1, size=128):
    return np.random.default_rng(seed).random((n, 3, size, size), dtype=np.float32)

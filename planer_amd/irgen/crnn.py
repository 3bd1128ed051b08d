"""CRNN (Shi, Bai & Yao 2015, "An End-to-End Trainable Neural Network for Image-based Sequence Recognition"), the line
recogniser of the OCR demos, as planer IR with seeded weights, laid out the way read_onnx would emit a PyTorch export.

    trunk      VGG-style 3x3 conv + BN + ReLU: 64, 128, 256, 256, 512, 512, 512; max-pools 2x2 behind the first two and
               (2, 1) -- height only -- behind the 4th, 6th and 7th conv while the map is higher than one row:
               (N, channels, 32, W) -> (N, 512, 1, W / 4)
    recurrent  squeeze -> (N, 512, T); transpose -> (T, N, 512); bidirectional lstm (hidden) -> (T, 2, N, hidden), transpose
               + reshape -> (T, N, 2 hidden); matmul + add -> (T, N, hidden); a second bidirectional lstm; matmul + add ->
               (T, N, classes): `net.text_output("tnc")`
    otherwise  a 1x1 conv 512 -> classes on the trunk: (N, classes, 1, W / 4), `net.text_output("nchw")`

An lstm step takes all seven operands as inits: W, R, B and, as zeros, sequence_lens, initial_h and initial_c.  The initial
states are (2, N, hidden), so a recurrent graph is built for one batch size, `batch`.
"""
import numpy as np

from .resnet18 import _Gen as _ResNetGen

TRUNK = (64, 128, 256, 256, 512, 512, 512)
SIZE = (32, 320)


class _Gen(_ResNetGen):
    def pool(self, src, tag, h, w):
        return self.g.op("maxpool", src, tag, name=tag, w=[h, w], pads=[0, 0, 0, 0], strides=[h, w])

    def linear(self, src, cin, cout, tag):
        rng, g = self.rng, self.g
        g.init(tag + "_w", (rng.standard_normal((cin, cout)) * np.sqrt(1.0 / cin)).astype(np.float32))
        g.init(tag + "_b", (rng.standard_normal(cout) * 0.1).astype(np.float32))
        y = g.op("matmul", [src, tag + "_w"], tag + "_m", name=tag + "_matmul")
        return g.op("add", [y, tag + "_b"], tag, name=tag + "_add")

    def bilstm(self, src, cin, hidden, batch, tag):
        """(T, N, cin) -> (T, N, 2 hidden)"""
        rng, g = self.rng, self.g
        g.init(tag + "_W", (rng.standard_normal((2, 4 * hidden, cin)) * np.sqrt(1.0 / cin)).astype(np.float32))
        g.init(tag + "_R", (rng.standard_normal((2, 4 * hidden, hidden)) * np.sqrt(1.0 / hidden)).astype(np.float32))
        g.init(tag + "_B", (rng.standard_normal((2, 8 * hidden)) * 0.1).astype(np.float32))
        g.init(tag + "_lens", np.zeros(batch, np.int64))
        g.init(tag + "_h0", np.zeros((2, batch, hidden), np.float32))
        g.init(tag + "_c0", np.zeros((2, batch, hidden), np.float32))
        g.op("lstm", [src] + [tag + s for s in ("_W", "_R", "_B", "_lens", "_h0", "_c0")], [tag + "_Y", tag + "_Yh", tag + "_Yc"],
             name=tag, hidden_size=hidden, direction="bidirectional")
        y = g.op("transpose", [tag + "_Y"], tag + "_t", name=tag + "_perm", axis=[0, 2, 1, 3])
        g.init(tag + "_shape", np.array([0, 0, 2 * hidden], np.int64))
        return g.op("reshape", [y, tag + "_shape"], tag + "_o", name=tag + "_merge")


def build(seed=0, classes=37, height=32, hidden=256, channels=1, recurrent=True, batch=1):
    if height < 4 or height & (height - 1):
        raise ValueError("crnn: height is a power of two, 4 at least, got %r" % (height,))
    m = _Gen(seed)
    y, cin, h = "x", channels, height
    for i, cout in enumerate(TRUNK):
        y = m.conv_bn(y, cin, cout, 3, 1, 1, True, "c%d" % i)
        cin = cout
        if i in (0, 1) and h > 1:
            y, h = m.pool(y, "p%d" % i, 2, 2), h // 2
        elif i in (3, 5, 6) and h > 1:
            y, h = m.pool(y, "p%d" % i, 2, 1), h // 2
    while h > 1:
        y, h = m.pool(y, "q%d" % h, 2, 1), h // 2
    if not recurrent:
        m.g.init("out_w", (m.rng.standard_normal((classes, cin, 1, 1)) * np.sqrt(1.0 / cin)).astype(np.float32))
        m.g.init("out_bias", (m.rng.standard_normal(classes) * 0.1).astype(np.float32))
        y = m.g.op("conv", [y, "out_w", "out_bias"], "logits", name="out_conv", group=1, strides=[1, 1], dilations=[1, 1], pads=[0, 0, 0, 0])
        return m.g.finish([y])
    y = m.g.op("squeeze", y, "seq_nct", name="squeeze", axes=[2])
    y = m.g.op("transpose", [y], "seq", name="to_tnc", axis=[2, 0, 1])
    y = m.bilstm(y, cin, hidden, batch, "lstm0")
    y = m.linear(y, 2 * hidden, hidden, "fc0")
    y = m.bilstm(y, hidden, hidden, batch, "lstm1")
    y = m.linear(y, 2 * hidden, classes, "logits")
    return m.g.finish([y])


def make_input(n, seed=1, size=SIZE, channels=1):
    return np.random.default_rng(seed).standard_normal((n, channels) + tuple(size)).astype(np.float32)

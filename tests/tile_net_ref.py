"""numpy mirrors of Net.tiled's two kernels (pl_tile_windows_*_nchw_f32, pl_tile_blend_*) and `tiled_ref`, the
whole tiled run built from them.

`geometry` restates util.tile's host arithmetic (util.py:300-316 of the reference).  `cut_ref` is the window stack: the image
(resampled with util.resize's roundings where the working size differs: tests/image_input_ref.py), cut, NCHW.  `blend_ref` is the
reference's blend loop (util.py:317-346) transcribed with its dtypes -- float32 `buf`, uint16 `weights` and `count`, the first
window assigned, the others added, one `numpy.divide(..., casting="unsafe")` -- on NCHW window results.  Both are bit-equal to
what the reference's own util.tile did on the geometries of tests/golden/tile_net.npz (tests/test_tile_net.py).

CASES are the geometries the tests and the fixture share: name -> (image H, W), tile arguments, k (output pixels per working
pixel)."""
import itertools
import math

import numpy as np

from tests import image_input_ref as RI
from tests import image_output_ref as RO

CASES = {
    "a": dict(size=(37, 45), tile=dict(window=16, margin=4), k=1),               # 3 x 4 grid, two-way overlaps
    "b": dict(size=(37, 45), tile=dict(window=16, margin=10), k=1),              # rows 0 5 10 15 21: four windows over a pixel per axis
    "c": dict(size=(37, 45), tile=dict(window=16, margin=0), k=1),               # ramp 0
    "d": dict(size=(12, 14), tile=dict(window=16, glob=8), k=1),                 # one window, the image grown to 16 x 16
    "e": dict(size=(37, 45), tile=dict(window=16, sample=(50, 61)), k=1),        # resampled both ways
    "f": dict(size=(37, 45), tile=dict(window=16, margin=4), k=2),               # window results 32 x 32
    "g": dict(size=(37, 45), tile=dict(window=16, margin=5), k=0.5),             # odd origins truncate
}


def canonical(a):
    """The bits of float32 `a` with every NaN as one pattern: which NaN an operation returns (sign, payload) is the one thing
    IEEE 754 leaves open, and an x86 host and the GPU differ there (inf - inf: 0xFFC00000 and 0x7FC00000)."""
    a = np.ascontiguousarray(a, np.float32)
    bits = a.view(np.uint32).copy()
    bits[np.isnan(a)] = 0x7FC00000
    return bits


def make_slice(l, w, mar):
    r = np.linspace(0, l - w, math.ceil((l - mar) / (w - mar)))
    return [slice(i, i + w) for i in r.astype(int).tolist()]


class Geometry:
    """util.tile's host arithmetic (util.py:300-316): working size, window extent, margin in pixels, the window grid."""

    def __init__(self, h, w, sample=1, glob=1, window=1024, margin=0.1):
        self.src = [h, w]
        ssz = list(sample) if isinstance(sample, tuple) else [int(h * sample), int(w * sample)]
        wsh = wsw = window
        if wsh > ssz[0]:
            wsh = ssz[0] = math.ceil(ssz[0] / glob) * glob
        if wsw > ssz[1]:
            wsw = ssz[1] = math.ceil(ssz[1] / glob) * glob
        self.work, self.win = ssz, (wsh, wsw)
        self.margin = int(window * margin) if isinstance(margin, float) else margin
        self.rows, self.cols = make_slice(ssz[0], wsh, self.margin), make_slice(ssz[1], wsw, self.margin)
        self.windows = list(itertools.product(self.rows, self.cols))
        self.resampled = ssz != [h, w]

    def scaled(self, k):
        """(R0, C0, ramp, (OH, OW)) of the blend for scale k (util.py:321-329)."""
        r0 = [int(r.start * k) for r, _ in self.windows]
        c0 = [int(c.start * k) for _, c in self.windows]
        return r0, c0, int(self.margin * k), (int(self.work[0] * k), int(self.work[1] * k))


def resize32(img, size):
    """util.resize on an (H, W, C) image of any dtype in float32 with the reference's roundings (RI.resize32 without its uint8
    restriction)."""
    img = np.asarray(img)
    ra, rs = RI.axis_samples(img.shape[0], size[0])
    ca, cs = RI.axis_samples(img.shape[1], size[1])
    gr, gc = np.float32(1) - rs, np.float32(1) - cs
    p = img.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = p[:, ca] * gc[None, :, None] + p[:, ca + 1] * cs[None, :, None]
        out = t[ra] * gr[:, None, None] + t[ra + 1] * rs[:, None, None]
    assert out.dtype == np.float32
    return out


def cut_ref(image, windows, k=None, b=None, order=None, work=None, slots=None):
    """(H, W[, C]) uint8 or float32 -> float32 (slots, Co, h, w): the working image (resampled where `work` differs), for uint8
    fl(fl(r k[c]) + b[c]) of source channel order[c], cut at `windows`; slots past the last window repeat it."""
    image = np.asarray(image)
    img = image[:, :, None] if image.ndim == 2 else image
    work = tuple(img.shape[:2]) if work is None else tuple(work)
    r = resize32(img, work) if work != tuple(img.shape[:2]) else img.astype(np.float32)
    if image.dtype == np.uint8:
        k, b = np.asarray(k, np.float32), np.asarray(b, np.float32)
        r = r if order is None else r[:, :, list(order)]
        r = r * k[None, None, :] + b[None, None, :]
        assert r.dtype == np.float32
    stack = [r[rs, cs].transpose(2, 0, 1) for rs, cs in windows]
    stack += [stack[-1]] * ((slots or len(stack)) - len(stack))
    return np.ascontiguousarray(np.stack(stack))


def blend_ref(outs, windows, k, margin, work):
    """float32 (n, Co, oh, ow) window results -> float32 (OH, OW, Co): util.py:317-346 with its dtypes."""
    outs = np.asarray(outs)
    assert outs.dtype == np.float32 and outs.ndim == 4 and len(outs) == len(windows)
    rsts = [np.ascontiguousarray(o.transpose(1, 2, 0)) for o in outs]          # what f returns: (oh, ow, Co)
    rst = rsts[0]
    if len(windows) == 1:
        return rst

    def sk(ss):
        return slice(int(ss[0].start * k), int(ss[0].stop * k)), slice(int(ss[1].start * k), int(ss[1].stop * k))
    outshp = (int(work[0] * k), int(work[1] * k)) + rst.shape[2:]
    weights = np.zeros(rst.shape[:2], dtype="uint16")[:, :, None]
    weights += int(margin * k) + 1
    for i in range(int(margin * k), 0, -1):
        weights[i - 1, :] = weights[-i, :] = i
        weights[:, i - 1] = weights[:, -i] = i
    buf = np.zeros(outshp, dtype=np.float32)
    count = np.zeros(outshp[:2], dtype="uint16")[:, :, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        buf[sk(windows[0])] = rst * weights
        count[sk(windows[0])] += weights
        for i in range(1, len(windows)):
            buf[sk(windows[i])] += rsts[i] * weights
            count[sk(windows[i])] += weights
        np.divide(buf, count, out=buf, casting="unsafe")
    return buf


def weights_formula(oh, ow, ramp):
    """min(distance to the nearest edge, ramp) + 1: what the blend kernel computes per pixel; equal to the loop of `blend_ref`."""
    r, c = np.arange(oh)[:, None], np.arange(ow)[None, :]
    return np.minimum(np.minimum(np.minimum(r, oh - 1 - r), np.minimum(c, ow - 1 - c)), ramp) + 1


def encode_ref(y, spec):
    """The blended float32 (OH, OW, Co) in an output form: ("float",), ("labels", threshold) or
    ("image", k, b, layout, order, trunc)."""
    if spec[0] == "float":
        return y
    planes = np.ascontiguousarray(y.transpose(2, 0, 1))[None]
    if spec[0] == "labels":
        return RO.labels(planes, spec[1])[0]
    _, k, b, layout, order, trunc = spec
    return RO.encode32(planes, k, b, layout, order, trunc)[0]


def tiled_ref(net_fn, image, k=None, b=None, order=None, out=("float",), progress=None, **tile):
    """Net.tiled's result from the mirrors: net_fn maps the float32 (n, Co, h, w) window stack to the (n, Co', oh, ow) results."""
    image = np.asarray(image)
    geo = Geometry(image.shape[0], image.shape[1], **tile)
    outs = np.asarray(net_fn(cut_ref(image, geo.windows, k, b, order, geo.work)), np.float32)
    scale = outs.shape[2] / geo.win[0]
    n = len(geo.windows)
    if progress is not None and n > 1:
        for i in range(n):
            progress(i + 1, n)
    y = blend_ref(outs, geo.windows, scale, geo.margin, geo.work)
    if geo.resampled:
        assert out[0] == "float"
        y = resize32(y, (int(image.shape[0] * scale), int(image.shape[1] * scale)))
    return encode_ref(y, out)


# ---- the exact net of the end-to-end tests ------------------------------------------------------------------------------------
def exact_net(cin, cout, k=1, seed=3):
    """conv 3x3 / pad 1 (cin -> 6) + relu, [nearest x2 | max-pool 2x2], conv 3x3 / pad 1 (6 -> cout): small-integer filters and
    biases, so with integer inputs every product and partial sum is an exact float32 whatever the summation order (the trick
    of tests/test_gpu_conv_exact.py).  -> (graph, blob, numpy function on NCHW float32 in float64 arithmetic)."""
    from planer_amd.irgen.builder import GraphBuilder
    rng = np.random.default_rng(seed)
    K1 = rng.integers(-2, 3, (6, cin, 3, 3)).astype(np.float32)
    B1 = rng.integers(-3, 4, 6).astype(np.float32)
    K2 = rng.integers(-2, 3, (cout, 6, 3, 3)).astype(np.float32)
    B2 = rng.integers(-3, 4, cout).astype(np.float32)
    conv = dict(group=1, strides=[1, 1], dilations=[1, 1], pads=[1, 1, 1, 1])
    g = GraphBuilder(["x"])
    for name, a in (("K1", K1), ("B1", B1), ("K2", K2), ("B2", B2)):
        g.init(name, a)
    g.op("conv", ["x", "K1", "B1"], "c1", name="conv1", **conv)
    y = g.op("relu", "c1", "r1", name="relu1")
    if k == 2:
        g.init("scales", np.array([1, 1, 2, 2], np.float32))
        y = g.op("upsample", [y, "scales"], "up", name="up", mode="nearest")
    elif k == 0.5:
        y = g.op("maxpool", y, "pool", name="pool", w=[2, 2], strides=[2, 2], pads=[0, 0, 0, 0])
    g.op("conv", [y, "K2", "B2"], "y", name="conv2", **conv)
    graph, blob = g.finish(["y"])

    def fn(x):
        from oracle import planer_np as onp
        t = np.maximum(onp.conv2d(np.asarray(x, np.float64), K1.astype(np.float64), B1.astype(np.float64), pads=(1, 1, 1, 1)), 0)
        if k == 2:
            t = t.repeat(2, axis=2).repeat(2, axis=3)
        elif k == 0.5:
            n, c, h, w = t.shape
            t = t[:, :, :h // 2 * 2, :w // 2 * 2].reshape(n, c, h // 2, 2, w // 2, 2).max(axis=(3, 5))
        y = onp.conv2d(np.ascontiguousarray(t), K2.astype(np.float64), B2.astype(np.float64), pads=(1, 1, 1, 1))
        assert np.abs(y).max() < 2 ** 24
        return y.astype(np.float32)
    return graph, blob, fn

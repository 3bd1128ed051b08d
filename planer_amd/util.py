"""Tiled large-image inference around `net(x)` -- the reference's `util.tile` decorator and the
helpers it needs (`util.resize`, `make_slice`, `grid_slice`; util.py:253-269, 236-243, 291-348),
device-resident on MI355X.

Same contract as the reference: `@tile(sample, glob, window, margin)` wraps `f(img, *args)` where
`img` is an H x W (x C) image; the image is resampled, cut into overlapping windows, `f` is applied
to every window and the results are blended with border-distance weights and resampled back.
Here the image, the windows, `f`'s results and the blend buffers live in HBM: resampling, window
cuts, the weighted accumulation and the final division are HIP kernels (include/planer_hip.h:
pl_resize_hwc_f32, pl_strided_map_f32, pl_tile_accumulate_f32, pl_tile_normalise_f32); the host
only does the window geometry.  `f` receives and returns `DeviceArray`s.

One extension, because windows are independent and all of one size: with `batched=True`, `f` is
called ONCE with the stack of all windows (n, h, w[, c]) and returns the stack of results, so the
windows go through the net as one batch (the same batch-shard machinery as the forward pass).
"""
import itertools
import math

import numpy

from . import _lib
from . import hip
from .hip import DeviceArray
from .layer import _strided_map, _contig_strides, _f32


def _is_int(v, lo, hi=None):
    """v is an integer, and no bool, in [lo, hi] (hi None: no upper end)"""
    return not isinstance(v, bool) and isinstance(v, (int, numpy.integer)) and lo <= v and (hi is None or v <= hi)


def _is_number(v, nan=False):
    """v is an integer or a float, and no bool; a NaN only where `nan`"""
    return not isinstance(v, bool) and isinstance(v, (int, float, numpy.integer, numpy.floating)) and (nan or v == v)


def _launch_or_zero(ctx, images, pixels, zeroed, scratch_bytes, launch):
    """Behind a head's fresh outputs: with images and no pixel nothing is launched (the input may own no memory to point at) and
    `zeroed`, what only a launch would write, is memset; with pixels, launch(`scratch_bytes` of scratch from `ctx`'s pool)."""
    if images and not pixels:
        for a in zeroed:
            if a.nbytes:
                _lib.call("pl_memset", ctx.handle, a.ptr, 0, a.nbytes)
    elif images:
        scratch = hip.empty(((scratch_bytes + 7) // 8,), numpy.int64, ctx=ctx)      # (held until the launch is enqueued)
        launch(scratch.ptr)


def make_slice(l, w, mar):
    """util.make_slice (util.py:236-238)"""
    r = numpy.linspace(0, l - w, math.ceil((l - mar) / (w - mar)))
    return [slice(i, i + w) for i in r.astype(int).tolist()]


def grid_slice(H, W, h, w, mar):
    """util.grid_slice (util.py:240-242)"""
    a, b = make_slice(H, h, mar), make_slice(W, w, mar)
    return list(itertools.product(a, b))


def _axis_samples(n, size):
    """Sample rows (or columns) of util.resize (util.py:256-266): float32 linspace, clip, floor."""
    k = size / n
    pos = numpy.linspace(-0.5 + 0.5 / k, n - 0.5 - 0.5 / k, size, dtype=numpy.float32)
    pos = numpy.clip(pos, 0, n - 1, out=pos)
    lo = numpy.floor(numpy.clip(pos, 0, n - 1.001)).astype(int)
    pos -= lo
    return lo.astype(numpy.int32), pos


def resize(img, size):
    """util.resize (util.py:253-269): separable bilinear resampling of an H x W (x C) device image."""
    _f32(img)
    h, w = img.shape[:2]
    c = img.size // (h * w) if img.size else 1
    oh, ow = int(size[0]), int(size[1])
    ra, rs = _axis_samples(h, oh)
    ca, cs = _axis_samples(w, ow)
    dev = [hip.asarray(a, ctx=img.ctx) for a in (ra, rs, ca, cs)]
    y = hip.empty((oh, ow) + tuple(img.shape[2:]), ctx=img.ctx)
    _lib.call("pl_resize_hwc_f32", img.ctx.handle, img.ptr, y.ptr, h, w, c, oh, ow, *[d.ptr for d in dev])
    return y


# ---- uint8 image batches as net input ----------------------------------------------------------------------
def image_affine(mean, std, scale=255.0):
    """(k, b) with x / scale, - mean, / std folded into one multiply and one add per element: k = 1 / (scale * std),
    b = -mean / std, evaluated in float64 and rounded once to float32.  mean and std: one value per output channel."""
    mean = numpy.atleast_1d(numpy.asarray(mean, numpy.float64))
    std = numpy.atleast_1d(numpy.asarray(std, numpy.float64))
    mean, std = numpy.broadcast_arrays(mean, std)
    return (1.0 / (float(scale) * std)).astype(numpy.float32), (-mean / std).astype(numpy.float32)


def _sampling_tables(ctx, h, w, oh, ow):
    """util.resize's sampling tables (ra, rs, ca, cs) for (h, w) -> (oh, ow) as device arrays, or None where the sizes agree."""
    key = (h, w, oh, ow)
    if key[:2] == key[2:]:
        return None
    cache = ctx.__dict__.setdefault("_image_tables", {})
    if key not in cache:
        ra, rs = _axis_samples(key[0], key[2])
        ca, cs = _axis_samples(key[1], key[3])
        cache[key] = tuple(hip.asarray(a, ctx=ctx) for a in (ra, rs, ca, cs))
        ctx.synchronize()
    return cache[key]


class ImageSpec:
    """How a uint8 image batch becomes a net's float32 NCHW input: y[:, c] = fl(fl(r * k[c]) + b[c]) with r the byte of source
    channel order[c], or util.resize's sample of those bytes where `size` differs from the batch's H x W.  Host values only."""

    def __init__(self, k, b, layout="nhwc", size=None, order=None):
        k, b = numpy.atleast_1d(numpy.asarray(k)), numpy.atleast_1d(numpy.asarray(b))
        if layout not in ("nhwc", "nchw"):
            raise ValueError("image input: layout is 'nhwc' or 'nchw', got %r" % (layout,))
        if k.ndim != 1 or k.shape != b.shape or not 1 <= k.size <= 4:
            raise ValueError("image input: k and b hold one value per output channel (1 to 4), got shapes %s and %s" % (k.shape, b.shape))
        if order is not None:
            order = tuple(int(c) for c in order)
            if len(order) != k.size or min(order) < 0 or max(order) > 3:
                raise ValueError("image input: order names one source channel (0..3) per output channel, got %r" % (order,))
        if size is not None:
            if len(tuple(size)) != 2 or min(size) < 1:
                raise ValueError("image input: size is (height, width), got %r" % (size,))
            size = (int(size[0]), int(size[1]))
            if layout == "nchw":
                raise NotImplementedError("image input: resizing takes the 'nhwc' layout only")
        self.k, self.b = k.astype(numpy.float32), b.astype(numpy.float32)
        self.layout, self.size, self.order, self.channels = layout, size, order, int(k.size)
        self._k = (_lib.c_float * self.channels)(*self.k.tolist())
        self._b = (_lib.c_float * self.channels)(*self.b.tolist())
        self._order = (_lib.c_int * self.channels)(*order) if order is not None else None

    def geometry(self, shape):
        """(N, H, W, C) of a uint8 batch of `shape` in this layout and the (N, Co, OH, OW) it decodes to."""
        if len(shape) != 4:
            raise ValueError("image input: a uint8 batch is 4-d (%s), got shape %s" % (self.layout, tuple(shape)))
        n, h, w, c = shape if self.layout == "nhwc" else (shape[0], shape[2], shape[3], shape[1])
        if not 1 <= c <= 4:
            raise NotImplementedError("image input: 1 to 4 source channels, got %d in shape %s (%s)" % (c, tuple(shape), self.layout))
        if self.order is None and self.channels != c:
            raise ValueError("image input: %d values in k for %d source channels and no order" % (self.channels, c))
        if self.order is not None and max(self.order) >= c:
            raise ValueError("image input: order %r names a channel the %d-channel batch does not have" % (self.order, c))
        oh, ow = self.size if self.size is not None else (h, w)
        if (oh, ow) != (h, w) and (h < 2 or w < 2):
            raise ValueError("image input: resizing needs H, W >= 2, got %d x %d" % (h, w))
        return (n, h, w, c), (n, self.channels, oh, ow)

    def tables(self, ctx, src, out):
        """util.resize's sampling tables for (H, W) -> (OH, OW) as device arrays, or None where the sizes agree.  Kept on the
        Context object for its lifetime (every stream of the device may read them: the upload is over on return)."""
        return _sampling_tables(ctx, src[1], src[2], out[2], out[3])

    def bind(self, x):
        return ImageFeed(self, x)


class ImageFeed:
    """A uint8 device batch standing for the float32 tensor it decodes to: `shape` / `dtype` are the decoded tensor's (a plan
    is looked up by them), `decode_into` writes that tensor wherever the caller wants it, on the stream the caller names."""

    def __init__(self, spec, x):
        if not isinstance(x, DeviceArray) or x.dtype != numpy.uint8:
            raise TypeError("image input: expected a uint8 DeviceArray, got %r" % (x,))
        self.spec, self.u8, self.ctx = spec, x, x.ctx
        self.src, self.shape = spec.geometry(x.shape)
        self.dtype, self.ndim = numpy.dtype(numpy.float32), 4
        self.tabs = spec.tables(x.ctx, self.src, self.shape)

    @property
    def nbytes(self):
        return 4 * self.shape[0] * self.shape[1] * self.shape[2] * self.shape[3]

    def decode_into(self, ptr, ctx=None):
        n, h, w, c = self.src
        sp, t = self.spec, self.tabs
        _lib.call("pl_image_u8_nchw_f32", (ctx or self.ctx).handle, self.u8.ptr, ptr, n, h, w, c, int(sp.layout == "nhwc"),
                  sp.channels, sp._order, self.shape[2], self.shape[3], *([a.ptr for a in t] if t else [None] * 4), sp._k, sp._b)

    def materialise(self):
        y = hip.empty(self.shape, ctx=self.ctx)
        self.decode_into(y.ptr)
        return y

    def rows(self, lo, hi):
        return ImageFeed(self.spec, self.u8.rows(lo, hi))


def decode_images(x, k, b, layout="nhwc", size=None, order=None):
    """A uint8 DeviceArray batch, (N, H, W, C) or (N, C, H, W), as the float32 (N, Co, OH, OW) DeviceArray
    fl(fl(r * k[c]) + b[c]) (pl_image_u8_nchw_f32): r is the byte of source channel order[c] (default: c), bilinearly resampled
    to `size` as util.resize does where that differs from H x W.  (k, b) from `image_affine`.  Asynchronous on x's stream."""
    return ImageFeed(ImageSpec(k, b, layout, size, order), x).materialise()


# ---- uint8 images and label maps as net output -------------------------------------------------------------
def image_affine_inverse(mean, std, scale=255.0):
    """(k, b) that undo `image_affine`: (x * std + mean) * scale as one multiply and one add per element, k = scale * std,
    b = scale * mean, evaluated in float64 and rounded once to float32."""
    mean = numpy.atleast_1d(numpy.asarray(mean, numpy.float64))
    std = numpy.atleast_1d(numpy.asarray(std, numpy.float64))
    mean, std = numpy.broadcast_arrays(mean, std)
    return (float(scale) * std).astype(numpy.float32), (float(scale) * mean).astype(numpy.float32)


def _f32_nchw(what, x):
    """(N, C, H, W) of a 4-d float32 DeviceArray, or an error that names what `x` is."""
    if not isinstance(x, DeviceArray):
        raise TypeError("%s: expected a float32 DeviceArray (N, C, H, W), got %s" % (what, type(x).__name__))
    if x.dtype != numpy.float32 or x.ndim != 4:
        raise ValueError("%s: expected a float32 tensor (N, C, H, W), got %s of shape %s" % (what, x.dtype, tuple(x.shape)))
    return x.shape


class ImageOutSpec:
    """How a float32 NCHW result becomes a uint8 image batch: channel c is the byte of fl(fl(v * k[c]) + b[c]), v the sample of
    source plane order[c]; NaN -> 0, clamped to [0, 255], then rounded to nearest even ("nearest") or truncated ("truncate", what
    `astype(uint8)` does).  One value in k and b serves every output channel.  Host values only."""

    places = 1                                            # what `Net` hands back in this output's place: one array

    def __init__(self, k, b, layout="nhwc", order=None, rounding="nearest"):
        k, b = numpy.atleast_1d(numpy.asarray(k)), numpy.atleast_1d(numpy.asarray(b))
        if layout not in ("nhwc", "nchw"):
            raise ValueError("image output: layout is 'nhwc' or 'nchw', got %r" % (layout,))
        if rounding not in ("nearest", "truncate"):
            raise ValueError("image output: rounding is 'nearest' or 'truncate', got %r" % (rounding,))
        if k.ndim != 1 or k.shape != b.shape or not 1 <= k.size <= 4:
            raise ValueError("image output: k and b hold one value per output channel (1 to 4), got shapes %s and %s" % (k.shape, b.shape))
        if order is not None:
            order = tuple(int(c) for c in order)
            if not 1 <= len(order) <= 4 or min(order) < 0 or k.size not in (1, len(order)):
                raise ValueError("image output: order names one source plane (>= 0) per output channel (1 to 4, as many as k "
                                 "holds unless that is one), got %r" % (order,))
        self.k, self.b = k.astype(numpy.float32), b.astype(numpy.float32)
        self.layout, self.order, self.rounding = layout, order, rounding
        # output channels: the order's, else k's; one value in k and no order: as many as the tensor has, known at encode time
        self.channels = len(order) if order is not None else (int(k.size) if k.size > 1 else None)
        self._order = (_lib.c_int * len(order))(*order) if order is not None else None
        self._kb = {}                # output channels -> (k, b) as ctypes arrays, kept alive here

    def _affine(self, co):
        if co not in self._kb:
            k, b = numpy.broadcast_to(self.k, (co,)), numpy.broadcast_to(self.b, (co,))
            self._kb[co] = (_lib.c_float * co)(*k.tolist()), (_lib.c_float * co)(*b.tolist())
        return self._kb[co]

    def geometry(self, shape):
        """(N, C, H, W, Co) for a float32 result of `shape`, or a ValueError that names what does not fit."""
        n, c, h, w = shape
        co = self.channels or c
        if not 1 <= co <= 4:
            raise ValueError("image output: 1 to 4 output channels, got %d from shape %s" % (co, tuple(shape)))
        if self.order is None and co != c:
            raise ValueError("image output: %d values in k for %d channels and no order" % (co, c))
        if self.order is not None and max(self.order) >= c:
            raise ValueError("image output: order %r names a plane the %d-channel tensor does not have" % (self.order, c))
        return n, c, h, w, co

    def check(self, x):
        self.geometry(_f32_nchw("image output", x))

    def encode(self, x, ctx=None):
        """The uint8 DeviceArray of float32 (N, C, H, W) `x`, (N, H, W, Co) or (N, Co, H, W) (pl_image_f32_u8), a fresh array;
        asynchronous on `ctx`'s stream (default: x's)."""
        n, c, h, w, co = self.geometry(_f32_nchw("image output", x))
        ctx = ctx or x.ctx
        y = hip.empty((n, h, w, co) if self.layout == "nhwc" else (n, co, h, w), numpy.uint8, ctx=ctx)
        k, b = self._affine(co)
        _lib.call("pl_image_f32_u8", ctx.handle, x.ptr, y.ptr, n, c, h, w, co, self._order, int(self.layout == "nhwc"), k, b,
                  int(self.rounding == "truncate"))
        return y


class LabelSpec:
    """A float32 (N, C, H, W) result as the uint8 label map (N, H, W): numpy's argmax over the C planes (2 to 256), for C == 1
    the comparison x > threshold.  Host values only."""

    places = 1

    def __init__(self, threshold=0.0):
        t = float(numpy.float32(threshold))
        if t != t:
            raise ValueError("label output: threshold is a number, got %r" % (threshold,))
        self.threshold = t

    def geometry(self, shape):
        n, c, h, w = shape
        if not 1 <= c <= 256:
            raise ValueError("label output: 1 to 256 planes fit a byte, got %d in shape %s" % (c, tuple(shape)))
        return n, c, h, w

    def check(self, x):
        self.geometry(_f32_nchw("label output", x))

    def encode(self, x, ctx=None):
        """The uint8 (N, H, W) DeviceArray of float32 (N, C, H, W) `x` (pl_labels_f32_u8), a fresh array; asynchronous on `ctx`'s
        stream (default: x's)."""
        n, c, h, w = self.geometry(_f32_nchw("label output", x))
        ctx = ctx or x.ctx
        y = hip.empty((n, h, w), numpy.uint8, ctx=ctx)
        _lib.call("pl_labels_f32_u8", ctx.handle, x.ptr, y.ptr, n, c, h, w, self.threshold)
        return y


def encode_images(x, k, b, layout="nhwc", order=None, rounding="nearest"):
    """A float32 (N, C, H, W) DeviceArray as the uint8 image batch, (N, H, W, Co) or (N, Co, H, W): the byte of
    fl(fl(v * k[c]) + b[c]), NaN -> 0, clamped to [0, 255], rounded to nearest even or truncated (pl_image_f32_u8); v is the sample
    of source plane order[c] (default: c).  (k, b) from `image_affine_inverse`.  Asynchronous on x's stream."""
    return ImageOutSpec(k, b, layout, order, rounding).encode(x)


def label_map(x, threshold=0.0):
    """A float32 (N, C, H, W) DeviceArray as the uint8 label map (N, H, W): numpy's argmax over axis 1, or x > threshold where
    C == 1 (pl_labels_f32_u8).  Asynchronous on x's stream."""
    return LabelSpec(threshold).encode(x)


# ---- detections as net output ---------------------------------------------------------------------------------
def _f32v(v):
    """`v` rounded to float32, as the Python float the kernels get (their doubles are cast back without loss)."""
    return float(numpy.float32(v))


def _nms_sorted(boxes, classes, scores, n, r, k, floor, iou, class_aware, max_det, ctx):
    """top-k of scores (N, R) and pl_nms_f32 on the k first of each image: (det (N, max_det, 6), num (N,)), fresh arrays."""
    vals, idx = hip.empty((n, k), ctx=ctx), hip.empty((n, k), numpy.int64, ctx=ctx)
    if n and k:
        _lib.call("pl_topk_f32", ctx.handle, scores.ptr, n, r, 1, k, 1, vals.ptr, idx.ptr)
    det, num = hip.empty((n, max_det, 6), ctx=ctx), hip.empty((n,), numpy.int32, ctx=ctx)
    _lib.call("pl_nms_f32", ctx.handle, boxes.ptr, classes.ptr if classes is not None else None, vals.ptr, idx.ptr, n, r, k,
              floor, iou, int(bool(class_aware)), max_det, det.ptr, num.ptr)
    return det, num


class DetectionSpec:
    """How YOLO-style head tensors become detections.  heads[h] = (anchors, stride): anchors a sequence of 1 to 8 (aw, ah) pairs
    in input pixels, stride a number, an (sx, sy) pair or None (then size[1] / Gw, size[0] / Gh from size = (H, W)).  Head h is
    float32 (N, A_h (5 + classes), Gh, Gw).  An anchor's class is the argmax of its class logits (the first of equal maxima),
    its score sigmoid(t4) * sigmoid(t[5 + class]); it is a candidate iff score > conf.  The max_candidates (at most 4096) first
    candidates by (score descending, anchor index ascending) go through greedy NMS (dropped iff inter > iou * union with a kept
    box, class_aware: of the same class), which stops after max_det.  conf, iou, anchors and strides are rounded to float32, the
    numbers the kernels compute with.  Host values only."""

    def __init__(self, heads, classes, conf=0.25, iou=0.45, max_det=100, max_candidates=1024, class_aware=True, size=None):
        self.heads = []
        for h, head in enumerate(heads):
            try:
                anchors, stride = head
                anchors = numpy.asarray(anchors, numpy.float64).reshape(-1, 2)
            except (TypeError, ValueError):
                raise ValueError("detection output: head %d is (anchors, stride or None), anchors (aw, ah) pairs, got %r" % (h, head))
            if not 1 <= len(anchors) <= _lib.YOLO_MAX_ANCHORS:
                raise ValueError("detection output: head %d has %d anchors, 1 to %d fit" % (h, len(anchors), _lib.YOLO_MAX_ANCHORS))
            if stride is not None:
                stride = tuple(_f32v(s) for s in numpy.broadcast_to(numpy.asarray(stride, numpy.float64), (2,)))
            self.heads.append((anchors.astype(numpy.float32), stride))
        if not self.heads:
            raise ValueError("detection output: no heads given")
        if not _is_int(classes, 1):
            raise ValueError("detection output: classes is a count >= 1, got %r" % (classes,))
        if not _is_int(max_candidates, 1, _lib.NMS_MAX_CANDIDATES):
            raise ValueError("detection output: max_candidates is 1 to %d, got %r" % (_lib.NMS_MAX_CANDIDATES, max_candidates))
        if not _is_int(max_det, 1):
            raise ValueError("detection output: max_det is a count >= 1, got %r" % (max_det,))
        if size is not None:
            size = tuple(int(s) for s in size)
            if len(size) != 2 or min(size) < 1:
                raise ValueError("detection output: size is the input's (H, W), got %r" % (size,))
        self.classes, self.max_det, self.max_candidates = int(classes), int(max_det), int(max_candidates)
        self.conf, self.iou, self.class_aware, self.size = _f32v(conf), _f32v(iou), bool(class_aware), size
        self._anchors = [(_lib.c_float * a.size)(*a.ravel().tolist()) for a, _ in self.heads]       # kept alive here

    def geometry(self, shapes):
        """(N, [(A, C, Gh, Gw, sx, sy, offset) per head], A_total, k, max_det) for head tensors of `shapes`, k the entries NMS
        sees and max_det the rows of det (min(self.max_det, k)), or a ValueError that names what does not fit."""
        shapes = [tuple(s) for s in shapes]
        if len(shapes) != len(self.heads):
            raise ValueError("detection output: %d heads declared, %d tensors given" % (len(self.heads), len(shapes)))
        rows, off = [], 0
        for h, (shape, (anchors, stride)) in enumerate(zip(shapes, self.heads)):
            if len(shape) != 4:
                raise ValueError("detection output: head %d is (N, A (5 + C), Gh, Gw), got shape %s" % (h, shape))
            n, ch, gh, gw = shape
            a = len(anchors)
            if ch != a * (5 + self.classes):
                raise ValueError("detection output: head %d has %d channels, %d anchors x (5 + %d classes) is %d"
                                 % (h, ch, a, self.classes, a * (5 + self.classes)))
            if n != shapes[0][0]:
                raise ValueError("detection output: head %d has batch size %d, head 0 has %d" % (h, n, shapes[0][0]))
            if stride is None:
                if self.size is None or not gh or not gw:
                    raise ValueError("detection output: head %d has no stride and there is no input size to derive it from" % h)
                stride = _f32v(self.size[1] / gw), _f32v(self.size[0] / gh)
            rows.append((a, self.classes, gh, gw, stride[0], stride[1], off))
            off += a * gh * gw
        k = min(self.max_candidates, off)
        return shapes[0][0], rows, off, k, min(self.max_det, k)

    def check(self, xs):
        self.geometry([_f32_nchw("detection output", x) for x in xs])

    def encode(self, xs, ctx=None):
        """(det, num) of the head tensors `xs`: det float32 (N, max_det, 6), rows [x1, y1, x2, y2, score, class] by descending
        score and +0.0 behind them, num int32 (N,); fresh arrays (max_det is at most the number of anchors).  One
        pl_yolo_decode_f32 per head, pl_topk_f32, pl_nms_f32, asynchronous on `ctx`'s stream (default: the first head's);
        scores, classes, boxes and the top-k results are scratch from that context's pool."""
        n, rows, total, k, max_det = self.geometry([_f32_nchw("detection output", x) for x in xs])
        ctx = ctx or xs[0].ctx
        scores, boxes = hip.empty((n, total), ctx=ctx), hip.empty((n, total, 4), ctx=ctx)
        classes = hip.empty((n, total), numpy.int32, ctx=ctx)
        for x, anchors, (a, c, gh, gw, sx, sy, off) in zip(xs, self._anchors, rows):
            _lib.call("pl_yolo_decode_f32", ctx.handle, x.ptr, n, a, c, gh, gw, anchors, sx, sy, self.conf, total, off,
                      scores.ptr, classes.ptr, boxes.ptr)
        return _nms_sorted(boxes, classes, scores, n, total, k, self.conf, self.iou, self.class_aware, max_det, ctx)


def decode_detections(xs, heads, classes, conf=0.25, iou=0.45, max_det=100, max_candidates=1024, class_aware=True, size=None):
    """(det, num) of YOLO-style head tensors `xs` (float32 DeviceArrays): `DetectionSpec(heads, classes, ...).encode(xs)`."""
    return DetectionSpec(heads, classes, conf, iou, max_det, max_candidates, class_aware, size).encode(list(xs))


def nms(boxes, scores, classes=None, iou=0.45, max_det=100, floor=-math.inf):
    """Greedy NMS of boxes (N, K0, 4) float32 (x1, y1, x2, y2) with scores (N, K0) float32 and, if given, classes (N, K0) int32
    (only boxes of one class suppress each other): the min(K0, 4096) first of each image by (score descending, index ascending)
    with score > floor go through pl_nms_f32.  Returns det (N, min(max_det, K0, 4096), 6) and num (N,) like `DetectionSpec.encode`.
    Asynchronous on boxes' stream."""
    for what, a, dt, nd in (("boxes", boxes, numpy.float32, 3), ("scores", scores, numpy.float32, 2), ("classes", classes, numpy.int32, 2)):
        if a is None and what == "classes":
            continue
        if not isinstance(a, DeviceArray):
            raise TypeError("nms: %s is a %s DeviceArray, got %s" % (what, numpy.dtype(dt).name, type(a).__name__))
        if a.dtype != dt or a.ndim != nd:
            raise ValueError("nms: %s is %d-d %s, got %s of shape %s" % (what, nd, numpy.dtype(dt).name, a.dtype, tuple(a.shape)))
    n, r = scores.shape
    if boxes.shape != (n, r, 4) or (classes is not None and classes.shape != (n, r)):
        raise ValueError("nms: boxes (N, K0, 4), scores (N, K0) and classes (N, K0) do not agree: %s, %s, %s"
                         % (tuple(boxes.shape), tuple(scores.shape), None if classes is None else tuple(classes.shape)))
    if not _is_int(max_det, 1):
        raise ValueError("nms: max_det is a count >= 1, got %r" % (max_det,))
    k = min(r, _lib.NMS_MAX_CANDIDATES)
    return _nms_sorted(boxes, classes, scores, n, r, k, float(floor), _f32v(iou), classes is not None, min(int(max_det), k), boxes.ctx)


# ---- objects as net output --------------------------------------------------------------------------------------
def _cc_scratch_bytes(n, h, w, max_objects):
    """include/planer_hip.h PL_CC_SCRATCH_BYTES"""
    return n * max_objects * 16 + n * h * w * 4 + n * ((h * w + _lib.CC_BLOCK - 1) // _lib.CC_BLOCK) * 4


def _cc_arguments(what, connectivity, background, max_objects):
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError("%s: connectivity is 4 or 8, got %r" % (what, connectivity))
    if not _is_int(background, -1, 255):
        raise ValueError("%s: background is a class 0 to 255, or -1 for none, got %r" % (what, background))
    if not _is_int(max_objects, 0, _lib.CC_MAX_OBJECTS):
        raise ValueError("%s: max_objects is 0 to %d, got %r" % (what, _lib.CC_MAX_OBJECTS, max_objects))
    return int(connectivity), int(background), int(max_objects)


def _table_geometry(what, n, h, w, rows, width):
    """Refuses (n, h, w) maps and tables of `rows` rows of `width` ints per image that int32 indices do not reach."""
    if h * w >= 1 << 31 or n * h * w >= 1 << 31:
        raise ValueError("%s: %d x %d x %d is 2^31 or more pixels" % (what, n, h, w))
    if n * rows * width >= 1 << 31:
        raise ValueError("%s: %d images x %d rows is 2^31 or more table entries" % (what, n, rows))


def _components(m, n, h, w, connectivity, background, max_objects, ctx):
    """pl_components_u8_i32 on the uint8 map `m` (n, h, w): fresh (labels, num, objects, centroids); link, counts and the
    coordinate sums are scratch from `ctx`'s pool."""
    labels, num = hip.empty((n, h, w), numpy.int32, ctx=ctx), hip.empty((n,), numpy.int32, ctx=ctx)
    objects = hip.empty((n, max_objects, 6), numpy.int32, ctx=ctx)
    centroids = hip.empty((n, max_objects, 2), numpy.float32, ctx=ctx)
    _launch_or_zero(ctx, n, h * w, (num, objects, centroids), _cc_scratch_bytes(n, h, w, max_objects), lambda scratch: _lib.call(
        "pl_components_u8_i32", ctx.handle, m.ptr, n, h, w, connectivity, background, max_objects, scratch, labels.ptr, num.ptr,
        objects.ptr if max_objects else None, centroids.ptr if max_objects else None))
    return labels, num, objects, centroids


class ObjectSpec:
    """A float32 (N, C, H, W) result as objects: `LabelSpec`'s uint8 label map (argmax over the C planes, or x > threshold for
    C == 1), then its connected components.  An object is a maximal set of pixels of one image with equal class other than
    `background` (0 to 255; -1: every pixel belongs to an object), joined through 4- or 8-neighbour steps.  Objects are numbered
    1, 2, ... per image by the raster position of their first pixel; the first `max_objects` of them get a table row.  Host
    values only."""

    places = 4                                            # labels, num, objects, centroids

    def __init__(self, threshold=0.0, connectivity=8, background=0, max_objects=256):
        self.labels = LabelSpec(threshold)
        self.threshold = self.labels.threshold
        self.connectivity, self.background, self.max_objects = _cc_arguments("object output", connectivity, background, max_objects)

    def geometry(self, shape):
        """(N, C, H, W) for a float32 result of `shape`, or a ValueError that names what does not fit."""
        n, c, h, w = shape
        if not 1 <= c <= 256:
            raise ValueError("object output: 1 to 256 planes fit a byte, got %d in shape %s" % (c, tuple(shape)))
        _table_geometry("object output", n, h, w, self.max_objects, 6)
        return n, c, h, w

    def check(self, x):
        self.geometry(_f32_nchw("object output", x))

    def components(self, m, ctx=None):
        """The four arrays of the uint8 label map `m` (N, H, W), a DeviceArray."""
        n, h, w = m.shape
        _table_geometry("object output", n, h, w, self.max_objects, 6)
        return _components(m, n, h, w, self.connectivity, self.background, self.max_objects, ctx or m.ctx)

    def encode(self, x, ctx=None):
        """(labels, num, objects, centroids) of float32 (N, C, H, W) `x`, fresh arrays: labels int32 (N, H, W), 0 on background;
        num int32 (N,), which may exceed max_objects; objects int32 (N, max_objects, 6), row j = object j + 1 as
        [class, area, y0, x0, y1, x1] with a half-open box; centroids float32 (N, max_objects, 2) as [cy, cx]; unused rows are
        zero.  pl_labels_f32_u8 into scratch from `ctx`'s pool, then pl_components_u8_i32; asynchronous on `ctx`'s stream
        (default: x's), nothing waits for the host."""
        n, c, h, w = self.geometry(_f32_nchw("object output", x))
        ctx = ctx or x.ctx
        m = hip.empty((n, h, w), numpy.uint8, ctx=ctx)
        _lib.call("pl_labels_f32_u8", ctx.handle, x.ptr, m.ptr, n, c, h, w, self.threshold)
        return _components(m, n, h, w, self.connectivity, self.background, self.max_objects, ctx)


def connected_components(m, connectivity=8, background=0, max_objects=256):
    """(labels, num, objects, centroids) of a uint8 class map `m`, a DeviceArray (N, H, W) or (H, W): see `ObjectSpec.encode`;
    for (H, W) labels is (H, W) and the others keep their leading 1.  Asynchronous on m's stream (pl_components_u8_i32)."""
    if not isinstance(m, DeviceArray):
        raise TypeError("connected components: expected a uint8 DeviceArray (N, H, W) or (H, W), got %s" % type(m).__name__)
    if m.dtype != numpy.uint8 or m.ndim not in (2, 3):
        raise ValueError("connected components: expected a uint8 map (N, H, W) or (H, W), got %s of shape %s" % (m.dtype, tuple(m.shape)))
    connectivity, background, max_objects = _cc_arguments("connected components", connectivity, background, max_objects)
    n, h, w = (1,) + tuple(m.shape) if m.ndim == 2 else m.shape
    _table_geometry("connected components", n, h, w, max_objects, 6)
    labels, num, objects, centroids = _components(m, n, h, w, connectivity, background, max_objects, m.ctx)
    return (labels.reshape(h, w) if m.ndim == 2 else labels), num, objects, centroids


# ---- keypoints as net output ------------------------------------------------------------------------------------
def _peaks_scratch_bytes(n, k, h, w, max_peaks):
    """include/planer_hip.h PL_PEAKS_SCRATCH_BYTES"""
    return n * k * (-(-h // _lib.PEAKS_TILE_H)) * (-(-w // _lib.PEAKS_TILE_W)) * (max_peaks * 8 + 4)


def _peaks_arguments(what, threshold, ties, max_peaks, refine, stride):
    t = _f32v(threshold)
    if t != t:
        raise ValueError("%s: threshold is a number, got %r" % (what, threshold))
    if ties not in _lib.PEAKS_TIES:
        raise ValueError("%s: ties is 'all' or 'first', got %r" % (what, ties))
    if refine not in _lib.PEAKS_REFINE:
        raise ValueError("%s: refine is 'none' or 'quarter', got %r" % (what, refine))
    if not _is_int(max_peaks, 1, _lib.PEAKS_MAX_PEAKS):
        raise ValueError("%s: max_peaks is 1 to %d, got %r" % (what, _lib.PEAKS_MAX_PEAKS, max_peaks))
    pair = tuple(stride) if isinstance(stride, (tuple, list)) else (stride, stride)
    if len(pair) != 2 or not all(_is_number(v, nan=True) for v in pair):   # (a NaN is refused below, as not positive)
        raise ValueError("%s: stride is a number or an (sy, sx) pair, got %r" % (what, stride))
    sy, sx = _f32v(pair[0]), _f32v(pair[1])
    if not (0 < sy < math.inf and 0 < sx < math.inf):
        raise ValueError("%s: stride is positive and finite, got %r" % (what, stride))
    return t, ties, int(max_peaks), refine, (sy, sx)


def _peaks_geometry(what, n, k, h, w, max_peaks):
    if h > _lib.PEAKS_MAX_EXTENT or w > _lib.PEAKS_MAX_EXTENT:
        raise ValueError("%s: a plane of %d x %d is above %d in one extent" % (what, h, w, _lib.PEAKS_MAX_EXTENT))
    if h * w >= 1 << 31 or n * k >= 1 << 31 or n * k * h * w >= 1 << 31:
        raise ValueError("%s: %d x %d x %d x %d is 2^31 or more pixels" % (what, n, k, h, w))
    if 3 * n * k * max_peaks >= 1 << 31:
        raise ValueError("%s: %d planes x %d rows is 2^31 or more output floats" % (what, n * k, max_peaks))


class KeypointSpec:
    """Float32 heat maps (N, K, H, W) as points: per plane the 3 x 3 local maxima above `threshold`, counted, and the best
    `max_peaks` (1 to 256) of them as [x, y, score] rows by descending score, equal scores by ascending raster position.  Pixel p
    is a peak iff v[p] > threshold and, against each of its up to eight neighbours q inside the plane, v[p] >= v[q] (`ties`
    "all": the `maximum_filter(h, 3) == h` idiom) or v[p] > v[q] for q in front of p in raster order and >= behind ("first": a
    plateau yields the pixel that comes first).  IEEE float32 comparisons: a NaN is no peak and cancels its neighbours.  `refine`
    "quarter" moves a peak a quarter pixel towards the higher of its two neighbours along each axis (not on the plane's border);
    `stride` (a number or (sy, sx), held as float32) scales pixel positions to input pixels in one rounding.
    With max_peaks=1, ties="first" and threshold=-inf row 0 is numpy's argmax of the plane -- on planes without NaN whose maximum
    is above -inf, the single-person pose case; numpy's argmax returns a NaN's position, this returns the largest number that no
    NaN touches, or nothing.  Host values only."""

    places = 2                                            # what `Net` hands back in this output's place: peaks, num

    def __init__(self, threshold=0.0, ties="all", max_peaks=32, refine="none", stride=1.0):
        self.threshold, self.ties, self.max_peaks, self.refine, self.stride = _peaks_arguments(
            "keypoint output", threshold, ties, max_peaks, refine, stride)

    def geometry(self, shape):
        """(N, K, H, W) for a float32 result of `shape`, or a ValueError that names what does not fit."""
        n, k, h, w = shape
        _peaks_geometry("keypoint output", n, k, h, w, self.max_peaks)
        return n, k, h, w

    def check(self, x):
        self.geometry(_f32_nchw("keypoint output", x))

    def encode(self, x, ctx=None):
        """(peaks, num) of float32 (N, K, H, W) `x`, fresh arrays: peaks float32 (N, K, max_peaks, 3), row j the plane's j-th
        peak as [x, y, score] and +0.0 from row min(num, max_peaks) on; num int32 (N, K), all peaks of the plane, which may
        exceed max_peaks.  pl_peaks_f32 with scratch from `ctx`'s pool; asynchronous on `ctx`'s stream (default: x's), nothing
        waits for the host."""
        n, k, h, w = self.geometry(_f32_nchw("keypoint output", x))
        ctx = ctx or x.ctx
        peaks, num = hip.empty((n, k, self.max_peaks, 3), numpy.float32, ctx=ctx), hip.empty((n, k), numpy.int32, ctx=ctx)
        _launch_or_zero(ctx, n * k, h * w, (peaks, num), _peaks_scratch_bytes(n, k, h, w, self.max_peaks), lambda scratch: _lib.call(
            "pl_peaks_f32", ctx.handle, x.ptr, n, k, h, w, self.threshold, _lib.PEAKS_TIES[self.ties], self.max_peaks,
            _lib.PEAKS_REFINE[self.refine], self.stride[0], self.stride[1], scratch, peaks.ptr, num.ptr))
        return peaks, num


def heatmap_peaks(x, threshold=0.0, ties="all", max_peaks=32, refine="none", stride=1.0):
    """(peaks, num) of float32 heat maps `x`, a DeviceArray (N, K, H, W), (K, H, W) or (H, W): see `KeypointSpec`; peaks is
    x.shape[:-2] + (max_peaks, 3) and num x.shape[:-2].  Asynchronous on x's stream (pl_peaks_f32)."""
    if not isinstance(x, DeviceArray):
        raise TypeError("heat-map peaks: expected a float32 DeviceArray (N, K, H, W), (K, H, W) or (H, W), got %s" % type(x).__name__)
    if x.dtype != numpy.float32 or x.ndim not in (2, 3, 4):
        raise ValueError("heat-map peaks: expected float32 maps (N, K, H, W), (K, H, W) or (H, W), got %s of shape %s"
                         % (x.dtype, tuple(x.shape)))
    spec = KeypointSpec(threshold, ties, max_peaks, refine, stride)
    lead = tuple(x.shape[:-2])
    peaks, num = spec.encode(x.reshape((1,) * (4 - x.ndim) + tuple(x.shape)))
    return peaks.reshape(lead + (spec.max_peaks, 3)), num.reshape(lead)


# ---- instances as net output ------------------------------------------------------------------------------------
def _flow_scratch_bytes(n, h, w, max_instances):
    """include/planer_hip.h PL_FLOW_SCRATCH_BYTES"""
    def align(b):
        return (b + 15) // 16 * 16
    return (16 + n * max_instances * 16 + 4 * align(n * h * w * 4) + align(n * ((h + 1) // 2) * ((w + 1) // 2) * 4) + align(n * 4)
            + align(n * h * w) + _cc_scratch_bytes(n, h, w, 0))


def _flow_arguments(what, level, min_flow, rounds, min_size, max_instances, planes):
    for name, v in (("level", level), ("min_flow", min_flow)):
        if not _is_number(v):
            raise ValueError("%s: %s is a number, got %r" % (what, name, v))
    for name, v, top in (("rounds", rounds, _lib.FLOW_MAX_ROUNDS), ("min_size", min_size, (1 << 31) - 1),
                         ("max_instances", max_instances, _lib.FLOW_MAX_INSTANCES)):
        if not _is_int(v, 0, top):
            raise ValueError("%s: %s is 0 to %d, got %r" % (what, name, top, v))
    try:
        planes = tuple(planes)
    except TypeError:
        planes = ()
    if len(planes) != 3 or not all(_is_int(p, 0) for p in planes) or len(set(planes)) != 3:
        raise ValueError("%s: planes names three distinct planes (dy, dx, prob), got %r" % (what, planes))
    return _f32v(level), _f32v(min_flow), int(rounds), int(min_size), int(max_instances), tuple(int(p) for p in planes)


class FlowSpec:
    """A float32 (N, C, H, W) result as instance masks by flow following (cellpose's product): planes[0], planes[1] are a flow
    field (dy, dx), planes[2] a probability.  A pixel is foreground iff prob > level.  A foreground pixel whose flow is longer
    than min_flow points at the neighbour in the flow's direction (eight directions, clamped at the border) if that neighbour is
    foreground, else at itself; every pixel follows the pointers for exactly 2^rounds steps; the pixels that were arrived at form
    the sink map, whose 8-connected regions number the raw instances (by the raster position of a region's first pixel); raw
    instances of fewer than `min_size` pixels are dropped and the rest renumbered 1, 2, ... in the same order.  The first
    `max_instances` of them get a table row.  Everything behind one float32 decision per pixel is integer arithmetic: the result is
    exact (include/planer_hip.h states the rule operation by operation).  level and min_flow are rounded to float32.  Host
    values only."""

    places = 4                                            # masks, num, instances, centres

    def __init__(self, level=0.0, min_flow=0.0, rounds=10, min_size=15, max_instances=256, planes=(0, 1, 2)):
        self.level, self.min_flow, self.rounds, self.min_size, self.max_instances, self.planes = _flow_arguments(
            "flow output", level, min_flow, rounds, min_size, max_instances, planes)

    def geometry(self, shape):
        """(N, C, H, W) for a float32 result of `shape`, or a ValueError that names what does not fit."""
        n, c, h, w = shape
        if c < 3 or max(self.planes) >= c:
            raise ValueError("flow output: planes %s of a result with %d planes, shape %s" % (self.planes, c, tuple(shape)))
        _table_geometry("flow output", n, h, w, self.max_instances, 5)
        return n, c, h, w

    def check(self, x):
        self.geometry(_f32_nchw("flow output", x))

    def follow(self, x, n, h, w, image_stride, pixel_stride, offsets, ctx):
        """pl_flow_instances_f32 on the float32 DeviceArray `x`, element (i, plane, y, x) at i image_stride + offsets[plane] +
        (y w + x) pixel_stride: fresh (masks, num, instances, centres); everything else is scratch from `ctx`'s pool."""
        m = self.max_instances
        _table_geometry("flow output", n, h, w, m, 5)
        masks, num = hip.empty((n, h, w), numpy.int32, ctx=ctx), hip.empty((n,), numpy.int32, ctx=ctx)
        instances, centres = hip.empty((n, m, 5), numpy.int32, ctx=ctx), hip.empty((n, m, 2), numpy.float32, ctx=ctx)
        _launch_or_zero(ctx, n, h * w, (num, instances, centres), _flow_scratch_bytes(n, h, w, m), lambda scratch: _lib.call(
            "pl_flow_instances_f32", ctx.handle, x.ptr, n, h, w, image_stride, pixel_stride, offsets[0], offsets[1], offsets[2],
            self.level, self.min_flow, self.rounds, self.min_size, m, scratch, masks.ptr, num.ptr,
            instances.ptr if m else None, centres.ptr if m else None))
        return masks, num, instances, centres

    def encode(self, x, ctx=None):
        """(masks, num, instances, centres) of float32 (N, C, H, W) `x`, fresh arrays: masks int32 (N, H, W), 0 on background
        and on dropped instances; num int32 (N,), which may exceed max_instances; instances int32 (N, max_instances, 5), row j =
        instance j + 1 as [area, y0, x0, y1, x1] with a half-open box; centres float32 (N, max_instances, 2) as [cy, cx]; unused
        rows are zero.  pl_flow_instances_f32 with scratch from `ctx`'s pool; asynchronous on `ctx`'s stream (default: x's),
        nothing waits for the host."""
        n, c, h, w = self.geometry(_f32_nchw("flow output", x))
        return self.follow(x, n, h, w, c * h * w, 1, [p * h * w for p in self.planes], ctx or x.ctx)

    def encode_hwc(self, x, ctx=None):
        """The same of ONE float32 map (H, W, C), `Net.tiled`'s blended result: (masks (1, H, W), num (1,), ...)."""
        h, w, c = x.shape
        self.geometry((1, c, h, w))
        return self.follow(x, 1, h, w, max(h * w * c, 1), c, list(self.planes), ctx or x.ctx)


def follow_flows(x, level=0.0, min_flow=0.0, rounds=10, min_size=15, max_instances=256, planes=(0, 1, 2)):
    """(masks, num, instances, centres) of float32 flow and probability planes `x`, a DeviceArray (N, C, H, W) or (C, H, W): see
    `FlowSpec`; for (C, H, W) masks is (H, W) and the others keep their leading 1.  Asynchronous on x's stream
    (pl_flow_instances_f32)."""
    if not isinstance(x, DeviceArray):
        raise TypeError("flow following: expected a float32 DeviceArray (N, C, H, W) or (C, H, W), got %s" % type(x).__name__)
    if x.dtype != numpy.float32 or x.ndim not in (3, 4):
        raise ValueError("flow following: expected float32 planes (N, C, H, W) or (C, H, W), got %s of shape %s" % (x.dtype, tuple(x.shape)))
    spec = FlowSpec(level, min_flow, rounds, min_size, max_instances, planes)
    masks, num, instances, centres = spec.encode(x.reshape((1,) * (4 - x.ndim) + tuple(x.shape)))
    return (masks.reshape(masks.shape[1:]) if x.ndim == 3 else masks), num, instances, centres


# ---- text as net output -------------------------------------------------------------------------------------------
TEXT_LAYOUTS = ("tnc", "ntc", "nchw")


def _text_scratch_bytes(s, t):
    """include/planer_hip.h PL_TEXT_SCRATCH_BYTES"""
    return s * t * 8


def _text_arguments(what, layout, blank, merge_repeated, confidence, max_len):
    if layout not in TEXT_LAYOUTS:
        raise ValueError("%s: layout is 'tnc', 'ntc' or 'nchw', got %r" % (what, layout))
    if not _is_int(blank, 0):
        raise ValueError("%s: blank is a class number >= 0, got %r" % (what, blank))
    if not isinstance(merge_repeated, (bool, numpy.bool_)):
        raise ValueError("%s: merge_repeated is True or False, got %r" % (what, merge_repeated))
    if confidence not in _lib.TEXT_CONF:
        raise ValueError("%s: confidence is 'softmax', 'value' or 'none', got %r" % (what, confidence))
    if not _is_int(max_len, 1, _lib.TEXT_MAX_LEN):
        raise ValueError("%s: max_len is 1 to %d, got %r" % (what, _lib.TEXT_MAX_LEN, max_len))
    return layout, int(blank), bool(merge_repeated), confidence, int(max_len)


class TextSpec:
    """A float32 sequence tensor as text by greedy CTC decoding.  `layout` says where sequences, frames and classes are: "tnc"
    (T, N, C) and "ntc" (N, T, C) hold N sequences, "nchw" (N, C, H, W) one per (n, h) with time along W.  A frame's label is
    numpy's argmax over its classes (the first of equal maxima, the first NaN before any number); a frame starts a symbol iff its
    label is not `blank` and, with `merge_repeated`, differs from the label of the frame in front.  The first `max_len` (1 to
    1024) symbols of a sequence come back with the confidence of their first frame -- `confidence` "softmax": 1 / sum exp(x - max)
    over the frame's classes, NaN where the maximum is not finite; "value": the bits of x at the argmax, for nets that end in
    their own softmax; "none": +0.0 -- and their [start, end) frames.  Everything but the softmax confidence is exact.  Host values
    only."""

    places = 4                                            # text, length, conf, spans

    def __init__(self, layout="tnc", blank=0, merge_repeated=True, confidence="softmax", max_len=64):
        self.layout, self.blank, self.merge_repeated, self.confidence, self.max_len = _text_arguments(
            "text output", layout, blank, merge_repeated, confidence, max_len)

    def geometry(self, shape):
        """(lead, S_outer, S_inner, T, C, (st_outer, st_inner, st_time, st_class)) for a float32 result of `shape`, lead the
        shape of the sequences, or a ValueError that names what does not fit."""
        shape = tuple(int(v) for v in shape)
        want = 4 if self.layout == "nchw" else 3
        if len(shape) != want:
            raise ValueError("text output: layout %r takes a %d-d tensor, got shape %s" % (self.layout, want, shape))
        if self.layout == "tnc":
            (t, n, c), inner = shape, 1
            strides = (c, 0, n * c, 1)
        elif self.layout == "ntc":
            (n, t, c), inner = shape, 1
            strides = (t * c, 0, c, 1)
        else:
            n, c, inner, t = shape
            strides = (c * inner * t, t, 1, inner * t)
        if c < 1:
            raise ValueError("text output: a frame has at least one class, got shape %s" % (shape,))
        if self.blank >= c:
            raise ValueError("text output: blank = %d is no class of the %d in shape %s" % (self.blank, c, shape))
        if t > _lib.TEXT_MAX_FRAMES:
            raise ValueError("text output: %d frames are above %d" % (t, _lib.TEXT_MAX_FRAMES))
        if n * inner * t * c >= 1 << 31 or n * inner >= 1 << 31:
            raise ValueError("text output: shape %s is 2^31 or more elements or sequences" % (shape,))
        return ((n, inner) if self.layout == "nchw" else (n,)), n, inner, t, c, strides

    def _shape(self, x):
        if not isinstance(x, DeviceArray):
            raise TypeError("text output: expected a float32 DeviceArray, got %s" % type(x).__name__)
        if x.dtype != numpy.float32:
            raise ValueError("text output: expected a float32 tensor, got %s of shape %s" % (x.dtype, tuple(x.shape)))
        return self.geometry(x.shape)

    def check(self, x):
        self._shape(x)

    def encode(self, x, ctx=None, lengths=None):
        """(text, length, conf, spans) of float32 `x`, fresh arrays with `lead` = (N,) or, for "nchw", (N, H): text int32
        lead + (max_len,), the labels of the first max_len symbols and -1 behind them; length int32 lead, all symbols of the
        sequence, which may exceed max_len; conf float32 lead + (max_len,), +0.0 behind; spans int32 lead + (max_len, 2),
        [start, end) in frames, 0 behind.  `lengths`: valid frames per sequence, a host int array or a device int32 array of
        `lead`'s size (values above T count as T, below 0 as 0); None: every frame.  pl_ctc_greedy_f32 with scratch from `ctx`'s
        pool; asynchronous on `ctx`'s stream (default: x's), nothing waits for the host."""
        lead, n, inner, t, c, strides = self._shape(x)
        ctx = ctx or x.ctx
        s, m = n * inner, self.max_len
        if lengths is not None:
            if not isinstance(lengths, DeviceArray):
                host = numpy.asarray(lengths)
                if host.dtype.kind not in "iu" or host.size != s:
                    raise ValueError("text output: lengths is an integer array with one entry per sequence (%d), got %s of shape %s"
                                     % (s, host.dtype, host.shape))
                lengths = hip.asarray(numpy.clip(host, 0, t).astype(numpy.int32).reshape(-1), ctx=ctx)
            elif lengths.dtype != numpy.int32 or lengths.size != s:
                raise ValueError("text output: lengths is an int32 array with one entry per sequence (%d), got %s of shape %s"
                                 % (s, lengths.dtype, tuple(lengths.shape)))
        text, length = hip.empty(lead + (m,), numpy.int32, ctx=ctx), hip.empty(lead, numpy.int32, ctx=ctx)
        conf, spans = hip.empty(lead + (m,), numpy.float32, ctx=ctx), hip.empty(lead + (m, 2), numpy.int32, ctx=ctx)
        if s and not t:                                     # no frame: no symbol, and -1 is four 0xFF bytes
            _lib.call("pl_memset", ctx.handle, text.ptr, 0xFF, text.nbytes)
        _launch_or_zero(ctx, s, t, (length, conf, spans), _text_scratch_bytes(s, t), lambda scratch: _lib.call(
            "pl_ctc_greedy_f32", ctx.handle, x.ptr, n, inner, t, c, strides[0], strides[1], strides[2], strides[3],
            None if lengths is None else lengths.ptr, self.blank, int(self.merge_repeated), _lib.TEXT_CONF[self.confidence], m,
            scratch, text.ptr, length.ptr, conf.ptr, spans.ptr))
        return text, length, conf, spans


def ctc_decode(x, layout="tnc", blank=0, merge_repeated=True, confidence="softmax", max_len=64, lengths=None):
    """(text, length, conf, spans) of the float32 DeviceArray `x` by greedy CTC decoding: see `TextSpec` and `TextSpec.encode`.
    Asynchronous on x's stream (pl_ctc_greedy_f32)."""
    return TextSpec(layout, blank, merge_repeated, confidence, max_len).encode(x, lengths=lengths)


def text_strings(text, length, alphabet):
    """The decoded strings of host arrays `text` (..., max_len) and `length` (...) as `TextSpec.encode` hands them back (after
    `.get()`): a list of str per sequence, nested like the leading axes, alphabet[label] the character of a label (the blank's
    entry is never used).  Only the first min(length, max_len) labels of a sequence are used."""
    text, length = numpy.asarray(text), numpy.asarray(length)
    if text.ndim < 1 or text.shape[:-1] != length.shape:
        raise ValueError("text strings: text is (..., max_len) and length (...), got %s and %s" % (text.shape, length.shape))
    if text.ndim == 1:
        labels = text[:min(int(length), text.shape[0])]
        if labels.size and (labels.min() < 0 or labels.max() >= len(alphabet)):
            raise ValueError("text strings: a label outside the alphabet of %d: %s" % (len(alphabet), labels.tolist()))
        return "".join(alphabet[int(v)] for v in labels)
    return [text_strings(t, n, alphabet) for t, n in zip(text, length)]


# ---- tiled inference around a plan: windows cut and blended in one launch each ----------------------------------
def _window_origins(windows):
    """(r0, c0, h, w) of a list of (row slice, column slice) windows of one size: int32 origin arrays and the extent."""
    windows = list(windows)
    if not windows:
        raise ValueError("tile windows: at least one window")
    r0 = numpy.array([r.start for r, _ in windows], numpy.int32)
    c0 = numpy.array([c.start for _, c in windows], numpy.int32)
    h, w = windows[0][0].stop - windows[0][0].start, windows[0][1].stop - windows[0][1].start
    if h < 1 or w < 1 or any((r.stop - r.start, c.stop - c.start) != (h, w) for r, c in windows):
        raise ValueError("tile windows: every window has the first one's size, %d x %d" % (h, w))
    return r0, c0, h, w


class WindowFeed(ImageFeed):
    """Windows of ONE device image (H, W[, C]), uint8 or float32, standing for the float32 (slots, Co, h, w) batch they are cut
    into (pl_tile_windows_*_nchw_f32): what `ImageFeed` is for a uint8 batch, so a plan is looked up by `shape` / `dtype` and fed
    by `decode_into`.  uint8 images need an `ImageSpec`, whose k, b and order are used (its size and layout are not); `work`:
    the working size the windows are cut from, the image resampled as util.resize does where it differs from H x W.  Slots
    past the last window repeat it.  The origins are uploaded once, here; `chunk` / `rows` hand out runs of slots."""

    def __init__(self, image, windows, spec=None, work=None, slots=None):
        if not isinstance(image, DeviceArray) or image.dtype not in (numpy.uint8, numpy.float32) or image.ndim not in (2, 3):
            raise TypeError("tile windows: expected a uint8 or float32 DeviceArray (H, W[, C]), got %r" % (image,))
        height, width = image.shape[:2]
        c = image.shape[2] if image.ndim == 3 else 1
        r0, c0, h, w = _window_origins(windows)
        wh, ww = (height, width) if work is None else (int(work[0]), int(work[1]))
        if min(r0.min(), c0.min()) < 0 or r0.max() + h > wh or c0.max() + w > ww:
            raise ValueError("tile windows: a %d x %d window lies outside the %d x %d working image" % (h, w, wh, ww))
        if (wh, ww) != (height, width) and (height < 2 or width < 2):
            raise ValueError("tile windows: resampling needs H, W >= 2, got %d x %d" % (height, width))
        if image.dtype == numpy.uint8:
            if spec is None:
                raise ValueError("tile windows: a uint8 image needs k and b (util.image_affine)")
            if not 1 <= c <= 4:
                raise NotImplementedError("tile windows: 1 to 4 uint8 source channels, got %d" % c)
            if spec.order is None and spec.channels != c:
                raise ValueError("tile windows: %d values in k for %d source channels and no order" % (spec.channels, c))
            if spec.order is not None and max(spec.order) >= c:
                raise ValueError("tile windows: order %r names a channel the %d-channel image does not have" % (spec.order, c))
            co = spec.channels
        else:
            if c < 1:
                raise ValueError("tile windows: an image without channels, shape %s" % (tuple(image.shape),))
            spec, co = None, c
        n = len(r0)
        slots = n if slots is None else int(slots)
        if slots < n:
            raise ValueError("tile windows: %d slots for %d windows" % (slots, n))
        self.spec, self.u8, self.ctx = spec, image, image.ctx
        self.src, self.work, self.shape = (height, width, c), (wh, ww), (slots, co, h, w)
        self.dtype, self.ndim = numpy.dtype(numpy.float32), 4
        self.tabs = _sampling_tables(image.ctx, height, width, wh, ww)
        self.origins = hip.asarray(numpy.concatenate([r0, c0]), ctx=image.ctx)      # [r0 of every window, c0 of every window]
        self.count, self.first, self.n = n, 0, n

    def chunk(self, lo, slots):
        """The feed of `slots` slots that starts at window `lo` of this one (windows past the last repeat it)."""
        if not 0 <= lo < self.n or slots < 1:
            raise IndexError((lo, slots))
        sub = WindowFeed.__new__(WindowFeed)
        for key, v in self.__dict__.items():
            setattr(sub, key, v)
        sub.first, sub.n, sub.shape = self.first + lo, min(self.n - lo, slots), (slots,) + self.shape[1:]
        return sub

    def rows(self, lo, hi):
        return self.chunk(min(lo, self.n - 1), hi - lo)

    def decode_into(self, ptr, ctx=None):
        height, width, c = self.src
        slots, co, h, w = self.shape
        r0 = self.origins.ptr + 4 * self.first
        geo = (r0, r0 + 4 * self.count, self.n, slots, h, w, self.work[0], self.work[1])
        tabs = [a.ptr for a in self.tabs] if self.tabs else [None] * 4
        handle = (ctx or self.ctx).handle
        if self.spec is not None:
            sp = self.spec
            _lib.call("pl_tile_windows_u8_nchw_f32", handle, self.u8.ptr, ptr, height, width, c, co, sp._order, *geo, *tabs, sp._k, sp._b)
        else:
            _lib.call("pl_tile_windows_f32_nchw_f32", handle, self.u8.ptr, ptr, height, width, c, *geo, *tabs)


def cut_windows(image, windows, k=None, b=None, order=None, work=None, slots=None):
    """The windows `windows` ((row slice, column slice) pairs of one size, as `grid_slice` returns them) of the device image
    (H, W[, C]) as the float32 (slots, Co, h, w) DeviceArray a net reads, in ONE launch (pl_tile_windows_*_nchw_f32).  uint8
    images: fl(fl(r * k[c]) + b[c]) of source channel order[c] ((k, b) from `image_affine`); float32 images: a copy (k, b, order
    unused).  `work`: the (height, width) the windows are cut from; where it differs from H x W the image is resampled as
    util.resize does, on the way and never as a whole.  `slots` (default: the number of windows): slots past the last window
    repeat it.  Asynchronous on the image's stream."""
    if isinstance(image, DeviceArray) and image.dtype == numpy.uint8:
        if k is None or b is None:
            raise ValueError("tile windows: a uint8 image needs k and b (util.image_affine)")
        spec = ImageSpec(k, b, "nhwc", None, order)
    else:
        spec = None
    return WindowFeed(image, windows, spec, work, slots).materialise()


class BlendGeometry:
    """Host arithmetic of one blend (util.py:317-343 of the reference): for windows cut from a working image of `work` pixels
    whose results are (oh, ow) each, the scale k, the scaled origins R0 / C0 (int(start * k), int32), the row-major grid shape
    (gr, gc), the output size (OH, OW) = (int(work_h * k), int(work_w * k)) and ramp = int(margin * k); one window: the output is
    the window result, ramp 0.  ValueError where a scaled window is not oh x ow (the reference's broadcast error), where a pixel
    is covered by no window, or where the weight total could pass the reference's uint16."""

    def __init__(self, windows, k, margin, work, oh, ow):
        windows = list(windows)
        r0, c0, _, _ = _window_origins(windows)
        self.n, self.k, self.oh, self.ow = len(windows), k, int(oh), int(ow)
        for gc in range(self.n, 0, -1):                   # (the widest grid that fits: any that fits visits the windows alike)
            rows, cols = [r for r, _ in windows[::gc]], [c for _, c in windows[:gc]]
            if self.n % gc == 0 and windows == list(itertools.product(rows, cols)):
                break
        else:
            raise ValueError("tile blend: the windows are no row-major grid (itertools.product(rows, columns))")
        self.gr, self.gc = self.n // gc, gc
        if self.n == 1:
            self.R0, self.C0 = numpy.zeros(1, numpy.int32), numpy.zeros(1, numpy.int32)
            self.OH, self.OW, self.ramp = self.oh, self.ow, 0
            return
        for axis, (cuts, size) in enumerate(((rows, self.oh), (cols, self.ow))):
            for s in cuts:
                if int(s.stop * k) - int(s.start * k) != size:
                    raise ValueError("tile blend: window %s [%d, %d) scales by %r to %d pixels, the net's result has %d"
                                     % ("rows" if axis == 0 else "columns", s.start, s.stop, k, int(s.stop * k) - int(s.start * k), size))
        self.R0 = numpy.array([int(r.start * k) for r, _ in windows], numpy.int32)
        self.C0 = numpy.array([int(c.start * k) for _, c in windows], numpy.int32)
        self.OH, self.OW, self.ramp = int(work[0] * k), int(work[1] * k), int(margin * k)
        most = 1
        for cuts, size, total in ((rows, self.oh, self.OH), (cols, self.ow, self.OW)):
            cover = numpy.zeros(total + 1, numpy.int64)
            for s in cuts:
                a = int(s.start * k)
                if a + size > total:
                    raise ValueError("tile blend: a window result ends at %d, the output has %d" % (a + size, total))
                cover[a] += 1
                cover[a + size] -= 1
            cover = numpy.cumsum(cover)[:total]
            if total and cover.min() < 1:
                raise ValueError("tile blend: output pixel %d is covered by no window" % int(cover.argmin()))
            most *= int(cover.max()) if total else 1
        if (self.ramp + 1) * most > 65535:
            raise ValueError("tile blend: weight %d on %d windows over one pixel passes 65535, the reference's uint16 count"
                             % (self.ramp + 1, most))


def blend_windows(outs, windows, k, margin, work, out="float"):
    """All window results `outs`, float32 (n, Co, oh, ow) as a net wrote them for `windows` (see `cut_windows`), blended into the
    whole output in ONE launch (pl_tile_blend_*): per pixel the covering windows in grid order, weights rising from 1 at a
    window's edge to int(margin * k) + 1, the reference's float32 loop bit for bit.  k: output pixels per working pixel; margin
    in working pixels; work: the working image's (height, width).  out="float": float32 (OH, OW, Co); an `ImageOutSpec`: the uint8
    image in its layout, (OH, OW, Co') or (Co', OH, OW); a `LabelSpec`: the uint8 label map (OH, OW).  Asynchronous on outs'
    stream; `BlendGeometry` raises ValueError for geometries the reference cannot blend."""
    n, c, oh, ow = _f32_nchw("tile blend", outs)
    windows = list(windows)
    if n != len(windows):
        raise ValueError("tile blend: %d results for %d windows" % (n, len(windows)))
    geo = BlendGeometry(windows, k, margin, work, oh, ow)
    ctx = outs.ctx
    origins = hip.asarray(numpy.concatenate([geo.R0, geo.C0]), ctx=ctx)
    args = (n, c, oh, ow, origins.ptr, origins.ptr + 4 * n, geo.gr, geo.gc, geo.OH, geo.OW, geo.ramp)
    if isinstance(out, ImageOutSpec):
        co = out.geometry((n, c, oh, ow))[4]
        y = hip.empty((geo.OH, geo.OW, co) if out.layout == "nhwc" else (co, geo.OH, geo.OW), numpy.uint8, ctx=ctx)
        kk, bb = out._affine(co)
        _lib.call("pl_tile_blend_u8", ctx.handle, outs.ptr, y.ptr, *args, co, out._order, int(out.layout == "nhwc"), kk, bb,
                  int(out.rounding == "truncate"))
    elif isinstance(out, LabelSpec):
        out.geometry((n, c, oh, ow))
        y = hip.empty((geo.OH, geo.OW), numpy.uint8, ctx=ctx)
        _lib.call("pl_tile_blend_labels_u8", ctx.handle, outs.ptr, y.ptr, *args, out.threshold)
    elif out == "float":
        y = hip.empty((geo.OH, geo.OW, c), ctx=ctx)
        _lib.call("pl_tile_blend_f32", ctx.handle, outs.ptr, y.ptr, *args)
    else:
        raise ValueError("tile blend: out is 'float', an ImageOutSpec or a LabelSpec, got %r" % (out,))
    return y


def _window(img, rc):
    """img[rows, cols] as a contiguous device array."""
    r, c = rc
    nd = img.ndim
    start = [r.start, c.start] + [0] * (nd - 2)
    out = [r.stop - r.start, c.stop - c.start] + list(img.shape[2:])
    return _strided_map(img, out, _contig_strides(img.shape), start, [1] * nd, extent=list(img.shape))


def _stack(arrays):
    out = hip.empty((len(arrays),) + arrays[0].shape, ctx=arrays[0].ctx)
    for i, a in enumerate(arrays):
        out[i].copy_from(a)
    return out


class _Tiling:
    """Geometry of one tiled run (host arithmetic only), following util.tile's rules
    (util.py:300-316): the working size after `sample`, growth of images smaller than the window to
    a multiple of `glob`, the window extents, the margin in pixels and the window grid."""

    def __init__(self, height, width, sample, glob, window, margin):
        self.src = [height, width]
        work = list(sample) if isinstance(sample, tuple) else [int(height * sample), int(width * sample)]
        extent = [window, window]
        for axis in (0, 1):
            if window > work[axis]:                      # smaller than one window: a single, glob-aligned one
                extent[axis] = work[axis] = math.ceil(work[axis] / glob) * glob
        self.work, self.win_h, self.win_w = work, extent[0], extent[1]
        self.margin = int(window * margin) if isinstance(margin, float) else margin
        self.windows = grid_slice(work[0], work[1], self.win_h, self.win_w, self.margin)
        self.resampled = work != self.src

    def back_size(self, k):
        return int(self.src[0] * k), int(self.src[1] * k)


_TILE_KEYS = ("sample", "window", "glob", "margin", "progress", "batched")


def tile(sample=1, glob=1, window=1024, margin=0.1, astype="float32", progress=print, batched=False):
    """util.tile (util.py:291-348).  sample: float factor or (h, w) size; glob: images smaller than
    the window are grown to a multiple of it; window: tile size after resampling; margin: overlap
    between windows (float = fraction of the window, int = pixels).  Every knob can be overridden
    per call by keyword, as in the reference."""
    defaults = dict(sample=sample, glob=glob, window=window, margin=margin, progress=progress, batched=batched)

    def decorate(f):
        def run(image, *rest, **kw):
            opt = dict(defaults, **{k: kw.pop(k) for k in list(kw) if k in _TILE_KEYS})
            host_in = isinstance(image, numpy.ndarray)
            dev = hip.asarray(numpy.ascontiguousarray(image, dtype=numpy.float32)) if host_in else image
            _f32(dev)
            geo = _Tiling(dev.shape[0], dev.shape[1], opt["sample"], opt["glob"], opt["window"], opt["margin"])
            if geo.resampled:
                dev = resize(dev, geo.work)
            n = len(geo.windows)
            report = opt["progress"]
            if n > 1:
                report(1, n)
            if opt["batched"]:                                 # all windows through f as ONE batch
                outs = f(_stack([_window(dev, rc) for rc in geo.windows]), *rest, **kw)
                produce = lambda i: outs[i]
            else:
                produce = lambda i: f(_window(dev, geo.windows[i]), *rest, **kw)
            first = produce(0)
            k = first.shape[0] / geo.win_h                     # output pixels per input pixel
            if n == 1:
                result = resize(first, geo.back_size(k)) if geo.resampled else first
                return result.get() if host_in else result
            # blend buffers in HBM: weighted sum and weight total (util.py:327-344)
            oh, ow = int(dev.shape[0] * k), int(dev.shape[1] * k)
            chans = first.size // (first.shape[0] * first.shape[1])
            total = hip.zeros((oh, ow) + tuple(first.shape[2:]), ctx=dev.ctx)
            weight = hip.zeros((oh, ow), ctx=dev.ctx)
            ramp = int(geo.margin * k)
            for i, (rows, cols) in enumerate(geo.windows):
                if i:
                    report(i + 1, n)
                piece = first if i == 0 else produce(i)
                _lib.call("pl_tile_accumulate_f32", dev.ctx.handle, piece.ptr, total.ptr, weight.ptr, piece.shape[0],
                          piece.shape[1], chans, int(rows.start * k), int(cols.start * k), oh, ow, ramp)
            _lib.call("pl_tile_normalise_f32", dev.ctx.handle, total.ptr, weight.ptr, oh, ow, chans)
            result = resize(total, geo.back_size(k)) if geo.resampled else total
            return result.get() if host_in else result
        return run
    return decorate

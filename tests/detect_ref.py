"""Detections as net output: numpy mirrors of pl_yolo_decode_f32, pl_topk_f32's order and pl_nms_f32, and a
generator of head tensors whose decisions survive inexact sigmoids.  numpy only.

`decode64` is the contract in float64: for head h, float32 (N, A (5 + C), Gh, Gw), with t[j] = x[n, a (5 + C) + j, gy, gx],

    class = np.argmax(t[5:5 + C])              on the float32 logits: the first of equal maxima, the first NaN before any number
    score = s(t4) * s(t[5 + class])            s(v) = 1 / (1 + exp(-v));  candidate iff score > conf (a NaN score is none)
    cx = (s(t0) + gx) * sx,  cy = (s(t1) + gy) * sy,  w = exp(t2) * aw,  h = exp(t3) * ah
    box = (cx - w/2, cy - h/2, cx + w/2, cy + h/2)

anchor index = heads in declared order, then (a Gh + gy) Gw + gx.  conf, sx, sy, aw, ah are the float32 numbers the kernel gets.

Tolerances (per element, u = 2^-24, sp(v) = the float32 spacing at v: one rounding of a result near v is at most sp(v) / 2, and
sp(v) also covers a result that lands in the next binade).  The device computes s and exp within tests/ref64_ops.py's
ULP["sigmoid"] and ULP["exp"] units in the last place (`ulp_bound`), sigmoid with SIGMOID_FLOOR and exp with SUBNORMAL_FLOOR of
absolute error where the result runs out of exponent.  Write E(v) for those bounds.  Carried through the formulas:

    score = fl(a b), a = s(t4), b = s(t5+class):   |err| <= b E(a) + a E(b) + E(a) E(b) + sp(score)
    cx = fl(fl(s + g) k):  the sum is off by E(s) + sp(s + g), the product by that times k, + sp(cx)
    w = fl(e k), e = exp(t2):  E(e) k + sp(w);  w/2 is exact (+ SUBNORMAL_FLOOR where it is subnormal)
    x1 = fl(cx - w/2):  err(cx) + err(w) / 2 + sp(x1), and x2 likewise

A reference value whose float32 rounding is not finite (an exp that overflows, an infinite or NaN logit) has no tolerance: the
device must give that very infinity, or a NaN for a NaN.

`nms32` is pl_nms_f32 operation by operation in numpy float32 (each numpy float32 operation rounds once, and numpy never fuses
a multiply with an add), so the kernel must equal it bit for bit.  `topk_order` is pl_topk_f32's order for largest = 1, the
stable ascending sort read from its end: descending value, NaN first, equal values by DESCENDING position.  The decode kernel
stores an image's row back to front (anchor index i at position row - 1 - i), which makes that (score descending, anchor index
ascending); `chain32` puts the three together from given float32 scores, classes and boxes.

`plant` writes head tensors from wanted boxes, scores and classes by inverse sigmoid and log, everything else far below any
threshold.  Because the device's sigmoid is not numpy's, decisions can only be compared where they do not hang on the last
bits; `margins` checks exactly that on the float64 reference, with margin = MARGIN (64) times the tolerance involved:

  * no score lies within margin x its tolerance of conf;
  * no two candidates that follow each other in score order lie within margin x (the sum of their tolerances) of each other,
    unless their objectness and class logits are bit-equal (then the device computes the same float32 score for both: an exact
    tie, broken by index);
  * for no pair of candidates among the k that reach NMS does inter - iou union lie within margin x its box-derived tolerance
    of zero, unless the pair is disjoint by more than margin x the boxes' tolerance on one axis (inter is then exactly 0 on the
    device too, and 0 > iou union is false for the non-negative areas of planted boxes).  The tolerance of d = inter - iou union
    from boxes off by at most e per coordinate: iw and ih are off by 2e + sp each, widths and heights likewise, so
        |err d| <= (1 + iou) (iw 2e' + ih 2e' + 4e'^2) + iou (sum over both boxes of w 2e' + h 2e' + 4e'^2)
                   + 6 u (|inter| + area_i + area_j),      e' = e + sp(largest coordinate)
    (the last term: the float32 roundings of the products, the sums and iou union).

These are conditions on the inputs, not measurements of the kernel."""
import numpy as np

from tests import ref64_ops as R64

F32 = np.float32
U = 2.0 ** -24
MARGIN = 64.0


def _f64(a):
    return np.asarray(a, np.float64)


def sp(v):
    """The float32 spacing at v as float64 (0 where v's float32 rounding is not finite)."""
    r = np.abs(_f64(v).astype(F32))
    return np.spacing(np.where(np.isfinite(r), r, F32(0))).astype(np.float64)


def sigmoid64(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-_f64(v)))


def _e_sigmoid(s):
    return R64.ulp_bound(s, "sigmoid") + R64.SIGMOID_FLOOR


def _e_exp(e):
    return R64.ulp_bound(e, "exp") + R64.SUBNORMAL_FLOOR


def head_geometry(shapes, heads, classes, size=None):
    """[(A, Gh, Gw, sx, sy, offset, anchors float32 (A, 2))] and A_total, strides as the float32 the kernel gets."""
    rows, off = [], 0
    for shape, (anchors, stride) in zip(shapes, heads):
        anchors = np.asarray(anchors, np.float64).reshape(-1, 2).astype(F32)
        n, ch, gh, gw = shape
        assert ch == len(anchors) * (5 + classes), (shape, len(anchors), classes)
        if stride is None:
            stride = (size[1] / gw, size[0] / gh)
        sx, sy = (float(F32(s)) for s in np.broadcast_to(np.asarray(stride, np.float64), (2,)))
        rows.append((len(anchors), gh, gw, sx, sy, off, anchors))
        off += len(anchors) * gh * gw
    return rows, off


def decode64(xs, heads, classes, conf, size=None):
    """The contract in float64 on float32 head tensors `xs`.  Returns a dict of arrays over (N, A_total): score, tol_score
    (float64), cls (int64), cand (bool), key (the pair of logits the score is computed from, as uint32 bit patterns, (.., 2)),
    and box, tol_box over (N, A_total, 4)."""
    conf = float(F32(conf))
    rows, total = head_geometry([x.shape for x in xs], heads, classes, size)
    n = xs[0].shape[0]
    out = {"score": np.empty((n, total)), "tol_score": np.empty((n, total)), "cls": np.empty((n, total), np.int64),
           "box": np.empty((n, total, 4)), "tol_box": np.empty((n, total, 4)), "key": np.empty((n, total, 2), np.uint32)}
    with np.errstate(all="ignore"):
        for x, (a, gh, gw, sx, sy, off, anchors) in zip(xs, rows):
            x = np.asarray(x, F32).reshape(n, a, 5 + classes, gh, gw)
            cls = np.argmax(x[:, :, 5:], axis=2)                                   # numpy's rule on the float32 logits
            best = np.take_along_axis(x[:, :, 5:], cls[:, :, None], axis=2)[:, :, 0]
            sa, sb = sigmoid64(x[:, :, 4]), sigmoid64(best)
            ea, eb = _e_sigmoid(sa), _e_sigmoid(sb)
            score = sa * sb
            tol = sb * ea + sa * eb + ea * eb + sp(score)
            gx, gy = np.arange(gw, dtype=np.float64)[None, None, None, :], np.arange(gh, dtype=np.float64)[None, None, :, None]
            box, tolb = [None] * 4, [None] * 4
            for axis, (g, k, t, tw, an) in enumerate(((gx, sx, x[:, :, 0], x[:, :, 2], anchors[:, 0]),
                                                      (gy, sy, x[:, :, 1], x[:, :, 3], anchors[:, 1]))):
                s = sigmoid64(t)
                c = (s + g) * k
                ec = (_e_sigmoid(s) + sp(s + g)) * k + sp(c)
                e = np.exp(_f64(tw))
                an = _f64(an)[None, :, None, None]
                w = e * an
                eh = (_e_exp(e) * an + sp(w)) / 2 + R64.SUBNORMAL_FLOOR
                for j, v in ((axis, c - w / 2), (axis + 2, c + w / 2)):
                    box[j], tolb[j] = v, ec + eh + sp(v)
            sl = slice(off, off + a * gh * gw)
            out["score"][:, sl], out["tol_score"][:, sl] = score.reshape(n, -1), tol.reshape(n, -1)
            out["cls"][:, sl] = cls.reshape(n, -1)
            out["box"][:, sl] = np.stack(box, -1).reshape(n, -1, 4)
            out["tol_box"][:, sl] = np.stack(tolb, -1).reshape(n, -1, 4)
            out["key"][:, sl] = np.stack([x[:, :, 4], best], -1).reshape(n, -1, 2).view(np.uint32)
        out["cand"] = out["score"] > conf
    return out


def close(got, ref, tol):
    """Per element: |got - ref| <= tol where ref's float32 rounding is finite, else got is that very infinity / a NaN for a NaN."""
    got, ref = _f64(got), _f64(ref)
    with np.errstate(all="ignore"):
        r32 = ref.astype(F32).astype(np.float64)
        fin = np.isfinite(r32)
        return np.where(fin, np.abs(got - ref) <= tol, (got == r32) | (np.isnan(got) & np.isnan(r32)))


# ---- the float32 mirrors ----------------------------------------------------------------------------------------------------
def topk_order(scores, k):
    """pl_topk_f32 (largest = 1) on one row: (values, positions) of the k first by descending value, NaN first, equal values by
    descending position -- a stable ascending argsort read from its end."""
    scores = np.asarray(scores, F32)
    order = np.argsort(scores, kind="stable")[::-1][:k].astype(np.int64)
    return scores[order], order


def nms32(boxes, classes, sorted_scores, order, floor, iou, class_aware, max_det, entries=False):
    """pl_nms_f32 on one image: boxes (R, 4) float32, classes (R,) or None, sorted_scores / order (K,).  -> det (max_det, 6)
    float32, num; with `entries`, also the list of the kept entries' positions in sorted_scores."""
    boxes, sc, order = np.asarray(boxes, F32).reshape(-1, 4), np.asarray(sorted_scores, F32), np.asarray(order, np.int64)
    floor, iou, zero = F32(floor), F32(iou), F32(0)
    r, k = len(boxes), len(sc)
    det = np.zeros((max_det, 6), F32)
    with np.errstate(all="ignore"):
        alive = (sc > floor) & (order >= 0) & (order < r)
        at = np.where(alive, order, 0)
        b = boxes[at] if r else np.zeros((k, 4), F32)
        cls = np.asarray(classes, np.int32)[at] if classes is not None and r else np.zeros(k, np.int32)
        x1, y1, x2, y2 = (b[:, j] for j in range(4))
        area = (x2 - x1) * (y2 - y1)
        kept, which = 0, []
        for i in range(k):
            if kept == max_det:
                break
            if not alive[i]:
                continue
            det[kept] = (x1[i], y1[i], x2[i], y2[i], sc[i], F32(cls[i]))
            kept += 1
            which.append(i)
            iw = np.fmax(zero, np.fmin(x2[i], x2) - np.fmax(x1[i], x1))
            ih = np.fmax(zero, np.fmin(y2[i], y2) - np.fmax(y1[i], y1))
            inter = iw * ih
            union = (area[i] + area) - inter
            sup = inter > iou * union
            assert inter.dtype == F32 and union.dtype == F32
            if class_aware:
                sup &= cls == cls[i]
            sup[:i + 1] = False
            alive &= ~sup
    return (det, kept, which) if entries else (det, kept)


def chain32(scores, classes, boxes, conf, iou, class_aware, max_det, max_candidates, anchors=False):
    """What DetectionSpec.encode returns for float32 scores (N, A), classes, boxes (N, A, 4) given in ANCHOR order with -1 as a
    non-candidate's score: the row back to front, top-k, NMS with floor = conf.  -> det (N, max_det', 6), num (N,); with
    `anchors`, also the anchor index of every row of det (N, max_det'), -1 in unused rows."""
    scores = np.asarray(scores, F32)
    n, total = scores.shape
    k = min(max_candidates, total)
    md = min(max_det, k)
    det, num, idx = np.zeros((n, md, 6), F32), np.zeros(n, np.int32), np.full((n, md), -1, np.int64)
    for i in range(n):
        v, o = topk_order(scores[i, ::-1], k)
        det[i], num[i], which = nms32(np.asarray(boxes, F32)[i, ::-1], np.asarray(classes)[i, ::-1], v, o, F32(conf), iou,
                                      class_aware, md, entries=True)
        idx[i, :num[i]] = total - 1 - o[which]
    return (det, num, idx) if anchors else (det, num)


def expected(ref, conf, iou, class_aware, max_det, max_candidates):
    """What the device must return for heads whose `decode64` result is `ref`, given that `margins` finds nothing: det and num
    from the float32 roundings of the reference's scores and boxes, and per element of det the reference value and its tolerance
    (class and unused rows: tolerance 0).  -> det (float64), tol, num."""
    with np.errstate(all="ignore"):
        scores = np.where(ref["cand"], ref["score"], -1.0).astype(F32)
        det32, num, idx = chain32(scores, ref["cls"], ref["box"].astype(F32), conf, iou, class_aware, max_det, max_candidates, anchors=True)
    det, tol = det32.astype(np.float64), np.zeros(det32.shape)
    for n in range(len(num)):
        at = idx[n, :num[n]]
        det[n, :num[n], :4], tol[n, :num[n], :4] = ref["box"][n, at], ref["tol_box"][n, at]
        det[n, :num[n], 4], tol[n, :num[n], 4] = ref["score"][n, at], ref["tol_score"][n, at]
    return det, tol, num


# ---- planted heads ----------------------------------------------------------------------------------------------------------
def logit(p):
    p = _f64(p)
    return np.log(p) - np.log1p(-p)


def plant(shapes, heads, classes, items, size=None, background=-14.0, rng=None):
    """Head tensors of `shapes` with every objectness and class logit at `background` (scores around 1e-12) and small random box
    logits, then one anchor per item (n, h, a, gy, gx, score, cls, (x1, y1, x2, y2)): objectness and the logit of class `cls`
    both at logit(sqrt(score)), so the score is `score` up to rounding; the other class logits stay at `background`; the box
    logits by inverse sigmoid and log (the box's centre must lie inside its cell)."""
    rng = rng or np.random.default_rng(0)
    rows, _ = head_geometry(shapes, heads, classes, size)
    xs = []
    for shape in shapes:
        x = np.full(shape, background, F32).reshape(shape[0], -1, 5 + classes, shape[2], shape[3])
        x[:, :, :4] = rng.uniform(-1, 1, x[:, :, :4].shape)
        xs.append(x)
    for n, h, a, gy, gx, score, cls, (x1, y1, x2, y2) in items:
        _, gh, gw, sx, sy, _, anchors = rows[h]
        fx, fy = (x1 + x2) / 2 / sx - gx, (y1 + y2) / 2 / sy - gy
        assert 0 < fx < 1 and 0 < fy < 1, "the centre of %r is not inside cell (%d, %d) of head %d" % ((x1, y1, x2, y2), gy, gx, h)
        t = xs[h][n, a, :, gy, gx]
        t[5:] = background
        t[4] = t[5 + cls] = logit(np.sqrt(score))
        t[0], t[1] = logit(fx), logit(fy)
        with np.errstate(divide="ignore"):
            t[2], t[3] = np.log(_f64(x2 - x1) / anchors[a, 0]), np.log(_f64(y2 - y1) / anchors[a, 1])
    return [x.reshape(shape) for x, shape in zip(xs, shapes)]


def margins(ref, conf, iou=0.45, max_candidates=4096, class_aware=True, decode_only=False):
    """The conditions of the module docstring on a `decode64` result: a list of the violations found (empty: decisions are
    comparable), each a short string.  `decode_only`: the first condition alone, all that candidate membership hangs on."""
    conf, iou = float(F32(conf)), float(F32(iou))
    bad = []
    score, tol = ref["score"], ref["tol_score"]
    with np.errstate(all="ignore"):
        near = np.abs(score - conf) <= MARGIN * tol
    if near.any():
        bad.append("%d score(s) within the margin of conf, e.g. %r at %r" % (near.sum(), score[near][0], tuple(np.argwhere(near)[0])))
    for n in range(0 if decode_only else score.shape[0]):
        c = np.flatnonzero(ref["cand"][n])
        o = c[np.lexsort((c, -score[n, c]))]                                       # score descending, anchor index ascending
        gap, both = score[n, o[:-1]] - score[n, o[1:]], tol[n, o[:-1]] + tol[n, o[1:]]
        same = (ref["key"][n, o[:-1]] == ref["key"][n, o[1:]]).all(-1)
        tight = (gap <= MARGIN * both) & ~same
        if tight.any():
            bad.append("image %d: scores %r and %r are within the margin of each other" % (n, score[n, o[:-1]][tight][0], score[n, o[1:]][tight][0]))
        o = o[:max_candidates]
        b, e = ref["box"][n, o], ref["tol_box"][n, o].max(-1)
        if not np.isfinite(b).all():
            continue                                                               # (NaN / infinite boxes suppress by the float32 rules alone)
        e = e + sp(np.abs(b).max(-1))
        ee = np.maximum(e[:, None], e[None, :])
        lo, hi = np.maximum(b[:, None, :2], b[None, :, :2]), np.minimum(b[:, None, 2:], b[None, :, 2:])
        raw = hi - lo
        ext = np.maximum(raw, 0)
        inter = ext[..., 0] * ext[..., 1]
        wh = b[:, 2:] - b[:, :2]
        area = wh[:, 0] * wh[:, 1]
        ea = (np.abs(wh).sum(-1) * 2 * e + 4 * e * e)
        d = inter - iou * ((area[:, None] + area[None, :]) - inter)
        ed = ((1 + iou) * (ext.sum(-1) * 2 * ee + 4 * ee * ee) + iou * (ea[:, None] + ea[None, :])
              + 6 * U * (np.abs(inter) + np.abs(area)[:, None] + np.abs(area)[None, :]))
        apart = (raw < -MARGIN * 2 * ee[..., None]).any(-1) & (area >= 0)[:, None] & (area >= 0)[None, :]
        tight = (np.abs(d) <= MARGIN * ed) & ~apart & ~np.eye(len(o), dtype=bool)
        if class_aware:
            tight &= ref["cls"][n, o][:, None] == ref["cls"][n, o][None, :]
        if tight.any():
            i, j = np.argwhere(tight)[0]
            bad.append("image %d: inter - iou union = %.3g of entries %d and %d is within the margin %.3g" % (n, d[i, j], i, j, MARGIN * ed[i, j]))
    return bad

"""Detections as net output on a real MI355X (pl_yolo_decode_f32, pl_nms_f32, util.decode_detections, util.nms,
Net.detection_output).

The decode kernel is held to the float64 contract (tests/detect_ref.py `decode64`) within its derived bounds, with candidate
membership and classes exact wherever no score lies within the margin of conf -- asserted on the reference first.  The NMS
kernel is held to its float32 mirror `nms32` BIT FOR BIT.  Every output sits between runs of sentinel words that must survive,
and what a non-candidate must not write keeps the sentinel.  Then the chain and nets: every call form against the mirror
applied to the float heads a second, undeclared net instance returns."""
import ctypes

import numpy as np
import pytest

from tests import detect_ref as R
from tests import image_input_ref as RI
from tests.head_kit import EINVAL, EUNSUPPORTED, F32, OK, SENT, Framed, host as _host

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SPECIALS = np.array([NAN, INF, -INF, -0.0], F32)


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


# ---- pl_yolo_decode_f32 -----------------------------------------------------------------------------------------------------
def _logits(n, a, c, gh, gw, seed, step=0.5):
    """Head logits: seeded normals (sigma 2) quantised to multiples of `step`, so equal class logits are common; candidates
    forced at the cells where the box planes then get NaN, +-inf and -0.0; the same specials at the first, the last and a
    middle cell of the objectness and class planes."""
    rng = np.random.default_rng([seed, n, a, c, gh, gw])
    hw = gh * gw
    x = (np.round(rng.standard_normal((n, a, 5 + c, hw)) * 2 / step) * step).astype(F32)
    # the first, the last and a middle cell, shifted by the special's number and the plane's; the box planes' 4 cells further in
    spots = lambda p, j, d=0: [(d + (j + p) % 4) % hw, (hw - 1 - d - (j + p) % 4) % hw, (hw // 2 + d + (j + p) % 4) % hw]      # noqa: E731
    for p in range(4):
        for j, s in enumerate(SPECIALS):
            for pos in spots(p, j, 4):
                x[:, :, 4, pos], x[:, :, 5:, pos] = 2.0, -1.0
                x[:, :, 5 + min(1, c - 1), pos] = 2.5
    for p in range(4):
        for j, s in enumerate(SPECIALS):
            for pos in spots(p, j, 4):
                x[:, :, p, pos] = s
    for p in range(4, 5 + c):
        for j, s in enumerate(SPECIALS):
            for pos in spots(p, j):
                x[:, :, p, pos] = s
    return x.reshape(n, a * (5 + c), gh, gw)


def _decode(pa, x, anchors, stride, conf, classes, row=None, offset=0, raw=None, null=()):
    """pl_yolo_decode_f32 itself on float32 DeviceArray `x`.  `raw` overrides what the entry point is TOLD, `null` names pointer
    arguments passed as NULL.  -> status, (scores, classes, boxes) as Framed."""
    lib, ctx = pa._lib.load(), pa.hip.context()
    n, ch, gh, gw = x.shape
    a = len(anchors)
    row = a * gh * gw + offset if row is None else row
    arg = dict(n=n, a=a, c=classes, gh=gh, gw=gw, row=row, offset=offset)
    arg.update(raw or {})
    out = [Framed(pa, n * row), Framed(pa, n * row), Framed(pa, n * row * 4)]
    an = (ctypes.c_float * (2 * a))(*[float(v) for pair in anchors for v in pair])
    ptr = dict(x=x.ptr, anchors=an, scores=out[0].ptr, classes=out[1].ptr, boxes=out[2].ptr)
    ptr.update({k: None for k in null})
    sx, sy = (stride, stride) if np.isscalar(stride) else stride
    rc = lib.pl_yolo_decode_f32(ctx.handle, ptr["x"], arg["n"], arg["a"], arg["c"], arg["gh"], arg["gw"], ptr["anchors"], float(sx),
                                float(sy), float(conf), arg["row"], arg["offset"], ptr["scores"], ptr["classes"], ptr["boxes"])
    return rc, out


def _check_decode(pa, xs, heads, classes, conf, expect_some=True):
    """All heads of one image row decoded into the same framed outputs, against decode64."""
    ref = R.decode64(xs, heads, classes, conf)
    assert R.margins(ref, conf, decode_only=True) == []
    rows, total = R.head_geometry([x.shape for x in xs], heads, classes)
    n = xs[0].shape[0]
    lib, ctx = pa._lib.load(), pa.hip.context()
    out = [Framed(pa, n * total), Framed(pa, n * total), Framed(pa, n * total * 4)]
    dev = [pa.hip.asarray(x) for x in xs]
    for x, (anchors, stride), (a, gh, gw, sx, sy, off, _) in zip(dev, heads, rows):
        an = (ctypes.c_float * (2 * a))(*[float(v) for pair in anchors for v in pair])
        rc = lib.pl_yolo_decode_f32(ctx.handle, x.ptr, n, a, classes, gh, gw, an, sx, sy, float(conf), total, off,
                                    out[0].ptr, out[1].ptr, out[2].ptr)
        assert rc == OK
    (sc, ok0), (cl, ok1), (bx, ok2) = out[0].get(F32), out[1].get(np.int32), out[2].get(F32)
    assert ok0 and ok1 and ok2, "a sentinel run around an output was overwritten"
    # rows are stored back to front: position row - 1 - i holds anchor index i
    sc, cl, bx = sc.reshape(n, total)[:, ::-1], cl.reshape(n, total)[:, ::-1], bx.reshape(n, total, 4)[:, ::-1]
    cand = ref["cand"]
    print("decode %s: %d of %d candidates" % ([x.shape for x in xs], cand.sum(), cand.size))
    assert ((sc > F32(conf)) == cand).all(), "candidate membership"
    assert (sc[~cand] == F32(-1)).all() and not np.signbit(sc[cand]).any()
    assert (cl.view(np.uint32)[~cand] == SENT).all() and (bx.view(np.uint32)[~cand] == SENT).all(), "a non-candidate wrote its class or box"
    assert (cl[cand] == ref["cls"][cand]).all(), "classes"
    ok = R.close(sc[cand], ref["score"][cand], ref["tol_score"][cand])
    assert ok.all(), "scores: %d off, e.g. %r want %r" % ((~ok).sum(), sc[cand][~ok][:1], ref["score"][cand][~ok][:1])
    ok = R.close(bx[cand], ref["box"][cand], ref["tol_box"][cand])
    assert ok.all(), "boxes: %d off, e.g. %r want %r" % ((~ok).sum(), bx[cand][~ok][:1], ref["box"][cand][~ok][:1])
    assert bool(cand.any()) == expect_some
    return ref, bx


ANCHORS = [(10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198)]
# (N, A, C, Gh, Gw): one cell, small grids, YOLO-v3's coarsest head; 63, 64 and 65 cells per plane; 255, 256 and 257 (one workgroup and its neighbours)
DECODE_SHAPES = [(1, 1, 1, 1, 1), (2, 3, 3, 2, 3), (2, 3, 80, 13, 13), (1, 2, 5, 7, 9), (1, 1, 2, 7, 9), (1, 1, 2, 8, 8), (1, 1, 2, 5, 13),
                 (1, 1, 2, 15, 17), (1, 1, 2, 16, 16), (1, 1, 2, 1, 257), (2, 8, 4, 3, 5)]


@pytest.mark.parametrize("shape", DECODE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_decode_against_float64(pa, shape):
    n, a, c, gh, gw = shape
    x = _logits(n, a, c, gh, gw, 1)
    ref, bx = _check_decode(pa, [x], [(ANCHORS[:a], (8.0, 16.0))], c, 0.3, expect_some=gh * gw > 1)
    if gh * gw >= 32:
        cand = ref["cand"]
        assert np.isnan(bx[cand]).any() and np.isinf(bx[cand]).any()       # the specials in the box planes reached candidates
        t = x.reshape(n, a, 5 + c, -1)
        assert np.isnan(t[:, :, 4]).any() and not cand.reshape(n, a, -1)[np.isnan(t[:, :, 4])].any()
        if c >= 3:
            top = t[:, :, 5:].max(2)
            assert ((t[:, :, 5:] == top[:, :, None]).sum(2) > 1)[cand.reshape(n, a, -1)].any()       # equal class logits among candidates


def test_decode_zero_and_all_candidates(pa):
    x = _logits(2, 3, 3, 6, 7, 2)
    _check_decode(pa, [x], [(ANCHORS[:3], 8.0)], 3, 0.9995, expect_some=False)
    full = np.full((2, 2 * 7, 9, 30), 1.0, F32)                            # 270 cells: two workgroups per plane
    full[:, 4::7] = 8.0
    full[:, 5::7] = 6.0
    ref, _ = _check_decode(pa, [full], [(ANCHORS[:2], 4.0)], 2, 0.25)
    assert ref["cand"].all()


def test_decode_second_head_at_an_offset(pa):
    xs = [_logits(2, 3, 4, 4, 5, 3), _logits(2, 2, 4, 2, 3, 4), _logits(2, 1, 4, 9, 29, 5)]
    heads = [(ANCHORS[:3], 8.0), (ANCHORS[3:5], (16.0, 15.5)), (ANCHORS[5:6], 4.0)]
    _check_decode(pa, xs, heads, 4, 0.3)
    # one head alone into a longer row leaves the rest of the row untouched
    x = pa.hip.asarray(xs[1])
    rc, out = _decode(pa, x, ANCHORS[3:5], 16.0, 0.3, 4, row=12 + 7 + 5, offset=7)
    assert rc == OK
    sc, intact = out[0].get()
    sc = sc.reshape(2, 24)
    assert intact and (sc[:, :5] == SENT).all() and (sc[:, 17:] == SENT).all() and (sc[:, 5:17] != SENT).all()


def test_decode_refusals(pa):
    x = pa.hip.asarray(_logits(2, 2, 3, 4, 5, 6))
    an = ANCHORS[:2]
    cases = [(EINVAL, dict(null=("x",))), (EINVAL, dict(null=("anchors",))), (EINVAL, dict(null=("scores",))),
             (EINVAL, dict(null=("classes",))), (EINVAL, dict(null=("boxes",))),
             (EINVAL, dict(raw=dict(n=-1))), (EINVAL, dict(raw=dict(a=-1))), (EINVAL, dict(raw=dict(gh=-4))), (EINVAL, dict(raw=dict(gw=-5))),
             (EINVAL, dict(raw=dict(row=-1))), (EINVAL, dict(raw=dict(c=0))), (EINVAL, dict(raw=dict(c=-2))),
             (EINVAL, dict(raw=dict(offset=-1))), (EINVAL, dict(raw=dict(offset=1))), (EINVAL, dict(raw=dict(row=39))),
             (EINVAL, dict(raw=dict(gh=1 << 16, gw=1 << 16))),
             (EUNSUPPORTED, dict(raw=dict(a=9, row=180))),
             (EUNSUPPORTED, dict(raw=dict(n=1 << 15, a=1, c=(1 << 16) - 5, gh=1, gw=1, row=1))),       # 2^31 source floats
             (EUNSUPPORTED, dict(raw=dict(n=1 << 29, a=1, c=1, gh=1, gw=1, row=1))),                    # 2^31 box floats
             (OK, dict(raw=dict(n=0))), (OK, dict(raw=dict(a=0))), (OK, dict(raw=dict(gh=0, row=40)))]
    for want, kw in cases:
        rc, out = _decode(pa, x, an, 8.0, 0.3, 3, **kw)
        assert rc == want, (kw, rc)
        assert all(o.untouched() for o in out), kw
    rc, out = _decode(pa, x, an, 8.0, 0.3, 3)
    assert rc == OK and not out[0].untouched()


# ---- pl_nms_f32 -------------------------------------------------------------------------------------------------------------
def _nms(pa, boxes, classes, sorted_scores, order, floor, iou, class_aware, max_det, raw=None, null=()):
    """pl_nms_f32 itself on host arrays boxes (N, R, 4), classes (N, R) or None, sorted_scores / order (N, K).
    -> status, det Framed, num Framed."""
    lib, ctx = pa._lib.load(), pa.hip.context()
    n, r = boxes.shape[:2]
    k = sorted_scores.shape[1]
    arg = dict(n=n, r=r, k=k, max_det=max_det)
    arg.update(raw or {})
    dev = dict(boxes=pa.hip.asarray(np.ascontiguousarray(boxes, F32)), sorted=pa.hip.asarray(np.ascontiguousarray(sorted_scores, F32)),
               order=pa.hip.asarray(np.ascontiguousarray(order, np.int64)),
               classes=None if classes is None else pa.hip.asarray(np.ascontiguousarray(classes, np.int32)))
    det, num = Framed(pa, n * max_det * 6), Framed(pa, n)
    ptr = {key: (None if v is None else v.ptr) for key, v in dev.items()}
    ptr.update(det=det.ptr, num=num.ptr)
    ptr.update({key: None for key in null})
    rc = lib.pl_nms_f32(ctx.handle, ptr["boxes"], ptr["classes"], ptr["sorted"], ptr["order"], arg["n"], arg["r"], arg["k"],
                        float(floor), float(iou), int(class_aware), arg["max_det"], ptr["det"], ptr["num"])
    return rc, det, num


def _nms_check(pa, boxes, classes, sorted_scores, order, floor, iou, class_aware, max_det, what):
    rc, det, num = _nms(pa, boxes, classes, sorted_scores, order, floor, iou, class_aware, max_det)
    assert rc == OK, what
    (d, ok0), (m, ok1) = det.get(F32), num.get(np.int32)
    assert ok0 and ok1, "%s: a sentinel run around det or num was overwritten" % what
    n = len(boxes)
    d = d.reshape(n, max_det, 6)
    for i in range(n):
        copy = i > 0 and all(a is None or RI.same_bits(a[i], a[0]) for a in (boxes, classes, sorted_scores, order))
        if not copy:                                                         # (a copy of image 0 must give image 0's result)
            wd, wm = R.nms32(boxes[i], None if classes is None else classes[i], sorted_scores[i], order[i], floor, iou, class_aware, max_det)
        assert m[i] == wm, "%s: image %d kept %d, the mirror %d" % (what, i, m[i], wm)
        assert RI.same_bits(d[i], wd), "%s: image %d differs from the mirror" % (what, i)
    return d, m


def _random_boxes(k, seed, span):
    """R = k + 5 boxes with many overlaps, three classes, k sorted scores with ties, and an order that skips some rows."""
    rng = np.random.default_rng([seed, k])
    r = k + 5
    c = rng.uniform(0, span, (r, 2))
    wh = rng.uniform(4, 40, (r, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(F32)
    classes = rng.integers(0, 3, r).astype(np.int32)
    scores = np.sort(np.round(rng.uniform(0.05, 1, k), 3).astype(F32))[::-1]
    order = rng.permutation(r)[:k].astype(np.int64)
    return boxes, classes, np.ascontiguousarray(scores), order


def _two(a):
    """Image 1 a copy of image 0."""
    return np.stack([a, a])


@pytest.mark.parametrize("k", [1, 63, 64, 65, 256, 257, 1024, 4096])
def test_nms_bit_for_bit(pa, k):
    boxes, classes, scores, order = _random_boxes(k, 11, span=3 * np.sqrt(k))
    B, C, S, O = _two(boxes), _two(classes), _two(scores), _two(order)
    # candidate prefixes of 0, 1, K - 1 and K entries: the floor sits on a score, and the comparison is exclusive
    for m in sorted({0, 1, k - 1, k}):
        floor = INF if m == 0 else -INF if m == k else float(scores[m])
        if 0 < m < k and scores[m - 1] == scores[m]:
            floor = float(np.nextafter(scores[m - 1], F32(0)))               # a tie across the cut: take both sides of it
        for aware in (True, False):
            d, num = _nms_check(pa, B, C, S, O, floor, 0.45, aware, k, "k=%d prefix=%d aware=%d" % (k, m, aware))
            assert num[0] == num[1] and RI.same_bits(d[0], d[1]) and num[0] <= max(m, int((scores > floor).sum()))
            assert m > 0 or num[0] == 0
    kept = int(R.nms32(boxes, classes, scores, order, -INF, 0.45, True, k)[1])
    print("k = %d: %d kept" % (k, kept))
    assert kept >= min(k, 2) and (k < 64 or kept < k)
    for md in sorted({1, kept - 1, kept, kept + 1}):
        if 1 <= md <= k:
            d, num = _nms_check(pa, B, C, S, O, -INF, 0.45, True, md, "k=%d max_det=%d" % (k, md))
            assert num[0] == min(md, kept)
    # no classes: one class; a repeated run gives the same bits
    first = _nms_check(pa, B, None, S, O, -INF, 0.6, True, k, "k=%d no classes" % k)
    again = _nms_check(pa, B, None, S, O, -INF, 0.6, True, k, "k=%d no classes, again" % k)
    assert RI.same_bits(first[0], again[0]) and (first[1] == again[1]).all()
    # two different images in one batch do not see each other
    b2, c2, s2, o2 = _random_boxes(k, 12, span=3 * np.sqrt(k))
    _nms_check(pa, np.stack([boxes, b2]), np.stack([classes, c2]), np.stack([scores, s2]), np.stack([order, o2]), 0.2, 0.45, True, k,
               "k=%d two images" % k)


def test_nms_planted(pa):
    b = np.array([[0, 0, 10, 10], [3, 0, 13, 10], [6, 0, 16, 10],            # a chain: A drops B, B would have dropped C
                  [50, 50, 60, 60], [50, 50, 60, 60], [50, 50, 60, 60],      # duplicates
                  [5, 5, 5, 5], [5, 5, 5, 5], [2, 5, 8, 5],                   # points and a zero-height box inside A
                  [0, 0, NAN, 10], [NAN, NAN, NAN, NAN], [9, 9, 1, 1],       # NaN and inverted boxes
                  [-INF, 0, INF, 10], [0, 0, INF, INF], [1e30, 1e30, 3e38, 3e38], [0, 0, 1e-30, 1e-30]], F32)
    k = len(b)
    scores = np.linspace(0.95, 0.2, k).astype(F32)
    scores[4] = scores[3]                                                    # an exact tie among the duplicates
    for order in (np.arange(k), np.arange(k)[::-1].copy(), np.random.default_rng(5).permutation(k)):
        classes = np.zeros(k, np.int32)
        for aware, cl in ((True, classes), (False, classes), (True, (np.arange(k) % 2).astype(np.int32)), (True, None)):
            for iou in (0.45, 0.0, 1.0):
                _nms_check(pa, _two(b), None if cl is None else _two(cl), _two(scores), _two(order.astype(np.int64)), 0.0, iou, aware, k,
                           "planted order=%s aware=%s iou=%s" % (order[:3], aware, iou))
    d, num = _nms_check(pa, _two(b), None, _two(scores), _two(np.arange(k, dtype=np.int64)), 0.0, 0.45, False, k, "planted")
    kept = d[0, :num[0], :4]
    assert (kept[0] == b[0]).all() and (kept[1] == b[2]).all()               # A, then C: B is gone
    assert (kept == b[3]).all(1).sum() == 1                                  # one of the three duplicates
    assert (kept == b[6]).all(1).sum() == 2                                  # both points: a zero union suppresses nothing
    # entries that name no row, and NaN scores in front (where pl_topk_f32 puts them), are dead and never read
    order = np.array([[0, -1, 99, 3, 1 << 40, -(1 << 40)]], np.int64)
    sc = np.array([[NAN, 0.9, 0.8, 0.7, 0.6, 0.5]], F32)
    d, num = _nms_check(pa, b[None, :6], None, sc, order, 0.0, 0.45, False, 6, "dead entries")
    assert num[0] == 1 and (d[0, 0, :4] == b[3]).all()
    # K == 0: nothing to read, num is still written
    rc, det, num = _nms(pa, b[None], None, np.zeros((1, 0), F32), np.zeros((1, 0), np.int64), 0.0, 0.45, False, 0)
    assert rc == OK and num.get(np.int32)[0].tolist() == [0] and num.get()[1]


def test_nms_refusals(pa):
    boxes, classes, scores, order = _random_boxes(8, 13, 60)
    B, C, S, O = _two(boxes), _two(classes), _two(scores), _two(order)
    cases = [(EINVAL, dict(null=("boxes",))), (EINVAL, dict(null=("sorted",))), (EINVAL, dict(null=("order",))),
             (EINVAL, dict(null=("det",))), (EINVAL, dict(null=("num",))),
             (EINVAL, dict(raw=dict(n=-1))), (EINVAL, dict(raw=dict(r=-1))), (EINVAL, dict(raw=dict(k=-1))), (EINVAL, dict(raw=dict(max_det=-1))),
             (EINVAL, dict(raw=dict(k=14))), (EINVAL, dict(raw=dict(r=7))),
             (EUNSUPPORTED, dict(raw=dict(k=4097, r=5000))), (EUNSUPPORTED, dict(raw=dict(max_det=9))),
             (EUNSUPPORTED, dict(raw=dict(n=1 << 29, r=8))), (EUNSUPPORTED, dict(raw=dict(n=1 << 29, r=1, k=1, max_det=1))),
             (OK, dict(raw=dict(n=0)))]
    for want, kw in cases:
        rc, det, num = _nms(pa, B, C, S, O, 0.0, 0.45, True, 4, **kw)
        assert rc == want, (kw, rc)
        assert det.untouched() and num.untouched(), kw
    rc, det, num = _nms(pa, B, C, S, O, 0.0, 0.45, True, 4, null=("classes",))
    assert rc == OK and not det.untouched() and not num.untouched()


# ---- the chain --------------------------------------------------------------------------------------------------------------
def _compare(got, ref, conf, iou, class_aware, max_det, max_candidates, what):
    """(det, num) as host arrays against the mirror applied to a decode64 result whose margins hold."""
    det, num = got
    want, tol, wnum = R.expected(ref, conf, iou, class_aware, max_det, max_candidates)
    assert det.dtype == F32 and num.dtype == np.int32 and det.shape == want.shape and num.shape == wnum.shape, (what, det.shape, want.shape)
    assert (num == wnum).all(), "%s: num %s, the mirror %s" % (what, num, wnum)
    assert (det[:, :, 5] == want[:, :, 5]).all(), "%s: classes" % what
    ok = R.close(det, want, tol)
    assert ok.all(), "%s: %d elements off, e.g. %r want %r" % (what, (~ok).sum(), det[~ok][:1], want[~ok][:1])
    for i, m in enumerate(num):
        assert (det[i, m:].view(np.uint32) == 0).all(), "%s: unused rows are +0.0" % what
        assert (np.diff(det[i, :m, 4]) <= 0).all(), "%s: descending scores" % what


CHAIN_HEADS = [([(20, 24)], (4.0, 4.0)), ([(40, 30)], (16.0, 16.0)), ([(90, 110)], (8.0, 8.0))]


@pytest.mark.parametrize("last", [(1, 83), (1, 84), (2, 106)], ids=["16383", "16384", "16512"])
def test_chain_across_the_topk_lds_limit(pa, last):
    """Three heads of 16 000 + 300 + (83, 84, 212) anchors and max_candidates = 8: rows of 16 383 and 16 384 anchors are sorted
    in LDS, 16 512 takes pl_topk_f32's selection rounds.  Twelve planted candidates per image, so the four lowest are dropped;
    two pairs of exact ties, one of them across the cut, where the lower anchor index goes on."""
    shapes = [(2, 6, 125, 128), (2, 6, 15, 20), (2, 6) + last]
    total = 16000 + 300 + last[0] * last[1]
    box = lambda h, gy, gx, w, hh: (lambda s: ((gx + 0.5) * s - w / 2, (gy + 0.5) * s - hh / 2, (gx + 0.5) * s + w / 2,        # noqa: E731
                                               (gy + 0.5) * s + hh / 2))(CHAIN_HEADS[h][1][0])
    items = []
    for n in range(2):
        sc = [0.9, 0.85, 0.8, 0.8, 0.7, 0.65, 0.6, 0.55, 0.55, 0.5, 0.4, 0.3]
        # (head, gy, gx): head 0 first, so anchor indices rise along the list; 0.55 twice: entries 8 and 9 by rank, one is cut
        where = [(0, 3, 5 + n), (0, 3, 6 + n), (0, 60, 60), (0, 60, 70), (0, 124, 122), (1, 2, 3), (1, 2, 9), (1, 14, 19), (2, 0, 5),
                 (2, 0, 40), (2, last[0] - 1, last[1] - 1), (0, 90, 10)]
        for s, (h, gy, gx) in zip(sc, where):
            items.append((n, h, 0, gy, gx, s, 0, box(h, gy, gx, 20.0 + h, 9.0 + gx % 3)))
    xs = R.plant(shapes, CHAIN_HEADS, 1, items)
    ref = R.decode64(xs, CHAIN_HEADS, 1, 0.25)
    assert ref["cand"].sum() == 24 and ref["score"].shape == (2, total)
    assert R.margins(ref, 0.25, 0.45, 8) == []
    got = pa.util.decode_detections([pa.hip.asarray(x) for x in xs], CHAIN_HEADS, 1, conf=0.25, iou=0.45, max_det=100, max_candidates=8)
    det, num = got[0].get(), got[1].get()
    assert det.shape == (2, 8, 6)
    _compare((det, num), ref, 0.25, 0.45, True, 100, 8, "A_total = %d" % total)
    assert num.tolist() == [7, 7]                                            # 8 went in, the first drops its neighbour
    assert abs(det[0, 6, 4] - 0.55) < 1e-5 and abs(det[0, 1, 4] - 0.8) < 1e-5 and abs(det[0, 2, 4] - 0.8) < 1e-5
    assert det[0, 1, 0] < det[0, 2, 0]                                       # the tie: the lower anchor index first
    assert det[0, 6, 0] > 200                                                # the 0.55 that went on is head 1's, not head 2's


def test_chain_small(pa):
    from tests.test_detection_output import HEADS, ITEMS, SHAPES
    extra = [(0, 0, 1, 1, 2, 0.75, 1, (14.0, 9.0, 28.0, 21.0)), (0, 0, 0, 3, 0, 0.6, 1, (1.0, 25.0, 9.0, 31.0)),
             (0, 0, 1, 1, 3, 0.81, 0, (24.0, 9.0, 31.0, 21.0))]
    xs = R.plant(SHAPES, HEADS, 3, ITEMS + extra, size=(32, 32))
    ref = R.decode64(xs, HEADS, 3, 0.25, size=(32, 32))
    dev = [pa.hip.asarray(x) for x in xs]
    for kw in (dict(), dict(class_aware=False), dict(max_det=2), dict(max_candidates=3), dict(iou=0.9), dict(conf=0.7)):
        a = dict(conf=0.25, iou=0.45, max_det=100, max_candidates=1024, class_aware=True)
        a.update(kw)
        r = R.decode64(xs, HEADS, 3, a["conf"], size=(32, 32)) if "conf" in kw else ref
        assert R.margins(r, a["conf"], a["iou"], a["max_candidates"], a["class_aware"]) == []
        det, num = pa.util.decode_detections(dev, HEADS, 3, size=(32, 32), **a)
        k = min(a["max_candidates"], 40)                                     # max_candidates > A_total = 40: every anchor goes in
        assert det.shape == (2, min(a["max_det"], k), 6) and num.shape == (2,)
        _compare((det.get(), num.get()), r, a["conf"], a["iou"], a["class_aware"], a["max_det"], a["max_candidates"], str(kw))
    assert pa.util.decode_detections(dev, HEADS, 3, size=(32, 32))[1].get().tolist() == [5, 2]
    assert pa.util.decode_detections(dev, HEADS, 3, size=(32, 32), class_aware=False)[1].get().tolist() == [4, 2]
    # util.nms on its own: boxes and scores in any order, top-k in front
    boxes, classes, scores, _ = _random_boxes(300, 21, 300)
    scores = np.resize(scores, 305)                                          # one per box, unsorted where it wraps, with ties
    for cl in (None, classes[None]):
        det, num = pa.util.nms(pa.hip.asarray(boxes[None]), pa.hip.asarray(scores[None]), None if cl is None else pa.hip.asarray(cl),
                               iou=0.5, max_det=50, floor=0.1)
        v, o = R.topk_order(scores, 305)
        wd, wn = R.nms32(boxes, None if cl is None else cl[0], v, o, 0.1, 0.5, cl is not None, 50)
        assert det.shape == (1, 50, 6) and num.get().tolist() == [wn] and RI.same_bits(det.get()[0], wd)
    with pytest.raises(ValueError, match="float64"):
        pa.util.decode_detections([pa.hip.zeros(SHAPES[0], np.float64), dev[1]], HEADS, 3, size=(32, 32))
    with pytest.raises(ValueError, match="channels"):
        pa.util.decode_detections(dev, HEADS, 4, size=(32, 32))


# ---- nets -------------------------------------------------------------------------------------------------------------------
TINY_HEADS = [([(6, 8), (12, 10)], None), ([(14, 20), (24, 18)], None)]
TINY = dict(classes=3, conf=0.3, iou=0.45, max_det=30, size=(32, 32))


def tiny_two_head_net(seed=6):
    """x (N, 3, 32, 32) -> three stride-2 convs to 4 x 4, a fourth to 2 x 2; outputs: the 4 x 4 features (8 channels, no head),
    a head on them and a head on the 2 x 2 map, 2 anchors x (5 + 3) channels each."""
    from planer_amd.irgen.builder import GraphBuilder
    rng = np.random.default_rng(seed)
    g = GraphBuilder(["x"])
    src, cin = "x", 3
    for i, cout in enumerate((8, 8, 8, 12)):
        g.init("K%d" % i, (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (cin * 9))).astype(F32))
        g.init("B%d" % i, (rng.standard_normal(cout) * 0.1).astype(F32))
        g.op("conv", [src, "K%d" % i, "B%d" % i], "c%d" % i, name="conv%d" % i, group=1, strides=[2, 2], dilations=[1, 1], pads=[1, 1, 1, 1])
        src, cin = g.op("relu", "c%d" % i, "f%d" % i, name="relu%d" % i), cout
    for tag, feat, cin in (("h4", "f2", 8), ("h2", "f3", 12)):
        g.init(tag + "_w", (rng.standard_normal((16, cin, 1, 1)) * 1.5 / np.sqrt(cin)).astype(F32))
        g.init(tag + "_b", rng.standard_normal(16).astype(F32))
        g.op("conv", [feat, tag + "_w", tag + "_b"], tag, name=tag + "_conv", group=1, strides=[1, 1], dilations=[1, 1], pads=[0, 0, 0, 0])
    return g.finish(["f2", "h4", "h2"])


def tiny_input(seed=7):
    return (np.random.default_rng(seed).standard_normal((2, 3, 32, 32)) * 1.5).astype(F32)


def _tiny_ref(heads):
    ref = R.decode64(list(heads), TINY_HEADS, TINY["classes"], TINY["conf"], size=TINY["size"])
    return ref, R.margins(ref, TINY["conf"], TINY["iou"], 1024)


def _declare(net):
    return net.detection_output(TINY_HEADS, TINY["classes"], conf=TINY["conf"], iou=TINY["iou"], max_det=TINY["max_det"],
                                size=TINY["size"], indices=(1, 2))


@pytest.mark.parametrize("streams", [None, "pipe2"])
def test_tiny_net_every_call_form(pa, streams):
    g, b = tiny_two_head_net()
    x = tiny_input()
    net, plain = pa.from_graph(g, b), pa.from_graph(g, b)
    if streams:
        net.streams = plain.streams = streams
    feat, h4, h2 = plain(x)
    assert feat.shape == (2, 8, 4, 4) and h4.shape == (2, 16, 4, 4) and h2.shape == (2, 16, 2, 2)
    ref, bad = _tiny_ref((h4, h2))
    assert bad == [], bad                                                    # the margin conditions hold on the heads the device computed
    assert 6 <= ref["cand"].sum() <= 60, ref["cand"].sum()

    def check(y, what, on_device=False):
        assert isinstance(y, tuple) and len(y) == 3, what
        assert all(isinstance(v, pa.hip.DeviceArray if on_device else np.ndarray) for v in y), what
        f, det, num = _host(y)
        assert RI.same_bits(f, feat), what                                   # the output that is no head: untouched
        assert det.shape == (2, 30, 6)
        _compare((det, num), ref, TINY["conf"], TINY["iou"], True, TINY["max_det"], 1024, what)
        return det, num

    base = net(x)                                                            # nothing declared yet: a plan exists before the declaration
    assert len(base) == 3 and RI.same_bits(base[1], h4)
    before = dict(net._plans)
    assert _declare(net) is net
    det, num = check(net(x), "host")
    assert 3 <= num.sum() < ref["cand"].sum()                               # some kept, some suppressed
    check(net(pa.asarray(x)), "device", True)
    check(net({net.input[0]: x}), "dict")
    check(net.submit(x).get(), "submit")
    check(net.submit(pa.asarray(x)).result(), "submit device", True)
    pend = [net.submit(x) for _ in range(3)]                                 # several in flight
    for p in pend:
        check(p.get(), "submits in flight")
    net.compile(pa.asarray(x))
    check(net(pa.asarray(x)), "compile + replay", True)
    assert all(net._plans[key] is before[key] for key in before)             # the declaration touched no plan
    for got, want in zip(plain.submit(x).get(), (feat, h4, h2)):            # (the plain net's throughput plan: the same heads)
        assert RI.same_bits(got, want)
    assert sorted(net._plans, key=repr) == sorted(plain._plans, key=repr)
    # the eager routes
    for how in ("debug", "eager"):
        if how == "eager":
            net.use_graph = False
        d2, n2 = check(net(x, debug=True) if how == "debug" else net(x), how)
        assert RI.same_bits(d2, det) and (n2 == num).all(), how
    net.use_graph = True
    # float_output on one of its positions restores the old result
    assert net.float_output(2) is net
    for got, want in zip(net(x), (feat, h4, h2)):
        assert RI.same_bits(got, want)
    for got, want in zip(net.submit(x).get(), (feat, h4, h2)):
        assert RI.same_bits(got, want)
    # checks come before anything is launched: a wrong class count, positions the net does not have
    net.detection_output(TINY_HEADS, 4, size=TINY["size"], indices=(1, 2))
    for call in (lambda: net(x), lambda: net(pa.asarray(x)), lambda: net.submit(x), lambda: net(x, debug=True)):
        with pytest.raises(ValueError, match="channels"):
            call()
    net.detection_output(TINY_HEADS, 3, size=TINY["size"], indices=(1, 3))
    with pytest.raises(ValueError, match="returns 3"):
        net(x)
    pa.hip.trim_side_contexts()


def test_tiny_net_from_uint8(pa):
    g, b = tiny_two_head_net()
    net, plain = pa.from_graph(g, b), pa.from_graph(g, b)
    k, bb = pa.util.image_affine([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    _declare(net.image_input(k, bb))
    i = np.arange(2 * 32 * 32 * 3, dtype=np.int64)
    x = ((i * 37 + i // 3072 * 53 + 11) % 256).astype(np.uint8).reshape(2, 32, 32, 3)
    feat, h4, h2 = plain(RI.decode32(x, k, bb))
    ref, bad = _tiny_ref((h4, h2))
    assert bad == [], bad
    for what, y in (("host", net(x)), ("device", net(pa.asarray(x))), ("submit", net.submit(x).get()),
                    ("float in", net(RI.decode32(x, k, bb)))):
        f, det, num = _host(y)
        assert RI.same_bits(f, feat), what
        _compare((det, num), ref, TINY["conf"], TINY["iou"], True, TINY["max_det"], 1024, what)
    pa.hip.trim_side_contexts()


YOLO_ANCHORS = [(10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198), (373, 326)]


def test_yolov3_at_160(pa):
    """irgen/yolov3.py at 160, its heads scaled to logits of a few units (the random weights' own are in the hundreds: every
    score 0 or 1, nothing but ties).  Shapes and order always; the mirror where the margin conditions hold for these heads --
    on the CPU oracle's heads they do, with three times the margin: 35 candidates, 23 kept."""
    from planer_amd.irgen import yolov3
    g, b = yolov3.build(head_gain=1 / 768)
    x = yolov3.make_input(1, seed=2, size=160)
    net, plain = pa.from_graph(g, b), pa.from_graph(g, b)
    heads = [(YOLO_ANCHORS[6:], None), (YOLO_ANCHORS[3:6], None), (YOLO_ANCHORS[:3], None)]
    conf = 0.8
    net.detection_output(heads, 80, conf=conf, size=(160, 160))
    h = plain(x)
    assert [v.shape for v in h] == [(1, 255, 5, 5), (1, 255, 10, 10), (1, 255, 20, 20)]
    # Both nets run the same kernel for every conv: `net` takes the picks `plain` has just timed instead of timing its own (two
    # timings of near-equal candidates can differ, and the heads `net` decodes would not be, bit for bit, the heads the float64
    # mirror reads).
    net._load_algo_cache()
    net._algo.update(plain._algo)
    net._algo_tp.update(plain._algo_tp)
    y = net(x)
    convs = lambda n: [(a["layer"], a["kind"], a["w_layout"], a["plan"], a["x"]) for a in n.compile(pa.asarray(x)).algos]
    assert convs(plain) and convs(net) == convs(plain), [ab for ab in zip(convs(net), convs(plain)) if ab[0] != ab[1]][:3]
    assert isinstance(y, tuple) and len(y) == 2
    det, num = y
    assert det.shape == (1, 100, 6) and det.dtype == F32 and num.shape == (1,) and num.dtype == np.int32
    assert 0 <= num[0] <= 100 and (det[0, num[0]:].view(np.uint32) == 0).all()
    assert (np.diff(det[0, :num[0], 4]) <= 0).all() and (det[0, :num[0], 4] > conf).all()
    d2, n2 = net.submit(pa.asarray(x)).get()
    assert RI.same_bits(d2, det) and (n2 == num).all()
    ref = R.decode64(list(h), heads, 80, conf, size=(160, 160))
    print("yolov3 at 160: %d candidates, %d kept" % (ref["cand"].sum(), num[0]))
    bad = R.margins(ref, conf, 0.45, 1024)
    pa.hip.trim_side_contexts()
    if bad:
        pytest.skip("the margin conditions do not hold for these heads, no comparison with the mirror: %s" % bad[0])
    _compare((det, num), ref, conf, 0.45, True, 100, 1024, "yolov3 at 160")

"""Anchor-free heads and prototype masks on a real MI355X (pl_dfl_decode_f32, pl_nms_rows_f32, pl_dfl_coefficients_f32,
pl_proto_masks_f32, util.decode_detections and Net.detection_output with "dfl" heads and protos).

The decode is held to tests/dfl_ref.py's float64 mirror within its derived bound, classes and candidates exactly; pl_nms_rows_f32
to pl_nms_f32 and detect_ref.nms32 bit for bit; the masks to the exact float32 crop and, where the float64 sign binds, to that
sign.  Outputs sit between sentinels.  head_kit.check_every_call_form puts its head on a 3-channel output, fewer than a "dfl"
head can have (4 R + C >= 5), so the net test walks the same call forms on a net of its own."""
import numpy as np
import pytest

from tests import detect_ref as R
from tests import dfl_ref as D
from tests.head_kit import F32, OK, EINVAL, EUNSUPPORTED, SENT, Framed, framed_call, host, same

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
CONF, SIZE = 0.3, (64, 96)


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _head(n, r, c, md, gh, gw, seed, specials=False):
    """Logits in multiples of 1/4 (bin differences are exact in float32; no sigmoid of them is within 1e-4 of CONF)."""
    rng = np.random.default_rng([seed, r, c, gh, gw])
    x = (np.round(rng.standard_normal((n, 4 * r + c + md, gh * gw)) * 8) / 4).astype(F32)
    if specials:                                   # cells 0-2: the class planes; cells 3-5: candidates with such bins
        x[:, 4 * r, 0], x[:, 4 * r + c - 1, 1], x[:, 4 * r:4 * r + c, 2] = NAN, INF, -INF
        x[:, 4 * r, 3:6] = 6.0
        x[:, 0, 3], x[:, r, 4], x[:, 2 * r:3 * r, 5], x[:, 4 * r - 1, 5] = NAN, INF, -INF, -INF
    return x.reshape(n, -1, gh, gw)


@pytest.mark.parametrize("classes", [1, 5, 6, 22])          # 22: one chunk of 16 planes, one of 4, one plane more
@pytest.mark.parametrize("r", [4, 16])
@pytest.mark.parametrize("grid", [(5, 7), (17, 19)])
def test_decode_against_float64(pa, grid, r, classes):
    md = 4
    xs = [_head(2, r, classes, md, *grid, 1), _head(2, 2, classes, md, 3, 4, 2, specials=True)]
    heads = [(r, (8.0, 8.0)), (2, (16.0, 15.5))]
    ref = D.decode64(xs, heads, classes, md, CONF)
    assert not (np.abs(ref["score"] - float(F32(CONF))) < 1e-4).any()
    n, total = ref["score"].shape
    out = [Framed(pa, n * total), Framed(pa, n * total), Framed(pa, n * total * 4)]
    off = 0
    for x, (hr, (sx, sy)) in zip(xs, heads):
        gh, gw = x.shape[2:]
        assert pa._lib.load().pl_dfl_decode_f32(pa.hip.context().handle, pa.hip.asarray(x).ptr, n, hr, classes, md, gh, gw, sx, sy, CONF,
                                                total, off, out[0].ptr, out[1].ptr, out[2].ptr) == OK
        off += gh * gw
    (sc, ok0), (cl, ok1), (bx, ok2) = out[0].get(F32), out[1].get(np.int32), out[2].get(F32)
    assert ok0 and ok1 and ok2
    sc, cl, bx = sc.reshape(n, total)[:, ::-1], cl.reshape(n, total)[:, ::-1], bx.reshape(n, total, 4)[:, ::-1]   # back to front
    cand = ref["cand"]
    assert ((sc > F32(CONF)) == cand).all() and (sc[~cand] == F32(-1)).all() and cand.any() and not cand.all()
    assert (cl.view(np.uint32)[~cand] == SENT).all() and (bx.view(np.uint32)[~cand] == SENT).all()
    assert (cl[cand] == ref["cls"][cand]).all()
    fin = np.isfinite(ref["box"][cand])
    with np.errstate(all="ignore"):
        print("worst box error / bound: %.3f" % np.max((np.abs(bx[cand] - ref["box"][cand]) / ref["tol_box"][cand])[fin]))
    assert R.close(bx[cand], ref["box"][cand], ref["tol_box"][cand]).all()
    assert np.isnan(ref["box"][cand]).any()                                     # the special bins reached candidates


def _nms_inputs(k, seed=3):
    rng = np.random.default_rng([seed, k])
    c, wh = rng.uniform(0, 3 * np.sqrt(k) + 8, (2, k + 5, 2)), rng.uniform(4, 40, (2, k + 5, 2))    # two images
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 2).astype(F32)
    scores = np.sort(np.round(rng.uniform(0.05, 1, (2, k)), 2).astype(F32), axis=1)[:, ::-1]
    order = np.stack([rng.permutation(k + 5)[:k] for _ in range(2)]).astype(np.int64)
    return boxes, rng.integers(0, 3, (2, k + 5)).astype(np.int32), np.ascontiguousarray(scores), order


@pytest.mark.parametrize("max_det", [1, 17])
@pytest.mark.parametrize("k", [1, 65, 300])
def test_nms_rows(pa, k, max_det):
    md = min(max_det, k)
    boxes, classes, scores, order = _nms_inputs(k)
    lib, ctx, dev = pa._lib.load(), pa.hip.context(), [pa.hip.asarray(a) for a in (boxes, classes, scores, order)]
    args = (ctx.handle, dev[0].ptr, dev[1].ptr, dev[2].ptr, dev[3].ptr, 2, k + 5, k, 0.2, 0.45, 1, md)
    det, num, det2, num2, rows = Framed(pa, 2 * md * 6), Framed(pa, 2), Framed(pa, 2 * md * 6), Framed(pa, 2), Framed(pa, 2 * md)
    assert lib.pl_nms_f32(*args, det.ptr, num.ptr) == OK and lib.pl_nms_rows_f32(*args, det2.ptr, num2.ptr, rows.ptr) == OK
    assert lib.pl_nms_rows_f32(*args, det2.ptr, num2.ptr, None) == EINVAL
    got = [f.get(t) for f, t in ((det, F32), (num, np.int32), (det2, F32), (num2, np.int32), (rows, np.int32))]
    assert all(ok for _, ok in got)
    same((got[2][0], got[3][0]), (got[0][0], got[1][0]), ("det", "num"), "pl_nms_rows_f32 against pl_nms_f32")
    for i in range(2):
        wd, wn, which = R.nms32(boxes[i], classes[i], scores[i], order[i], 0.2, 0.45, True, md, entries=True)
        want = np.full(md, -1, np.int32)
        want[:wn] = order[i][which]
        same((got[2][0].reshape(2, md, 6)[i], got[4][0].reshape(2, md)[i]), (wd, want), ("det", "rows"), "image %d" % i)


def _mask_inputs(max_det, md, ph, pw, n=3, seed=5):
    """Images with 0, some and max_det rows; boxes in input pixels: random ones, an empty one, one over the whole plane, one
    hanging over every edge."""
    rng = np.random.default_rng([seed, max_det, md, ph, pw])
    c, wh = rng.uniform(0, (SIZE[1], SIZE[0]), (n, max_det, 2)), rng.uniform(2, 60, (n, max_det, 2))
    det = np.concatenate([c - wh / 2, c + wh / 2, rng.uniform(0.3, 1, (n, max_det, 2))], 2).astype(F32)
    for d, box in enumerate(([40, 20, 40, 50], [0, 0, SIZE[1], SIZE[0]], [-9, -9, SIZE[1] + 9, SIZE[0] + 9])[:max_det]):
        det[:, d, :4] = box
    num = np.array([0, (max_det + 1) // 2, max_det], np.int32)[:n]
    return det, num, rng.standard_normal((n, max_det, md)).astype(F32), rng.standard_normal((n, md, ph, pw)).astype(F32)


def _masks(pa, det, num, coef, protos, ptr=None, raw=None):
    n, max_det, md = coef.shape
    arg = dict(dict(max_det=max_det, md=md), **(raw or {}))
    dev = [pa.hip.asarray(a) for a in (det, num, coef, protos)]
    out = pa.hip.empty((n, max_det) + protos.shape[2:], np.uint8) if ptr is None else None
    rc = pa._lib.load().pl_proto_masks_f32(pa.hip.context().handle, *(a.ptr for a in dev), n, arg["max_det"], arg["md"], *protos.shape[2:],
                                           *SIZE, out.ptr if ptr is None else ptr)
    return rc, out


def _check_masks(got, det, num, coef, protos):
    inside, positive, decided = D.masks64(det, num, coef, protos, SIZE)
    assert (~decided & inside).sum() <= 1e-3 * max(1, inside.sum())
    assert got.dtype == np.uint8 and got.max(initial=0) <= 1 and not got[~inside].any()
    assert ((got == 1) == positive)[inside & decided].all()


@pytest.mark.parametrize("plane", [(5, 7), (16, 16), (13, 20)])
@pytest.mark.parametrize("md", [4, 32])
@pytest.mark.parametrize("max_det", [1, 16, 17, 100])
def test_masks(pa, max_det, md, plane):
    det, num, coef, protos = _mask_inputs(max_det, md, *plane)
    rc, out = _masks(pa, det, num, coef, protos)
    assert rc == OK
    _check_masks(out.get(), det, num, coef, protos)
    if max_det >= 16:
        assert out.get()[2].any() and not out.get()[0].any()


def test_masks_framed_and_refusals(pa):
    det, num, coef, protos = _mask_inputs(17, 8, 16, 16)
    for off in (0, 3):                                                           # 16-byte stores, and bytes at an odd address
        rc, got, intact = framed_call(pa, (3, 17, 16, 16), np.uint8, off, lambda p: _masks(pa, det, num, coef, protos, ptr=p)[0])
        assert rc == OK and intact
        _check_masks(got, det, num, coef, protos)
    for want, raw in ((EINVAL, dict(md=6)), (EINVAL, dict(md=0)), (EUNSUPPORTED, dict(md=68)), (EUNSUPPORTED, dict(max_det=129)),
                      (EINVAL, dict(max_det=-1))):
        rc, got, intact = framed_call(pa, (3, 17, 16, 16), np.uint8, 0, lambda p: _masks(pa, det, num, coef, protos, ptr=p, raw=raw)[0])
        assert rc == want and intact and (got == 0xA5).all(), raw


HEADS = [("dfl", 8, 4), ("dfl", None, 4)]


def _chain_inputs(seed=9):
    xs = [_head(2, 4, 3, 8, 8, 12, seed), _head(2, 4, 3, 8, 4, 6, seed + 1)]
    return xs, np.random.default_rng(seed).standard_normal((2, 8, 16, 24)).astype(F32)


def test_chain_equals_the_entries_composed_by_hand(pa):
    from planer_amd import layer
    xs, protos = _chain_inputs()
    dev, p = [pa.hip.asarray(x) for x in xs], pa.hip.asarray(protos)
    got = host(pa.util.decode_detections(dev, HEADS, 3, conf=CONF, max_det=20, max_candidates=64, size=SIZE, protos=p))
    lib, ctx, total, k, md = pa._lib, pa.hip.context(), 96 + 24, 64, 20
    scores, boxes, classes = pa.hip.empty((2, total)), pa.hip.empty((2, total, 4)), pa.hip.empty((2, total), np.int32)
    geo = [(8, 12, 8.0, 8.0, 0), (4, 6, 16.0, 16.0, 96)]
    for x, (gh, gw, sx, sy, off) in zip(dev, geo):
        lib.call("pl_dfl_decode_f32", ctx.handle, x.ptr, 2, 4, 3, 8, gh, gw, sx, sy, CONF, total, off, scores.ptr, classes.ptr, boxes.ptr)
    vals, idx = pa.hip.empty((2, k)), pa.hip.empty((2, k), np.int64)
    layer._topk_launch(ctx, scores.ptr, 2, total, 1, k, 1, vals, idx)
    det, num, rows = pa.hip.empty((2, md, 6)), pa.hip.empty((2,), np.int32), pa.hip.empty((2, md), np.int32)
    lib.call("pl_nms_rows_f32", ctx.handle, boxes.ptr, classes.ptr, vals.ptr, idx.ptr, 2, total, k, float(F32(CONF)), float(F32(0.45)), 1, md,
             det.ptr, num.ptr, rows.ptr)
    coef = Framed(pa, 2 * md * 8)
    for x, (gh, gw, sx, sy, off) in zip(dev, geo):
        lib.call("pl_dfl_coefficients_f32", ctx.handle, x.ptr, 2, 4, 3, 8, gh, gw, rows.ptr, num.ptr, total, off, md, coef.ptr)
    masks = pa.hip.empty((2, md, 16, 24), np.uint8)
    lib.call("pl_proto_masks_f32", ctx.handle, det.ptr, num.ptr, coef.ptr, p.ptr, 2, md, 8, 16, 24, *SIZE, masks.ptr)
    same(got, host((det, num, masks)), ("det", "num", "masks"), "decode_detections")
    c, intact = coef.get(F32, (2, md, 8))
    r, m = rows.get(), num.get()
    assert intact and 0 < m.min() and got[2].any()
    for n in range(2):                                                          # the coefficients are the kept cells' own
        cells = np.concatenate([x[n, 4 * 4 + 3:].reshape(8, -1) for x in xs], 1).T
        same((c[n],), (np.concatenate([cells[total - 1 - r[n, :m[n]]], np.zeros((md - m[n], 8), F32)]),), ("coef",), "image %d" % n)


def test_net_every_call_form(pa):
    """A conv net with two "dfl" heads and a prototype output, small-integer filters and inputs (exact sums, whichever kernels
    run): every call route returns f, det, num, masks, the chain's result on a second, undeclared instance's float outputs."""
    from planer_amd.irgen.builder import GraphBuilder
    rng = np.random.default_rng(4)
    g = GraphBuilder(["x"])
    for name, src, co, ci, stride in (("f", "x", 8, 3, 1), ("h0", "f", 27, 8, 2), ("p", "f", 8, 8, 1), ("h1", "f", 27, 8, 4)):
        g.init("K" + name, rng.integers(-1, 2, (co, ci, 3, 3)).astype(F32))
        g.init("B" + name, rng.integers(-2, 3, co).astype(F32))
        g.op("conv", [src, "K" + name, "B" + name], name, name="conv_" + name, group=1, strides=[stride] * 2, dilations=[1, 1], pads=[1] * 4)
    gb = g.finish(["f", "h0", "p", "h1"])
    x = np.repeat(np.repeat(rng.integers(-1, 2, (2, 3, 8, 8)).astype(F32), 4, 2), 4, 3)
    net, plain = pa.from_graph(*gb), pa.from_graph(*gb)
    f, h0, p, h1 = plain(x)
    kw = dict(conf=0.6, max_det=10, size=(32, 32))
    want = (f,) + host(pa.util.decode_detections([pa.asarray(h0), pa.asarray(h1)], HEADS, 3, protos=pa.asarray(p), **kw))
    assert want[2].min() > 0 and want[3].any()
    assert net.detection_output(HEADS, 3, indices=(1, 3), protos=2, **kw) is net
    names = ("f", "det", "num", "masks")
    same(host(net(x)), want, names, "host")
    same(host(net(pa.asarray(x))), want, names, "device")
    same(host(net({net.input[0]: x})), want, names, "dict")
    for pend in [net.submit(x) for _ in range(3)]:
        same(host(pend.get()), want, names, "submits in flight")
    net.compile(pa.asarray(x))
    for what in ("compile + replay", "replay again"):
        same(host(net(pa.asarray(x))), want, names, what)
    same(host(net(x, debug=True)), want, names, "debug")
    net.use_graph = False
    same(host(net(x)), want, names, "eager")
    net.use_graph = True
    with pytest.raises(ValueError, match="cannot be blended"):
        net.tiled(x[0].transpose(1, 2, 0))
    assert net.float_output(2) is net                                           # on the prototype position: the declaration goes
    same(host(net(x)), (f, h0, p, h1), ("f", "h0", "p", "h1"), "float_output")
    pa.hip.trim_side_contexts()

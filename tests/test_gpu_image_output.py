"""uint8 images and label maps as net output on a real MI355X (pl_image_f32_u8, pl_labels_f32_u8, util.encode_images,
util.label_map, Net.image_output / label_output / float_output).

Both kernels are held to their numpy mirrors (tests/image_output_ref.py) BIT FOR BIT: over the tile boundaries
(PL_IMAGE_OUT_TILE_PIXELS, read from the header), outputs that start 1 to 13 bytes into a block, sources that start 1 to 3 floats
into one, channel orders, both roundings and both layouts, with NaN, +-inf and -0.0 planted at the first, the last and a mid-tile
position of every plane; the output sits between two runs of 64 sentinel bytes that must survive.  Then nets: every call form
against the mirror of what a second net instance that declares nothing returns for the same call form."""
import ctypes

import numpy as np
import pytest

from tests import image_input_ref as RI
from tests import image_output_ref as R
from tests.head_kit import framed_call

pytestmark = pytest.mark.gpu

T, L = R.tile_constants()   # PL_IMAGE_OUT_TILE_PIXELS, PL_IMAGE_OUT_LANE_PIXELS
SENTINEL = 0xA5             # what framed_call fills the block around an output with
K4 = np.array([-0.75, 2.0 ** 20, 2.0 ** -20, 58.4], np.float32)
B4 = np.array([0.5, -3.0, 1e-3, 124.0], np.float32)
OK, EINVAL, EUNSUPPORTED = 0, 1, 2
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)

# (N, H, W, C): the small ones, a row one pixel longer than a tile, planes of T - 1, T and T + 1 pixels, two full tiles of the
# widest pixel, three tiles and a bit in one plane
SHAPES = [(1, 1, 1, 1), (2, 5, 7, 3), (1, 3, 4, 3), (2, 4, 6, 4), (1, 9, 13, 1), (1, 2, T + 1, 3), (2, 3, (T - 1) // 3, 3),
          (2, 32, T // 32, 3), (2, 5, (T + 1) // 5, 3), (1, 4, 512, 4), (2, 55, 59, 2)]
OFFSET_SHAPES = [(2, 5, 7, 3), (1, 2, T + 1, 3), (2, 3, (T - 1) // 3, 3), (1, 4, 512, 4), (1, 9, 13, 1)]
LABEL_PLANES = [(1, 1, 1), (2, 5, 7), (1, 2, T + 1), (2, 3, (T - 1) // 3), (2, 32, T // 32), (2, 5, (T + 1) // 5)]
assert T == 1024 and [s[1] * s[2] for s in SHAPES[6:9]] == [T - 1, T, T + 1]


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _id(shape):
    return "x".join(str(v) for v in shape)


def _plant(x):
    """NaN, +inf, -inf and -0.0 at the first, the last and a mid-tile position of every (n, c) plane, in place."""
    n, c, h, w = x.shape
    hw = h * w
    flat = x.reshape(n * c, hw)
    mid = min(hw - 1, T // 2 + 1)
    for j, s in enumerate(SPECIALS):
        for p in range(n * c):
            r = (j + p) % len(SPECIALS)
            for pos in (r, hw - 1 - r, mid + r):
                flat[p, pos % hw] = s
    return x


def _halves(shape_nhwc):
    """Half-integers from -3 to 262 cycled through the (N, C, H, W) tensor: every tie, both clamps, both sides of 255."""
    n, h, w, c = shape_nhwc
    vals = np.arange(-3, 262.5, 0.5, dtype=np.float32)
    x = vals[np.arange(n * c * h * w) % len(vals)].reshape(n, c, h, w).copy()
    return _plant(x)


def _normals(shape_nhwc, seed):
    n, h, w, c = shape_nhwc
    return _plant(np.random.default_rng(seed).standard_normal((n, c, h, w)).astype(np.float32))


def _scores(n, c, h, w, seed):
    """Seeded normals quantised to multiples of 0.5, so that ties are common, with the specials planted."""
    x = np.round(np.random.default_rng(seed).standard_normal((n, c, h, w)) * 2) / 2
    return _plant(x.astype(np.float32))


def _source(pa, host, off):
    """float32 `host` on the device, starting `off` floats into a larger block."""
    if not off:
        return pa.hip.asarray(host)
    flat = np.zeros(host.size + 4, np.float32)
    flat[off:off + host.size] = host.ravel()
    buf = pa.hip.asarray(flat)
    return pa.hip.DeviceArray(host.shape, np.float32, buf.ctx, buf.ptr + 4 * off, buf)


def _image(pa, x, k, b, layout, order=None, trunc=False, y_off=0, raw=None):
    """pl_image_f32_u8 itself on a float32 DeviceArray.  `raw` overrides what the entry point is TOLD (refusals)."""
    lib, ctx = pa._lib.load(), pa.hip.context()
    n, c, h, w = x.shape
    co = len(k)
    nbytes = n * co * h * w
    if raw:
        n, c, h, w, co = [raw.get(key, v) for key, v in zip("n c h w co".split(), (n, c, h, w, co))]
    ka, ba = (ctypes.c_float * len(k))(*[float(v) for v in k]), (ctypes.c_float * len(b))(*[float(v) for v in b])
    oa = None if order is None else (ctypes.c_int * len(order))(*order)
    return framed_call(pa, (nbytes,), np.uint8, y_off, lambda y: lib.pl_image_f32_u8(ctx.handle, x.ptr, y, n, c, h, w, co, oa,
                                                                                     int(layout == "nhwc"), ka, ba, int(trunc)))


def _labels(pa, x, threshold=0.0, y_off=0, raw=None):
    lib, ctx = pa._lib.load(), pa.hip.context()
    n, c, h, w = x.shape
    nbytes = n * h * w
    if raw:
        n, c, h, w = [raw.get(key, v) for key, v in zip("n c h w".split(), (n, c, h, w))]
    return framed_call(pa, (nbytes,), np.uint8, y_off, lambda y: lib.pl_labels_f32_u8(ctx.handle, x.ptr, y, n, c, h, w, float(threshold)))


def _same(got, want):
    want = np.asarray(want)
    return want.dtype == np.uint8 and got.size == want.size and bool((got.reshape(want.shape) == want).all())


# ---- the image kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_image_kernel_is_numpy_bit_for_bit(pa, shape, layout):
    c = shape[3]
    for x, k, b in ((_halves(shape), np.ones(c, np.float32), np.zeros(c, np.float32)),
                    (_normals(shape, sum(shape)), K4[:c], B4[:c])):
        dx = pa.hip.asarray(x)
        for trunc in (False, True):
            want = R.encode32(x, k, b, layout, trunc=trunc)
            rc, got, intact = _image(pa, dx, k, b, layout, trunc=trunc)
            assert rc == OK and intact
            assert _same(got, want), (trunc, int((got.reshape(want.shape) != want).sum()))
            y = pa.util.encode_images(dx, k, b, layout=layout, rounding="truncate" if trunc else "nearest")
            assert y.shape == want.shape and y.dtype == np.uint8 and (y.get() == want).all()
    if shape[1] * shape[2] * c >= 2 * 531:
        assert set(range(256)) <= set(R.encode32(_halves(shape), np.ones(c), np.zeros(c)).ravel().tolist())


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("shape", OFFSET_SHAPES, ids=_id)
def test_outputs_and_sources_that_start_anywhere(pa, shape, layout):
    c = shape[3]
    x = _normals(shape, 5)
    want = R.encode32(x, K4[:c], B4[:c], layout)
    dx = pa.hip.asarray(x)
    for y_off in (1, 2, 3, 7, 13):
        rc, got, intact = _image(pa, dx, K4[:c], B4[:c], layout, y_off=y_off)
        assert rc == OK and intact and _same(got, want), y_off
    for x_off in (1, 2, 3):
        rc, got, intact = _image(pa, _source(pa, x, x_off), K4[:c], B4[:c], layout, y_off=x_off + 4)
        assert rc == OK and intact and _same(got, want), x_off


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("c, order", [(3, (2, 1, 0)), (4, (0, 1, 2)), (4, (3,)), (1, (0, 0, 0)), (2, (1, 0, 1, 0)), (8, (7, 0))])
def test_channel_order(pa, c, order, layout):
    x = _normals((2, 6, 173, c), 11)                   # 1038 pixels: a second tile of 14
    k, b = K4[:len(order)], B4[:len(order)]
    want = R.encode32(x, k, b, layout, order)
    rc, got, intact = _image(pa, pa.hip.asarray(x), k, b, layout, order=order)
    assert rc == OK and intact and _same(got, want)
    assert (pa.util.encode_images(pa.hip.asarray(x), k, b, layout=layout, order=order).get() == want).all()


# ---- the label kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [2, 3, 5, 21, 256])
def test_label_kernel_is_numpy_argmax(pa, c):
    for n, h, w in LABEL_PLANES[:3] if c == 256 else LABEL_PLANES:
        x = _scores(n, c, h, w, c + h)
        want = np.argmax(x, axis=1)
        assert (R.labels(x) == want).all()
        rc, got, intact = _labels(pa, pa.hip.asarray(x))
        assert rc == OK and intact and _same(got, want.astype(np.uint8)), (n, h, w)
        y = pa.util.label_map(pa.hip.asarray(x))
        assert y.shape == (n, h, w) and y.dtype == np.uint8 and (y.get() == want).all()
    n, h, w = 2, 5, (T + 1) // 5
    for plane in (c - 1, 0):                            # the maximum in the last plane everywhere, then in the first
        x = _scores(n, c, h, w, 3)
        x[~np.isfinite(x)] = 0
        x[:, plane] = 9
        assert (np.argmax(x, axis=1) == plane).all()
        rc, got, intact = _labels(pa, pa.hip.asarray(x))
        assert rc == OK and intact and (got == plane).all()
    for y_off in (1, 2, 3, 7):
        x = _scores(n, c, h, w, y_off)
        rc, got, intact = _labels(pa, _source(pa, x, y_off % 4), y_off=y_off)
        assert rc == OK and intact and _same(got, R.labels(x)), y_off


@pytest.mark.parametrize("threshold", [0.0, 0.25])
def test_one_plane_is_a_threshold(pa, threshold):
    for n, h, w in LABEL_PLANES:
        x = _scores(n, 1, h, w, h)
        want = (x[:, 0] > threshold).astype(np.uint8)
        assert (R.labels(x, threshold) == want).all()
        for y_off in (0, 1, 2, 3, 7):
            rc, got, intact = _labels(pa, pa.hip.asarray(x), threshold, y_off=y_off)
            assert rc == OK and intact and _same(got, want), (n, h, w, y_off)
        assert (pa.util.label_map(pa.hip.asarray(x), threshold).get() == want).all()
    assert {0, 1} == set(R.labels(_scores(2, 1, 5, 7, 5), threshold).ravel().tolist())


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _last_error(pa):
    return pa._lib.load().pl_last_error()


def test_refusals_return_their_codes_and_leave_the_output_alone(pa):
    lib, ctx = pa._lib.load(), pa.hip.context()
    x = pa.hip.asarray(_normals((2, 6, 8, 3), 1))
    k3, b3 = K4[:3], B4[:3]
    big_src = (1 << 31) // (6 * 8 * 3) + 1             # the first batch size with 2^31 source floats
    big_out = (1 << 31) // (6 * 8 * 4) + 1             # four output channels: 2^31 output bytes from fewer source floats
    assert (big_src - 1) * 6 * 8 * 3 < 1 << 31 <= big_src * 6 * 8 * 3 and big_out * 6 * 8 * 3 < 1 << 31 <= big_out * 6 * 8 * 4
    cases = [
        ("five output channels", EUNSUPPORTED, dict(raw={"co": 5})),
        ("no output channel", EUNSUPPORTED, dict(raw={"co": 0})),
        ("no order and Co != C", EINVAL, dict(raw={"co": 2})),
        ("order names plane 3 of 3", EINVAL, dict(order=(0, 1, 3))),
        ("order names plane -1", EINVAL, dict(order=(0, -1, 2))),
        ("negative batch", EINVAL, dict(raw={"n": -1})),
        ("negative height", EINVAL, dict(raw={"h": -1})),
        ("no source plane", EINVAL, dict(raw={"c": 0}, order=(0, 0, 0))),
        ("2^31 source floats", EUNSUPPORTED, dict(raw={"n": big_src})),
        ("2^31 output bytes", EUNSUPPORTED, dict(raw={"n": big_out}, order=(0, 1, 2, 0), k=K4, b=B4)),
    ]
    for layout in ("nhwc", "nchw"):
        for what, code, kw in cases:
            kw = dict(kw)
            rc, body, intact = _image(pa, x, kw.pop("k", k3), kw.pop("b", b3), layout, **kw)
            assert rc == code, (what, rc)
            assert intact and (body == SENTINEL).all(), what
            assert _last_error(pa), what
    label_cases = [
        ("257 planes", EUNSUPPORTED, {"c": 257}),
        ("no plane", EINVAL, {"c": 0}),
        ("negative width", EINVAL, {"w": -1}),
        ("2^31 source floats", EUNSUPPORTED, {"n": big_src}),
    ]
    for what, code, raw in label_cases:
        rc, body, intact = _labels(pa, x, raw=raw)
        assert rc == code, (what, rc)
        assert intact and (body == SENTINEL).all() and _last_error(pa), what
    # null arguments
    ka, ba = (ctypes.c_float * 3)(*k3.tolist()), (ctypes.c_float * 3)(*b3.tolist())
    for args in ((None, x.ptr, x.ptr, ka, ba), (ctx.handle, None, x.ptr, ka, ba), (ctx.handle, x.ptr, None, ka, ba),
                 (ctx.handle, x.ptr, x.ptr, None, ba), (ctx.handle, x.ptr, x.ptr, ka, None)):
        h_, x_, y_, k_, b_ = args
        assert lib.pl_image_f32_u8(h_, x_, y_, 2, 3, 6, 8, 3, None, 1, k_, b_, 0) == EINVAL and _last_error(pa)
    for h_, x_, y_ in ((None, x.ptr, x.ptr), (ctx.handle, None, x.ptr), (ctx.handle, x.ptr, None)):
        assert lib.pl_labels_f32_u8(h_, x_, y_, 2, 3, 6, 8, 0.0) == EINVAL and _last_error(pa)
    assert (x.get().view(np.uint32) == _normals((2, 6, 8, 3), 1).view(np.uint32)).all()     # (x stood in for y above)
    # an empty batch, an empty plane: nothing to do
    for raw in ({"n": 0}, {"h": 0}, {"w": 0}):
        rc, body, intact = _image(pa, x, k3, b3, "nhwc", raw=raw)
        assert rc == OK and intact and (body == SENTINEL).all(), raw
        rc, body, intact = _labels(pa, x, raw=raw)
        assert rc == OK and intact and (body == SENTINEL).all(), raw
    assert pa.util.label_map(pa.hip.zeros((0, 3, 4, 4))).shape == (0, 4, 4)
    # the Python surface says the same before any call
    with pytest.raises(ValueError, match="float64"):
        pa.util.encode_images(pa.hip.zeros((1, 3, 4, 4), np.float64), k3, b3)
    with pytest.raises(ValueError, match=r"\(3, 4, 4\)"):
        pa.util.label_map(pa.hip.zeros((3, 4, 4)))
    with pytest.raises(ValueError, match="256"):
        pa.util.label_map(pa.hip.zeros((1, 257, 2, 2)))
    with pytest.raises(ValueError, match="does not have"):
        pa.util.encode_images(pa.hip.zeros((1, 3, 4, 4)), k3, b3, order=(0, 1, 3))


# ---- nets -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def picks():
    """Conv algorithm picks shared by every net of this module: a net times the candidates of a conv shape the shipped database
    does not have, and two nets could come to different picks for the same shape.  Shared, the picks are by shape alone."""
    return {}


def _net(pa, g, b, picks, streams=None):
    net = pa.from_graph(g, b)
    if streams:
        net.streams = streams
    net._load_algo_cache()
    picks.update({k: v for k, v in net._algo.items() if k not in picks})
    net._algo = picks
    return net


def _first(y):
    return y[0] if isinstance(y, tuple) else y


def _forms(pa, net, x):
    """name -> what each call form returns for host batch `x` (device results still on the device)."""
    return {"host": net(x), "device": net(pa.asarray(x)), "dict": net({net.input[0]: x}), "submit": net.submit(x).get(),
            "submit device": net.submit(pa.asarray(x)).result()}


def _check_forms(pa, net, plain, x, mirror, shape):
    got, want = _forms(pa, net, x), _forms(pa, plain, x)
    for name in got:
        y, w = _first(got[name]), _first(want[name])
        on_device = name in ("device", "submit device")
        assert isinstance(y, pa.hip.DeviceArray if on_device else np.ndarray), (name, type(y))
        assert isinstance(w, pa.hip.DeviceArray if on_device else np.ndarray), (name, type(w))
        y, w = (y.get(), w.get()) if on_device else (y, w)
        assert w.dtype == np.float32 and y.dtype == np.uint8 and y.shape == shape, (name, y.dtype, y.shape)
        assert (y == mirror(w)).all(), name


@pytest.mark.parametrize("streams", [None, "pipe2", "2x2"])
def test_fpn_label_output(pa, picks, streams):
    from planer_amd.irgen import fpn
    g, b = fpn.build()
    x = fpn.make_input(2, size=64)
    net, plain = _net(pa, g, b, picks, streams), _net(pa, g, b, picks, streams)
    want = plain(x)
    assert want.shape == (2, 21, 64, 64)
    base = net(x)                                      # nothing declared yet: float32, and the plans of a plain net
    assert RI.same_bits(base, want)
    before = dict(net._plans)
    assert net.label_output() is net
    assert list(net._plans) == list(before) and all(net._plans[key] is before[key] for key in before)
    _check_forms(pa, net, plain, x, R.labels, (2, 64, 64))
    assert all(net._plans[key] is before[key] for key in before)
    assert sorted(net._plans, key=repr) == sorted(plain._plans, key=repr)
    assert len(np.unique(R.labels(want))) > 2
    if streams:
        kinds = {type(p).__name__ for p in net._plans.values()}
        assert ("_PipelinePlan" if streams == "pipe2" else "_MultiPlan") in kinds, kinds
    # float32 again: the bits of the undeclared net
    assert net.float_output() is net
    assert RI.same_bits(net(x), want) and RI.same_bits(net.submit(x).get(), plain.submit(x).get())
    pa.hip.trim_side_contexts()


EDSR = dict(blocks=2, feats=8, size=12)


@pytest.mark.parametrize("streams", [None, "pipe2"])
@pytest.mark.parametrize("kw", [dict(layout="nhwc"), dict(layout="nchw", rounding="truncate", order=(2, 1, 0))],
                         ids=["nhwc", "nchw-truncate-bgr"])
def test_edsr_image_output(pa, picks, kw, streams):
    from planer_amd.irgen import edsr
    g, b = edsr.build(**EDSR)
    x = edsr.make_input(2, size=EDSR["size"])
    net, plain = _net(pa, g, b, picks, streams), _net(pa, g, b, picks, streams)
    k, bb = pa.util.image_affine_inverse(0, 1)
    net.image_output(k, bb, **kw)
    mirror = lambda w: R.encode32(w, k, bb, kw["layout"], kw.get("order"), kw.get("rounding") == "truncate")     # noqa: E731
    shape = (2, 48, 48, 3) if kw["layout"] == "nhwc" else (2, 3, 48, 48)
    _check_forms(pa, net, plain, x, mirror, shape)
    assert len(np.unique(mirror(plain(x)))) > 16
    # the eager routes encode what they computed: the bytes of the graph route
    want = net(x)
    for how in ("debug", "eager"):
        if how == "eager":
            net.use_graph = False
        got = net(x, debug=True) if how == "debug" else net(x)
        assert got.dtype == np.uint8 and (got == want).all(), how
        d = net(pa.asarray(x), debug=True) if how == "debug" else net(pa.asarray(x))
        assert isinstance(d, pa.hip.DeviceArray) and (d.get() == want).all(), how
    p = net.submit(x)                                  # no graph: the pass ran, the handle is finished
    assert (p.get() == want).all()
    pa.hip.trim_side_contexts()


def test_uint8_in_and_uint8_out(pa, picks):
    g, b = RI.rgba_net()
    net, plain = _net(pa, g, b, picks), _net(pa, g, b, picks)
    k, bb = pa.util.image_affine([0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.25])
    ko, bo = np.array([40, 90, 255], np.float32), np.array([10, -20, 0.5], np.float32)
    net.image_input(k, bb).image_output(ko, bo, order=(7, 0, 3))
    x = ((np.arange(2 * 6 * 10 * 4, dtype=np.int64) * 37 + 5) % 256).astype(np.uint8).reshape(2, 6, 10, 4)
    want = R.encode32(plain(RI.decode32(x, k, bb)), ko, bo, order=(7, 0, 3))
    assert want.shape == (2, 6, 10, 3) and len(np.unique(want)) > 16
    for name, y in _forms(pa, net, x).items():
        y = y.get() if isinstance(y, pa.hip.DeviceArray) else y
        assert y.dtype == np.uint8 and (y == want).all(), name
    pa.hip.trim_side_contexts()


def test_submits_in_flight_keep_their_own_batches(pa, picks):
    from planer_amd.irgen import fpn
    reps = 2
    g, b = fpn.build()
    net, plain = _net(pa, g, b, picks, "pipe%d" % reps), _net(pa, g, b, picks, "pipe%d" % reps)
    net.label_output()
    xs = [fpn.make_input(2, seed=10 + i, size=64) for i in range(2 * reps + 1)]
    want = [R.labels(plain.submit(x).get()) for x in xs]
    for form in (lambda x: x, pa.asarray):
        pend = [net.submit(form(x)) for x in xs]       # all in flight
        for i, (p, w) in enumerate(zip(pend, want)):
            y = p.get()
            assert y.dtype == np.uint8 and (y == w).all(), i
    assert (want[0] != want[1]).any()
    plan, = net._plans.values()
    assert len(plan.replicas) == reps
    pa.hip.trim_side_contexts()


def _two_outputs(seed=9):
    """conv 3x3 (3 -> 5) -> y0; relu, conv 1x1 (5 -> 3) -> y1: two outputs of different shapes."""
    from planer_amd.irgen.builder import GraphBuilder
    rng = np.random.default_rng(seed)
    g = GraphBuilder(["x"])
    g.init("K", (rng.standard_normal((5, 3, 3, 3)) * 0.3).astype(np.float32))
    g.init("B", rng.standard_normal(5).astype(np.float32))
    g.init("K2", (rng.standard_normal((3, 5, 1, 1)) * 0.5).astype(np.float32))
    g.op("conv", ["x", "K", "B"], "y0", name="conv", group=1, strides=[1, 1], dilations=[1, 1], pads=[1, 1, 1, 1])
    g.op("relu", "y0", "r", name="relu")
    g.op("conv", ["r", "K2"], "y1", name="head", group=1, strides=[1, 1], dilations=[1, 1], pads=[0, 0, 0, 0])
    return g.finish(["y0", "y1"])


def test_only_the_declared_output_of_two_changes(pa, picks):
    g, b = _two_outputs()
    net, plain = _net(pa, g, b, picks), _net(pa, g, b, picks)
    x = np.random.default_rng(2).standard_normal((2, 3, 9, 11)).astype(np.float32)
    w0, w1 = plain(x)
    assert w0.shape == (2, 5, 9, 11) and w1.shape == (2, 3, 9, 11)
    k, bb = np.float32([60, 60, 60]), np.float32([128, 128, 128])
    net.image_output(k, bb, index=1)
    for name, (y0, y1) in _forms(pa, net, x).items():
        y0, y1 = (y0.get(), y1.get()) if isinstance(y0, pa.hip.DeviceArray) else (y0, y1)
        assert y0.dtype == np.float32 and RI.same_bits(y0, w0), name
        assert y1.dtype == np.uint8 and (y1 == R.encode32(w1, k, bb)).all(), name
    net.label_output(index=1)                          # replaces
    assert (net(x)[1] == R.labels(w1)).all()
    net.label_output(index=2)                          # no such output
    with pytest.raises(ValueError, match="returns 2"):
        net(x)
    pa.hip.trim_side_contexts()


def test_a_declared_output_that_is_no_image_is_refused(pa, picks):
    from planer_amd.irgen import resnet18
    g, b = resnet18.build(classes=10)
    x = resnet18.make_input(2, size=32)
    net, plain = _net(pa, g, b, picks), _net(pa, g, b, picks)
    want = plain(x)
    assert want.shape == (2, 10)
    for declare in (lambda: net.label_output(), lambda: net.image_output(1.0, 0.0)):
        declare()
        for call in (lambda: net(x), lambda: net(pa.asarray(x)), lambda: net.submit(x), lambda: net(x, debug=True)):
            with pytest.raises(ValueError, match=r"\(2, 10\)"):
                call()
    net.float_output()
    assert RI.same_bits(net(x), want) and RI.same_bits(net.submit(x).get(), plain.submit(x).get())
    pa.hip.trim_side_contexts()


def test_under_pool_hygiene(pa, picks):
    """Every fresh block poisoned and guarded: the encoders' outputs and a declared net's -- guards intact, the bytes of the
    plain run."""
    from planer_amd.irgen import edsr
    ctx = pa.hip.context()
    g, b = edsr.build(**EDSR)
    x = edsr.make_input(2, size=EDSR["size"])
    net = _net(pa, g, b, picks)
    k, bb = pa.util.image_affine_inverse(0, 1)
    net.image_output(k, bb)
    img, sc = _normals((2, 5, (T + 1) // 5, 3), 7), _scores(2, 21, 5, (T + 1) // 5, 8)
    run = lambda: (net(x), net(pa.asarray(x)).get(), net.submit(x).get(),                                    # noqa: E731
                   pa.util.encode_images(_source(pa, img, 1), K4[:3], B4[:3]).get(),
                   pa.util.encode_images(pa.hip.asarray(img), K4[:3], B4[:3], layout="nchw", rounding="truncate").get(),
                   pa.util.label_map(_source(pa, sc, 3)).get())
    base = run()
    ctx.synchronize()
    ctx.pool_debug(pa.hip.POOL_GUARD_BYTES, 0xFF)
    try:
        got = run()
        dirty, report = ctx.pool_debug_check()
    finally:
        ctx.pool_debug(0)
    assert dirty == 0, report
    for y, w in zip(got, base):
        assert y.dtype == np.uint8 and (y == w).all()
    assert (got[3] == R.encode32(img, K4[:3], B4[:3])).all() and (got[5] == R.labels(sc)).all()
    pa.hip.trim_side_contexts()

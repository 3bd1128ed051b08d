"""uint8 image batches as net input on a real MI355X (pl_image_u8_nchw_f32, util.decode_images, Net.image_input).

The kernel without resize is held to fl(fl(x k) + b) in numpy BIT FOR BIT, for both source layouts, over the tile boundaries
(PL_IMAGE_U8_TILE_PIXELS, PL_IMAGE_U8_LANE_PIXELS), source views that start 1, 2 and 3 bytes into a buffer, an output that is
not 16-byte aligned, and channel orders; the output tensor sits between two runs of sentinel floats that must survive.  With
resize it is held to the float64 reference and the bound of tests/image_input_ref.py on every image of
tests/golden/image_input.npz, and whether its bits are the reference's is reported (run with -s).  Then three tiny nets, one per
feed route: uint8 batches, host and device, against the same net given the decoded float batch."""
import ctypes
import zlib

import numpy as np
import pytest

from oracle import planer_np as onp
from tests import image_input_ref as R
from tests.conftest import RTOL, assert_close
from tests.test_image_input import golden_cases

pytestmark = pytest.mark.gpu

T, L = 1024, 4              # PL_IMAGE_U8_TILE_PIXELS, PL_IMAGE_U8_LANE_PIXELS (tests/test_image_input.py holds them to the header)
PAD = 64                    # sentinel floats on either side of the output
SENTINEL = np.float32(-12345.5)
K4 = np.array([-0.75, 2.0 ** 20, 2.0 ** -20, 1 / (255 * 0.229)], np.float32)      # a negative k, 2^+-20, an ordinary one
B4 = np.array([0.5, -3.0, 1e-3, -2.1179], np.float32)
OK, EINVAL, EUNSUPPORTED = 0, 1, 2

# (N, H, W, C): the issue's five, a row one pixel longer than a tile, planes of T - 1, T and T + 1 pixels, two full tiles of the
# widest pixel, three tiles and a bit in one plane
SHAPES = [(1, 1, 1, 1), (2, 5, 7, 3), (1, 3, 4, 3), (2, 4, 6, 4), (1, 9, 13, 1), (1, 2, T + 1, 3), (2, 3, 341, 3), (2, 32, 32, 3),
          (2, 5, 205, 3), (1, 4, 512, 4), (2, 55, 59, 2)]


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _bytes(shape, seed):
    """Every byte value as soon as there are 256 elements (37 is coprime to 256); another seed, another batch."""
    n = int(np.prod(shape))
    return ((np.arange(n, dtype=np.int64) * 37 + seed * 101) % 256).astype(np.uint8).reshape(shape)


def _view(pa, host, off):
    """`host` (uint8) on the device, starting `off` bytes into a larger block."""
    buf = pa.hip.zeros((host.size + 16,), np.uint8)
    flat = np.zeros(host.size + 16, np.uint8)
    flat[off:off + host.size] = host.ravel()
    buf.set(flat)
    return pa.hip.DeviceArray(host.shape, np.uint8, buf.ctx, buf.ptr + off, buf)


def _call(pa, x, layout, k, b, order=None, size=None, y_off=0, tables=None, raw=None):
    """The entry point itself on a uint8 DeviceArray, the output framed by sentinels.  -> (status, output, frame intact)."""
    lib, ctx = pa._lib.load(), pa.hip.context()
    n, h, w, c = x.shape if layout == "nhwc" else (x.shape[0], x.shape[2], x.shape[3], x.shape[1])
    co = len(k)
    oh, ow = size or (h, w)
    out_n = n * co * oh * ow                           # the frame is cut for the true shapes ...
    if raw:                                            # ... `raw` then overrides what the entry point is TOLD (refusals)
        n, h, w, c, co, oh, ow = [raw.get(key, v) for key, v in zip("n h w c co oh ow".split(), (n, h, w, c, co, oh, ow))]
    frame = pa.hip.empty((PAD + out_n + PAD + y_off,))
    frame.set(np.full(frame.shape, SENTINEL, np.float32))
    if tables is None and size is not None:
        tables = [pa.hip.asarray(a) for pair in (pa.util._axis_samples(h, oh), pa.util._axis_samples(w, ow)) for a in pair]
    tp = [None if t is None else t.ptr for t in (tables or [None] * 4)]
    rc = lib.pl_image_u8_nchw_f32(ctx.handle, x.ptr, frame.ptr + 4 * (PAD + y_off), n, h, w, c, int(layout == "nhwc"), co,
                                  None if order is None else (ctypes.c_int * len(order))(*order), oh, ow, *tp,
                                  (ctypes.c_float * len(k))(*[float(v) for v in k]), (ctypes.c_float * len(b))(*[float(v) for v in b]))
    got = frame.get()
    body = got[PAD + y_off:PAD + y_off + out_n]
    intact = bool((got[:PAD + y_off] == SENTINEL).all() and (got[PAD + y_off + out_n:] == SENTINEL).all())
    return rc, body, intact


def _id(shape):
    return "x".join(str(v) for v in shape)


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_kernel_without_resize_is_numpy_bit_for_bit(pa, shape, layout):
    c = shape[3]
    host = _bytes(shape, zlib.crc32(repr(shape).encode()))
    if host.size >= 256:
        assert len(np.unique(host)) == 256
    if layout == "nchw":
        host = np.ascontiguousarray(host.transpose(0, 3, 1, 2))
    k, b = K4[:c], B4[:c]
    want = R.decode32(host, k, b, layout)
    rc, got, intact = _call(pa, pa.hip.asarray(host), layout, k, b)
    assert rc == OK and intact
    assert R.same_bits(got.reshape(want.shape), want)
    y = pa.util.decode_images(pa.hip.asarray(host), k, b, layout=layout)          # the Python surface: the same bits
    assert y.shape == want.shape and y.dtype == np.float32 and R.same_bits(y.get(), want)


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("off", [1, 2, 3, 7, 13])
@pytest.mark.parametrize("shape", [(2, 5, 7, 3), (1, 2, T + 1, 3), (2, 3, 341, 3), (1, 4, 512, 4), (1, 9, 13, 1)], ids=_id)
def test_source_views_that_start_at_any_byte(pa, shape, off, layout):
    host = _bytes(shape, off)
    if layout == "nchw":
        host = np.ascontiguousarray(host.transpose(0, 3, 1, 2))
    c = shape[3]
    want = R.decode32(host, K4[:c], B4[:c], layout)
    rc, got, intact = _call(pa, _view(pa, host, off), layout, K4[:c], B4[:c])
    assert rc == OK and intact and R.same_bits(got.reshape(want.shape), want)


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("shape", [(2, 32, 32, 3), (1, 2, T + 1, 3), (2, 4, 6, 4)], ids=_id)
def test_output_that_is_not_16_byte_aligned(pa, shape, layout):
    host = _bytes(shape, 3)
    if layout == "nchw":
        host = np.ascontiguousarray(host.transpose(0, 3, 1, 2))
    c = shape[3]
    want = R.decode32(host, K4[:c], B4[:c], layout)
    for y_off in (1, 2, 3):
        rc, got, intact = _call(pa, pa.hip.asarray(host), layout, K4[:c], B4[:c], y_off=y_off)
        assert rc == OK and intact and R.same_bits(got.reshape(want.shape), want)


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("c, order", [(3, (2, 1, 0)), (4, (0, 1, 2)), (4, (3,)), (1, (0, 0, 0)), (2, (1, 0, 1, 0))])
def test_channel_order(pa, c, order, layout):
    host = _bytes((2, 6, 173, c), 11)                  # 1038 pixels: a second tile of 14
    if layout == "nchw":
        host = np.ascontiguousarray(host.transpose(0, 3, 1, 2))
    k, b = K4[:len(order)], B4[:len(order)]
    want = R.decode32(host, k, b, layout, order)
    rc, got, intact = _call(pa, pa.hip.asarray(host), layout, k, b, order=order)
    assert rc == OK and intact and R.same_bits(got.reshape(want.shape), want)
    assert R.same_bits(pa.util.decode_images(pa.hip.asarray(host), k, b, layout=layout, order=order).get(), want)


@pytest.mark.parametrize("name", sorted(golden_cases()))
def test_kernel_with_resize_within_the_bound_of_float64(pa, name):
    img, size, out = golden_cases()[name]
    c = img.shape[2]
    batch = np.stack([img, img[::-1, ::-1].copy()])
    # the resize alone against the reference's own output
    y = pa.util.decode_images(pa.hip.asarray(batch), np.ones(c), np.zeros(c), size=size).get()
    y64, bound = R.decode64(batch, np.ones(c), np.zeros(c), size=size)
    bits = R.same_bits(y[0].transpose(1, 2, 0), out)
    print("%s: bits equal to the reference's util.resize: %s; worst err / bound %.3f" % (name, bits, R.worst(y, y64, bound)))
    assert R.worst(y, y64, bound) <= 1.0
    # (the reference's six roundings and the kernel's, each at most U 255; k = 1 and b = 0 add none)
    assert np.abs(y[0].transpose(1, 2, 0).astype(np.float64) - out).max() <= 12 * R.U * 255
    # with the affine part, a channel order, through the entry point with a framed output and a view as the source
    order = {1: (0,), 3: (2, 0, 1), 4: (2, 1, 0, 3)}[c]
    co = c if order is None else len(order)
    rc, got, intact = _call(pa, _view(pa, batch, 3), "nhwc", K4[:co], B4[:co], order=order, size=size)
    y64, bound = R.decode64(batch, K4[:co], B4[:co], order=order, size=size)
    q = R.worst(got.reshape(y64.shape), y64, bound)
    print("%s: affine, worst err / bound %.3f; bits equal to the float32 restatement: %s"
          % (name, q, R.same_bits(got.reshape(y64.shape), R.decode32(batch, K4[:co], B4[:co], order=order, size=size))))
    assert rc == OK and intact and q <= 1.0


def test_refusals_return_their_codes_and_leave_the_output_alone(pa):
    x = pa.hip.asarray(_bytes((2, 6, 8, 3), 1))
    xp = pa.hip.asarray(_bytes((2, 3, 6, 8), 1))
    tabs = [pa.hip.asarray(a) for pair in (pa.util._axis_samples(6, 6), pa.util._axis_samples(8, 8)) for a in pair]
    k3, b3 = K4[:3], B4[:3]
    big_src = (1 << 31) // (6 * 8 * 3) + 1             # the first batch size with 2^31 source bytes
    big_out = (1 << 31) // (6 * 8 * 4) + 1             # with four output channels: 2^31 output floats from fewer source bytes
    assert (big_src - 1) * 6 * 8 * 3 < 1 << 31 <= big_src * 6 * 8 * 3 and big_out * 6 * 8 * 3 < 1 << 31 <= big_out * 6 * 8 * 4
    cases = [
        ("five source channels", EUNSUPPORTED, dict(raw={"c": 5})),
        ("no source channel", EUNSUPPORTED, dict(raw={"c": 0})),
        ("five output channels", EUNSUPPORTED, dict(raw={"co": 5})),
        ("no output channel", EUNSUPPORTED, dict(raw={"co": 0})),
        ("tables with the planar layout", EUNSUPPORTED, dict(layout="nchw", tables=tabs)),
        ("tables and H = 1", EINVAL, dict(tables=tabs, raw={"h": 1})),
        ("tables and W = 1", EINVAL, dict(tables=tabs, raw={"w": 1})),
        ("three of four tables", EINVAL, dict(tables=tabs[:3] + [None])),
        ("another size without tables", EINVAL, dict(raw={"oh": 5})),
        ("no order and Co != C", EINVAL, dict(raw={"co": 2})),
        ("order names channel 3 of 3", EINVAL, dict(order=(0, 1, 3))),
        ("order names channel -1", EINVAL, dict(order=(0, -1, 2))),
        ("2^31 source bytes", EUNSUPPORTED, dict(raw={"n": big_src})),
        ("2^31 output floats", EUNSUPPORTED, dict(raw={"n": big_out}, order=(0, 1, 2, 0), k=K4, b=B4)),
        ("negative batch", EINVAL, dict(raw={"n": -1})),
    ]
    for what, code, kw in cases:
        layout = kw.pop("layout", "nhwc")
        rc, body, intact = _call(pa, xp if layout == "nchw" else x, layout, kw.pop("k", k3), kw.pop("b", b3), **kw)
        assert rc == code, (what, rc)
        assert intact and (body == SENTINEL).all(), what
    lib, ctx = pa._lib.load(), pa.hip.context()
    assert lib.pl_image_u8_nchw_f32(ctx.handle, x.ptr, None, 2, 6, 8, 3, 1, 3, None, 6, 8, None, None, None, None,
                                    (ctypes.c_float * 3)(), (ctypes.c_float * 3)()) == EINVAL
    assert lib.pl_image_u8_nchw_f32(ctx.handle, x.ptr, x.ptr, 2, 6, 8, 3, 1, 3, None, 6, 8, None, None, None, None, None, None) == EINVAL
    # the Python surface says the same before any call
    with pytest.raises(NotImplementedError):
        pa.util.decode_images(pa.hip.asarray(_bytes((1, 4, 4, 5), 0)), K4, B4, order=(0, 1, 2, 3))     # five source channels
    with pytest.raises(TypeError):
        pa.util.decode_images(pa.hip.zeros((1, 4, 4, 3)), k3, b3)                 # float32: not an image batch
    # an empty batch is nothing to do
    rc, body, intact = _call(pa, pa.hip.asarray(np.zeros((0, 6, 8, 3), np.uint8)), "nhwc", k3, b3)
    assert rc == OK and intact and body.size == 0


# ---- nets -----------------------------------------------------------------------------------------------------------------------
def _smallest_stem():
    """The smallest H x W pl_conv2d_stem_pool_nchw_supported accepts for a 3 -> 16 stem."""
    from planer_amd import _lib
    lib, ok, best = _lib.load(), ctypes.c_int(), None
    for h in range(1, 12):
        for w in range(1, 24):
            _lib.check(lib.pl_conv2d_stem_pool_nchw_supported(3, h, w, 16, 7, 7, 2, 2, 3, 3, ctypes.byref(ok)))
            if ok.value and (best is None or h * w < best[0] * best[1]):
                best = (h, w)
    return best


MEAN, STD = [0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.25]


def _nets(pa):
    """name -> (graph, blob, (N, H, W, C) of the uint8 batch, image_input arguments, route, force channel-quad plans)"""
    from planer_amd.irgen import customnet
    h, w = _smallest_stem()
    return {
        "stem": (R.stem_net(), (2, h, w, 3), dict(), "prefed", False),
        # (customnet's default plan keeps NCHW and copies the batch in; with channel-quad layout forced its conv is the row-packed
        #  one, the form whose packed image the feed writes)
        "custom": (customnet.build(), (2, 10, 14, 3), dict(order=(2, 1, 0)), "packed", True),
        "rgba": (R.rgba_net(), (2, 6, 10, 4), dict(), "neither", False),
    }


def _make(pa, name, declare=True, streams=None, **over):
    (g, b), shape, kw, route, force = _nets(pa)[name]
    net = pa.from_graph(g, b)
    if force:
        net.use_q4 = "force"
    if streams:
        net.streams = streams
    co = 3 if name != "rgba" else 4
    k, bb = pa.util.image_affine(MEAN[:co], STD[:co])
    kw = dict(kw, **over)
    if declare:
        net.image_input(k, bb, **kw)
    return net, g, b, shape, (k, bb, kw), route


def _out(y):
    y = y[0] if isinstance(y, tuple) else y
    return y.get() if hasattr(y, "get") else y


@pytest.mark.parametrize("name", ["stem", "custom", "rgba"])
def test_uint8_batches_run_the_plan_of_the_decoded_batch(pa, name):
    net, g, b, shape, (k, bb, kw), route = _make(pa, name)
    plain, *_ = _make(pa, name, declare=False)
    xs = [_bytes(shape, 20 + i) for i in range(3)]
    for i, x in enumerate(xs):
        xf = pa.util.decode_images(pa.asarray(x), k, bb, **kw)
        want = _out(net(xf))
        if i == 0:
            plan = net.compile(xf)
            s = plan.inputs[0]
            assert {"prefed": s.prefed is not None, "packed": s.packed is not None} == \
                {"prefed": route == "prefed", "packed": route == "packed"}, (route, plan.streams)
            ref = onp.OracleNet()
            ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
            ref.load_weights(b)
            assert_close(want, ref(R.decode32(x, k, bb, order=kw.get("order"))), RTOL, name + " against the oracle")
        assert R.same_bits(_out(net(x)), want), "host uint8, batch %d" % i
        assert R.same_bits(_out(net(pa.asarray(x))), want), "device uint8, batch %d" % i
        assert R.same_bits(_out(net({"x": x})), want), "dict input, batch %d" % i
        # float32 inputs are taken as before: the bits of a net that never heard of image_input
        assert R.same_bits(_out(net(xf.get())), _out(plain(xf.get()))), "float32 after image_input"
    assert R.same_bits(_out(net(pa.asarray(xs[0]))), _out(net(pa.util.decode_images(pa.asarray(xs[0]), k, bb, **kw))))
    assert len(net._plans) == 1, list(net._plans)                # one plan: the decoded signature's
    assert net.compile(pa.asarray(xs[0])) is net.compile(pa.util.decode_images(pa.asarray(xs[0]), k, bb, **kw))
    assert net.compile(xs[0]) is plan


@pytest.mark.parametrize("name", ["stem", "rgba"])
def test_submits_in_flight_keep_their_own_batches(pa, name):
    """2 R + 1 submits of different uint8 host batches on R replicas: every replica's upload buffer is reused, every result is
    its own batch's."""
    reps = 2
    net, g, b, shape, (k, bb, kw), route = _make(pa, name, streams="pipe%d" % reps)
    xs = [_bytes(shape, 40 + i) for i in range(2 * reps + 1)]
    want = [_out(net.submit(pa.util.decode_images(pa.asarray(x), k, bb, **kw)).result()) for x in xs]
    plans = dict(net._plans)
    assert len(plans) == 1 and len(next(iter(plans.values())).replicas) == reps
    for form in (lambda x: x, pa.asarray):
        pend = [net.submit(form(x)) for x in xs]                  # all in flight
        for i, (p, w) in enumerate(zip(pend, want)):
            assert R.same_bits(_out(p.get()), w), (form, i)
    assert net._plans == plans
    rp = next(iter(plans.values())).replicas[0]
    assert rp.host_in[0].dtype == np.uint8 and rp.host_in[0].shape == shape      # the upload buffer holds bytes, not floats
    ref = onp.OracleNet()
    ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
    ref.load_weights(b)
    assert_close(want[-1], ref(R.decode32(xs[-1], k, bb, order=kw.get("order"))), RTOL, name + " against the oracle")
    assert not R.same_bits(want[0], want[1])
    pa.hip.trim_side_contexts()


def test_a_resized_input(pa):
    h, w = _smallest_stem()
    net, g, b, shape, (k, bb, kw), route = _make(pa, "stem", streams="pipe2", size=(h, w))
    for src in ((2, 9, 11, 3), (2, 2, 2, 3), (2, h, w, 3)):       # down, up, and the net's own size (no resize)
        x = _bytes(src, 60)
        xf = pa.util.decode_images(pa.asarray(x), k, bb, size=(h, w))
        assert xf.shape == (2, 3, h, w)
        y64, bound = R.decode64(x, k, bb, size=None if src[1:3] == (h, w) else (h, w))
        assert R.worst(xf.get(), y64, bound) <= 1.0
        want = _out(net(xf))
        assert R.same_bits(_out(net(x)), want) and R.same_bits(_out(net(pa.asarray(x))), want)
        assert R.same_bits(_out(net.submit(x).get()), _out(net.submit(xf).result()))
    assert sorted(m for m, *_ in net._plans) == ["latency", "throughput"]         # one decoded signature, whatever the source size
    pa.hip.trim_side_contexts()


def test_uint8_without_image_input_is_refused_as_before(pa):
    net, g, b, shape, _, _ = _make(pa, "rgba", declare=False)
    x = _bytes(shape, 1)
    for form in (x, pa.asarray(x), np.ascontiguousarray(x.transpose(0, 3, 1, 2))):
        with pytest.raises(NotImplementedError, match="float32, got uint8"):
            net(form)
    with pytest.raises(NotImplementedError, match="float32, got uint8"):
        net.submit(x)
    # a declaration covers its own input only, and uint8 only
    two = pa.Net()
    two.input = ["a", "b"]
    two.image_input(K4[:3], B4[:3], key="b")
    assert two._image_spec(0) is None and two._image_spec(1) is not None
    # the eager routes decode into a fresh array
    net2, *_ = _make(pa, "rgba")
    net2.use_graph = False
    k, bb = pa.util.image_affine(MEAN, STD)
    assert R.same_bits(_out(net2(x)), _out(net2(R.decode32(x, k, bb))))


def test_under_pool_hygiene(pa):
    """Every fresh block poisoned and guarded: the decode's output, the uint8 upload, the net's outputs -- guards intact and the
    bits of the plain run."""
    ctx = pa.hip.context()
    net, g, b, shape, (k, bb, kw), route = _make(pa, "stem")
    x = _bytes(shape, 77)
    big = _bytes((2, 37, 29, 3), 78)
    base = _out(net(x))
    base_dec = pa.util.decode_images(_view(pa, big, 1), k, bb).get()
    base_res = pa.util.decode_images(pa.asarray(big), k, bb, size=(24, 40)).get()
    ctx.synchronize()
    ctx.pool_debug(pa.hip.POOL_GUARD_BYTES, 0xFF)
    try:
        y = _out(net(x))
        yd = _out(net(pa.asarray(x)))
        dec = pa.util.decode_images(_view(pa, big, 1), k, bb).get()
        res = pa.util.decode_images(pa.asarray(big), k, bb, size=(24, 40)).get()
        dirty, report = ctx.pool_debug_check()
    finally:
        ctx.pool_debug(0)
    assert dirty == 0, report
    assert R.same_bits(y, base) and R.same_bits(yd, base) and R.same_bits(dec, base_dec) and R.same_bits(res, base_res)
    assert R.same_bits(dec, R.decode32(big, k, bb))

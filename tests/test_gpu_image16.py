"""uint16 image batches and per-image percentile scaling as net input on a real MI355X (pl_image_u16_nchw_f32,
pl_image_norm_nchw_f32, util.decode_images, Net.image_input).

The decode is held to tests/image16_ref.py BIT FOR BIT: both sides select the same samples and round alike, so there is no
tolerance.  Then once against a plain float64 formula with np.percentile and a derived bound, and through a tiny net."""
import numpy as np
import pytest

from tests import head_kit, image16_ref as R16
from tests.image_input_ref import same_bits

pytestmark = pytest.mark.gpu

T, CHUNK = 1024, 4096         # PL_IMAGE_U8_TILE_PIXELS, PL_IMAGE_NORM_CHUNK_PIXELS
K4 = np.array([-0.75, 2.0 ** 12, 2.0 ** -12, 1 / 0.229], np.float32)
B4 = np.array([0.5, -3.0, 1e-3, -2.1179], np.float32)
PCTS = [(1, 99), (0, 100), (50, 50), (0.1, 99.9)]


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _out(y):
    y = y[0] if isinstance(y, tuple) else y
    return y.get() if hasattr(y, "get") else y


def _samples(shape, seed, dtype=np.uint16):
    """Uniform over the whole range, both extremes present in every batch of two samples or more."""
    x = np.random.default_rng(seed).integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)
    x.ravel()[:2] = [0, np.iinfo(dtype).max][:x.size]
    return x


def _view(pa, host, off):
    """`host` on the device, `off` bytes past a 16-byte boundary inside a block whose other bytes are all ones."""
    buf = pa.hip.empty((host.size * host.itemsize + 32,), np.uint8)
    assert buf.ptr % 16 == 0
    flat = np.full(buf.shape, 0xFF, np.uint8)
    flat[off:off + host.nbytes] = host.view(np.uint8).ravel()
    buf.set(flat)
    return pa.hip.DeviceArray(host.shape, host.dtype, buf.ctx, buf.ptr + off, buf)


def _check(pa, x, layout, order, pct, size=None, dev=None):
    """`x` is (N, H, W, C); decoded in `layout` with K4, B4: the mirror's bits."""
    co = x.shape[3] if order is None else len(order)
    if layout == "nchw":
        x = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    norm = None if pct is None else ("percentile",) + tuple(pct)
    want = R16.decode32(x, K4[:co], B4[:co], layout, order, size, norm)
    got = pa.util.decode_images(pa.hip.asarray(x) if dev is None else dev(x), K4[:co], B4[:co], layout=layout, size=size, order=order,
                                normalise=norm)
    assert got.shape == want.shape and got.dtype == np.float32
    assert same_bits(got.get(), want), np.flatnonzero(got.get().ravel().view(np.uint32) != want.ravel().view(np.uint32))[:4]


# plane sizes 1, 2, a tile - 1, a tile + 1, three chunks + 5 pixels (19 * 647), an odd W with three channels
SHAPES = [((2, 1, 1, 3), None), ((1, 1, 2, 1), (0, 0, 0)), ((2, 3, 341, 3), (2, 1, 0)), ((1, 25, 41, 4), (3, 0)),
          ((2, 19, 647, 2), (1, 0, 1, 0)), ((1, 19, 647, 1), None), ((2, 7, 13, 3), None), ((1, 5, 9, 4), (0, 1, 2))]
assert 19 * 647 == 3 * CHUNK + 5 and 3 * 341 == T - 1 and 25 * 41 == T + 1


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_shapes_orders_and_layouts(pa, case, layout):
    shape, order = SHAPES[case]
    _check(pa, _samples(shape, case), layout, order, PCTS[case % len(PCTS)])


@pytest.mark.parametrize("pct", PCTS)
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
def test_percentiles(pa, layout, pct):
    _check(pa, _samples((2, 70, 61, 3), 11), layout, None, pct)                    # 4270 pixels: a second chunk of 174


def _values(kind, m):
    rng = np.random.default_rng(5)
    half = np.arange(m) < m // 2
    return {"one high byte": lambda: 0x1200 + rng.integers(0, 256, m),
            "constant": lambda: np.full(m, 777),
            "two values": lambda: np.where(half, 100, 60000),                      # (50, 50) of an even count: on the step
            "neighbours in two buckets": lambda: np.where(half, 0x12FF, 0x1300),
            "twelve bits": lambda: rng.integers(0, 4096, m)}[kind]()


@pytest.mark.parametrize("pct", [(50, 50), (1, 99)])
@pytest.mark.parametrize("kind", ["one high byte", "constant", "two values", "neighbours in two buckets", "twelve bits"])
def test_values(pa, kind, pct):
    n, h, w, c = 2, 70, 61, 2
    assert (h * w) % 2 == 0
    x = np.stack([np.random.default_rng(i).permutation(_values(kind, h * w)) for i in range(n * c)])
    x = np.ascontiguousarray(x.reshape(n, c, h, w).transpose(0, 2, 3, 1)).astype(np.uint16)
    for layout in ("nhwc", "nchw"):
        _check(pa, x, layout, (1, 0), pct)


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("shape", [(2, 7, 13, 3), (1, 66, 64, 4)])
def test_a_uint8_batch_with_normalise(pa, shape, layout):
    _check(pa, _samples(shape, 3, np.uint8), layout, None, (1, 99))


@pytest.mark.parametrize("pct", [None, (1, 99)])
@pytest.mark.parametrize("off", [2, 6, 14])
@pytest.mark.parametrize("shape", [(2, 7, 13, 3), (1, 19, 647, 1)])
def test_views_at_even_addresses_read_nothing_outside(pa, shape, off, pct):
    for layout in ("nhwc", "nchw"):
        _check(pa, _samples(shape, off) // 2, layout, None, pct, dev=lambda x: _view(pa, x, off))      # (no sample is 0xFFFF)


@pytest.mark.parametrize("size", [(5, 7), (18, 23)])
def test_resized_with_the_percentiles_of_the_source(pa, size):
    _check(pa, _samples((2, 9, 11, 3), 8), "nhwc", (2, 0, 1), (1, 99), size=size)
    _check(pa, _samples((2, 9, 11, 3), 8), "nhwc", (2, 0, 1), None, size=size)


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 5, 7, 3), (1, 2, T + 1, 3), (2, 4, 512, 4)])
def test_uint16_without_normalise(pa, shape, layout):
    x = _samples(shape, 2)
    _check(pa, x, layout, None, None)
    k, b = pa.util.image_affine([0.485, 0.456, 0.406, 0.5][:shape[3]], [0.229, 0.224, 0.225, 0.25][:shape[3]], scale=65535)
    xs = x if layout == "nhwc" else np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    assert same_bits(pa.util.decode_images(pa.hip.asarray(xs), k, b, layout=layout).get(), R16.decode32(xs, k, b, layout))


@pytest.mark.parametrize("pct", [(1, 99), (0.1, 99.9)])
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
def test_within_the_bound_of_a_plain_float64_formula(pa, layout, pct):
    """y = fl(fl(r kk) + bb) with kk = K (1 + e1), bb = B (1 + e2), the product (1 + e3), the sum (1 + e4), every |e| <= U = 2^-24:
    y - (r K + B) = r K (e1 + e3 + e1 e3) + B e2 + e4 (r K (1 + e1)(1 + e3) + B (1 + e2)), so
    |err| <= (1 + U) U ((2 + U) |r K| + |B|) + U |y|: the issue's first-order 2^-24 (2 |r K| + |B| + |y|) with its second-order terms
    kept.  K and B here come from np.percentile and the unfolded formula, a few float64 roundings from the kernel's: 2^-50 of the
    same magnitudes allows for them."""
    x = _samples((2, 70, 61, 3), 21)
    xs = x if layout == "nhwc" else np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    k, b = K4[:3].astype(np.float64)[None, :, None, None], B4[:3].astype(np.float64)[None, :, None, None]
    r = x.transpose(0, 3, 1, 2).astype(np.float64)
    p_lo, p_hi = (np.percentile(r, q, axis=(2, 3), keepdims=True) for q in pct)
    y64 = (r - p_lo) / (p_hi - p_lo) * k + b
    K = k / (p_hi - p_lo)
    B = b - p_lo * K
    U = 2.0 ** -24
    bound = (1 + U) * U * ((2 + U) * np.abs(r * K) + np.abs(B)) + U * np.abs(y64) + 2.0 ** -50 * (np.abs(r * K) + np.abs(B) + np.abs(y64))
    got = pa.util.decode_images(pa.hip.asarray(xs), K4[:3], B4[:3], layout=layout, normalise=("percentile",) + pct).get()
    worst = float((np.abs(got.astype(np.float64) - y64) / bound).max())
    print("worst |err| / bound: %.3f" % worst)
    assert worst <= 1.0


def test_through_a_net(pa):
    """Different host batches through net(x) twice, then through submit: a histogram or an affine table left over from the call
    before would show in the next.  Then the refusals, after which the net answers as before."""
    g, b = head_kit.tiny_net(["s"])
    net = pa.from_graph(g, b)
    norm = ("percentile", 1, 99)
    net.image_input(np.ones(3, np.float32), np.zeros(3, np.float32), normalise=norm)
    xs = [_samples((2, 32, 32, 3), 30 + i) >> i for i in range(4)]               # (other ranges: other percentiles)
    want = [_out(net(R16.decode32(x, np.ones(3), np.zeros(3), normalise=norm))) for x in xs]
    assert not same_bits(want[0], want[1])
    for x, w in zip(xs[:2], want[:2]):
        assert same_bits(_out(net(x)), w)
    assert same_bits(_out(net(pa.hip.asarray(xs[2]))), want[2])
    pend = [net.submit(x) for x in xs]                                           # all in flight
    for p, w in zip(pend, want):
        assert same_bits(_out(p.get()), w)
    from planer_amd import _lib, export
    with pytest.raises(NotImplementedError, match="uint16"):
        export.export_plan(net, xs[0])
    assert _lib._recorder is None and pa.hip._free_hook is None
    with pytest.raises(NotImplementedError, match="uint16"):
        net.tiled(xs[0][0], window=16)
    with pytest.raises(TypeError, match="int16"):
        net(xs[0].astype(np.int16))
    assert same_bits(_out(net(xs[1])), want[1])
    pa.hip.trim_side_contexts()


def test_under_pool_hygiene(pa):
    """Fresh blocks poisoned and guarded: the counters are cleared by the call, not by the pool."""
    ctx = pa.hip.context()
    x = _samples((2, 70, 61, 3), 41)
    ctx.synchronize()
    ctx.pool_debug(pa.hip.POOL_GUARD_BYTES, 0xFF)
    try:
        for pct in ((1, 99), (50, 50)):
            _check(pa, x, "nhwc", None, pct)
            _check(pa, x, "nhwc", (2, 1, 0), pct, size=(35, 30))
        dirty, report = ctx.pool_debug_check()
    finally:
        ctx.pool_debug(0)
    assert dirty == 0, report

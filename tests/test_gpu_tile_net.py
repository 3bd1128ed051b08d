"""Net.tiled on a real MI355X (pl_tile_windows_*_nchw_f32, pl_tile_blend_*, util.cut_windows, util.blend_windows).

Everything here is exact by construction, so every comparison is on bits (tests/tile_net_ref.py `canonical`: float32 as uint32,
every NaN as one pattern -- which NaN an operation returns is the one thing IEEE 754 leaves open).  The kernels alone are held
to their numpy mirrors on the geometries of tests/tile_net_ref.py CASES, inputs and outputs inside larger buffers whose other
bytes must survive; then Net.tiled end to end on a net whose arithmetic is exact (small-integer filters on integer inputs),
against the mirrors around the oracle's conv; against util.tile(batched=True) around the same net; and the plan count."""
import ctypes

import numpy as np
import pytest

from tests import tile_net_ref as T
from tests.head_kit import framed_call

pytestmark = pytest.mark.gpu

PAD = 64                     # sentinel elements on either side of an input
SENT8 = 0xA5
K4 = np.array([-0.75, 2.0 ** 20, 2.0 ** -20, 58.4], np.float32)
B4 = np.array([0.5, -3.0, 1e-3, 124.0], np.float32)
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], np.float32)


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _geo(name):
    case = T.CASES[name]
    return case, T.Geometry(*case["size"], **case["tile"])


def _image(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    x = rng.standard_normal(shape).astype(np.float32)
    x.flat[:4] = SPECIALS[:4]
    return x


def _inside(pa, host, off):
    """`host` on the device, `off` elements into a larger block of sentinels.  -> (view, check that the block is as uploaded)."""
    sent = SENT8 if host.dtype == np.uint8 else np.float32(-77.25)
    flat = np.full(PAD + off + host.size + PAD, sent, host.dtype)
    flat[PAD + off:PAD + off + host.size] = host.ravel()
    buf = pa.hip.asarray(flat)
    view = pa.hip.DeviceArray(host.shape, host.dtype, buf.ctx, buf.ptr + (PAD + off) * host.dtype.itemsize, buf)
    return view, lambda: bool((buf.get().view(np.uint8) == flat.view(np.uint8)).all())


def _same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        np.testing.assert_array_equal(T.canonical(got), T.canonical(want))
    else:
        np.testing.assert_array_equal(got, want)


# ---- the gather kernel ------------------------------------------------------------------------------------------------------------
def _cut(pa, host, off, windows, k=None, b=None, order=None, work=None, slots=None, y_off=0):
    """pl_tile_windows_* through WindowFeed.decode_into on a framed output, the image `off` elements into a larger block; and
    util.cut_windows on the same image."""
    dev, unchanged = _inside(pa, host, off)
    spec = pa.util.ImageSpec(k, b, "nhwc", None, order) if host.dtype == np.uint8 else None
    feed = pa.util.WindowFeed(dev, windows, spec, work, slots)
    _, got, intact = framed_call(pa, feed.shape, np.float32, y_off, feed.decode_into)
    assert intact and unchanged()
    whole = pa.util.cut_windows(dev, windows, k, b, order, work, slots)
    assert isinstance(whole, pa.hip.DeviceArray) and whole.shape == feed.shape
    _same(whole.get(), got)
    return got


@pytest.mark.parametrize("name", ["a", "b", "e", "d"])
@pytest.mark.parametrize("c, order", [(1, None), (3, None), (3, (2, 1, 0)), (4, (3, 0, 1)), (4, None), (1, (0, 0, 0))])
def test_cut_windows_from_uint8(pa, name, c, order):
    case, geo = _geo(name)
    img = _image(case["size"] + (c,), np.uint8, 11 * c + len(name))
    co = len(order) if order else c
    work = geo.work if geo.resampled else None
    for off in (0, 1, 2, 3):
        want = T.cut_ref(img, geo.windows, K4[:co], B4[:co], order, geo.work)
        got = _cut(pa, img, off, geo.windows, K4[:co], B4[:co], order, work, y_off=off)
        assert got.shape == (len(geo.windows), co) + geo.win
        _same(got, want)


@pytest.mark.parametrize("name", ["a", "e", "g"])
@pytest.mark.parametrize("c", [0, 1, 2, 5])
def test_cut_windows_from_float32(pa, name, c):
    case, geo = _geo(name)
    img = _image(case["size"] + ((c,) if c else ()), np.float32, 5 + c)          # c = 0: a 2-d image counts as one channel
    for off in (0, 1, 3):
        got = _cut(pa, img, off, geo.windows, work=geo.work if geo.resampled else None, y_off=(off + 1) % 4)
        _same(got, T.cut_ref(img, geo.windows, work=geo.work))


def test_cut_windows_odd_window_sizes_and_more_slots_than_windows(pa):
    """h w % 4 != 0 (single-float stores, groups that span rows), a run of slots in the middle, slots past the last window."""
    img = _image((23, 31, 3), np.uint8, 3)
    windows = [(slice(r, r + 7), slice(c, c + 9)) for r in (0, 8, 16) for c in (0, 11, 22)]
    k, b = K4[:3], B4[:3]
    want = T.cut_ref(img, windows, k, b)
    _same(_cut(pa, img, 1, windows, k, b), want)
    _same(_cut(pa, img, 2, windows, k, b, slots=13, y_off=1), T.cut_ref(img, windows, k, b, slots=13))
    fimg = _image((23, 31, 2), np.float32, 4)
    _same(_cut(pa, fimg, 1, windows, slots=11), T.cut_ref(fimg, windows, slots=11))
    feed = pa.util.WindowFeed(pa.hip.asarray(img), windows, pa.util.ImageSpec(k, b))
    for lo, slots in ((0, 4), (4, 4), (8, 4), (7, 1)):                     # chunks as Net.tiled cuts them: the last one padded
        _, got, intact = framed_call(pa, (slots, 3, 7, 9), np.float32, 0, feed.chunk(lo, slots).decode_into)
        assert intact
        _same(got, T.cut_ref(img, windows[lo:lo + slots], k, b, slots=slots))
    with pytest.raises(ValueError, match="slots"):
        pa.util.cut_windows(pa.hip.asarray(img), windows, k, b, slots=8)
    with pytest.raises(ValueError, match="outside"):
        pa.util.cut_windows(pa.hip.asarray(img), [(slice(20, 27), slice(0, 9))], k, b)
    with pytest.raises(ValueError, match="k and b"):
        pa.util.cut_windows(pa.hip.asarray(img), windows)


# ---- the blend kernel -------------------------------------------------------------------------------------------------------------
def _results(n, c, oh, ow, seed):
    """Multiples of 0.5 (ties between planes are common, so are exact cancellations) with NaN, +-inf and +-0.0 planted; the
    centre of every window is -0.0 in plane 0."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-6, 7, (n, c, oh, ow)) / 2).astype(np.float32)
    where = rng.random(x.shape) < 0.04
    x[where] = SPECIALS[rng.integers(0, len(SPECIALS), int(where.sum()))]
    x[:, 0, oh // 2, ow // 2] = -0.0
    return x


FORMS = {
    "float": ("float",),
    "labels": ("labels", 0.25),
    "nhwc": ("image", K4[:3], B4[:3], "nhwc", (2, 0, 1), False),
    "nchw-truncate": ("image", np.float32([40.0]), np.float32([100.0]), "nchw", None, True),
}


def _out_spec(pa, form):
    if form[0] == "float":
        return "float"
    if form[0] == "labels":
        return pa.util.LabelSpec(form[1])
    _, k, b, layout, order, trunc = form
    return pa.util.ImageOutSpec(k, b, layout, order, "truncate" if trunc else "nearest")


def _blend(pa, x, geo, k, form, x_off=0, y_off=0):
    """The blend entry point itself on a framed output (the results `x_off` floats into a larger block), and util.blend_windows."""
    lib, ctx = pa._lib.load(), pa.hip.context()
    dev, unchanged = _inside(pa, x, x_off)
    n, c, oh, ow = x.shape
    bg = pa.util.BlendGeometry(geo.windows, k, geo.margin, geo.work, oh, ow)
    origins = pa.hip.asarray(np.concatenate([bg.R0, bg.C0]))
    args = (n, c, oh, ow, origins.ptr, origins.ptr + 4 * n, bg.gr, bg.gc, bg.OH, bg.OW, bg.ramp)
    if form[0] == "float":
        shape, dtype = (bg.OH, bg.OW, c), np.float32
        call = lambda y: lib.pl_tile_blend_f32(ctx.handle, dev.ptr, y, *args)                                   # noqa: E731
    elif form[0] == "labels":
        shape, dtype = (bg.OH, bg.OW), np.uint8
        call = lambda y: lib.pl_tile_blend_labels_u8(ctx.handle, dev.ptr, y, *args, float(form[1]))             # noqa: E731
    else:
        _, kk, bb, layout, order, trunc = form
        co = len(order) if order else c
        kk, bb = np.broadcast_to(kk, (co,)), np.broadcast_to(bb, (co,))
        shape, dtype = ((bg.OH, bg.OW, co) if layout == "nhwc" else (co, bg.OH, bg.OW)), np.uint8
        ka, ba = (ctypes.c_float * co)(*kk.tolist()), (ctypes.c_float * co)(*bb.tolist())
        oa = None if order is None else (ctypes.c_int * co)(*order)
        call = lambda y: lib.pl_tile_blend_u8(ctx.handle, dev.ptr, y, *args, co, oa, int(layout == "nhwc"), ka, ba, int(trunc))  # noqa: E731
    status, got, intact = framed_call(pa, shape, dtype, y_off, call)
    assert status == 0 and intact and unchanged()
    whole = pa.util.blend_windows(dev, geo.windows, k, geo.margin, geo.work, _out_spec(pa, form))
    _same(whole.get(), got)
    return got


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", sorted(T.CASES))
def test_blend_windows_is_the_reference_loop_bit_for_bit(pa, name, form):
    case, geo = _geo(name)
    k = case["k"]
    oh, ow = int(geo.win[0] * k), int(geo.win[1] * k)
    c = 1 if form == "nchw-truncate" else 3
    for seed, (x_off, y_off) in enumerate(((0, 0), (1, 3), (3, 1))):
        x = _results(len(geo.windows), c, oh, ow, 100 * seed + len(name) + c)
        want = T.encode_ref(T.blend_ref(x, geo.windows, k, geo.margin, geo.work), FORMS[form])
        _same(_blend(pa, x, geo, k, FORMS[form], x_off, y_off), want)
        if form == "float":
            assert np.isnan(want).any() and np.isinf(want).any()
            if name in "acd":
                assert (np.signbit(want) & (want == 0)).any()       # a -0.0 under window 0 alone stays -0.0


@pytest.mark.parametrize("c", [1, 2, 5, 21])
def test_blend_labels_and_planes(pa, c):
    """One plane is a threshold; more planes than one chunk of four; exact ties between classes after blending."""
    case, geo = _geo("b")
    x = _results(len(geo.windows), c, 16, 16, c)
    x[:, c - 1] = x[:, 0]                                             # the last plane ties with the first everywhere
    blended = T.blend_ref(x, geo.windows, 1, geo.margin, geo.work)
    for form in (("labels", 0.0), ("labels", -0.5), ("float",)):
        _same(_blend(pa, x, geo, 1, form, 1, 1), T.encode_ref(blended, form))
    if c > 1:
        assert (T.encode_ref(blended, ("labels", 0.0)) != c - 1).all()  # the first of equal maxima


def test_blend_refusals(pa):
    lib, ctx = pa._lib.load(), pa.hip.context()
    case, geo = _geo("a")
    x = pa.hip.asarray(_results(12, 3, 16, 16, 1))
    y = pa.hip.empty((37, 45, 3))
    origins = pa.hip.asarray(np.zeros(24, np.int32))
    ok = [12, 3, 16, 16, origins.ptr, origins.ptr + 48, 3, 4, 37, 45, 4]
    for i, bad, code in ((0, 11, 1), (6, 4, 1), (2, 40, 1), (10, -1, 1), (1, 0, 1), (8, -1, 1)):
        args = list(ok)
        args[i] = bad
        assert lib.pl_tile_blend_f32(ctx.handle, x.ptr, y.ptr, *args) == code, (i, bad)
        assert lib.pl_last_error()
    args = list(ok)
    args[1] = 257                                                     # (refused before anything is read)
    assert lib.pl_tile_blend_labels_u8(ctx.handle, x.ptr, y.ptr, *args, 0.0) == 2
    assert lib.pl_tile_blend_f32(ctx.handle, None, y.ptr, *ok) == 1
    with pytest.raises(ValueError, match="12 windows"):
        pa.util.blend_windows(pa.hip.zeros((11, 3, 16, 16)), geo.windows, 1, geo.margin, geo.work)


# ---- Net.tiled --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets(pa):
    """k -> (net with image_input k = 1, b = 0 declared, numpy function of the same net): built once, shared and left as built
    (the tests declare output forms and take them back)."""
    made = {}
    for k in (1, 2, 0.5):
        g, b, fn = T.exact_net(3, 3, k)
        net = pa.from_graph(g, b)
        net.image_input(np.ones(3, np.float32), np.zeros(3, np.float32))
        made[k] = (net, fn)
    return made


def _declare(net, form):
    net.float_output()
    if form[0] == "labels":
        net.label_output(form[1])
    elif form[0] == "image":
        _, k, b, layout, order, trunc = form
        net.image_output(k, b, layout=layout, order=order, rounding="truncate" if trunc else "nearest")


E2E_FORMS = [("float",), ("labels", 0.0), ("image", np.float32([0.01]), np.float32([128.0]), "nhwc", None, False)]


@pytest.mark.parametrize("name, batch", [("a", None), ("a", 5), ("b", None), ("c", 4), ("f", None), ("f", 5), ("g", None), ("g", 7)])
def test_net_tiled_equals_the_mirror_around_the_oracle(pa, nets, name, batch):
    case, geo = _geo(name)
    net, fn = nets[case["k"]]
    img = _image(case["size"] + (3,), np.uint8, 40 + len(name))
    one, zero = np.ones(3, np.float32), np.zeros(3, np.float32)
    n = len(geo.windows)
    try:
        for form in E2E_FORMS:
            _declare(net, form)
            calls, want_calls = [], []
            want = T.tiled_ref(fn, img, one, zero, out=form, progress=lambda i, m: want_calls.append((i, m)), **case["tile"])
            got = net.tiled(img, batch=batch, progress=lambda i, m: calls.append((i, m)), **case["tile"])
            assert isinstance(got, np.ndarray)
            _same(got, want)
            step = batch or n
            assert calls == [(min(lo + step, n), n) for lo in range(0, n, step)] and set(calls) <= set(want_calls)
            dev = net.tiled(pa.hip.asarray(img), batch=batch, **case["tile"])                 # device in, device out
            assert isinstance(dev, pa.hip.DeviceArray)
            _same(dev.get(), want)
        assert len(np.unique(want)) > 8
        net.float_output()
        got = net.tiled(img.astype(np.float32), batch=batch, **case["tile"])                  # float32 is taken as it is
        _same(got, T.tiled_ref(fn, img.astype(np.float32), **case["tile"]))
    finally:
        net.float_output()
    pa.hip.trim_side_contexts()


@pytest.mark.parametrize("name", ["d", "e"])
def test_net_tiled_resampled(pa, nets, name):
    """The working size differs from the image's: the gather kernel resamples, so the net's inputs are no integers and its sums
    depend on their order -- the mirror is built around THIS net's own plan for the window stack (the same signature, so the same
    plan Net.tiled runs), everything else is as above.  One window (d): the result is the window's, resized back."""
    case, geo = _geo(name)
    net, _ = nets[1]
    img = _image(case["size"] + (3,), np.uint8, 7)
    one, zero = np.ones(3, np.float32), np.zeros(3, np.float32)
    plain = lambda x: net(np.ascontiguousarray(x))                                            # noqa: E731
    want = T.tiled_ref(plain, img, one, zero, **case["tile"])
    calls = []
    got = net.tiled(img, progress=lambda i, m: calls.append((i, m)), **case["tile"])
    _same(got, want)
    assert got.shape == case["size"] + (3,) and calls == ([] if name == "d" else [(len(geo.windows), len(geo.windows))])
    _same(net.tiled(pa.hip.asarray(img.astype(np.float32)), **case["tile"]).get(),
          T.tiled_ref(plain, img.astype(np.float32), **case["tile"]))
    net.label_output()
    try:
        with pytest.raises(NotImplementedError, match="different product"):
            net.tiled(img, **case["tile"])
    finally:
        net.float_output()
    pa.hip.trim_side_contexts()


def test_net_tiled_equals_util_tile_batched(pa, nets):
    """The old route around the same net on case (a): equal values (a -0.0 the accumulate path turns into +0.0 compares equal)."""
    case, geo = _geo("a")
    net, _ = nets[1]
    img = _image(case["size"] + (3,), np.uint8, 9).astype(np.float32)

    def f(stack):
        return pa.Transpose(net(pa.Transpose(stack, [0, 3, 1, 2])), [0, 2, 3, 1])
    old = pa.util.tile(progress=lambda i, n: None, batched=True, **case["tile"])(f)(img)
    new = net.tiled(img, **case["tile"])
    assert old.dtype == new.dtype == np.float32 and old.shape == new.shape
    np.testing.assert_array_equal(new, old)
    pa.hip.trim_side_contexts()


def test_a_second_call_compiles_nothing_and_refusals(pa, nets):
    case, geo = _geo("a")
    net, _ = nets[1]
    img = _image(case["size"] + (3,), np.uint8, 21)
    first = net.tiled(img, batch=5, **case["tile"])
    plans = dict(net._plans)
    again = net.tiled(_image(case["size"] + (3,), np.uint8, 22), batch=5, **case["tile"])
    assert len(net._plans) == len(plans) and all(net._plans[key] is plans[key] for key in plans)
    assert first.shape == again.shape and (first != again).any()
    _same(net.tiled(img, batch=5, **case["tile"]), first)
    with pytest.raises(ValueError, match="no order"):                  # three values in image_input's k, a one-channel image
        net.tiled(img[:, :, :1].copy(), **case["tile"])
    with pytest.raises(ValueError, match="does not have"):
        pa.util.cut_windows(pa.hip.asarray(img[:, :, :1].copy()), geo.windows, np.ones(3), np.zeros(3), order=(0, 1, 2))
    from tests.test_gpu_image_output import _two_outputs
    g, b = _two_outputs()
    two = pa.from_graph(g, b)
    with pytest.raises(ValueError, match="one output"):
        two.tiled(img.astype(np.float32), **case["tile"])
    pa.hip.trim_side_contexts()

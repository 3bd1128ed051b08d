"""Transposed convs by output phase (pl_conv2d_convt_q4_f32) on the GPU.  On integer operands (tests/ref64.py) the kernel must
equal the float64 reference of the equivalent zero-stuffed conv bit for bit -- through the eager NCHW entry and the channel-quad
entry under every fused tail, every tile config and split-K; on float data it must stay within that conv's per-element bound.
Each case asserts the plan string, so a silent fallback cannot pass.  The refusals and the stuffed path (dilation > 1) are
unchanged; both U-Net variants run through Net, the pipelined path and a plan file."""
import zlib

import numpy as np
import pytest

from oracle import planer_np as onp
from tests import ref64 as R
from tests.conftest import RTOL, assert_close
from tests.test_gpu_conv_exact import TAILS
from tests.test_plan_convtranspose import GEOMS as ALL_GEOMS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _dev(pa, a):
    return None if a is None else pa.asarray(np.ascontiguousarray(a))


def stuffed(x, K, strides, pads, output_padding):
    """The reference's form (layer.py:28-34): zero-stuffed x and the flipped, transposed filter of a stride-1 conv."""
    (s1, s2), (kh, kw) = strides, K.shape[2:]
    lo_h, hi_h = kh - 1 - pads[0], kh - 1 - pads[2] + output_padding[0]
    lo_w, hi_w = kw - 1 - pads[1], kw - 1 - pads[3] + output_padding[1]
    n, c, h, w = x.shape
    buf = np.zeros((n, c, (h - 1) * s1 + lo_h + hi_h + 1, (w - 1) * s2 + lo_w + hi_w + 1), x.dtype)
    buf[:, :, lo_h:buf.shape[2] - hi_h:s1, lo_w:buf.shape[3] - hi_w:s2] = x
    return buf, np.ascontiguousarray(K.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def _case(key, xs, ks, tail, strides, pads, op):
    bias, bn, res, act = tail
    rng = np.random.default_rng(zlib.crc32(repr((key, xs, ks, tail)).encode()))
    x, K = R.int_tensor(rng, xs), R.int_tensor(rng, ks)
    buf, Kt = stuffed(x, K, strides, pads, op)
    out = (xs[0], ks[1], buf.shape[2] - ks[2] + 1, buf.shape[3] - ks[3] + 1)
    B, sc, sh, r = R.int_tail(rng, ks[1], out, bias, bn, res)
    R.assert_exact(buf, Kt, B, sc, sh, r)
    return (x, K, B, sc, sh, r), act, R.ref64(buf, Kt, B, sc, sh, r, act=act, alpha=R.ALPHA)


def _q4(pa, x, K, B, sc, sh, r, act, strides, pads, op, Kp=None):
    q4 = pa.q4
    resq = q4.to_q4(_dev(pa, r)) if r is not None else None
    Kd = Kp if Kp is not None else _dev(pa, K)
    y = q4.ConvTransposeQ4(q4.to_q4(_dev(pa, x)), Kd, _dev(pa, B), _dev(pa, sc), _dev(pa, sh), resq, strides=list(strides),
                           pads=list(pads), output_padding=list(op), act=act, alpha=R.ALPHA, w_layout=14 if Kp is not None else 0)
    return q4.from_q4(y).get()


def _expect_plan(ctx, strides, K):
    plan = ctx.last_conv_plan()
    th, tw = -(-K.shape[2] // strides[0]), -(-K.shape[3] // strides[1])
    assert plan.startswith("convt-q4 phases=%dx%d taps=%dx%d " % (strides[0], strides[1], th, tw)), plan
    return plan


def _exact(y, want, what, plan):
    assert y.shape == want.shape, (what, plan, y.shape, want.shape)
    np.testing.assert_array_equal(np.asarray(y).astype(np.float64), want, err_msg="%s [%s]" % (what, plan))


GEOMS = ALL_GEOMS[::3]


@pytest.mark.parametrize("gi", range(0, len(GEOMS), 8))
def test_geometry_sweep_exact_both_entries_every_tail(pa, gi):
    ctx = pa.hip.context()
    for i, ((kh, kw), s, pads, op) in enumerate(GEOMS[gi:gi + 8]):
        h, w = [(1, 1), (1, 4), (3, 1), (4, 5), (6, 3)][(gi + i) % 5]
        if (h - 1) * s[0] - pads[0] - pads[2] + kh + op[0] <= 0 or (w - 1) * s[1] - pads[1] - pads[3] + kw + op[1] <= 0:
            continue
        n = 1 + 2 * ((gi + i) % 2)
        what = "k%dx%d s%s p%s op%s %dx%d" % (kh, kw, s, pads, op, h, w)
        # eager NCHW entry (bias only, the reference op's signature)
        (x, K, B, _, _, _), _, want = _case(what, (n, 3, h, w), (3, 5, kh, kw), TAILS[1], s, pads, op)
        y = pa.ConvTranspose2d(_dev(pa, x), _dev(pa, K), _dev(pa, B), strides=list(s), dilations=[1, 1], pads=list(pads),
                               output_padding=list(op))
        _exact(y.get(), want, "nchw " + what, _expect_plan(ctx, s, K))
        for t, tail in enumerate(TAILS):
            ops, act, want = _case(what, (n, 3, h, w), (3, 5, kh, kw), tail, s, pads, op)
            y = _q4(pa, *ops, act, s, pads, op)
            _exact(y, want, "q4 %s tail %d" % (what, t), _expect_plan(ctx, s, ops[1]))


CHANNELS = [(ci, co) for ci in (1, 3, 5, 8, 13, 64, 256) for co in (1, 5, 8, 64, 512)]


@pytest.mark.parametrize("ci, co", CHANNELS)
def test_channels_exact_k3_and_k2(pa, ci, co):
    ctx = pa.hip.context()
    for j, (k, s, pads, op) in enumerate([(3, (2, 2), (1, 1, 1, 1), (1, 1)), (2, (2, 2), (0, 0, 0, 0), (0, 0))]):
        tail = TAILS[(ci + co + j) % len(TAILS)]
        n = 3 if j == 0 else 1
        ops, act, want = _case("ch", (n, ci, 5, 6), (ci, co, k, k), tail, s, pads, op)
        y = _q4(pa, *ops, act, s, pads, op)
        _exact(y, want, "q4 %d->%d k%d" % (ci, co, k), _expect_plan(ctx, s, ops[1]))


def test_every_tile_config_and_split_k(pa):
    from tests.test_gpu_conv_exact import _cfg_names
    ctx = pa.hip.context()
    names = _cfg_names(pa)
    s, pads, op = (2, 2), (1, 1, 1, 1), (1, 1)
    ops, act, want = _case("cfg", (2, 40, 9, 7), (40, 36, 3, 3), TAILS[3], s, pads, op)
    ran = 0
    try:
        for cfg, name in enumerate(names):
            if not name.startswith("q"):
                continue
            for split in (1, 2, 3):
                ctx.set_conv_config(cfg, split)
                y = _q4(pa, *ops, act, s, pads, op)
                plan = _expect_plan(ctx, s, ops[1])
                assert name in plan and ("split=%d" % split in plan or split > 1 and "split=1" not in plan), plan
                _exact(y, want, "cfg %s split %d" % (name, split), plan)
                ran += 1
    finally:
        ctx.set_conv_config(-1, 0)
    assert ran >= 36


def test_prepared_filter_matches_host_packing(pa):
    rng = np.random.default_rng(5)
    for (ci, co, kh, kw, sh, sw) in [(5, 6, 3, 3, 2, 2), (3, 2, 2, 5, 2, 3), (8, 4, 1, 1, 2, 2), (4, 9, 4, 2, 1, 2)]:
        K = rng.standard_normal((ci, co, kh, kw)).astype(np.float32)
        got = pa.q4.prepare_convt_q4_weights(_dev(pa, K), (sh, sw))
        th, tw, cq = -(-kh // sh), -(-kw // sw), (ci + 3) // 4
        qtot = th * tw * cq
        qpad = (qtot + 7) // 8 * 8
        want = np.zeros((sh * sw, qpad, co, 4), np.float32)
        for ph in range(sh * sw):
            rh, rw = divmod(ph, sw)
            for a in range(th):
                for b in range(tw):
                    ky, kx = rh + sh * (th - 1 - a), rw + sw * (tw - 1 - b)
                    if ky < kh and kx < kw:
                        for c in range(ci):
                            want[ph, (a * tw + b) * cq + c // 4, :, c % 4] = K[c, :, ky, kx]
        assert got.shape == K.shape
        host = pa.hip.DeviceArray((want.size,), np.float32, got.ctx, got.ptr, got).get()     # the packed allocation
        np.testing.assert_array_equal(host, want.ravel())


@pytest.mark.parametrize("xs, ks, s, pads, op", [
    ((8, 1024, 16, 16), (1024, 512, 2, 2), (2, 2), (0, 0, 0, 0), (0, 0)),
    ((2, 128, 128, 128), (128, 64, 2, 2), (2, 2), (0, 0, 0, 0), (0, 0)),     # batch 2: the float64 reference's im2col of the
                                                                              # stuffed 257^2 map is 0.5 GB per image
    ((2, 64, 20, 18), (64, 40, 3, 3), (2, 2), (1, 1, 1, 1), (1, 1)),
    ((3, 13, 11, 9), (13, 7, 5, 4), (3, 2), (2, 1, 0, 3), (1, 0)),
])
def test_float_bounds_skewed_operands(pa, xs, ks, s, pads, op):
    ctx = pa.hip.context()
    rng = np.random.default_rng(zlib.crc32(repr((xs, ks)).encode()))
    x, Kt0, sc = R.skewed_operands(rng, xs, (ks[1], ks[0], ks[2], ks[3]))
    K = np.ascontiguousarray(Kt0.transpose(1, 0, 2, 3))
    B = rng.standard_normal(ks[1]).astype(np.float32)
    sh = rng.standard_normal(ks[1]).astype(np.float32)
    buf, Kt = stuffed(x, K, s, pads, op)
    want = R.ref64(buf, Kt, B, sc, sh, act=R.ACT_RELU)
    tol = R.bound(buf, Kt, B, sc, sh, lam=R.LAMBDA["direct"])
    y = _q4(pa, x, K, B, sc, sh, None, R.ACT_RELU, s, pads, op)
    R.check(y, want, tol, "q4 %s %s" % (xs, ks), _expect_plan(ctx, s, K))
    if xs[2] > 32:
        return
    y = pa.ConvTranspose2d(_dev(pa, x), _dev(pa, K), _dev(pa, B), strides=list(s), dilations=[1, 1], pads=list(pads),
                           output_padding=list(op)).get()
    R.check(y, R.ref64(buf, Kt, B), R.bound(buf, Kt, B), "nchw %s %s" % (xs, ks), _expect_plan(ctx, s, K))


def test_refusals_and_the_stuffed_path_unchanged(pa):
    rng = np.random.default_rng(9)
    x = rng.standard_normal((1, 4, 5, 5)).astype(np.float32)
    with pytest.raises(NotImplementedError):
        pa.ConvTranspose2d(_dev(pa, x), _dev(pa, rng.standard_normal((4, 2, 3, 3)).astype(np.float32)), group=2)
    with pytest.raises(NotImplementedError):
        pa.ConvTranspose2d(_dev(pa, x), _dev(pa, rng.standard_normal((4, 3, 3, 3)).astype(np.float32)), pads=[3, 0, 0, 0])
    K = rng.standard_normal((4, 3, 3, 3)).astype(np.float32)
    para = dict(strides=[2, 2], dilations=[2, 2], pads=[1, 1, 1, 1], output_padding=[1, 1])
    y = pa.ConvTranspose2d(_dev(pa, x), _dev(pa, K), **para)
    assert not pa.hip.context().last_conv_plan().startswith("convt-q4")
    assert_close(y.get(), onp.convtranspose2d(x, K, **para), RTOL, "stuffed path")


def test_golden_convtranspose_cases_on_the_new_kernel(pa, golden_layers):
    from tests.cases import layer_cases
    z, _ = golden_layers
    ctx = pa.hip.context()
    ran = 0
    for name, kind, args, params in layer_cases():
        if kind != "convtranspose" or list(params.get("dilations", [1, 1])) != [1, 1]:
            continue
        y = pa.layer_map[kind](*[pa.asarray(a.copy()) for a in args], **params)
        _expect_plan(ctx, params.get("strides", [2, 2]), args[1])
        assert_close(y.get(), z["%s/out0" % name], RTOL, name)
        ran += 1
    assert ran == 3


@pytest.fixture(scope="module", params=["k2", "k3"])
def unet_model(request):
    from planer_amd.irgen import unet
    g, b = unet.build(up=request.param)
    x = unet.make_input(2, size=64)
    ref = onp.OracleNet()
    ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
    ref.load_weights(b)
    return request.param, g, b, x, ref(x.copy())


def test_unet_through_net_pipelined_and_plan_file(pa, unet_model, tmp_path):
    from planer_amd.export import export_plan
    from tests.test_gpu_plan_file import _bind, _run_plan
    up, g, b, x, want = unet_model
    net = pa.from_graph(g, b)
    got = net(pa.asarray(x)).get()
    assert got.shape == (2, 2, 64, 64)
    assert_close(got, want, RTOL, "unet-%s b2" % up)
    plan = net.compile(pa.asarray(x))
    ups = [a for a in plan.algos if a["kind"] == "convt_q4"]
    assert len(ups) == 4 and all(a["w_layout"] == 14 and a["plan"].startswith("convt-q4 phases=2x2") for a in ups), plan.algos
    assert_close(net.submit(pa.asarray(x, ctx=net.ctx)).get(), want, RTOL, "unet-%s submit" % up)
    path = tmp_path / ("unet_%s.plplan" % up)
    blob = export_plan(net, x, path=str(path))
    assert b"pl_conv2d_convt_q4_f32" in blob
    out, = _run_plan(_bind(), open(path, "rb").read(), [x])
    assert_close(out, want, RTOL, "unet-%s plan file" % up)

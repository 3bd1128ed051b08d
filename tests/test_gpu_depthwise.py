"""Depthwise convolution kernels on a real MI355X (csrc/conv_dw_kernel.h): the NCHW form that pl_conv2d_fused_f32 routes
group == Cin == Cout convs to, and the channel-quad form (pl_conv2d_dw_q4_f32, w_layout 13), against the oracle's grouped conv
plus the fused tail, to tests.conftest.RTOL of max|ref|; MobileNet-v2 end to end through Net, core(numpy) and a plan file."""
import numpy as np
import pytest

from oracle import planer_np as onp
from planer_amd.plan import ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_RES_AFTER
from tests.cases import layer_cases
from tests.conftest import RTOL, assert_close
from tests.test_plan_fusion import conv_fused_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def q4_host(x):
    n, c, h, w = x.shape
    cq = (c + 3) // 4
    pad = np.zeros((n, cq * 4, h, w), x.dtype)
    pad[:, :c] = x
    return np.ascontiguousarray(pad.reshape(n, cq, 4, h, w).transpose(0, 1, 3, 4, 2))


# (bias, scale/shift, residual, act): every tail the epilogue knows, the residual before and after the activation
TAILS = [(False, False, False, ACT_NONE), (True, False, False, ACT_NONE), (False, True, False, ACT_RELU),
         (True, True, True, ACT_RELU), (False, True, True, ACT_LEAKY | ACT_RES_AFTER), (True, False, True, ACT_NONE),
         (False, True, False, ACT_LEAKY), (True, True, True, ACT_RELU | ACT_RES_AFTER)]
CHANNELS = [4, 8, 12, 32, 144, 960, 6, 10]
SPATIAL = [(1, 1, 1), (3, 7, 9), (1, 13, 5), (3, 17, 23), (32, 7, 7), (1, 30, 31), (3, 1, 12), (32, 14, 15)]


def _cases():
    out, i = [], 0
    for k in (1, 3, 5, 7):
        for s in (1, 2):
            for d in (1, 2):
                for v in range(3):
                    c = CHANNELS[(i * 3 + v) % len(CHANNELS)]
                    n, h, w = SPATIAL[(i * 5 + v * 3) % len(SPATIAL)]
                    while n > 1 and n * c * h * w > 600000:       # keep the oracle quick
                        n = max(1, n // 4)
                    p = (k - 1) * d // 2 if v != 2 else 0
                    if h + 2 * p < (k - 1) * d + 1 or w + 2 * p < (k - 1) * d + 1:
                        p = (k - 1) * d // 2
                    out.append((k, s, d, p, c, n, h, w, TAILS[i % len(TAILS)]))
                    i += 1
    return out


CASES = _cases()


def _operands(case):
    k, s, d, p, c, n, h, w, (bias, ss, res, act) = case
    rng = np.random.default_rng(abs(hash(case[:8])) % (1 << 32))
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    K = (rng.standard_normal((c, 1, k, k)) * 0.3).astype(np.float32)
    ho = (h + 2 * p - (k - 1) * d - 1) // s + 1
    wo = (w + 2 * p - (k - 1) * d - 1) // s + 1
    B = rng.standard_normal(c).astype(np.float32) if bias else None
    sc = rng.uniform(0.5, 1.5, c).astype(np.float32) if ss else None
    sh = rng.standard_normal(c).astype(np.float32) if ss else None
    r = rng.standard_normal((n, c, ho, wo)).astype(np.float32) if res else None
    conv = dict(group=c, strides=[s, s], dilations=[d, d], pads=[p, p, p, p])
    ref = conv_fused_np(x, K, B, sc, sh, r, act=act, alpha=0.1, **conv)
    return x, K, B, sc, sh, r, act, conv, np.ascontiguousarray(ref)


def _dev(pa, a):
    return None if a is None else pa.asarray(a)


@pytest.mark.parametrize("case", CASES, ids=["k%d_s%d_d%d_p%d_c%d_n%d_%dx%d_t%d" % (c[:8] + (TAILS.index(c[8]),)) for c in CASES])
def test_depthwise_nchw_and_q4_match_the_oracle(pa, case):
    from planer_amd import layer, q4
    x, K, B, sc, sh, r, act, conv, ref = _operands(case)
    ctx = pa.hip.context()
    y = layer.ConvFused(pa.asarray(x), pa.asarray(K), _dev(pa, B), _dev(pa, sc), _dev(pa, sh), _dev(pa, r), act=act, alpha=0.1,
                        **conv)
    assert ctx.last_conv_plan().startswith("depthwise-nchw"), ctx.last_conv_plan()
    assert ctx.last_conv_extents()[1] == 1                                    # one FMA row per channel, no MFMA tile
    assert_close(y.get(), ref, RTOL, "nchw %s" % (case,))

    assert q4.dw_q4_eligible(K.shape, **conv)
    rq = q4.to_q4(pa.asarray(r)) if r is not None else None
    yq = q4.ConvQ4(q4.to_q4(pa.asarray(x)), q4.prepare_dw_q4_weights(pa.asarray(K)), _dev(pa, B), _dev(pa, sc), _dev(pa, sh), rq,
                   act=act, alpha=0.1, w_layout=13, **conv)
    assert ctx.last_conv_plan().startswith("depthwise-q4"), ctx.last_conv_plan()
    assert q4.logical_shape(yq) == ref.shape
    raw = yq.get()
    assert_close(q4.from_q4(yq).get(), ref, RTOL, "q4 %s" % (case,))
    np.testing.assert_array_equal(raw, q4_host(q4.from_q4(yq).get()))          # padding lanes of a partial quad stay zero


def test_prepared_filter_layout(pa):
    from planer_amd import q4
    K = np.random.default_rng(2).standard_normal((10, 1, 3, 5)).astype(np.float32)
    got = q4.prepare_dw_q4_weights(pa.asarray(K))
    assert got.shape == K.shape
    raw = pa.hip.DeviceArray((3 * 15 * 4,), np.float32, got.ctx)
    pa._lib.call("pl_d2d", got.ctx.handle, raw.ptr, got.ptr, raw.nbytes)
    want = np.zeros((12, 15), np.float32)
    want[:10] = K.reshape(10, 15)
    np.testing.assert_array_equal(raw.get().reshape(3, 15, 4), want.reshape(3, 4, 15).transpose(0, 2, 1))


def test_asymmetric_pads_are_refused_as_before(pa):
    """util.pad honours pads[0] / pads[1] only (util.py:8): asymmetric pads stay PL_EUNSUPPORTED on both forms."""
    from planer_amd import layer, q4
    x = pa.asarray(np.ones((1, 8, 9, 9), np.float32))
    K = pa.asarray(np.ones((8, 1, 3, 3), np.float32))
    with pytest.raises(NotImplementedError):
        layer.Conv2d(x, K, group=8, pads=(1, 0, 1, 2))
    assert not q4.dw_q4_eligible(K.shape, group=8, pads=(1, 0, 1, 2))
    xq, kq = q4.to_q4(x), q4.prepare_dw_q4_weights(K)
    yq = q4.to_q4(x)
    with pytest.raises(NotImplementedError):
        pa._lib.call("pl_conv2d_dw_q4_f32", x.ctx.handle, xq.ptr, 1, 8, 9, 9, kq.ptr, 3, 3, None, yq.ptr,
                     1, 1, 1, 1, 1, 0, 1, 2, None, None, None, 0, 0.0)


def test_forced_configuration_still_reaches_the_generic_kernel(pa):
    from planer_amd import layer
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 16, 12, 12)).astype(np.float32)
    K = rng.standard_normal((16, 1, 3, 3)).astype(np.float32)
    ctx = pa.hip.context()
    ctx.set_conv_config(0)
    try:
        y = layer.Conv2d(pa.asarray(x), pa.asarray(K), group=16, pads=(1, 1, 1, 1))
        assert not ctx.last_conv_plan().startswith("depthwise"), ctx.last_conv_plan()
    finally:
        ctx.set_conv_config(-1)
    assert_close(y.get(), np.ascontiguousarray(onp.conv2d(x, K, group=16, pads=(1, 1, 1, 1))), RTOL)


def test_golden_depthwise_case_runs_the_new_kernel(pa, golden_layers):
    case = next(c for c in layer_cases() if c[0] == "conv_depthwise_g8")
    name, kind, args, params = case
    z, _ = golden_layers
    ctx = pa.hip.context()
    y = pa.layer_map["conv"](pa.asarray(args[0]), pa.asarray(args[1]), pa.asarray(args[2]), **params)
    assert ctx.last_conv_plan().startswith("depthwise-nchw"), ctx.last_conv_plan()
    assert_close(y.get(), z["%s/out0" % name], RTOL, name)


@pytest.fixture(scope="module")
def mobilenet():
    from planer_amd.irgen import mobilenetv2
    g, b = mobilenetv2.build()
    x = mobilenetv2.make_input(4)
    ref = onp.OracleNet()
    ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
    ref.load_weights(b)
    return g, b, x, ref(x.copy())


def test_mobilenetv2_through_net(pa, mobilenet):
    from planer_amd.net import prog_body
    g, b, x, want = mobilenet
    net = pa.from_graph(g, b)
    got = net(pa.asarray(x)).get()
    assert got.shape == (4, 1000)
    assert_close(got, want, RTOL, "mobilenetv2 b4")
    # the compiled program: no layout conversion, every depthwise conv on w_layout 13, every clip in Q4
    xd = pa.asarray(x)
    shapes = {k: a.shape for k, a in zip(net.input, [xd])}
    shapes.update({k: w.shape for k, w in zip(net.inits, net.weights)})
    net._interpret(net._program, [xd.copy()], shapes=shapes)
    prog, _ = net._fuse(shapes, net.use_fusion)
    kinds = [e[1] for e in prog_body(prog)]
    assert "to_q4" not in kinds and "from_q4" not in kinds and "clip" not in kinds
    assert kinds.count("clip_q4") == 35
    plan = net.compile(xd)
    dw = [a for a in plan.algos if a["layer"].endswith("d_conv+")]
    assert len(dw) == 17 and all(a["w_layout"] == 13 and a["plan"].startswith("depthwise-q4") for a in dw), plan.algos
    # core(numpy): host arrays in and out, the same kernels
    try:
        assert pa.core(np, silent=True) is np
        host = net(x.copy())
        assert isinstance(host, np.ndarray)
        assert_close(host, want, RTOL, "mobilenetv2 b4 under core(numpy)")
        assert_close(host, got, 1e-6, "core(numpy) against device arrays")
    finally:
        pa.core("hip", silent=True)


def test_mobilenetv2_from_a_plan_file(pa, mobilenet, tmp_path):
    from planer_amd.export import export_plan
    from tests.test_gpu_plan_file import _bind, _run_plan
    g, b, x, want = mobilenet
    net = pa.from_graph(g, b)
    path = tmp_path / "mobilenetv2_b4.plplan"
    blob = export_plan(net, x, path=str(path))
    assert b"pl_conv2d_dw_q4_f32" in blob
    got, = _run_plan(_bind(), open(path, "rb").read(), [x])
    assert got.shape == (4, 1000)
    assert_close(got, want, RTOL, "mobilenetv2 b4 plan file")

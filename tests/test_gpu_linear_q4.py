"""Linear upsample and resize on channel-quad (Q4) tensors on a real MI355X: pl_upsample_linear_q4_f32 / pl_resize_linear_q4_f32
against their NCHW twins BIT FOR BIT (the existing tests pin the NCHW kernels to the reference's roundings, so equality with them
is the whole criterion: no tolerance anywhere in the kernel tests), the fused residual against AddQ4, padding lanes, special
values, refusals, pool hygiene; and the nets that use them -- a small graph and the Panoptic-FPN of planer_amd.irgen.fpn -- against
the oracle, switch on against switch off, step by step, and from a plan file."""
import ctypes

import numpy as np
import pytest

from oracle import planer_np as onp
from tests.conftest import RTOL, assert_close
from tests.linear_q4_ref import LINEAR_KINDS, Small, assert_same_bits, check_linear_steps, padding_lanes

pytestmark = pytest.mark.gpu

# (N, C, H, W, fh, fw): every clamp at once; a partial quad; unequal factors; the two two-term forms; a full 64-entry table; several
# quads and images; 544 960 output quads -- more than the 524 288 lanes one pass launches on 256 CUs, so the stride loop turns twice
INT_CASES = [(1, 1, 1, 1, 2, 2), (2, 5, 3, 5, 2, 2), (1, 4, 4, 7, 3, 2), (1, 8, 4, 5, 1, 2), (2, 4, 3, 5, 4, 1), (1, 4, 2, 2, 8, 8),
             (3, 12, 5, 6, 2, 2), (1, 32, 130, 131, 2, 2)]
PARTIAL, TWO_PASS = INT_CASES[1], INT_CASES[7]
# (shape, scales (fh, fw) or None, size (OH, OW) or None): the geometries of tests/cases.py, and a 2 x 2 map
FRAC_CASES = [((2, 3, 6, 8), (1.5, 2.25), None), ((1, 2, 9, 11), (0.5, 0.7), None), ((1, 3, 5, 7), None, (13, 10)),
              ((1, 5, 2, 2), (2.5, 2.5), None)]
EMPTY = np.zeros(0, np.float32)


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _rand(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _int_case(pa, case, x=None, res=None):
    """-> (raw Q4 result buffer, its channel count, the NCHW kernel's result)."""
    from planer_amd import layer, q4
    n, c, h, w, fh, fw = case
    x = _rand((n, c, h, w), sum(case)) if x is None else x
    k = np.array([1, 1, fh, fw], np.float32)
    xd = pa.hip.asarray(x)
    want = layer.UpSample(xd, k, mode="linear")
    rq = None
    if res is not None:
        rd = pa.hip.asarray(res)
        want, rq = layer.Add(want, rd), q4.to_q4(rd)
    yq = q4.UpSampleQ4(q4.to_q4(xd), k, "linear", resq=rq)
    assert q4.logical_shape(yq) == want.shape
    return yq.get(), c, q4.from_q4(yq).get(), want.get()


def _frac_case(pa, case, x=None, res=None):
    from planer_amd import layer, q4
    shape, scales, size = case
    x = _rand(shape, 7 + shape[2]) if x is None else x
    k = EMPTY if scales is None else np.array([1, 1, scales[0], scales[1]], np.float32)
    sz = None if size is None else np.array([shape[0], shape[1], size[0], size[1]], np.int64)
    xd = pa.hip.asarray(x)
    want = layer.Resize(xd, EMPTY, k, sz, mode="linear")
    rq = None
    if res is not None:
        rd = pa.hip.asarray(res)
        want, rq = layer.Add(want, rd), q4.to_q4(rd)
    yq = q4.ResizeQ4(q4.to_q4(xd), EMPTY, k, sz, mode="linear", resq=rq)
    assert q4.logical_shape(yq) == want.shape
    return yq.get(), shape[1], q4.from_q4(yq).get(), want.get()


def _out_shape(case):
    if len(case) == 6:
        n, c, h, w, fh, fw = case
        return (n, c, h * fh, w * fw)
    shape, scales, size = case
    oh, ow = size if size is not None else (int(round(scales[0] * shape[2])), int(round(scales[1] * shape[3])))
    return (shape[0], shape[1], oh, ow)


def _run(pa, case, **kw):
    return (_int_case if len(case) == 6 else _frac_case)(pa, case, **kw)


ALL_CASES = INT_CASES + FRAC_CASES


@pytest.mark.parametrize("case", ALL_CASES, ids=[str(c).replace(" ", "") for c in ALL_CASES])
def test_q4_kernels_equal_the_nchw_kernels_bit_for_bit(pa, case):
    raw, c, got, want = _run(pa, case)
    assert_same_bits(got, want, str(case))
    if c % 4:
        assert not padding_lanes(raw, c).any(), "padding lanes are not +0"


def test_integer_factors_through_resize_and_nearest_resize(pa):
    """ResizeQ4 dispatches like layer.Resize: integer scales -> the weight-table kernel; nearest with a zero shift -> the nearest
    Q4 kernel; a shifted nearest pair has no Q4 form."""
    from planer_amd import layer, q4
    x = _rand((2, 5, 3, 5), 5)
    xd = pa.hip.asarray(x)
    k = np.array([1, 1, 2, 3], np.float32)
    for mode, para in (("linear", {}), ("nearest", {}),
                       ("nearest", dict(coordinate_transformation_mode="asymmetric", nearest_mode="floor"))):
        got = q4.from_q4(q4.ResizeQ4(q4.to_q4(xd), EMPTY, k, mode=mode, **para)).get()
        assert_same_bits(got, layer.Resize(xd, EMPTY, k, mode=mode, **para).get(), mode)
    with pytest.raises(NotImplementedError, match="no channel-quad form"):
        q4.ResizeQ4(q4.to_q4(xd), EMPTY, k, mode="nearest", coordinate_transformation_mode="asymmetric", nearest_mode="ceil")
    with pytest.raises(NotImplementedError, match="nearest down-scaling"):
        q4.ResizeQ4(q4.to_q4(xd), EMPTY, np.array([1, 1, 0.5, 2], np.float32), mode="nearest")
    with pytest.raises(NotImplementedError, match="fh \\* fw <= 64"):
        q4.UpSampleQ4(q4.to_q4(xd), np.array([1, 1, 9, 8], np.float32), "linear")
    with pytest.raises(ValueError, match="at least 2 x 2"):
        q4.ResizeQ4(q4.to_q4(pa.hip.asarray(x[:, :, :1])), EMPTY, np.array([1, 1, 1.5, 1.5], np.float32), mode="linear")
    # layer.UpSample truncates its factors: so does the Q4 layer
    kt = np.array([1, 1, 2.9, 2.2], np.float32)
    assert_same_bits(q4.from_q4(q4.UpSampleQ4(q4.to_q4(xd), kt, "linear")).get(), layer.UpSample(xd, kt, mode="linear").get())


RES_CASES = [PARTIAL, TWO_PASS, FRAC_CASES[0], FRAC_CASES[3]]


@pytest.mark.parametrize("case", RES_CASES, ids=[str(c).replace(" ", "") for c in RES_CASES])
def test_fused_residual_equals_upsample_then_add(pa, case):
    """With a `resq` the result is AddQ4 of the unfused result and the residual, bit for bit, on the raw buffers (padding lanes
    included) -- and equals the NCHW upsample followed by layer.Add."""
    from planer_amd import q4
    res = _rand(_out_shape(case), 99)
    raw, c, got, want = _run(pa, case, res=res)
    assert_same_bits(got, want, "fused against NCHW upsample + add")
    raw0, _, _, _ = _run(pa, case)
    plain = pa.hip.asarray(raw0)
    plain.chan = c
    unfused = q4.AddQ4(plain, q4.to_q4(pa.hip.asarray(res))).get()
    assert_same_bits(raw, unfused, "fused against AddQ4 of the unfused result")
    if c % 4:
        assert not padding_lanes(raw, c).any(), "padding lanes are not +0 with a residual"


def test_special_values(pa):
    """NaN, +-inf and denormals planted in single pixels give the NCHW kernels' bits; an all -0 plane gives +0 from the weight-table
    kernel (its chain starts from +0); the lanes of the other channels of the same quads are untouched by them."""
    x = _rand((1, 6, 4, 5), 21)
    x[0, 0, 1, 1] = np.nan
    x[0, 1, 0, 0] = np.inf
    x[0, 2, 3, 4] = -np.inf
    x[0, 3, 2, 2] = np.float32(1e-40)
    x[0, 3, 0, 4] = np.float32(-1e-45)
    x[0, 4] = -0.0
    for case in ((1, 6, 4, 5, 2, 2), (1, 6, 4, 5, 1, 3), ((1, 6, 4, 5), (1.5, 2.25), None)):
        raw, c, got, want = _run(pa, case, x=x)
        assert_same_bits(got, want, str(case))
        assert np.isnan(got[0, 0]).any() and np.isinf(got[0, 1]).any() and np.isinf(got[0, 2]).any()
        assert np.isfinite(got[0, 3:]).all(), "a special value leaked into another channel's lane"
        assert not padding_lanes(raw, c).any()
        if len(case) == 6:
            assert not got[0, 4].view(np.uint32).any(), "an all -0 plane must give +0"
    clean = x.copy()
    clean[0, :3] = _rand((3, 4, 5), 22)
    _, _, got_clean, _ = _run(pa, (1, 6, 4, 5, 2, 2), x=clean)
    _, _, got, _ = _run(pa, (1, 6, 4, 5, 2, 2), x=x)
    assert_same_bits(got[0, 3:], got_clean[0, 3:], "channels 3.. do not depend on channels 0..2")


def test_entry_points_refuse_before_they_launch(pa):
    """Each guard stands before the CtxGuard, before any allocation and before the launch (read in csrc/pointwise.hip): the small
    buffers handed in are unchanged afterwards."""
    lib = pa._lib.load()
    ctx = pa.hip.context()
    xb, yb = pa.hip.zeros((1024,)), pa.hip.zeros((1024,))
    ib = pa.hip.zeros((1024,), np.int32)
    xb.set(np.arange(1024, dtype=np.float32))
    before = (xb.get(), yb.get())
    h, x, y, q = ctx.handle, xb.ptr, yb.ptr, ib.ptr
    tab = (ctypes.c_float * 256)()
    up, rs = lib.pl_upsample_linear_q4_f32, lib.pl_resize_linear_q4_f32
    INVAL, UNSUP = pa._lib.PL_EINVAL, pa._lib.PL_EUNSUPPORTED
    calls = [
        (UNSUP, "upsample: tensor too large", up, (h, x, y, None, 1, 4096, 512, 1024, 2, 1, tab)),                 # 2^30 quads
        (UNSUP, "resize: tensor too large", rs, (h, x, y, None, 1, 4096, 2, 2, 1024, 1024, q, x, q, x)),           # 2^30 quads
        (UNSUP, "fh \\* fw <= 64 supported, got 72", up, (h, x, y, None, 1, 4, 2, 2, 9, 8, tab)),
        (INVAL, "factors 1 x 1 are the identity", up, (h, x, y, None, 1, 4, 2, 2, 1, 1, tab)),
        (INVAL, "bad shape \\(needs H, W >= 2\\)", rs, (h, x, y, None, 1, 4, 1, 4, 3, 6, q, x, q, x)),
        (INVAL, "bad shape \\(needs H, W >= 2\\)", rs, (h, x, y, None, 1, 4, 4, 1, 6, 3, q, x, q, x)),
        (INVAL, "bad shape", up, (h, x, y, None, 1, 0, 2, 2, 2, 2, tab)),
        (INVAL, "16-byte aligned", up, (h, x + 4, y, None, 1, 4, 2, 2, 2, 2, tab)),
        (INVAL, "16-byte aligned", up, (h, x, y + 8, None, 1, 4, 2, 2, 2, 2, tab)),
        (INVAL, "16-byte aligned", up, (h, x, y, x + 4, 1, 4, 2, 2, 2, 2, tab)),
        (INVAL, "16-byte aligned", rs, (h, x + 4, y, None, 1, 4, 2, 2, 3, 3, q, x, q, x)),
        (INVAL, "16-byte aligned", rs, (h, x, y + 12, None, 1, 4, 2, 2, 3, 3, q, x, q, x)),
        (INVAL, "16-byte aligned", rs, (h, x, y, y + 4, 1, 4, 2, 2, 3, 3, q, x, q, x)),
        (INVAL, "cannot run in place", up, (h, x, x, None, 1, 4, 2, 2, 2, 2, tab)),
        (INVAL, "cannot run in place", rs, (h, x, x, None, 1, 4, 2, 2, 3, 3, q, x, q, x)),
        (INVAL, "null argument", up, (h, None, y, None, 1, 4, 2, 2, 2, 2, tab)),
        (INVAL, "null argument", up, (h, x, y, None, 1, 4, 2, 2, 2, 2, None)),
        (INVAL, "null argument", rs, (h, x, None, None, 1, 4, 2, 2, 3, 3, q, x, q, x)),
        (INVAL, "null argument", rs, (h, x, y, None, 1, 4, 2, 2, 3, 3, q, x, None, x)),
    ]
    for code, text, fn, args in calls:
        rc = fn(*args)
        assert rc == code, (fn.__name__, text, rc, lib.pl_last_error())
        with pytest.raises(NotImplementedError if code == UNSUP else ValueError, match=text):
            pa._lib.check(rc)
    ctx.synchronize()
    np.testing.assert_array_equal(xb.get(), before[0])
    np.testing.assert_array_equal(yb.get(), before[1])


def test_kernels_under_pool_hygiene(pa):
    """Every kernel case once more with poisoned, guarded blocks: no guard touched, results unchanged -- so no quad
    of the output is left unwritten and nothing is read that was not written."""
    ctx = pa.hip.context()
    cases = [(c, None) for c in ALL_CASES] + [(c, _rand(_out_shape(c), 99)) for c in RES_CASES]
    normal = [_run(pa, c, res=r) for c, r in cases]
    ctx.synchronize()
    ctx.__dict__.pop("_linear_q4_tables", None)    # the position tables are made again under the mode: their reads are guarded too
    ctx.pool_debug(pa.hip.POOL_GUARD_BYTES, 0xFF)
    try:
        guarded = [_run(pa, c, res=r) for c, r in cases]
        dirty, report = ctx.pool_debug_check()
    finally:
        ctx.pool_debug(0)
    assert dirty == 0, report
    for (case, _), a, b in zip(cases, normal, guarded):
        assert_same_bits(b[0], a[0], "raw Q4 buffer of %s under hygiene" % (case,))
        assert_same_bits(b[2], b[3], "%s under hygiene" % (case,))


# ---- nets ---------------------------------------------------------------------------------------------------------------------
def _small_graph():
    """N x 4 x 12 x 14: conv -> linear x2 -> add(other branch) -> conv (+ that branch again); a fractional resize to (17, 19) feeding
    a conv; a nearest resize feeding a concat."""
    s = Small(seed=5)
    s.g.init("sz", np.array([2, 8, 17, 19], np.int64))
    u0 = s.g.op("upsample", ["x", "scales2"], "x2", name="up0", mode="nearest")
    yb = s.conv(u0, "b", cin=4)
    ya = s.conv("x", "a", cin=4)
    up = s.g.op("upsample", [ya, "scales2"], "u", name="up", mode="linear")
    t = s.g.op("add", [up, yb], "s", name="sum")
    c = s.conv(t, "c")
    c = s.g.op("add", [c, yb], "c2", name="late")
    f = s.g.op("resize", [c, "roi", "none", "sz"], "f", name="to_17x19", mode="linear")
    d = s.conv(f, "d")
    nr = s.g.op("resize", [d, "roi", "scales2"], "nr", name="nearest2", mode="nearest")
    e = s.conv(nr, "e")
    cat = s.g.op("concat", [nr, e], "cat", name="cat", axis=1)
    z = s.conv(cat, "z", cin=16)
    return s.finish(z)


def _oracle(g, b, x):
    ref = onp.OracleNet()
    ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
    ref.load_weights(b)
    return ref(x.copy())


@pytest.fixture(scope="module")
def models():
    from planer_amd.irgen import fpn
    out = {"small": _small_graph() + (_rand((2, 4, 12, 14), 8),)}
    for via in ("upsample", "resize"):
        out["fpn-" + via] = fpn.build(via=via) + (fpn.make_input(2, size=64),)
    return out


@pytest.fixture(scope="module")
def picks():
    """Conv algorithm picks shared by every net of this module: a net times the candidates of a conv shape the shipped database
    does not have, and two nets could come to different picks for the same shape.  Shared, the picks are by shape alone."""
    return {}


def _net(pa, g, b, picks, force=False):
    net = pa.from_graph(g, b)
    if force:
        net.use_q4 = "force"                       # these maps are small: by its cost estimate the plan would stay NCHW
    net._load_algo_cache()
    picks.update({k: v for k, v in net._algo.items() if k not in picks})
    net._algo = picks
    return net


@pytest.fixture(scope="module")
def results(pa, models, picks):
    """name -> (net, net(x)) with the switch at its default."""
    out = {}
    for name, (g, b, x) in models.items():
        net = _net(pa, g, b, picks, force=name == "small")
        out[name] = (net, net(x))
    return out


@pytest.mark.parametrize("name", ["small", "fpn-upsample", "fpn-resize"])
def test_nets_against_the_oracle(pa, models, results, name):
    g, b, x = models[name]
    net, got = results[name]
    want = _oracle(g, b, x)
    assert got.shape == want.shape
    assert_close(got, want, RTOL, name)
    prog, _ = __import__("tests.plan_audit", fromlist=["program"]).program(net, [pa.hip.asarray(x)])
    kinds = [obj.name for obj in prog.objs.values()]
    if name == "small":
        assert "upsample_add_q4" in kinds and kinds.count("resize_q4") == 2 and "resize" not in kinds
        assert "add_q4" not in kinds and "from_q4" in kinds
    else:
        via = name.split("-")[1]
        flow_kinds = [prog.objs[names[0]].name for _, names, _ in prog.flow]
        assert flow_kinds.count(via + "_q4") == 7 and flow_kinds.count(via + "_add_q4") == 2 and net.linear_adds_fused == 2
        assert flow_kinds.count("from_q4") == 1 and flow_kinds.count("to_q4") == 0 and flow_kinds[-2] == via


def test_fpn_through_upsample_and_through_resize_are_equal(results):
    np.testing.assert_array_equal(results["fpn-upsample"][1], results["fpn-resize"][1])


@pytest.mark.parametrize("name", ["small", "fpn-upsample"])
def test_switch_on_equals_switch_off_bit_for_bit(pa, models, results, picks, name, monkeypatch):
    g, b, x = models[name]
    monkeypatch.setenv("PLANER_HIP_LINEAR_Q4", "0")
    net = _net(pa, g, b, picks, force=name == "small")
    off = net(x)
    prog, _ = __import__("tests.plan_audit", fromlist=["program"]).program(net, [pa.hip.asarray(x)])
    kinds = [obj.name for obj in prog.objs.values()]
    assert not any(k in LINEAR_KINDS for k in kinds) and ("upsample" in kinds or "resize" in kinds)
    assert_same_bits(results[name][1], off, "%s: PLANER_HIP_LINEAR_Q4=1 against =0" % name)


@pytest.mark.parametrize("name", ["small", "fpn-upsample", "fpn-resize"])
def test_every_linear_step_equals_the_nchw_layer_on_its_own_inputs(pa, models, results, name):
    from tests.plan_audit import capture, host_inits
    g, b, x = models[name]
    net, got = results[name]
    trace, out = capture(net, [pa.hip.asarray(x)])
    n = check_linear_steps(pa, trace, host_inits(net))
    assert n == (3 if name == "small" else 9), [st.kind for st in trace]
    assert_close(out[0], got, 1e-5, "the traced eager pass against net(x)")


@pytest.mark.parametrize("name", ["small", "fpn-upsample"])
def test_plan_file_replays_the_linear_steps(pa, models, results, name, tmp_path):
    from planer_amd.export import export_plan
    from tests.test_gpu_plan_file import _bind, _run_plan
    g, b, x = models[name]
    net, want = results[name]
    blob = export_plan(net, x)
    assert b"pl_upsample_linear_q4_f32" in blob
    if name == "small":
        assert b"pl_resize_linear_q4_f32" in blob and b"pl_upsample_nearest_q4_f32" in blob
    out, = _run_plan(_bind(), blob, [x])
    np.testing.assert_array_equal(out, want)

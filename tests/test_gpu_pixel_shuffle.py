"""Pixel shuffle / unshuffle on channel-quad (Q4) tensors on a real MI355X: pl_pixel_shuffle_q4_f32 against numpy's own
reshape / transpose / reshape BIT FOR BIT (data movement: no tolerance in any kernel test), padding lanes, refusals, pool hygiene;
and the nets that use it -- the four forms between two convs and tiny EDSRs (planer_amd.irgen.edsr) -- against the oracle, switch
on against switch off, step by step, and from a plan file."""
import numpy as np
import pytest

from oracle import planer_np as onp
from tests.conftest import RTOL, assert_close
from tests.linear_q4_ref import assert_same_bits, padding_lanes
from tests.pixel_shuffle_ref import FORM_IDS, FORMS, out_shape, sandwich, shuffle_np

pytestmark = pytest.mark.gpu
N = 2


def _cases():
    """(inverse, order, r, C, (H, W)) with C, H, W the narrow side's, as the entry point takes them."""
    out = []
    for c in (1, 3, 4, 5, 8):
        for hw in ((6, 10), (4, 134)):               # 134 / 2 = 67 small pixels a row: a row crosses a 64-lane wave
            out.append((False, "crd", 2, c, hw))
    out += [(False, "crd", 3, c, (9, 15)) for c in (3, 4)]    # C = 3: 27 wide channels, a partial wide quad and two absent ones
    out += [(False, "crd", 4, c, (8, 20)) for c in (1, 6)]
    out += [(False, "dcr", 2, c, (6, 10)) for c in (4, 8)] + [(False, "dcr", 3, c, (9, 15)) for c in (4, 8)]
    out += [(True, "crd", 2, 3, (6, 10)), (True, "crd", 2, 4, (6, 10)), (True, "crd", 3, 5, (9, 15)), (True, "crd", 4, 2, (8, 20))]
    out += [(True, "dcr", 2, 4, (6, 10))]
    return out


CASES = _cases()
SHUFFLES = [c for c in CASES if not c[0]]
# 8 quads x 260 x 262 small pixels = 544 960 threads' worth: more than the 524 288 lanes one pass launches on 256 CUs, so the
# stride loop turns twice (the only case with more than a few blocks)
TWO_PASS = (False, "crd", 2, 32, (520, 524))


def _id(case):
    return "%s-%s-r%d-c%d-%dx%d" % (("unshuffle" if case[0] else "shuffle", case[1], case[2], case[3]) + tuple(case[4]))


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _rand(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _in_shape(case, n=N):
    inverse, order, r, c, (h, w) = case
    return (n, c, h, w) if inverse else (n, c * r * r, h // r, w // r)


def _dirty_q4(pa, x):
    """to_q4(x) with every padding lane of the buffer set to 1.0: the kernel must not carry them over."""
    from planer_amd import q4
    raw = q4.to_q4(pa.hip.asarray(x)).get()
    c = x.shape[1]
    for ch in range(c, raw.shape[1] * 4):
        raw[:, ch // 4, :, :, ch % 4] = 1.0
    xq = pa.hip.asarray(raw)
    xq.chan = c
    return xq


def _run(pa, case, nchw_out=False, n=N):
    """-> (result as NCHW, raw Q4 buffer or None, its channel count, numpy's result)."""
    from planer_amd import q4
    inverse, order, r, c, hw = case
    x = _rand(_in_shape(case, n), 1 + r + c + hw[1])
    want = shuffle_np(x, r, order, inverse)
    y = q4.PixelShuffleQ4(_dirty_q4(pa, x), r, order, inverse, nchw_out=nchw_out)
    if nchw_out:
        assert not q4.is_q4(y) and y.shape == want.shape
        return y.get(), None, want.shape[1], want
    assert q4.logical_shape(y) == want.shape
    return q4.from_q4(y).get(), y.get(), want.shape[1], want


@pytest.mark.parametrize("case", CASES + [TWO_PASS], ids=_id)
def test_entry_point_equals_numpy_bit_for_bit(pa, case):
    got, raw, c, want = _run(pa, case, n=1 if case is TWO_PASS else N)
    assert_same_bits(got, want, _id(case))
    assert raw.shape[1] == -(-c // 4)
    assert not padding_lanes(raw, c).any(), "padding lanes are not +0"


@pytest.mark.parametrize("case", SHUFFLES + [TWO_PASS], ids=_id)
def test_shuffle_straight_to_nchw(pa, case):
    got, _, _, want = _run(pa, case, nchw_out=True, n=1 if case is TWO_PASS else N)
    assert_same_bits(got, want, _id(case) + " nchw_out")


def test_nchw_out_leaves_the_bytes_behind_the_tensor_alone(pa):
    """C = 3 has a padding lane per quad: with nchw_out it has no place in the result, so nothing may be written for it."""
    lib = pa._lib.load()
    ctx = pa.hip.context()
    case = (False, "crd", 2, 3, (6, 10))
    x = _rand(_in_shape(case), 4)
    want = shuffle_np(x, 2)
    ybuf = pa.hip.zeros((want.size + 256,))
    ybuf.set(np.full(want.size + 256, 7.0, np.float32))
    pa._lib.check(lib.pl_pixel_shuffle_q4_f32(ctx.handle, _dirty_q4(pa, x).ptr, ybuf.ptr, N, 3, 6, 10, 2, 0, 0, 1))
    got = ybuf.get()
    assert_same_bits(got[:want.size].reshape(want.shape), want)
    assert (got[want.size:] == 7.0).all()


def test_special_values_are_moved_as_bits(pa):
    from planer_amd import q4
    x = _rand((1, 12, 3, 5), 6)
    x[0, 0, 0, 0], x[0, 5, 1, 1], x[0, 7, 2, 4], x[0, 9, 0, 3], x[0, 11, 2, 2] = np.nan, np.inf, -np.inf, -0.0, np.float32(1e-45)
    got = q4.from_q4(q4.PixelShuffleQ4(_dirty_q4(pa, x), 2)).get()
    want = shuffle_np(x, 2)
    assert_same_bits(got, want)
    assert np.signbit(got[want == 0]).all() and (got.view(np.uint32) == 1).sum() == 1


def test_entry_point_refuses_before_it_launches(pa):
    """Each guard stands before the CtxGuard and the launch (read in csrc/pointwise.hip): the small buffers handed in are
    unchanged afterwards, so the size refusals need no tensor of that size."""
    lib = pa._lib.load()
    ctx = pa.hip.context()
    xb, yb = pa.hip.zeros((4096,)), pa.hip.zeros((4096,))
    xb.set(np.arange(4096, dtype=np.float32))
    before = (xb.get(), yb.get())
    h, x, y = ctx.handle, xb.ptr, yb.ptr
    ps = lib.pl_pixel_shuffle_q4_f32
    INVAL, UNSUP = pa._lib.PL_EINVAL, pa._lib.PL_EUNSUPPORTED
    big = 2 ** 31 - 2
    calls = [
        (UNSUP, "r = 2, 3, 4 supported, got 5", (h, x, y, 1, 4, 10, 10, 5, 0, 0, 0)),
        (UNSUP, "r = 2, 3, 4 supported, got 1", (h, x, y, 1, 4, 10, 10, 1, 0, 0, 0)),
        (UNSUP, "DCR order needs C % 4 == 0, got C = 6", (h, x, y, 1, 6, 4, 4, 2, 1, 0, 0)),
        (UNSUP, "DCR order needs C % 4 == 0, got C = 6", (h, x, y, 1, 6, 4, 4, 2, 1, 1, 0)),
        (INVAL, "not an in-place operation", (h, x, x, 1, 4, 4, 4, 2, 0, 0, 0)),
        (INVAL, "16-byte aligned", (h, x + 4, y, 1, 4, 4, 4, 2, 0, 0, 0)),
        (INVAL, "16-byte aligned", (h, x, y + 8, 1, 4, 4, 4, 2, 0, 1, 0)),
        (INVAL, "16-byte aligned", (h, x, y + 4, 1, 4, 4, 4, 2, 0, 0, 1)),
        (INVAL, "nchw_out goes with a shuffle", (h, x, y, 1, 4, 4, 4, 2, 0, 1, 1)),
        (INVAL, "multiples of r", (h, x, y, 1, 4, 5, 4, 2, 0, 0, 0)),
        (INVAL, "multiples of r", (h, x, y, 1, 4, 6, 8, 3, 0, 1, 0)),
        (INVAL, "order is 0 \\(CRD\\) or 1 \\(DCR\\)", (h, x, y, 1, 4, 4, 4, 2, 2, 0, 0)),
        (INVAL, "bad shape", (h, x, y, 1, 0, 4, 4, 2, 0, 0, 0)),
        (INVAL, "null argument", (h, None, y, 1, 4, 4, 4, 2, 0, 0, 0)),
        (INVAL, "null argument", (h, x, None, 1, 4, 4, 4, 2, 0, 0, 0)),
        # 2^29 quads on the narrow side (the wide side has as many); one quad less on the wide side of a partial quad; factors
        # whose product leaves 64 bits
        (UNSUP, "2\\^29 pixel quads", (h, x, y, 1, 4096, 1024, 512, 2, 0, 0, 0)),
        (UNSUP, "2\\^29 pixel quads", (h, x, y, 1, 4096, 1024, 512, 2, 1, 1, 0)),
        (UNSUP, "2\\^29 pixel quads", (h, x, y, 2, 4096, 512, 512, 4, 0, 0, 1)),
        (UNSUP, "2\\^29 pixel quads", (h, x, y, big, big, big, big, 2, 0, 0, 0)),
        (UNSUP, "2\\^29 pixel quads", (h, x, y, 65536, 2, 65536 * 3, 3, 3, 0, 1, 0)),
    ]
    for code, text, args in calls:
        rc = ps(*args)
        assert rc == code, (text, rc, lib.pl_last_error())
        with pytest.raises(NotImplementedError if code == UNSUP else ValueError, match=text):
            pa._lib.check(rc)
    ctx.synchronize()
    np.testing.assert_array_equal(xb.get(), before[0])
    np.testing.assert_array_equal(yb.get(), before[1])


def test_layer_functions_refuse_what_has_no_form(pa):
    from planer_amd import layer, q4
    xq = q4.to_q4(pa.hip.asarray(_rand((1, 24, 4, 4), 2)))
    with pytest.raises(NotImplementedError, match="DCR order needs"):
        q4.PixelShuffleQ4(xq, 2, "dcr")
    with pytest.raises(ValueError, match="does not fit"):
        q4.PixelShuffleQ4(xq, 3)
    with pytest.raises(ValueError, match="nchw_out goes with a shuffle"):
        q4.PixelShuffleQ4(xq, 2, inverse=True, nchw_out=True)
    with pytest.raises(TypeError):
        q4.PixelShuffleQ4(pa.hip.asarray(_rand((1, 24, 4, 4), 2)), 2)
    folded = q4.refold_q4(xq, 2, 2)
    with pytest.raises(ValueError, match="folded"):
        q4.PixelShuffleQ4(folded, 2)
    # the NCHW kind is the trio on pl_transpose_f32, DCR with any channel count included
    x = _rand((2, 24, 3, 5), 3)
    for order in ("crd", "dcr"):
        y = layer.PixelShuffle(pa.hip.asarray(x), 2, order)
        assert_same_bits(y.get(), shuffle_np(x, 2, order))
        assert_same_bits(layer.PixelShuffle(y, 2, order, inverse=True).get(), x)


def test_kernel_under_pool_hygiene(pa):
    """Poisoned, guarded blocks: guards intact, result equal in bits, and the padding lanes zero although the output
    block came filled with 0xFF -- so every lane of the output is written and no absent wide quad is touched."""
    ctx = pa.hip.context()
    cases = [((False, "crd", 3, 3, (9, 15)), False), ((True, "crd", 2, 3, (6, 10)), False), ((False, "crd", 3, 3, (9, 15)), True)]
    ctx.synchronize()
    ctx.pool_debug(pa.hip.POOL_GUARD_BYTES, 0xFF)
    try:
        guarded = [_run(pa, c, nchw_out=o) for c, o in cases]
        dirty, report = ctx.pool_debug_check()
    finally:
        ctx.pool_debug(0)
    assert dirty == 0, report
    for (case, nchw_out), (got, raw, c, want) in zip(cases, guarded):
        assert_same_bits(got, want, "%s under hygiene" % _id(case))
        if raw is not None:
            assert not padding_lanes(raw, c).any(), "padding lanes under hygiene"


# ---- nets ---------------------------------------------------------------------------------------------------------------------
TINY = dict(blocks=2, feats=8, size=12)
EDSRS = {"edsr-x2": dict(scale=2), "edsr-x3": dict(scale=3), "edsr-x4": dict(scale=4), "edsr-shuffle-tail": dict(scale=4, tail="shuffle"),
         "edsr-unshuffle-in": dict(scale=2, unshuffle_in=True)}
# name -> pixelshuffle_q4 steps of the plan
NETS = dict({fid: 1 for fid in FORM_IDS}, **{"edsr-x2": 1, "edsr-x3": 1, "edsr-x4": 2, "edsr-shuffle-tail": 1, "edsr-unshuffle-in": 1})


def _oracle(g, b, x):
    ref = onp.OracleNet()
    ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
    ref.load_weights(b)
    return ref(x.copy())


@pytest.fixture(scope="module")
def models():
    from planer_amd.irgen import edsr
    out = {}
    for fid, (order, inverse) in zip(FORM_IDS, FORMS):
        out[fid] = sandwich(order, inverse, r=2, hw=(6, 8)) + (_rand((N, 4, 6, 8), 8),)
    for name, opts in EDSRS.items():
        out[name] = edsr.build(**TINY, **opts) + (edsr.make_input(N, size=TINY["size"]),)
    return out


@pytest.fixture(scope="module")
def picks():
    """Conv algorithm picks shared by every net of this module, so that a shape is run by one kernel whichever net has it."""
    return {}


def _net(pa, g, b, picks):
    net = pa.from_graph(g, b)
    net.use_q4 = "force"                           # these maps are small: by its cost estimate the plan would stay NCHW
    net._load_algo_cache()
    picks.update({k: v for k, v in net._algo.items() if k not in picks})
    net._algo = picks
    return net


@pytest.fixture(scope="module")
def results(pa, models, picks):
    """name -> (net, net(x)) with the switch at its default."""
    out = {}
    for name, (g, b, x) in models.items():
        net = _net(pa, g, b, picks)
        out[name] = (net, net(x))
    return out


def _flow_kinds(pa, net, x):
    prog, _ = __import__("tests.plan_audit", fromlist=["program"]).program(net, [pa.hip.asarray(x)])
    return [prog.objs[names[0]].name for _, names, _ in prog.flow]


@pytest.mark.parametrize("name", list(NETS))
def test_nets_against_the_oracle(pa, models, results, name):
    g, b, x = models[name]
    net, got = results[name]
    want = _oracle(g, b, x)
    assert got.shape == want.shape
    assert_close(got, want, RTOL, name)
    kinds = _flow_kinds(pa, net, x)
    assert kinds.count("pixelshuffle_q4") == NETS[name] and "transpose" not in kinds and "reshape" not in kinds
    assert kinds.count("pixelshuffle") == (1 if name == "edsr-unshuffle-in" else 0)
    assert net.pixel_shuffles_fused == NETS[name] + kinds.count("pixelshuffle")
    assert kinds.count("from_q4") == (0 if name == "edsr-shuffle-tail" else 1)


@pytest.mark.parametrize("name", list(NETS))
def test_switch_on_equals_switch_off_bit_for_bit(pa, models, results, picks, name, monkeypatch):
    g, b, x = models[name]
    monkeypatch.setenv("PLANER_HIP_PIXEL_SHUFFLE_Q4", "0")
    net = _net(pa, g, b, picks)
    off = net(x)
    kinds = _flow_kinds(pa, net, x)
    assert "pixelshuffle_q4" not in kinds and "pixelshuffle" not in kinds and "transpose" in kinds and net.pixel_shuffles_fused == 0
    assert_same_bits(results[name][1], off, "%s: PLANER_HIP_PIXEL_SHUFFLE_Q4=1 against =0" % name)


@pytest.mark.parametrize("name", list(NETS))
def test_every_pixelshuffle_q4_step_equals_the_nchw_layer_on_its_own_input(pa, models, results, name):
    from planer_amd import layer
    from tests.plan_audit import capture, nchw
    g, b, x = models[name]
    net, got = results[name]
    trace, out = capture(net, [pa.hip.asarray(x)])
    n = 0
    for st in trace:
        if st.kind != "pixelshuffle_q4":
            continue
        para = {k: v for k, v in st.para.items() if k != "nchw_out"}
        want = layer.PixelShuffle(pa.hip.asarray(nchw(st.ins[0])), **para)
        assert_same_bits(nchw(st.outs[0]), want.get(), "%s (%s)" % (st.name, st.para))
        n += 1
    assert n == NETS[name], [st.kind for st in trace]
    assert_close(out[0], got, 1e-5, "the traced eager pass against net(x)")


def test_plan_file_replays_the_shuffle(pa, models, results):
    from planer_amd.export import export_plan
    from tests.test_gpu_plan_file import _bind, _run_plan
    g, b, x = models["edsr-x2"]
    net, want = results["edsr-x2"]
    blob = export_plan(net, x)
    assert b"pl_pixel_shuffle_q4_f32" in blob and b"pl_transpose_f32" not in blob
    out, = _run_plan(_bind(), blob, [x])
    assert_same_bits(out, want, "plan file against net(x)")

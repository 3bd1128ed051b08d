"""The F(4,3) Winograd conv kernels against float64 bit for bit, on a real MI355X.

Operands (tests/ref64.py, `wino_exact_operands`): filters whose nonzero taps are +-576 = +-24^2, integer inputs.  The filter kernels
apply G in two stages with every product rounded on its own, and fl(1/6), fl(1/12), fl(1/24), fl(1/3), fl(2/3) are each off by
exactly 2^-25 -- less than half an ulp -- so fl(c) * (24 m) is the integer 24 m c: U = G g G^T is integer.  B^T and A^T are integer
matrices; where the pipeline in absolute values stays below 2^24 (`wino_exact_assert`, asserted for every case) every partial
sum in ANY order is an integer below 2^24, hence exact.  So every form of every kernel of the family -- the fused kernel (w_layout
9: 16-tile blocks woven and phased, 32-tile blocks, packed and plain), the one-call and staged pipeline (w_layout 7, both LDS
modes, the filter-stationary GEMM, the full-tile transform kernels), the chain kernels, the 1-D kernel (w_layout 8), the mixed tiles
(w_layout 11), and all of them through the plan compiler -- must equal `ref64`, and therefore each other, in every bit, under the
eight tails of tests/test_gpu_conv_exact.py.  Every comparison of a conv output here is
np.testing.assert_array_equal(y.astype(float64), ref64(...)); each case asserts the plan string it expects; the geometries the
fused kernel refuses must raise NotImplementedError and are counted against what `_patch_cells` predicts.

One comparison is not exact everywhere, by arithmetic and not by kernel: the chain kernels' second output V2 = B^T y1 B.  y1
carries the tail's grain -- quarters behind a BN, 1/8 of that behind a leaky ReLU -- so an element of V2 is exact in any order only
where (|B^T| |y1| |B|) / grain < 2^24 at that element.  That holds for every element under six of the eight tails and for most
under BN + leaky ReLU; the elements where it does not are held to 8 u (|B^T| |y1| |B|), the transform's own rounding (two passes,
at most four roundings a term, tests/test_gpu_conv_bounds.py), and every other element exactly.  y1 itself is exact under every tail.

The last test asserts what the module reached.  No form turned out inexact: none is held to a looser bound."""
import functools
import time
import zlib

import numpy as np
import pytest

from tests import ref64 as R
from tests.ref64 import ACT_LEAKY, ACT_RELU
from tests.test_gpu_conv_exact import TAILS
from tests.test_gpu_wf4 import _patch_cells

pytestmark = pytest.mark.gpu

# (N, Cin, H, W, Cout)
LADDER = [(2, c, 8, 8, 64) for c in (4, 8, 12, 16, 20)]                      # one to five K chunks of the fused kernel
EDGES = [(1, 8, h, w, 8) for h in (5, 6, 7, 8) for w in (5, 6, 7, 8)]         # rows and columns fall off the map one at a time
PARTIAL, TWO_BLOCKS, PACKED, BIG = (2, 8, 8, 8, 40), (2, 16, 28, 28, 128), (8, 8, 56, 56, 64), (8, 64, 56, 56, 128)
WF4_SHAPES = LADDER + [PARTIAL, TWO_BLOCKS] + EDGES + [(1, 4, 1, 1, 4), (1, 8, 13, 17, 40), (5, 20, 3, 17, 24), (33, 4, 2, 2, 4),
                                                       PACKED, (1, 8, 70, 66, 8)]
WF4_FORMS = ["wf4_half=1", "wf4_half=0", "wf4_weave=0", "wf4_pack=0"]
WIDE = [(2, 128, 8, 8, 128), (1, 128, 14, 14, 128), (1, 256, 7, 7, 16)]
W7_SHAPES = [LADDER[0], LADDER[4], (1, 4, 1, 1, 4), (1, 8, 13, 17, 40), (3, 16, 7, 14, 32), (5, 20, 3, 17, 24), TWO_BLOCKS] + WIDE
CHAIN_SHAPES = [(2, 8, 8, 8, 8), (1, 8, 13, 17, 40), (3, 16, 7, 14, 32), (2, 16, 14, 14, 16), (2, 16, 28, 28, 128), WIDE[0], WIDE[1]]
CHAIN43_SHAPES = [(3, 16, 7, 14, 32), (2, 16, 14, 14, 16), (2, 8, 7, 7, 12), WIDE[1], WIDE[2]]
W8_SHAPES = [LADDER[1], LADDER[4], (1, 8, 13, 17, 40), (5, 20, 3, 17, 24), (1, 8, 6, 5, 8), (3, 16, 7, 14, 32), TWO_BLOCKS] + WIDE
W11_SHAPES = [(3, 16, 7, 14, 32), (2, 16, 14, 14, 16), (2, 8, 7, 7, 12), (1, 8, 21, 14, 8), WIDE[1], WIDE[2]]
W11_REFUSED = [(2, 16, 28, 28, 128)]             # the mixed-tile kernels take sides of 7, 14 and 21: a 28-pixel map is refused
NET_SHAPE = (16, 16, 14, 14, 16)                 # 64 tile columns per mixed-tile GEMM: the plan compiler offers all four layouts
FOLD_SIDES = [8, 7, 16, 14]                      # dilation 2: phases of 4 x 4 (whole and zero-filled), 8 x 8 and 7 x 7
# every (shape, families whose precondition it must meet), for tests/test_conv_ref64.py
FAMILIES = {}
for _s in WF4_SHAPES + W7_SHAPES + CHAIN_SHAPES + [BIG, NET_SHAPE] + [(2, 16, s, s, 16) for s in FOLD_SIDES]:
    FAMILIES.setdefault(_s, set()).add("f4x4")
for _s in W8_SHAPES + [NET_SHAPE]:
    FAMILIES.setdefault(_s, set()).add("w1d4")
for _s in W11_SHAPES + CHAIN43_SHAPES + [NET_SHAPE]:
    FAMILIES.setdefault(_s, set()).add("wino43")

# what the module reached (test_zz_coverage_and_times)
REACHED = {"plans": set(), "lds": set(), "layouts": set(), "net_layouts": set(), "entries": set(), "refused": [], "predicted": [],
           "folds": set(), "times": {}}
PAD1 = dict(pads=[1, 1, 1, 1])


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    REACHED["times"][request.node.name] = time.perf_counter() - t0


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


def _dev(pa, a):
    return None if a is None else pa.asarray(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def operands(shape):
    """The exact operands of a shape with the full tail, drawn once -> (x, K, B, scale, shift, res)."""
    n, cin, h, w, cout = shape
    rng = np.random.default_rng(zlib.crc32(repr(("wino-exact", shape)).encode()))
    return R.wino_exact_operands(rng, (n, cin, h, w), cout, True, True, True)


@functools.lru_cache(maxsize=None)
def _conv(shape):
    """The float64 conv of a shape's operands, computed once and shared by every tail and form (read only)."""
    x, K = operands(shape)[:2]
    y = R.conv64(x, K, **PAD1)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def _precondition(shape, fam):
    R.wino_exact_assert(fam, *operands(shape))
    return True


def _tail(shape, tail):
    """-> ((B, scale, shift, res) of this tail, act, want)"""
    bias, bn, res, act = tail
    _, _, B, sc, sh, r = operands(shape)
    t = (B if bias else None, sc if bn else None, sh if bn else None, r if res else None)
    return t, act, R.tail64(_conv(shape), *t, act, R.ALPHA)


class Device:
    """A shape's operands on the device, uploaded once per test."""

    def __init__(self, pa, shape, fam):
        from planer_amd import q4
        assert _precondition(shape, fam)
        x, K, B, sc, sh, r = operands(shape)
        self.shape, self.pa = shape, pa
        self.xq, self.K = q4.to_q4(_dev(pa, x)), _dev(pa, K)
        self.B, self.sc, self.sh, self.rq = _dev(pa, B), _dev(pa, sc), _dev(pa, sh), q4.to_q4(_dev(pa, r))

    def tail(self, tail):
        """-> (device (B, scale, shift, res) of this tail, keyword arguments of the activation, want)"""
        bias, bn, res, act = tail
        _, _, want = _tail(self.shape, tail)
        return ((self.B if bias else None, self.sc if bn else None, self.sh if bn else None, self.rq if res else None),
                dict(act=act, alpha=R.ALPHA), want)


def _exact(y, want, what, plan=""):
    y = np.asarray(y)
    assert y.shape == want.shape, (what, plan, y.shape, want.shape)
    np.testing.assert_array_equal(y.astype(np.float64), want, err_msg="%s [%s]" % (what, plan))


def _plan(pa, layout=None):
    plan = pa.hip.context().last_conv_plan()
    REACHED["plans"].add(plan)
    if layout is not None:
        REACHED["layouts"].add(layout)
    return plan


# ---- the fused kernel, w_layout 9 --------------------------------------------------------------------------------------------
def _wf4_refused(shape, form):
    """Does wf4_launch decline the geometry?  One block's input patch against its LDS buffer (tests/test_gpu_wf4.py)."""
    tiles, cells = (32, 1024) if form == "wf4_half=0" else (16, 512)
    return _patch_cells(shape[2], shape[3], tiles) > cells


def _wf4_plan_ok(shape, form, plan):
    assert plan.startswith("wf4 64co x "), plan
    assert ("32tiles" in plan) == (form == "wf4_half=0") and ("16tiles" in plan) == (form != "wf4_half=0"), (form, plan)
    assert ("woven" in plan) == (form in ("wf4_half=1", "wf4_pack=0")), (form, plan)
    if shape == PACKED:
        assert ("packed" in plan) == (form != "wf4_pack=0"), (form, plan)
    if shape == TWO_BLOCKS and form != "wf4_half=0":
        # two images x one tile row x eight tile columns: seven row blocks x two channel blocks
        assert "(2x1x8)" in plan and "blocks=14" in plan, (form, plan)


@pytest.mark.parametrize("shape", WF4_SHAPES, ids=_ids(WF4_SHAPES))
def test_fused_kernel_every_form_and_tail(pa, shape, monkeypatch):
    from planer_amd import q4
    dev = Device(pa, shape, "f4x4")
    u = q4.prepare_wf4_q4_weights(dev.K)
    for form in WF4_FORMS:
        monkeypatch.setenv("PLANER_HIP_EXPERIMENT", form)
        refused = _wf4_refused(shape, form)
        for t, tail in enumerate(TAILS):
            dt, kw, want = dev.tail(tail)
            call = lambda: q4.ConvQ4(dev.xq, u, *dt, w_layout=9, **PAD1, **kw)
            REACHED["predicted"].append((shape, form, t, refused))
            try:
                yq = call()
            except NotImplementedError:
                REACHED["refused"].append((shape, form, t))
                assert refused, "refused, not predicted: %s %s tail %d" % (shape, form, t)
                continue
            assert not refused, "predicted to be refused: %s %s tail %d [%s]" % (shape, form, t, _plan(pa))
            plan = _plan(pa, 9)
            _wf4_plan_ok(shape, form, plan)
            assert q4.logical_shape(yq) == (shape[0], shape[4]) + shape[2:4]
            _exact(q4.from_q4(yq).get(), want, "wf4 %s %s tail %d" % (shape, form, t), plan)


@pytest.mark.parametrize("shape", [TWO_BLOCKS, PACKED], ids=_ids([TWO_BLOCKS, PACKED]))
@pytest.mark.parametrize("form", WF4_FORMS)
def test_fused_kernel_four_launches_back_to_back(pa, shape, form, monkeypatch):
    """Four launches with no host synchronisation between them, each into its own output buffer: all four equal the reference (a
    block that reads what a neighbouring launch left in LDS or in flight shows here)."""
    from planer_amd import q4
    dev = Device(pa, shape, "f4x4")
    u = q4.prepare_wf4_q4_weights(dev.K)
    dt, kw, want = dev.tail((True, True, True, ACT_RELU))
    monkeypatch.setenv("PLANER_HIP_EXPERIMENT", form)
    ys = [q4.ConvQ4(dev.xq, u, *dt, w_layout=9, **PAD1, **kw) for _ in range(4)]
    plan = _plan(pa, 9)
    _wf4_plan_ok(shape, form, plan)
    assert len({y.ptr for y in ys}) == 4
    for i, yq in enumerate(ys):                          # (stops at the first mismatch)
        _exact(q4.from_q4(yq).get(), want, "wf4 %s %s launch %d of 4" % (shape, form, i), plan)


# ---- the one-call and staged pipeline, w_layout 7 ------------------------------------------------------------------------------
def _pipeline(pa, dev, lds, what, expect=None):
    """One-call conv and In -> Gemm -> Out under every tail, against float64."""
    from planer_amd import q4
    n, cin, h, w, cout = dev.shape
    u = q4.prepare_winograd4_q4_weights(dev.K)
    for t, tail in enumerate(TAILS):
        dt, kw, want = dev.tail(tail)
        yq = q4.ConvQ4(dev.xq, u, *dt, w_layout=7, **PAD1, **kw)
        plan = _plan(pa, 7)
        assert plan.startswith("wino4["), plan
        if expect is not None:
            assert plan.startswith("wino4[as128x32") == expect, (expect, plan)
        _exact(q4.from_q4(yq).get(), want, "one-call %s lds %s tail %d" % (what, lds, t), plan)
        v = q4.Wino4In(dev.xq)
        m = q4.Wino4Gemm(v, u)
        plan = _plan(pa)
        assert plan.startswith("wino4[") and v.meta == (n, cin, h, w) and m.meta == (n, cout, h, w), plan
        got = q4.Wino4Out(m, *dt, **kw)
        _exact(q4.from_q4(got).get(), want, "staged %s lds %s tail %d" % (what, lds, t), plan)
    REACHED["lds"].add(lds)


@pytest.mark.parametrize("lds", ["1", "2"], ids=["register-transforms", "lds-transforms"])
@pytest.mark.parametrize("shape", W7_SHAPES, ids=_ids(W7_SHAPES))
def test_one_call_and_staged_pipeline(pa, shape, lds, monkeypatch):
    monkeypatch.setenv("PLANER_HIP_WINO_LDS", lds)
    monkeypatch.delenv("PLANER_HIP_WINO_GEMM_AS", raising=False)
    _pipeline(pa, Device(pa, shape, "f4x4"), lds, str(shape))


@pytest.mark.parametrize("lds", ["1", "2"], ids=["register-transforms", "lds-transforms"])
@pytest.mark.parametrize("gemm_as", ["0", "1"], ids=["tile-gemm", "filter-stationary-gemm"])
def test_pipeline_on_both_gemms_at_128_channels(pa, gemm_as, lds, monkeypatch):
    monkeypatch.setenv("PLANER_HIP_WINO_LDS", lds)
    monkeypatch.setenv("PLANER_HIP_WINO_GEMM_AS", gemm_as)
    _pipeline(pa, Device(pa, WIDE[0], "f4x4"), lds, "%s gemm_as %s" % (WIDE[0], gemm_as), expect=gemm_as == "1")


def test_pipeline_on_the_full_tile_transform_kernels(pa, monkeypatch):
    """conv_winograd.hip takes the row-split transform kernels where ceil(Cin T / 256) < CUs (input) and ceil(Cout/4 T / 256) <
    CUs / 2 (output); this shape is above both on this device, so the full-tile kernels run (register transforms: LDS mode 1)."""
    n, cin, h, w, cout = BIG
    cus = pa.hip.context().cu_count
    T = n * -(-h // 4) * -(-w // 4)
    assert -(-cin * T // 256) >= cus and -(-(cout // 4) * T // 256) >= cus // 2, (cus, T)
    monkeypatch.setenv("PLANER_HIP_WINO_LDS", "1")
    monkeypatch.delenv("PLANER_HIP_WINO_ROWS", raising=False)
    _pipeline(pa, Device(pa, BIG, "f4x4"), "1", str(BIG))


# ---- the chain kernels -----------------------------------------------------------------------------------------------------------
def _grain(tail):
    bias, bn, res, act = tail
    return (0.25 if bn else 1.0) * (R.ALPHA if act & 15 == ACT_LEAKY else 1.0)


def _v2_check(v2, y1, tail, transform, what):
    """V2 = B^T y1 B against float64: exact wherever (|B^T| |y1| |B|) / grain < 2^24 at the element (every partial sum of the
    element is then a multiple of the grain below 2^24 grains), within 8 u (|B^T| |y1| |B|) elsewhere (module docstring)."""
    want = transform(y1)
    mag = transform(np.abs(y1), True)
    got = v2.get()[:want.size].reshape(want.shape).astype(np.float64)
    exact = mag / _grain(tail) < R.WINO_CAP
    bn_leaky = tail[1] and tail[3] & 15 == ACT_LEAKY
    assert exact.all() or bn_leaky, "%s: %d elements above the cap" % (what, (~exact).sum())
    assert exact.mean() > 0.5, (what, exact.mean())
    np.testing.assert_array_equal(got[exact], want[exact], err_msg=what)
    assert (np.abs(got - want)[~exact] <= 8 * R.U * mag[~exact]).all(), what


def _wino4_in64(y, absolute=False):
    return R.wino4_input(y, np.abs(R._F[4][0]) if absolute else None)


def _chain(pa, shape, fam, prep, win, gemm, chain, transform, entry):
    from planer_amd import q4
    dev = Device(pa, shape, fam)
    u = prep(dev.K)
    for t, tail in enumerate(TAILS):
        dt, kw, want = dev.tail(tail)
        for keep in (True, False):
            m1 = gemm(win(dev.xq), u)
            plan = _plan(pa)
            out = chain(m1, *dt, keep_y=keep, **kw)
            y1, v2 = out if keep else (None, out)
            what = "%s %s tail %d keep_y=%s" % (entry, shape, t, keep)
            if keep:
                _exact(q4.from_q4(y1).get(), want, "y1 " + what, plan)
            _v2_check(v2, want, tail, transform, "V2 " + what)
    REACHED["entries"].add(entry)


@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=_ids(CHAIN_SHAPES))
def test_wino4_chain(pa, shape):
    from planer_amd import q4
    n, cin, h, w, cout = shape
    assert q4.wino4_chain_supported((n, cout, h, w), pa.hip.context()), shape
    _chain(pa, shape, "f4x4", q4.prepare_winograd4_q4_weights, q4.Wino4In, q4.Wino4Gemm, q4.Wino4Chain, _wino4_in64,
           "pl_wino4_chain_q4_f32")


@pytest.mark.parametrize("shape", CHAIN43_SHAPES, ids=_ids(CHAIN43_SHAPES))
def test_wino43_chain(pa, shape):
    from planer_amd import q4
    _chain(pa, shape, "wino43", q4.prepare_winograd43_q4_weights, q4.Wino43In, q4.Wino43Gemm, q4.Wino43Chain, R.wino43_input,
           "pl_wino43_chain_q4_f32")


# ---- w_layout 8 and 11 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", W8_SHAPES, ids=_ids(W8_SHAPES))
def test_one_dimensional_f43(pa, shape):
    from planer_amd import q4
    dev = Device(pa, shape, "w1d4")
    u = q4.prepare_w1d4_q4_weights(dev.K)
    for t, tail in enumerate(TAILS):
        dt, kw, want = dev.tail(tail)
        yq = q4.ConvQ4(dev.xq, u, *dt, w_layout=8, **PAD1, **kw)
        plan = _plan(pa, 8)
        assert plan.startswith("w1d4 "), plan
        _exact(q4.from_q4(yq).get(), want, "w1d4 %s tail %d" % (shape, t), plan)


@pytest.mark.parametrize("lds", ["1", "0"], ids=["lds-transforms", "whole-tile-transforms"])
@pytest.mark.parametrize("shape", W11_SHAPES, ids=_ids(W11_SHAPES))
def test_mixed_tiles(pa, shape, lds, monkeypatch):
    from planer_amd import q4
    monkeypatch.setenv("PLANER_HIP_WINO43_LDS", lds)
    dev = Device(pa, shape, "wino43")
    u = q4.prepare_winograd43_q4_weights(dev.K)
    for t, tail in enumerate(TAILS):
        dt, kw, want = dev.tail(tail)
        yq = q4.ConvQ4(dev.xq, u, *dt, w_layout=11, **PAD1, **kw)
        plan = _plan(pa, 11)
        assert plan.startswith("wino43["), plan
        _exact(q4.from_q4(yq).get(), want, "wino43 %s lds %s tail %d" % (shape, lds, t), plan)
        got = q4.Wino43Out(q4.Wino43Gemm(q4.Wino43In(dev.xq), u), *dt, **kw)
        _exact(q4.from_q4(got).get(), want, "wino43 staged %s lds %s tail %d" % (shape, lds, t), plan)


@pytest.mark.parametrize("shape", W11_REFUSED, ids=_ids(W11_REFUSED))
def test_mixed_tiles_refuse_a_28_pixel_map(pa, shape):
    """7 | 28, but the mixed-tile kernels are built for 1, 2 or 3 tiles of 7 a side: refused, never computed."""
    from planer_amd import q4
    n, cin, h, w, cout = shape
    x, K = operands(shape)[:2]
    assert not q4.winograd43_eligible((n, cin, h, w), K.shape, strides=(1, 1), pads=(1, 1, 1, 1))
    with pytest.raises((ValueError, NotImplementedError)):
        q4.ConvQ4(q4.to_q4(_dev(pa, x)), q4.prepare_winograd43_q4_weights(_dev(pa, K)), w_layout=11, **PAD1)
    with pytest.raises((ValueError, NotImplementedError)):
        q4.Wino43In(q4.to_q4(_dev(pa, x)))


# ---- through the plan compiler -----------------------------------------------------------------------------------------------------
def fold_phases(shape, d=2):
    """The d x d pixel phases of a shape's input, each zero-filled to ceil(H/d) x ceil(W/d): the images of the folded tensor."""
    x = operands(shape)[0]
    n, c, h, w = x.shape
    for i in range(d):
        for j in range(d):
            ph = np.zeros((n, c, -(-h // d), -(-w // d)), np.float32)
            sub = x[:, :, i::d, j::d]
            ph[:, :, :sub.shape[2], :sub.shape[3]] = sub
            yield ph


def _one_conv_net(pa, shape, dilation=1):
    """relu -> conv 3x3 -> batchnorm -> add(the conv's input) -> relu on the exact operands -> (graph, blob, x, want)"""
    from planer_amd.irgen.builder import GraphBuilder
    n, c, h, w, cout = shape
    assert c == cout
    x, K, _, sc, sh, _ = operands(shape)
    d = int(dilation)
    gb = GraphBuilder(["x"])
    gb.init("K", K)
    gb.init("s", sc.reshape(1, c, 1, 1))
    gb.init("t", sh.reshape(1, c, 1, 1))
    gb.op("relu", ["x"], "x0", name="r0")
    gb.op("conv", ["x0", "K"], "c1", name="c1", group=1, strides=[1, 1], dilations=[d, d], pads=[d, d, d, d])
    gb.op("batchnorm", ["c1", "s", "t"], "b1", name="b1")
    gb.op("add", ["b1", "x0"], "a1", name="a1")
    gb.op("relu", ["a1"], "r1", name="r1")
    g, blob = gb.finish(["r1"])
    x0 = np.maximum(x, 0)
    want = R.ref64(x0, K, None, sc, sh, x0, ACT_RELU, dilations=[d, d], pads=[d, d, d, d])
    return g, blob, x, want


def _run_net(pa, g, blob, x, lay):
    net = pa.from_graph(g, blob)
    net.force_algo, net.streams, net.use_q4 = lay, "1x1", "force"
    y = net(pa.asarray(x.copy()))
    y = y[0] if isinstance(y, tuple) else y
    algos = net.compile(pa.asarray(x)).algos
    return net, y.get(), algos


@pytest.mark.parametrize("lay", [7, 8, 9, 11])
def test_one_conv_net_with_the_layout_forced(pa, lay):
    for fam in ("f4x4", "w1d4", "wino43"):
        assert _precondition(NET_SHAPE, fam)
    g, blob, x, want = _one_conv_net(pa, NET_SHAPE)
    net, y, algos = _run_net(pa, g, blob, x, lay)
    used = [a["w_layout"] for a in algos if a["w_layout"] is not None]
    assert used == [lay], algos
    REACHED["net_layouts"].add(lay)
    _exact(y, want, "one-conv net, w_layout %d" % lay, algos[0]["plan"])


@pytest.mark.parametrize("side", FOLD_SIDES)
def test_dilated_conv_folded_onto_the_winograd_kernels(pa, side, monkeypatch):
    """A dilation-2 conv under PLANER_HIP_DILATED_FOLD=force: each pixel phase is a plain 3x3 conv of a subset of the map's pixels
    with the same filter; the precondition is asserted on the four phases as the kernel sees them."""
    monkeypatch.setenv("PLANER_HIP_DILATED_FOLD", "force")
    shape = (2, 16, side, side, 16)
    _, K, _, sc, sh, _ = operands(shape)
    for xph in fold_phases(shape):
        R.wino_exact_assert("f4x4", xph, K, None, sc, sh, xph)
    g, blob, x, want = _one_conv_net(pa, shape, dilation=2)
    for lay in ((7, 9) if side == 16 else (7,)):
        net, y, algos = _run_net(pa, g, blob, x, lay)
        assert net.fold_dilated == "force" and net.dilated_folds == 1, (net.fold_dilated, net.dilated_folds)
        conv = [a for a in algos if a["w_layout"] is not None]
        assert [a["w_layout"] for a in conv] == [lay] and conv[0].get("fold"), algos
        assert conv[0]["x"] == [8, 16, -(-side // 2), -(-side // 2)], conv[0]
        REACHED["folds"].add((side, lay))
        _exact(y, want, "dilation 2 folded, side %d, w_layout %d" % (side, lay), conv[0]["plan"])


# ---- what the module reached ---------------------------------------------------------------------------------------------------
def test_zz_coverage_and_times(pa):
    """Runs last (file order): needs the whole module to have run."""
    for name, t in sorted(REACHED["times"].items(), key=lambda kv: -kv[1])[:12]:
        print("%6.2f s  %s" % (t, name))
    plans = REACHED["plans"]
    has = lambda *words: any(all(w in p for w in words) for p in plans)
    assert has("wf4 ", "16tiles woven"), "the woven 16-tile block did not run"
    assert any("wf4 " in p and "16tiles (" in p for p in plans), "the phased 16-tile block did not run"
    assert has("wf4 ", "32tiles"), "the 32-tile block did not run"
    assert has("wf4 ", "16tiles", "packed") and has("wf4 ", "32tiles", "packed"), "no packed blocks ran"
    assert has("wf4 ", "(2x1x8)"), "the two-image one-row block did not run"
    assert has("wino4[as128x32"), "the filter-stationary GEMM did not run"
    assert any(p.startswith("wino4[") and "as128x32" not in p for p in plans), "the tile GEMM did not run"
    assert REACHED["lds"] == {"1", "2"}, REACHED["lds"]
    assert REACHED["layouts"] == {7, 8, 9, 11} and REACHED["net_layouts"] == {7, 8, 9, 11}, (REACHED["layouts"], REACHED["net_layouts"])
    assert REACHED["entries"] == {"pl_wino4_chain_q4_f32", "pl_wino43_chain_q4_f32"}, REACHED["entries"]
    assert REACHED["folds"] == {(8, 7), (7, 7), (16, 7), (16, 9), (14, 7)}, REACHED["folds"]
    predicted = sorted(k[:3] for k in REACHED["predicted"] if k[3])
    # every form and tail of the two one-tile maps, and nothing else
    assert predicted == sorted((s, f, t) for s in ((1, 4, 1, 1, 4), (33, 4, 2, 2, 4)) for f in WF4_FORMS for t in range(len(TAILS)))
    assert sorted(REACHED["refused"]) == predicted, (len(REACHED["refused"]), len(predicted))
    print("fused kernel: %d launches exact, %d refusals as predicted" % (len(REACHED["predicted"]) - len(predicted), len(predicted)))

"""Plan compiler: linear upsample and resize in channel-quad (Q4) plans (plan.assign_layouts, plan.fuse_linear_add) and the
Panoptic-FPN net that needs them (planer_amd.irgen.fpn).  Host logic only."""
import numpy as np
import pytest

from planer_amd import layer
from planer_amd.irgen import drn, fpn
from planer_amd.plan import fuse_linear_add
from tests.conftest import assert_close
from tests.linear_q4_ref import Small, compile_plan, kinds_of, make_x, run_on_oracle, sandwich, steps_of

CONVERSIONS = ("to_q4", "from_q4")
TRANSFORMS = ("half_pixel", "asymmetric", "align_corners", "pytorch_half_pixel")
ROUNDINGS = ("round_prefer_floor", "round_prefer_ceil", "floor", "ceil")
ZERO_SHIFT = [(t, r) for t in TRANSFORMS for r in ROUNDINGS if layer._nearest_shift(2, t, r) == 0]
SHIFTED = [(t, r) for t in TRANSFORMS for r in ROUNDINGS if layer._nearest_shift(2, t, r) != 0]


def _up(mode="linear", scales="scales2"):
    return lambda s, y: s.g.op("upsample", [y, scales], "u", name="up", mode=mode)


def _resize(scales=None, sizes=None, **para):
    def step(s, y):
        srcs = [y, "roi"]
        if scales is not None:
            s.g.init("k", np.array(scales, np.float32))
            srcs.append("k")
        else:
            s.g.init("sz", np.array(sizes, np.int64))
            srcs += ["none", "sz"]
        return s.g.op("resize", srcs, "u", name="up", **para)
    return step


def _middle(step, x=None):
    g, b = sandwich(step)
    body, flow, nadd, _ = compile_plan(g, b, make_x() if x is None else x)
    return kinds_of(body, flow)


def test_linear_upsample_between_convs_stays_channel_quad(monkeypatch):
    """conv -> upsample(linear x2) -> conv is one Q4 run; PLANER_HIP_LINEAR_Q4=0 gives the program with both conversions.  (This
    test fails on a compiler without the linear Q4 kinds: it gives the second program either way.)"""
    assert _middle(_up()) == ["to_q4", "conv_q4", "upsample_q4", "conv_q4", "from_q4", "return"]
    monkeypatch.setenv("PLANER_HIP_LINEAR_Q4", "0")
    assert _middle(_up()) == ["to_q4", "conv_q4", "from_q4", "upsample", "to_q4", "conv_q4", "from_q4", "return"]


Q4_RESIZES = [("linear scales", _resize(scales=[1, 1, 2, 2], mode="linear")),
              ("linear sizes", _resize(sizes=[1, 8, 12, 14], mode="linear")),
              ("linear fractional", _resize(scales=[1, 1, 1.5, 2.25], mode="linear")),
              ("linear fractional sizes", _resize(sizes=[1, 8, 13, 10], mode="linear"))]
Q4_RESIZES += [("nearest %s %s" % p, _resize(scales=[1, 1, 2, 2], mode="nearest", coordinate_transformation_mode=p[0], nearest_mode=p[1]))
               for p in ZERO_SHIFT]


@pytest.mark.parametrize("what,step", Q4_RESIZES, ids=[w for w, _ in Q4_RESIZES])
def test_resize_goes_channel_quad(what, step, monkeypatch):
    assert _middle(step) == ["to_q4", "conv_q4", "resize_q4", "conv_q4", "from_q4", "return"]
    monkeypatch.setenv("PLANER_HIP_LINEAR_Q4", "0")
    assert _middle(step) == ["to_q4", "conv_q4", "from_q4", "resize", "to_q4", "conv_q4", "from_q4", "return"]


def test_zero_shift_pairs_are_the_documented_ones():
    """layer.Resize's docstring: zero for (half_pixel, round_prefer_*) and (asymmetric, floor)."""
    assert {("half_pixel", "round_prefer_floor"), ("half_pixel", "round_prefer_ceil"), ("asymmetric", "floor")} <= set(ZERO_SHIFT)
    assert SHIFTED


def _graph_scales(s, y):
    s.g.init("k0", np.array([1, 1, 2, 2], np.float32))
    k = s.g.op("identity", "k0", "k1", name="copy_scales")
    return s.g.op("resize", [y, "roi", k], "u", name="up", mode="linear")


def _by_72(s, y):
    s.g.init("k72", np.array([1, 1, 9, 8], np.float32))
    return s.g.op("upsample", [y, "k72"], "u", name="up", mode="linear")


NCHW_STEPS = [("shifted nearest %s %s" % SHIFTED[0], "resize",
               _resize(scales=[1, 1, 2, 2], mode="nearest", coordinate_transformation_mode=SHIFTED[0][0], nearest_mode=SHIFTED[0][1])),
              ("resize 1x1", "resize", _resize(scales=[1, 1, 1, 1], mode="linear")),
              ("upsample 1x1", "upsample", lambda s, y: (s.g.init("k11", np.array([1, 1, 1, 1], np.float32)),
                                                         s.g.op("upsample", [y, "k11"], "u", name="up", mode="linear"))[1]),
              ("72 weights", "upsample", _by_72),
              ("resize 72 weights", "resize", _resize(scales=[1, 1, 9, 8], mode="linear")),
              ("scales from the graph", "resize", _graph_scales)]


@pytest.mark.parametrize("what,kind,step", NCHW_STEPS, ids=[w for w, _, _ in NCHW_STEPS])
def test_steps_without_a_channel_quad_form_stay_nchw(what, kind, step):
    names = _middle(step)
    assert kind in names and kind + "_q4" not in names, names
    i = names.index(kind)
    assert names[i - 1] == "from_q4" and names[i + 1] == "to_q4", names


def test_fractional_resize_of_a_one_pixel_row_stays_nchw():
    """H = 1 has no row + 1 for the fractional kernel: the step keeps its NCHW place, where layer.Resize raises the reference's
    error.  Compiled by hand, since the oracle cannot run the shape either."""
    from planer_amd.plan import assign_layouts
    body = [["c", "conv", dict(group=1, strides=[1, 1], dilations=[1, 1], pads=[0, 0, 0, 0])],
            ["up", "resize", {"mode": "linear"}], ["z", "conv", dict(group=1, strides=[1, 1], dilations=[1, 1], pads=[0, 0, 0, 0])]]
    flow = [[["x", "w"], ["c"], "a"], [["a", "roi", "k"], ["up"], "u"], [["u", "w"], ["z"], "y"]]
    vals = {"k": np.array([1, 1, 1.5, 1.5], np.float32), "roi": np.zeros(0, np.float32)}
    for h, want in ((1, "resize"), (2, "resize_q4")):
        shapes = {"x": (1, 8, h, 4), "w": (8, 8, 1, 1), "a": (1, 8, h, 4), "u": (1, 8, round(1.5 * h), 6), "y": (1, 8, round(1.5 * h), 6),
                  "k": (4,), "roi": (0,)}
        b2, f2, _ = assign_layouts(body, flow, ["w", "roi", "k"], shapes, force=True, values=vals.get)
        assert kinds_of(b2, f2)[2 if want == "resize_q4" else 3] == want, kinds_of(b2, f2)


@pytest.mark.parametrize("via", ["upsample", "resize"])
def test_a_linear_upsample_that_ends_the_program_stays_nchw(via):
    s = Small()
    y = s.conv("x", "a", cin=4)
    if via == "upsample":
        y = s.g.op("upsample", [y, "scales2"], "u", name="up", mode="linear")
    else:
        y = s.g.op("resize", [y, "roi", "scales2"], "u", name="up", mode="linear")
    g, b = s.finish(y)
    body, flow, _, _ = compile_plan(g, b, make_x())
    assert kinds_of(body, flow) == ["to_q4", "conv_q4", "from_q4", via, "return"]
    # ... also where the upsample is the flow's very last step (no `return` layer behind it)
    g["layers"], g["flow"] = g["layers"][:-1], g["flow"][:-1]
    body, flow, _, _ = compile_plan(g, b, make_x())
    assert kinds_of(body, flow) == ["to_q4", "conv_q4", "from_q4", via]


def test_drn_compiles_to_the_same_program_with_the_switch_on_and_off(monkeypatch):
    g, b = drn.build()
    x = drn.make_input(1, size=64)
    on = compile_plan(g, b, x, force=False)[:3]
    monkeypatch.setenv("PLANER_HIP_LINEAR_Q4", "0")
    off = compile_plan(g, b, x, force=False)[:3]
    assert on == off and on[2] == 0
    names = kinds_of(on[0], on[1])
    assert names[-3:] == ["from_q4", "upsample", "return"] and "upsample_q4" not in names


# ---- fuse_linear_add ------------------------------------------------------------------------------------------------------
def _sum_graph(first, extra=None):
    """a = conv(x); b = conv(nearest x2 of x), read twice so that no conv takes the add into its epilogue; s = linear x2 of a + b,
    the upsample as the add's first or second operand; z = conv(s) + b."""
    s = Small()
    u0 = s.g.op("upsample", ["x", "scales2"], "x2", name="up0", mode="nearest")
    yb = s.conv(u0, "b", cin=4)
    ya = s.conv("x", "a", cin=4)
    up = s.g.op("upsample", [ya, "scales2"], "u", name="up", mode="linear")
    if extra:
        extra(s, ya, up)
    t = s.g.op("add", [up, yb] if first else [yb, up], "s", name="sum")
    z = s.conv(t, "z")
    o = s.g.op("add", [z, yb], "o", name="late")
    return s.finish(o)


@pytest.mark.parametrize("first", [True, False], ids=["upsample first", "upsample second"])
def test_an_add_behind_a_linear_upsample_is_fused_in_either_operand_position(first):
    g, b = _sum_graph(first)
    x = make_x(2)
    body, flow, nadd, _ = compile_plan(g, b, x)
    steps = steps_of(body, flow)
    names = [s[0] for s in steps]
    assert nadd == 1 and "add_q4" not in names and "upsample_q4" not in names
    fused = [s for s in steps if s[0] == "upsample_add_q4"]
    assert len(fused) == 1 and fused[0][2] == ["a", "scales2", "b"] and fused[0][3] == "s" and fused[0][1]["mode"] == "linear"
    assert_close(run_on_oracle(g, b, x, body, flow), run_on_oracle(g, b, x, g["layers"], g["flow"]), 1e-6)


def test_a_linear_resize_with_sizes_is_fused_too():
    s = Small()
    s.g.init("sz", np.array([2, 8, 12, 14], np.int64))
    u0 = s.g.op("upsample", ["x", "scales2"], "x2", name="up0", mode="nearest")
    yb = s.conv(u0, "b", cin=4)
    ya = s.conv("x", "a", cin=4)
    up = s.g.op("resize", [ya, "roi", "none", "sz"], "u", name="up", mode="linear")
    t = s.g.op("add", [yb, up], "s", name="sum")
    o = s.g.op("add", [s.conv(t, "z"), yb], "o", name="late")
    g, b = s.finish(o)
    x = make_x(2)
    body, flow, nadd, _ = compile_plan(g, b, x)
    fused = [st for st in steps_of(body, flow) if st[0] == "resize_add_q4"]
    assert nadd == 1 and len(fused) == 1 and fused[0][2] == ["a", "roi", "none", "sz", "b"]
    assert_close(run_on_oracle(g, b, x, body, flow), run_on_oracle(g, b, x, g["layers"], g["flow"]), 1e-6)


def test_no_fusion_where_the_upsampled_tensor_has_two_readers():
    g, b = _sum_graph(True, extra=lambda s, ya, up: s.g.op("leakyrelu", up, "side", name="second_reader", alpha=0.1))
    # (`side` is dead code for the result; the reader is what matters)
    body, flow, nadd, _ = compile_plan(g, b, make_x())
    names = kinds_of(body, flow)
    assert nadd == 0 and "upsample_q4" in names and "add_q4" in names and "upsample_add_q4" not in names


def _hand(steps, shapes):
    body = [[name, kind, para] for _, name, kind, para, _ in steps]
    flow = [[list(srcs), [name], dst] for srcs, name, _, _, dst in steps]
    return fuse_linear_add(body, flow, shapes)


UP = (["a", "k"], "up", "upsample_q4", {"mode": "linear"}, "u")
SHAPES = {"a": (1, 8, 3, 4), "u": (1, 8, 6, 8), "r": (1, 8, 6, 8), "s": (1, 8, 6, 8), "x": (1, 8, 6, 8)}


def test_fuse_linear_add_by_hand():
    """The pass on hand-written programs: the plain pair fuses; a nearest upsample, a broadcast add, an in-place relu_q4 on the
    upsample's source between the two, and a step between the two that writes the other operand do not."""
    add = (["u", "r"], "sum", "add_q4", {}, "s")
    body, flow, n = _hand([UP, add], SHAPES)
    assert n == 1 and flow == [[["a", "k", "r"], ["up+"], "s"]] and body == [["up+", "upsample_add_q4", {"mode": "linear"}]]
    # the fused step sits where the add was
    mid = (["x"], "other", "leakyrelu_q4", {}, "x2")
    body, flow, n = _hand([UP, mid, add], dict(SHAPES, x2=(1, 8, 6, 8)))
    assert n == 1 and [f[1][0] for f in flow] == ["other", "up+"]
    # nearest: nothing to fuse into
    assert _hand([(UP[0], "up", "upsample_q4", {"mode": "nearest"}, "u"), add], SHAPES)[2] == 0
    assert _hand([(UP[0], "up", "upsample_q4", {}, "u"), add], SHAPES)[2] == 0
    # a broadcast add: the other operand has another shape (or none that is known)
    assert _hand([UP, add], dict(SHAPES, r=(1, 8, 1, 1)))[2] == 0
    assert _hand([UP, add], {k: v for k, v in SHAPES.items() if k != "r"})[2] == 0
    # relu_q4 rewrites the upsample's source in place between the two: the delayed upsample would read the rectified values
    relu = (["a"], "rect", "relu_q4", {}, "a2")
    body, flow, n = _hand([UP, relu, add], dict(SHAPES, a2=SHAPES["a"]))
    assert n == 0 and [f[1][0] for f in flow] == ["up", "rect", "sum"]
    # ... a pure reader of the source between the two is harmless
    assert _hand([UP, (["a"], "leak", "leakyrelu_q4", {}, "a2"), add], dict(SHAPES, a2=SHAPES["a"]))[2] == 1
    # a step between the two writes the other operand
    wr = (["x"], "other", "leakyrelu_q4", {}, "r")
    assert _hand([UP, wr, add], SHAPES)[2] == 0
    assert _hand([wr, UP, add], SHAPES)[2] == 1
    # two readers, two writers
    assert _hand([UP, add, (["u"], "again", "leakyrelu_q4", {}, "v")], SHAPES)[2] == 0
    assert _hand([UP, (["x"], "other", "leakyrelu_q4", {}, "u"), add], SHAPES)[2] == 0


def test_no_fusion_on_a_broadcast_add_in_a_compiled_graph():
    """An add with a (1, C, 1, 1) operand has no Q4 kind at all: it stays `add` on NCHW copies, the upsample stays a step."""
    def tail(s, y):
        s.g.init("bias", np.arange(8, dtype=np.float32).reshape(1, 8, 1, 1))
        up = s.g.op("upsample", [y, "scales2"], "u", name="up", mode="linear")
        return s.g.op("add", [up, "bias"], "s", name="sum")
    g, b = sandwich(tail)
    body, flow, nadd, _ = compile_plan(g, b, make_x())
    names = kinds_of(body, flow)
    assert nadd == 0 and "upsample_add_q4" not in names and "upsample_q4" in names and "add" in names


# ---- the FPN net ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("via", ["upsample", "resize"])
def test_fpn_is_one_channel_quad_run(via):
    """fpn.build() at 64 x 64.  The net has ten linear steps and six adds besides ResNet-18's eight:
      * the three top-down adds `lateral + up2(P)` follow a conv (the lateral), so fuse_flow puts them into that conv's epilogue
        with the upsampled map as the residual: three `upsample_q4` steps feeding conv residuals;
      * the sum of the four head maps is ((h2 + u3) + u4) + u5.  Its first add follows h2's conv + ReLU and goes into that conv's
        epilogue (residual after the activation); the other two have no conv ahead of them and are what fuse_linear_add takes:
        two `upsample_add_q4` steps;
      * so 9 - 2 = 7 plain `upsample_q4` steps, 2 fused adds, 3 + 1 = 4 adds in conv epilogues that read an upsampled map, and no
        `add_q4` left;
      * the x4 step at the end stays NCHW behind the only `from_q4`; the row-packed stem reads NCHW itself, so there is no
        `to_q4` anywhere."""
    g, b = fpn.build(via=via)
    x = fpn.make_input(1, size=64)
    body, flow, nadd, shapes = compile_plan(g, b, x, force=False)
    steps = steps_of(body, flow)
    names = [s[0] for s in steps]
    assert names.count(via + "_q4") == 7 and names.count(via + "_add_q4") == 2 and nadd == 2
    assert names.count("add_q4") == 0 and names.count("add") == 0
    ups = {s[3] for s in steps if s[0] == via + "_q4"}
    epilogue = [s for s in steps if s[0] == "conv_q4" and len(s[2]) > 5 and s[2][5] in ups]
    assert len(epilogue) == 4
    assert names.count("conv_q4") == 36
    assert names.count("from_q4") == 1 and names[-3:] == ["from_q4", via, "return"]
    assert names.count("to_q4") == 0
    assert shapes["out"] == (1, 21, 64, 64) and shapes["lat5_c"] == (1, 128, 2, 2)


def test_fpn_switch_off_gives_the_program_with_a_conversion_pair_per_upsample(monkeypatch):
    monkeypatch.setenv("PLANER_HIP_LINEAR_Q4", "0")
    g, b = fpn.build()
    body, flow, nadd, _ = compile_plan(g, b, fpn.make_input(1, size=64), force=False)
    names = kinds_of(body, flow)
    assert nadd == 0 and names.count("upsample") == 10 and names.count("upsample_q4") == 0
    assert names.count("from_q4") == 10 and names.count("to_q4") == 9 and names.count("add_q4") == 2


def test_fpn_compiled_program_and_both_forms_match_the_oracle():
    x = fpn.make_input(1, size=32)
    outs = []
    for via in ("upsample", "resize"):
        g, b = fpn.build(via=via)
        body, flow, _, _ = compile_plan(g, b, x, force=False)
        want = run_on_oracle(g, b, x, g["layers"], g["flow"])
        got = run_on_oracle(g, b, x, body, flow)
        assert got.shape == want.shape == (1, 21, 32, 32)
        assert_close(got, want, 1e-5, via)
        outs.append(want)
    np.testing.assert_array_equal(outs[0], outs[1])

"""Plan compiler: group normalisation written as reshape -> instancenormalization -> reshape -> mul -> add (plan.fuse_groupnorm),
its place in channel-quad (Q4) plans (plan.assign_layouts, the tail fusion of plan.fuse_instnorm_q4) and the ResNet-18-GN net that
needs it (planer_amd.irgen.resnet_gn).  Host logic only.  Programs are compared in bits on the numpy oracle, with `groupnorm`
standing for the five oracle operators; the kernel's arithmetic is held to float64 through a float32 emulation
(tests/groupnorm_ref.py)."""
import zlib

import numpy as np
import pytest

from planer_amd.irgen import resnet_gn
from planer_amd import plan
from planer_amd.plan import _FOLD_POINTWISE, _IN_PLACE, _PURE_READERS, Q4_POINTWISE, fuse_groupnorm, groupnorm_q4_ok
from tests import ref64_ops as R
from tests.groupnorm_ref import (compile_plan, cpu_front, emulate, five_steps, kinds_of, make_x, operands, reference, run_on_oracle,
                                 sandwich, steps_of)
from tests.linear_q4_ref import Small, assert_same_bits

ONE_STEP = ["to_q4", "conv_q4", "groupnorm_q4", "conv_q4", "from_q4", "return"]


def _original(g, b, x):
    return run_on_oracle(g, b, x, g["layers"], g["flow"])


def _norm(flow):
    return [[list(s) if isinstance(s, (list, tuple)) else [s], list(nm), d] for s, nm, d in flow]


def _fused(g, b, x):
    """fuse_flow's program and what fuse_groupnorm makes of it -> (body, flow, body', flow', n)."""
    body, flow, _, shapes = cpu_front(g, b, x, stop="fuse_flow")
    return (body, flow) + tuple(fuse_groupnorm(body, flow, shapes, [i[0] for i in g["inits"]]))


def _left_alone(g, b, x):
    body, flow, body2, flow2, n = _fused(g, b, x)
    assert n == 0
    assert [list(e) for e in body2] == [list(e) for e in body] and _norm(flow2) == _norm(flow)
    names = kinds_of(*compile_plan(g, b, x)[:2])
    assert "groupnorm" not in names and "groupnorm_q4" not in names and "instancenormalization" in names


# ---- 1. every form is one channel-quad step -------------------------------------------------------------------------------------
FORMS = {"3d": dict(), "4d-middle": dict(mid="4d"), "shape-const-step": dict(via_const=True), "mul-swapped": dict(swap_mul=True),
         "add-swapped": dict(swap_add=True), "both-swapped-leading-1": dict(swap_mul=True, swap_add=True, lead=True),
         "leading-1": dict(lead=True), "only-mul": dict(affine="mul"), "only-mul-swapped": dict(affine="mul", swap_mul=True, lead=True),
         "no-affine": dict(affine="none"), "no-affine-4d-const": dict(affine="none", mid="4d", via_const=True)}


@pytest.mark.parametrize("groups", [2, 4, 8], ids=["cpg4", "cpg2", "cpg1"])
@pytest.mark.parametrize("form", list(FORMS))
def test_each_form_between_convs_is_one_channel_quad_step(form, groups):
    kw = FORMS[form]
    g, b = sandwich(c=8, groups=groups, **kw)
    x = make_x()
    body, flow, ngn, _ = compile_plan(g, b, x)
    steps = steps_of(body, flow)
    assert ngn == 1 and [s[0] for s in steps if s[0] != "const"] == ONE_STEP, [s[0] for s in steps]
    gn = [s for s in steps if s[0] == "groupnorm_q4"][0]
    affine = kw.get("affine", "both")
    want = ["a", "gn_ones", "gn_zeros", "gn_gamma" if affine != "none" else "None", "gn_beta" if affine == "both" else "None"]
    assert gn[1] == {"groups": groups, "epsilon": 1e-5} and gn[2] == want
    assert gn[3] == {"both": "gn_b", "mul": "gn_k", "none": "gn_m"}[affine]
    # the steps that only fed the reshapes' shape operands stay where they are
    assert [s[0] for s in steps].count("const") == (2 if kw.get("via_const") else 0)
    got = run_on_oracle(g, b, x, body, flow, mid=kw.get("mid", "3d"))
    if kw.get("mid") == "4d":
        # the oracle's conv hands out a strided view and conv_q4's stand-in a contiguous array; numpy's mean over the two trailing
        # axes of the 4-D split adds those in different orders.  So the 4-D forms are held to the program of the switched-off
        # compiler -- the same conv stand-ins, the five oracle steps -- and to the original at the project's tolerance
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PLANER_HIP_GROUPNORM_Q4", "0")
            off = compile_plan(g, b, x)
        assert off[2] == 0 and "instancenormalization" in kinds_of(*off[:2])
        assert_same_bits(got, run_on_oracle(g, b, x, off[0], off[1]), "rewritten program against the switched-off compiler's")
        np.testing.assert_allclose(got, _original(g, b, x), rtol=1e-5, atol=1e-5)
    else:
        assert_same_bits(got, _original(g, b, x), "rewritten program against the original")


def test_which_channel_counts_have_a_channel_quad_form():
    assert all(groupnorm_q4_ok(c, g) for c, g in ((5, 5), (6, 3), (8, 4), (8, 2), (16, 2), (12, 1), (64, 32), (512, 32), (4, 1)))
    assert not any(groupnorm_q4_ok(c, g) for c, g in ((6, 2), (12, 2), (20, 2), (9, 3), (8, 3), (8, 0), (0, 1), (10, 1)))
    assert "groupnorm" in Q4_POINTWISE and {"groupnorm", "groupnorm_q4"} <= set(_IN_PLACE)
    assert "groupnorm_q4" not in _PURE_READERS and "groupnorm_q4" not in _FOLD_POINTWISE


# ---- 2. patterns that must be left alone ----------------------------------------------------------------------------------------
def _with(extra=None, **kw):
    """conv -> five steps -> `extra(small, keys)` -> conv -> return"""
    s = Small()
    y = s.conv("x", "a", cin=4, cout=8)
    y = five_steps(s, y, (1, 8, 6, 7), 2, **kw)
    if extra is not None:
        y = extra(s, y) or y
    return s.finish(s.conv(y, "z", cin=8))


def test_an_input_with_a_second_reader_is_left_alone():
    """The norm rewrites x in place: another reader of x would see other values once the step has moved."""
    g, b = _with(lambda s, y: s.g.op("add", [y, "a"], "o", name="skip"))
    _left_alone(g, b, make_x())


@pytest.mark.parametrize("key", ["gn_g", "gn_n", "gn_m", "gn_k"], ids=["split", "normalised", "merged", "scaled"])
def test_a_middle_tensor_with_a_second_reader_is_left_alone_or_ends_the_chain(key):
    def side(s, y):
        s.g.op("leakyrelu", key, "side", name="second_reader", alpha=0.1)
    g, b = _with(side)
    x = make_x()
    if key in ("gn_g", "gn_n"):
        _left_alone(g, b, x)
        return
    # behind the second reshape the norm is complete: what follows the shared tensor stays a step of its own
    body, flow, body2, flow2, n = _fused(g, b, x)
    names = [k for k in kinds_of(body2, flow2)]
    assert n == 1 and names.count("groupnorm") == 1
    gn = [s for s in steps_of(body2, flow2) if s[0] == "groupnorm"][0]
    assert gn[3] == key and gn[2][3:] == (["None", "None"] if key == "gn_m" else ["gn_gamma", "None"])
    assert names.count("mul") == (1 if key == "gn_m" else 0) and names.count("add") == 1
    body, flow, _, _ = compile_plan(g, b, x)
    assert_same_bits(run_on_oracle(g, b, x, body, flow), _original(g, b, x))


def test_a_second_reshape_to_another_shape_is_left_alone():
    g, b = _with(affine="none", merge=[0, 8, 7, 6])
    _left_alone(g, b, make_x())


@pytest.mark.parametrize("shape", [(1, 1, 6, 7), (8, 6, 7)], ids=["per-pixel", "CHW"])
def test_a_mul_by_a_constant_of_another_shape_stays_a_mul(shape):
    g, b = _with(affine="mul", gamma_shape=shape)
    x = make_x()
    body, flow, body2, flow2, n = _fused(g, b, x)
    gn = [s for s in steps_of(body2, flow2) if s[0] == "groupnorm"]
    assert n == 1 and gn[0][2][3:] == ["None", "None"] and kinds_of(body2, flow2).count("mul") == 1
    body, flow, _, _ = compile_plan(g, b, x)
    assert_same_bits(run_on_oracle(g, b, x, body, flow), _original(g, b, x))


def test_a_mul_by_an_activation_stays_a_mul():
    def gate(s, y):
        return s.g.op("mul", [y, s.conv("x", "w", cin=4, cout=8)], "gated", name="gate")
    g, b = _with(gate, affine="none")
    body, flow, body2, flow2, n = _fused(g, b, make_x())
    assert n == 1 and kinds_of(body2, flow2).count("mul") == 1
    assert [s for s in steps_of(body2, flow2) if s[0] == "groupnorm"][0][2][3:] == ["None", "None"]


def test_an_instance_norm_with_a_computed_scale_is_left_alone():
    s = Small()
    y = s.conv("x", "a", cin=4, cout=8)
    s.g.init("s3", np.array([0, 2, -1], np.int64))
    s.g.init("s4", np.array([0, 8, 6, 7], np.int64))
    s.g.init("half", np.array([0.5, 2.0], np.float32))
    s.g.init("zeros", np.zeros(2, np.float32))
    s.g.op("leakyrelu", "half", "scale", name="make_scale", alpha=0.5)
    y = s.g.op("reshape", [y, "s3"], "g3", name="split")
    y = s.g.op("instancenormalization", [y, "scale", "zeros"], "n", name="in", epsilon=1e-5)
    y = s.g.op("reshape", [y, "s4"], "m", name="merge")
    g, b = s.finish(s.conv(y, "z", cin=8))
    _left_alone(g, b, make_x())


def test_a_three_dimensional_input_is_left_alone():
    layers = [["split", "reshape", {}], ["in", "instancenormalization", {"epsilon": 1e-5}], ["merge", "reshape", {}]]
    flow = [[["a", "s3"], ["split"], "g"], [["g", "ones", "zeros"], ["in"], "n"], [["n", "s4"], ["merge"], "m"]]
    shapes = {"a": (2, 8, 42), "g": (2, 2, 168), "n": (2, 2, 168), "m": (2, 8, 42), "ones": (2,), "zeros": (2,)}
    body, out, n = fuse_groupnorm(layers, flow, shapes)
    assert n == 0 and body == layers and _norm(out) == _norm(flow)
    body, out, n = fuse_groupnorm(layers, flow, dict(shapes, a=(2, 8, 6, 7), m=(2, 8, 6, 7)))
    assert n == 1 and body == [["in+", "groupnorm", {"groups": 2, "epsilon": 1e-5}]]
    assert out == [[["a", "ones", "zeros", "None", "None"], ["in+"], "m"]]


def test_a_write_of_the_input_between_the_steps_blocks_the_rewrite():
    layers = [["split", "reshape", {}], ["again", "leakyrelu", {"alpha": 0.1}], ["in", "instancenormalization", {}], ["merge", "reshape", {}]]
    flow = [[["a", "s3"], ["split"], "g"], ["q", ["again"], "a"], [["g", "ones", "zeros"], ["in"], "n"], [["n", "s4"], ["merge"], "m"]]
    shapes = {"a": (2, 8, 6, 7), "g": (2, 2, 168), "n": (2, 2, 168), "m": (2, 8, 6, 7), "ones": (2,), "zeros": (2,), "q": (2, 8, 6, 7)}
    assert fuse_groupnorm(layers, flow, shapes)[2] == 0
    flow[1] = ["q", ["again"], "other"]
    assert fuse_groupnorm(layers, flow, shapes)[2] == 1


def test_three_channels_per_group_are_named_but_run_nchw():
    g, b = sandwich(c=6, groups=2)
    x = make_x()
    body, flow, ngn, _ = compile_plan(g, b, x)
    assert ngn == 1
    assert kinds_of(body, flow) == ["to_q4", "conv_q4", "from_q4", "groupnorm", "to_q4", "conv_q4", "from_q4", "return"]
    assert_same_bits(run_on_oracle(g, b, x, body, flow), _original(g, b, x))


# ---- 3. tail fusion ---------------------------------------------------------------------------------------------------------------
def _block(order, spoil=False):
    """conv a -> conv c -> norm(c) -> tail with residual a -> conv z"""
    s = Small()
    a = s.conv("x", "a", cin=4, cout=8)
    y = s.conv(a, "c", cin=8, cout=8)
    y = five_steps(s, y, (1, 8, 6, 7), 2)
    if order == "add-relu":
        y = s.g.op("add", [y, a], "sum", name="residual")
        if spoil:
            s.g.op("relu", a, "a_r", name="rewrites_the_residual")
        y = s.g.op("relu", y, "out", name="out_relu")
    else:
        y = s.g.op("relu", y, "pos", name="first_relu")
        y = s.g.op("add", [y, a], "out", name="residual")
    return s.finish(s.conv(y, "z", cin=8))


def test_norm_add_relu_is_one_step_with_res_and_act():
    g, b = _block("add-relu")
    x = make_x()
    body, flow, _, _ = compile_plan(g, b, x)
    steps = steps_of(body, flow)
    assert [s[0] for s in steps] == ["to_q4", "conv_q4", "conv_q4", "groupnorm_q4", "conv_q4", "from_q4", "return"]
    gn = steps[3]
    assert gn[1] == {"groups": 2, "epsilon": 1e-5, "act": 1} and gn[2] == ["c", "gn_ones", "gn_zeros", "gn_gamma", "gn_beta", "a"]
    assert gn[3] == "out"
    assert_same_bits(run_on_oracle(g, b, x, body, flow), _original(g, b, x))


def test_norm_relu_add_keeps_the_add():
    g, b = _block("relu-add")
    x = make_x()
    body, flow, _, _ = compile_plan(g, b, x)
    steps = steps_of(body, flow)
    assert [s[0] for s in steps] == ["to_q4", "conv_q4", "conv_q4", "groupnorm_q4", "add_q4", "conv_q4", "from_q4", "return"]
    assert steps[3][1]["act"] == 1 and steps[3][2][5] == "None"
    assert_same_bits(run_on_oracle(g, b, x, body, flow), _original(g, b, x))


def test_a_residual_rewritten_between_the_add_and_the_relu_breaks_the_chain():
    g, b = _block("add-relu", spoil=True)
    x = make_x()
    body, flow, _, _ = compile_plan(g, b, x)
    steps = steps_of(body, flow)
    names = [s[0] for s in steps]
    gn = steps[names.index("groupnorm_q4")]
    assert gn[1]["act"] == 0 and gn[2][5] == "a" and names.count("relu_q4") == 2 and "add_q4" not in names
    assert_same_bits(run_on_oracle(g, b, x, body, flow), _original(g, b, x))


# ---- 4. the switch ----------------------------------------------------------------------------------------------------------------
def test_switch_off_gives_the_program_without_the_pass(monkeypatch):
    g, b = sandwich()
    x = make_x()
    with monkeypatch.context() as m:             # the compiler with the pass taken out
        m.setattr(plan, "fuse_groupnorm", lambda body, flow, *_: (body, flow, 0))
        want = compile_plan(g, b, x)[:2]
    monkeypatch.setenv("PLANER_HIP_GROUPNORM_Q4", "0")
    got = compile_plan(g, b, x)
    assert got[2] == 0 and (got[0], got[1]) == want
    assert kinds_of(*want) == ["to_q4", "conv_q4", "from_q4", "reshape", "instancenormalization", "reshape", "mul", "add", "to_q4",
                               "conv_q4", "from_q4", "return"]


# ---- 5. the net -------------------------------------------------------------------------------------------------------------------
def test_resnet_gn_is_twenty_channel_quad_norms_and_nothing_between():
    g, b = resnet_gn.build()
    assert resnet_gn.params() == 11689512
    learned = sum(int(np.prod(s)) for n, s, _ in g["inits"] if not n.startswith("gn_"))
    assert learned == resnet_gn.params()
    x = resnet_gn.make_input(1)
    body, flow, ngn, _ = compile_plan(g, b, x)
    names = kinds_of(body, flow)
    assert ngn == 20 and names.count("groupnorm_q4") == 20
    assert not {"reshape", "instancenormalization", "mul", "add_q4", "relu_q4", "groupnorm", "add", "relu"} & set(names)
    first, gap = names.index("conv_q4"), names.index("gap_q4")
    assert first == 0 and not {"to_q4", "from_q4"} & set(names[first:gap + 1])


def test_resnet_gn_stages_and_tiny_variant():
    g, b = resnet_gn.build()
    chans = {n: s[0] for n, s, _ in g["inits"] if n.endswith("_gamma")}
    assert sorted({c // 32 for c in chans.values()}) == [2, 4, 8, 16] and len(chans) == 20
    opts = dict(width=8, groups=4, classes=10, size=32)
    g, b = resnet_gn.build(**opts)
    assert resnet_gn.params(groups=4, width=8, classes=10) == sum(int(np.prod(s)) for n, s, _ in g["inits"] if not n.startswith("gn_"))
    assert sorted({s[0] // 4 for n, s, _ in g["inits"] if n.endswith("_gamma")}) == [2, 4, 8, 16]
    x = resnet_gn.make_input(2, size=32)
    want = _original(g, b, x)
    assert want.shape == (2, 10)
    body, flow, ngn, _ = compile_plan(g, b, x)
    names = kinds_of(body, flow)
    assert ngn == 20 and names.count("groupnorm_q4") == 20 and "add_q4" not in names and "relu_q4" not in names
    # (the stem's conv_q4 stand-in and the oracle's conv differ in the last bit on this net with the switch off as well: the
    # rewritten program is held to the switched-off compiler's in bits, and to the original at 1e-5)
    got = run_on_oracle(g, b, x, body, flow)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PLANER_HIP_GROUPNORM_Q4", "0")
        off = compile_plan(g, b, x)
    assert off[2] == 0 and kinds_of(*off[:2]).count("instancenormalization") == 20
    assert_same_bits(got, run_on_oracle(g, b, x, off[0], off[1]), "tiny ResNet-GN, switch on against off")
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)
    with pytest.raises(ValueError):
        resnet_gn.build(width=8, groups=3)


# ---- 6. no existing behaviour changes -----------------------------------------------------------------------------------------
OTHERS = {"resnet18": dict(size=64), "yolov3": dict(size=64), "mobilenetv2": dict(size=64), "unet": dict(size=32),
          "stylenet": dict(size=32), "drn": dict(size=64), "fpn": dict(size=64), "edsr": dict(size=12)}


@pytest.mark.parametrize("name", list(OTHERS))
def test_the_other_generators_hold_no_such_pattern(name, monkeypatch):
    import importlib
    mod = importlib.import_module("planer_amd.irgen." + name)
    g, b = mod.build(size=12, blocks=2, feats=8) if name == "edsr" else mod.build()
    x = mod.make_input(1, **OTHERS[name])
    body, flow, body2, flow2, n = _fused(g, b, x)
    assert n == 0 and [list(e) for e in body2] == [list(e) for e in body] and _norm(flow2) == _norm(flow)
    if name in ("resnet18", "stylenet"):
        on = compile_plan(g, b, x, force=False)[:3]
        monkeypatch.setenv("PLANER_HIP_GROUPNORM_Q4", "0")
        off = compile_plan(g, b, x, force=False)[:3]
        assert on == off and on[2] == 0 and kinds_of(*on[:2]) == kinds_of(*off[:2])


# ---- 7. the bound is usable, and the one-pass form leaves it ------------------------------------------------------------------
# (C, G, H, W): values per group 9, 130, 512, 1020, 756, 24000
BOUND_CASES = [(5, 5, 3, 3), (6, 3, 5, 13), (8, 4, 16, 16), (8, 2, 17, 15), (12, 1, 7, 9), (16, 2, 50, 60)]
SHORT = 260          # values per group up to which the one-pass variance is claimed to leave the bound at offset 1e3


@pytest.mark.parametrize("case", BOUND_CASES, ids=["%d/%d@%dx%d" % c for c in BOUND_CASES])
def test_the_centred_emulation_stays_inside_the_bound_and_one_pass_leaves_it(case):
    c, groups, h, w = case
    for dc in (0.0, 50.0, 1e3):
        for k, (res, act, gamma, beta) in enumerate([(False, 0, True, True), (True, 1, True, True), (True, 0, True, False),
                                                    (False, 1, False, False)]):
            rng = np.random.default_rng(zlib.crc32(repr(("gn-bound", case, dc, k)).encode()))
            x, gs, gb, ga, be, r = operands(rng, (2, c, h, w), groups, dc, res, gamma, beta)
            ref, tol = reference(x, gs, gb, ga, be, r, act, groups)
            what = "C=%d G=%d %dx%d dc=%g res=%d act=%d gamma=%d beta=%d" % (c, groups, h, w, dc, res, act, gamma, beta)
            worst = R.check(emulate(x, gs, gb, ga, be, r, act, groups), ref, tol, what)
            print("%-70s centred err/tol %.3f" % (what, worst))
            if dc == 1e3 and (c // groups) * h * w <= SHORT:
                one = float(R.ratio(emulate(x, gs, gb, ga, be, r, act, groups, two_pass=False), ref, tol).max())
                print("%-70s one-pass err/tol %.1f" % (what, one))
                assert one > 1.0, what

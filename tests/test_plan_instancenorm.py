"""Plan compiler: instance norm and pixel padding in channel-quad (Q4) plans (plan.assign_layouts, plan.fuse_instnorm_q4) on the
fast-neural-style net (planer_amd.irgen.stylenet).  Host logic only.

The net has 16 conv layers, each a reflect `pad` followed by a conv, so 16 pads in all: the first reads the NCHW input ahead of
the row-packed stem and stays `pad`, the other 15 become `pad_q4`."""
import json
import os

import numpy as np
import pytest

from oracle import planer_np as onp
from planer_amd.irgen import stylenet
from planer_amd.irgen.builder import GraphBuilder
from planer_amd.plan import ACT_NONE, ACT_RELU, assign_layouts, fuse_instnorm_q4, pad_q4_ok
from tests.conftest import GOLDEN, assert_close
from tests.plan_audit import blob_inits, cpu_front, run_on_oracle, steps_of
from tests.test_plan_fusion import shapes_of


def _compile(g, b, x, fuse=True, force=False):
    body, flow, counts, shapes = cpu_front(g, b, x, force, stop="fuse_instnorm_q4" if fuse else "assign_layouts")
    return body, flow, counts["assign_layouts"], counts.get("fuse_instnorm_q4", 0), shapes


@pytest.fixture(scope="module")
def style():
    g, b = stylenet.build()
    return g, b, stylenet.make_input(1, size=32)


def test_generator_parameters_and_op_census(style):
    g, b, _ = style
    assert stylenet.params() == stylenet.PARAMS == sum(int(np.prod(s)) for _, s, d in g["inits"] if d == "float32") - 4
    census = {}
    for _, kind, _ in g["layers"]:
        census[kind] = census.get(kind, 0) + 1
    assert census == {"pad": 16, "conv": 16, "instancenormalization": 15, "relu": 10, "add": 5, "upsample": 2, "return": 1}


def test_style_net_is_one_q4_run_with_fused_norm_tails(style):
    g, b, x = style
    body, flow, nq4, nf, _ = _compile(g, b, x)
    steps = steps_of(body, flow)
    names = [s[0] for s in steps]
    first_conv = names.index("conv_q4")
    # no conversion between the first conv and the single final from_q4 (ahead of `return`)
    assert [i for i, k in enumerate(names) if k in ("to_q4", "from_q4")] == [len(names) - 2] and names[-2:] == ["from_q4", "return"]
    assert names[:first_conv] == ["pad"] and steps[first_conv][1].get("rowpack")
    assert names.count("pad_q4") == 15 and names.count("pad") == 1
    norms = [s for s in steps if s[0] == "instancenormalization_q4"]
    assert len(norms) == 15 and all(len(s[2]) == 4 for s in norms), norms
    relu = [s for s in norms if s[1]["act"] == ACT_RELU]
    res = [s for s in norms if s[2][3] != "None"]
    assert len(relu) == 10 and all(s[2][3] == "None" for s in relu)
    assert len(res) == 5 and all(s[1]["act"] == ACT_NONE for s in res)
    assert nf == 15 and "relu_q4" not in names and "add_q4" not in names and "instancenormalization" not in names
    assert names.count("conv_q4") == 16 and names.count("upsample_q4") == 2


def _in_q4(x, s, b, res=None, epsilon=1e-5, act=0):
    y = onp.OPS["instancenormalization"](x, s.copy(), b.copy(), epsilon=epsilon)
    if res is not None:
        y += res
    return onp.OPS["relu"](y) if act else y


def _run(g, b, x, body, flow):
    return run_on_oracle(g, b, x, body, flow, instancenormalization_q4=_in_q4, pad_q4=onp.OPS["pad"])


def test_compiled_style_program_matches_the_oracle(style):
    g, b, x = style
    body, flow, _, _, _ = _compile(g, b, x)
    want = _run(g, b, x, g["layers"], g["flow"])
    got = _run(g, b, x, body, flow)
    assert got.shape == want.shape == (1, 3, 32, 32)
    assert_close(np.ascontiguousarray(got), np.ascontiguousarray(want), 1e-5)


# ---- small graphs: conv -> IN -> ... ---------------------------------------------------------------------------------------
def _small(tail):
    """x -> conv (8 channels) -> instance norm -> `tail(g, normed, conv_of_x)` -> conv -> return."""
    rng = np.random.default_rng(7)
    g = GraphBuilder(["x"])
    for tag, cin in (("a", 4), ("b", 4), ("z", 8)):
        g.init(tag + "_w", (rng.standard_normal((8, cin, 3, 3)) * 0.2).astype(np.float32))
    g.init("s", rng.uniform(0.5, 1.5, 8).astype(np.float32))
    g.init("t", rng.standard_normal(8).astype(np.float32))
    kw = dict(group=1, strides=[1, 1], dilations=[1, 1], pads=[1, 1, 1, 1])
    g.op("conv", ["x", "a_w"], "ca", name="conv_a", **kw)
    g.op("conv", ["x", "b_w"], "cb", name="conv_b", **kw)
    g.op("instancenormalization", ["ca", "s", "t"], "n", name="norm", epsilon=1e-5)
    y = tail(g, "n", "cb")
    g.op("conv", [y, "z_w"], "out", name="conv_z", **kw)
    graph, blob = g.finish(["out"])
    return graph, blob, rng.standard_normal((2, 4, 6, 6)).astype(np.float32)


def _fused_norm(tail, force=True):
    g, b, x = _small(tail)
    shapes = shapes_of(g, b, x)
    inits = [i[0] for i in g["inits"]]
    body, flow, _ = assign_layouts(g["layers"], g["flow"], inits, shapes, force=force, values=blob_inits(g, b).get)
    body2, flow2, nf = fuse_instnorm_q4(body, flow, shapes)
    want = _run(g, b, x, g["layers"], g["flow"])
    assert_close(np.ascontiguousarray(_run(g, b, x, body2, flow2)), np.ascontiguousarray(want), 1e-5)
    return steps_of(body2, flow2), nf


def test_fuse_residual_then_relu():
    def tail(g, n, other):
        return g.op("relu", g.op("add", [other, n], "sum", name="add"), "r", name="relu")
    steps, nf = _fused_norm(tail)
    norm, = [s for s in steps if s[0] == "instancenormalization_q4"]
    assert nf == 2 and norm[2][3] == "cb" and norm[1]["act"] == ACT_RELU and norm[3] == "r"
    assert not any(s[0] in ("add_q4", "relu_q4") for s in steps)


def test_fuse_refused_when_the_norm_output_is_read_twice():
    def tail(g, n, other):
        r = g.op("relu", n, "r", name="relu")               # in place on n, which the add reads as well
        return g.op("add", [r, n], "sum", name="add")
    steps, nf = _fused_norm(tail)
    norm, = [s for s in steps if s[0] == "instancenormalization_q4"]
    assert nf == 0 and len(norm[2]) == 3 and "act" not in norm[1]
    assert [s[0] for s in steps].count("relu_q4") == 1 and [s[0] for s in steps].count("add_q4") == 1


def test_fuse_refuses_an_add_of_unequal_shapes():
    def tail(g, n, other):
        g.init("row", np.ones((1, 8, 1, 1), np.float32))
        g.op("mul", [other, "row"], "m", name="mul")        # keeps the graph's second conv alive
        g.op("gap", "m", "pooled", name="gap")
        return g.op("add", [n, "pooled"], "sum", name="add")  # (2, 8, 6, 6) + (2, 8, 1, 1): broadcast, not a residual
    steps, nf = _fused_norm(tail)
    norm, = [s for s in steps if s[0] == "instancenormalization_q4"]
    assert nf == 0 and len(norm[2]) == 3
    assert "add" in [s[0] for s in steps]                    # (unequal shapes: the add itself stays NCHW too)
    # the pass itself, on a hand-written program whose add_q4 broadcasts
    body = [["norm", "instancenormalization_q4", {"epsilon": 1e-5}], ["add", "add_q4", {}], ["relu", "relu_q4", {}]]
    flow = [[["c", "s", "t"], ["norm"], "n"], [["n", "p"], ["add"], "sum"], [["sum"], ["relu"], "r"]]
    for pshape, want in (((2, 8, 1, 1), 0), ((2, 8, 6, 6), 2)):
        _, out, nf = fuse_instnorm_q4(body, flow, {"c": (2, 8, 6, 6), "n": (2, 8, 6, 6), "p": pshape})
        assert nf == want and len(out) == 3 - want


def test_fuse_keeps_the_order_residual_before_activation():
    def tail(g, n, other):
        return g.op("add", [g.op("relu", n, "r", name="relu"), other], "sum", name="add")
    steps, nf = _fused_norm(tail)
    norm, = [s for s in steps if s[0] == "instancenormalization_q4"]
    assert nf == 1 and norm[1]["act"] == ACT_RELU and norm[2][3] == "None"       # relu folded, the add behind it is not
    assert [s[0] for s in steps].count("add_q4") == 1


def test_fuse_refused_when_the_rewritten_tensor_has_another_reader():
    def tail(g, n, other):
        r = g.op("relu", n, "r", name="relu")
        return g.op("add", [r, "ca"], "sum", name="add")      # `ca` is the buffer the norm rewrites in place
    steps, nf = _fused_norm(tail)
    assert nf == 0


# ---- stale converted copies -------------------------------------------------------------------------------------------------
def _flow_text(body, flow):
    k = {b[0]: b[1] for b in body}
    return ["%s %s -> %s" % (k[names[0]], ",".join(src), dst) for src, names, dst in flow]


def test_converted_copies_are_dropped_when_an_nchw_norm_rewrites_their_tensor(monkeypatch):
    """(a) x is NCHW with a cached Q4 copy (made for a conv): an instance norm on x that stays NCHW rewrites x, so the next conv
    must convert x again.  (b) c is Q4 with a cached NCHW copy: a norm that has to stay NCHW (switch off) works on a copy, the Q4
    tensor is made again from it for the later Q4 reader, and a later NCHW reader does not get the copy from before the norm."""
    rng = np.random.default_rng(3)
    kw = dict(group=1, strides=[1, 1], dilations=[1, 1], pads=[1, 1, 1, 1])

    def weights(g):
        for tag in ("a", "b"):
            g.init(tag + "_w", (rng.standard_normal((4, 4, 3, 3)) * 0.2).astype(np.float32))
        g.init("s", rng.uniform(0.5, 1.5, 4).astype(np.float32))
        g.init("t", rng.standard_normal(4).astype(np.float32))
    x = rng.standard_normal((1, 4, 5, 5)).astype(np.float32)

    g = GraphBuilder(["x"])
    weights(g)
    g.op("conv", ["x", "a_w"], "ca", name="conv_a", **kw)
    g.op("instancenormalization", ["x", "s", "t"], "n", name="norm", epsilon=1e-5)
    g.op("conv", ["x", "b_w"], "cb", name="conv_b", **kw)
    g.op("add", ["ca", "cb"], "sum", name="add")
    graph, blob = g.finish(["sum"])
    shapes = shapes_of(graph, blob, x)
    inits = [i[0] for i in graph["inits"]]
    body, flow, _ = assign_layouts(graph["layers"], graph["flow"], inits, shapes, force=True, values=blob_inits(graph, blob).get)
    text = _flow_text(body, flow)
    assert text.count("to_q4 x -> x@q4") == 2 and text.index("instancenormalization x,s,t -> n") < len(text) - 1 - text[::-1].index("to_q4 x -> x@q4"), text
    assert_close(_run(graph, blob, x, body, flow), _run(graph, blob, x, graph["layers"], graph["flow"]), 1e-5)

    monkeypatch.setenv("PLANER_HIP_INSTNORM_Q4", "0")
    g = GraphBuilder(["x"])
    weights(g)
    g.init("shape", np.array([1, -1], np.int64))
    g.op("conv", ["x", "a_w"], "ca", name="conv_a", **kw)
    g.op("reshape", ["ca", "shape"], "flat0", name="reshape0")            # an NCHW reader: caches ca@nchw
    g.op("instancenormalization", ["ca", "s", "t"], "n", name="norm", epsilon=1e-5)
    g.op("reshape", ["ca", "shape"], "flat1", name="reshape1")            # must see the normalised values
    g.op("conv", ["ca", "b_w"], "cb", name="conv_b", **kw)                # ... and so must this Q4 reader
    g.op("reshape", ["cb", "shape"], "flat2", name="reshape2")
    g.op("concat", ["flat0", "flat1", "flat2"], "all", name="cat", axis=1)
    graph, blob = g.finish(["all"])
    shapes = shapes_of(graph, blob, x)
    inits = [i[0] for i in graph["inits"]]
    body, flow, _ = assign_layouts(graph["layers"], graph["flow"], inits, shapes, force=True, values=blob_inits(graph, blob).get)
    text = _flow_text(body, flow)
    assert "instancenormalization ca@nchw,s,t -> n" in text and "to_q4 ca@nchw -> ca" in text, text
    assert text.count("from_q4 ca -> ca@nchw") == 2, text
    assert_close(_run(graph, blob, x, body, flow), _run(graph, blob, x, graph["layers"], graph["flow"]), 1e-5)


# ---- pad predicate and the switch -----------------------------------------------------------------------------------------------
def test_pad_goes_q4_only_for_pixel_pads_with_a_padding_safe_constant():
    assert pad_q4_ok(3, [0, 0, 1, 2, 0, 0, 3, 4], 0, "reflect") and pad_q4_ok(3, [0, 0, 1, 2, 0, 0, 3, 4], 0.0, "constant")
    assert pad_q4_ok(8, [0, 0, 1, 1, 0, 0, 1, 1], 2.5, "constant") and not pad_q4_ok(3, [0, 0, 1, 1, 0, 0, 1, 1], 2.5, "constant")
    assert pad_q4_ok(3, [0, 0, 1, 1, 0, 0, 1, 1], 2.5, "edge")                      # the value only counts in constant mode
    assert not pad_q4_ok(8, [0, 1, 1, 1, 0, 0, 1, 1], 0, "constant") and not pad_q4_ok(8, [0, 0, 1, 1, 1, 0, 1, 1], 0, "edge")
    assert not pad_q4_ok(8, [0, 0, 1, 1], 0, "constant") and not pad_q4_ok(8, [0, 0, 1, 1, 0, 0, 1, 1], 0, "mean")
    # without the constants' values the compiler cannot tell: pad stays NCHW
    g, b = stylenet.build()
    x = stylenet.make_input(1, size=32)
    shapes = shapes_of(g, b, x)
    body, _, _ = assign_layouts(g["layers"], g["flow"], [i[0] for i in g["inits"]], shapes, force=True)
    assert not any(e[1] == "pad_q4" for e in body) and any(e[1] == "instancenormalization_q4" for e in body)


def test_switch_off_gives_the_program_of_a_compiler_without_the_new_kinds(style, monkeypatch):
    """tests/golden/stylenet_plan_before.json is what the plan compiler gave for this graph before it knew the two kinds
    (fuse_flow + assign_layouts(force=True) at size 32, as JSON: at that size the cost estimate turns the conversion-ridden
    program down, so it is forced on both sides)."""
    g, b, x = style
    monkeypatch.setenv("PLANER_HIP_INSTNORM_Q4", "0")
    body, flow, nq4, nf, _ = _compile(g, b, x, force=True)
    want = json.load(open(os.path.join(GOLDEN, "stylenet_plan_before.json")))
    assert nf == 0 and nq4 == want["nq4"]
    assert json.loads(json.dumps(body)) == want["body"] and json.loads(json.dumps(flow)) == want["flow"]
    names = [s[0] for s in steps_of(body, flow)]
    assert names.count("from_q4") >= 15 and "pad_q4" not in names and "instancenormalization_q4" not in names

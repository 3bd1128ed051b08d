"""Dilated 3x3 convs folded by pixel phase (plan.fold_dilated, tests/fold_ref.py).  Host logic only.

The identity -- a 3x3 / stride 1 conv with dilation d and pads d is the pad 1 / dilation 1 conv on the folded tensor -- in float64
on integer operands, exactly; the pass on the dilated ResNet-18 (planer_amd.irgen.drn) on maps the dilations divide (size 64:
8 x 8) and maps they do not (size 40: 5 x 5); and the rewritten program against the original on integer operands, exactly,
through a small float64 evaluator of the kinds a folded region can hold.

Refold counts on DRN.  Size 64: five -- layer3.0's conv b input and residual, 2 -> 4 for layer4.0's conv b input and residual,
one unfold behind the head conv.  Size 40: every conv folds alone; seven inputs, seven outputs and TWO residuals, sixteen in
all -- the residuals of layer3.1's and layer4.1's conv b are the tensors their conv a read, and that folded copy is cached."""
import json
import os

import numpy as np
import pytest

from planer_amd.irgen import drn
from planer_amd.irgen.builder import GraphBuilder
from planer_amd.plan import fold_dilated, folded_key
from tests import ref64
from tests.conftest import GOLDEN
from tests.fold_ref import fold_np, folded_shape, refold_np, unfold_np
from tests.plan_audit import cpu_front, steps_of

ALWAYS = lambda xs, ks, para: True          # noqa: E731
NEVER = lambda xs, ks, para: False          # noqa: E731

# (x shape, (dh, dw), group): the geometries of the issue's table; d does not divide the map in most of them
IDENTITY = [((2, 8, 8, 8), (2, 2), 1), ((1, 4, 12, 8), (4, 2), 1), ((2, 5, 7, 9), (2, 2), 1), ((1, 8, 5, 6), (3, 4), 2),
            ((1, 4, 3, 3), (4, 4), 1), ((3, 4, 28, 28), (4, 4), 1), ((1, 4, 13, 10), (6, 6), 1)]


@pytest.mark.parametrize("xs,d,group", IDENTITY, ids=["%s-d%dx%d" % ("x".join(map(str, c[0])), c[1][0], c[1][1]) for c in IDENTITY])
def test_folded_conv_is_the_dilated_conv_exactly(xs, d, group):
    rng = np.random.default_rng(sum(xs) * 31 + d[0])
    ks = (8, xs[1] // group, 3, 3)
    geo = dict(group=group, strides=(1, 1), dilations=d, pads=(d[0], d[1], d[0], d[1]))
    x, K, B, sc, sh, res = ref64.int_operands(rng, xs, ks, bias=True, bn=True, res=True, **geo)
    ref64.assert_exact(x, K, B, sc, sh, res, **geo)
    want = ref64.ref64(x, K, B, sc, sh, res, act=ref64.ACT_RELU, **geo)
    one = dict(group=group, strides=(1, 1), dilations=(1, 1), pads=(1, 1, 1, 1))
    got = ref64.ref64(fold_np(x, *d), K, B, sc, sh, fold_np(res, *d), act=ref64.ACT_RELU, **one)
    assert got.shape == folded_shape(want.shape, *d)
    assert np.array_equal(unfold_np(got, d[0], d[1], xs[2], xs[3]), want)


def test_refold_composes_and_two_folded_convs_chain_only_on_dividing_maps():
    rng = np.random.default_rng(5)
    x = ref64.int_tensor(rng, (2, 5, 12, 9))
    assert np.array_equal(refold_np(fold_np(x, 2, 2), (2, 2), (4, 4), 12, 9), fold_np(x, 4, 4))
    assert np.array_equal(refold_np(fold_np(x, 2, 2), (2, 2), (3, 3), 12, 9), fold_np(x, 3, 3))
    assert np.array_equal(unfold_np(fold_np(x, 4, 2), 4, 2, 12, 9), x)
    geo = dict(strides=(1, 1), dilations=(2, 2), pads=(2, 2, 2, 2))
    one = dict(strides=(1, 1), dilations=(1, 1), pads=(1, 1, 1, 1))
    for side, chains in ((8, True), (7, False)):
        x = ref64.int_tensor(rng, (1, 4, side, side))
        K1, K2 = ref64.int_tensor(rng, (4, 4, 3, 3)), ref64.int_tensor(rng, (4, 4, 3, 3))
        want = ref64.conv64(ref64.conv64(x, K1, **geo), K2, **geo)
        got = unfold_np(ref64.conv64(ref64.conv64(fold_np(x, 2, 2), K1, **one), K2, **one), 2, 2, side, side)
        assert np.array_equal(got, want) == chains           # on 7 x 7 the second conv reads the first one's junk as padding


# ---- a float64 evaluator of the kinds a folded region can hold ------------------------------------------------------------------
class _T:
    """An activation: float64 NCHW values (folded or not) and the fold (dh, dw, H, W) a DeviceArray would carry."""
    def __init__(self, a, fold=None):
        self.a, self.fold = a, fold


def _evaluate(graph, blob, x, body, flow):
    vals, pos = {"None": None}, 0
    for name, shape, dt in graph["inits"]:
        n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
        vals[name] = blob[pos:pos + n].view(dt).reshape(shape).astype(np.float64)
        pos += n
    vals[graph["input"][0]] = _T(np.array(x, np.float64))
    kinds = {b[0]: b for b in body}
    out = None
    for src, names, dst in flow:
        _, kind, para = kinds[names[0]]
        args = [vals[k] for k in (src if isinstance(src, list) else [src])]
        acts = [a for a in args if isinstance(a, _T)]
        if kind in ("to_q4", "from_q4"):
            assert acts[0].fold is None, "a layout conversion reads an unfolded tensor"
            y = _T(acts[0].a.copy())
        elif kind == "conv_q4":
            xa, K, B, sc, sh, res = (args + [None] * 6)[:6]
            assert res is None or res.fold == xa.fold, "the residual is folded like the input"
            geo = {k: para[k] for k in ("group", "strides", "dilations", "pads")}
            r = ref64.ref64(xa.a, K, B, sc, sh, None if res is None else res.a, act=para.get("act", 0),
                            alpha=para.get("alpha", 0.0), **geo)
            assert xa.fold is None or r.shape[2:] == xa.a.shape[2:]
            y = _T(r, xa.fold)
        elif kind == "relu_q4":
            acts[0].a *= acts[0].a > 0                    # in place, like ReLUQ4
            y = acts[0]
        elif kind == "add_q4":
            assert acts[0].fold == acts[1].fold and acts[0].a.shape == acts[1].a.shape
            y = _T(acts[0].a + acts[1].a, acts[0].fold)
        elif kind == "batchnorm_q4":
            y = _T(acts[0].a * args[1].reshape(1, -1, 1, 1) + args[2].reshape(1, -1, 1, 1), acts[0].fold)
        elif kind == "concat_q4":
            assert len({a.fold for a in acts}) == 1
            y = _T(np.concatenate([a.a for a in acts], axis=1), acts[0].fold)
        elif kind == "refold_q4":
            t = acts[0]
            dh, dw, h, w = t.fold if t.fold is not None else (1, 1) + t.a.shape[2:]
            assert [dh, dw] == list(para["from"]), (src, para, t.fold)
            to = tuple(para["to"])
            y = _T(refold_np(t.a, (dh, dw), to, h, w), to + (h, w) if to != (1, 1) else None)
        elif kind == "return":
            y = acts[0]
        else:
            raise AssertionError("evaluator: kind %r" % kind)
        assert kind in ("conv_q4", "relu_q4", "add_q4", "batchnorm_q4", "concat_q4", "refold_q4") or all(a.fold is None for a in acts)
        vals[dst] = out = y
    assert out.fold is None, "the program's result is unfolded"
    return out.a


def _compile(g, b, x, worth=ALWAYS):
    """The compiler's front half up to the pass (forced Q4), and what the pass makes of that program."""
    body, flow, _, shapes = cpu_front(g, b, x, force=True, stop="fuse_linear_add")
    fbody, fflow, regions = fold_dilated(body, flow, shapes, worth)
    return (body, flow), (fbody, fflow), regions, shapes


def _refolds(body, flow):
    return [(src[0], tuple(p["from"]), tuple(p["to"]), dst) for kind, p, src, dst, _ in steps_of(body, flow) if kind == "refold_q4"]


class _Ints:
    """Graphs with integer weights and power-of-two BatchNorm scales: every sum is exact in float32 and float64."""
    def __init__(self, seed, cin):
        self.rng, self.g, self.cin = np.random.default_rng(seed), GraphBuilder(["x"]), cin

    def conv(self, src, cin, cout, k, d, tag, bn=True, relu=False, p=None):
        g, rng = self.g, self.rng
        g.init(tag + "_w", ref64.int_tensor(rng, (cout, cin, k, k), -2, 2))
        p = (d * (k // 2)) if p is None else p
        y = g.op("conv", [src, tag + "_w"], tag + "_c", name=tag + "_conv", group=1, strides=[1, 1], dilations=[d, d], pads=[p] * 4)
        if bn:
            g.init(tag + "_K", rng.choice([0.5, 1.0, 2.0, -1.0], cout).reshape(1, -1, 1, 1).astype(np.float32))
            g.init(tag + "_B", rng.integers(-4, 5, cout).reshape(1, -1, 1, 1).astype(np.float32))
            y = g.op("batchnorm", [y, tag + "_K", tag + "_B"], tag + "_b", name=tag + "_bn")
        if relu:
            y = g.op("relu", y, tag + "_r", name=tag + "_relu")
        return y

    def block(self, src, cin, cout, da, db, tag):
        y = self.conv(src, cin, cout, 3, da, tag + "a", relu=True)
        y = self.conv(y, cout, cout, 3, db, tag + "b")
        if cin != cout:
            src = self.conv(src, cin, cout, 1, 1, tag + "d")
        s = self.g.op("add", [y, src], tag + "_s", name=tag + "_add")
        return self.g.op("relu", s, tag + "_o", name=tag + "_out")

    def finish(self, y, n, side):
        graph, blob = self.g.finish([y])
        return graph, blob, ref64.int_tensor(self.rng, (n, self.cin, side, side), -2, 2)


def _drn_slice(side):
    """DRN's layer3 and layer4 (irgen/drn.py) at 4 -> 8 -> 8 channels, and its 1x1 head with a bias."""
    m = _Ints(side, 4)
    y = m.block("x", 4, 8, 1, 2, "l30")
    y = m.block(y, 8, 8, 2, 2, "l31")
    y = m.block(y, 8, 8, 2, 4, "l40")
    y = m.block(y, 8, 8, 4, 4, "l41")
    m.g.init("head_w", ref64.int_tensor(m.rng, (3, 8, 1, 1), -2, 2))
    m.g.init("head_b", m.rng.integers(-4, 5, 3).astype(np.float32))
    y = m.g.op("conv", [y, "head_w", "head_b"], "head", name="head_conv", group=1, strides=[1, 1], dilations=[1, 1], pads=[0] * 4)
    return m.finish(y, 2, side)


def _same(g, b, x, before, after):
    want = _evaluate(g, b, x, *before)
    got = _evaluate(g, b, x, *after)
    assert want.shape == got.shape and np.abs(want).max() < 2.0 ** 40 and np.array_equal(got, want)
    return want


@pytest.mark.parametrize("side,nrefold", [(8, 5), (5, 16)])
def test_drn_slice_rewritten_equals_original_exactly(side, nrefold):
    g, b, x = _drn_slice(side)
    before, after, regions, _ = _compile(g, b, x)
    assert len(_refolds(*after)) == nrefold and sum(len(r["heads"]) for r in regions) == 7
    _same(g, b, x, before, after)


# ---- the pass on DRN -----------------------------------------------------------------------------------------------------
HEADS = ["l30b", "l31a", "l31b", "l40a", "l40b", "l41a", "l41b"]


_DRN = {}


def _drn(size):
    """(size, graph, program before, program after, regions, shapes) of DRN at `size`, compiled once."""
    if size not in _DRN:
        g, b = drn.build()
        _DRN[size] = (size, g) + _compile(g, b, drn.make_input(1, size=size))
    return _DRN[size]


@pytest.fixture(params=[64, 40], ids=["size64", "size40"])
def drn_plan(request):
    return _drn(request.param)


def test_generator_op_census():
    g, _ = drn.build()
    census = {}
    for _, kind, _ in g["layers"]:
        census[kind] = census.get(kind, 0) + 1
    assert census == {"conv": 21, "batchnorm": 20, "relu": 17, "maxpool": 1, "add": 8, "upsample": 1, "return": 1}
    dil = [(n, p["dilations"], p["pads"]) for n, k, p in g["layers"] if k == "conv" and p["dilations"] != [1, 1]]
    assert [n[:4] for n, _, _ in dil] == HEADS and all(p == d + d for _, d, p in dil)
    assert [d[0] for _, d, _ in dil] == [2, 2, 2, 2, 4, 4, 4]


def test_all_seven_heads_run_at_dilation_one_on_their_own_filter_keys(drn_plan):
    size, g, before, after, regions, shapes = drn_plan
    was = {s[4]: s for s in steps_of(*before)}
    heads = [s for s in steps_of(*after) if s[0] == "conv_q4" and was[s[4]][1]["dilations"] != [1, 1]]
    assert [s[4][:4] for s in heads] == HEADS
    for kind, para, src, dst, name in heads:
        d = was[name][1]["dilations"]
        assert para["dilations"] == [1, 1] and para["pads"] == [1, 1, 1, 1] and was[name][1]["pads"] == d + d
        assert src[1] == was[name][2][1] == name[:4] + "_w" and src[2:5] == was[name][2][2:5]
        assert {k: v for k, v in para.items() if k not in ("dilations", "pads")} == \
            {k: v for k, v in was[name][1].items() if k not in ("dilations", "pads")}
        # the input, the residual and the output are folded by the conv's dilation, and `shapes` knows the folded shapes
        for key, orig in ((src[0], was[name][2][0]), (src[5], was[name][2][5]), (dst, was[name][3])):
            if orig == "None":
                assert key == "None"
                continue
            assert key in (folded_key(orig, d), folded_key(orig, d, junk=True)) and key != orig
            assert tuple(shapes[key.split("@")[0]]) == folded_shape(shapes[orig.split("@")[0]], *d)
    assert sorted(n for r in regions for n in r["heads"]) == sorted(s[4] for s in heads)


def test_regions_and_refolds_on_dividing_maps():
    size, g, before, after, regions, shapes = _drn(64)
    assert [(r["fold"], r["dividing"], [n[:4] for n in r["steps"]]) for r in regions] == [
        ([2, 2], True, ["l30b", "l31a", "l31b", "l40a", "l40d"]), ([4, 4], True, ["l40b", "l41a", "l41b", "head"])]
    assert _refolds(*after) == [("l30a_r", (1, 1), (2, 2), "l30a_r~2x2"), ("l30d_b", (1, 1), (2, 2), "l30d_b~2x2"),
                                ("l40a_r~2x2", (2, 2), (4, 4), "l40a_r~4x4"), ("l40d_b~2x2", (2, 2), (4, 4), "l40d_b~4x4"),
                                ("head~4x4", (4, 4), (1, 1), "head")]
    names = [s[0] for s in steps_of(*after)]
    assert names[-3:] == ["from_q4", "upsample", "return"] and names[-4] == "refold_q4"
    assert tuple(shapes["l40_o~4x4"]) == (16, 512, 2, 2) and tuple(shapes["l31_o~2x2"]) == (4, 256, 4, 4)
    # the 1x1 projection of layer4.0 and the head conv joined: they read and write folded tensors
    s = {x[4]: x for x in steps_of(*after)}
    assert s["l40d_conv+"][2][0] == "l31_o~2x2" and s["l40d_conv+"][3] == "l40d_b~2x2"
    assert s["head_conv"][2][0] == "l41_o~4x4" and s["head_conv"][3] == "head~4x4"


def test_every_conv_folds_alone_on_maps_the_dilation_does_not_divide():
    size, g, before, after, regions, shapes = _drn(40)
    assert [(r["dividing"], [n[:4] for n in r["steps"]]) for r in regions] == [(False, [h]) for h in HEADS]
    re = _refolds(*after)
    ins = [r for r in re if r[1] == (1, 1)]
    outs = [r for r in re if r[2] == (1, 1)]
    assert len(re) == 16 and len(outs) == 7 and len(ins) == 9 and not [r for r in re if (1, 1) not in r[1:3]]
    # seven inputs and the residuals of layer3.0 / layer4.0 (their projections); the other two residuals are cached copies
    assert [r[0] for r in ins] == ["l30a_r", "l30d_b", "l30_o", "l31a_r", "l31_o", "l40a_r", "l40d_b", "l40_o", "l41a_r"]
    steps = steps_of(*after)
    for i, s in enumerate(steps):
        if s[0] == "conv_q4" and s[4][:4] in HEADS:          # in, conv, out: the junk-tailed output has one reader, its unfold
            assert steps[i + 1][0] == "refold_q4" and steps[i + 1][2] == [s[3]] and steps[i + 1][1]["to"] == [1, 1]
            assert s[3].split("@")[0].endswith("j") and sum(s[3] in t[2] for t in steps) == 1
    s = {x[4]: x for x in steps}
    assert s["l31b_conv+"][2][5] == "l30_o~2x2" and s["l31a_conv+"][2][0] == "l30_o~2x2"
    assert s["l40d_conv+"][2][0] == "l31_o" and s["head_conv"][2][0] == "l41_o"          # not members: unfolded operands


def test_worth_never_returns_the_input_program(drn_plan):
    size, g, before, after, regions, shapes = drn_plan
    known = dict(shapes)
    body, flow, regions = fold_dilated(before[0], before[1], shapes, NEVER)
    assert regions == [] and json.loads(json.dumps(body)) == json.loads(json.dumps(before[0]))
    assert json.loads(json.dumps(flow)) == json.loads(json.dumps(before[1])) and shapes == known


def test_worth_is_asked_per_head_with_the_unfolded_shapes():
    g, b = drn.build()
    x = drn.make_input(1, size=64)
    asked = []

    def only_d4(xs, ks, para):
        asked.append((tuple(xs), tuple(ks), para["dilations"]))
        return para["dilations"] == [4, 4]
    _, after, regions, _ = _compile(g, b, x, only_d4)
    assert asked == [((1, 256, 8, 8), (256, 256, 3, 3), [2, 2])] * 3 + [((1, 256, 8, 8), (512, 256, 3, 3), [2, 2])] + \
        [((1, 512, 8, 8), (512, 512, 3, 3), [4, 4])] * 3
    assert [(r["fold"], [n[:4] for n in r["steps"]]) for r in regions] == [([4, 4], ["l40b", "l41a", "l41b", "head"])]
    assert [(r[1], r[2]) for r in _refolds(*after)] == [((1, 1), (4, 4))] * 2 + [((4, 4), (1, 1))]


def test_switch_off_program_is_the_parents(drn_plan):
    """tests/golden/drn_plan_before.json: fuse_flow + assign_layouts + fuse_instnorm_q4 on DRN at sizes 64 and 40, written by the
    plan compiler before it had the pass.  With the switch off Net._fuse gives plan.compile_front no `worth`, which leaves it out."""
    size = drn_plan[0]
    g, b = drn.build()
    body, flow, counts, _ = cpu_front(g, b, drn.make_input(1, size=size))
    nf, nq4 = counts["fuse_flow"], counts["assign_layouts"]
    want = json.load(open(os.path.join(GOLDEN, "drn_plan_before.json")))[str(size)]
    assert (nf, nq4) == (want["nfused"], want["nq4"])
    assert json.loads(json.dumps(body)) == want["body"] and json.loads(json.dumps(flow)) == want["flow"]
    assert not any(b_[1] == "refold_q4" for b_ in body)


def test_net_reads_the_switch(monkeypatch):
    import planer_amd.net as pnet
    for val, want in ((None, False), ("0", False), ("1", True), ("force", "force")):
        if val is None:
            monkeypatch.delenv("PLANER_HIP_DILATED_FOLD", raising=False)
        else:
            monkeypatch.setenv("PLANER_HIP_DILATED_FOLD", val)
        net = pnet.Net(ctx=object())
        assert net.fold_dilated == want and net.dilated_folds == 0 and net.refolds == 0


# ---- hazard graphs --------------------------------------------------------------------------------------------------------
def test_in_place_relu_on_a_folded_tensor_with_a_later_unfolded_reader():
    m = _Ints(11, 4)
    c0 = m.conv("x", 4, 4, 3, 1, "c0", relu=True)
    h = m.conv(c0, 4, 4, 3, 2, "h")                      # a head; two readers, so the relu below is not absorbed
    r = m.g.op("relu", h, "r", name="relu")              # in place on the folded tensor ...
    u = m.conv(h, 4, 4, 3, 1, "u", bn=False)             # ... whose unfolded copy is made AFTER it: relu'd values
    y = m.g.op("add", [r, u], "sum", name="add")
    g, b, x = m.finish(y, 1, 8)
    before, after, regions, _ = _compile(g, b, x)
    steps = steps_of(*after)
    kinds = [s[0] for s in steps]
    assert kinds.count("relu_q4") == 1 and steps[kinds.index("relu_q4")][2] == ["h_b~2x2"] and steps[kinds.index("relu_q4")][3] == "r~2x2"
    # (fuse_flow made the add the residual of conv u, which is no member: both its operands are unfolded, behind the relu)
    assert _refolds(*after) == [("c0_r", (1, 1), (2, 2), "c0_r~2x2"), ("h_b~2x2", (2, 2), (1, 1), "h_b"), ("r~2x2", (2, 2), (1, 1), "r")]
    assert kinds.index("relu_q4") < [s[3] for s in steps].index("h_b")
    assert regions[0]["steps"] == ["h_conv+", "relu"]
    _same(g, b, x, before, after)


def test_unfolded_copy_cached_before_an_in_place_relu_is_dropped():
    m = _Ints(12, 4)
    c0 = m.conv("x", 4, 4, 3, 1, "c0", relu=True)
    h = m.conv(c0, 4, 4, 3, 2, "h")
    u1 = m.conv(h, 4, 4, 3, 1, "u1", bn=False)           # unfolded reader BEFORE the relu: caches the unfolded copy
    r = m.g.op("relu", h, "r", name="relu")
    u2 = m.conv(h, 4, 4, 3, 1, "u2", bn=False)           # unfolded reader AFTER it: must not get that copy
    y = m.g.op("add", [m.g.op("add", [r, u1], "s1", name="add1"), u2], "s2", name="add2")
    g, b, x = m.finish(y, 1, 8)
    before, after, _, _ = _compile(g, b, x)
    assert [r_[:3] for r_ in _refolds(*after)].count(("h_b~2x2", (2, 2), (1, 1))) == 2
    _same(g, b, x, before, after)


def test_operand_produced_outside_the_region_is_folded_in():
    m = _Ints(13, 4)
    c0 = m.conv("x", 4, 4, 3, 1, "c0", relu=True)
    side = m.conv("x", 4, 4, 1, 1, "side")               # (fuse_flow makes add2 its residual: it joins, and the net's input is folded in)
    h = m.conv(c0, 4, 4, 3, 2, "h")
    s = m.g.op("add", [h, c0], "s", name="add")          # c0 is folded already (the head read it); h has two readers
    t = m.g.op("add", [side, h], "t", name="add2")       # the folded operand comes second
    y = m.conv(m.g.op("add", [s, t], "v", name="add3"), 4, 4, 3, 2, "z")
    g, b, x = m.finish(y, 2, 8)
    before, after, regions, _ = _compile(g, b, x)
    re = _refolds(*after)
    assert [r[0] for r in re] == ["c0_r", "x@q4", "z_b~2x2"] and len(regions) == 1 and len(regions[0]["heads"]) == 2
    _same(g, b, x, before, after)


def test_two_heads_of_different_dilation_on_one_source_keep_separate_copies():
    m = _Ints(14, 4)
    c0 = m.conv("x", 4, 4, 3, 1, "c0", relu=True)
    a = m.conv(c0, 4, 4, 3, 2, "a", relu=True)
    c = m.conv(c0, 4, 4, 3, 4, "c", relu=True)
    e = m.conv(c0, 4, 4, 3, 2, "e", relu=True)           # takes the cached 2 x 2 copy
    cat = m.g.op("concat", [a, c, e], "cat", name="cat", axis=1)
    y = m.conv(cat, 12, 4, 1, 1, "mix")
    g, b, x = m.finish(y, 1, 8)
    before, after, regions, _ = _compile(g, b, x)
    assert _refolds(*after) == [("c0_r", (1, 1), (2, 2), "c0_r~2x2"), ("c0_r", (1, 1), (4, 4), "c0_r~4x4"),
                                ("c_r~4x4", (4, 4), (2, 2), "c_r~2x2"), ("mix_b~2x2", (2, 2), (1, 1), "mix_b")]
    assert [r["fold"] for r in regions] == [[2, 2], [4, 4]]
    assert regions[0]["steps"] == ["a_conv+", "e_conv+", "cat", "mix_conv+"]
    _same(g, b, x, before, after)


@pytest.mark.parametrize("side", [8, 7])
def test_a_region_that_ends_the_program_is_unfolded(side):
    rng = np.random.default_rng(side)
    K = ref64.int_tensor(rng, (4, 4, 3, 3), -2, 2)
    g = {"input": ["x"], "inits": [["w", [4, 4, 3, 3], "float32"]]}
    para = {"group": 1, "strides": [1, 1], "dilations": [2, 2], "pads": [2, 2, 2, 2], "act": 1}
    body = [["c1", "conv_q4", dict(para)], ["c2", "conv_q4", dict(para)]]
    flow = [[["x", "w", "None", "None", "None", "None"], ["c1"], "y1"], [["y1", "w", "None", "None", "None", "x"], ["c2"], "y2"]]
    shapes = {"x": (1, 4, side, side), "w": (4, 4, 3, 3), "y1": (1, 4, side, side), "y2": (1, 4, side, side)}
    fbody, fflow, regions = fold_dilated(body, flow, shapes)
    assert steps_of(fbody, fflow)[-1][0] == "refold_q4" and fflow[-1][2] == "y2" and len(_refolds(fbody, fflow)) == (2 if side == 8 else 4)
    x = ref64.int_tensor(rng, (1, 4, side, side))
    _same(g, K.view(np.uint8).reshape(-1), x, (body, flow), (fbody, fflow))


def test_what_is_no_head():
    """Strided, asymmetric-pad, 5x5, depthwise and Cin % 4 != 0 dilated convs stay as they are."""
    base = {"group": 1, "strides": [1, 1], "dilations": [2, 2], "pads": [2, 2, 2, 2]}
    cases = [(dict(base, strides=[2, 2]), (8, 8, 3, 3)), (dict(base, pads=[1, 1, 1, 1]), (8, 8, 3, 3)), (dict(base, pads=[4, 4, 4, 4]), (8, 8, 5, 5)),
             (dict(base, group=8), (8, 1, 3, 3)), (base, (8, 6, 3, 3)), (dict(base, dilations=[1, 1], pads=[1, 1, 1, 1]), (8, 8, 3, 3)),
             (dict(base, rowpack=True), (8, 8, 3, 3))]
    for para, ks in cases:
        cin = ks[1] * para["group"]
        shapes = {"x": (1, cin, 8, 8), "w": ks, "y": (1, 8, 8, 8)}
        _, flow, regions = fold_dilated([["c", "conv_q4", para]], [[["x", "w"], ["c"], "y"]], shapes)
        assert regions == [] and flow == [[["x", "w"], ["c"], "y"]], (para, ks)
    shapes = {"x": (1, 8, 8, 8), "w": (8, 8, 3, 3), "y": (1, 8, 8, 8)}
    _, flow, regions = fold_dilated([["c", "conv_q4", dict(base, dilations=[2, 1], pads=[2, 1, 2, 1])]], [[["x", "w"], ["c"], "y"]], shapes)
    assert len(regions) == 1 and regions[0]["fold"] == [2, 1] and tuple(shapes["x~2x1"]) == (2, 8, 4, 8)

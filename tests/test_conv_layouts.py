"""The w_layout table (planer_amd/conv_layouts.py) on the CPU: the persisted codes and their report names, the candidate
order the conv picker times, and the code + filter key every conv of the generator nets gets."""
import collections
import glob
import json
import os

import pytest

from planer_amd import conv_layouts as cl
from planer_amd import net as net_mod
from planer_amd.irgen import customnet, mobilenetv2, resnet18, unet, yolov3
from planer_amd.plan import compile_front
from tests.conftest import ROOT
from tests.test_plan_fusion import shapes_of

SWITCHES = ("PLANER_HIP_WINOGRAD", "PLANER_HIP_WINOGRAD4", "PLANER_HIP_WF4", "PLANER_HIP_WINOGRAD43", "PLANER_HIP_ROWPACK")

# the report names as they were before the table existed: tools compare them across checkouts
NAMES = {0: "igemm-nchw", 1: "tap-nchw", 2: "direct-q4 (conv_q4_kernel)", 3: "wino2x2-nchw",
         4: "wino2x2-q4 (transforms + grouped conv_q4_kernel)",
         6: "rowpack-q4 (nchw_to_rowpack + conv_q4_kernel)",
         7: "wino4x4-q4 (transforms + grouped conv_q4_kernel)", 8: "w1d4 F(4,3) (conv_w1d4_kernel)",
         9: "wf4 fused F(4x4,3x3) (conv_wf4_kernel)", 10: "stem + maxpool (conv_stem_pool_kernel)",
         11: "wino43-q4 (mixed F(4,3) x F(3,3) tiles: transforms + 121 grouped conv_q4_kernel)",
         12: "stem + maxpool (conv_stem_pool_kernel)",
         13: "depthwise-q4 (conv_dw_kernel)",
         14: "convt-q4 (phase-decomposed convt_q4_kernel)"}


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def test_codes_and_report_names_are_the_persisted_ones():
    assert {c: lay.name for c, lay in cl.LAYOUTS.items()} == NAMES
    assert net_mod.W_LAYOUT_NAMES == NAMES
    assert cl.STAGED_LAYOUTS == {7: "wino4", 11: "wino43"}
    suffixes = {c: cl.suffix(c, {"group": 2, "strides": [2, 1]}) for c, lay in cl.LAYOUTS.items() if lay.suffix}
    assert suffixes == {1: "@tap", 2: "@q4g2", 3: "@wino", 4: "@winoq4", 6: "@rowpack", 7: "@wino4q4", 8: "@w1d4q4", 9: "@wf4q4",
                        10: "@rowpack", 11: "@wino43q4", 12: "@stemnchw", 13: "@dwq4", 14: "@convt2x1"}
    assert all(lay.prepare is not None and lay.eligible is not None for c, lay in cl.LAYOUTS.items() if c)


def test_every_shipped_pick_is_in_the_table():
    paths = glob.glob(os.path.join(ROOT, "planer_amd", "tuned", "*.algo.json"))
    assert paths
    for path in paths:
        with open(path) as f:
            stored = json.load(f)
        codes = {int(v) for table in ("algo", "algo_throughput") for v in stored.get(table, {}).values()}
        assert codes and codes <= set(cl.LAYOUTS), (path, codes - set(cl.LAYOUTS))


def _choose(kind, k_shape, x_shape, rowpack=False, **para):
    seen = []

    def pick(cands):
        seen.append(list(cands))
        return cands[-1]
    got = cl.choose(kind, k_shape, para, x_shape, rowpack, pick)
    return got, (seen[0] if seen else None)


S1 = {"strides": [1, 1], "pads": [1, 1, 1, 1], "dilations": [1, 1], "group": 1}


@pytest.mark.parametrize("case, kind, k_shape, x_shape, para, rowpack, expect", [
    # 3x3 / s1 / p1 on a 14x14 map: every Q4 family, the mixed tiles where the batch gives each GEMM 64 tile columns
    ("3x3 s1 14x14 b32", "conv_q4", (256, 256, 3, 3), (32, 256, 14, 14), S1, False, ((11, "@wino43q4"), [2, 8, 4, 7, 9, 11])),
    ("3x3 s1 14x14 b8", "conv_q4", (256, 256, 3, 3), (8, 256, 14, 14), S1, False, ((9, "@wf4q4"), [2, 8, 4, 7, 9])),
    ("3x3 s1 56x56", "conv_q4", (64, 64, 3, 3), (32, 64, 56, 56), S1, False, ((9, "@wf4q4"), [2, 8, 4, 7, 9])),
    ("3x3 s1 Cout % 4", "conv_q4", (6, 8, 3, 3), (1, 8, 56, 56), S1, False, ((8, "@w1d4q4"), [2, 8])),
    ("3x3 s1 NCHW", "conv_fused", (64, 64, 3, 3), (32, 64, 56, 56), S1, False, ((3, "@wino"), [1, 3])),
    ("3x3 s1 unknown input", "conv_q4", (64, 64, 3, 3), None, S1, False, ((2, "@q4g1"), None)),
    ("depthwise", "conv_q4", (32, 1, 3, 3), (32, 32, 112, 112), dict(S1, group=32), False, ((13, "@dwq4"), None)),
    ("Cin<4 stem", "conv_q4", (64, 3, 7, 7), (32, 3, 224, 224), {"strides": [2, 2], "pads": [3, 3, 3, 3]}, True,
     ((6, "@rowpack"), None)),
    ("Cin<4 not fed NCHW", "conv_q4", (64, 3, 7, 7), (32, 3, 224, 224), {"strides": [2, 2], "pads": [3, 3, 3, 3]}, False,
     ((2, "@q4g1"), None)),
    ("1x1", "conv_q4", (128, 64, 1, 1), (32, 64, 56, 56), {"strides": [1, 1]}, False, ((2, "@q4g1"), None)),
    ("1x1 NCHW", "conv", (128, 64, 1, 1), (32, 64, 56, 56), {}, False, ((1, "@tap"), None)),
    ("NCHW Cin % 16", "conv_fused", (64, 8, 3, 3), (32, 8, 56, 56), S1, False, (None, None)),
    ("grouped", "conv_q4", (64, 16, 3, 3), (32, 64, 56, 56), dict(S1, group=4), False, ((2, "@q4g4"), None)),
    ("transposed k2 s2", "convt_fused", (128, 64, 2, 2), (8, 128, 32, 32), {"strides": [2, 2]}, False, ((14, "@convt2x2"), None)),
    ("transposed k3 s2 p1 op1", "convtranspose", (128, 64, 3, 3), (8, 128, 32, 32),
     {"strides": [2, 2], "pads": [1, 1, 1, 1], "output_padding": [1, 1]}, False, ((14, "@convt2x2"), None)),
    ("transposed dilated", "convt_q4", (128, 64, 3, 3), (8, 128, 32, 32), {"strides": [2, 2], "dilations": [2, 2]}, False,
     (None, None)),
])
def test_choice_and_candidate_order(case, kind, k_shape, x_shape, para, rowpack, expect):
    assert _choose(kind, k_shape, x_shape, rowpack, **para) == expect, case


def test_switches_take_candidates_out_and_winograd_0_times_nothing(monkeypatch):
    monkeypatch.setenv("PLANER_HIP_WF4", "0")
    monkeypatch.setenv("PLANER_HIP_WINOGRAD43", "0")
    assert _choose("conv_q4", (256, 256, 3, 3), (32, 256, 14, 14), **S1) == ((7, "@wino4q4"), [2, 8, 4, 7])
    monkeypatch.setenv("PLANER_HIP_WINOGRAD", "0")
    assert _choose("conv_q4", (256, 256, 3, 3), (32, 256, 14, 14), **S1) == ((2, "@q4g1"), None)
    assert _choose("conv_fused", (64, 64, 3, 3), (32, 64, 56, 56), **S1) == ((1, "@tap"), None)


def _decisions(mod, batch, size, q4=True, **kw):
    """What plan.lower decides for every conv of a generator net at this batch, with the picker taking the first
    and the last candidate: Counter of (kind, w_layout, suffix, candidates) per pick."""
    g, b = mod.build(**kw)
    inits = [i[0] for i in g["inits"]]
    shapes = {k: ((batch,) + tuple(s[1:]) if k not in inits and s is not None and len(s) and s[0] == 1 else s)
              for k, s in shapes_of(g, b, mod.make_input(1, size=size)).items()}
    body, flow, _ = compile_front(g["layers"], g["flow"], inits, shapes, q4=q4, stop="assign_layouts")
    kinds = {e[0]: e for e in body}
    out = []
    for first in (True, False):
        seen = collections.Counter()
        for src, names, _ in flow:
            _, kind, para = kinds[names[0]]
            srcs = src if isinstance(src, list) else [src]
            if len(srcs) < 2 or srcs[1] not in inits:
                continue
            xs = shapes.get(srcs[0].split("@")[0] if kind == "conv_q4" else srcs[0])
            cands = []
            got = cl.choose(kind, shapes[srcs[1]], para, xs, para.get("rowpack"),
                            lambda c: cands.extend(c) or (c[0] if first else c[-1]))
            if got is not None:
                seen[(kind, got[0], got[1], tuple(cands))] += 1
        out.append(dict(seen))
    return out


# (the same decisions as before the table: a dump of every fused step's w_layout, filter key and candidates, made with the
# decision code this table replaced, matched byte for byte)
D, ROWPACK = ("conv_q4", 2, "@q4g1", ()), ("conv_q4", 6, "@rowpack", ())
T, T43 = (2, 8, 4, 7, 9), (2, 8, 4, 7, 9, 11)
UNET = [{D: 1, ("conv_q4", 2, "@q4g1", T): 17, ROWPACK: 1, ("convt_q4", 14, "@convt2x2", ()): 4},
        {D: 1, ("conv_q4", 9, "@wf4q4", T): 17, ROWPACK: 1, ("convt_q4", 14, "@convt2x2", ()): 4}]
NETS = {
    "resnet18 b32@224": (resnet18, 32, 224, {}, True, [
        {D: 6, ("conv_q4", 2, "@q4g1", T): 10, ("conv_q4", 2, "@q4g1", T43): 3, ROWPACK: 1},
        {D: 6, ("conv_q4", 9, "@wf4q4", T): 10, ("conv_q4", 11, "@wino43q4", T43): 3, ROWPACK: 1}]),
    "yolov3 b1@416": (yolov3, 1, 416, {}, True, [
        {D: 42, ("conv_q4", 2, "@q4g1", T): 32, ROWPACK: 1},
        {D: 42, ("conv_q4", 9, "@wf4q4", T): 32, ROWPACK: 1}]),
    "mobilenetv2 b32@224": (mobilenetv2, 32, 224, {}, True, [{D: 34, ROWPACK: 1, ("conv_q4", 13, "@dwq4", ()): 17}] * 2),
    "unet-k2 b8@256": (unet, 8, 256, {"up": "k2"}, True, UNET),
    "unet-k3 b8@256": (unet, 8, 256, {"up": "k3"}, True, UNET),
    "customnet b1@64": (customnet, 1, 64, {}, True, [{}, {}]),
    "resnet18 NCHW b32@224": (resnet18, 32, 224, {}, False, [
        {("conv_fused", 1, "@tap", ()): 6, ("conv_fused", 1, "@tap", (1, 3)): 13},
        {("conv_fused", 1, "@tap", ()): 6, ("conv_fused", 3, "@wino", (1, 3)): 13}]),
}


@pytest.mark.parametrize("name", sorted(NETS))
def test_decisions_for_the_generator_nets(name):
    mod, batch, size, kw, q4, expect = NETS[name]
    assert _decisions(mod, batch, size, q4, **kw) == expect

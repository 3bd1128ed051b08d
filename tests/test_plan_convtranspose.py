"""Transposed convs by output phase, checked on the CPU: the phase decomposition the kernel computes (a float64 emulation
against the oracle's zero-stuffed form), the U-Net generator, and what the plan compiler does with transposed convs --
fused tails, channel-quad layouts, the convs it must leave alone, and the meaning of the rewritten flow (numpy stand-ins)."""
import itertools
from collections import Counter

import numpy as np
import pytest

from oracle import planer_np as onp
from planer_amd.irgen import unet
from planer_amd.layer import convt_out_hw, convt_phase_eligible
from planer_amd.plan import ACT_RELU, assign_layouts, fuse_flow
from tests.conftest import assert_close
from tests.plan_audit import cpu_front, run_on_oracle
from tests.test_plan_fusion import conv_fused_np


def phase_convt(x, K, B=None, strides=(2, 2), pads=(0, 0, 0, 0), output_padding=(0, 0)):
    """float64 emulation of pl_conv2d_convt_q4_f32: every output phase (rh, rw) is a stride-1 conv of x with the
    ceil(kh/sh) x ceil(kw/sw) sub-filter K[.., rh + sh*(th-1-a), rw + sw*(tw-1-b)] (zero beyond the filter) and pad
    th-1-pt//sh, written to output pixel (sh*(i + pt//sh) + rh - pt, ...) where that lies inside the output."""
    x, K = x.astype(np.float64), K.astype(np.float64)
    n, cin, h, w = x.shape
    _, cout, kh, kw = K.shape
    (sh, sw), (pt, pl) = strides, pads[:2]
    ho, wo = convt_out_hw(h, w, kh, kw, strides, pads, output_padding)
    th, tw = -(-kh // sh), -(-kw // sw)
    hq, wq = (ho - 1 + pt) // sh - pt // sh + 1, (wo - 1 + pl) // sw - pl // sw + 1
    y = np.zeros((n, cout, ho, wo))
    for rh, rw in itertools.product(range(sh), range(sw)):
        acc = np.zeros((n, cout, hq, wq))
        for a, b in itertools.product(range(th), range(tw)):
            ky, kx = rh + sh * (th - 1 - a), rw + sw * (tw - 1 - b)
            if ky >= kh or kx >= kw:
                continue
            rows = np.arange(hq) - (th - 1 - pt // sh) + a
            cols = np.arange(wq) - (tw - 1 - pl // sw) + b
            rin, cin_ = (rows >= 0) & (rows < h), (cols >= 0) & (cols < w)
            xs = np.zeros((n, cin, hq, wq))
            xs[:, :, np.ix_(rin, cin_)[0], np.ix_(rin, cin_)[1]] = x[:, :, rows[rin]][:, :, :, cols[cin_]]
            acc += np.einsum("nchw,cd->ndhw", xs, K[:, :, ky, kx])
        oh = sh * (np.arange(hq) + pt // sh) + rh - pt
        ow = sw * (np.arange(wq) + pl // sw) + rw - pl
        mh, mw = (oh >= 0) & (oh < ho), (ow >= 0) & (ow < wo)
        y[:, :, oh[mh][:, None], ow[mw][None, :]] = acc[:, :, mh][:, :, :, mw]
    if B is not None:
        y += B.astype(np.float64).reshape(1, -1, 1, 1)
    return y


def _geometries():
    """k 1-5 (kh != kw), s 1-3 (sh != sw), pads up to the kernel reach (asymmetric), output_padding in [0, s), k < s."""
    out = []
    for kh, kw in [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (1, 3), (2, 5), (3, 1), (4, 2)]:
        for sh, sw in [(1, 1), (2, 2), (3, 3), (1, 2), (2, 3), (3, 1)]:
            for pt, pl, pb, pr in {(0, 0, 0, 0), (kh - 1, kw - 1, kh - 1, kw - 1), ((kh - 1) // 2, kw // 2, kh // 2, (kw - 1) // 2),
                                   (kh - 1, 0, 0, kw - 1)}:
                for oph, opw in {(0, 0), (sh - 1, sw - 1), (0, sw - 1)}:
                    out.append(((kh, kw), (sh, sw), (pt, pl, pb, pr), (oph, opw)))
    return out


GEOMS = _geometries()


def test_phase_decomposition_is_bit_exact_against_the_zero_stuffed_oracle():
    rng = np.random.default_rng(0)
    checked = 0
    for i, ((kh, kw), s, pads, op) in enumerate(GEOMS):
        h, w = [(1, 1), (1, 4), (3, 1), (4, 5), (6, 3)][i % 5]
        ho, wo = convt_out_hw(h, w, kh, kw, s, pads, op)
        if ho <= 0 or wo <= 0:
            continue
        x = rng.integers(-3, 4, (2, 3, h, w)).astype(np.float32)
        K = rng.integers(-3, 4, (3, 5, kh, kw)).astype(np.float32)
        B = rng.integers(-3, 4, 5).astype(np.float32)
        want = onp.convtranspose2d(x.astype(np.float64), K.astype(np.float64), B.astype(np.float64), strides=list(s),
                                   dilations=[1, 1], pads=list(pads), output_padding=list(op))
        got = phase_convt(x, K, B, s, pads, op)
        assert got.shape == want.shape == (2, 5, ho, wo), ((kh, kw), s, pads, op)
        assert np.array_equal(got, want), ((kh, kw), s, pads, op)
        assert convt_phase_eligible((3, 5, kh, kw), 1, s, (1, 1), pads, op)
        checked += 1
    assert checked > 300
    # k < s: phases without a single tap are the bias alone
    y = phase_convt(np.ones((1, 1, 2, 2), np.float32), np.ones((1, 1, 1, 1), np.float32), np.array([7.0], np.float32), (2, 2))
    assert y.shape == (1, 1, 3, 3) and y[0, 0, 1, 1] == 7.0 and y[0, 0, 0, 0] == 8.0


def test_eligibility_keeps_todays_refusals_and_the_stuffed_path():
    assert not convt_phase_eligible((4, 4, 3, 3), group=2)
    assert not convt_phase_eligible((4, 4, 3, 3), strides=(2, 2), dilations=(2, 2))
    assert not convt_phase_eligible((4, 4, 3, 3), strides=(1, 1), dilations=(2, 1))
    assert not convt_phase_eligible((4, 4, 3, 3), pads=(3, 0, 0, 0))            # beyond the kernel reach
    assert not convt_phase_eligible((4, 4, 3, 3), pads=(0, 0, 3, 0))
    assert convt_phase_eligible((4, 4, 3, 3), pads=(0, 0, 3, 0), output_padding=(1, 0))
    assert convt_phase_eligible((4, 4, 2, 2))                                     # the U-Net up-step, default strides 2


@pytest.mark.parametrize("up", ["k2", "k3"])
def test_generator_parameters_and_op_census(up):
    g, b = unet.build(up=up)
    n = sum(int(np.prod(s)) for _, s, _ in g["inits"])
    assert n == unet.params(up=up) and b.size == 4 * n
    if up == "k2":
        assert n == unet.PARAMS == 31037698
    kinds = Counter(k for _, k, _ in g["layers"])
    bn = 18 + (4 if up == "k3" else 0)
    assert kinds == Counter({"conv": 19, "batchnorm": bn, "relu": bn, "maxpool": 4, "convtranspose": 4, "concat": 4,
                             "return": 1})
    shapes = {k: s for k, s, _ in g["inits"]}
    ups = [(p, shapes[f[0][1]], len(f[0])) for (_, k, p), f in zip(g["layers"], g["flow"]) if k == "convtranspose"]
    assert [s[:2] for _, s, _ in ups] == [[1024, 512], [512, 256], [256, 128], [128, 64]]
    if up == "k2":
        assert all(s[2:] == [2, 2] and p["strides"] == [2, 2] and p["pads"] == [0] * 4 and nsrc == 3 for p, s, nsrc in ups)
    else:
        assert all(s[2:] == [3, 3] and p["pads"] == [1] * 4 and p["output_padding"] == [1, 1] and nsrc == 2 for p, s, nsrc in ups)
    assert unet.make_input(2, size=32).shape == (2, 3, 32, 32)


def _program(up, size):
    g, b = unet.build(up=up)
    x = unet.make_input(1, size=size)
    body, flow, counts, _ = cpu_front(g, b, x, stop="fuse_flow")
    fused = (body, flow, counts["fuse_flow"])
    body, flow, counts, _ = cpu_front(g, b, x, stop="assign_layouts")
    kinds = {b_[0]: b_[1] for b_ in body}
    paras = {b_[0]: b_[2] for b_ in body}
    return g, b, x, fused, [(kinds[f[1][0]], f[0], f[2], paras[f[1][0]]) for f in flow], counts["assign_layouts"]


@pytest.mark.parametrize("up", ["k2", "k3"])
def test_layouts_unet_up_convs_are_q4_and_no_conversion_but_the_result(up):
    _, _, _, _, steps, nq4 = _program(up, 64)
    kinds = [k for k, _, _, _ in steps]
    assert nq4 > 0
    assert kinds.count("convt_q4") == 4 and "convtranspose" not in kinds and "convt_fused" not in kinds
    assert kinds.count("conv_q4") == 19 and "conv" not in kinds and "conv_fused" not in kinds
    assert kinds.count("concat_q4") == 4 and "concat" not in kinds
    assert kinds.count("maxpool_q4") == 4
    # the stem reads the NCHW input itself (row-packed); only the returned class map goes back to NCHW
    assert "to_q4" not in kinds and kinds.count("from_q4") == 1 and kinds[-2:] == ["from_q4", "return"]
    assert [s for _, srcs, _, _ in steps for s in srcs if s.endswith("@nchw")] == ["logits@nchw"]
    if up == "k3":
        ups = [p for k, _, _, p in steps if k == "convt_q4"]
        assert all(p["act"] == ACT_RELU and p["output_padding"] == [1, 1] for p in ups)


def test_fusion_folds_bn_relu_into_each_k3_up_conv():
    g, _, _, (body, flow, nf), _, _ = _program("k3", 32)
    convt = [b_ for b_ in body if b_[1] == "convt_fused"]
    assert len(convt) == 4 and all(b_[2]["act"] == ACT_RELU for b_ in convt)
    steps = {f[1][0]: f[0] for f in flow}
    assert all(steps[b_[0]][3].endswith("_invK") and steps[b_[0]][4].endswith("_invB") for b_ in convt)
    assert nf == 2 * 22                     # every batchnorm and relu, the 4 up-steps' included
    # k2: the up-conv's only reader is the concat -- nothing to fold, the step keeps its kind
    g, _, _, (body, _, nf), _, _ = _program("k2", 32)
    assert Counter(b_[1] for b_ in body)["convtranspose"] == 4 and nf == 2 * 18


def test_fusion_leaves_an_intermediate_with_a_second_reader():
    layers = [["t", "convtranspose", {"strides": [2, 2], "pads": [1, 1, 1, 1], "output_padding": [1, 1]}],
              ["bn", "batchnorm", {}], ["r", "relu", {}], ["f", "flatten", {}], ["return", "return", {}]]
    flow = [[["x", "K"], ["t"], "a"], [["a", "s", "h"], ["bn"], "b"], [["b"], ["r"], "c"], [["b"], ["f"], "d"],
            [["c", "d"], ["return"], "plrst"]]
    shp = {"x": (1, 4, 5, 5), "K": (4, 8, 3, 3), "s": (1, 8, 1, 1), "h": (1, 8, 1, 1), "a": (1, 8, 10, 10),
           "b": (1, 8, 10, 10), "c": (1, 8, 10, 10), "d": (1, 800)}
    body, out, nf = fuse_flow(layers, flow, ["K", "s", "h"], shp)
    # bn folds (a has one reader); relu does not: b is also read by flatten
    assert nf == 1
    fused = [b_ for b_ in body if b_[1] == "convt_fused"]
    assert len(fused) == 1 and fused[0][2]["act"] == 0 and "relu" in [b_[1] for b_ in body]
    # a second reader of the transposed conv's own output: nothing folds
    flow2 = [[["x", "K"], ["t"], "a"], [["a", "s", "h"], ["bn"], "b"], [["b"], ["r"], "c"], [["a"], ["f"], "d"],
             [["c", "d"], ["return"], "plrst"]]
    body, _, nf = fuse_flow(layers, flow2, ["K", "s", "h"], shp)
    assert nf == 0 and "convt_fused" not in [b_[1] for b_ in body]


@pytest.mark.parametrize("para, kshape, const", [
    ({"group": 2, "strides": [2, 2]}, (8, 4, 3, 3), True),
    ({"strides": [2, 2], "dilations": [2, 2]}, (8, 8, 3, 3), True),
    ({"strides": [2, 2]}, (8, 8, 2, 2), False),
])
def test_ineligible_transposed_convs_stay_nchw_with_todays_kind(para, kshape, const):
    layers = [["c", "conv", {"pads": [1, 1, 1, 1]}], ["t", "convtranspose", para], ["bn", "batchnorm", {}], ["r", "relu", {}],
              ["return", "return", {}]]
    flow = [[["x", "K0"], ["c"], "a"], [["a", "K"], ["t"], "b"], [["b", "s", "h"], ["bn"], "d"], [["d"], ["r"], "e"],
            [["e"], ["return"], "plrst"]]
    shp = {"x": (1, 8, 6, 6), "K0": (8, 8, 3, 3), "a": (1, 8, 6, 6), "K": kshape, "b": (1, 8, 12, 12),
           "s": (1, 8, 1, 1), "h": (1, 8, 1, 1), "d": (1, 8, 12, 12), "e": (1, 8, 12, 12)}
    inits = ["K0", "s", "h"] + (["K"] if const else [])
    body, out, _ = fuse_flow(layers, flow, inits, shp)
    body, out, _ = assign_layouts(body, out, inits, shp, force=True)
    kinds = {b_[0]: b_[1] for b_ in body}
    seq = [kinds[f[1][0]] for f in out]
    assert "convtranspose" in seq and "convt_q4" not in seq and "convt_fused" not in seq
    i = seq.index("convtranspose")
    assert seq[i - 1] == "from_q4" and out[i][0][0].endswith("@nchw")


def convt_fused_np(x, K, B=None, scale=None, shift=None, res=None, act=0, alpha=0.0, w_layout=0, **para):
    y = onp.convtranspose2d(x, K, B, **para)
    return conv_fused_np(y, np.ones((y.shape[1], y.shape[1], 1, 1), y.dtype) * np.eye(y.shape[1], dtype=y.dtype)[:, :, None, None],
                         None, scale, shift, res, act, alpha) if any(v is not None for v in (scale, shift, res)) or act else y


@pytest.mark.parametrize("up", ["k2", "k3"])
def test_unet_fused_and_layout_assigned_flow_matches_the_oracle(up):
    g, b = unet.build(up=up)
    x = unet.make_input(1, size=32)
    body, flow, counts, _ = cpu_front(g, b, x, stop="assign_layouts")
    assert counts["assign_layouts"] > 0 and any(b_[1] == "convt_q4" for b_ in body)

    ref = onp.OracleNet()
    ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
    ref.load_weights(b)
    want = ref(x.copy())

    got = run_on_oracle(g, b, x, body, flow, convt_q4=convt_fused_np, convt_fused=convt_fused_np)
    assert got.shape == want.shape == (1, 2, 32, 32)
    assert_close(np.ascontiguousarray(got), np.ascontiguousarray(want), 1e-5)

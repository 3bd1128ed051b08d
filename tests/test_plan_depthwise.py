"""Depthwise convs and ReLU6 (clip) in channel-quad plans, checked on the CPU: MobileNet-v2's layout assignment, the in-place
clip's converted copies, and the meaning of the rewritten flow (numpy stand-ins for the Q4 kernels)."""
from collections import Counter

import numpy as np

from oracle import planer_np as onp
from planer_amd.irgen import mobilenetv2
from planer_amd.plan import assign_layouts
from tests.conftest import assert_close
from tests.plan_audit import cpu_front, run_on_oracle
from tests.test_plan_fusion import _layout_program, _q4_standins


def test_generator_parameters_and_op_census():
    g, b = mobilenetv2.build()
    assert sum(int(np.prod(s)) for _, s, _ in g["inits"]) == mobilenetv2.PARAMS == 3504872
    assert b.size == 4 * mobilenetv2.PARAMS
    kinds = Counter(k for _, k, _ in g["layers"])
    assert kinds == Counter({"conv": 52, "batchnorm": 52, "clip": 35, "add": 10, "gap": 1, "flatten": 1, "dense": 1,
                             "return": 1})
    shapes = {n: s for n, s, _ in g["inits"]}
    dw = [(p, shapes[f[0][1]]) for (_, k, p), f in zip(g["layers"], g["flow"]) if k == "conv" and p["group"] > 1]
    assert len(dw) == 17
    assert all(s[1] == 1 and s[0] == p["group"] and s[2:] == [3, 3] for p, s in dw)
    assert all(p == {"min": 0.0, "max": 6.0} for _, k, p in g["layers"] if k == "clip")
    assert mobilenetv2.make_input(2, size=32).shape == (2, 3, 32, 32)


def test_layouts_mobilenetv2_all_q4_no_conversion():
    steps, _ = _layout_program(mobilenetv2, mobilenetv2.make_input(1, size=64))
    kinds = [k for k, _, _, _ in steps]
    # the 3-channel stem reads the NCHW input itself (row-packed); gap hands NCHW to flatten / dense
    assert "to_q4" not in kinds and "from_q4" not in kinds
    assert kinds[0] == "conv_q4" and steps[0][3].get("rowpack") and steps[0][1][0] == "x"
    assert kinds.count("conv_q4") == 52 and "conv" not in kinds and "conv_fused" not in kinds
    assert kinds.count("clip_q4") == 35 and "clip" not in kinds
    assert sum(1 for k, _, _, p in steps if k == "conv_q4" and int(p.get("group", 1)) > 1) == 17
    assert "gap_q4" in kinds and kinds[-3:] == ["flatten", "dense", "return"]
    assert all(not s.endswith("@nchw") and not s.endswith("@q4") for _, srcs, _, _ in steps for s in srcs)


def test_layouts_inplace_clip_invalidates_converted_copies():
    layers = [["c", "conv", {}], ["f", "flatten", {}], ["r", "clip", {"min": 0.0, "max": 6.0}], ["g", "flatten", {}],
              ["return", "return", {}]]
    flow = [[["x", "K"], ["c"], "t"], [["t"], ["f"], "a"], [["t"], ["r"], "u"], [["t"], ["g"], "b"],
            [["a", "b"], ["return"], "plrst"]]
    shp = {"x": (1, 4, 5, 5), "K": (8, 4, 3, 3), "t": (1, 8, 3, 3), "u": (1, 8, 3, 3)}
    body, out, _ = assign_layouts(layers, flow, ["K"], shp, force=True)
    kinds = {b_[0]: b_[1] for b_ in body}
    seq = [kinds[f[1][0]] for f in out]
    # t is converted for the first flatten, mutated in place by clip_q4, and converted AGAIN for the second
    assert seq == ["to_q4", "conv_q4", "from_q4", "flatten", "clip_q4", "from_q4", "flatten", "return"]


def test_layouts_clip_that_would_dirty_padding_stays_nchw_and_refreshes_the_q4_value():
    # 6 channels (a partial quad) clipped to [1, 2]: clip(0) = 1 would dirty the padding lanes, so the clip runs on an NCHW
    # copy; the conv that reads t afterwards must see the clipped values (layer.py:250-251 mutates t)
    layers = [["c", "conv", {}], ["r", "clip", {"min": 1.0, "max": 2.0}], ["d", "conv", {}], ["return", "return", {}]]
    flow = [[["x", "K"], ["c"], "t"], [["t"], ["r"], "u"], [["t", "K2"], ["d"], "v"], [["u", "v"], ["return"], "plrst"]]
    shp = {"x": (1, 4, 7, 7), "K": (6, 4, 3, 3), "t": (1, 6, 5, 5), "u": (1, 6, 5, 5), "K2": (4, 6, 3, 3), "v": (1, 4, 3, 3)}
    body, out, _ = assign_layouts(layers, flow, ["K", "K2"], shp, force=True)
    kinds = {b_[0]: b_[1] for b_ in body}
    seq = [kinds[f[1][0]] for f in out]
    assert "clip_q4" not in seq and "clip" in seq
    i = seq.index("clip")
    assert seq[i + 1] == "to_q4" and out[i + 1][2] == "t"
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 4, 7, 7)).astype(np.float32)
    K = rng.standard_normal((6, 4, 3, 3)).astype(np.float32)
    K2 = rng.standard_normal((4, 6, 3, 3)).astype(np.float32)
    want = _run_flow(layers, flow, {"x": x, "K": K, "K2": K2})
    got = _run_flow(body, out, {"x": x, "K": K, "K2": K2})
    for o, w in zip(got, want):
        assert_close(np.ascontiguousarray(o), np.ascontiguousarray(w), 1e-5)


def _run_flow(layers, flow, env):
    """A minimal interpreter of a one-layer-per-step flow with the oracle's ops and the Q4 stand-ins."""
    ops = dict(onp.OPS)
    ops.update(_q4_standins())
    ops["clip_q4"] = onp.OPS["clip"]
    kinds = {b[0]: (b[1], b[2]) for b in layers}
    env = dict({k: v.copy() for k, v in env.items()}, **{"None": None})
    out = None
    for src, names, dst in flow:
        kind, para = kinds[names[0]]
        args = [env[k] for k in src]
        while len(args) > 1 and args[-1] is None:
            args.pop()
        if kind == "return":
            out = tuple(args)
            break
        env[dst] = ops[kind](*args, **{k: v for k, v in para.items() if k not in ("rowpack", "w_layout")})
    return out


def test_mobilenetv2_fused_and_layout_assigned_flow_matches_the_oracle():
    g, b = mobilenetv2.build()
    x = mobilenetv2.make_input(1, size=64)
    body, flow, counts, _ = cpu_front(g, b, x, stop="assign_layouts")
    assert counts["fuse_flow"] == 52 + 10      # every batchnorm and every residual add folds into its conv
    assert counts["assign_layouts"] > 0

    ref = onp.OracleNet()
    ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
    ref.load_weights(b)
    want = ref(x.copy())

    got = run_on_oracle(g, b, x, body, flow, clip_q4=onp.OPS["clip"])
    assert got.shape == want.shape == (1, 1000)
    assert_close(np.ascontiguousarray(got), np.ascontiguousarray(want), 1e-5)

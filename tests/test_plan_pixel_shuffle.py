"""Plan compiler: pixel shuffle / unshuffle written as reshape -> transpose -> reshape (plan.fuse_pixel_shuffle), its place in
channel-quad (Q4) plans (plan.assign_layouts) and the EDSR net that needs it (planer_amd.irgen.edsr).  Host logic only; numpy's
own reshape / transpose / reshape is the reference and every comparison is in bits."""
import numpy as np
import pytest

from planer_amd.irgen import edsr
from planer_amd.irgen.builder import save_model
from planer_amd.plan import fuse_pixel_shuffle, match_pixel_shuffle
from tests.linear_q4_ref import Small, assert_same_bits
from tests.pixel_shuffle_ref import (AXES, FORM_IDS, FORMS, compile_plan, cpu_front, kinds_of, make_x, mid_shape, out_shape, run_on_oracle,
                                     sandwich, shuffle_np, steps_of, trio)


def _original(g, b, x):
    return run_on_oracle(g, b, x, g["layers"], g["flow"])


@pytest.mark.parametrize("via_const", [False, True], ids=["shape-init", "shape-const-step"])
@pytest.mark.parametrize("r", [2, 3, 4])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_each_form_between_convs_is_one_channel_quad_step(form, r, via_const):
    order, inverse = form
    hw = (2 * r, 3 * r)
    g, b = sandwich(order, inverse, r=r, hw=hw, via_const=via_const)
    x = make_x(hw=hw)
    body, flow, nps, _ = compile_plan(g, b, x)
    steps = steps_of(body, flow)
    names = [s[0] for s in steps if s[0] != "const"]
    assert nps == 1
    assert names == ["to_q4", "conv_q4", "pixelshuffle_q4", "conv_q4", "from_q4", "return"], names
    ps = [s for s in steps if s[0] == "pixelshuffle_q4"][0]
    assert ps[1] == {"r": r, "order": order, "inverse": inverse} and ps[2] == ["a"] and ps[3] == "ps"
    # the steps that only fed the reshapes' shape operands stay where they are
    assert [s[0] for s in steps].count("const") == (2 if via_const else 0)
    assert_same_bits(run_on_oracle(g, b, x, body, flow), _original(g, b, x), "rewritten program against the original")


def test_the_stand_in_is_the_trio_and_crd_is_torch_pixel_shuffle():
    """shuffle_np against the definition, element by element: CRD wide channel c r^2 + i r + j, DCR (i r + j) C + c."""
    r, c, h, w = 3, 2, 2, 3
    x = np.arange(2 * c * r * r * h * w, dtype=np.float32).reshape(2, c * r * r, h, w)
    for order in ("crd", "dcr"):
        y = shuffle_np(x, r, order, False)
        assert y.shape == (2, c, h * r, w * r)
        for cc in range(c):
            for i in range(r):
                for j in range(r):
                    wide = cc * r * r + i * r + j if order == "crd" else (i * r + j) * c + cc
                    np.testing.assert_array_equal(y[:, cc, i::r, j::r], x[:, wide])
        np.testing.assert_array_equal(shuffle_np(y, r, order, True), x)


def _unchanged(g, b, x):
    body, flow, _, shapes = cpu_front(g, b, x, stop="fuse_flow")
    body2, flow2, n = fuse_pixel_shuffle(body, flow, shapes)
    assert n == 0
    assert [list(e) for e in body2] == [list(e) for e in body]
    assert [[list(s) if isinstance(s, (list, tuple)) else [s], list(nm), d] for s, nm, d in flow2] == \
           [[list(s) if isinstance(s, (list, tuple)) else [s], list(nm), d] for s, nm, d in flow]
    names = kinds_of(*compile_plan(g, b, x)[:2])
    assert "pixelshuffle" not in names and "pixelshuffle_q4" not in names and "transpose" in names


def test_a_permutation_off_by_one_swap_is_left_alone():
    for form in FORMS:
        ax = list(AXES[form])
        ax[4], ax[5] = ax[5], ax[4]
        hw = (6, 6)
        # (the last reshape's target is the swapped tensor's element count in 4-D: square maps and factors keep the shape legal)
        g, b = sandwich(form[0], form[1], hw=hw, axis=ax)
        _unchanged(g, b, make_x(hw=hw))


def test_rectangular_factors_are_left_alone():
    """(2, 3): a legal depth-to-space by unequal factors, but not a pixel shuffle by r."""
    s = Small()
    y = s.conv("x", "a", cin=4, cout=24)
    s.g.init("s6", np.array([0, 4, 2, 3, 6, 8], np.int64))
    s.g.init("s4", np.array([0, 4, 12, 24], np.int64))
    y = s.g.op("reshape", [y, "s6"], "m", name="split")
    y = s.g.op("transpose", y, "t", name="perm", axis=[0, 1, 4, 2, 5, 3])
    y = s.g.op("reshape", [y, "s4"], "ps", name="merge")
    g, b = s.finish(s.conv(y, "z", cin=4))
    _unchanged(g, b, make_x())


def test_r_5_is_left_alone():
    g, b = sandwich("crd", False, r=5, narrow=1, hw=(2, 3))
    _unchanged(g, b, make_x(hw=(2, 3)))
    g, b = sandwich("crd", True, r=5, narrow=4, hw=(5, 10))
    _unchanged(g, b, make_x(hw=(5, 10)))


@pytest.mark.parametrize("which", ["6-D tensor", "transposed tensor"])
def test_a_middle_tensor_with_a_second_reader_is_left_alone(which):
    s = Small()
    y = s.conv("x", "a", cin=4, cout=16)
    y = trio(s, y, (1, 16, 6, 8), 2, "crd", False)
    s.g.op("leakyrelu", "ps_6" if which == "6-D tensor" else "ps_t", "side", name="second_reader", alpha=0.1)
    g, b = s.finish(s.conv(y, "z", cin=4))
    _unchanged(g, b, make_x())


def test_a_first_reshape_whose_input_is_not_4d_is_left_alone():
    """A 5-D tensor reshaped to the 6-D form: the same transpose, but no NCHW activation in front of it."""
    s = Small()
    y = s.conv("x", "a", cin=4, cout=16)
    s.g.init("s5", np.array([0, 4, 4, 6, 8], np.int64))
    y = s.g.op("reshape", [y, "s5"], "five", name="to5")
    y = trio(s, y, (1, 16, 6, 8), 2, "crd", False)
    g, b = s.finish(s.conv(y, "z", cin=4))
    _unchanged(g, b, make_x())


def test_match_pixel_shuffle_wants_every_shape_to_agree():
    ok = dict(s_in=(2, 16, 3, 5), s_mid=(2, 4, 2, 2, 3, 5), axis=[0, 1, 4, 2, 5, 3], s_out=(2, 4, 6, 10))
    assert match_pixel_shuffle(**ok) == {"r": 2, "order": "crd", "inverse": False}
    assert match_pixel_shuffle(**dict(ok, s_out=(2, 4, 10, 6))) is None
    assert match_pixel_shuffle(**dict(ok, s_out=(2, 4, 60))) is None
    assert match_pixel_shuffle(**dict(ok, s_mid=(2, 2, 2, 4, 3, 5))) is None            # the DCR split under the CRD permutation
    assert match_pixel_shuffle(**dict(ok, s_in=(2, 16, 15))) is None
    assert match_pixel_shuffle(**dict(ok, s_mid=None)) is None
    assert match_pixel_shuffle((2, 4, 6, 10), (2, 4, 3, 2, 5, 2), [0, 1, 3, 5, 2, 4], (2, 16, 3, 5)) == {"r": 2, "order": "crd", "inverse": True}
    assert match_pixel_shuffle((2, 4, 6, 9), (2, 4, 3, 2, 3, 3), [0, 1, 3, 5, 2, 4], (2, 24, 3, 3)) is None    # (2, 3)


@pytest.mark.parametrize("inverse", [False, True], ids=["shuffle", "unshuffle"])
def test_dcr_with_six_channels_is_named_but_stays_nchw(inverse):
    g, b = sandwich("dcr", inverse, narrow=6)
    x = make_x()
    body, flow, nps, _ = compile_plan(g, b, x)
    names = kinds_of(body, flow)
    assert nps == 1 and names == ["to_q4", "conv_q4", "from_q4", "pixelshuffle", "to_q4", "conv_q4", "from_q4", "return"], names
    assert_same_bits(run_on_oracle(g, b, x, body, flow), _original(g, b, x))
    # CRD takes the same channel count
    g, b = sandwich("crd", inverse, narrow=6)
    assert "pixelshuffle_q4" in kinds_of(*compile_plan(g, b, x)[:2])


@pytest.mark.parametrize("with_return", [True, False], ids=["return-layer", "last-step"])
def test_a_trailing_shuffle_writes_nchw_itself_and_a_trailing_unshuffle_is_converted(with_return):
    def compiled(inverse):
        g, b = sandwich("crd", inverse, narrow=3 if not inverse else 4, tail=False)
        if not with_return:
            g["layers"], g["flow"] = g["layers"][:-1], g["flow"][:-1]
        x = make_x()
        body, flow, nps, _ = compile_plan(g, b, x)
        assert nps == 1
        assert_same_bits(run_on_oracle(g, b, x, body, flow), _original(g, b, x))
        return steps_of(body, flow)
    end = ["return"] if with_return else []
    steps = compiled(False)
    assert [s[0] for s in steps] == ["to_q4", "conv_q4", "pixelshuffle_q4"] + end
    assert steps[2][1] == {"r": 2, "order": "crd", "inverse": False, "nchw_out": True} and steps[2][3] == "ps"
    steps = compiled(True)
    assert [s[0] for s in steps] == ["to_q4", "conv_q4", "pixelshuffle_q4", "from_q4"] + end
    assert "nchw_out" not in steps[2][1]


def test_a_shuffle_whose_result_is_read_again_before_the_return_keeps_a_q4_result():
    s = Small()
    y = s.conv("x", "a", cin=4, cout=16)
    y = trio(s, y, (1, 16, 6, 8), 2, "crd", False)
    z = s.conv(y, "z", cin=4, cout=4)
    g, b = s.finish(s.g.op("add", [y, z], "o", name="late"))
    body, flow, _, _ = compile_plan(g, b, make_x())
    ps = [st for st in steps_of(body, flow) if st[0] == "pixelshuffle_q4"]
    assert len(ps) == 1 and "nchw_out" not in ps[0][1]


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_switch_off_gives_the_program_without_the_pass(form, monkeypatch):
    from planer_amd import plan
    g, b = sandwich(*form)
    x = make_x()
    with monkeypatch.context() as m:             # the compiler with the pass taken out
        m.setattr(plan, "fuse_pixel_shuffle", lambda body, flow, *_: (body, flow, 0))
        want = compile_plan(g, b, x)[:2]
    monkeypatch.setenv("PLANER_HIP_PIXEL_SHUFFLE_Q4", "0")
    got = compile_plan(g, b, x)
    assert got[2] == 0 and (got[0], got[1]) == want
    assert kinds_of(*want) == ["to_q4", "conv_q4", "from_q4", "reshape", "transpose", "reshape", "to_q4", "conv_q4", "from_q4", "return"]


def test_an_in_place_relu_on_the_input_between_the_steps_blocks_the_rewrite():
    """The fused step reads the first reshape's input where the LAST reshape stood."""
    layers = [["split", "reshape", {}], ["rect", "relu", {}], ["perm", "transpose", {"axis": [0, 1, 4, 2, 5, 3]}], ["merge", "reshape", {}]]
    flow = [[["a", "s6"], ["split"], "m"], ["a", ["rect"], "a2"], ["m", ["perm"], "t"], [["t", "s4"], ["merge"], "y"]]
    shapes = {"a": (1, 16, 3, 5), "m": (1, 4, 2, 2, 3, 5), "t": (1, 4, 3, 2, 5, 2), "y": (1, 4, 6, 10), "a2": (1, 16, 3, 5)}
    assert fuse_pixel_shuffle(layers, flow, shapes)[2] == 0
    pure = [[n, "leakyrelu" if k == "relu" else k, p] for n, k, p in layers]
    body, out, n = fuse_pixel_shuffle(pure, flow, shapes)
    assert n == 1 and [f[1][0] for f in out] == ["rect", "perm+"] and out[1][0] == ["a"] and out[1][2] == "y"
    assert ["perm+", "pixelshuffle", {"r": 2, "order": "crd", "inverse": False}] in body


# ---- EDSR ---------------------------------------------------------------------------------------------------------------------
TINY = dict(blocks=2, feats=8, size=12)
# name -> (options, trios, pixelshuffle_q4 steps, NCHW pixelshuffle steps, from_q4 steps, output size)
EDSR_CASES = {"x2": (dict(scale=2), 1, 1, 0, 1, 24), "x3": (dict(scale=3), 1, 1, 0, 1, 36), "x4": (dict(scale=4), 2, 2, 0, 1, 48),
              "x4-shuffle-tail": (dict(scale=4, tail="shuffle"), 1, 1, 0, 0, 48),
              "x3-shuffle-tail": (dict(scale=3, tail="shuffle"), 1, 1, 0, 0, 36),
              "x2-unshuffle-in": (dict(scale=2, unshuffle_in=True), 2, 1, 1, 1, 12)}


@pytest.mark.parametrize("name", list(EDSR_CASES))
def test_edsr_counts_shape_and_round_trip(name, tmp_path):
    opts, trios, nq4, nnchw, nfrom, size = EDSR_CASES[name]
    g, b = edsr.build(**TINY, **opts)
    x = edsr.make_input(2, size=TINY["size"])
    body, flow, nps, shapes = compile_plan(g, b, x)            # (forced: by its cost estimate a net this small stays NCHW)
    names = kinds_of(body, flow)
    assert nps == trios and names.count("pixelshuffle_q4") == nq4 and names.count("pixelshuffle") == nnchw
    assert names.count("from_q4") == nfrom and "transpose" not in names and "reshape" not in names
    # the row-packed head reads the 3-channel image itself; only the 12-channel unshuffled image is converted
    assert names.count("to_q4") == (1 if opts.get("unshuffle_in") else 0)
    want = _original(g, b, x)
    assert want.shape == (2, 3, size, size)
    assert_same_bits(run_on_oracle(g, b, x, body, flow), want, name)
    save_model(str(tmp_path / name), g, b)
    import json
    g2 = json.load(open(str(tmp_path / name) + ".json"))
    b2 = np.load(str(tmp_path / name) + ".npy")
    assert g2 == g and np.array_equal(b2, b)
    assert kinds_of(*compile_plan(g2, b2, x)[:2]) == names


def test_edsr_baseline_is_the_papers_net():
    g, b = edsr.build()
    kinds = [l[1] for l in g["layers"]]
    assert kinds.count("conv") == 1 + 32 + 1 + 2 + 1 and kinds.count("add") == 17 and kinds.count("relu") == 16
    assert kinds.count("transpose") == 2 and kinds.count("reshape") == 4 and "batchnorm" not in kinds
    w = {n: s for n, s, _ in g["inits"]}
    assert w["head_w"] == [64, 3, 3, 3] and w["up0_w"] == [256, 64, 3, 3] and w["up1_w"] == [256, 64, 3, 3] and w["tail_w"] == [3, 64, 3, 3]
    assert edsr.build(scale=3)[0]["inits"][[i[0] for i in edsr.build(scale=3)[0]["inits"]].index("up0_w")][1] == [576, 64, 3, 3]
    assert edsr.make_input(2, seed=1, size=16).shape == (2, 3, 16, 16)
    with pytest.raises(ValueError):
        edsr.build(scale=5)
    # at its real width the cost estimate keeps the net channel-quad without being forced
    g, b = edsr.build(blocks=1, size=16)
    names = kinds_of(*compile_plan(g, b, edsr.make_input(1, size=16), force=False)[:2])
    assert names.count("pixelshuffle_q4") == 2 and names.count("from_q4") == 1 and names.count("to_q4") == 0 and "transpose" not in names


def test_resnet18_compiles_to_the_same_program_with_the_switch_on_and_off(monkeypatch):
    """The benchmark's net has no such trio: the pass finds nothing and the program is the same, step for step."""
    from planer_amd.irgen import resnet18
    g, b = resnet18.build()
    x = resnet18.make_input(1, size=64)
    on = compile_plan(g, b, x, force=False)[:3]
    monkeypatch.setenv("PLANER_HIP_PIXEL_SHUFFLE_Q4", "0")
    off = compile_plan(g, b, x, force=False)[:3]
    assert on == off and on[2] == 0

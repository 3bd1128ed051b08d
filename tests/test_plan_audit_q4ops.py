"""The plan audit (tests/plan_audit.py) on the CPU for the kinds behind the conv kernels -- instance and group norm, pad, pixel
shuffle, linear upsample / resize with their fused adds, refold_q4 and every step on a pixel-phase-folded tensor: it passes on
the oracle's own float32 run of stylenet, drn (every eligible conv folded), fpn, edsr, resnet_gn and the random nets of
random_net_q4ops, no step of any of them is left out, and it fails on each kind of fault it is there to find."""
import collections

import numpy as np
import pytest

from oracle import planer_np as onp
from planer_amd.irgen import drn, edsr, fpn, resnet_gn, stylenet
from tests import fold_ref as FR
from tests import groupnorm_ref as GN
from tests import pixel_shuffle_ref as PS
from tests import plan_audit as PA
from tests import ref64_ops as RO
from tests.audit_nets import SWITCHED_OFF, TINY_EDSR, TINY_GN, small_net
from tests.conftest import assert_close
from tests.linear_q4_ref import Small
from tests.random_nets import random_net_q4ops, random_net_real
from tests.test_conv_layouts import SWITCHES
from tests.test_plan_audit import PICKS

ALWAYS = lambda x_shape, k_shape, para: True              # noqa: E731  fold_dilated's `worth` under net.fold_dilated = "force"
SEEDS = 20


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for k in SWITCHES + ("PLANER_HIP_INSTNORM_Q4", "PLANER_HIP_LINEAR_Q4", "PLANER_HIP_GROUPNORM_Q4", "PLANER_HIP_PIXEL_SHUFFLE_Q4"):
        monkeypatch.delenv(k, raising=False)


def _nets():
    """name -> (graph, blob, x, compile arguments)"""
    out = {"stylenet b2@32": stylenet.build() + (stylenet.make_input(2, size=32), {}),
           "drn b2@64 folded": drn.build() + (drn.make_input(2, size=64), dict(worth=ALWAYS)),
           "drn b1@40 folded": drn.build() + (drn.make_input(1, size=40), dict(worth=ALWAYS)),
           "fpn-upsample b2@64": fpn.build(via="upsample") + (fpn.make_input(2, size=64), {}),
           "fpn-resize b2@64": fpn.build(via="resize") + (fpn.make_input(2, size=64), {}),
           "edsr-x2": edsr.build(**TINY_EDSR, scale=2) + (edsr.make_input(2, size=TINY_EDSR["size"]), dict(force_q4=True)),
           "edsr-shuffle-tail": edsr.build(**TINY_EDSR, scale=4, tail="shuffle") + (edsr.make_input(2, size=TINY_EDSR["size"]),
                                                                                    dict(force_q4=True)),
           "edsr-unshuffle-in": edsr.build(**TINY_EDSR, scale=2, unshuffle_in=True) + (edsr.make_input(2, size=TINY_EDSR["size"]),
                                                                                       dict(force_q4=True)),
           "resnet_gn": resnet_gn.build(**TINY_GN) + (resnet_gn.make_input(2, size=TINY_GN["size"]), dict(force_q4=True))}
    for s in range(SEEDS):
        g, b, xs = random_net_q4ops(s)
        out["q4ops%d" % s] = (g, b, xs[0], dict(force_q4=True, worth=ALWAYS))
    for s in (3, 18):                                    # the real-scale nets whose dilated convs fold_dilated takes
        g, b, xs = random_net_real(s)
        out["real%d folded" % s] = (g, b, xs[0], dict(worth=ALWAYS))
    return out


NETS = _nets()
# what the audit must have gone through, at the least
MUST = {"stylenet b2@32": {"instancenormalization_q4": 15, "pad_q4": 15},
        "drn b2@64 folded": {"refold_q4": 5},
        "drn b1@40 folded": {"refold_q4": 16},
        "fpn-upsample b2@64": {"upsample_q4": 7, "upsample_add_q4": 2},
        "fpn-resize b2@64": {"resize_q4": 7, "resize_add_q4": 2},
        "edsr-x2": {"pixelshuffle_q4": 1}, "edsr-shuffle-tail": {"pixelshuffle_q4": 1}, "edsr-unshuffle-in": {"pixelshuffle_q4": 1},
        "resnet_gn": {"groupnorm_q4": 20}, "real3 folded": {"refold_q4": 2}, "real18 folded": {"refold_q4": 2}}


def _run(name, pick="first", **kw):
    g, b, x, how = NETS[name] if isinstance(name, str) else name
    body, flow, _ = PA.cpu_program(g, b, x, PICKS[pick], **how)
    trace, outs = PA.cpu_trace(g, b, x, body, flow, **kw)
    return trace, outs, PA.blob_inits(g, b)


@pytest.mark.parametrize("pick", sorted(PICKS))
@pytest.mark.parametrize("name", sorted(NETS))
def test_audit_passes_on_the_oracles_own_run(name, pick):
    trace, _, inits = _run(name, pick)
    worst, census = PA.audit(trace, inits)
    assert max(worst.values()) <= 1.0
    PA.assert_every_step_audited(trace, census)          # a condition: a step the audit has no arm for fails the audit itself
    assert sum(census.kinds.values()) == len(trace) == sum(trace.flow_kinds.values())
    for kind, n in MUST.get(name, {}).items():
        assert census.kinds[kind] >= n, (name, kind, dict(census.kinds))
    if name == "drn b2@64 folded":                       # layer4.0's 1x1 projection and the head conv joined their folds
        assert census.joined_1x1 == 2 and census.junk == 0 and sum(census.folded.values()) >= 8, (census.joined_1x1, dict(census.folded))


@pytest.mark.parametrize("switch", sorted(SWITCHED_OFF))
def test_audit_passes_with_a_feature_switch_off(switch, monkeypatch):
    """The programs of a compiler without the feature: the same checks through the NCHW arms."""
    monkeypatch.setenv(switch, "0")
    name, has, has_not = SWITCHED_OFF[switch]
    g, b, x = small_net(name)
    trace, _, inits = _run((g, b, x, dict(force_q4=True)))
    worst, census = PA.audit(trace, inits)
    assert max(worst.values()) <= 1.0
    PA.assert_every_step_audited(trace, census)
    assert all(census.kinds[k] for k in has) and not any(census.kinds[k] for k in has_not), dict(census.kinds)


def test_every_step_audited_sees_a_step_left_out():
    trace, _, inits = _run("edsr-x2")
    _, census = PA.audit(trace, inits)
    census.kinds["pixelshuffle_q4"] -= 1
    with pytest.raises(AssertionError, match="pixelshuffle_q4"):
        PA.assert_every_step_audited(trace, census)


def test_in_place_kinds_come_from_the_plans_table():
    from planer_amd import plan
    assert set(PA.IN_PLACE) == {k for k, t in plan.KINDS.items() if plan.W in t}
    assert {"instancenormalization", "instancenormalization_q4", "groupnorm", "groupnorm_q4", "erf", "relu_q4", "clip"} <= set(PA.IN_PLACE)


def test_q4ops_generator_reaches_every_kind():
    """Over the seeds the tests use (forced Q4, every eligible conv folded): each audited kind, a junk-keyed tensor, a refold from
    fold to fold, a shuffle that ends the program, a group norm that stays NCHW, joins, and every block."""
    seen = collections.Counter()
    for seed in range(SEEDS):
        g, b, x, how = NETS["q4ops%d" % seed]
        assert 1 <= x.shape[0] <= 3 and all(10 <= v <= 40 for v in x.shape[2:])
        body, flow, shapes = PA.cpu_program(g, b, x, **how)
        for kind, para, srcs, dst, name in PA.steps_of(body, flow):
            seen[kind] += 1
            keys = [k for k in srcs + PA._as_list(dst) if PA.key_fold(k)]
            seen["junk key"] += any(PA.key_fold(k)[1] for k in PA._as_list(dst) if PA.key_fold(k))
            if kind == "refold_q4":
                seen["fold to fold"] += (1, 1) not in (tuple(para["from"]), tuple(para["to"]))
            elif keys:
                seen["folded " + kind] += 1
            if kind == "pixelshuffle_q4":
                seen["nchw_out"] += bool(para.get("nchw_out"))
                seen.update(["shuffle " + para["order"], "shuffle r%d" % para["r"], "unshuffle" if para["inverse"] else "shuffle"])
            if kind in ("instancenormalization_q4", "groupnorm_q4"):
                seen[kind + " with residual"] += srcs[-1] != "None" and len(srcs) in (4, 6)
                seen[kind + " with relu"] += bool(para.get("act"))
            if kind == "pad_q4":
                seen["pad " + para.get("mode", "constant")] += 1
            if kind == "pad" and para.get("constant_value"):             # what plan.pad_q4_ok declines, between convs that run Q4
                seen["pad NCHW, nonzero constant, partial quad"] += shapes[srcs[0].split("@")[0]][1] % 4 > 0
            if kind in ("resize", "resize_q4") and para.get("mode") == "nearest":
                seen["%s nearest" % kind] += 1
                seen["%s nearest by %s" % (kind, "sizes" if len(srcs) > 3 and srcs[3] != "None" else "scales")] += 1
            if kind.endswith("_q4") and isinstance(dst, str) and len(shapes.get(dst.split("@")[0], ())) == 4:
                seen["partial quad"] += shapes[dst.split("@")[0]][1] % 4 > 0
    want = ["instancenormalization_q4", "groupnorm_q4", "groupnorm", "pad_q4", "pixelshuffle_q4", "upsample_q4", "resize_q4",
            "upsample_add_q4", "resize_add_q4", "refold_q4", "junk key", "fold to fold", "nchw_out", "folded conv_q4",
            "instancenormalization_q4 with residual", "instancenormalization_q4 with relu", "groupnorm_q4 with relu",
            "pad reflect", "pad edge", "pad constant", "partial quad", "shuffle crd", "shuffle dcr", "shuffle r2", "shuffle r3",
            "shuffle", "unshuffle", "folded relu_q4", "folded add_q4", "folded concat_q4", "resize_q4 nearest", "resize nearest",
            "resize_q4 nearest by sizes", "resize_q4 nearest by scales", "pad NCHW, nonzero constant, partial quad"]
    assert all(seen[k] >= 1 for k in want), [(k, seen[k]) for k in want if seen[k] < 1]


@pytest.mark.parametrize("pick", sorted(PICKS))
def test_rewrites_preserve_the_flow_on_q4ops_graphs(pick):
    """The compiler's passes, fold_dilated among them, interpreted with the numpy stand-ins, give the tensors of the flow as written."""
    for seed in range(SEEDS):
        g, b, x, _ = NETS["q4ops%d" % seed]
        ref = onp.OracleNet()
        ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
        ref.load_weights(b)
        want = ref(x.copy())
        want = want if isinstance(want, tuple) else (want,)
        _, got, _ = _run("q4ops%d" % seed, pick)
        assert len(got) == len(want)
        for o, w in zip(got, want):
            assert o.shape == w.shape, seed
            assert_close(np.ascontiguousarray(o), np.ascontiguousarray(w), 1e-5, "seed %d" % seed)


# ---- planted faults -------------------------------------------------------------------------------------------------------------
def _first(trace, pred):
    return next(s for s in trace if pred(s))


def _rewrite(q, y):
    """Put the NCHW values `y` into the Q4Host `q` (which may be the tensor an in-place step hands on)."""
    if isinstance(q, PA.Q4Host):
        q.data[...] = PA.pack_q4(np.asarray(y, np.float32)).data
    else:
        q[...] = y
    return q


def _fails(name, step, pick="first", match=None, **kw):
    bad, outs, inits = _run(name, pick, **kw)
    with pytest.raises(PA.AuditError, match=match or step.name.replace("+", r"\+")):
        PA.audit(bad, inits)
    return outs


def _at(step_name, change):
    def fault(s, outs):
        return change(s, outs) if s.name == step_name else outs
    return fault


def test_planted_fault_one_instancenorm_element_off_by_twice_its_tol():
    trace, clean, inits = _run("stylenet b2@32")
    step = _first(trace, lambda s: s.name == "r2a_in+")
    x = PA.nchw(step.ins[0])
    ref, tol = GN.reference(x, inits[step.src[1]], inits[step.src[2]], act=step.para["act"], groups=x.shape[1])
    c, y, xx = np.unravel_index(int(np.argmax(np.abs(ref[0]))), ref[0].shape)

    def change(s, outs):
        outs[0].data[0, c // 4, y, xx, c % 4] += np.float32(2 * tol[0, c, y, xx])
        return outs
    outs = _fails("stylenet b2@32", step, fault=_at(step.name, change))
    for o, w in zip(outs, clean):
        assert_close(o, w, 1e-4)                       # the end-to-end check does not see it


def _norm_on_input(dc):
    """x (2, 8, 9, 11) with a DC offset -> instance norm -> conv."""
    s = Small()
    rng = np.random.default_rng(2)
    s.g.init("n_s", rng.uniform(0.5, 1.5, 8).astype(np.float32))
    s.g.init("n_t", (rng.standard_normal(8) * 0.1).astype(np.float32))
    y = s.g.op("relu", "x", "x_r", name="front")
    y = s.g.op("instancenormalization", [y, "n_s", "n_t"], "n", name="norm", epsilon=1e-5)
    g, b = s.finish(s.conv(y, "z"))
    return g, b, (rng.standard_normal((2, 8, 9, 11)) + dc).astype(np.float32), dict(force_q4=True)


def test_planted_fault_variance_as_mean_of_squares_minus_square_of_mean():
    net = _norm_on_input(64.0)
    trace, _, inits = _run(net)
    step = _first(trace, lambda s: s.kind.startswith("instancenormalization"))
    x = PA.nchw(step.ins[0])
    rows = x.reshape(-1, x.shape[2] * x.shape[3])
    sr, br = np.tile(inits["n_s"], x.shape[0]), np.tile(inits["n_t"], x.shape[0])
    PA.audit(trace, inits)
    good = RO.emulate_instancenorm(rows, sr, br, 1e-5)                 # the kernel's own order of operations is inside the bound
    PA.audit(_run(net, fault=_at(step.name, lambda s, outs: [_rewrite(outs[0], good.reshape(x.shape))]))[0], inits)
    bad = RO.emulate_instancenorm(rows, sr, br, 1e-5, two_pass=False)
    _fails(net, step, fault=_at(step.name, lambda s, outs: [_rewrite(outs[0], bad.reshape(x.shape))]))


def test_planted_fault_norm_residual_from_another_tensor_of_the_same_shape():
    trace, _, _ = _run("stylenet b2@32")
    step = _first(trace, lambda s: s.kind == "instancenormalization_q4" and len(s.src) == 4 and s.src[3] != "None")
    before, res = PA.nchw(step.ins[0]).copy(), PA.nchw(step.ins[3]).copy()       # the norm's own input has the residual's shape
    assert before.shape == res.shape and not np.array_equal(before, res)
    _fails("stylenet b2@32", step, fault=_at(step.name, lambda s, outs: [_rewrite(outs[0], PA.nchw(outs[0]) - res + before)]))


def test_planted_fault_edge_where_reflect_was_asked_at_one_border():
    trace, _, _ = _run("stylenet b2@32")
    step = _first(trace, lambda s: s.kind == "pad_q4" and s.para["mode"] == "reflect")

    def change(s, outs):
        outs[0].data[:, :, 0] = outs[0].data[:, :, 1]                            # the top row only: row 0 of x again, not row 1
        return outs
    _fails("stylenet b2@32", step, fault=_at(step.name, change))


def test_planted_fault_dcr_shuffle_written_as_crd():
    g, b = PS.sandwich("dcr", False, r=2, narrow=4)
    net = (g, b, PS.make_x(), dict(force_q4=True))
    step = _first(_run(net)[0], lambda s: s.kind == "pixelshuffle_q4")
    assert step.para["order"] == "dcr"
    _fails(net, step, fault=_at(step.name, lambda s, outs: [_rewrite(outs[0], PS.shuffle_np(PA.nchw(s.ins[0]), 2, "crd"))]))


def _align_corners_x2(x):
    n, c, h, w = x.shape
    ry, rx = np.linspace(0, h - 1, 2 * h), np.linspace(0, w - 1, 2 * w)
    y0, x0 = np.minimum(ry.astype(int), h - 2), np.minimum(rx.astype(int), w - 2)
    fy, fx = (ry - y0)[:, None], (rx - x0)[None, :]
    a, b_, c_, d = (x[:, :, y0 + i][:, :, :, x0 + j] for i in (0, 1) for j in (0, 1))
    return (a * (1 - fy) * (1 - fx) + b_ * (1 - fy) * fx + c_ * fy * (1 - fx) + d * fy * fx).astype(np.float32)


def test_planted_fault_linear_upsample_with_align_corners_weights():
    name = "fpn-upsample b2@64"
    step = _first(_run(name)[0], lambda s: s.kind == "upsample_q4" and s.para["mode"] == "linear" and PA.nchw(s.ins[0]).shape[2] >= 4)
    _fails(name, step, fault=_at(step.name, lambda s, outs: [_rewrite(outs[0], _align_corners_x2(PA.nchw(s.ins[0])))]))


def test_planted_fault_resize_add_that_drops_the_add():
    name = "fpn-resize b2@64"
    step = _first(_run(name)[0], lambda s: s.kind == "resize_add_q4")
    plain = lambda s: onp.OPS["resize"](PA.nchw(s.ins[0]), np.zeros(0, np.float32), np.array([1, 1, 2, 2], np.float32), **s.para)   # noqa: E731
    _fails(name, step, fault=_at(step.name, lambda s, outs: [_rewrite(outs[0], plain(s))]))


def _tail_cell(q):
    dh, dw, h, w = q.fold
    a = q.nchw()
    return tuple(int(v) for v in np.argwhere(FR.tail_mask((a.shape[0] // (dh * dw), a.shape[1], h, w), dh, dw))[-1])


def test_planted_fault_refold_leaves_a_value_in_a_zero_fill_cell():
    """5 x 5 maps folded by 2: the refold's own check sees the cell; and the folded 3x3 conv that reads the tensor refuses it too."""
    name = "drn b1@40 folded"
    trace, _, inits = _run(name)
    reader = _first(trace, lambda s: s.kind == "conv_q4" and PA.fold_of(s.ins[0]) is not None and inits[s.src[1].split("@")[0]].shape[2:] == (3, 3))
    step = _first(trace, lambda s: s.kind == "refold_q4" and s.dst[0] == reader.src[0])
    n, c, y, x = _tail_cell(step.outs[0])

    def change(s, outs):
        if s.dst[0] == reader.src[0]:
            outs[0].data[n, c // 4, y, x, c % 4] = 1e-3
        return outs
    bad, outs, _ = _run(name, fault=change)
    with pytest.raises(PA.AuditError, match=r"refold_q4.*element \(%d, %d, %d, %d\)" % (n, c, y, x)):
        PA.audit(bad, inits)
    for o, w in zip(outs, _run(name)[1]):
        assert_close(o, w, 1e-4)                       # one cell along a phase border: well inside the end-to-end tolerance
    dirty = _first(bad, lambda s: s.name == reader.name)
    with pytest.raises(PA.AuditError, match=r"zero-fill cell \(%d, %d, %d, %d\) = 0.001" % (n, c, y, x)):
        PA.Audit(inits).check(dirty)


def test_planted_fault_junk_keyed_tensor_read_by_another_step():
    name = "drn b1@40 folded"
    trace, _, inits = _run(name)
    step = _first(trace, lambda s: s.kind == "refold_q4" and PA.key_fold(s.src[0]) and PA.key_fold(s.src[0])[1])
    step.kind = "relu_q4"
    with pytest.raises(PA.AuditError, match="junk key"):
        PA.audit(trace, inits)


def test_planted_fault_reader_of_what_an_nchw_groupnorm_rewrote():
    """layer.GroupNorm leaves the inner norm's values in x, which no trace holds: a later reader of x is refused."""
    g, b = GN.sandwich(c=6, groups=2)                                     # 3 channels per group: no channel-quad form
    net = (g, b, GN.make_x(), dict(force_q4=True))
    trace, _, inits = _run(net)
    at = next(i for i, s in enumerate(trace) if s.kind == "groupnorm")
    PA.audit(trace, inits)
    x = trace[at].ins[0]
    trace.insert(at + 1, PA.Step("late", "leakyrelu", {"alpha": 0.1}, [trace[at].src[0]], ["late_y"], [x], [onp.OPS["leakyrelu"](x.copy(), alpha=0.1)]))
    with pytest.raises(PA.AuditError, match="late.*rewritten by an NCHW groupnorm"):
        PA.audit(trace, inits)


def test_planted_fault_folded_conv_with_two_phases_swapped():
    name = "drn b2@64 folded"
    step = _first(_run(name)[0], lambda s: s.kind == "conv_q4" and PA.fold_of(s.ins[0]) is not None)

    def change(s, outs):
        outs[0].data[[0, 1]] = outs[0].data[[1, 0]]
        return outs
    _fails(name, step, fault=_at(step.name, change))


def test_planted_fault_folded_residual_reshaped_instead_of_folded():
    name = "drn b2@64 folded"
    step = _first(_run(name)[0], lambda s: s.kind == "conv_q4" and PA.fold_of(s.ins[0]) is not None and len(s.src) > 5 and s.src[5] != "None")
    dh, dw, h, w = step.ins[0].fold

    def conv(s, x, K, B=None, scale=None, shift=None, res=None, **kw):
        if s.name == step.name:
            res = FR.unfold_np(res, dh, dw, h, w).reshape(res.shape)              # the unfolded tensor's bytes read as a folded one
        return PA._conv_np(x, K, B, scale, shift, res, **kw)
    _fails(name, step, conv=conv)


def test_planted_fault_dirty_padding_lane_after_pad_q4():
    s = Small()
    s.g.init("pads", np.array([0, 0, 1, 2, 0, 0, 2, 1], np.int64))
    y = s.conv("x", "a", cin=4, cout=6)
    y = s.g.op("pad", [y, "pads"], "p", name="pad", mode="reflect")
    g, b = s.finish(s.conv(y, "z", cin=6))
    net = (g, b, np.random.default_rng(3).standard_normal((2, 4, 6, 7)).astype(np.float32), dict(force_q4=True))
    step = _first(_run(net)[0], lambda s: s.kind == "pad_q4")
    assert step.outs[0].chan == 6

    def change(s, outs):
        outs[0].data[0, -1, 0, 0, 3] = 1e-3
        return outs
    _fails(net, step, fault=_at(step.name, change), match="padding lane 3")


@pytest.mark.parametrize("fam", ["f2x2", "f4x4", "w1d4"])
def test_winograd_bound_counts_the_tile_on_maps_with_holes(fam):
    """A ReLU map behind a nearest upsample has 2x2 blocks of zeros over every channel.  A Winograd output whose own receptive
    field is all zeros still gets the rounding error of its tile: the float32 emulation of the family is outside the element's
    own bound there and inside ref64.bound(reach=REACH[fam]), as it is on the dense calibration maps."""
    from tests import ref64 as R
    rng = np.random.default_rng(19)
    x = np.maximum(rng.standard_normal((2, 4, 11, 9)) - 0.8, 0).astype(np.float32).repeat(2, axis=2).repeat(2, axis=3)
    K = (rng.standard_normal((5, 4, 3, 3)) * 0.3).astype(np.float32)
    conv = dict(pads=[1, 1, 1, 1])
    ref = R.conv64(x, K, **conv)
    y = R.wino_emulate(x, K, *R.wino_family(fam, *x.shape[2:]))
    if fam != "f2x2":                                  # (2x2 tiles reach one pixel: the element's own bound still holds here)
        assert R.ratio(y, ref, R.bound(x, K, lam=R.LAMBDA[fam], **conv)).max() > 1.0
    assert R.ratio(y, ref, R.bound(x, K, lam=R.LAMBDA[fam], reach=R.REACH[fam], **conv)).max() <= 0.25
    for name, xc, Kc in R.calibration_cases():
        if name in ("skew", "odd", "dc50"):
            yc = R.wino_emulate(xc, Kc, *R.wino_family(fam, *xc.shape[2:]))
            assert R.ratio(yc, R.conv64(xc, Kc, **conv), R.bound(xc, Kc, lam=R.LAMBDA[fam], reach=R.REACH[fam], **conv)).max() <= 0.25

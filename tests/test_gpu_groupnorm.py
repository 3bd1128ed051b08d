"""pl_groupnorm_q4_f32 on a real MI355X (q4.GroupNormQ4; csrc/groupnorm_q4_kernel.h) and the nets that use it.

The kernel is held to the float64 reference and the per-element bound of tests/groupnorm_ref.py -- tests/ref64_ops.instancenorm_bound
on the group rows, carried through the roundings of gamma, beta and the residual -- at DC offsets 0, 50 and 1e3, for every tail
and every affine form, over a grid that reaches each form (single, pair, wide with 1, 2 and 3 planes per group), the wave and
workgroup boundaries, the one-workgroup limit from both sides, a last chunk of 2 float4s and a chunk that straddles two planes.
Run with -s for the worst err / bound per case.  Then tiny ResNet-GN and the conv -> norm -> conv sandwiches against the oracle,
switch on against switch off, step by step, and from a plan file."""
import zlib

import numpy as np
import pytest

from oracle import planer_np as onp
from tests import ref64_ops as R
from tests.conftest import RTOL, assert_close
from tests.groupnorm_ref import operands, reference, sandwich
from tests.linear_q4_ref import assert_same_bits, padding_lanes

pytestmark = pytest.mark.gpu

N = 2
P, K = 4096, 2048           # PL_INSTNORM_Q4_ONE_WG_PIXELS, PL_INSTNORM_Q4_CHUNK_PIXELS (tests/test_gpu_instancenorm_q4.py asserts them)
# (C, G): cpg 1 with a partial quad; cpg 2 with a padding pair and without; cpg 4; cpg 8, two planes per group; cpg 12, three
FORMS = [(5, 5), (6, 3), (8, 4), (8, 2), (16, 2), (12, 1)]
# 1, 63, 64, 65, 255, 256, 257 pixels
PLANES = [(1, 1), (7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (1, 257)]
# cpg 8: a run of exactly P float4s, one more (three chunks, 2 float4s in the last), a chunk that straddles the two planes of a
# group at float4 3000 of 6000; a pair and a single plane just over the one-workgroup limit
EDGES = [((16, 2), (32, 64)), ((16, 2), (3, 683)), ((16, 2), (50, 60)), ((6, 3), (17, 241)), ((5, 5), (17, 241))]
GRID = [(f, p) for f in FORMS for p in PLANES] + EDGES
DCS = [0.0, 50.0, 1e3]
TAILS = [(False, 0), (True, 0), (False, 1), (True, 1)]          # (residual, act)
AFFINE = [(True, True), (True, False), (False, False)]          # (gamma, beta)


def _id(case):
    (c, g), (h, w) = case
    return "C%d-G%d-%dx%d" % (c, g, h, w)


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _form(c, g, hw):
    """The launch-plan string pl_groupnorm_q4_f32 leaves for C channels in G groups on hw pixels."""
    cpg = c // g
    lanes, row = ("wide", cpg // 4 * hw) if cpg % 4 == 0 else ("pair" if cpg == 2 else "single", hw)
    return "groupnorm-q4 %s %s" % (lanes, "one-wg" if row <= P else "chunks=%d" % -(-row // K))


def test_the_grid_reaches_every_boundary():
    rows = {_id(case): _form(case[0][0], case[0][1], case[1][0] * case[1][1]) for case in GRID}
    assert rows["C16-G2-32x64"] == "groupnorm-q4 wide one-wg" and 2 * 32 * 64 == P
    assert rows["C16-G2-3x683"] == "groupnorm-q4 wide chunks=3" and 2 * 3 * 683 - 2 * K == 2
    assert rows["C16-G2-50x60"] == "groupnorm-q4 wide chunks=3" and K < 3000 < 2 * K
    assert rows["C6-G3-17x241"] == "groupnorm-q4 pair chunks=3" and rows["C5-G5-17x241"] == "groupnorm-q4 single chunks=3"
    assert {r.split()[1] for r in rows.values()} == {"wide", "pair", "single"}


def _dirty_q4(pa, x):
    """to_q4(x) with every padding lane of the buffer set to NaN: the kernel must write +0.0 there and keep them out of the sums."""
    from planer_amd import q4
    raw = q4.to_q4(pa.hip.asarray(x)).get()
    c = x.shape[1]
    for ch in range(c, raw.shape[1] * 4):
        raw[:, ch // 4, :, :, ch % 4] = np.nan
    xq = pa.hip.asarray(raw)
    xq.chan = c
    return xq


def _run(pa, x, gs, gb, ga, be, r, act, groups):
    """-> (NCHW result, raw Q4 buffer) of GroupNormQ4; asserts that it worked in place and which form ran."""
    q4 = pa.q4
    dev = lambda v: None if v is None else pa.hip.asarray(v)           # noqa: E731
    xq = _dirty_q4(pa, x)
    rq = q4.to_q4(pa.hip.asarray(r)) if r is not None else None
    yq = q4.GroupNormQ4(xq, dev(gs), dev(gb), dev(ga), dev(be), rq, groups=groups, act=act)
    assert yq is xq
    assert xq.ctx.last_conv_plan() == _form(x.shape[1], groups, x.shape[2] * x.shape[3])
    raw = xq.get()
    if r is not None:
        assert (rq.get() == q4.to_q4(pa.hip.asarray(r)).get()).all()             # the residual is only read
    return q4.from_q4(xq).get(), raw


@pytest.mark.parametrize("case", GRID, ids=_id)
def test_against_float64_within_the_bound(pa, case):
    (c, groups), (h, w) = case
    worst = 0.0
    for dc in DCS:
        for res, act in TAILS:
            for gamma, beta in AFFINE:
                x, gs, gb, ga, be, r = operands(_rng("gnq4", case, dc, res, act, gamma), (N, c, h, w), groups, dc, res, gamma, beta)
                ref, tol = reference(x, gs, gb, ga, be, r, act, groups)
                y, raw = _run(pa, x, gs, gb, ga, be, r, act, groups)
                what = "groupnorm q4 %s dc=%g res=%d act=%d gamma=%d beta=%d" % (_id(case), dc, res, act, gamma, beta)
                ratio = R.check(y, ref, tol, what)
                worst = max(worst, ratio)
                assert not padding_lanes(raw, c).any(), what + ": padding lanes are not +0.0"
                if act:
                    assert (y[ref < -tol] == 0).all(), what
    print("%-24s %-28s worst err/tol %.3f over %d runs" % (_id(case), _form(c, groups, h * w), worst, len(DCS) * len(TAILS) * len(AFFINE)))


@pytest.mark.parametrize("case", [((6, 3), (5, 13)), ((8, 2), (16, 16)), ((16, 2), (50, 60)), ((5, 5), (17, 241))], ids=_id)
def test_images_are_independent_and_runs_repeat(pa, case):
    (c, groups), (h, w) = case
    for res, act in ((False, 0), (True, 1)):
        x, gs, gb, ga, be, r = operands(_rng("gn-rep", case, res), (N, c, h, w), groups, 50.0, res)
        x[1] = x[0]
        if r is not None:
            r[1] = r[0]
        y, raw = _run(pa, x, gs, gb, ga, be, r, act, groups)
        assert_same_bits(y[1], y[0], "two images that hold the same data")
        again, raw2 = _run(pa, x, gs, gb, ga, be, r, act, groups)
        assert (raw.view(np.uint32) == raw2.view(np.uint32)).all(), "two runs differ"
        alone, _ = _run(pa, x[:1], gs, gb, ga, be, None if r is None else r[:1], act, groups)
        assert_same_bits(alone, y[:1], "an image alone against the same image in a batch of two")


@pytest.mark.parametrize("case", [((6, 3), (5, 13)), ((8, 4), (17, 241)), ((8, 2), (5, 13)), ((16, 2), (50, 60)), ((5, 5), (8, 8))], ids=_id)
def test_a_nan_stays_in_its_group(pa, case):
    (c, groups), (h, w) = case
    cpg = c // groups
    x, gs, gb, ga, be, _ = operands(_rng("gn-nan", case), (N, c, h, w), groups)
    clean = x.copy()
    g = 1                                               # the poisoned group: it shares a quad, or a plane boundary, with group 0 / 2
    x[1, g * cpg + cpg - 1, h // 2, w - 1] = np.nan
    y, _ = _run(pa, x, gs, gb, ga, be, None, 0, groups)
    assert np.isnan(y[1, g * cpg:(g + 1) * cpg]).all()
    keep = np.ones(y.shape, bool)
    keep[1, g * cpg:(g + 1) * cpg] = False
    assert not np.isnan(y[keep]).any()
    ref, tol = reference(clean, gs, gb, ga, be, None, 0, groups)
    R.check(np.where(keep, y, 0), np.where(keep, ref, 0), tol, "the other groups beside the NaN group")


@pytest.mark.parametrize("case", [((8, 2), (16, 16)), ((16, 2), (50, 60)), ((6, 3), (17, 241))], ids=["one-wg", "chunked", "pair"])
def test_under_pool_hygiene(pa, case):
    """Every fresh block poisoned and guarded (the statistics scratch block included): guards intact, the result within the bound
    and the same bits as without the mode."""
    (c, groups), (h, w) = case
    ctx = pa.hip.context()
    x, gs, gb, ga, be, r = operands(_rng("gn-hyg", case), (N, c, h, w), groups, 50.0, True)
    ref, tol = reference(x, gs, gb, ga, be, r, 1, groups)
    base, _ = _run(pa, x, gs, gb, ga, be, r, 1, groups)
    ctx.synchronize()
    ctx.pool_debug(pa.hip.POOL_GUARD_BYTES, 0xFF)
    try:
        y, raw = _run(pa, x, gs, gb, ga, be, r, 1, groups)
        dirty, report = ctx.pool_debug_check()
    finally:
        ctx.pool_debug(0)
    assert dirty == 0, report
    R.check(y, ref, tol, "under hygiene")
    assert_same_bits(y, base, "under hygiene against the plain run")
    assert not padding_lanes(raw, c).any()


def test_entry_point_refuses_before_it_launches(pa):
    """Every refusal comes back from the argument checks: the tensor is unchanged afterwards."""
    lib = pa._lib.load()
    ctx = pa.hip.context()
    xb = pa.hip.zeros((4096,))
    xb.set(np.arange(4096, dtype=np.float32))
    sb = pa.hip.asarray(np.ones(16, np.float32))
    before = xb.get()
    h, x, s = ctx.handle, xb.ptr, sb.ptr
    gn = lib.pl_groupnorm_q4_f32
    INVAL, UNSUP = pa._lib.PL_EINVAL, pa._lib.PL_EUNSUPPORTED
    calls = [
        (UNSUP, "3 channels per group", (h, x, s, s, s, s, None, 1, 6, 16, 2, 1e-5, 0)),
        (UNSUP, "6 channels per group", (h, x, s, s, None, None, None, 1, 12, 16, 2, 1e-5, 0)),
        (UNSUP, "3 channels per group", (h, x, s, s, None, None, None, 0, 6, 16, 2, 1e-5, 0)),
        (INVAL, "must divide the channel count", (h, x, s, s, s, s, None, 1, 8, 16, 3, 1e-5, 0)),
        (INVAL, "act must be 0 \\(none\\) or 1 \\(relu\\)", (h, x, s, s, s, s, None, 1, 8, 16, 2, 1e-5, 2)),
        (INVAL, "16-byte aligned", (h, x + 4, s, s, s, s, None, 1, 8, 16, 2, 1e-5, 0)),
        (INVAL, "16-byte aligned", (h, x, s, s, s, s, x + 8, 1, 8, 16, 2, 1e-5, 0)),
        (INVAL, "null argument", (h, x, None, s, s, s, None, 1, 8, 16, 2, 1e-5, 0)),
        (INVAL, "null argument", (h, x, s, None, s, s, None, 1, 8, 16, 2, 1e-5, 0)),
        (INVAL, "null argument", (h, None, s, s, s, s, None, 1, 8, 16, 2, 1e-5, 0)),
        (INVAL, "bad shape", (h, x, s, s, s, s, None, 1, 8, 16, 0, 1e-5, 0)),
        (UNSUP, "tensor too large", (h, x, s, s, s, s, None, 2 ** 15, 8, 2 ** 14, 2, 1e-5, 0)),
    ]
    for code, text, args in calls:
        rc = gn(*args)
        assert rc == code, (text, rc, lib.pl_last_error())
        with pytest.raises(NotImplementedError if code == UNSUP else ValueError, match=text):
            pa._lib.check(rc)
    ctx.synchronize()
    np.testing.assert_array_equal(xb.get(), before)


def test_layer_functions_refuse_what_has_no_form(pa):
    from planer_amd import layer, q4
    dev = pa.hip.asarray
    x = _rng("gn-refuse").standard_normal((2, 6, 4, 4)).astype(np.float32)
    xq = q4.to_q4(dev(x))
    two, six = dev(np.ones(2, np.float32)), dev(np.ones(6, np.float32))
    with pytest.raises(NotImplementedError, match="3 channels per group"):
        q4.GroupNormQ4(xq, two, two, groups=2)
    with pytest.raises(ValueError, match="do not divide"):
        q4.GroupNormQ4(xq, two, two, groups=4)
    with pytest.raises(ValueError, match="do not divide"):
        q4.GroupNormQ4(xq, two, two)
    with pytest.raises(ValueError, match="act is 0"):
        q4.GroupNormQ4(xq, six, six, groups=6, act=2)
    with pytest.raises(ValueError, match="per group"):
        q4.GroupNormQ4(xq, two, two, groups=6)
    with pytest.raises(ValueError, match="per channel"):
        q4.GroupNormQ4(xq, six, six, gamma=two, groups=6)
    with pytest.raises(ValueError, match="residual shape"):
        q4.GroupNormQ4(xq, six, six, resq=q4.to_q4(dev(x[:1])), groups=6)
    with pytest.raises(TypeError):
        q4.GroupNormQ4(dev(x), six, six, groups=6)
    with pytest.raises(ValueError, match="null argument"):
        pa._lib.call("pl_groupnorm_q4_f32", xq.ctx.handle, xq.ptr, None, six.ptr, None, None, None, 2, 6, 16, 6, 1e-5, 0)
    with pytest.raises(ValueError, match="16-byte aligned"):
        pa._lib.call("pl_groupnorm_q4_f32", xq.ctx.handle, xq.ptr + 4, six.ptr, six.ptr, None, None, None, 1, 6, 16, 6, 1e-5, 0)
    assert_same_bits(q4.from_q4(xq).get(), x, "a refused call leaves the tensor alone")
    # the NCHW kind is the five steps on their own kernels, three channels per group included
    s, b = np.array([0.5, 2.0], np.float32), np.array([0.1, -0.2], np.float32)
    ga, be = np.linspace(0.5, 1.5, 6, dtype=np.float32).reshape(6, 1, 1), np.linspace(-1, 1, 6, dtype=np.float32).reshape(1, 6, 1, 1)
    xd = dev(x.copy())
    want = layer.InstanceNormalization(dev(x.copy()).reshape((2, 2, -1)), dev(s), dev(b)).reshape(x.shape)
    want = layer.Add(layer.Mul(want, dev(ga)), dev(be))
    got = layer.GroupNorm(xd, dev(s), dev(b), dev(ga), dev(be), groups=2)
    assert_same_bits(got.get(), want.get(), "layer.GroupNorm against the five layers")
    ref, tol = reference(x, s, b, ga, be, None, 0, 2)
    R.check(got.get(), ref, tol, "layer.GroupNorm against float64")
    assert layer.GroupNorm(xd, dev(s), dev(b), groups=2).ptr == xd.ptr          # without gamma and beta: in place, like the norm


def test_empty_tensors_make_no_launch(pa, monkeypatch):
    from planer_amd import _lib
    q4 = pa.q4
    s, b, ga = (pa.hip.asarray(np.ones(n, np.float32)) for n in (4, 4, 8))
    empties = [q4.to_q4(pa.hip.asarray(np.zeros(xs, np.float32))) for xs in ((0, 8, 4, 4), (2, 8, 0, 4), (2, 8, 3, 0))]
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for xq in empties:
        assert q4.GroupNormQ4(xq, s, b, ga, ga, groups=4, act=1) is xq
    assert calls == []
    x = np.ones((1, 8, 2, 2), np.float32)
    q4.GroupNormQ4(q4.to_q4(pa.hip.asarray(x)), s, b, groups=4)
    assert "pl_groupnorm_q4_f32" in calls
    monkeypatch.undo()
    xq = q4.to_q4(pa.hip.asarray(x))            # the entry point itself: nothing to do is not an error
    _lib.call("pl_groupnorm_q4_f32", xq.ctx.handle, xq.ptr, s.ptr, b.ptr, None, None, None, 0, 8, 4, 4, 1e-5, 0)
    _lib.call("pl_groupnorm_q4_f32", xq.ctx.handle, xq.ptr, s.ptr, b.ptr, None, None, None, 1, 8, 0, 4, 1e-5, 0)
    assert (q4.from_q4(xq).get() == x).all()


# ---- nets ---------------------------------------------------------------------------------------------------------------------
TINY = dict(width=8, groups=4, classes=10, size=32)
# name -> (sandwich options, groupnorm_q4 steps, NCHW groupnorm steps)
SANDWICHES = {"cpg4": dict(groups=2), "cpg2-4d-middle": dict(groups=4, mid="4d"), "cpg1-shape-const-step": dict(groups=8, via_const=True),
              "swapped-leading-1": dict(groups=2, swap_mul=True, swap_add=True, lead=True), "only-mul": dict(groups=2, affine="mul"),
              "no-affine": dict(groups=4, affine="none"), "cpg3": dict(c=6, groups=2)}
NETS = dict({name: (0, 1) if name == "cpg3" else (1, 0) for name in SANDWICHES}, **{"resnet-gn": (20, 0)})


def _oracle(g, b, x):
    ref = onp.OracleNet()
    ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
    ref.load_weights(b)
    return ref(x.copy())


@pytest.fixture(scope="module")
def models():
    from planer_amd.irgen import resnet_gn
    out = {name: sandwich(hw=(6, 7), **opts) + (_rng("gn-net", name).standard_normal((N, 4, 6, 7)).astype(np.float32),)
           for name, opts in SANDWICHES.items()}
    out["resnet-gn"] = resnet_gn.build(**TINY) + (resnet_gn.make_input(N, size=TINY["size"]),)
    return out


@pytest.fixture(scope="module")
def picks():
    """Conv algorithm picks shared by every net of this module, so that a shape is run by one kernel whichever net has it."""
    return {}


def _net(pa, g, b, picks):
    net = pa.from_graph(g, b)
    net.use_q4 = "force"                           # these maps are small: by its cost estimate the plan would stay NCHW
    net._load_algo_cache()
    picks.update({k: v for k, v in net._algo.items() if k not in picks})
    net._algo = picks
    return net


@pytest.fixture(scope="module")
def results(pa, models, picks):
    """name -> (net, net(x)) with the switch at its default."""
    out = {}
    for name, (g, b, x) in models.items():
        net = _net(pa, g, b, picks)
        out[name] = (net, net(x))
    return out


def _flow_kinds(pa, net, x):
    prog, _ = __import__("tests.plan_audit", fromlist=["program"]).program(net, [pa.hip.asarray(x)])
    return [prog.objs[names[0]].name for _, names, _ in prog.flow]


@pytest.mark.parametrize("name", list(NETS))
def test_nets_against_the_oracle(pa, models, results, name):
    g, b, x = models[name]
    net, got = results[name]
    want = _oracle(g, b, x)
    assert got.shape == want.shape
    assert_close(got, want, RTOL, name)
    kinds = _flow_kinds(pa, net, x)
    nq4, nnchw = NETS[name]
    assert kinds.count("groupnorm_q4") == nq4 and kinds.count("groupnorm") == nnchw and net.groupnorms_fused == nq4 + nnchw
    assert not {"reshape", "instancenormalization", "mul", "add_q4", "relu_q4"} & set(kinds), kinds
    if name == "resnet-gn":
        first, gap = kinds.index("conv_q4"), kinds.index("gap_q4")
        assert not {"to_q4", "from_q4"} & set(kinds[first:gap + 1]), kinds


@pytest.mark.parametrize("name", list(NETS))
def test_switch_off_is_the_old_program_and_within_tolerance(pa, models, results, picks, name, monkeypatch):
    g, b, x = models[name]
    monkeypatch.setenv("PLANER_HIP_GROUPNORM_Q4", "0")
    net = _net(pa, g, b, picks)
    off = net(x)
    kinds = _flow_kinds(pa, net, x)
    assert not [k for k in kinds if k.startswith("groupnorm")] and "instancenormalization" in kinds and net.groupnorms_fused == 0
    assert_close(off, _oracle(g, b, x), RTOL, name + " with the switch off")
    if name == "cpg3":          # its only norm runs the NCHW kind: the same kernels on the same values
        assert_same_bits(results[name][1], off, "three channels per group: switch on against off")


@pytest.mark.parametrize("name", list(NETS))
def test_every_groupnorm_q4_step_is_within_the_bound_on_its_own_input(pa, models, results, name):
    from tests.plan_audit import capture, host_inits, nchw
    g, b, x = models[name]
    net, got = results[name]
    trace, out = capture(net, [pa.hip.asarray(x)])
    inits = host_inits(net)
    n, worst = 0, 0.0
    for st in trace:
        if st.kind != "groupnorm_q4":
            continue
        const = lambda key: None if key == "None" else inits[key]          # noqa: E731
        src = st.src + ["None"] * (6 - len(st.src))
        res = None if src[5] == "None" else nchw(st.ins[5])
        ref, tol = reference(nchw(st.ins[0]), const(src[1]), const(src[2]), const(src[3]), const(src[4]), res,
                             int(st.para.get("act", 0)), int(st.para["groups"]), float(st.para.get("epsilon", 1e-5)))
        worst = max(worst, R.check(nchw(st.outs[0]), ref, tol, "%s (%s)" % (st.name, st.para)))
        n += 1
    print("%-24s %d groupnorm_q4 steps, worst err/tol %.3f" % (name, n, worst))
    assert n == NETS[name][0], [st.kind for st in trace]
    assert_close(out[0], got, 1e-5, "the traced eager pass against net(x)")


def test_plan_file_replays_the_norm(pa, models, results):
    from planer_amd.export import export_plan
    from tests.test_gpu_plan_file import _bind, _run_plan
    g, b, x = models["resnet-gn"]
    net, want = results["resnet-gn"]
    blob = export_plan(net, x)
    assert b"pl_groupnorm_q4_f32" in blob and b"pl_instancenorm_f32" not in blob
    out, = _run_plan(_bind(), blob, [x])
    assert_same_bits(out, want, "plan file against net(x)")

"""One NaN, +inf or -inf planted in the input, the filter or the tail of every conv family: which outputs change, and how
(tests/nonfinite_ref.py: containment by bits against the kernel's own clean run under the same plan, propagation and IEEE class
against the float64 reference of the poisoned operands).  Finite data cannot see a stray term that meets a zero filter value or
lands in a discarded lane -- a clamped load times a 0 mask, a neighbour's value under k-step or quad padding, a stale LDS slot, a
tile that reaches into the next image, a tail term of the next channel, a split-K partial sum of another output; one planted
value makes the output provably depend on the wrong input, and the check needs no tolerance.

Every entry point runs the shared table `nonfinite_ref.CASES` the way tests/test_gpu_conv_bounds.py and the per-family files drive
it.  The F(4,4) stem keeps its own test (tests/test_gpu_stem_wino_ring.py).  The last test asserts what the module reached."""
import collections
import re

import numpy as np
import pytest

from tests import nonfinite_ref as NF
from tests.nonfinite_ref import ALPHA, CASES
from tests.ref64 import ACT_NONE, ACT_RELU
from tests.test_gpu_conv_bounds import FAM, PLAN, _cfg_names, _dev
from tests.test_gpu_wf4 import _patch_cells

pytestmark = pytest.mark.gpu
SEEN = {"layouts": set(), "plans": set(), "entries": set(), "plants": 0}


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


class Uploads:
    """Device copies by host array identity: a plant replaces one operand, the others (and what was prepared from them: the Q4
    form of an activation, a packed filter) are uploaded once."""

    def __init__(self, pa):
        self.pa, self.kept = pa, collections.OrderedDict()

    def __call__(self, a, prepare=None, tag=None):
        if a is None:
            return None
        key = (id(a), tag)
        if key not in self.kept or self.kept[key][0] is not a:
            d = _dev(self.pa, a)
            self.kept[key] = (a, prepare(d) if prepare else d)
            while len(self.kept) > 48:
                self.kept.popitem(last=False)
        return self.kept[key][1]


def _entry(pa, case, call, lay, prefix=None, entry=None):
    """-> run(ops, act, what) for nonfinite_ref.sweep: `call(up, ops, act) -> list of (device array, channels or None)`; a Q4
    result is read raw and its padding lanes checked.  The plan of a plant's run is the plan of the clean run."""
    up, ctx, state = Uploads(pa), pa.hip.context(), {}

    def run(ops, act, what):
        outs = call(up, ops, act)
        plan = ctx.last_conv_plan()
        if what.endswith(" clean"):
            state["plan"] = plan
            assert prefix is None or plan.startswith(prefix), (what, plan)
            SEEN["plans"].add(plan)
            SEEN["layouts"].add(lay)
            if entry:
                SEEN["entries"].add(entry)
        assert plan == state["plan"], "%s ran [%s], the clean run [%s]" % (what, plan, state["plan"])
        return [NF.padding_lanes(y.get(), chan, what) if chan else np.ascontiguousarray(y.get() if hasattr(y, "get") else y)
                for y, chan in outs]
    return run


def _sweep(case, run, label, **kw):
    SEEN["plants"] += NF.sweep(case, run, label=label + " ", **kw)


def _q4res(up, r):
    from planer_amd import q4
    return up(r, q4.to_q4, "q4")


# ---- direct families --------------------------------------------------------------------------------------------------------------
def _nchw(pa, case, lay=0, prepare=None):
    def call(up, ops, act):
        x, K, B, sc, sh, r = ops
        return [(pa.ConvFused(up(x), up(K, prepare, lay), up(B), up(sc), up(sh), up(r), act=act, alpha=ALPHA, w_layout=lay, **case.conv),
                 None)]
    return call


def _quad(pa, case, lay, prepare, x_nchw=False):
    from planer_amd import q4

    def call(up, ops, act):
        x, K, B, sc, sh, r = ops
        xq = up(x) if x_nchw else up(x, q4.to_q4, "q4")
        y = q4.ConvQ4(xq, up(K, prepare, lay), up(B), up(sc), up(sh), _q4res(up, r), act=act, alpha=ALPHA, w_layout=lay, **case.conv)
        return [(y, K.shape[0])]
    return call


DIRECT = ["d_6to10", "k3x5_s2x1_d1x2", "k1x7_s1x2", "g2_cin3_cout5", "c32_1x1_s2"]


@pytest.mark.parametrize("name", DIRECT)
def test_direct_nchw_tap_major_and_q4_default_plan(pa, name):
    from planer_amd import q4
    case = CASES[name]
    _sweep(case, _entry(pa, case, _nchw(pa, case), 0), "nchw")
    if case.ks[1] % 16 == 0 and case.conv["group"] == 1:
        _sweep(case, _entry(pa, case, _nchw(pa, case, 1, pa.prepare_conv_weights), 1), "tap-major")
    prep = lambda d: q4.prepare_q4_weights(d, case.conv["group"])
    if q4.q4_conv_eligible(case.ks, **case.conv):
        _sweep(case, _entry(pa, case, _quad(pa, case, 2, prep), 2), "q4")
    else:                                                   # a group that splits a channel quad: refused, never computed
        ops, act = case.operands(0)
        with pytest.raises((NotImplementedError, ValueError)):
            _quad(pa, case, 2, prep)(Uploads(pa), ops, act)


@pytest.mark.parametrize("split", [1, 2, 3])
def test_every_forced_tile_config(pa, split):
    """Every tile config of the NCHW, tap-major and channel-quad implicit GEMM x split-K (the tail then runs in the reduce kernel,
    whose workspace rows belong to other outputs)."""
    from planer_amd import q4
    ctx, names, case = pa.hip.context(), _cfg_names(pa), CASES["cfg"]
    try:
        for cfg, name in enumerate(names):
            if name.startswith("k") and split > 1:
                continue
            ctx.set_conv_config(cfg, split)
            if name[0] in "qk":
                call, lay = _quad(pa, case, 2, q4.prepare_q4_weights), 2
            elif name.startswith("t"):
                call, lay = _nchw(pa, case, 1, pa.prepare_conv_weights), 1
            else:
                call, lay = _nchw(pa, case), 0
            _sweep(case, _entry(pa, case, call, lay, name + " "), "%s split %d" % (name, split))
    finally:
        ctx.set_conv_config(-1, 0)


HYBRID = [("t64x64x16", 64, 6, 0), ("t128x64x16", 0, 9, 0), ("64x64", 0, 3, 0), ("t64x64x32", 32, 2, 4), ("128x32", 8, 5, 2)]


@pytest.mark.parametrize("row", HYBRID, ids=[r[0] + "-dp%d" % r[1] for r in HYBRID])
def test_hybrid_plans(pa, row):
    """A data-parallel prefix of dp tiles + a split-K tail with the tile reduce (the rows of tests/test_gpu_conv_bounds.py)."""
    name, dp, split, occ = row
    ctx, names, case = pa.hip.context(), _cfg_names(pa), CASES["hybrid"]
    tap = name.startswith("t")
    try:
        ctx.set_conv_plan(names.index(name), dp, split, occ)
        run = _entry(pa, case, _nchw(pa, case, int(tap), pa.prepare_conv_weights if tap else None), int(tap), name + " ", "hybrid")
        _sweep(case, run, "hybrid %s dp %d split %d" % (name, dp, split))
    finally:
        ctx.set_conv_config(-1, 0)


def test_rowpack(pa):
    from planer_amd import q4
    case = CASES["rowpack"]
    _sweep(case, _entry(pa, case, _quad(pa, case, 6, q4.prepare_rowpack_weights, x_nchw=True), 6), "rowpack")


@pytest.mark.parametrize("lay", [10, 12])
def test_stem_maxpool(pa, lay):
    from planer_amd import q4
    case = CASES["stem"]
    prepare = q4.prepare_rowpack_weights if lay == 10 else q4.prepare_stem_nchw_weights
    extra = {} if lay == 10 else dict(w_layout=12)

    def call(up, ops, act):
        x, K, B, sc, sh, _ = ops
        return [(q4.ConvPoolQ4(up(x), up(K, prepare, lay), up(B), up(sc), up(sh), act=act, alpha=ALPHA, **extra, **case.conv), K.shape[0])]
    _sweep(case, _entry(pa, case, call, lay, "stem+maxpool " if lay == 10 else "stem+maxpool(nchw)"), "stem+maxpool %d" % lay)


@pytest.mark.parametrize("name", ["smallcin_2to70", "smallcin_1to20"])
@pytest.mark.parametrize("valu", ["0", "1"], ids=["mfma", "valu"])
def test_small_cin(pa, name, valu, monkeypatch):
    case = CASES[name]
    monkeypatch.setenv("PLANER_HIP_SMALLCIN", "1")
    monkeypatch.setenv("PLANER_HIP_SMALLCIN_VALU", valu)

    def call(up, ops, act):
        x, K, B = ops[:3]
        return [(pa.Conv2d(up(x), up(K), up(B), pads=case.conv["pads"]), None)]
    run = _entry(pa, case, call, 0, "smallcin3x3valu" if valu == "1" else "smallcin3x3")
    _sweep(case, run, "smallcin valu=" + valu)
    plan = pa.hip.context().last_conv_plan()
    assert plan.startswith("smallcin3x3valu") == (valu == "1"), plan


@pytest.mark.parametrize("name", ["dw_7x7_d8", "dw_3x5_s2x1_d1x2"])
def test_depthwise(pa, name):
    from planer_amd import q4
    case = CASES[name]
    _sweep(case, _entry(pa, case, _nchw(pa, case), 0, "depthwise-nchw"), "depthwise-nchw")
    _sweep(case, _entry(pa, case, _quad(pa, case, 13, q4.prepare_dw_q4_weights), 13, "depthwise-q4"), "depthwise-q4")


@pytest.mark.parametrize("name", ["convt_k3_even", "convt_k3_odd"])
@pytest.mark.parametrize("prepared", [True, False], ids=["layout14", "unprepared"])
def test_convtranspose_by_phase(pa, name, prepared):
    from planer_amd import q4
    case = CASES[name]
    geo = {k: list(case.extra[k]) for k in ("strides", "pads", "output_padding")}
    prepare = (lambda d: q4.prepare_convt_q4_weights(d, tuple(geo["strides"]))) if prepared else None

    def call(up, ops, act):
        x, K, B, sc, sh, r = ops
        y = q4.ConvTransposeQ4(up(x, q4.to_q4, "q4"), up(K, prepare, prepared), up(B), up(sc), up(sh), _q4res(up, r), act=act,
                               alpha=ALPHA, w_layout=14 if prepared else 0, **geo)
        return [(y, K.shape[1])]
    _sweep(case, _entry(pa, case, call, 14, "convt-q4 phases=2x2"), "convt")


def test_sibling_pair(pa):
    """The plant reaches both outputs, each by its own receptive field; a filter or tail plant of one sibling leaves the other's
    bits alone."""
    from planer_amd import q4
    case = CASES["pair"]
    s = case.conv["strides"]
    p1 = dict(strides=s, pads=case.conv["pads"], act=ACT_RELU, alpha=0.0)
    p2 = dict(strides=s, pads=[0, 0, 0, 0], act=ACT_NONE, alpha=0.0)

    def call(up, ops, act):
        x, K1, _, s1, t1, _, K2, b2, s2, t2, _ = ops
        y1, y2 = q4.ConvQ4Pair(up(x, q4.to_q4, "q4"), up(K1, q4.prepare_q4_weights, 2), None, up(s1), up(t1),
                               up(K2, q4.prepare_q4_weights, 2), up(b2), up(s2), up(t2), para1=p1, para2=p2)
        return [(y1, K1.shape[0]), (y2, K2.shape[0])]
    _sweep(case, _entry(pa, case, call, 2, "pair["), "pair")


@pytest.mark.parametrize("name", ["dense_5x72x40", "dense_65x96x255"])
def test_dense(pa, name):
    """Dense as the 1x1 conv of an (m, k, 1, 1) input: a plant in row m changes row m only; in filter row n, column n only."""
    case = CASES[name]
    (m, k), n = case.xs[:2], case.ks[0]
    small = m <= 64 and n >= 32 and k % 8 == 0

    def call(up, ops, act):
        x, W, B = ops[:3]
        y = pa.Dense(up(x.reshape(m, k)), up(W.reshape(n, k)), up(B))
        return [(y.get().reshape(m, n, 1, 1), None)]
    run = _entry(pa, case, call, 0, entry="dense-small" if small else "dense-general")
    _sweep(case, run, "dense")
    plan = pa.hip.context().last_conv_plan()
    assert ("dense32x32" in plan) == small, plan


def test_conv1x1_winograd_in(pa):
    from planer_amd import q4
    from tests import ref64 as R
    case = CASES["c1w"]
    shape = R.wino4_input(np.zeros((case.xs[0], case.ks[0]) + case.xs[2:])).shape

    def call(up, ops, act):
        x, K, B, sc, sh, _ = ops
        v = q4.Conv1x1WinoIn(up(x, q4.to_q4, "q4"), up(K, q4.prepare_q4_weights, 2), up(B), up(sc), up(sh), act=act, alpha=ALPHA, wino=4)
        return [(v.get()[:int(np.prod(shape))].reshape(shape), None)]
    _sweep(case, _entry(pa, case, call, 2, "conv1x1+wino4-in", "conv1x1+wino4-in"), "conv1x1+wino4-in")


# ---- Winograd families ----------------------------------------------------------------------------------------------------------------
LAYS = {"f2x2": (3, 4), "f4x4": (7, 9), "w1d4": (8,), "wino43": (11,)}
WINO = [n for n, c in CASES.items() if c.fam != "direct" and c.kind == "conv"]


def _prep(pa):
    from planer_amd import q4
    return {3: pa.prepare_winograd_weights, 4: q4.prepare_winograd_q4_weights, 7: q4.prepare_winograd4_q4_weights,
            9: q4.prepare_wf4_q4_weights, 8: q4.prepare_w1d4_q4_weights, 11: q4.prepare_winograd43_q4_weights}


@pytest.mark.parametrize("name", WINO)
def test_winograd_families(pa, name, monkeypatch):
    from planer_amd import q4
    from tests.test_gpu_dilated_fold import _folded_conv
    case, prep = CASES[name], _prep(pa)
    d = case.fold
    h, w = -(-case.xs[2] // d), -(-case.xs[3] // d)
    ran = 0
    for lay in LAYS[case.fam]:
        if lay == 3 and (case.xs[1] % 16 or d > 1):
            continue                                            # NCHW F(2x2): Cin % 16 == 0; a folded conv is a Q4 step
        for half in (("1", "0") if lay == 9 else ("",)):
            if half:
                monkeypatch.setenv("PLANER_HIP_EXPERIMENT", "wf4_half=" + half)
            label = "layout %d%s" % (lay, " wf4_half=" + half if half else "")
            if d > 1:
                def call(up, ops, act, lay=lay):
                    x, K, B, sc, sh, r = ops
                    return [(_folded_conv(pa, x, K, B, sc, sh, r, (d, d), lay, prep[lay], act, ALPHA), None)]
            elif lay == 3:
                call = _nchw(pa, case, 3, prep[3])
            else:
                call = _quad(pa, case, lay, prep[lay])
            if lay == 9 and _patch_cells(h, w, 16 if half == "1" else 32) > (512 if half == "1" else 1024):
                # the fused kernel declines patches beyond its LDS buffers: refused, never computed
                with pytest.raises(NotImplementedError):
                    call(Uploads(pa), *case.operands(0))
                continue
            _sweep(case, _entry(pa, case, call, lay, "wino2[" if lay == 3 else PLAN[lay]), label)
            plan = pa.hip.context().last_conv_plan()
            assert lay != 9 or ("16tiles" in plan) == (half == "1"), plan
            assert FAM.get(lay, "f2x2") == case.fam
            ran += 1
        monkeypatch.delenv("PLANER_HIP_EXPERIMENT", raising=False)
    assert ran >= 1


@pytest.mark.parametrize("name", ["chain_f4x4", "chain_wino43"])
def test_winograd_chains(pa, name):
    """Two 3x3 convs with the middle output transform and the next input transform in one kernel: y1, and through a second output
    stage the conv that reads the chain's V."""
    from planer_amd import q4
    case = CASES[name]
    if case.fam == "f4x4":
        prepare, win, gemm, chain, wout = q4.prepare_winograd4_q4_weights, q4.Wino4In, q4.Wino4Gemm, q4.Wino4Chain, q4.Wino4Out
        assert q4.wino4_chain_supported((case.xs[0], case.ks[0]) + case.xs[2:], pa.hip.context())
    else:
        prepare, win, gemm, chain, wout = q4.prepare_winograd43_q4_weights, q4.Wino43In, q4.Wino43Gemm, q4.Wino43Chain, q4.Wino43Out

    def call(up, ops, act):
        x, K, B, sc, sh, r, K2, sc2, sh2 = ops
        m = gemm(win(up(x, q4.to_q4, "q4")), up(K, prepare, name))
        y1, v2 = chain(m, up(B), up(sc), up(sh), _q4res(up, r), act=act, alpha=ALPHA)
        y2 = wout(gemm(v2, up(K2, prepare, name)), None, up(sc2), up(sh2), None, act=ACT_RELU)
        return [(y1, K.shape[0]), (y2, K2.shape[0])]
    _sweep(case, _entry(pa, case, call, 7 if case.fam == "f4x4" else 11, entry=name), name)


# ---- what the module reached ----------------------------------------------------------------------------------------------------------
def test_zz_every_family_was_planted(pa):
    """Runs last (file order): needs the whole module to have run.  Every w_layout of planer_amd/conv_layouts.py under at least one
    plant, and the plans a family could quietly refuse."""
    from planer_amd import conv_layouts
    plans, entries = SEEN["plans"], SEEN["entries"]
    print("w_layouts planted: %s; %d plants; %d plans" % (sorted(SEEN["layouts"]), SEEN["plants"], len(plans)))
    for p in sorted(plans):
        print("  plan", p)
    assert set(conv_layouts.LAYOUTS) <= SEEN["layouts"], sorted(set(conv_layouts.LAYOUTS) - SEEN["layouts"])
    numbers = [{k: int(v) for k, v in re.findall(r"(tiles|dp|split)=(\d+)", p)} for p in plans]
    assert any(n.get("split", 1) > 1 and n.get("dp", 0) == 0 for n in numbers), "no split-K plan"
    assert any(n.get("split", 1) > 1 and 0 < n.get("dp", 0) < n.get("tiles", 0) for n in numbers), "no hybrid plan"
    for prefix in ("smallcin3x3 ", "smallcin3x3valu", "dense32x32", "pair[", "wino2[", "wino4[", "wino43[", "w1d4 ", "wf4 ",
                   "depthwise-nchw", "depthwise-q4", "convt-q4", "stem+maxpool ", "stem+maxpool(nchw)", "conv1x1+wino4-in"):
        assert any(p.startswith(prefix) or (prefix == "smallcin3x3 " and p.startswith("smallcin3x3w ")) for p in plans), prefix
    assert any(p.startswith("wf4 ") and "16tiles" in p for p in plans) and any(p.startswith("wf4 ") and "16tiles" not in p for p in plans)
    assert {"dense-small", "dense-general", "chain_f4x4", "chain_wino43", "hybrid", "conv1x1+wino4-in"} <= entries, sorted(entries)

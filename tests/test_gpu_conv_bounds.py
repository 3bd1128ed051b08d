"""Convolution kernels on float data against the float64 reference (tests/ref64.py) element by element: |y - ref| <= bound(lam)
with the lam of the family's algorithm (ref64.LAMBDA: direct sums, F(2x2,3x3), F(4x4,3x3) staged / fused / chained, 1-D F(4,3),
mixed F(4,3) / F(3,3) tiles).  Operands that stress the kernels: per-channel magnitudes 2^U(-10, 6) on input channels, filters
and BN scales (negative included), inputs with a DC offset of 50, channels whose shift cancels the conv, real layer sizes.
Each case prints its worst err / tol (run with -s to collect them)."""
import zlib

import numpy as np
import pytest

from oracle import planer_np as onp
from tests import ref64 as R
from tests.test_gpu_wf4 import _patch_cells
from tests.ref64 import ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_RES_AFTER

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


ALPHA = 0.1
TAILS = [(True, True, True, ACT_RELU), (False, True, False, ACT_NONE), (True, True, True, ACT_LEAKY | ACT_RES_AFTER)]


def _dev(pa, a):
    return None if a is None else pa.asarray(np.ascontiguousarray(a))


def _operands(key, xs, ks, tail, dc=0.0, **conv):
    """Skewed float operands + tail; a quarter of the channels get the shift that cancels their mean conv output."""
    bias, bn, res, act = tail
    rng = np.random.default_rng(zlib.crc32(repr((key, xs, ks, tail, dc)).encode()))
    x, K, sc = R.skewed_operands(rng, xs, ks, dc=dc)
    cout = ks[0]
    B = (rng.standard_normal(cout) * 2.0 ** rng.uniform(-10, 6, cout)).astype(np.float32) if bias else None
    sh = None
    if bn:
        raw = R.conv64(x, K, B, **conv)
        sh = (rng.standard_normal(cout) * 2.0 ** rng.uniform(-10, 6, cout))
        cancel = rng.random(cout) < 0.25
        sh = np.where(cancel, -raw.mean(axis=(0, 2, 3)) * sc, sh).astype(np.float32)
    else:
        sc = None
    out = R.conv64(np.zeros(xs), np.zeros(ks), **conv).shape
    r = (rng.standard_normal(out) * 2.0 ** rng.uniform(-10, 6, (1, cout, 1, 1))).astype(np.float32) if res else None
    want = R.ref64(x, K, B, sc, sh, r, act, ALPHA, **conv)
    return (x, K, B, sc, sh, r), act, want


def _check(pa, y, ops, want, fam, what, label=None, tol=None, **conv):
    """check y against bound(LAMBDA[fam]) (or `tol`); prints the worst err / tol under the family label (default: fam)."""
    tol = R.bound(*ops, lam=R.LAMBDA[fam], **conv) if tol is None else tol
    plan = pa.hip.context().last_conv_plan()
    worst = R.check(y, want, tol, "%s %s" % (label or fam, what), plan)
    print("ratio %-15s %.3g  %s [%s]" % (label or fam, worst, what, plan))


# ---- direct families ----------------------------------------------------------------------------------------------------------
DIRECT = [("c256_14", (1, 256, 14, 14), (256, 256, 3, 3), dict(pads=[1, 1, 1, 1])),
          ("c512_7", (1, 512, 7, 7), (512, 512, 3, 3), dict(pads=[1, 1, 1, 1])),
          ("b32_c32_14", (32, 32, 14, 14), (64, 32, 3, 3), dict(pads=[1, 1, 1, 1])),
          ("c256_1x1_s2", (2, 256, 14, 14), (512, 256, 1, 1), dict(strides=[2, 2])),
          ] + [g for g in R.geometries() if g[0] in ("k1x7_s1x2", "k3x5_s2x1_d1x2", "g2_cin3_cout5", "draw5", "draw16")]


@pytest.mark.parametrize("geom", DIRECT, ids=[g[0] for g in DIRECT])
@pytest.mark.parametrize("dc", [0.0, 50.0], ids=["dc0", "dc50"])
def test_direct_nchw_and_q4(pa, geom, dc):
    from planer_amd import q4
    name, xs, ks, conv = geom
    conv = dict(dict(group=1, strides=[1, 1], dilations=[1, 1], pads=[0, 0, 0, 0]), **conv)
    for t, tail in enumerate(TAILS):
        ops, act, want = _operands(name, xs, ks, tail, dc, **conv)
        x, K, B, sc, sh, r = ops
        y = pa.ConvFused(_dev(pa, x), _dev(pa, K), _dev(pa, B), _dev(pa, sc), _dev(pa, sh), _dev(pa, r), act=act, alpha=ALPHA, **conv)
        _check(pa, y.get(), ops, want, "direct", "%s dc %g tail %d" % (name, dc, t), "nchw", **conv)
        if q4.q4_conv_eligible(ks, **conv):
            rq = q4.to_q4(_dev(pa, r)) if r is not None else None
            yq = q4.ConvQ4(q4.to_q4(_dev(pa, x)), q4.prepare_q4_weights(_dev(pa, K), conv["group"]), _dev(pa, B), _dev(pa, sc),
                           _dev(pa, sh), rq, act=act, alpha=ALPHA, **conv)
            _check(pa, q4.from_q4(yq).get(), ops, want, "direct", "%s dc %g tail %d" % (name, dc, t), "q4", **conv)


@pytest.mark.parametrize("c,k,s,d", [(32, (3, 3), (1, 1), (1, 1)), (144, (3, 5), (2, 1), (1, 2)), (5, (7, 7), (1, 1), (8, 8))])
def test_depthwise_nchw_and_q4(pa, c, k, s, d):
    from planer_amd import q4
    p = ((k[0] - 1) * d[0] // 2, (k[1] - 1) * d[1] // 2)
    conv = dict(group=c, strides=list(s), dilations=list(d), pads=[p[0], p[1], p[0], p[1]])
    xs, ks = (3, c, 17, 19), (c, 1) + k
    for t, tail in enumerate(TAILS):
        ops, act, want = _operands("dw", xs, ks, tail, **conv)
        x, K, B, sc, sh, r = ops
        y = pa.ConvFused(_dev(pa, x), _dev(pa, K), _dev(pa, B), _dev(pa, sc), _dev(pa, sh), _dev(pa, r), act=act, alpha=ALPHA, **conv)
        assert pa.hip.context().last_conv_plan().startswith("depthwise-nchw")
        _check(pa, y.get(), ops, want, "direct", "%s tail %d" % (xs, t), "depthwise-nchw", **conv)
        rq = q4.to_q4(_dev(pa, r)) if r is not None else None
        yq = q4.ConvQ4(q4.to_q4(_dev(pa, x)), q4.prepare_dw_q4_weights(_dev(pa, K)), _dev(pa, B), _dev(pa, sc), _dev(pa, sh), rq,
                       act=act, alpha=ALPHA, w_layout=13, **conv)
        assert pa.hip.context().last_conv_plan().startswith("depthwise-q4")
        _check(pa, q4.from_q4(yq).get(), ops, want, "direct", "%s tail %d" % (xs, t), "depthwise-q4", **conv)


# ---- the other direct entry points: forced tile configs, split-K, hybrid plans, tap-major, row-packed, stem + maxpool, small-Cin,
# the sibling pair, Dense, conv1x1 + Winograd-in ------------------------------------------------------------------------------
def _cfg_names(pa):
    from tests.test_gpu_layers import _cfg_names as names
    return names(pa)


def _full(conv):
    return dict(dict(group=1, strides=[1, 1], dilations=[1, 1], pads=[0, 0, 0, 0]), **conv)


DCS = pytest.mark.parametrize("dc", [0.0, 50.0], ids=["dc0", "dc50"])


@DCS
def test_forced_tile_configs_split_k_and_hybrid_plans(pa, dc):
    from planer_amd import q4
    ctx = pa.hip.context()
    names = _cfg_names(pa)
    conv = _full(dict(pads=[1, 1, 1, 1]))
    ops, act, want = _operands("cfg", (2, 32, 14, 14), (40, 32, 3, 3), TAILS[0], dc, **conv)
    x, K, B, sc, sh, r = ops
    dx, dK, dt = _dev(pa, x), _dev(pa, K), [_dev(pa, a) for a in (B, sc, sh, r)]
    dKt = pa.prepare_conv_weights(dK)
    xq, kq = q4.to_q4(dx), q4.prepare_q4_weights(dK)
    dtq = dt[:3] + [q4.to_q4(dt[3])]
    hops, hact, hwant = _operands("hybrid", (3, 64, 28, 28), (128, 64, 3, 3), TAILS[2], dc, **conv)
    hx, hK, hB, hsc, hsh, hr = hops
    hdK = _dev(pa, hK)
    hd = dict(B=_dev(pa, hB), scale=_dev(pa, hsc), shift=_dev(pa, hsh), res=_dev(pa, hr))
    hdx, hdKt = _dev(pa, hx), pa.prepare_conv_weights(hdK)
    try:
        for cfg, name in enumerate(names):
            for split in ((1,) if name.startswith("k") else (1, 2, 3)):
                ctx.set_conv_config(cfg, split)
                if name[0] in "qk":
                    y = q4.from_q4(q4.ConvQ4(xq, kq, *dtq, act=act, alpha=ALPHA, **conv)).get()
                    label = "q4-cfg"
                else:
                    tap = name.startswith("t")
                    y = pa.ConvFused(dx, dKt if tap else dK, *dt, act=act, alpha=ALPHA, w_layout=int(tap), **conv).get()
                    label = "tapmajor-cfg" if tap else "nchw-cfg"
                assert ctx.last_conv_plan().startswith(name + " "), (name, ctx.last_conv_plan())
                _check(pa, y, ops, want, "direct", "split %d dc %g" % (split, dc), label, **conv)
        for name, dp, split, occ in [("t64x64x16", 64, 6, 0), ("t128x64x16", 0, 9, 0), ("64x64", 0, 3, 0), ("t64x64x32", 32, 2, 4),
                                     ("128x32", 8, 5, 2)]:
            tap = name.startswith("t")
            ctx.set_conv_plan(names.index(name), dp, split, occ)
            y = pa.ConvFused(hdx, hdKt if tap else hdK, hd["B"], hd["scale"], hd["shift"], hd["res"], act=hact, alpha=ALPHA,
                             w_layout=int(tap), **conv)
            assert ctx.last_conv_plan().startswith(name + " "), ctx.last_conv_plan()
            _check(pa, y.get(), hops, hwant, "direct", "%s dp %d split %d dc %g" % (name, dp, split, dc), "hybrid", **conv)
    finally:
        ctx.set_conv_config(-1, 0)
    y = pa.ConvFused(dx, dKt, *dt, act=act, alpha=ALPHA, w_layout=1, **conv)
    _check(pa, y.get(), ops, want, "direct", "default plan dc %g" % dc, "tapmajor", **conv)


@DCS
def test_rowpack_and_stem_maxpool(pa, dc):
    from planer_amd import q4
    ctx = pa.hip.context()
    for xs, ks, conv in [((2, 3, 33, 35), (20, 3, 7, 7), dict(strides=[2, 2], pads=[3, 3, 3, 3])),
                         ((3, 2, 15, 17), (9, 2, 5, 5), dict(strides=[2, 2], pads=[2, 2, 2, 2])),
                         ((1, 3, 12, 40), (8, 3, 3, 5), dict(strides=[1, 2], pads=[0, 2, 0, 2]))]:
        conv = _full(conv)
        for t, tail in enumerate(TAILS):
            ops, act, want = _operands("rowpack", xs, ks, tail, dc, **conv)
            x, K, B, sc, sh, r = ops
            rq = q4.to_q4(_dev(pa, r)) if r is not None else None
            yq = q4.ConvQ4(_dev(pa, x), q4.prepare_rowpack_weights(_dev(pa, K)), _dev(pa, B), _dev(pa, sc), _dev(pa, sh), rq, act=act,
                           alpha=ALPHA, w_layout=6, **conv)
            _check(pa, q4.from_q4(yq).get(), ops, want, "direct", "%s dc %g tail %d" % (xs, dc, t), "rowpack", **conv)
    # stem + maxpool(3x3, s2, p1): max is 1-Lipschitz in the largest element, so the pooled tolerance is the pooled bound
    conv = _full(dict(strides=[2, 2], pads=[3, 3, 3, 3]))
    pool = dict(w=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2])
    for n, h, w, cout in [(2, 64, 64, 64), (1, 50, 36, 36)]:
        for t, tail in enumerate([(False, True, False, ACT_RELU), (True, True, False, ACT_LEAKY), (True, False, False, ACT_NONE)]):
            ops, act, want = _operands("stem", (n, 3, h, w), (cout, 3, 7, 7), tail, dc, **conv)
            x, K, B, sc, sh, _ = ops
            want = onp.maxpool(want, **pool)
            tol = onp.maxpool(R.bound(*ops, lam=R.LAMBDA["direct"], **conv), **pool)
            dx, dB, dsc, dsh = (_dev(pa, a) for a in (x, B, sc, sh))
            y = q4.ConvPoolQ4(dx, q4.prepare_rowpack_weights(_dev(pa, K)), dB, dsc, dsh, act=act, alpha=ALPHA, **conv)
            assert ctx.last_conv_plan().startswith("stem+maxpool "), ctx.last_conv_plan()
            _check(pa, q4.from_q4(y).get(), ops, want, "direct", "%s dc %g tail %d" % ((n, h, w, cout), dc, t), "stem+maxpool", tol)
            y = q4.ConvPoolQ4(dx, q4.prepare_stem_nchw_weights(_dev(pa, K)), dB, dsc, dsh, act=act, alpha=ALPHA, w_layout=12, **conv)
            assert ctx.last_conv_plan().startswith("stem+maxpool(nchw)"), ctx.last_conv_plan()
            _check(pa, q4.from_q4(y).get(), ops, want, "direct", "%s dc %g tail %d" % ((n, h, w, cout), dc, t), "stem+maxpool-nchw",
                   tol)


@DCS
def test_small_cin_mfma_and_valu(pa, dc, monkeypatch):
    ctx = pa.hip.context()
    for n, c, h, w, co in [(2, 3, 32, 32, 64), (1, 2, 17, 44, 70), (3, 1, 9, 16, 20)]:
        conv = _full(dict(pads=[1, 1, 1, 1]))
        ops, _, want = _operands("smallcin", (n, c, h, w), (co, c, 3, 3), (True, False, False, ACT_NONE), dc, **conv)
        x, K, B = ops[:3]
        args = (_dev(pa, x), _dev(pa, K), _dev(pa, B))
        for valu, label in (("0", "smallcin-mfma"), ("1", "smallcin-valu")):
            monkeypatch.setenv("PLANER_HIP_SMALLCIN", "1")
            monkeypatch.setenv("PLANER_HIP_SMALLCIN_VALU", valu)
            y = pa.Conv2d(*args, pads=conv["pads"]).get()
            plan = ctx.last_conv_plan()
            assert plan.startswith("smallcin3x3") and plan.startswith("smallcin3x3valu") == (valu == "1"), plan
            _check(pa, y, ops, want, "direct", "%s dc %g" % ((n, c, h, w, co), dc), label, **conv)


@DCS
def test_sibling_pair(pa, dc):
    from planer_amd import q4
    n, cin, h, w, cout, s = 4, 64, 14, 14, 128, 2
    c1 = _full(dict(strides=[s, s], pads=[1, 1, 1, 1]))
    c2 = _full(dict(strides=[s, s]))
    ops1, _, want1 = _operands("pair1", (n, cin, h, w), (cout, cin, 3, 3), (False, True, False, ACT_RELU), dc, **c1)
    x, K1, _, s1, t1, _ = ops1
    ops2, _, _ = _operands("pair2", (n, cin, h, w), (cout + 4, cin, 1, 1), (True, True, False, ACT_NONE), dc, **c2)
    ops2 = (x,) + ops2[1:]                                   # both convs read the same input
    want2 = R.ref64(*ops2, **c2)
    _, K2, b2, s2, t2, _ = ops2
    xq = q4.to_q4(_dev(pa, x))
    p1 = dict(strides=[s, s], pads=[1, 1, 1, 1], act=ACT_RELU, alpha=0.0)
    p2 = dict(strides=[s, s], pads=[0, 0, 0, 0], act=ACT_NONE, alpha=0.0)
    y1, y2 = q4.ConvQ4Pair(xq, q4.prepare_q4_weights(_dev(pa, K1)), None, _dev(pa, s1), _dev(pa, t1), q4.prepare_q4_weights(_dev(pa, K2)),
                           _dev(pa, b2), _dev(pa, s2), _dev(pa, t2), para1=p1, para2=p2)
    assert pa.hip.context().last_conv_plan().startswith("pair[")
    _check(pa, q4.from_q4(y1).get(), ops1, want1, "direct", "3x3 dc %g" % dc, "pair", **c1)
    _check(pa, q4.from_q4(y2).get(), ops2, want2, "direct", "1x1 dc %g" % dc, "pair", **c2)


@DCS
@pytest.mark.parametrize("mkn", [(32, 512, 1000), (64, 256, 40), (100, 77, 10), (65, 1024, 255)])
def test_dense_small_batch_and_general(pa, mkn, dc):
    """Dense as the 1x1 conv of a (m, k, 1, 1) input: the bound of that conv."""
    m, k, n = mkn
    ops, _, want = _operands("dense", (m, k, 1, 1), (n, k, 1, 1), (True, False, False, ACT_NONE), dc)
    x, W, B = ops[:3]
    y = pa.Dense(pa.asarray(x.reshape(m, k)), pa.asarray(W.reshape(n, k)), pa.asarray(B)).get()
    plan = pa.hip.context().last_conv_plan()
    small = m <= 64 and n >= 32 and k % 8 == 0
    assert ("dense32x32" in plan) == small, plan
    _check(pa, y.reshape(m, n, 1, 1), ops, want, "direct", "%s dc %g" % (mkn, dc), "dense-small" if small else "dense")


@DCS
@pytest.mark.parametrize("shape", [(2, 64, 14, 14, 64), (4, 32, 13, 13, 64)], ids=["64x14", "32x13"])
def test_conv1x1_winograd_in(pa, shape, dc):
    """V = B^T y B of the fused 1x1 conv's output y: the bound of y carried through |B^T| . |B|, plus 8u of |B^T| |y| |B| for the
    transform's own roundings (two passes of at most three rounded terms a row)."""
    from planer_amd import q4
    n, cin, h, w, cout = shape
    bt = np.abs(R._F[4][0])
    for t, tail in enumerate([(True, True, False, ACT_LEAKY), (False, True, False, ACT_RELU)]):
        ops, act, y = _operands("c1w", (n, cin, h, w), (cout, cin, 1, 1), tail, dc)
        x, K, B, sc, sh, _ = ops
        v = q4.Conv1x1WinoIn(q4.to_q4(_dev(pa, x)), q4.prepare_q4_weights(_dev(pa, K)), _dev(pa, B), _dev(pa, sc), _dev(pa, sh),
                             act=act, alpha=ALPHA, wino=4)
        assert pa.hip.context().last_conv_plan().startswith("conv1x1+wino4-in"), pa.hip.context().last_conv_plan()
        want = R.wino4_input(y)
        tol = R.wino4_input(R.bound(*ops), bt) + 8 * R.U * R.wino4_input(np.abs(y), bt)
        _check(pa, v.get()[:want.size].reshape(want.shape), ops, want, "direct", "%s dc %g tail %d" % (shape, dc, t),
               "conv1x1-wino-in", tol)


# ---- Winograd families -------------------------------------------------------------------------------------------------------
WINO = [(1, 256, 14, 14, 256), (1, 512, 7, 7, 512), (32, 32, 14, 14, 32), (2, 64, 28, 28, 64), (3, 16, 9, 13, 24), (1, 8, 21, 21, 8)]
PLAN = {2: "wino2[", 4: "wino2[", 7: "wino4[", 9: "wf4 ", 8: "w1d4 ", 11: "wino43["}
FAM = {2: "f2x2", 4: "f2x2", 7: "f4x4", 9: "f4x4", 8: "w1d4", 11: "wino43"}
LABEL = {4: "f2x2-q4", 7: "f4x4-staged", 9: "wf4", 8: "w1d4", 11: "wino43"}


@pytest.mark.parametrize("shape", WINO, ids=["x".join(map(str, s)) for s in WINO])
@pytest.mark.parametrize("dc", [0.0, 50.0], ids=["dc0", "dc50"])
def test_winograd_families(pa, shape, dc, monkeypatch):
    from planer_amd import q4
    n, cin, h, w, cout = shape
    conv = dict(pads=[1, 1, 1, 1])
    prep = {4: q4.prepare_winograd_q4_weights, 7: q4.prepare_winograd4_q4_weights, 9: q4.prepare_wf4_q4_weights,
            8: q4.prepare_w1d4_q4_weights, 11: q4.prepare_winograd43_q4_weights}
    wf4_runs = 0
    for t, tail in enumerate(TAILS):
        ops, act, want = _operands("wino", (n, cin, h, w), (cout, cin, 3, 3), tail, dc, **conv)
        x, K, B, sc, sh, r = ops
        dK, dt = _dev(pa, K), [_dev(pa, a) for a in (B, sc, sh)]
        xq, rq = q4.to_q4(_dev(pa, x)), (q4.to_q4(_dev(pa, r)) if r is not None else None)
        if cin % 16 == 0:
            y = pa.ConvFused(_dev(pa, x), pa.prepare_winograd_weights(dK), *dt, _dev(pa, r), act=act, alpha=ALPHA, w_layout=3, **conv)
            assert pa.hip.context().last_conv_plan().startswith("wino2[")
            _check(pa, y.get(), ops, want, "f2x2", "%s dc %g tail %d" % (shape, dc, t), "f2x2-nchw", **conv)
        for lay in (4, 7, 9, 8, 11):
            if lay == 11 and (h not in (7, 14, 21) or w not in (7, 14, 21)):
                continue
            for half in (("1", "0") if lay == 9 else ("",)):
                if half:
                    monkeypatch.setenv("PLANER_HIP_EXPERIMENT", "wf4_half=" + half)
                fits = lay != 9 or _patch_cells(h, w, 16 if half == "1" else 32) <= (512 if half == "1" else 1024)
                try:
                    if fits:
                        yq = q4.ConvQ4(xq, prep[lay](dK), *dt, rq, act=act, alpha=ALPHA, w_layout=lay, **conv)
                    else:
                        # the fused kernel declines patches beyond its LDS buffers (tests/test_gpu_wf4.py): refused, never computed
                        with pytest.raises(NotImplementedError):
                            q4.ConvQ4(xq, prep[lay](dK), *dt, rq, act=act, alpha=ALPHA, w_layout=lay, **conv)
                        continue
                finally:
                    monkeypatch.delenv("PLANER_HIP_EXPERIMENT", raising=False)
                plan = pa.hip.context().last_conv_plan()
                assert plan.startswith(PLAN[lay]), (lay, plan)
                if lay == 9:
                    assert ("16tiles" in plan) == (half == "1"), plan
                    wf4_runs += 1
                _check(pa, q4.from_q4(yq).get(), ops, want, FAM[lay], "%s dc %g tail %d" % (shape, dc, t),
                       LABEL[lay] + (" half=" + half if half else ""), **conv)
    assert wf4_runs > 0 or all(_patch_cells(h, w, tiles) > cells for tiles, cells in ((16, 512), (32, 1024))), shape


@pytest.mark.parametrize("shape", [(2, 64, 14, 14), (2, 128, 7, 7), (3, 32, 28, 28)], ids=["64x14", "128x7", "32x28"])
def test_winograd_chains(pa, shape):
    """Two 3x3 convs through the staged pipelines with the middle output transform and the next input transform in one
    kernel (Wino4Chain / Wino43Chain); each output inside its bound against the float64 reference of its own input."""
    from planer_amd import q4
    n, c, h, w = shape
    conv = dict(pads=[1, 1, 1, 1])
    ops1, act1, want1 = _operands("chain1", (n, c, h, w), (c, c, 3, 3), TAILS[0], 50.0, **conv)
    x, K1, B1, s1, t1, r1 = ops1
    stages = [("f4x4", q4.prepare_winograd4_q4_weights, q4.Wino4In, q4.Wino4Gemm, q4.Wino4Chain, q4.Wino4Out)]
    if h in (7, 14, 21):
        stages.append(("wino43", q4.prepare_winograd43_q4_weights, q4.Wino43In, q4.Wino43Gemm, q4.Wino43Chain, q4.Wino43Out))
    for fam, prep, win, gemm, chain, wout in stages:
        v = win(q4.to_q4(_dev(pa, x)))
        m = gemm(v, prep(_dev(pa, K1)))
        y1, v2 = chain(m, _dev(pa, B1), _dev(pa, s1), _dev(pa, t1), q4.to_q4(_dev(pa, r1)), act=act1, alpha=ALPHA)
        got1 = q4.from_q4(y1).get()
        _check(pa, got1, ops1, want1, fam, "first conv %s" % (shape,), fam + "-chain", **conv)
        # the second conv reads the chain's own first output (what the next layer sees)
        rng = np.random.default_rng(zlib.crc32(repr(("chain2", shape)).encode()))
        K2 = (rng.standard_normal((c, c, 3, 3)) / np.sqrt(9 * c)).astype(np.float32)
        sc2 = (rng.choice([-1.0, 1.0], c) * 2.0 ** rng.uniform(-10, 6, c)).astype(np.float32)
        sh2 = rng.standard_normal(c).astype(np.float32)
        y2 = wout(gemm(v2, prep(_dev(pa, K2))), None, _dev(pa, sc2), _dev(pa, sh2), None, act=ACT_RELU)
        ops2 = (got1, K2, None, sc2, sh2, None)
        _check(pa, q4.from_q4(y2).get(), ops2, R.ref64(*ops2, act=ACT_RELU, **conv), fam, "second conv %s" % (shape,),
               fam + "-chain", **conv)

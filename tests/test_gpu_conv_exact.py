"""Convolution kernels on integer operands (tests/ref64.py): every product and partial sum is an exact fp32 value whatever the
summation order, so every family whose arithmetic is exact must equal the float64 reference bit for bit -- the implicit GEMM
(NCHW, tap-major, channel-quad; every tile config, split-K, hybrid plans), row-packed, small-Cin, stem + maxpool, the sibling
pair, F(2x2,3x3), the exact stages of F(4x4,3x3), conv1x1 + Winograd-in, depthwise and Dense, under every fused tail with
negative BN scales and the residual before and after the activation.  Each case asserts the plan it expects, so a silent
fallback cannot pass for the family; a geometry a family refuses must raise NotImplementedError / ValueError."""
import re
import zlib

import numpy as np
import pytest

from oracle import planer_np as onp
from tests import ref64 as R
from tests.ref64 import ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_RES_AFTER

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


# (bias, scale / shift, residual, act)
TAILS = [(False, False, False, ACT_NONE), (True, False, False, ACT_NONE), (False, True, False, ACT_RELU),
         (True, True, True, ACT_RELU), (False, True, True, ACT_LEAKY | ACT_RES_AFTER), (True, True, False, ACT_LEAKY),
         (True, True, True, ACT_RELU | ACT_RES_AFTER), (False, False, True, ACT_LEAKY)]
GEOMS = R.geometries()


def _dev(pa, a):
    return None if a is None else pa.asarray(np.ascontiguousarray(a))


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _case(key, xs, ks, tail, **conv):
    """Integer operands and their float64 reference -> (host operands, act, want)."""
    bias, bn, res, act = tail
    ops = R.int_operands(np.random.default_rng(_seed(key, xs, ks, tail)), xs, ks, bias, bn, res, **conv)
    R.assert_exact(*ops, **conv)
    return ops, act, R.ref64(*ops, act=act, alpha=R.ALPHA, **conv)


def _exact(y, want, what, plan):
    y = np.asarray(y)
    assert y.shape == want.shape, (what, plan, y.shape, want.shape)
    np.testing.assert_array_equal(y.astype(np.float64), want, err_msg="%s [%s]" % (what, plan))


def _cfg_names(pa):
    from tests.test_gpu_layers import _cfg_names as names
    return names(pa)


# ---- NCHW implicit GEMM ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS, ids=[g[0] for g in GEOMS])
def test_nchw_conv_default_plan_every_tail(pa, geom):
    name, xs, ks, conv = geom
    ctx = pa.hip.context()
    for t, tail in enumerate(TAILS):
        (x, K, B, sc, sh, r), act, want = _case(name, xs, ks, tail, **conv)
        y = pa.ConvFused(_dev(pa, x), _dev(pa, K), _dev(pa, B), _dev(pa, sc), _dev(pa, sh), _dev(pa, r), act=act, alpha=R.ALPHA,
                         **conv)
        plan = ctx.last_conv_plan()
        dw = conv["group"] == xs[1] == ks[0]
        assert plan.startswith("depthwise-nchw") == dw, plan
        _exact(y.get(), want, "nchw %s tail %d" % (name, t), plan)


TILE_SHAPES = [((3, 32, 14, 14), (40, 32, 3, 3), dict(pads=[1, 1, 1, 1])),
               ((2, 3, 17, 19), (20, 3, 7, 7), dict(strides=[2, 2], pads=[3, 3, 3, 3])),
               ((2, 64, 7, 7), (70, 64, 1, 1), {}),
               ((2, 6, 9, 9), (10, 3, 3, 3), dict(group=2, strides=[2, 1], pads=[1, 1, 1, 1])),
               ((1, 15, 7, 8), (3, 5, 1, 3), dict(group=3, pads=[0, 1, 0, 1])),
               ((2, 64, 9, 9), (48, 32, 3, 3), dict(group=2, dilations=[2, 2], pads=[2, 2, 2, 2]))]


def _full(conv):
    return dict(dict(group=1, strides=[1, 1], dilations=[1, 1], pads=[0, 0, 0, 0]), **conv)


def test_nchw_every_tile_config_and_split_k(pa):
    """Every NCHW / tap-major tile config x split 1 / 2 / 3 x every tail (under split-K the tail runs in the reduce kernel)."""
    ctx = pa.hip.context()
    names = _cfg_names(pa)
    try:
        for xs, ks, conv in TILE_SHAPES:
            conv = _full(conv)
            cases = []
            for tail in TAILS:
                (x, K, B, sc, sh, r), act, want = _case("tiles", xs, ks, tail, **conv)
                dK = _dev(pa, K)
                dKt = pa.prepare_conv_weights(dK) if ks[1] % 16 == 0 and conv["group"] == 1 else None
                cases.append((_dev(pa, x), dK, dKt, [_dev(pa, a) for a in (B, sc, sh, r)], act, want))
            for cfg, name in enumerate(names):
                if name.startswith("q") or name.startswith("k"):
                    continue                  # channel-quad configs (the NCHW kernels run another config for them)
                tap = name.startswith("t")
                if tap and (cases[0][2] is None or ks[1] % int(name.split("x")[-1])):
                    continue
                for split in (1, 2, 3):
                    ctx.set_conv_config(cfg, split)
                    for t, (dx, dK, dKt, dt, act, want) in enumerate(cases):
                        y = pa.ConvFused(dx, dKt if tap else dK, *dt, act=act, alpha=R.ALPHA, w_layout=int(tap), **conv)
                        plan = ctx.last_conv_plan()
                        assert plan.startswith(name + " "), (name, plan)
                        _exact(y.get(), want, "cfg %s split %d %s tail %d" % (name, split, xs, t), plan)
    finally:
        ctx.set_conv_config(-1, 0)


def _plan_numbers(plan):
    """'<cfg> tiles=T dp=D split=S occ=O' -> {'tiles': T, 'dp': D, 'split': S, 'occ': O}"""
    return {k: int(v) for k, v in re.findall(r"(tiles|dp|split|occ)=(\d+)", plan)}


def test_hybrid_split_k_plans_and_tap_major(pa):
    """Hybrid plans (data-parallel prefix of dp tiles + split-K tail with the tile reduce): each plan string must show a real
    split-K tail (dp < tiles, split > 1) -- a dp at or above the tile count is clamped to a purely data-parallel launch."""
    ctx = pa.hip.context()
    names = _cfg_names(pa)
    conv = _full(dict(pads=[1, 1, 1, 1]))
    (x, K, B, sc, sh, r), act, want = _case("hybrid", (3, 64, 28, 28), (128, 64, 3, 3), (False, True, True, ACT_RELU), **conv)
    dx, dK, dsc, dsh, dr = (_dev(pa, a) for a in (x, K, sc, sh, r))
    dKt = pa.prepare_conv_weights(dK)
    try:
        for name, dp, split, occ in [("t64x64x16", 0, 4, 0), ("t64x64x16", 64, 6, 0), ("t128x64x16", 0, 9, 0),
                                     ("64x64", 0, 3, 0), ("t64x64x32", 32, 2, 4), ("128x32", 8, 5, 2)]:
            tap = name.startswith("t")
            ctx.set_conv_plan(names.index(name), dp, split, occ)
            y = pa.ConvFused(dx, dKt if tap else dK, None, dsc, dsh, dr, act=act, w_layout=int(tap), **conv)
            plan = ctx.last_conv_plan()
            assert plan.startswith(name + " "), plan
            got = _plan_numbers(plan)
            assert got["dp"] == dp < got["tiles"] and got["split"] > 1, plan
            _exact(y.get(), want, "hybrid %s dp%d s%d" % (name, dp, split), plan)
    finally:
        ctx.set_conv_config(-1, 0)
    # tap-major under its own default plan
    y = pa.ConvFused(dx, dKt, None, dsc, dsh, dr, act=act, w_layout=1, **conv)
    _exact(y.get(), want, "tap-major default", ctx.last_conv_plan())


# ---- channel-quad direct (w_layout 2) -------------------------------------------------------------------------------------
Q4_PLAN = re.compile(r"[qk]\d+x\d+x\d+ tiles=")        # a channel-quad tile config (conv_q4_kernel / conv_ks_kernel)


@pytest.mark.parametrize("geom", GEOMS, ids=[g[0] for g in GEOMS])
def test_q4_direct_default_plan_every_tail(pa, geom):
    from planer_amd import q4
    name, xs, ks, conv = geom
    ctx = pa.hip.context()
    for t, tail in enumerate(TAILS):
        (x, K, B, sc, sh, r), act, want = _case(name, xs, ks, tail, **conv)
        xq = q4.to_q4(_dev(pa, x))
        rq = q4.to_q4(_dev(pa, r)) if r is not None else None
        call = lambda: q4.ConvQ4(xq, q4.prepare_q4_weights(_dev(pa, K), conv["group"]), _dev(pa, B), _dev(pa, sc), _dev(pa, sh), rq,
                                 act=act, alpha=R.ALPHA, w_layout=2, **conv)
        if not q4.q4_conv_eligible(K.shape, **conv):
            with pytest.raises((NotImplementedError, ValueError)):
                call()
            return
        yq = call()
        plan = ctx.last_conv_plan()
        assert Q4_PLAN.match(plan), plan
        _exact(q4.from_q4(yq).get(), want, "q4 %s tail %d" % (name, t), plan)


def test_q4_direct_every_tile_config_and_split_k(pa):
    from planer_amd import q4
    ctx = pa.hip.context()
    names = _cfg_names(pa)
    qnames = [n for n in names if n.startswith("q") or n.startswith("k")]
    try:
        for xs, ks, conv in TILE_SHAPES + [((32, 16, 7, 7), (36, 16, 3, 3), dict(pads=[1, 1, 1, 1]))]:
            conv = _full(conv)
            if not q4.q4_conv_eligible(ks, **conv):
                continue
            cases = []
            for tail in TAILS:
                (x, K, B, sc, sh, r), act, want = _case("q4tiles", xs, ks, tail, **conv)
                dt = [_dev(pa, a) for a in (B, sc, sh)] + [q4.to_q4(_dev(pa, r)) if r is not None else None]
                cases.append((q4.to_q4(_dev(pa, x)), q4.prepare_q4_weights(_dev(pa, K), conv["group"]), dt, act, want))
            for name in qnames:
                for split in ((1,) if name.startswith("k") else (1, 2, 3)):
                    ctx.set_conv_config(names.index(name), split)
                    for t, (xq, kq, dt, act, want) in enumerate(cases):
                        yq = q4.ConvQ4(xq, kq, *dt, act=act, alpha=R.ALPHA, **conv)
                        plan = ctx.last_conv_plan()
                        assert plan.startswith(name + " "), (name, plan)
                        _exact(q4.from_q4(yq).get(), want, "q4 cfg %s split %d %s tail %d" % (name, split, xs, t), plan)
    finally:
        ctx.set_conv_config(-1, 0)


def test_same_image_alone_and_in_a_batch_of_32(pa):
    """Rows of a batch do not depend on their neighbours: on integer operands under the default plans (exact either way), and on
    float data under one pinned tile config without split-K (the same summation order at both batch sizes: bit-identical)."""
    from planer_amd import q4
    ctx = pa.hip.context()
    conv = _full(dict(pads=[1, 1, 1, 1]))
    (x, K, B, sc, sh, _), act, want = _case("batch32", (32, 24, 14, 14), (40, 24, 3, 3), (True, True, False, ACT_LEAKY), **conv)
    rng = np.random.default_rng(3)
    xf = rng.standard_normal(x.shape).astype(np.float32)
    names = _cfg_names(pa)
    dK, dt = _dev(pa, K), [_dev(pa, a) for a in (B, sc, sh)]
    nchw = lambda a: pa.ConvFused(_dev(pa, a), dK, *dt, act=act, alpha=R.ALPHA, **conv).get()
    quad = lambda a: q4.from_q4(q4.ConvQ4(q4.to_q4(_dev(pa, a)), q4.prepare_q4_weights(dK), *dt, act=act, alpha=R.ALPHA,
                                          **conv)).get()
    for form, run, cfg in (("nchw", nchw, "64x64"), ("q4", quad, "q64x64x16")):
        big = run(x)
        _exact(big, want, "%s batch 32" % form, ctx.last_conv_plan())
        try:
            ctx.set_conv_config(names.index(cfg), 1)
            bigf = run(xf)
            for i in (0, 17, 31):
                np.testing.assert_array_equal(run(x[i:i + 1].copy())[0], big[i])
                np.testing.assert_array_equal(run(xf[i:i + 1].copy())[0], bigf[i], err_msg="%s image %d" % (form, i))
        finally:
            ctx.set_conv_config(-1, 0)


# ---- row-packed, small-Cin, stem + maxpool, pair ------------------------------------------------------------------------------
ROWPACK = [((2, 3, 33, 35), (20, 3, 7, 7), dict(strides=[2, 2], pads=[3, 3, 3, 3])),
           ((1, 1, 20, 21), (6, 1, 3, 3), dict(pads=[1, 1, 1, 1])),
           ((3, 2, 15, 17), (9, 2, 5, 5), dict(strides=[2, 2], pads=[2, 2, 2, 2])),
           ((1, 3, 12, 40), (8, 3, 3, 5), dict(strides=[1, 2], pads=[0, 2, 0, 2])),
           ((1, 3, 9, 10), (5, 3, 1, 7), dict(strides=[2, 1], pads=[0, 3, 0, 3]))]


def test_rowpack_every_tail(pa):
    from planer_amd import q4
    ctx = pa.hip.context()
    for xs, ks, conv in ROWPACK:
        conv = _full(conv)
        assert q4.rowpack_eligible(ks, **conv)
        for t, tail in enumerate(TAILS):
            (x, K, B, sc, sh, r), act, want = _case("rowpack", xs, ks, tail, **conv)
            wq = q4.prepare_rowpack_weights(_dev(pa, K))
            rq = q4.to_q4(_dev(pa, r)) if r is not None else None
            yq = q4.ConvQ4(_dev(pa, x), wq, _dev(pa, B), _dev(pa, sc), _dev(pa, sh), rq, act=act, alpha=R.ALPHA, w_layout=6, **conv)
            plan = ctx.last_conv_plan()
            assert Q4_PLAN.match(plan), plan                    # the channel-quad kernel with the row-packed gather
            _exact(q4.from_q4(yq).get(), want, "rowpack %s tail %d" % (xs, t), plan)


def test_stem_conv_maxpool_every_entry(pa):
    """Row-packed stem + maxpool(3x3, s2, p1) (ConvPoolQ4) and its NCHW-reading form (w_layout 12): the max and the ReLU
    commute in the kernel, also under negative BN scales and leaky ReLU."""
    from planer_amd import q4
    ctx = pa.hip.context()
    conv = _full(dict(strides=[2, 2], pads=[3, 3, 3, 3]))
    pool = dict(w=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2])
    for n, h, w, cout in [(2, 64, 64, 64), (1, 50, 37, 36), (3, 30, 8, 8), (1, 33, 100, 12)]:
        for t, tail in enumerate([(False, True, False, ACT_RELU), (True, False, False, ACT_NONE), (False, True, False, ACT_LEAKY),
                                  (True, True, False, ACT_NONE)]):
            (x, K, B, sc, sh, _), act, want = _case("stem", (n, 3, h, w), (cout, 3, 7, 7), tail, **conv)
            want = onp.maxpool(want.astype(np.float32), **pool)            # exact values: the float32 pool is exact
            dx, dB, dsc, dsh = (_dev(pa, a) for a in (x, B, sc, sh))
            y = q4.ConvPoolQ4(dx, q4.prepare_rowpack_weights(_dev(pa, K)), dB, dsc, dsh, act=act, alpha=R.ALPHA, **conv)
            plan = ctx.last_conv_plan()
            assert plan.startswith("stem+maxpool "), plan
            _exact(q4.from_q4(y).get(), want, "stem+maxpool %s tail %d" % ((n, h, w, cout), t), plan)
            if w % 4 == 0:
                y = q4.ConvPoolQ4(dx, q4.prepare_stem_nchw_weights(_dev(pa, K)), dB, dsc, dsh, act=act, alpha=R.ALPHA, w_layout=12,
                                  **conv)
                plan = ctx.last_conv_plan()
                assert plan.startswith("stem+maxpool(nchw)"), plan
                _exact(q4.from_q4(y).get(), want, "stem+maxpool nchw %s tail %d" % ((n, h, w, cout), t), plan)


def test_small_cin_mfma_and_valu_kernels(pa, monkeypatch):
    ctx = pa.hip.context()
    conv_for = lambda pad: _full(dict(pads=[pad] * 4))
    for n, c, h, w, co, pad in [(2, 3, 9, 16, 20, 1), (1, 1, 5, 300, 70, 0), (3, 4, 17, 16, 64, 1), (2, 2, 40, 8, 130, 1),
                                (2, 3, 9, 14, 5, 0)]:
        conv = conv_for(pad)
        (x, K, B, _, _, _), _, want = _case("smallcin", (n, c, h, w), (co, c, 3, 3), (True, False, False, ACT_NONE), **conv)
        args = (_dev(pa, x), _dev(pa, K), _dev(pa, B))
        monkeypatch.setenv("PLANER_HIP_SMALLCIN", "1")
        monkeypatch.setenv("PLANER_HIP_SMALLCIN_VALU", "0")
        y = pa.Conv2d(*args, pads=conv["pads"]).get()
        plan = ctx.last_conv_plan()
        assert plan.startswith("smallcin3x3 ") or plan.startswith("smallcin3x3w "), plan
        _exact(y, want, "smallcin mfma %s" % ((n, c, h, w, co, pad),), plan)
        if (w - 2 + 2 * pad) % 4 == 0:                  # the vector-ALU kernel takes rows of whole pixel quads
            monkeypatch.setenv("PLANER_HIP_SMALLCIN_VALU", "1")
            for cpb in [""] + [str(c) for c in range(8, 65, 8)]:      # every block of 8..64 channels, partial last blocks included
                if cpb:
                    monkeypatch.setenv("PLANER_HIP_SCV_CPB", cpb)
                else:
                    monkeypatch.delenv("PLANER_HIP_SCV_CPB", raising=False)
                y = pa.Conv2d(*args, pads=conv["pads"]).get()
                plan = ctx.last_conv_plan()
                assert plan.startswith("smallcin3x3valu") and (not cpb or plan.endswith(" %sco" % cpb)), plan
                _exact(y, want, "smallcin valu cpb %s %s" % (cpb, (n, c, h, w, co, pad)), plan)
            monkeypatch.delenv("PLANER_HIP_SCV_CPB", raising=False)


@pytest.mark.parametrize("case", [(2, 8, 9, 11, 12, 2), (1, 6, 7, 7, 5, 3), (3, 16, 16, 16, 40, 2), (4, 64, 14, 14, 128, 2)])
def test_sibling_pair(pa, case):
    from planer_amd import q4
    n, cin, h, w, cout, s = case
    c1 = _full(dict(strides=[s, s], pads=[1, 1, 1, 1]))
    c2 = _full(dict(strides=[s, s]))
    (x, K1, _, s1, t1, _), _, want1 = _case("pair1", (n, cin, h, w), (cout, cin, 3, 3), (False, True, False, ACT_RELU), **c1)
    rng = np.random.default_rng(_seed("pair2", case))
    K2 = R.int_tensor(rng, (cout + 4, cin, 1, 1))
    b2, s2, t2, _ = R.int_tail(rng, cout + 4, None, True, True, False)
    want1 = R.ref64(x, K1, None, s1, t1, None, ACT_RELU, **c1)
    want2 = R.ref64(x, K2, b2, s2, t2, **c2)
    xq = q4.to_q4(_dev(pa, x))
    kq1, kq2 = q4.prepare_q4_weights(_dev(pa, K1)), q4.prepare_q4_weights(_dev(pa, K2))
    p1 = dict(strides=[s, s], pads=[1, 1, 1, 1], act=ACT_RELU, alpha=0.0)
    p2 = dict(strides=[s, s], pads=[0, 0, 0, 0], act=ACT_NONE, alpha=0.0)
    y1, y2 = q4.ConvQ4Pair(xq, kq1, None, _dev(pa, s1), _dev(pa, t1), kq2, _dev(pa, b2), _dev(pa, s2), _dev(pa, t2), para1=p1,
                           para2=p2)
    plan = pa.hip.context().last_conv_plan()
    assert plan.startswith("pair["), plan
    _exact(q4.from_q4(y1).get(), want1, "pair 3x3 %s" % (case,), plan)
    _exact(q4.from_q4(y2).get(), want2, "pair 1x1 %s" % (case,), plan)


# ---- Winograd: F(2x2,3x3) whole, F(4x4,3x3) stage by stage ---------------------------------------------------------------------
W2_SHAPES = [(2, 16, 14, 14, 8), (1, 64, 7, 7, 12), (3, 32, 9, 13, 6), (1, 256, 4, 4, 4), (2, 16, 1, 1, 4), (32, 16, 7, 7, 16)]


@pytest.mark.parametrize("shape", W2_SHAPES, ids=["x".join(map(str, s)) for s in W2_SHAPES])
def test_winograd_f2x2_nchw_and_q4(pa, shape):
    from planer_amd import q4
    n, cin, h, w, cout = shape
    ctx = pa.hip.context()
    conv = _full(dict(pads=[1, 1, 1, 1]))
    for t, tail in enumerate(TAILS):
        (x, K, B, sc, sh, r), act, want = _case("w2", (n, cin, h, w), (cout, cin, 3, 3), tail, **conv)
        R.winograd_f2_assert_exact(x, K, B, sc, sh, r)
        dK, dt = _dev(pa, K), [_dev(pa, a) for a in (B, sc, sh)]
        y = pa.ConvFused(_dev(pa, x), pa.prepare_winograd_weights(dK), *dt, _dev(pa, r), act=act, alpha=R.ALPHA, w_layout=3, **conv)
        plan = ctx.last_conv_plan()
        assert plan.startswith("wino2["), plan
        _exact(y.get(), want, "F(2x2) nchw %s tail %d" % (shape, t), plan)
        if cout % 4 == 0:
            rq = q4.to_q4(_dev(pa, r)) if r is not None else None
            yq = q4.ConvQ4(q4.to_q4(_dev(pa, x)), q4.prepare_winograd_q4_weights(dK), *dt, rq, act=act, alpha=R.ALPHA, w_layout=4,
                           **conv)
            plan = ctx.last_conv_plan()
            assert plan.startswith("wino2["), plan
            _exact(q4.from_q4(yq).get(), want, "F(2x2) q4 %s tail %d" % (shape, t), plan)


AT4 = R._F[4][2]


WIN_SHAPES = [(2, 8, 14, 14), (1, 12, 7, 7), (3, 4, 9, 13), (1, 20, 1, 1), (2, 64, 28, 28)]


@pytest.mark.parametrize("shape", WIN_SHAPES, ids=["x".join(map(str, s)) for s in WIN_SHAPES])
def test_wino4_input_and_output_stages(pa, shape):
    from planer_amd import q4
    n, c, h, w = shape
    rng = np.random.default_rng(_seed("w4", shape))
    ctx = pa.hip.context()
    x = R.int_tensor(rng, shape)
    v = q4.Wino4In(q4.to_q4(_dev(pa, x)))
    want = R.wino4_input(x)
    np.testing.assert_array_equal(v.get()[:want.size].reshape(want.shape), want, err_msg="Wino4In %s" % (shape,))
    # output stage: an integer M -> A^T M A + every tail
    th, tw = -(-h // 4), -(-w // 4)
    T = n * th * tw
    for t, (bias, bn, res, act) in enumerate(TAILS):
        m = rng.integers(-3, 4, (36, c // 4, T, 4)).astype(np.float32)
        B, sc, sh, r = R.int_tail(rng, c, (n, c, h, w), bias, bn, res)
        mt = m.reshape(6, 6, c // 4, n, th, tw, 4).transpose(3, 2, 6, 4, 5, 0, 1).reshape(n, c, th, tw, 6, 6)
        y = np.einsum("ia,nctuab,jb->nctiuj", AT4, mt.astype(np.float64), AT4).reshape(n, c, 4 * th, 4 * tw)[:, :, :h, :w]
        want = R.tail64(y, B, sc, sh, r, act, R.ALPHA)
        dm = q4._wino_tensor(n, c, h, w, ctx)
        host = np.zeros(dm.shape, np.float32)
        host[:m.size] = m.ravel()
        dm = pa.asarray(host)
        dm.meta = (n, c, h, w)
        rq = q4.to_q4(_dev(pa, r)) if r is not None else None
        got = q4.Wino4Out(dm, _dev(pa, B), _dev(pa, sc), _dev(pa, sh), rq, act=act, alpha=R.ALPHA)
        _exact(q4.from_q4(got).get(), want, "Wino4Out %s tail %d" % (shape, t), "")


@pytest.mark.parametrize("shape", [(2, 8, 14, 14, 16), (1, 16, 7, 7, 8), (3, 4, 9, 13, 12), (4, 32, 13, 13, 64)])
def test_conv1x1_winograd_in(pa, shape):
    from planer_amd import q4
    n, cin, h, w, cout = shape
    ctx = pa.hip.context()
    for t, tail in enumerate([(False, False, False, ACT_NONE), (True, True, False, ACT_LEAKY), (False, True, False, ACT_RELU)]):
        (x, K, B, sc, sh, _), act, y = _case("c1w", (n, cin, h, w), (cout, cin, 1, 1), tail)
        v = q4.Conv1x1WinoIn(q4.to_q4(_dev(pa, x)), q4.prepare_q4_weights(_dev(pa, K)), _dev(pa, B), _dev(pa, sc), _dev(pa, sh),
                             act=act, alpha=R.ALPHA, wino=4)
        plan = ctx.last_conv_plan()
        assert plan.startswith("conv1x1+wino4-in"), plan
        want = R.wino4_input(y)
        np.testing.assert_array_equal(v.get()[:want.size].reshape(want.shape), want, err_msg="%s tail %d [%s]" % (shape, t, plan))


# ---- depthwise -----------------------------------------------------------------------------------------------------------------------
def _dw(c, k, s=(1, 1), d=(1, 1), p=None, mult=1):
    kh, kw = k
    p = ((kh - 1) * d[0] // 2, (kw - 1) * d[1] // 2) if p is None else p
    return (c * mult, 1, kh, kw), dict(group=c, strides=list(s), dilations=list(d), pads=[p[0], p[1], p[0], p[1]])


# (x shape, K shape, conv, unstaged path expected)
DW = [((2, 1, 9, 10), *_dw(1, (3, 3)), False), ((1, 2, 11, 7), *_dw(2, (3, 5), (2, 1)), False),
      ((3, 3, 12, 13), *_dw(3, (5, 3), (1, 2), (2, 1)), False), ((1, 5, 8, 9), *_dw(5, (1, 7), (1, 3)), False),
      ((2, 1001, 5, 6), *_dw(1001, (3, 3), (2, 2)), False), ((1, 12, 13, 14), *_dw(12, (7, 2), (1, 1), (2, 1), (4, 0)), False),
      ((1, 8, 20, 20), *_dw(8, (7, 7), (1, 1), (16, 16)), True), ((2, 4, 12, 12), *_dw(4, (3, 3), (1, 1), (46, 46)), True),
      ((1, 6, 16, 17), *_dw(6, (7, 7), (1, 1), (8, 8)), False), ((1, 16, 9, 9), *_dw(16, (3, 3), (1, 1), (2, 3)), False),
      ((2, 5, 9, 8), *_dw(5, (3, 3), mult=2), False), ((1, 4, 7, 11), *_dw(4, (3, 3), (2, 2), mult=3), False)]


@pytest.mark.parametrize("case", DW, ids=["c%d_k%dx%d_s%d%d_d%d%d" % (c[0][1], c[1][2], c[1][3], *c[2]["strides"], *c[2]["dilations"])
                                          for c in DW])
def test_depthwise_nchw_and_q4(pa, case):
    from planer_amd import q4
    xs, ks, conv, unstaged = case
    ctx = pa.hip.context()
    mult = ks[0] // xs[1]
    for t, tail in enumerate(TAILS):
        (x, K, B, sc, sh, r), act, want = _case("dw", xs, ks, tail, **conv)
        y = pa.ConvFused(_dev(pa, x), _dev(pa, K), _dev(pa, B), _dev(pa, sc), _dev(pa, sh), _dev(pa, r), act=act, alpha=R.ALPHA,
                         **conv)
        plan = ctx.last_conv_plan()
        assert plan.startswith("depthwise-nchw") == (mult == 1), plan
        if mult == 1:
            assert plan.endswith(" unstaged") == unstaged, plan
        _exact(y.get(), want, "dw nchw %s tail %d" % (xs, t), plan)
        if mult > 1:
            continue
        rq = q4.to_q4(_dev(pa, r)) if r is not None else None
        call = lambda: q4.ConvQ4(q4.to_q4(_dev(pa, x)), q4.prepare_dw_q4_weights(_dev(pa, K)), _dev(pa, B), _dev(pa, sc), _dev(pa, sh),
                                 rq, act=act, alpha=R.ALPHA, w_layout=13, **conv)
        if not q4.dw_q4_eligible(ks, **conv):
            with pytest.raises((NotImplementedError, ValueError)):
                call()
            continue
        yq = call()
        plan = ctx.last_conv_plan()
        assert plan.startswith("depthwise-q4"), plan
        _exact(q4.from_q4(yq).get(), want, "dw q4 %s tail %d" % (xs, t), plan)


def test_depthwise_q4_unstaged_window(pa):
    from planer_amd import q4
    ks, conv = _dw(8, (7, 7), (1, 1), (8, 8))
    (x, K, B, sc, sh, r), act, want = _case("dwq4u", (2, 8, 16, 16), ks, (True, True, True, ACT_LEAKY | ACT_RES_AFTER), **conv)
    yq = q4.ConvQ4(q4.to_q4(_dev(pa, x)), q4.prepare_dw_q4_weights(_dev(pa, K)), _dev(pa, B), _dev(pa, sc), _dev(pa, sh),
                   q4.to_q4(_dev(pa, r)), act=act, alpha=R.ALPHA, w_layout=13, **conv)
    plan = pa.hip.context().last_conv_plan()
    assert plan.startswith("depthwise-q4") and plan.endswith(" unstaged"), plan
    _exact(q4.from_q4(yq).get(), want, "dw q4 unstaged", plan)


def test_depthwise_more_planes_than_the_grid_holds(pa):
    """NCHW with 70 000 channels takes the generic kernel (exact); Q4 with 65 536 channel quads is refused, never computed."""
    from planer_amd import q4
    ks, conv = _dw(70000, (3, 3))
    (x, K, B, sc, sh, r), act, want = _case("dw70k", (1, 70000, 1, 1), ks, (True, True, True, ACT_RELU), **conv)
    y = pa.ConvFused(_dev(pa, x), _dev(pa, K), _dev(pa, B), _dev(pa, sc), _dev(pa, sh), _dev(pa, r), act=act, **conv)
    plan = pa.hip.context().last_conv_plan()
    assert not plan.startswith("depthwise"), plan
    _exact(y.get(), want, "dw 70000 channels", plan)
    c = 262144
    ks, conv = _dw(c, (3, 3))
    xq = q4.to_q4(pa.asarray(np.ones((1, c, 1, 1), np.float32)))
    assert q4.dw_q4_eligible(ks, **conv)
    with pytest.raises(NotImplementedError):
        q4.ConvQ4(xq, q4.prepare_dw_q4_weights(pa.asarray(np.ones(ks, np.float32))), w_layout=13, **conv)


# ---- Dense ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mkn", [(1, 64, 32), (5, 72, 40), (64, 512, 1000), (33, 1024, 33), (65, 96, 255), (100, 77, 10),
                                 (2, 1000, 1031)])
def test_dense_small_batch_and_general(pa, mkn):
    m, k, n = mkn
    rng = np.random.default_rng(_seed("dense", mkn))
    x = rng.integers(-3, 4, (m, k)).astype(np.float32)
    W = rng.integers(-3, 4, (n, k)).astype(np.float32)
    B = rng.integers(-8, 9, n).astype(np.float32)
    want = x.astype(np.float64) @ W.T.astype(np.float64) + B
    y = pa.Dense(pa.asarray(x), pa.asarray(W), pa.asarray(B)).get()
    plan = pa.hip.context().last_conv_plan()
    assert ("dense32x32" in plan) == (m <= 64 and n >= 32 and k % 8 == 0), (plan, mkn)
    _exact(y, want, "dense %s" % (mkn,), plan)

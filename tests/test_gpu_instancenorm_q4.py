"""pl_instancenorm_q4_f32 and pad_q4 on the GPU (q4.InstanceNormQ4, q4.PadQ4; csrc/instnorm_q4_kernel.h).

The norm is held to the float64 reference and per-element bound of the NCHW kernel (tests/ref64_ops.py: instancenorm64,
instancenorm_bound, default LAM), at DC offsets 0, 50 and 1e3 -- the last one is where a one-pass E[x^2] - mean^2 variance leaves
the bound (3.7 times over at HW = 2049) while chunked centred sums merged by Chan's update stay inside it.  With a tail the
reference is relu(IN64(x) + res) and the bound grows by the one rounding of the addition, u |IN64(x) + res|; relu is exact and
1-Lipschitz, so it changes neither.  Pixel counts straddle both constants the header exports (P = one-workgroup limit, K = chunk):
every count up to P runs the one-workgroup kernel, P + 1 = 2K + 1 is three chunks with a single pixel in the last.
Run with -s for the worst err / bound per case."""
import zlib

import numpy as np
import pytest

from tests import ref64_ops as R
from tests.test_gpu_hygiene_sweep import POISONS, hygiene

pytestmark = pytest.mark.gpu

P, K = 4096, 2048           # PL_INSTNORM_Q4_ONE_WG_PIXELS, PL_INSTNORM_Q4_CHUNK_PIXELS (asserted against the library below)
# (H, W) per pixel count: 1, 63, 64, 65, K-1, K, K+1, P-1, P, P+1 = 2K+1, 3K-1, 3K, 3K+1, 4K+3 (S = 5); non-square, W odd
PLANES = [(1, 1), (7, 9), (8, 8), (5, 13), (23, 89), (32, 64), (3, 683), (65, 63), (64, 64), (17, 241), (6143, 1), (64, 96),
          (5, 1229), (5, 1639)]
CHANNELS = [1, 3, 4, 5, 8]
DCS = [0.0, 50.0, 1e3]
TAILS = [(False, 0), (True, 0), (False, 1), (True, 1)]          # (residual, act)


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def test_constants_are_the_headers(pa):
    import os
    import re
    from planer_amd import _lib
    text = open(os.path.join(os.path.dirname(_lib.HERE), "include", "planer_hip.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define PL_INSTNORM_Q4_(ONE_WG_PIXELS|CHUNK_PIXELS) (\d+)", text)}
    assert got == {"ONE_WG_PIXELS": P, "CHUNK_PIXELS": K}
    assert (_lib.INSTNORM_Q4_ONE_WG_PIXELS, _lib.INSTNORM_Q4_CHUNK_PIXELS) == (P, K) and P >= 56 * 56
    assert sorted(h * w for h, w in PLANES) == [1, 63, 64, 65, K - 1, K, K + 1, P - 1, P, P + 1, 3 * K - 1, 3 * K, 3 * K + 1, 4 * K + 3]
    assert 2 * K + 1 == P + 1


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _operands(xs, dc, res):
    rng = _rng("inq4", xs, dc, res)
    x = (rng.standard_normal(xs) * 2.0 ** rng.uniform(-10, 6, (xs[0], xs[1], 1, 1)) + dc).astype(np.float32)
    s = (rng.choice([-1, 1], xs[1]) * 2.0 ** rng.uniform(-10, 6, xs[1])).astype(np.float32)
    b = rng.standard_normal(xs[1]).astype(np.float32)
    r = rng.standard_normal(xs).astype(np.float32) if res else None
    return x, s, b, r


def _reference(x, s, b, r, act):
    """-> (float64 reference, per-element bound), both shaped like x."""
    n, c = x.shape[:2]
    rows = x.reshape(n * c, -1)
    sr, br = np.tile(s, n), np.tile(b, n)
    ref = R.instancenorm64(rows, sr, br).reshape(x.shape)
    tol = R.instancenorm_bound(rows, sr, br).reshape(x.shape)
    if r is not None:
        ref = ref + r.astype(np.float64)
        tol = tol + R.U * np.abs(ref)
    if act:
        ref = np.maximum(ref, 0.0)
    return ref, tol


def _run(pa, x, s, b, r, act):
    """-> (NCHW result, raw Q4 buffer) of InstanceNormQ4; asserts that it worked in place and which form ran."""
    q4 = pa.q4
    xq = q4.to_q4(pa.asarray(x))
    rq = q4.to_q4(pa.asarray(r)) if r is not None else None
    yq = q4.InstanceNormQ4(xq, pa.asarray(s), pa.asarray(b), rq, act=act)
    assert yq is xq
    hw = x.shape[2] * x.shape[3]
    want = "instnorm-q4 one-wg" if hw <= P else "instnorm-q4 chunks=%d" % -(-hw // K)
    assert xq.ctx.last_conv_plan() == want
    raw = xq.get()
    if r is not None:
        assert (rq.get() == q4.to_q4(pa.asarray(r)).get()).all()             # the residual is only read
    return q4.from_q4(xq).get(), raw


def _padding_is_plus_zero(raw, c):
    return c % 4 == 0 or not raw[:, -1, :, :, c % 4:].view(np.uint32).any()


@pytest.mark.parametrize("plane", PLANES, ids=["%dx%d" % p for p in PLANES])
def test_against_float64_within_the_bound(pa, plane):
    h, w = plane
    k = 0
    for c in CHANNELS:
        for n in (1, 3):
            for dc in DCS:
                res, act = TAILS[k % 4]
                k += 1
                x, s, b, r = _operands((n, c, h, w), dc, res)
                ref, tol = _reference(x, s, b, r, act)
                y, raw = _run(pa, x, s, b, r, act)
                what = "instnorm q4 %s dc=%g res=%d act=%d" % ((n, c, h, w), dc, res, act)
                print("%-60s worst err/tol %.3f" % (what, R.check(y, ref, tol, what)))
                assert _padding_is_plus_zero(raw, c), what


@pytest.mark.parametrize("plane", [(5, 13), (64, 64), (17, 241), (5, 1639)], ids=["65", "P", "P+1", "4K+3"])
def test_every_tail_in_place_with_zero_padding_lanes(pa, plane):
    h, w = plane
    for c in (3, 8, 5):
        for res, act in TAILS:
            for dc in DCS:
                x, s, b, r = _operands((3, c, h, w), dc, res)
                ref, tol = _reference(x, s, b, r, act)
                y, raw = _run(pa, x, s, b, r, act)
                what = "tail res=%d act=%d %s dc=%g" % (res, act, (3, c, h, w), dc)
                print("%-60s worst err/tol %.3f" % (what, R.check(y, ref, tol, what)))
                assert _padding_is_plus_zero(raw, c), what
                if act:
                    assert (y[ref < -tol] == 0).all(), what


@pytest.mark.parametrize("plane", [(8, 8), (64, 64), (17, 241), (5, 1639)], ids=["64", "P", "P+1", "4K+3"])
def test_batch_rows_are_independent_and_runs_repeat(pa, plane):
    h, w = plane
    for c in (5, 8):
        for res, act in ((False, 0), (True, 1)):
            x, s, b, r = _operands((3, c, h, w), 50.0, res)
            y, raw = _run(pa, x, s, b, r, act)
            again, raw2 = _run(pa, x, s, b, r, act)
            assert (raw.view(np.uint32) == raw2.view(np.uint32)).all(), "two runs differ"
            alone, _ = _run(pa, x[1:2], s, b, None if r is None else r[1:2], act)
            assert (alone.view(np.uint32) == y[1:2].view(np.uint32)).all(), "row 1 of a batch of 3 != that image alone"


@pytest.mark.parametrize("plane", [(5, 13), (17, 241)], ids=["one-wg", "chunks"])
def test_a_nan_stays_in_its_plane(pa, plane):
    h, w = plane
    x, s, b, _ = _operands((2, 8, h, w), 0.0, False)
    clean = x.copy()
    x[1, 1, h // 2, w - 1] = np.nan
    y, _ = _run(pa, x, s, b, None, 0)
    assert np.isnan(y[1, 1]).all()
    keep = np.ones(y.shape, bool)
    keep[1, 1] = False
    assert not np.isnan(y[keep]).any()
    ref, tol = _reference(clean, s, b, None, 0)
    R.check(np.where(keep, y, 0), np.where(keep, ref, 0), tol, "neighbours of the NaN plane")


@pytest.mark.parametrize("plane", [(64, 64), (17, 241)], ids=["one-wg", "chunks"])
def test_under_pool_hygiene(pa, plane):
    """Every fresh block poisoned and guarded (the statistics scratch block included): the result may not depend on bytes nobody
    wrote, and nothing outside the blocks' payloads may change."""
    h, w = plane
    x, s, b, r = _operands((2, 5, h, w), 50.0, True)
    ref, tol = _reference(x, s, b, r, 1)
    base, _ = _run(pa, x, s, b, r, 1)
    for poison in POISONS:
        with hygiene(poison):
            y, raw = _run(pa, x, s, b, r, 1)
        R.check(y, ref, tol, "hygiene %#x" % poison)
        assert (y.view(np.uint32) == base.view(np.uint32)).all() and _padding_is_plus_zero(raw, 5)


def test_empty_tensors_make_no_launch(pa, monkeypatch):
    from planer_amd import _lib
    q4 = pa.q4
    s, b = pa.asarray(np.ones(5, np.float32)), pa.asarray(np.zeros(5, np.float32))
    empties = [q4.to_q4(pa.asarray(np.zeros(xs, np.float32))) for xs in ((0, 5, 4, 4), (2, 5, 0, 4), (2, 5, 3, 0))]
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for xq in empties:
        assert q4.InstanceNormQ4(xq, s, b, act=1) is xq
    assert calls == []
    x = np.ones((1, 5, 2, 2), np.float32)
    q4.InstanceNormQ4(q4.to_q4(pa.asarray(x)), s, b)
    assert "pl_instancenorm_q4_f32" in calls
    monkeypatch.undo()
    # the entry point itself: nothing to do is not an error; a bad activation code is
    xq = q4.to_q4(pa.asarray(x))
    _lib.call("pl_instancenorm_q4_f32", xq.ctx.handle, xq.ptr, s.ptr, b.ptr, None, 0, 5, 4, 1e-5, 0)
    _lib.call("pl_instancenorm_q4_f32", xq.ctx.handle, xq.ptr, s.ptr, b.ptr, None, 1, 5, 0, 1e-5, 0)
    assert (q4.from_q4(xq).get() == x).all()
    with pytest.raises(ValueError):
        q4.InstanceNormQ4(xq, s, b, act=2)
    with pytest.raises(ValueError):
        q4.InstanceNormQ4(xq, pa.asarray(np.ones(4, np.float32)), b)


# ---- pad -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["reflect", "edge", "symmetric", "wrap", "constant"])
def test_pad_q4_is_np_pad_bit_for_bit(pa, mode):
    q4 = pa.q4
    for c, value in ((3, 0.0), (8, -2.5)):
        for (h, w), (pt, pl, pb, pr) in (((5, 7), (1, 2, 3, 0)), ((3, 4), (7, 9, 8, 6)), ((6, 1), (0, 3, 2, 5)), ((9, 9), (4, 4, 4, 4))):
            x = _rng("pad", c, h, w).standard_normal((2, c, h, w)).astype(np.float32)
            pads = np.array([0, 0, pt, pl, 0, 0, pb, pr], np.int64)
            kw = {"constant_values": value} if mode == "constant" else {}
            want = np.pad(x, ((0, 0), (0, 0), (pt, pb), (pl, pr)), mode=mode, **kw)
            yq = q4.PadQ4(q4.to_q4(pa.asarray(x)), pads, constant_value=value, mode=mode)
            assert q4.is_q4(yq) and q4.logical_shape(yq) == want.shape
            got = q4.from_q4(yq).get()
            assert (got.view(np.uint32) == want.view(np.uint32)).all(), (mode, c, (h, w), (pt, pl, pb, pr))
            assert _padding_is_plus_zero(yq.get(), c)
            # ... and equals the NCHW operator
            assert (pa.layer.Pad(pa.asarray(x), pads, constant_value=value, mode=mode).get() == got).all()
    x3 = q4.to_q4(pa.asarray(np.ones((1, 3, 2, 2), np.float32)))
    with pytest.raises(ValueError):
        q4.PadQ4(x3, np.array([0, 0, 1, 1, 0, 0, 1, 1], np.int64), constant_value=2.5)      # would dirty the padding lane
    with pytest.raises(ValueError):
        q4.PadQ4(x3, np.array([0, 1, 1, 1, 0, 0, 1, 1], np.int64))                          # channel padding

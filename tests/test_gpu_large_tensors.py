"""Kernels on the far side of their 32-bit boundaries: tensors of 2 GiB (byte offsets past 2^31), 4 GiB (byte offsets past 2^32)
and more than 2^29 / 2^30 elements, on a real MI355X.  Every other GPU test works on a few MB, while the library changes code
path at these sizes in dozens of places (csrc/: every guard at 1 << 29 / 30 / 31 / 32 and every switch keyed on a byte count).

Conventions
* integer operands (tests/ref64.py): every sum is an exact fp32 value, so each comparison is equality, no tolerance;
* host data is one block of PERIOD = 8191 integers (a prime: no factor in common with any row, plane or image stride) tiled over
  a 4 GiB source, with distinctive values at its first and last elements and on both sides of byte offsets 2^31 and 2^32; the
  tests read prefixes of it (`src[:n]`) and the device copy is uploaded once;
* each case names the branch it reaches ("reaches:") -- flipping that branch's index type to int, or removing the switch, makes
  the case fail;
* device memory: the shared 4 GiB source plus one case's tensors; the pool is trimmed after every test and the largest
  reservation seen is checked against 12 GiB at the end.

Findings these cases record ("Size limits"):
* depthwise, NCHW (layer.Conv2d): the limits are conv_launch's -- input below 2^29 elements, output below 2^31.  An input of
  2^29 elements is refused with NotImplementedError (the guard stands before the depthwise kernel, so there is no fall-through
  to the generic kernel at that size); an output of 2^29 elements from a smaller input runs on conv_dw_kernel
  ("depthwise-nchw" in last_conv_plan) and is right.  Depthwise, Q4 (pl_conv2d_dw_q4_f32): input and output below 2^29
  elements, NotImplementedError above.  A Net with such a layer raises the same NotImplementedError when it is first called;
* the Winograd entry points refuse once the transformed input V reaches 2^29 elements (an input of 2^27 elements); called
  directly (layer.ConvFused / q4.ConvQ4 with a Winograd w_layout) that is a NotImplementedError before anything is allocated,
  launched or written.  A Net that picks its conv algorithm by timing skips the candidates that refuse and computes the conv
  right; a Net with that algorithm forced (PLANER_HIP_CONV_ALGO) raises NotImplementedError when it is first called.
"""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PERIOD = 8191
E29, E30 = 1 << 29, 1 << 30                 # element offsets of byte offsets 2^31 and 2^32
SRC_ELEMS = 130 << 23                       # 4.06 GiB: room for the largest case (129 * 2^23 floats)
MARK = np.array([5, -6, 7, -5], np.float32)
PEAK = [0]
GIB = float(1 << 30)


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    ctx = planer_amd.hip.context()
    ctx.trim()
    yield planer_amd
    gc.collect()
    ctx.trim()


@pytest.fixture(scope="module")
def big(pa):
    """(host source, its device copy): SRC_ELEMS integers in [-3, 3] of period 8191, marked at the 32-bit boundaries."""
    rng = np.random.default_rng(2031)
    block = rng.integers(-3, 4, PERIOD).astype(np.float32)
    src = np.tile(block, SRC_ELEMS // PERIOD + 1)[:SRC_ELEMS]
    for at in (0, E29, E30, SRC_ELEMS):
        lo = max(at - 4, 0)
        hi = min(at + 4, SRC_ELEMS)
        src[lo:hi] = np.resize(MARK, hi - lo)
    dsrc = pa.hip.empty((SRC_ELEMS,))
    dsrc.set(src)
    src.setflags(write=False)
    yield src, dsrc
    del dsrc


@pytest.fixture(autouse=True)
def _trim_after_each_test(pa):
    # a device fault is sticky: the rest of the module would only pile launches onto a faulted GPU, so the session ends here
    try:
        pa.hip.context().synchronize()
    except pa._lib.HipBackendError as e:
        pytest.exit("the device reported a fault before this test: %s" % e, returncode=3)
    yield
    gc.collect()
    ctx = pa.hip.context()
    PEAK[0] = max(PEAK[0], ctx.pool_stats()[0])
    ctx.trim()


def dview(pa, dsrc, shape, offset=0, chan=None):
    """A device tensor of `shape` that aliases the shared source from element `offset` on."""
    n = int(np.prod(shape, dtype=np.int64))
    assert offset + n <= SRC_ELEMS and offset % 4 == 0
    v = pa.hip.DeviceArray(shape, np.float32, dsrc.ctx, dsrc.ptr + 4 * offset, dsrc)
    v.chan = chan
    return v


def hview(src, shape, offset=0):
    n = int(np.prod(shape, dtype=np.int64))
    return src[offset:offset + n].reshape(shape)


def assert_same(got, want, what):
    """Equality of two large host arrays, chunk by chunk; the first mismatch is reported by flat index and byte offset."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g = np.ascontiguousarray(got).reshape(-1)
    w = np.ascontiguousarray(want).reshape(-1)
    step = 1 << 26
    for lo in range(0, g.size, step):
        a, b = g[lo:lo + step], w[lo:lo + step]
        if not np.array_equal(a, b):
            i = lo + int(np.flatnonzero(a != b)[0])
            raise AssertionError("%s: first mismatch at element %d (byte offset %d = 2^%.3f): got %r, want %r; %d of %d differ in this chunk"
                                 % (what, i, 4 * i, np.log2(max(4 * i, 1)), g[i], w[i], int((a != b).sum()), a.size))


def q4_host(x):
    """(N, C, H, W) -> (N, ceil(C/4), H, W, 4), zero padded."""
    n, c, h, w = x.shape
    cq = (c + 3) // 4
    out = np.zeros((n, cq, h, w, 4), x.dtype)
    for q in range(cq):
        k = min(4, c - 4 * q)
        out[:, q, :, :, :k] = x[:, 4 * q:4 * q + k].transpose(0, 2, 3, 1)
    return out


def cfg_index(pa, name):
    lib = pa._lib.load()
    for c in range(lib.pl_conv2d_num_configs()):
        buf = ctypes.create_string_buffer(32)
        lib.pl_conv2d_config_name(c, buf, 32)
        if buf.value.decode() == name:
            return c
    raise KeyError(name)


# ---- 1. Q4 implicit GEMM, output of 2 GiB and more: the pointer-addressed store tail -------------------------------------------
H1 = W1 = 2048
HW1 = H1 * W1


def conv1x1_q4_ref(xq, K):
    """1x1 conv of a host Q4 tensor (N, Cq, HW, 4) with K (Cout, Cin) -> Q4 (N, Coq, HW, 4), float32 (exact on integers)."""
    n, cq, hw, _ = xq.shape
    cout, cin = K.shape
    coq = (cout + 3) // 4
    Kp = np.zeros((coq * 4, cq * 4), np.float32)
    Kp[:cout, :cin] = K
    out = np.empty((n, coq, hw, 4), np.float32)
    for i in range(n):
        for o in range(coq):
            acc = xq[i, 0] @ Kp[4 * o:4 * o + 4, 0:4].T
            for q in range(1, cq):
                acc += xq[i, q] @ Kp[4 * o:4 * o + 4, 4 * q:4 * q + 4].T
            out[i, o] = acc
    return out


def tail_q4(base, cout, B=None, scale=None, shift=None, res=None, act=0, alpha=0.0, res_post=False):
    """The fused tail in apply_epilogue's order on a host Q4 tensor (N, Coq, HW, 4); padding lanes stay zero."""
    n, coq = base.shape[:2]

    def lanes(v):
        p = np.zeros(coq * 4, np.float32)
        p[:cout] = v
        return p.reshape(1, coq, 1, 4)
    y = base.copy()
    if B is not None:
        y += lanes(B)
    if scale is not None:
        y *= lanes(scale)
    if shift is not None:
        y += lanes(shift)
    if res is not None and not res_post:
        y += res
    if act == 1:
        np.maximum(y, 0, out=y)
    elif act == 2:
        y *= ((y > 0) * np.float32(1.0 - alpha) + np.float32(alpha)).astype(np.float32)
    if res is not None and res_post:
        y += res
    if cout % 4:
        y[:, -1, :, cout % 4:] = 0
    return y


class TestQ4ConvPointerTail:
    """x Q4 (2, 4, 2048, 2048), K (66, 4, 1, 1): Coq = 17, the output is 2.125 GiB, so conv_launch sets y_bytes = 0 and
    store_tile_q4 takes its pointer-addressed tail with unsigned quad indices ("ptrtail" in last_conv_plan).  The twin with
    Cout = 60 (1.875 GiB) must stay on the buffer-descriptor tail.  Cout = 66 also has a partial last quad."""

    @pytest.fixture(scope="class")
    def ops(self, pa, big):
        from planer_amd import q4
        src, dsrc = big
        rng = np.random.default_rng(66)
        x = hview(src, (2, 4, H1, W1))
        xq_h = np.ascontiguousarray(x.reshape(2, 4, HW1).transpose(0, 2, 1)).reshape(2, 1, HW1, 4)
        K = rng.integers(-3, 4, (66, 4)).astype(np.float32)
        K[5] = 0
        base = conv1x1_q4_ref(xq_h, K)
        # the residual: a legitimate Q4 tensor (zero padding lanes) whose values differ from the conv's input
        res_h = hview(src, (2, 17, HW1, 4), offset=1 << 25).copy()
        res_h[:, 16, :, 2:] = 0
        xq = q4.to_q4(dview(pa, dsrc, (2, 4, H1, W1)))
        resq = pa.hip.empty((2, 17, H1, W1, 4))
        resq.set(res_h.reshape(resq.shape))
        resq.chan = 66
        B = rng.integers(-8, 9, 66).astype(np.float32)
        sc = rng.choice(np.array([-4.0, -2.0, -1.0, -0.5, 0.5, 1.0, 2.0, 4.0]), 66).astype(np.float32)
        sh = (rng.integers(-16, 17, 66) * 0.25).astype(np.float32)
        yield dict(xq=xq, xq_h=xq_h, K=K, base=base, res_h=res_h, resq=resq, B=B, sc=sc, sh=sh)

    def run(self, pa, ops, cout, **tail):
        from planer_amd import q4
        K = ops["K"][:cout]
        kq = q4.prepare_q4_weights(pa.asarray(K.reshape(cout, 4, 1, 1)))
        dev = {k: (None if v is None else pa.asarray(v[:cout])) for k, v in
               (("B", tail.get("B")), ("scale", tail.get("scale")), ("shift", tail.get("shift")))}
        yq = q4.ConvQ4(ops["xq"], kq, dev["B"], dev["scale"], dev["shift"], tail.get("resq"), act=tail.get("act", 0),
                       alpha=tail.get("alpha", 0.0))
        plan = pa.hip.context().last_conv_plan()
        return yq.get().reshape(2, (cout + 3) // 4, HW1, 4), plan

    def test_bias_relu_above_2gib_takes_the_pointer_tail(self, pa, ops):
        """reaches: store_tile_q4's second tail (y_bytes == 0), `idx` as unsigned quad index, partial last quad."""
        got, plan = self.run(pa, ops, 66, B=ops["B"], act=1)
        assert "ptrtail" in plan, plan
        assert_same(got, tail_q4(ops["base"], 66, B=ops["B"], act=1), "bias + relu, Cout 66")

    def test_scale_shift_residual_leaky_above_2gib(self, pa, ops):
        """reaches: the pointer tail's residual read res4[idx] past byte offset 2^31."""
        got, plan = self.run(pa, ops, 66, scale=ops["sc"], shift=ops["sh"], resq=ops["resq"], act=2, alpha=0.125)
        assert "ptrtail" in plan, plan
        want = tail_q4(ops["base"], 66, scale=ops["sc"], shift=ops["sh"], res=ops["res_h"], act=2, alpha=0.125)
        assert_same(got, want, "scale + shift + residual + leaky, Cout 66")

    def test_residual_after_the_activation_above_2gib(self, pa, ops):
        """reaches: the pointer tail with res_post (ACT_RES_AFTER)."""
        got, plan = self.run(pa, ops, 66, B=ops["B"], resq=ops["resq"], act=1 | 16)
        assert "ptrtail" in plan, plan
        assert_same(got, tail_q4(ops["base"], 66, B=ops["B"], res=ops["res_h"], act=1, res_post=True), "res_post, Cout 66")

    def test_twin_below_2gib_keeps_the_buffer_tail(self, pa, ops):
        """reaches: the buffer-descriptor tail with a byte count just under 2^31 (1.875 GiB)."""
        got, plan = self.run(pa, ops, 60, B=ops["B"], act=1)
        assert "ptrtail" not in plan, plan
        assert_same(got, tail_q4(ops["base"][:, :15], 60, B=ops["B"][:60], act=1), "bias + relu, Cout 60")

    def test_nchw_layout0_output_above_2_29_elements(self, pa, ops, big):
        """The same conv through layer.ConvFused on NCHW tensors (w_layout 0): 2 * 66 * 2^22 = 5.5e8 outputs >= 2^29.
        reaches: the generic kernel's size_t output index and its residual read res[idx] past byte offset 2^31, with the fused
        bias + residual + relu."""
        src, dsrc = big
        K = ops["K"]
        roff = 3 << 25
        y = pa.ConvFused(dview(pa, dsrc, (2, 4, H1, W1)), pa.asarray(K.reshape(66, 4, 1, 1)), pa.asarray(ops["B"]),
                         res=dview(pa, dsrc, (2, 66, H1, W1), offset=roff), act=1)
        plan = pa.hip.context().last_conv_plan()
        assert "smallcin" not in plan and "depthwise" not in plan, plan
        got = y.get().reshape(2, 66, HW1)
        want, res = tail_q4(ops["base"], 66, B=ops["B"]), hview(src, (2, 66, HW1), offset=roff)
        for n in range(2):
            for c in range(66):
                if not np.array_equal(got[n, c], np.maximum(want[n, c // 4, :, c % 4] + res[n, c], 0)):
                    raise AssertionError("layout 0: image %d channel %d differs (plan %s)" % (n, c, plan))


def test_q4_conv_split_k_reduce_above_2gib(pa, big):
    """A forced split-K plan on the tiles at the END of a 2.125 GiB output, so reduce_tiles_q4_kernel writes past byte offset 2^31.
    Cin = 20 instead of the 4 of the cases above: with K = 4 there is a single K chunk and effective_splits() turns every split-K
    request into an unsplit pass, so the reduce kernel would not run at all.
    reaches: reduce_tiles_q4_kernel's size_t idx4 / residual read, next to the data-parallel pointer tail in one output."""
    from planer_amd import q4
    src, dsrc = big
    ctx = pa.hip.context()
    rng = np.random.default_rng(20)
    xq_h = hview(src, (2, 5, HW1, 4))
    K = rng.integers(-3, 4, (66, 20)).astype(np.float32)
    base = conv1x1_q4_ref(xq_h, K)
    res_h = hview(src, (2, 17, HW1, 4), offset=1 << 28).copy()
    res_h[:, 16, :, 2:] = 0
    resq = pa.hip.empty((2, 17, H1, W1, 4))
    resq.set(res_h.reshape(resq.shape))
    resq.chan = 66
    sc = rng.choice(np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]), 66).astype(np.float32)
    sh = (rng.integers(-16, 17, 66) * 0.25).astype(np.float32)
    kq = q4.prepare_q4_weights(pa.asarray(K.reshape(66, 20, 1, 1)))
    xq = dview(pa, dsrc, (2, 5, H1, W1, 4), chan=20)
    tiles = 2 * (2 * HW1 // 64)                       # q64x64x16: two row tiles, 2^17 column tiles
    try:
        ctx.set_conv_plan(cfg_index(pa, "q64x64x16"), tiles - 1024, 2)
        yq = q4.ConvQ4(xq, kq, None, pa.asarray(sc), pa.asarray(sh), resq, act=2, alpha=0.125)
        plan = ctx.last_conv_plan()
    finally:
        ctx.set_conv_config(-1, 0)
    assert "tiles=%d dp=%d split=2" % (tiles, tiles - 1024) in plan and "ptrtail" in plan, plan
    want = tail_q4(base, 66, scale=sc, shift=sh, res=res_h, act=2, alpha=0.125)
    assert_same(yq.get().reshape(2, 17, HW1, 4), want, "split-K tail of a 2.125 GiB output")


# ---- 2. Q4 conv, input just under / at 2^31 bytes ---------------------------------------------------------------------------------
def test_q4_conv_input_just_under_2gib(pa, big):
    """x Q4 (2, 124, 1024, 2048) is 1.94 GiB: x_bytes = 2 080 374 784 < 2^31, the largest input the gather's buffer descriptor
    takes.  reaches: the input gather at byte offsets just below 2^31 (an int offset would still fit; a wrong x_bytes would not)."""
    from planer_amd import q4
    src, dsrc = big
    hw = 1024 * 2048
    xq_h = hview(src, (2, 31, hw, 4))
    K = np.random.default_rng(124).integers(-3, 4, (4, 124)).astype(np.float32)
    want = conv1x1_q4_ref(xq_h, K)
    yq = q4.ConvQ4(dview(pa, dsrc, (2, 31, 1024, 2048, 4), chan=124), q4.prepare_q4_weights(pa.asarray(K.reshape(4, 124, 1, 1))))
    assert_same(yq.get().reshape(2, 1, hw, 4), want, "Q4 conv, 1.94 GiB input")


def test_q4_conv_input_of_2gib_is_refused(pa, big):
    """(2, 128, 1024, 2048) is 2^29 input elements: the public layer API raises NotImplementedError with the guard's text."""
    from planer_amd import q4
    src, dsrc = big
    K = np.ones((4, 128, 1, 1), np.float32)
    with pytest.raises(NotImplementedError, match="input/filter above 2 GiB"):
        q4.ConvQ4(dview(pa, dsrc, (2, 32, 1024, 2048, 4), chan=128), q4.prepare_q4_weights(pa.asarray(K)))
    with pytest.raises(NotImplementedError, match="input/filter above 2 GiB"):
        pa.Conv2d(dview(pa, dsrc, (2, 128, 1024, 2048)), pa.asarray(K))


# ---- 3. small-Cin 3x3 routing at 2^29 outputs ------------------------------------------------------------------------------------
def conv3x3_rows(x, K, B, r0, r1):
    """Rows [r0, r1) of the 3x3 / pad 1 conv of one image x (C, H, W) with K (Cout, C, 3, 3) + B, by shifted sums (float32)."""
    c, h, w = x.shape
    xp = np.zeros((c, r1 - r0 + 2, w + 2), np.float32)
    lo, hi = max(r0 - 1, 0), min(r1 + 1, h)
    xp[:, lo - (r0 - 1):hi - (r0 - 1), 1:w + 1] = x[:, lo:hi]
    out = np.zeros((K.shape[0], r1 - r0, w), np.float32)
    for dy in range(3):
        for dx in range(3):
            out += np.tensordot(K[:, :, dy, dx], xp[:, dy:dy + r1 - r0, dx:dx + w], axes=([1], [0]))
    return out + B.reshape(-1, 1, 1)


@pytest.mark.parametrize("cout, small", [(64, False), (60, True)])
def test_smallcin_3x3_routing_at_2_29_outputs(pa, big, cout, small):
    """(2, 3, 2048, 2048) -> cout channels, 3x3 / pad 1.  cout = 64 gives exactly 2^29 outputs and must leave the small-Cin
    kernels (their y_bytes is a 32-bit count) for the generic one; cout = 60 (1.875 GiB) must stay on them.
    Checked two ways: an independent numpy reference on three row bands of every channel (the first rows, the rows on both
    sides of the image boundary -- byte offset 2^31 for cout = 64 -- and the last rows), and whole-tensor equality with the
    same layer called per image (below the boundary, vouched for by the float64 suite).
    reaches: `out_elems < 2^29` of both small-Cin branches of conv_launch; the generic kernel's stores past 2^31 bytes."""
    src, dsrc = big
    ctx = pa.hip.context()
    rng = np.random.default_rng(cout)
    K = rng.integers(-3, 4, (cout, 3, 3, 3)).astype(np.float32)
    B = rng.integers(-8, 9, cout).astype(np.float32)
    x = hview(src, (2, 3, H1, W1))
    dK, dB = pa.asarray(K), pa.asarray(B)
    y = pa.Conv2d(dview(pa, dsrc, (2, 3, H1, W1)), dK, dB, pads=[1, 1, 1, 1])
    plan = ctx.last_conv_plan()
    assert ("smallcin" in plan) is small, plan
    got = y.get()
    del y
    for n, r0, r1 in ((0, 0, 3), (0, H1 - 3, H1), (1, 0, 3), (1, H1 - 3, H1)):
        assert_same(got[n, :, r0:r1], conv3x3_rows(x[n], K, B, r0, r1), "image %d rows %d..%d (plan %s)" % (n, r0, r1, plan))
    for n in range(2):
        yi = pa.Conv2d(dview(pa, dsrc, (1, 3, H1, W1), offset=n * 3 * HW1), dK, dB, pads=[1, 1, 1, 1])
        assert "smallcin" in ctx.last_conv_plan(), ctx.last_conv_plan()
        assert_same(got[n:n + 1], yi.get(), "image %d against the per-image call (plan %s)" % (n, plan))
        del yi


# ---- 4. depthwise and 5. Winograd: refusals ----------------------------------------------------------------------------------------
def test_depthwise_of_2_29_elements_is_refused_not_misrouted(pa, big):
    """A depthwise 3x3 conv on (2, 64, 2048, 2048) = 2^29 elements.  Finding: both entry points refuse.  The Q4 one
    (pl_conv2d_dw_q4_f32) has its own guard; the NCHW one never reaches the depthwise kernel's fall-through to the generic
    kernel, because conv_launch's guard (input below 2^29 elements) stands before both.  Nothing is launched."""
    from planer_amd import q4
    src, dsrc = big
    K = np.ones((64, 1, 3, 3), np.float32)
    with pytest.raises(NotImplementedError, match="input/filter above 2 GiB"):
        pa.Conv2d(dview(pa, dsrc, (2, 64, H1, W1)), pa.asarray(K), group=64, pads=[1, 1, 1, 1])
    kq = q4.prepare_dw_q4_weights(pa.asarray(K))
    with pytest.raises(NotImplementedError, match="pl_conv2d_dw_q4_f32: tensor above 2 GiB"):
        q4.ConvQ4(dview(pa, dsrc, (2, 16, H1, W1, 4), chan=64), kq, group=64, pads=[1, 1, 1, 1], w_layout=13)


def dw3x3_rows(x, K, B, pad, r0, r1):
    """Rows [r0, r1) of the depthwise 3x3 conv (pad `pad`, stride 1) of one image x (C, H, W) with K (C, 3, 3) + B, float32."""
    c, h, w = x.shape
    xp = np.zeros((c, r1 - r0 + 2, w + 2 * pad), np.float32)
    lo, hi = max(r0 - pad, 0), min(r1 + 2 - pad, h)
    xp[:, lo - (r0 - pad):hi - (r0 - pad), pad:pad + w] = x[:, lo:hi]
    wo = w + 2 * pad - 2
    out = np.zeros((c, r1 - r0, wo), np.float32)
    for dy in range(3):
        for dx in range(3):
            out += K[:, dy, dx].reshape(c, 1, 1) * xp[:, dy:dy + r1 - r0, dx:dx + wo]
    return out + B.reshape(-1, 1, 1)


def test_depthwise_nchw_output_of_2_29_elements_runs_on_the_depthwise_kernel(pa, big):
    """(2, 64, 2046, 2046), depthwise 3x3 / pad 2 -> (2, 64, 2048, 2048): the input is under conv_launch's 2^29-element guard,
    the output is exactly 2^29 elements, and dw_launch has no size guard of its own, so conv_dw_kernel<float, 3, 3> stores past
    byte offset 2^31.  Checked like the other 3x3 cases: numpy on row bands of every channel (first rows, both sides of the
    image boundary = byte offset 2^31, last rows) and whole-tensor equality with the per-image calls.
    reaches: conv_dw_kernel's `yp = y + plane * Ho * Wo` and apply_epilogue's flat index past 2^29 elements."""
    src, dsrc = big
    ctx = pa.hip.context()
    rng = np.random.default_rng(64)
    K = rng.integers(-3, 4, (64, 1, 3, 3)).astype(np.float32)
    B = rng.integers(-8, 9, 64).astype(np.float32)
    h = 2046
    x = hview(src, (2, 64, h, h))
    dK, dB = pa.asarray(K), pa.asarray(B)
    y = pa.Conv2d(dview(pa, dsrc, (2, 64, h, h)), dK, dB, group=64, pads=[2, 2, 2, 2])
    plan = ctx.last_conv_plan()
    assert "depthwise-nchw" in plan, plan
    assert y.shape == (2, 64, 2048, 2048) and y.size == E29
    got = y.get()
    del y
    for n, r0, r1 in ((0, 0, 3), (0, 2045, 2048), (1, 0, 3), (1, 2045, 2048)):
        assert_same(got[n, :, r0:r1], dw3x3_rows(x[n], K[:, 0], B, 2, r0, r1), "image %d rows %d..%d (plan %s)" % (n, r0, r1, plan))
    for n in range(2):
        yi = pa.Conv2d(dview(pa, dsrc, (1, 64, h, h), offset=n * 64 * h * h), dK, dB, group=64, pads=[2, 2, 2, 2])
        assert "depthwise-nchw" in ctx.last_conv_plan(), ctx.last_conv_plan()
        assert_same(got[n:n + 1], yi.get(), "image %d against the per-image call (plan %s)" % (n, plan))
        del yi


def one_conv_net(pa, K, B, group, pads):
    """A Net of one conv layer (the reference's json / flow IR)."""
    from planer_amd.irgen.builder import GraphBuilder
    g = GraphBuilder(["x"])
    g.init("K", K)
    g.init("B", B)
    g.op("conv", ["x", "K", "B"], "y", name="conv", group=group, strides=[1, 1], dilations=[1, 1], pads=list(pads))
    return pa.from_graph(*g.finish(["y"]))


def test_net_with_a_depthwise_layer_of_2_29_elements_raises(pa, big):
    """The same refusal through a compiled plan: a Net of one depthwise conv called on (2, 64, 2048, 2048).  No route of the plan
    compiler (NCHW or Q4 depthwise) may produce a plan that runs a kernel at that size; the call raises NotImplementedError."""
    src, dsrc = big
    net = one_conv_net(pa, np.ones((64, 1, 3, 3), np.float32), np.zeros(64, np.float32), 64, [1, 1, 1, 1])
    with pytest.raises(NotImplementedError, match="above 2 GiB"):
        net(dview(pa, dsrc, (2, 64, H1, W1)))


def test_net_skips_the_winograd_candidates_that_refuse(pa, big):
    """A Net of one 3x3 / pad 1 conv on (2, 16, 2048, 2048), algorithm picked by timing (Net._pick_conv_algo): the Winograd
    candidates whose V passes their guard raise NotImplementedError and are skipped, the plan computes the conv with what is
    left, and the result equals numpy on row bands of every channel."""
    src, dsrc = big
    rng = np.random.default_rng(7)
    K = rng.integers(-3, 4, (16, 16, 3, 3)).astype(np.float32)
    B = rng.integers(-8, 9, 16).astype(np.float32)
    net = one_conv_net(pa, K, B, 1, [1, 1, 1, 1])
    y = net(dview(pa, dsrc, (2, 16, H1, W1)))
    got = y.get()
    assert got.shape == (2, 16, H1, W1)
    x = hview(src, (2, 16, H1, W1))
    for n, r0, r1 in ((0, 0, 2), (0, 1023, 1025), (0, H1 - 2, H1), (1, 0, 2), (1, H1 - 2, H1)):
        assert_same(got[n, :, r0:r1], conv3x3_rows(x[n], K, B, r0, r1), "net: image %d rows %d..%d" % (n, r0, r1))
    # the input the caller handed in is untouched
    assert_same(dview(pa, dsrc, (1 << 20,)).get(), src[:1 << 20], "net input")


def test_net_with_a_forced_winograd_algorithm_raises(pa, big, monkeypatch):
    """PLANER_HIP_CONV_ALGO=3 (F(2x2,3x3) on NCHW; PLANER_HIP_Q4=0 keeps the plan on NCHW so that the code applies) on the same
    conv: a forced algorithm is not tried first, so the refusal surfaces as NotImplementedError when the plan is built."""
    src, dsrc = big
    monkeypatch.setenv("PLANER_HIP_Q4", "0")
    monkeypatch.setenv("PLANER_HIP_CONV_ALGO", "3")
    K = np.ones((16, 16, 3, 3), np.float32)
    net = one_conv_net(pa, K, np.zeros(16, np.float32), 1, [1, 1, 1, 1])
    assert net.force_algo == 3
    with pytest.raises(NotImplementedError, match="winograd: tensor too large"):
        net(dview(pa, dsrc, (2, 16, H1, W1)))


def test_winograd_refusal_writes_nothing(pa, big):
    """The raw entry point with a Winograd filter layout and a pre-filled output: PL_EUNSUPPORTED, and the output is unchanged."""
    src, dsrc = big
    lib = pa._lib.load()
    ctx = pa.hip.context()
    n = 2 * 16 * HW1
    y = dview(pa, dsrc, (n,), offset=n).copy()
    U = pa.prepare_winograd_weights(pa.asarray(np.ones((16, 16, 3, 3), np.float32)))
    rc = lib.pl_conv2d_fused_f32(ctx.handle, dsrc.ptr, 2, 16, H1, W1, U.ptr, 16, 3, 3, None, y.ptr, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                 None, None, None, 0, 0.0, 3)
    assert rc == pa._lib.PL_EUNSUPPORTED, (rc, lib.pl_last_error())
    ctx.synchronize()
    assert_same(y.get(), src[n:2 * n], "output of the refused call")


def test_winograd_refuses_when_v_reaches_2_29_elements(pa, big):
    """3x3 / stride 1 / pad 1 on (2, 16, 2048, 2048): the Winograd-domain input V = 16 * Cin * tiles is 2^29 elements, the
    guard of winograd_launch / winograd_q4_launch.  Forced (a Winograd w_layout) the call raises before it allocates V or
    launches; unforced the direct kernel computes the conv, checked on row bands against numpy."""
    from planer_amd import q4
    src, dsrc = big
    ctx = pa.hip.context()
    rng = np.random.default_rng(5)
    K = rng.integers(-3, 4, (16, 16, 3, 3)).astype(np.float32)
    B = rng.integers(-8, 9, 16).astype(np.float32)
    dx = dview(pa, dsrc, (2, 16, H1, W1))
    before = ctx.pool_stats()[0]
    with pytest.raises(NotImplementedError, match="winograd: tensor too large"):
        pa.ConvFused(dx, pa.prepare_winograd_weights(pa.asarray(K)), pa.asarray(B), pads=[1, 1, 1, 1], w_layout=3)
    with pytest.raises(NotImplementedError, match="winograd: tensor too large"):
        q4.ConvQ4(dview(pa, dsrc, (2, 4, H1, W1, 4), chan=16), q4.prepare_winograd_q4_weights(pa.asarray(K)), pa.asarray(B),
                  pads=[1, 1, 1, 1], w_layout=4)
    # only the outputs the layers allocate before the call (2 x 512 MiB) and the small filters: no V, no M
    assert ctx.pool_stats()[0] - before < (1 << 30) + (64 << 20)
    y = pa.Conv2d(dx, pa.asarray(K), pa.asarray(B), pads=[1, 1, 1, 1])
    plan = ctx.last_conv_plan()
    got = y.get()
    x = hview(src, (2, 16, H1, W1))
    for n, r0, r1 in ((0, 0, 2), (0, 1023, 1025), (1, H1 - 2, H1)):
        assert_same(got[n, :, r0:r1], conv3x3_rows(x[n], K, B, r0, r1), "direct conv rows %d..%d (plan %s)" % (r0, r1, plan))


# ---- 6. Q4 max-pool 3x3 / stride 2 / pad 1 -----------------------------------------------------------------------------------------
def maxpool_k3s2p1_q4_ref(x):
    """util.pool's max on a host Q4 tensor (N, Cq, H, W, 4): zero padding, accumulator starts at -1e4 (as onp.maxpool)."""
    n, cq, h, w, _ = x.shape
    ho, wo = (h + 2 - 3 + 2) // 2, (w + 2 - 3 + 2) // 2
    out = np.full((n, cq, ho, wo, 4), -1e4, np.float32)
    for dy in range(3):
        for dx in range(3):
            # output (i, j) reads input (2i + dy - 1, 2j + dx - 1); outside the map the tap is the zero padding
            i0 = 1 if dy == 0 else 0
            j0 = 1 if dx == 0 else 0
            i1 = min(ho, (h - dy) // 2 + 1)
            j1 = min(wo, (w - dx) // 2 + 1)
            sub = out[:, :, i0:i1, j0:j1]
            np.maximum(sub, x[:, :, 2 * i0 + dy - 1:2 * (i1 - 1) + dy:2, 2 * j0 + dx - 1:2 * (j1 - 1) + dx:2], out=sub)
            for edge in (out[:, :, :i0], out[:, :, i1:], out[:, :, :, :j0], out[:, :, :, j1:]):
                np.maximum(edge, 0, out=edge)
    return out


@pytest.mark.parametrize("c", [64, 60])
def test_q4_maxpool_k3s2p1_at_2_27_quads(pa, big, c):
    """Input Q4 (2, c, 2048, 2048).  c = 64 is 2^27 quads (2 GiB): pl_pool2d_q4_f32 leaves maxpool_q4_k3s2p1_2x1, whose buffer
    descriptor counts bytes in 32 bits, for the generic kernel; c = 60 stays on the 2x1 kernel with a byte count just under
    2^31 (1.875 GiB) and int byte offsets `(base + hi * W + wi) << 4` just under 2^31.
    reaches: the `< 2^27` switch; the 2x1 kernel's largest offsets; pool2d_q4_kernel's size_t reads past 2^31 bytes."""
    from planer_amd import q4
    src, dsrc = big
    cq = c // 4
    y = q4.MaxpoolQ4(dview(pa, dsrc, (2, cq, H1, W1, 4), chan=c), (3, 3), (1, 1, 1, 1), (2, 2))
    got = y.get()
    del y
    assert_same(got, maxpool_k3s2p1_q4_ref(hview(src, (2, cq, H1, W1, 4))), "Q4 maxpool 3x3 s2 p1, C = %d" % c)


# ---- 7. layout conversion -------------------------------------------------------------------------------------------------------------
def test_q4_layout_conversion_above_1gib(pa, big):
    """to_q4 / from_q4 on (2, 66, 2048, 1024): 2.77e8 elements (1.03 GiB NCHW, 1.06 GiB Q4), partial last quad.  The kernels
    index quads in 32 bits and every float offset in size_t, so their first boundary is the guard itself (2^29 quads = 8 GiB,
    which the guard's message now states); this is the largest shape that is cheap to check in both directions.
    reaches: `src[3 * (size_t)HW]` / `dst[...]` plane offsets and the float4 index past 2^30 bytes."""
    from planer_amd import q4
    src, dsrc = big
    shape = (2, 66, 2048, 1024)
    x = hview(src, shape)
    xq = q4.to_q4(dview(pa, dsrc, shape))
    want = q4_host(x)
    assert_same(xq.get(), want, "to_q4")
    back = q4.from_q4(xq)
    assert_same(back.get(), x, "from_q4(to_q4(x))")
    del back, xq
    # from_q4 on its own, from a Q4 tensor that numpy laid out
    dq = pa.hip.empty(want.shape)
    dq.set(want)
    dq.chan = 66
    assert_same(q4.from_q4(dq).get(), x, "from_q4")


# ---- 8. pointwise and data movement, one case per loop family -------------------------------------------------------------------

def test_add_and_leakyrelu_above_2_29_elements(pa, big):
    """reaches: the size_t loops of add_vec4 / unary_vec4 (float4 index, byte offsets past 2^31) and their scalar remainders
    (n % 4 = 3)."""
    src, dsrc = big
    n = E29 + 4099
    a, b = dview(pa, dsrc, (n,)), dview(pa, dsrc, (n,), offset=PERIOD // 4 * 4)
    assert_same(pa.Add(a, b).get(), src[:n] + src[PERIOD // 4 * 4:PERIOD // 4 * 4 + n], "Add")
    x = src[:n]
    assert_same(pa.LeakyReLU(a, 0.125).get(), x * ((x > 0) * np.float32(0.875) + np.float32(0.125)), "LeakyReLU")


@pytest.mark.parametrize("elems", [E29, E30], ids=["2^29", "2^30"])
def test_binary_channel_broadcast(pa, big, elems):
    """Mul by one value per channel (pl_binary_f32, b_mode 1) on (2, 5, inner) with 10 * inner just over `elems`.
    reaches: binary_kernel's size_t i with FastDiv on (unsigned)i; at 2^30 elements y[i] / a[i] pass byte offset 2^32."""
    src, dsrc = big
    inner = elems // 10 + 7
    shape = (2, 5, inner)
    s = np.array([2, -1, 0.5, 4, -2], np.float32).reshape(1, 5, 1)
    y = pa.Mul(dview(pa, dsrc, shape), pa.asarray(s))
    assert_same(y.get(), hview(src, shape) * s, "Mul by channel")


@pytest.mark.parametrize("shape, form", [((2, 5, E29 // 10 + 1027), "plane"), ((2, E29 // 1022 + 1, 511), "flat")])
def test_batchnorm_both_forms_above_2_29_elements(pa, big, shape, form):
    """BatchNorm through affine_plane (inner >= 1024, few planes: one block row per plane, now an unsigned counter) and
    through affine_flat (inner < 1024: size_t loop, FastDiv on (unsigned)i).
    reaches: `x + (size_t)plane * inner` past 2^31 bytes / the flat index past 2^29."""
    src, dsrc = big
    c = shape[1]
    rng = np.random.default_rng(c)
    k = rng.choice(np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]), c).astype(np.float32).reshape(1, c, 1)
    b = (rng.integers(-16, 17, c) * 0.25).astype(np.float32).reshape(1, c, 1)
    y = pa.BatchNorm(dview(pa, dsrc, shape), pa.asarray(k), pa.asarray(b))
    assert_same(y.get(), hview(src, shape) * k + b, "BatchNorm (%s)" % form)


@pytest.mark.parametrize("elems", [E29, E30], ids=["2^29", "2^30"])
def test_transpose(pa, big, elems):
    """(A, 3, 1031) -> (3, A, 1031) with just over `elems` elements (rows stay contiguous, so numpy's copy is quick).  reaches: transpose_kernel's unsigned i and size_t src;
    at 2^30 elements both y[i] and x[src] pass byte offset 2^32."""
    src, dsrc = big
    a = elems // (3 * 1031) + 1
    shape = (a, 3, 1031)
    y = pa.Transpose(dview(pa, dsrc, shape), [1, 0, 2])
    assert_same(y.get(), hview(src, shape).transpose(1, 0, 2), "Transpose")


@pytest.mark.parametrize("elems", [E29, E30], ids=["2^29", "2^30"])
def test_upsample_nearest(pa, big, elems):
    """(3, 43, H, 1024) x (2, 2) with an output just over `elems` elements.  reaches: upsample_kernel's unsigned i up to 2^30
    and y[i] past byte offsets 2^31 / 2^32."""
    src, dsrc = big
    h = elems // (4 * 129 * 1024) + 1
    shape = (3, 43, h, 1024)
    y = pa.UpSample(dview(pa, dsrc, shape), np.array([1, 1, 2, 2], np.float32))
    assert_same(y.get(), np.repeat(np.repeat(hview(src, shape), 2, axis=2), 2, axis=3), "UpSample")


def test_pools_nchw_above_2_29_outputs(pa, big):
    """Maxpool 3x3 / 1 / pad 1 (generic pool2d_kernel) and AveragePool 2x2 / 1 on (3, 43, 2040, 2048): outputs just over 2^29.
    reaches: pool2d_kernel's unsigned i past 2^29 and `x + (size_t)nc * H * W` past 2^31 bytes."""
    src, dsrc = big
    shape = (3, 43, 2040, 2048)
    assert 129 * 2040 * 2048 > E29
    x = hview(src, shape)
    y = pa.Maxpool(dview(pa, dsrc, shape), (3, 3), (1, 1, 1, 1), (1, 1))
    xp = np.zeros((3, 43, 2042, 2050), np.float32)
    xp[:, :, 1:-1, 1:-1] = x
    want = np.full(shape, -1e4, np.float32)
    for dy in range(3):
        for dx in range(3):
            np.maximum(want, xp[:, :, dy:dy + 2040, dx:dx + 2048], out=want)
    assert_same(y.get(), want, "Maxpool 3x3")
    del y, want, xp
    y = pa.AveragePool(dview(pa, dsrc, shape), (2, 2), (0, 0, 0, 0), (1, 1))
    want = ((x[:, :, :-1, :-1] + x[:, :, :-1, 1:]) + x[:, :, 1:, :-1] + x[:, :, 1:, 1:]) / np.float32(4)
    assert_same(y.get(), want, "AveragePool 2x2")


def test_maxpool_k3s2p1_x4_kernel_above_2_29_inputs(pa, big):
    """The 4-outputs-per-thread stem pool (maxpool_k3s2p1_x4) on (3, 43, 2048, 2048): 5.4e8 inputs, reads past 2^31 bytes.
    reaches: `x + (size_t)nc * H * W + wi0` and the float4 store index of that kernel."""
    src, dsrc = big
    shape = (3, 43, 2048, 2048)
    y = pa.Maxpool(dview(pa, dsrc, shape), (3, 3), (1, 1, 1, 1), (2, 2))
    xp = np.zeros((129, 2050, 2050), np.float32)
    xp[:, 1:-1, 1:-1] = hview(src, (129, 2048, 2048))
    want = np.full((129, 1024, 1024), -1e4, np.float32)
    for dy in range(3):
        for dx in range(3):
            np.maximum(want, xp[:, dy:dy + 2047:2, dx:dx + 2047:2], out=want)
    assert_same(y.get().reshape(129, 1024, 1024), want, "Maxpool 3x3 / 2 / pad 1")


def test_concatenate_above_2_29_elements(pa, big):
    """Concatenate along axis 1 of (3, 20, R, 1024) and (3, 23, R, 1024): copy2d_vec4 with pitches, output just over 2^29.
    reaches: `dst[(size_t)r * dst_pitch4 + c]` past 2^31 bytes."""
    src, dsrc = big
    r = E29 // (129 * 1024) + 1
    sa, sb = (3, 20, r, 1024), (3, 23, r, 1024)
    off = int(np.prod(sa)) + 1024
    y = pa.Concatenate(dview(pa, dsrc, sa), dview(pa, dsrc, sb, offset=off), axis=1)
    assert_same(y.get(), np.concatenate([hview(src, sa), hview(src, sb, offset=off)], axis=1), "Concatenate")


def test_slice_and_pad_above_2_29_elements(pa, big):
    """Slice (a step-2 cut of a 4 GiB tensor) and constant Pad through pl_strided_map_f32, outputs just over 2^29 elements.
    reaches: strided_map_kernel's size_t i / long long src; the Slice reads x past byte offset 2^32."""
    src, dsrc = big
    shape = (2, 129, 2049, 2040)
    assert int(np.prod(shape)) > E30
    y = pa.Slice(dview(pa, dsrc, shape), np.array([1]), np.array([2049]), np.array([2]), np.array([2]))
    assert y.size > E29
    assert_same(y.get(), hview(src, shape)[:, :, 1::2], "Slice")
    del y
    shape = (3, 43, 2040, 2040)
    y = pa.Pad(dview(pa, dsrc, shape), np.array([0, 0, 2, 3, 0, 0, 1, 2]), 1.5)
    assert y.size > E29
    assert_same(y.get(), np.pad(hview(src, shape), ((0, 0), (0, 0), (2, 1), (3, 2)), constant_values=1.5), "Pad")


# ---- 8b. the Q4 twins at more than 2^28 quads (4 GiB) -------------------------------------------------------------------------------
QC = 516                      # 129 quads: 129 * 2^21 pixels = 2.7e8 quads > 2^28, 4.03 GiB


def test_q4_avgpool_above_2_28_quads(pa, big):
    """AveragePoolQ4 2x2 / 2 on Q4 (1, 516, 1024, 2048): the input is 4.03 GiB.
    reaches: pool2d_q4_kernel's `x + (size_t)nc * H * W` in float4 units past byte offset 2^32."""
    from planer_amd import q4
    src, dsrc = big
    shape = (1, 129, 1024, 2048, 4)
    x = hview(src, shape)
    y = q4.AveragePoolQ4(dview(pa, dsrc, shape, chan=QC), (2, 2), (0, 0, 0, 0), (2, 2))
    want = ((x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2]) + x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2]) / np.float32(4)
    assert_same(y.get(), want, "AveragePoolQ4")


def test_q4_upsample_above_2_28_quads(pa, big):
    """UpSampleQ4 x (2, 2) of Q4 (1, 516, 512, 1024): the output is 2.7e8 quads, 4.03 GiB.
    reaches: upsample_q4_kernel's y[i] (float4 index, unsigned i > 2^28) past byte offset 2^32."""
    from planer_amd import q4
    src, dsrc = big
    shape = (1, 129, 512, 1024, 4)
    y = q4.UpSampleQ4(dview(pa, dsrc, shape, chan=QC), np.array([1, 1, 2, 2], np.float32))
    assert_same(y.get(), np.repeat(np.repeat(hview(src, shape), 2, axis=2), 2, axis=3), "UpSampleQ4")


def test_q4_upsample_concat_above_2_28_quads(pa, big):
    """UpConcatQ4: a (1, 256, 512, 1024) upsampled x 2 next to b (1, 260, 1024, 2048), output 129 quads x 2^21 pixels.
    reaches: concat2_q4_kernel's y[i] and b[...] past byte offset 2^32 / 2^31."""
    from planer_amd import q4
    src, dsrc = big
    sa, sb = (1, 64, 512, 1024, 4), (1, 65, 1024, 2048, 4)
    off = int(np.prod(sa))
    y = q4.UpConcatQ4(dview(pa, dsrc, sa, chan=256), np.array([1, 1, 2, 2], np.float32), dview(pa, dsrc, sb, offset=off, chan=260))
    got = y.get()
    del y
    assert_same(got[:, :64], np.repeat(np.repeat(hview(src, sa), 2, axis=2), 2, axis=3), "UpConcatQ4, upsampled half")
    assert_same(got[:, 64:], hview(src, sb, offset=off), "UpConcatQ4, copied half")


def test_q4_scale_shift_above_2_28_quads(pa, big):
    """BatchNormQ4 on Q4 (1, 514, 1024, 2048): 129 quads with a partial last one (padding lanes written as zero).
    reaches: affine_q4_kernel's x[i] / y[i] past byte offset 2^32."""
    from planer_amd import q4
    src, dsrc = big
    c = 514
    shape = (1, 129, 1024, 2048, 4)
    rng = np.random.default_rng(c)
    k = rng.choice(np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]), c).astype(np.float32)
    b = (rng.integers(-16, 17, c) * 0.25).astype(np.float32)
    y = q4.BatchNormQ4(dview(pa, dsrc, shape, chan=c), pa.asarray(k.reshape(1, c, 1, 1)), pa.asarray(b.reshape(1, c, 1, 1)))
    kp, bp = np.zeros(516, np.float32), np.zeros(516, np.float32)
    kp[:c], bp[:c] = k, b
    want = hview(src, shape) * kp.reshape(1, 129, 1, 1, 4) + bp.reshape(1, 129, 1, 1, 4)
    want[:, 128, :, :, 2:] = 0
    assert_same(y.get(), want, "BatchNormQ4")


# ---- 9. host paths ------------------------------------------------------------------------------------------------------------------------
def test_host_copies_of_a_2_1_gib_array(pa, big):
    """DeviceArray.set / get / copy and set_staged / get_begin + get_finish on 2.1 GiB (byte counts past 2^31)."""
    src, dsrc = big
    n = (E29 + (25 << 20)) // 4 * 4
    host = src[:n]
    d = pa.hip.empty((n,))
    d.set(host)
    assert_same(d.get(), host, "set -> get")
    c = d.copy()
    del d
    assert_same(c.get(), host, "copy -> get")
    c.set_staged(src[4:n + 4])
    ticket = c.get_begin()
    assert_same(c.get_finish(ticket), src[4:n + 4], "set_staged -> get_begin / get_finish")


# ---- B. the 2^32 frontier: refusals through the real entry points, nothing launched -------------------------------------------------
def test_entry_points_refuse_work_counts_that_would_wrap_a_32_bit_loop(pa):
    """Every entry point that was moved to the shared guard (pl_loop32_ok, csrc/common.h) refuses a work count of 2^32 - 1, and
    the Q4 ones refuse 2^30 quads, with PL_EUNSUPPORTED and the guard's text.  Each guard stands before the CtxGuard, before any
    allocation and before the launch (read in csrc/pointwise.hip), so the small buffers handed in are never touched.
    2^32 - 1 = 3 * 5 * 17 * 257 * 65537.  Left out: the entry points whose kernels count in size_t (Add, unary ops, the binary
    ops, BatchNorm's flat form, the strided map, Gather, Scatter, compare / where / cast) -- 2^32 - 1 is a legal size there; and the
    row-per-wave kernels with an int row count (gap, softmax, reduce, instance norm): their counters are unsigned now, every int
    row count is legal, and one with 2^31 - 1 rows cannot be asked for without a tensor of that many rows."""
    lib = pa._lib.load()
    ctx = pa.hip.context()
    ok = ctypes.c_int(-1)
    pa._lib.call("pl_stream_loop32_ok", (1 << 32) - 1, ctx.cu_count, ctypes.byref(ok))
    assert ok.value == 0                    # the library's own verdict first: nothing below may reach a launch
    buf = pa.hip.zeros((1024,))
    ibuf = pa.hip.zeros((1024,), np.int32)
    before = buf.get()
    h, p, q = ctx.handle, buf.ptr, ibuf.ptr
    A, Bf, Cf = 65537, 257, 255
    assert A * Bf * Cf == (1 << 32) - 1
    ci = ctypes.c_int
    calls = [
        ("upsample: tensor too large", lib.pl_upsample_nearest_f32, (h, p, p, A, Bf, Cf, 1, 1)),
        ("upsample: tensor too large", lib.pl_upsample_linear_f32, (h, p, p, A, Bf, 85, 1, 3, (ctypes.c_float * 256)())),
        ("resize: tensor too large", lib.pl_resize_linear_f32, (h, p, p, A, 2, 2, Bf, Cf, q, p, q, p)),
        ("resize: image too large", lib.pl_resize_hwc_f32, (h, p, p, 2, 2, Cf, A, Bf, q, p, q, p)),
        ("tile: window too large", lib.pl_tile_accumulate_f32, (h, p, p, p, A, Bf, Cf, 0, 0, A, Bf, 0)),
        ("tile: image too large", lib.pl_tile_normalise_f32, (h, p, p, A, Bf, Cf)),
        ("transpose: tensor too large", lib.pl_transpose_f32, (h, p, p, 3, (ci * 3)(A, Bf, Cf), (ci * 3)(2, 0, 1))),
        ("pool: tensor too large", lib.pl_pool2d_f32, (h, p, p, A, Bf, Cf, 1, 1, 1, 1, 0, 0, 0, 0, 0)),
        ("copy2d: tensor too large", lib.pl_copy2d_f32, (h, p, 65535, p, 65535, 65535, A)),
        ("splitk reduce: tensor too large", lib.pl_splitk_reduce_f32, (h, p, 2, p, A, Bf, Cf, None, None, None, None, 0, 0.0)),
        # channel-quad entry points: 2^30 quads
        ("pool: tensor too large", lib.pl_pool2d_q4_f32, (h, p, p, 1, 4096, 1024, 1024, 1, 1, 1, 1, 0, 0, 0, 0, 0)),
        ("upsample: tensor too large", lib.pl_upsample_nearest_q4_f32, (h, p, p, 1, 4096, 512, 1024, 2, 1)),
        ("concat: tensor too large", lib.pl_concat2_q4_f32, (h, p, p, p, 1, 2048, 2048, 1024, 1024, 1, 1)),
        ("scale_shift: tensor too large", lib.pl_scale_shift_q4_f32, (h, p, p, p, p, 1, 4096, 1 << 20)),
        ("q4 layout conversion: Q4 tensor of 2\\^29 pixel quads", lib.pl_nchw_to_q4_f32, (h, p, p, 1, 2048, 1 << 20)),
        ("q4 layout conversion: Q4 tensor of 2\\^29 pixel quads", lib.pl_q4_to_nchw_f32, (h, p, p, 1, 2048, 1 << 20)),
        # row-per-wave kernels whose row count is a size_t product: 2^31 rows
        ("gap: tensor too large", lib.pl_gap_q4_f32, (h, p, p, 65536, 131072, 1)),
        ("topk: too many rows", lib.pl_topk_f32, (h, p, 65536, 1, 32768, 1, 1, p, p)),
    ]
    for text, fn, args in calls:
        rc = fn(*args)
        assert rc == pa._lib.PL_EUNSUPPORTED, (fn.__name__, rc, lib.pl_last_error())
        with pytest.raises(NotImplementedError, match=text):
            pa._lib.check(rc)
    ctx.synchronize()
    np.testing.assert_array_equal(buf.get(), before)


def test_zz_peak_device_memory_stays_under_12_gib(pa):
    """The largest pool reservation any test of this module left behind (the shared 4 GiB source included)."""
    print("peak device memory of tests/test_gpu_large_tensors.py: %.2f GiB" % (PEAK[0] / GIB))
    assert 0 < PEAK[0] < 12 * (1 << 30), PEAK[0] / GIB

"""Channel-quad ("Q4") tensors: the compiled plan's internal activation layout.

A Q4 tensor holds the reference's (N, C, H, W) array as a DeviceArray of shape
(N, ceil(C/4), H, W, 4) -- channel c sits in quad c // 4, lane c % 4, padding
lanes are zero -- with `.chan = C`.  Nothing here is a reference op: the plan
compiler (plan.assign_layouts) rewrites runs of layers that have Q4 kernels
to the `*_q4` kinds below and puts `to_q4` / `from_q4` at the edges, so what
`Net.__call__` takes and returns is NCHW exactly as in net.py:94-101.

Why: include/planer_hip.h ("channel-quad activations") and DESIGN.md section 4 --
one 16-byte load per (pixel, 4 channels) instead of four 4-byte loads keeps the
fp32 MFMA pipe 13-17 % busier, and every HBM-bound layer moves float4s.
"""
import ctypes
import weakref

import numpy

from . import _lib
from .conv_layouts import CONVT_Q4, DIRECT_Q4, DW_Q4, LAYOUTS, ROWPACK_Q4, STEM_POOL, STEM_POOL_NCHW, STEM_WINO, WF4_Q4, WINO43_Q4
# the packers and predicates of the Q4 layouts, importable from here
from .conv_layouts import (dw_q4_eligible, prepare_dw_q4_weights, prepare_q4_weights, prepare_rowpack_weights,  # noqa: F401
                           prepare_stem_nchw_weights, prepare_stem_wino_weights, prepare_w1d4_q4_weights, prepare_wf4_q4_weights, prepare_winograd4_q4_weights,
                           prepare_winograd43_q4_weights, prepare_winograd_q4_weights, q4_conv_eligible, rowpack_eligible,
                           stem_pool_eligible, stem_pool_nchw_eligible, stem_pool_wino_eligible, w1d_q4_eligible, winograd43_eligible, winograd_q4_eligible)
from .conv_layouts import convt_phase_eligible as convt_q4_eligible, prepare_convt_weights as prepare_convt_q4_weights
from .hip import DeviceArray, _f32, asarray, empty
from .layer import (ACT_NONE, PIXEL_SHUFFLE_AXES, _PAD_MODES, _contig_strides, _full, _host_values, _linear_positions, _linear_weights,
                    _ptr, _strided_map, conv_out_hw, convt_out_hw, convt_q4_call, pixel_shuffle_shapes)
from .plan import ACT_RELU, groupnorm_q4_ok, pad_q4_ok, resize_nearest_q4_ok


def is_q4(a):
    return isinstance(a, DeviceArray) and a.chan is not None


def _new_q4(n, c, h, w, ctx):
    y = empty((n, (c + 3) // 4, h, w, 4), ctx=ctx)
    y.chan = c
    return y


def logical_shape(a):
    n, _, h, w, _ = a.shape
    return (n, a.chan, h, w)


def to_q4(x):
    """NCHW -> Q4 (one HBM pass)."""
    _f32(x)
    if is_q4(x):
        return x
    n, c, h, w = x.shape
    y = _new_q4(n, c, h, w, x.ctx)
    if y.size:
        _lib.call("pl_nchw_to_q4_f32", x.ctx.handle, x.ptr, y.ptr, n, c, h * w)
    return y


def from_q4(xq):
    """Q4 -> NCHW."""
    if not is_q4(xq):
        return xq
    n, c, h, w = logical_shape(xq)
    y = empty((n, c, h, w), ctx=xq.ctx)
    if y.size:
        _lib.call("pl_q4_to_nchw_f32", xq.ctx.handle, xq.ptr, y.ptr, n, c, h * w)
    return y


def _carry_fold(dst, src):
    """A position-independent step keeps its input's pixel-phase fold (refold_q4): same map, same image order."""
    if dst is not None and src is not None and src.fold is not None:
        dst.fold = src.fold
    return dst


def folded_shape(shape, dh, dw):
    """Logical shape of the (N, C, H, W) activation folded by (dh, dw): the pixel phases x[:, :, i::dh, j::dw] as images."""
    n, c, h, w = shape
    return (n * dh * dw, c, -(-h // dh), -(-w // dw))


def refold_q4(xq, dh=1, dw=1, to=None, **check):
    """The Q4 tensor `xq` folded by (dh, dw) (pl_refold_q4_f32): image (n*dh + i)*dw + j of the result holds the pixels
    x[n, :, i::dh, j::dw] of the activation `xq` stands for, zero-filled to ceil(H/dh) x ceil(W/dw).  `xq` may itself be folded
    (`xq.fold`): (1, 1) unfolds, anything else goes from fold to fold in one pass.  A 3x3 / stride 1 conv with dilation (dh, dw)
    and pads (dh, dw, dh, dw) is ConvQ4(dilations=(1, 1), pads=(1, 1, 1, 1)) on the folded tensor, residual folded the same way.
    As a plan step (kind `refold_q4`) the target comes as `to=[dh, dw]`; `from=[dh, dw]`, where the plan gives it, must be the
    fold the input really carries."""
    _f32(xq)
    if not is_q4(xq):
        raise TypeError("refold_q4 needs a Q4 activation (planer_amd.q4.to_q4)")
    if to is not None:
        dh, dw = to
    dh, dw = int(dh), int(dw)
    if dh < 1 or dw < 1:
        raise ValueError("refold_q4: a fold is at least 1, got (%d, %d)" % (dh, dw))
    nf, c, hf, wf = logical_shape(xq)
    sdh, sdw, h, w = xq.fold if xq.fold is not None else (1, 1, hf, wf)
    if check.get("from") is not None and tuple(int(v) for v in check["from"]) != (sdh, sdw):
        raise ValueError("refold_q4: the plan expects an input folded by %s, this one is folded by %s" % (tuple(check["from"]), (sdh, sdw)))
    n = nf // (sdh * sdw)
    y = _new_q4(*folded_shape((n, c, h, w), dh, dw), xq.ctx)
    if dh * dw > 1:
        y.fold = (dh, dw, h, w)
    if y.size:
        _lib.call("pl_refold_q4_f32", xq.ctx.handle, xq.ptr, y.ptr, n, c, h, w, sdh, sdw, dh, dw)
    return y


def ConvTransposeQ4(xq, Kq, B=None, scale=None, shift=None, resq=None, strides=(2, 2), dilations=(1, 1), pads=(0, 0, 0, 0),
                    output_padding=(0, 0), group=1, act=ACT_NONE, alpha=0.0, w_layout=0, **_):
    """layer.ConvTranspose2d with the fused tail of ConvQ4 on Q4 tensors, by output phase (pl_conv2d_convt_q4_f32).
    w_layout CONVT_Q4: Kq from prepare_convt_q4_weights() for these strides; otherwise the filter is prepared here."""
    _f32(xq, Kq, B, scale, shift, resq)
    if not is_q4(xq) or (resq is not None and not is_q4(resq)):
        raise TypeError("ConvTransposeQ4 needs Q4 activations (planer_amd.q4.to_q4)")
    if not convt_q4_eligible(Kq.shape, group, strides, dilations, pads, output_padding):
        raise ValueError("phase-decomposed convtranspose: group 1, dilation 1 and pads within the kernel reach only")
    n, cin, h, w = logical_shape(xq)
    if Kq.shape[0] != cin:
        raise ValueError("convtranspose: weight %s does not match input %s" % (Kq.shape, (n, cin, h, w)))
    cout, kh, kw = Kq.shape[1:]
    ho, wo = convt_out_hw(h, w, kh, kw, strides, pads, output_padding)
    y = _new_q4(n, cout, ho, wo, xq.ctx)
    if resq is not None and resq.shape != y.shape:
        raise ValueError("fused residual shape %s != convtranspose output %s" % (resq.shape, y.shape))
    if y.size:
        Kp = Kq if int(w_layout) == CONVT_Q4 else prepare_convt_q4_weights(Kq, strides)
        convt_q4_call(xq, Kp, B, y, scale, shift, resq, strides, pads, output_padding, act, alpha)
    return y


def pack_rows(x, geom=None, src_ptr=None, ctx=None):
    """The row-packed (zero-padded NHWC) image the stem kernel reads (pl_rowpack_input_f32), kept BESIDE a plan's static
    NCHW input `x` as `x.packed = (geom, image)`, geom = (kw, stride_w, pad_top, pad_left).  First call (geom given):
    allocates the image and fills it from `x`.  Later calls re-fill it from `src_ptr` -- the batch a caller feeds the
    plan -- on `ctx`'s stream: the re-layout then IS the copy into the plan, the NCHW tensor is not written."""
    n, c, h, w = x.shape
    if x.packed is None:
        elems = ctypes.c_size_t()
        _lib.call("pl_rowpack_input_elems", n, c, h, w, geom[0], geom[1], geom[2], geom[3], ctypes.byref(elems))
        x.packed = (tuple(geom), empty((int(elems.value),), ctx=x.ctx))
    g, img = x.packed
    cx = ctx or x.ctx
    _lib.call("pl_rowpack_input_f32", cx.handle, x.ptr if src_ptr is None else src_ptr, img.ptr, n, c, h, w, g[0], g[1], g[2], g[3])
    return img


def ConvQ4(xq, Kq, B=None, scale=None, shift=None, resq=None, group=1, strides=(1, 1),
           dilations=(1, 1), pads=(0, 0, 0, 0), act=ACT_NONE, alpha=0.0, w_layout=DIRECT_Q4, **_):
    """layer.ConvFused on Q4 tensors: act((conv(x,K)+B)*scale + shift + res), all activations Q4.  Kq holds the filter
    prepared for `w_layout` (conv_layouts.LAYOUTS): the direct kernel, the row-packed stem (NCHW input), depthwise, or one of
    the same-signature Winograd / 1-D F(4,3) kernels."""
    _f32(xq, Kq, B, scale, shift, resq)
    if w_layout == ROWPACK_Q4:
        # row-packed stem: the input is the reference's NCHW tensor, the output is Q4
        if is_q4(xq) or (resq is not None and not is_q4(resq)):
            raise TypeError("row-packed ConvQ4 takes an NCHW input (and a Q4 residual)")
        if not rowpack_eligible(Kq.shape, group, strides, dilations, pads):
            raise ValueError("row-packed filters serve group 1 / dilation 1 / Cin < 4 convs only")
        n, cin, h, w = xq.shape
        cout, cin_g, kh, kw = Kq.shape
        if cin_g != cin:
            raise ValueError("conv: weight %s does not match input %s" % (Kq.shape, xq.shape))
        pads, strides = [int(p) for p in pads], [int(s) for s in strides]
        ho, wo = conv_out_hw(h, w, kh, kw, strides, [1, 1], pads)
        y = _new_q4(n, cout, ho, wo, xq.ctx)
        if resq is not None and resq.shape != y.shape:
            raise ValueError("fused residual shape %s != conv output %s" % (resq.shape, y.shape))
        if xq.packed is not None and xq.packed[0] == (kw, strides[1], pads[0], pads[1]):
            # a plan's static input whose row-packed image is kept up to date by whoever feeds the plan (pack_rows)
            _lib.call("pl_conv2d_rowpacked_q4_f32", xq.ctx.handle, xq.packed[1].ptr, n, cin, h, w, Kq.ptr, cout, kh, kw, _ptr(B),
                      y.ptr, strides[0], strides[1], pads[0], pads[1], _ptr(scale), _ptr(shift), _ptr(resq), int(act), float(alpha))
            return y
        _lib.call("pl_conv2d_rowpack_q4_f32", xq.ctx.handle, xq.ptr, n, cin, h, w, Kq.ptr, cout, kh, kw, _ptr(B), y.ptr,
                  strides[0], strides[1], pads[0], pads[1], _ptr(scale), _ptr(shift), _ptr(resq), int(act), float(alpha))
        return y
    if not is_q4(xq) or (resq is not None and not is_q4(resq)):
        raise TypeError("ConvQ4 needs Q4 activations (planer_amd.q4.to_q4)")
    n, cin, h, w = logical_shape(xq)
    cout, cin_g, kh, kw = Kq.shape
    if cin_g * group != cin:
        raise ValueError("conv: weight %s does not match input %s with group=%d" % (Kq.shape, (n, cin, h, w), group))
    pads = [int(p) for p in pads]
    strides = [int(s) for s in strides]
    dilations = [int(d) for d in dilations]
    ho, wo = conv_out_hw(h, w, kh, kw, strides, dilations, pads)
    y = _new_q4(n, cout, ho, wo, xq.ctx)
    if resq is not None and resq.shape != y.shape:
        raise ValueError("fused residual shape %s != conv output %s" % (resq.shape, y.shape))
    if (ho, wo) == (h, w):
        _carry_fold(y, xq)                             # a folded conv (refold_q4): the output is folded like the input
    lay = LAYOUTS.get(w_layout)
    if lay is not None and lay.kernel:
        # the Winograd families and the fused 1-D F(4,3) share one signature
        if not lay.eligible(Kq.shape, (n, cin, h, w), group=group, strides=strides, dilations=dilations, pads=pads):
            raise ValueError("w_layout %d (%s) serves 3x3 / stride 1 / pad 1 / group 1 convs only%s"
                             % (w_layout, lay.name, ", on maps whose sides are 7, 14 or 21" if w_layout == WINO43_Q4 else ""))
        if w_layout == WF4_Q4 and any(a is not None and a.ptr % 16 for a in (B, scale, shift)):
            raise ValueError("the fused F(4x4,3x3) kernel reads bias / scale / shift as 16-byte quads: misaligned parameter")
        _lib.call(lay.kernel, xq.ctx.handle, xq.ptr, n, cin, h, w, Kq.ptr, cout, _ptr(B), y.ptr,
                  _ptr(scale), _ptr(shift), _ptr(resq), int(act), float(alpha))
        return y
    if w_layout == DW_Q4:
        if not dw_q4_eligible(Kq.shape, group, strides, dilations, pads):
            raise ValueError("depthwise Q4 filters serve group == Cin == Cout convs with kh, kw <= 7 and symmetric pads")
        _lib.call("pl_conv2d_dw_q4_f32", xq.ctx.handle, xq.ptr, n, cin, h, w, Kq.ptr, kh, kw, _ptr(B), y.ptr,
                  strides[0], strides[1], dilations[0], dilations[1], pads[0], pads[1], pads[2], pads[3],
                  _ptr(scale), _ptr(shift), _ptr(resq), int(act), float(alpha))
        return y
    _lib.call("pl_conv2d_q4_f32", xq.ctx.handle, xq.ptr, n, cin, h, w, Kq.ptr, cout, kh, kw,
              _ptr(B), y.ptr, strides[0], strides[1], dilations[0], dilations[1],
              pads[0], pads[1], pads[2], pads[3], int(group),
              _ptr(scale), _ptr(shift), _ptr(resq), int(act), float(alpha))
    return y


def ConvPoolQ4(x, Kq, B=None, scale=None, shift=None, group=1, strides=(1, 1), dilations=(1, 1), pads=(0, 0, 0, 0),
               act=ACT_NONE, alpha=0.0, w_layout=STEM_POOL, out=None, src_ptr=None, ctx=None, strip_rows=0, wino=0, **_):
    """Row-packed stem conv (ConvQ4 w_layout 6: NCHW input, filter from prepare_rowpack_weights) with its fused tail, followed
    by layer.Maxpool(w=(3, 3), strides=(2, 2), pads=(1, 1, 1, 1)) (layer.py:71-72), in ONE kernel: only the pooled Q4 tensor is
    written.  Emitted by the plan compiler (plan.fuse_stem_pool) where the max-pool is the conv's only reader.
    w_layout 12: the kernel reads the NCHW tensor itself (filter from prepare_stem_nchw_weights; W % 4 == 0) -- no row-packed
    copy.  A plan's static input then carries `x.prefed = (feed, pooled)`: whoever feeds the plan runs this kernel from the
    caller's batch straight into `pooled` (`out` / `src_ptr` / `ctx` below), and the captured pass starts behind it.
    wino=44 (w_layout 12 only): the polyphase F(4,4) form of that kernel, filter from prepare_stem_wino_weights; a direct-form
    filter that carries one (attach_stem_wino) runs that form too."""
    _f32(x, Kq, B, scale, shift)
    if wino and (w_layout != STEM_POOL_NCHW or int(wino) != STEM_WINO):
        raise ValueError("conv + maxpool: wino=%d is the F(4,4) form of w_layout %d only" % (STEM_WINO, STEM_POOL_NCHW))
    if w_layout == STEM_POOL_NCHW and not wino and Kq in _STEM_WINO:
        Kq, wino = _STEM_WINO[Kq], STEM_WINO      # a plan's stem filter with the F(4,4) form attached (Net picks it)
    if w_layout == STEM_POOL_NCHW and out is None and getattr(x, "prefed", None) is not None:
        return x.prefed[1]                         # a plan's static input: the feed has already run this step
    if is_q4(x) or not stem_pool_eligible(x.shape, Kq.shape, group, strides, dilations, pads):
        raise NotImplementedError("conv + maxpool in one kernel: NCHW 3-channel input, 7x7 / stride 2 / pad 3")
    if any(a is not None and a.ptr % 16 for a in (B, scale, shift)):
        raise ValueError("the stem + max-pool kernel reads bias / scale / shift as 16-byte quads: misaligned parameter")
    n, cin, h, w = x.shape
    cout, _, kh, kw = Kq.shape
    pads, strides = [int(p) for p in pads], [int(s) for s in strides]
    ho, wo = conv_out_hw(h, w, kh, kw, strides, [1, 1], pads)
    cx = ctx or x.ctx
    if w_layout == STEM_POOL_NCHW:
        xptr = x.ptr if src_ptr is None else src_ptr
        if w % 4 or xptr % 16:
            raise NotImplementedError("the NCHW stem + max-pool kernel needs W % 4 == 0 and a 16-byte aligned input")
        y = out if out is not None else _new_q4(n, cout, (ho + 1) // 2, (wo + 1) // 2, cx)
        _lib.call(_stem_entry(wino), cx.handle, xptr, n, h, w, Kq.ptr, cout, _ptr(B), y.ptr, _ptr(scale),
                  _ptr(shift), int(act), float(alpha), int(strip_rows))
        return y
    geom = (kw, strides[1], pads[0], pads[1])
    if x.packed is not None and x.packed[0] == geom:
        img = x.packed[1]                          # a plan's static input: whoever feeds the plan keeps the image current
    else:
        elems = ctypes.c_size_t()
        _lib.call("pl_rowpack_input_elems", n, cin, h, w, geom[0], geom[1], geom[2], geom[3], ctypes.byref(elems))
        img = empty((int(elems.value),), ctx=x.ctx)
        _lib.call("pl_rowpack_input_f32", x.ctx.handle, x.ptr, img.ptr, n, cin, h, w, geom[0], geom[1], geom[2], geom[3])
    y = _new_q4(n, cout, (ho + 1) // 2, (wo + 1) // 2, x.ctx)
    _lib.call("pl_conv2d_rowpacked_pool_q4_f32", x.ctx.handle, img.ptr, n, cin, h, w, Kq.ptr, cout, kh, kw, _ptr(B), y.ptr,
              strides[0], strides[1], pads[0], pads[1], _ptr(scale), _ptr(shift), int(act), float(alpha))
    return y


_STEM_WINO = weakref.WeakKeyDictionary()      # direct-form stem filter (w_layout 12) -> its F(4,4) filter


def attach_stem_wino(Kq, K):
    """Give the prepared stem filter `Kq` (prepare_stem_nchw_weights) the F(4,4) form of the OIHW filter `K` to run instead
    (ConvPoolQ4, stem_pool_feeder), or take it away (K = None).  How a plan carries the form: the step, its w_layout and its
    filter key stay what they are."""
    if K is None:
        _STEM_WINO.pop(Kq, None)
    elif Kq not in _STEM_WINO:
        _STEM_WINO[Kq] = prepare_stem_wino_weights(K)


def _stem_entry(wino):
    return "pl_conv2d_stem_pool_wino_q4_f32" if wino else "pl_conv2d_stem_pool_nchw_q4_f32"


def stem_pool_feeder(x_shape, Kq, B, scale, shift, act, alpha, pooled, strip_rows=0, wino=0):
    """feed(src_ptr, ctx): the NCHW stem + max-pool kernel from the batch at `src_ptr` into the persistent tensor `pooled`, on
    `ctx`'s stream -- what `DeviceArray.prefed` holds for a plan's static input (Net._pack_static_inputs)."""
    n, _, h, w = (int(v) for v in x_shape)
    cout = int(Kq.shape[0])
    if not wino and Kq in _STEM_WINO:
        Kq, wino = _STEM_WINO[Kq], STEM_WINO

    def feed(src_ptr, ctx):
        _lib.call(_stem_entry(wino), ctx.handle, src_ptr, n, h, w, Kq.ptr, cout, _ptr(B), pooled.ptr, _ptr(scale),
                  _ptr(shift), int(act), float(alpha), int(strip_rows))
    return feed


def ConvQ4Pair(xq, K1, B1, scale1, shift1, K2, B2, scale2, shift2, para1=None, para2=None, **_):
    """Two fused convs (ConvQ4, w_layout 2, group 1, no dilation, no residual) that read the SAME Q4 input, in one
    launch -> (y1, y2).  Emitted by plan.pair_sibling_convs where a graph forks into two convs (ResNet's stride-2
    3x3 conv and the 1x1 stride-2 projection of the same block)."""
    _f32(xq, K1, B1, scale1, shift1, K2, B2, scale2, shift2)
    if not is_q4(xq):
        raise TypeError("ConvQ4Pair needs a Q4 activation")
    n, cin, h, w = logical_shape(xq)
    outs, args = [], []
    for K, B, sc, sh, para in ((K1, B1, scale1, shift1, para1 or {}), (K2, B2, scale2, shift2, para2 or {})):
        cout, cin_g, kh, kw = K.shape
        strides = [int(v) for v in para.get("strides", (1, 1))]
        pads = [int(v) for v in para.get("pads", (0, 0, 0, 0))]
        if (cin_g != cin or int(para.get("group", 1)) != 1 or [int(v) for v in para.get("dilations", (1, 1))] != [1, 1]
                or pads[0] != pads[2] or pads[1] != pads[3] or int(para.get("act", 0)) & ~3):
            raise ValueError("ConvQ4Pair: group 1, dilation 1, symmetric pads, no residual; weight %s on input %s"
                             % (K.shape, (n, cin, h, w)))
        ho, wo = conv_out_hw(h, w, kh, kw, strides, [1, 1], pads)
        y = _new_q4(n, cout, ho, wo, xq.ctx)
        outs.append(y)
        args += [K.ptr, cout, kh, kw, strides[0], strides[1], pads[0], pads[1], _ptr(B), _ptr(sc), _ptr(sh),
                 int(para.get("act", 0)), float(para.get("alpha", 0.0)), y.ptr]
    _lib.call("pl_conv2d_q4_pair_f32", xq.ctx.handle, xq.ptr, n, cin, h, w, *args)
    return tuple(outs)


# ---- Winograd F(4x4,3x3) stage by stage (plan-internal; plan.chain_winograd emits these) -----------
def _wino_tensor(n, c, h, w, ctx):
    """V or M of an (n, c, h, w) activation: [36][c/4][T][4], T = n * ceil(h/4) * ceil(w/4)."""
    e = ctypes.c_size_t()
    _lib.call("pl_wino4_elems", n, c, h, w, ctypes.byref(e))
    t = empty((max(e.value, 1),), ctx=ctx)
    t.meta = (n, c, h, w)
    return t


def wino4_chain_supported(shape, ctx):
    """Can the LDS transform kernel (whole planes per workgroup) take an (N, C, H, W) activation?"""
    n, c, h, w = shape
    if c % 4:
        return False
    ok = ctypes.c_int()
    _lib.call("pl_wino4_chain_supported", ctx.handle, n, c, h, w, ctypes.byref(ok))
    return bool(ok.value)


def Wino4In(xq):
    """B^T d B of every 6x6 tile of a Q4 activation -> V."""
    _f32(xq)
    if not is_q4(xq):
        raise TypeError("Wino4In needs a Q4 activation")
    n, c, h, w = logical_shape(xq)
    v = _carry_fold(_wino_tensor(n, c, h, w, xq.ctx), xq)
    _lib.call("pl_wino4_input_q4_f32", xq.ctx.handle, xq.ptr, n, c, h, w, v.ptr)
    return v


def Wino4Gemm(v, Kq, **_):
    """The 36 per-frequency GEMMs: V (Cin) x Winograd-domain filters -> M (Cout)."""
    n, cin, h, w = v.meta
    cout, cin_k, kh, kw = Kq.shape
    if cin_k != cin or (kh, kw) != (3, 3):
        raise ValueError("conv: weight %s does not match input %s" % (Kq.shape, (n, cin, h, w)))
    m = _carry_fold(_wino_tensor(n, cout, h, w, v.ctx), v)
    _lib.call("pl_wino4_gemm_q4_f32", v.ctx.handle, v.ptr, n, cin, h, w, Kq.ptr, cout, m.ptr)
    return m


def _wino_tail_check(m, resq):
    n, c, h, w = m.meta
    if resq is not None and (not is_q4(resq) or logical_shape(resq) != (n, c, h, w)):
        raise ValueError("fused residual %s != conv output %s" % (getattr(resq, "shape", None), (n, c, h, w)))
    return n, c, h, w


def Wino4Out(m, B=None, scale=None, shift=None, resq=None, act=ACT_NONE, alpha=0.0, **_):
    """A^T m A + the conv's fused tail -> y (Q4)."""
    _f32(B, scale, shift, resq)
    n, c, h, w = _wino_tail_check(m, resq)
    y = _carry_fold(_new_q4(n, c, h, w, m.ctx), m)
    _lib.call("pl_wino4_output_q4_f32", m.ctx.handle, m.ptr, n, c, h, w, _ptr(B), _ptr(scale), _ptr(shift), _ptr(resq),
              int(act), float(alpha), y.ptr)
    return y


def Wino4Chain(m, B=None, scale=None, shift=None, resq=None, act=ACT_NONE, alpha=0.0, keep_y=True, **_):
    """Wino4Out and the Wino4In of the next 3x3 conv in one kernel: -> (y, V) or, with keep_y=False
    (nothing else reads y), V alone -- y then never exists in memory."""
    _f32(B, scale, shift, resq)
    n, c, h, w = _wino_tail_check(m, resq)
    y = _carry_fold(_new_q4(n, c, h, w, m.ctx), m) if keep_y else None
    v = _carry_fold(_wino_tensor(n, c, h, w, m.ctx), m)
    _lib.call("pl_wino4_chain_q4_f32", m.ctx.handle, m.ptr, n, c, h, w, _ptr(B), _ptr(scale), _ptr(shift), _ptr(resq),
              int(act), float(alpha), _ptr(y), v.ptr)
    return (y, v) if keep_y else v


# ---- mixed-tile Winograd (maps of 7 / 14 / 21 a side) stage by stage: the same four stages, other kernels ----
def _wino43_tensor(n, c, h, w, ctx):
    e = ctypes.c_size_t()
    _lib.call("pl_wino43_elems", n, c, h, w, ctypes.byref(e))
    t = empty((max(e.value, 1),), ctx=ctx)
    t.meta = (n, c, h, w)
    return t


def Wino43In(xq):
    _f32(xq)
    if not is_q4(xq):
        raise TypeError("Wino43In needs a Q4 activation")
    n, c, h, w = logical_shape(xq)
    v = _carry_fold(_wino43_tensor(n, c, h, w, xq.ctx), xq)
    _lib.call("pl_wino43_input_q4_f32", xq.ctx.handle, xq.ptr, n, c, h, w, v.ptr)
    return v


def Wino43Gemm(v, Kq, **_):
    n, cin, h, w = v.meta
    cout, cin_k, kh, kw = Kq.shape
    if cin_k != cin or (kh, kw) != (3, 3):
        raise ValueError("conv: weight %s does not match input %s" % (Kq.shape, (n, cin, h, w)))
    m = _carry_fold(_wino43_tensor(n, cout, h, w, v.ctx), v)
    _lib.call("pl_wino43_gemm_q4_f32", v.ctx.handle, v.ptr, n, cin, h, w, Kq.ptr, cout, m.ptr)
    return m


def Wino43Out(m, B=None, scale=None, shift=None, resq=None, act=ACT_NONE, alpha=0.0, **_):
    _f32(B, scale, shift, resq)
    n, c, h, w = _wino_tail_check(m, resq)
    y = _carry_fold(_new_q4(n, c, h, w, m.ctx), m)
    _lib.call("pl_wino43_output_q4_f32", m.ctx.handle, m.ptr, n, c, h, w, _ptr(B), _ptr(scale), _ptr(shift), _ptr(resq),
              int(act), float(alpha), y.ptr)
    return y


def Wino43Chain(m, B=None, scale=None, shift=None, resq=None, act=ACT_NONE, alpha=0.0, keep_y=True, **_):
    _f32(B, scale, shift, resq)
    n, c, h, w = _wino_tail_check(m, resq)
    y = _carry_fold(_new_q4(n, c, h, w, m.ctx), m) if keep_y else None
    v = _carry_fold(_wino43_tensor(n, c, h, w, m.ctx), m)
    _lib.call("pl_wino43_chain_q4_f32", m.ctx.handle, m.ptr, n, c, h, w, _ptr(B), _ptr(scale), _ptr(shift), _ptr(resq),
              int(act), float(alpha), _ptr(y), v.ptr)
    return (y, v) if keep_y else v


def Conv1x1WinoIn(xq, Kq, B=None, scale=None, shift=None, act=ACT_NONE, alpha=0.0, wino=4, **_):
    """ConvQ4 (1x1, stride 1, group 1, fused bias / scale / shift / activation, no residual) and the Wino4In of the 3x3 conv
    that is its only reader, in one kernel -> V (csrc/conv1x1_wino_in_kernel.h).  Emitted by plan.fuse_conv1x1_wino_in for the
    1x1 -> 3x3 pairs of a detection net's blocks at small maps; the 1x1 conv's own output never exists."""
    _f32(xq, Kq, B, scale, shift)
    if not is_q4(xq):
        raise TypeError("Conv1x1WinoIn needs a Q4 activation")
    n, cin, h, w = logical_shape(xq)
    cout, cin_k, kh, kw = Kq.shape
    if (kh, kw) != (1, 1) or cin_k != cin or cout % 4 or int(wino) != 4:
        raise ValueError("Conv1x1WinoIn: 1x1 filter %s on input %s, Cout %% 4 == 0, F(4x4,3x3) tiles" % (Kq.shape, (n, cin, h, w)))
    v = _carry_fold(_wino_tensor(n, cout, h, w, xq.ctx), xq)
    _lib.call("pl_conv1x1_wino_in_q4_f32", xq.ctx.handle, xq.ptr, n, cin, h, w, Kq.ptr, cout, _ptr(B), _ptr(scale), _ptr(shift),
              int(act), float(alpha), int(wino), v.ptr)
    return v


# ---- HBM-bound layers on Q4 tensors ---------------------------------------------------------
def _like(x, shape=None):
    y = empty(shape or x.shape, ctx=x.ctx)
    y.chan = x.chan
    return _carry_fold(y, x) if shape is None else y


def _pool_q4(xq, w, pads, strides, mode):
    _f32(xq)
    n, c, h, wd = logical_shape(xq)
    kh, kw = int(w[0]), int(w[1])
    sh, sw = int(strides[0]), int(strides[1])
    pads = [int(p) for p in pads]
    ho = (h + pads[0] + pads[2] - kh + sh) // sh        # util.py:84
    wo = (wd + pads[1] + pads[3] - kw + sw) // sw       # util.py:85
    y = _new_q4(n, c, ho, wo, xq.ctx)
    _lib.call("pl_pool2d_q4_f32", xq.ctx.handle, xq.ptr, y.ptr, n, c, h, wd, kh, kw, sh, sw,
              pads[0], pads[1], pads[2], pads[3], mode)
    return y


def MaxpoolQ4(xq, w=(2, 2), pads=(0, 0, 0, 0), strides=(2, 2)):
    """layer.Maxpool (layer.py:71-72) on a Q4 tensor."""
    return _pool_q4(xq, w, pads, strides, 0)


def AveragePoolQ4(xq, w=(2, 2), pads=(0, 0, 0, 0), strides=(2, 2)):
    """layer.AveragePool (layer.py:74-75) on a Q4 tensor."""
    return _pool_q4(xq, w, pads, strides, 1)


def GlobalAveragePoolQ4(xq):
    """layer.GlobalAveragePool (layer.py:77-78): Q4 in, plain (N, C, 1, 1) out."""
    _f32(xq)
    n, c, h, w = logical_shape(xq)
    if h * w == 0:                                      # numpy: the mean of an empty slice is NaN
        return _full((n, c, 1, 1), numpy.nan, xq.ctx)
    y = empty((n, c, 1, 1), ctx=xq.ctx)
    _lib.call("pl_gap_q4_f32", xq.ctx.handle, xq.ptr, y.ptr, n, c, h * w)
    return y


def _linear_tables(ctx, h, w, oh, ow):
    """The device position tables of layer._linear_positions for one geometry, uploaded once and kept with the context: a
    captured plan or a plan file then reads them as constants (an upload cannot be captured).  This differs from the NCHW
    layer._upsample_linear on purpose: that one uploads on every call and so cannot run inside a captured plan at all.  Four
    small arrays (OH + OW entries each) per geometry a context has seen, never evicted -- a net has a handful.  A table made
    before Context.pool_debug was switched on is an ordinary block: a hygiene check that wants the table reads under guard
    drops the cache first (`ctx.__dict__.pop("_linear_q4_tables", None)`, as tests/test_gpu_linear_q4.py does)."""
    cache = ctx.__dict__.setdefault("_linear_q4_tables", {})
    t = cache.get((h, w, oh, ow))
    if t is None:
        t = cache[(h, w, oh, ow)] = [asarray(a, ctx=ctx) for a in _linear_positions(h, oh) + _linear_positions(w, ow)]
    return t


def _check_res(resq, y):
    if resq is not None and (not is_q4(resq) or resq.shape != y.shape or resq.chan != y.chan):
        raise ValueError("fused residual %s != upsample output %s" % (getattr(resq, "shape", None), y.shape))


def _upsample_linear_q4(xq, fh, fw, resq=None):
    """layer._upsample_linear on a Q4 tensor: integer factors -> pl_upsample_linear_q4_f32, anything else ->
    pl_resize_linear_q4_f32 at round(k * size); `resq` is added in the kernel's write pass."""
    n, c, h, w = logical_shape(xq)
    if fh == int(fh) and fw == int(fw):
        fh, fw = int(fh), int(fw)
        if fh == 1 and fw == 1:
            return xq if resq is None else AddQ4(xq, resq)
        y = _new_q4(n, c, h * fh, w * fw, xq.ctx)
        _check_res(resq, y)
        if fh * fw > 64:
            raise NotImplementedError("linear upsample: fh * fw <= 64 on the HIP path, got %d x %d" % (fh, fw))
        tab = _linear_weights(fh, fw)
        _lib.call("pl_upsample_linear_q4_f32", xq.ctx.handle, xq.ptr, y.ptr, _ptr(resq), n, c, h, w, fh, fw,
                  (_lib.c_float * tab.size)(*tab.reshape(-1).tolist()))
        return y
    oh, ow = int(round(fh * h)), int(round(fw * w))
    if h < 2 or w < 2:
        raise ValueError("linear resize needs at least 2 x 2 pixels (the reference indexes row / column + 1)")
    y = _new_q4(n, c, oh, ow, xq.ctx)
    _check_res(resq, y)
    if y.size:
        dev = _linear_tables(xq.ctx, h, w, oh, ow)
        _lib.call("pl_resize_linear_q4_f32", xq.ctx.handle, xq.ptr, y.ptr, _ptr(resq), n, c, h, w, oh, ow, *[d.ptr for d in dev])
    return y


def _upsample_nearest_q4(xq, fh, fw):
    n, c, h, w = logical_shape(xq)
    y = _new_q4(n, c, h * fh, w * fw, xq.ctx)
    _lib.call("pl_upsample_nearest_q4_f32", xq.ctx.handle, xq.ptr, y.ptr, n, c, h, w, fh, fw)
    return y


def UpSampleQ4(xq, k, mode="nearest", resq=None):
    """layer.UpSample (layer.py:80-82) on a Q4 tensor.  `resq` (linear only): a Q4 tensor of the output's shape added on the
    way out -- what plan.fuse_linear_add folds an add_q4 behind the upsample into."""
    _f32(xq, resq)
    if not is_q4(xq):
        raise TypeError("UpSampleQ4 needs a Q4 activation (planer_amd.q4.to_q4)")
    if mode not in ("nearest", "linear"):
        raise NotImplementedError("upsample mode %r is not on the HIP path" % mode)
    kv = _host_values(k)
    if kv.size == 0:
        raise ValueError("upsample needs scales (the reference's size-only branch is broken, layer.py:81)")
    fh, fw = [int(v) for v in kv[-2:].astype(int).tolist()]       # truncated, layer.py:82
    if mode == "linear":
        return _upsample_linear_q4(xq, fh, fw, resq)
    if resq is not None:
        raise ValueError("UpSampleQ4: a fused residual goes with mode 'linear' only")
    return _upsample_nearest_q4(xq, fh, fw)


def ResizeQ4(xq, roi, k, size=None, mode="nearest", coordinate_transformation_mode="half_pixel",
             nearest_mode="round_prefer_floor", resq=None):
    """layer.Resize (layer.py:84-88) on a Q4 tensor: scales or sizes; linear as in UpSampleQ4 (the mode names are ignored, as
    the reference ignores them), nearest for the pairs whose shift is zero.  The shifted nearest pairs have no Q4 form."""
    _f32(xq, resq)
    if not is_q4(xq):
        raise TypeError("ResizeQ4 needs a Q4 activation (planer_amd.q4.to_q4)")
    if mode not in ("nearest", "linear"):
        raise NotImplementedError("resize mode %r is not on the HIP path" % mode)
    kv = _host_values(k)
    if kv.size == 0:
        sz = _host_values(size)
        kv = sz[-2:] / numpy.array(logical_shape(xq)[-2:])
    fh, fw = [float(v) for v in kv[-2:].tolist()]
    if mode == "linear":
        return _upsample_linear_q4(xq, fh, fw, resq)
    if resq is not None:
        raise ValueError("ResizeQ4: a fused residual goes with mode 'linear' only")
    fh, fw = int(fh), int(fw)                      # util.py:213
    if fh < 1 or fw < 1:
        raise NotImplementedError("resize: nearest down-scaling (the reference returns an empty map) is not on the HIP path")
    if not resize_nearest_q4_ok(fh, fw, coordinate_transformation_mode, nearest_mode):
        raise NotImplementedError("ResizeQ4: nearest up-scaling with (%s, %s) shifts the map; that has no channel-quad form"
                                  % (coordinate_transformation_mode, nearest_mode))
    return _upsample_nearest_q4(xq, fh, fw)


def UpSampleAddQ4(xq, k, resq, **para):
    """UpSampleQ4(mode="linear") + AddQ4 in one kernel: the plan step `upsample_add_q4` (plan.fuse_linear_add)."""
    return UpSampleQ4(xq, k, resq=resq, **para)


def ResizeAddQ4(xq, roi, k, size, resq, **para):
    """ResizeQ4(mode="linear") + AddQ4 in one kernel: the plan step `resize_add_q4`; `size` may be None."""
    return ResizeQ4(xq, roi, k, size, resq=resq, **para)


def PixelShuffleQ4(xq, r, order="crd", inverse=False, nchw_out=False):
    """layer.PixelShuffle on a Q4 tensor in one pass (pl_pixel_shuffle_q4_f32): r = 2, 3, 4; CRD order for any channel
    count, DCR where the narrow side has C % 4 == 0.  `nchw_out` (shuffles only): the result is the plain NCHW tensor -- what a
    shuffle that ends the program is compiled to, instead of a Q4 result and a from_q4 behind it.  A folded input (refold_q4)
    raises: the shuffle moves pixels between phases."""
    _f32(xq)
    if not is_q4(xq):
        raise TypeError("PixelShuffleQ4 needs a Q4 activation (planer_amd.q4.to_q4)")
    if xq.fold is not None:
        raise ValueError("PixelShuffleQ4: the input is folded by %s; a pixel shuffle has no folded form" % (tuple(xq.fold[:2]),))
    r, inverse = int(r), bool(inverse)
    if (order, inverse) not in PIXEL_SHUFFLE_AXES:
        raise ValueError("PixelShuffleQ4: order is 'crd' or 'dcr', got %r" % (order,))
    if nchw_out and inverse:
        raise ValueError("PixelShuffleQ4: nchw_out goes with a shuffle only")
    shp = pixel_shuffle_shapes(logical_shape(xq), r, order, inverse)
    if shp is None:
        raise ValueError("pixelshuffle: r = %s, order %r does not fit the input %s" % (r, order, logical_shape(xq)))
    n, c, h, w = shp[1]
    y = empty(shp[1], ctx=xq.ctx) if nchw_out else _new_q4(n, c, h, w, xq.ctx)
    narrow = logical_shape(xq) if inverse else shp[1]
    if y.size:
        _lib.call("pl_pixel_shuffle_q4_f32", xq.ctx.handle, xq.ptr, y.ptr, narrow[0], narrow[1], narrow[2], narrow[3], r,
                  0 if order == "crd" else 1, int(inverse), int(bool(nchw_out)))
    return y


def BatchNormQ4(xq, K, B):
    """layer.BatchNorm (layer.py:125-127) on a Q4 tensor (only reached when it could not be fused)."""
    _f32(xq, K, B)
    n, c, h, w = logical_shape(xq)
    if K.size != c or B.size != c:
        raise ValueError("batchnorm: K/B must hold one value per channel")
    y = _like(xq)
    _lib.call("pl_scale_shift_q4_f32", xq.ctx.handle, xq.ptr, y.ptr, K.ptr, B.ptr, n, c, h * w)
    return y


def ReLUQ4(xq):
    """layer.ReLU (layer.py:44-46): in place on the padded buffer (relu(0) = 0 keeps the padding)."""
    _lib.call("pl_relu_f32", xq.ctx.handle, xq.ptr, xq.ptr, xq.size)
    return xq


def clip_q4_ok(c, min=0, max=1, **_):
    """ClipQ4 keeps the zero padding of a partial last quad only when clip(0) == 0."""
    return c % 4 == 0 or float(min) <= 0.0 <= float(max)


def ClipQ4(xq, min=0, max=1):
    """layer.Clip (layer.py:247-251): in place on the padded buffer like the reference's in-place numpy branch.  Only
    scheduled where clip_q4_ok holds (ReLU6 = clip(0, 6) always does)."""
    _lib.call("pl_unary_f32", xq.ctx.handle, xq.ptr, xq.ptr, xq.size, 6, float(min), float(max))
    return xq


def InstanceNormQ4(xq, s, bias, resq=None, epsilon=1e-5, act=ACT_NONE):
    """layer.InstanceNormalization (layer.py:217-226) on a Q4 tensor, IN PLACE like the reference, with the tail the plan
    compiler folds in (plan.fuse_instnorm_q4): xq = IN(xq) [+ resq] [relu].  One workgroup per (image, quad) for planes of up to
    _lib.INSTNORM_Q4_ONE_WG_PIXELS pixels, chunk statistics + merge-and-apply above (pl_instancenorm_q4_f32)."""
    _f32(xq, s, bias, resq)
    if not is_q4(xq) or (resq is not None and not is_q4(resq)):
        raise TypeError("InstanceNormQ4 needs Q4 activations (planer_amd.q4.to_q4)")
    n, c, h, w = logical_shape(xq)
    if s.size != c or bias.size != c:
        raise ValueError("instancenormalization: one scale / bias value per channel")
    if resq is not None and (resq.shape != xq.shape or resq.chan != c):
        raise ValueError("fused residual shape %s != instancenormalization input %s" % (resq.shape, xq.shape))
    if int(act) not in (ACT_NONE, ACT_RELU):
        raise ValueError("InstanceNormQ4: act is 0 (none) or 1 (relu)")
    if h * w == 0 or xq.size == 0:                      # numpy leaves an empty x as it is
        return xq
    _lib.call("pl_instancenorm_q4_f32", xq.ctx.handle, xq.ptr, s.ptr, bias.ptr, _ptr(resq), n, c, h * w, float(epsilon), int(act))
    return xq


def GroupNormQ4(xq, s, bias, gamma=None, beta=None, resq=None, groups=None, epsilon=1e-5, act=ACT_NONE):
    """layer.GroupNorm -- reshape (N, G, -1), InstanceNormalization with the G values s / bias, reshape back, [mul gamma], [add
    beta] -- on a Q4 tensor, IN PLACE like the instance norm inside it, with the tail the plan compiler folds in
    (plan.fuse_instnorm_q4): xq = GN(xq) [+ resq] [relu].  One launch where the group's run (C / G a multiple of 4) or the plane
    (C / G of 2 or 1) has up to _lib.INSTNORM_Q4_ONE_WG_PIXELS float4s, chunk statistics + merge-and-apply above
    (pl_groupnorm_q4_f32).  Other C / G have no channel-quad form (groupnorm_q4_ok) and raise."""
    _f32(xq, s, bias, gamma, beta, resq)
    if not is_q4(xq) or (resq is not None and not is_q4(resq)):
        raise TypeError("GroupNormQ4 needs Q4 activations (planer_amd.q4.to_q4)")
    n, c, h, w = logical_shape(xq)
    if groups is None or int(groups) < 1 or c % int(groups):
        raise ValueError("groupnorm: %r groups do not divide %d channels" % (groups, c))
    groups = int(groups)
    if s.size != groups or bias.size != groups:
        raise ValueError("groupnorm: one scale / bias value per group")
    if any(p is not None and p.size != c for p in (gamma, beta)):
        raise ValueError("groupnorm: one gamma / beta value per channel")
    if resq is not None and (resq.shape != xq.shape or resq.chan != c):
        raise ValueError("fused residual shape %s != groupnorm input %s" % (resq.shape, xq.shape))
    if int(act) not in (ACT_NONE, ACT_RELU):
        raise ValueError("GroupNormQ4: act is 0 (none) or 1 (relu)")
    if not groupnorm_q4_ok(c, groups):
        raise NotImplementedError("GroupNormQ4: %d channels per group split a channel quad unevenly; 1, 2 or a multiple of 4 have a "
                                  "channel-quad form" % (c // groups))
    if h * w == 0 or xq.size == 0:                      # numpy leaves an empty x as it is
        return xq
    _lib.call("pl_groupnorm_q4_f32", xq.ctx.handle, xq.ptr, s.ptr, bias.ptr, _ptr(gamma), _ptr(beta), _ptr(resq), n, c, h * w, groups,
              float(epsilon), int(act))
    return xq


def PadQ4(xq, pads, constant_value=0, mode="constant"):
    """layer.Pad (layer.py:241-245) of the pixel axes of a Q4 tensor: the strided-map kernel on the 5-D view (N, quads, H, W, 4),
    whose last axis -- the four lanes of a pixel -- is copied as it is.  Only scheduled where plan.pad_q4_ok holds: no padding of
    N or C, and in constant mode a value that keeps the padding lanes zero."""
    _f32(xq)
    if not is_q4(xq):
        raise TypeError("PadQ4 needs a Q4 activation (planer_amd.q4.to_q4)")
    if isinstance(constant_value, DeviceArray):
        constant_value = _host_values(constant_value).reshape(-1)[0]
    pv = [int(v) for v in _host_values(pads).reshape(-1)]
    if not pad_q4_ok(xq.chan, pv, constant_value, mode):
        raise ValueError("PadQ4: pixel pads only (N, C pads 0), modes %s, and a constant of 0 unless C %% 4 == 0" % (sorted(_PAD_MODES),))
    n, cq, h, w, _ = xq.shape
    (pt, pl), (pb, pr) = pv[2:4], pv[6:8]
    if mode != "constant" and ((h == 0 and pt + pb) or (w == 0 and pl + pr)):
        raise ValueError("can't extend empty axis using modes other than 'constant' or 'empty'")      # np.pad's refusal
    m = _PAD_MODES[mode]
    y = _strided_map(xq, [n, cq, h + pt + pb, w + pl + pr, 4], _contig_strides(xq.shape), [0, 0, -pt, -pl, 0], [1] * 5,
                     extent=list(xq.shape), wrap=[0, 0, m, m, 0], fill=float(constant_value))
    y.chan = xq.chan
    return y


def LeakyReLUQ4(xq, alpha=0.2):
    y = _like(xq)
    _lib.call("pl_leakyrelu_f32", xq.ctx.handle, xq.ptr, y.ptr, xq.size, float(alpha))
    return y


def SigmoidQ4(xq):
    """Only scheduled for C % 4 == 0 (sigmoid(0) = 0.5 would dirty the padding lanes)."""
    y = _like(xq)
    _lib.call("pl_sigmoid_f32", xq.ctx.handle, xq.ptr, y.ptr, xq.size)
    return y


def AddQ4(x1, x2):
    """layer.Add (layer.py:93-95), equal shapes, both Q4."""
    if not (is_q4(x1) and is_q4(x2)) or x1.shape != x2.shape or x1.chan != x2.chan:
        raise ValueError("AddQ4 needs two Q4 tensors of one shape")
    y = _like(x1)
    _lib.call("pl_add_f32", x1.ctx.handle, x1.ptr, x2.ptr, y.ptr, x1.size)
    return y


def ConcatenateQ4(*xs, axis=1):
    """layer.Concatenate (layer.py:90-91) along channels; every input needs C % 4 == 0 so that the
    quads of consecutive inputs abut."""
    if axis != 1 or any(not is_q4(a) or a.chan % 4 for a in xs):
        raise ValueError("ConcatenateQ4: channel axis, C % 4 == 0 inputs only")
    n, _, h, w, _ = xs[0].shape
    if any(a.shape[0] != n or a.shape[2:] != xs[0].shape[2:] for a in xs):
        raise ValueError("concat: shapes differ off the axis: %s" % [logical_shape(b) for b in xs])
    total = sum(a.chan for a in xs)
    if len(xs) == 2:
        return UpConcatQ4(xs[0], None, xs[1])
    y = _carry_fold(_new_q4(n, total, h, w, xs[0].ctx), xs[0])
    off, pitch = 0, (total // 4) * h * w * 4
    for a in xs:
        width = a.shape[1] * h * w * 4
        if width and n:
            _lib.call("pl_copy2d_f32", y.ctx.handle, y.ptr + off * 4, pitch, a.ptr, width, width, n)
        off += width
    return y


def UpConcatQ4(aq, k, bq, mode="nearest", axis=1):
    """layer.Concatenate([layer.UpSample(a, k), b], axis=1) on Q4 tensors in one kernel (k = None: no upsampling).
    Emitted by the plan compiler for upsample -> concat routes; also serves every two-input Q4 concat."""
    _f32(aq, bq)
    if axis != 1 or mode != "nearest" or not is_q4(aq) or not is_q4(bq) or aq.chan % 4 or bq.chan % 4:
        raise ValueError("UpConcatQ4: two Q4 tensors with C % 4 == 0, channel axis, nearest mode")
    fh = fw = 1
    if k is not None:
        kv = _host_values(k)
        if kv.size == 0:
            raise ValueError("upsample needs scales (the reference's size-only branch is broken, layer.py:81)")
        fh, fw = [int(v) for v in kv[-2:].astype(int).tolist()]
    n, ca, ha, wa = logical_shape(aq)
    nb, cb, h, w = logical_shape(bq)
    if nb != n or (ha * fh, wa * fw) != (h, w):
        raise ValueError("concat: shapes differ off the axis: %s (x%d, x%d) vs %s" % ((n, ca, ha, wa), fh, fw, (nb, cb, h, w)))
    y = _carry_fold(_new_q4(n, ca + cb, h, w, aq.ctx), bq)
    _lib.call("pl_concat2_q4_f32", aq.ctx.handle, aq.ptr, bq.ptr, y.ptr, n, ca, cb, h, w, fh, fw)
    return y


# kind -> Q4 implementation, for plan.assign_layouts (conv kinds are handled by the plan compiler)
Q4_LAYERS = {"maxpool": MaxpoolQ4, "averagepool": AveragePoolQ4, "gap": GlobalAveragePoolQ4,
             "upsample": UpSampleQ4, "batchnorm": BatchNormQ4, "relu": ReLUQ4, "leakyrelu": LeakyReLUQ4,
             "sigmoid": SigmoidQ4, "add": AddQ4, "concat": ConcatenateQ4, "clip": ClipQ4,
             "instancenormalization": InstanceNormQ4, "pad": PadQ4, "resize": ResizeQ4, "pixelshuffle": PixelShuffleQ4,
             "groupnorm": GroupNormQ4}


def register(layer_map):
    """Plan-internal kinds (never present in a user's IR)."""
    layer_map.update({"to_q4": to_q4, "from_q4": from_q4, "refold_q4": refold_q4, "conv_q4": ConvQ4, "convt_q4": ConvTransposeQ4, "upconcat_q4": UpConcatQ4,
                      "wino4_in": Wino4In, "wino4_gemm": Wino4Gemm, "wino4_out": Wino4Out, "wino4_chain": Wino4Chain,
                      "conv_q4_pair": ConvQ4Pair, "conv_pool_q4": ConvPoolQ4, "conv1x1_wino_in": Conv1x1WinoIn,
                      "upsample_add_q4": UpSampleAddQ4, "resize_add_q4": ResizeAddQ4,
                      "wino43_in": Wino43In, "wino43_gemm": Wino43Gemm, "wino43_out": Wino43Out, "wino43_chain": Wino43Chain})
    layer_map.update({k + "_q4": f for k, f in Q4_LAYERS.items()})

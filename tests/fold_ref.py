"""Pixel-phase folding in numpy: the definition that q4.refold_q4 / pl_refold_q4_f32 and plan.fold_dilated are tested against.

The (N, C, H, W) array folded by (dh, dw) is (N dh dw, C, ceil(H/dh), ceil(W/dw)): image (n dh + i) dw + j holds
x[n, :, i::dh, j::dw], zero where the phase is shorter than the folded map.  A 3x3 / stride 1 conv with dilation (dh, dw) and pads
(dh, dw, dh, dw) on x equals the 3x3 / pad 1 / dilation 1 conv on fold_np(x), unfolded again (the zero cells stand in for the
conv's own padding; what the conv writes there is dropped by unfold_np)."""
import numpy as np


def folded_shape(shape, dh, dw):
    n, c, h, w = shape
    return (n * dh * dw, c, -(-h // dh), -(-w // dw))


def fold_np(x, dh, dw):
    n, c, h, w = x.shape
    _, _, hf, wf = folded_shape(x.shape, dh, dw)
    y = np.zeros((n, dh, dw, c, hf, wf), x.dtype)
    for i in range(dh):
        for j in range(dw):
            p = x[:, :, i::dh, j::dw]
            y[:, i, j, :, :p.shape[2], :p.shape[3]] = p
    return y.reshape(n * dh * dw, c, hf, wf)


def unfold_np(y, dh, dw, h, w):
    """The (N, C, h, w) array whose fold by (dh, dw) is `y`; the zero-fill cells of `y` are not read."""
    nf, c, hf, wf = y.shape
    assert nf % (dh * dw) == 0 and (hf, wf) == (-(-h // dh), -(-w // dw)), (y.shape, dh, dw, h, w)
    n = nf // (dh * dw)
    y = y.reshape(n, dh, dw, c, hf, wf)
    x = np.empty((n, c, h, w), y.dtype)
    for i in range(dh):
        for j in range(dw):
            rows, cols = len(range(i, h, dh)), len(range(j, w, dw))
            x[:, :, i::dh, j::dw] = y[:, i, j, :, :rows, :cols]
    return x


def refold_np(y, src, dst, h, w):
    """`y` folded by `src` -> the same (N, C, h, w) array folded by `dst`."""
    return fold_np(unfold_np(y, src[0], src[1], h, w), dst[0], dst[1])


def tail_mask(shape, dh, dw):
    """True at the zero-fill cells of the (N, C, H, W) = `shape` array folded by (dh, dw)."""
    return ~fold_np(np.ones(shape, bool), dh, dw)


def to_q4_np(x):
    """(N, C, H, W) -> the channel-quad array (N, ceil(C/4), H, W, 4), padding lanes zero."""
    n, c, h, w = x.shape
    cq = -(-c // 4)
    y = np.zeros((n, cq * 4, h, w), x.dtype)
    y[:, :c] = x
    return np.ascontiguousarray(y.reshape(n, cq, 4, h, w).transpose(0, 1, 3, 4, 2))


def from_q4_np(q, c):
    n, cq, h, w, _ = q.shape
    return np.ascontiguousarray(q.transpose(0, 1, 4, 2, 3).reshape(n, cq * 4, h, w)[:, :c])

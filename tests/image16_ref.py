"""numpy mirror of the uint16 / percentile-scaled image input (pl_image_u16_nchw_f32, pl_image_norm_nchw_f32):
np.sort per plane, the lerp and the affine in float64 with every operation rounded on its own, the decode in float32."""
import math

import numpy as np

from tests.image_input_ref import axis_samples, pick


def ranks(m, q):
    """(j, j1, g) of percentile q among m sorted samples: numpy's linear rule."""
    v = q / 100 * (m - 1)
    j = math.floor(v)
    return j, min(j + 1, m - 1), v - j


def percentiles(planes, lo, hi):
    """(..., H, W) integer planes -> (p_lo, p_hi) float64 per plane."""
    s = np.sort(planes.reshape(planes.shape[:-2] + (-1,)), axis=-1).astype(np.float64)

    def p(q):
        j, j1, g = ranks(s.shape[-1], q)
        return s[..., j] + (s[..., j1] - s[..., j]) * g
    return p(lo), p(hi)


def affine(x, k, b, layout, order, normalise):
    """(kk, bb), float32 (N, Co): the multiplier and the offset of every image and output channel."""
    k, b = np.asarray(k, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    n = np.asarray(x).shape[0]
    if normalise is None:
        return np.tile(k.astype(np.float32), (n, 1)), np.tile(b.astype(np.float32), (n, 1))
    p_lo, p_hi = percentiles(pick(x, layout, order), *normalise[1:])
    d = p_hi - p_lo
    d = np.where(d > 0, d, 1.0)
    K = k[None] / d
    return K.astype(np.float32), (b[None] - p_lo * K).astype(np.float32)


def resize32(img, size):
    """tests/image_input_ref.resize32 for any integer image: util.resize in float32, every product and sum rounded on its own."""
    ra, rs = axis_samples(img.shape[0], size[0])
    ca, cs = axis_samples(img.shape[1], size[1])
    gr, gc = np.float32(1) - rs, np.float32(1) - cs
    p = img.astype(np.float32)
    t = p[:, ca] * gc[None, :, None] + p[:, ca + 1] * cs[None, :, None]
    return t[ra] * gr[:, None, None] + t[ra + 1] * rs[:, None, None]


def decode32(x, k, b, layout="nhwc", order=None, size=None, normalise=None):
    """The contract restated: float32 (N, Co, OH, OW).  The percentiles are those of the SOURCE planes."""
    kk, bb = affine(x, k, b, layout, order, normalise)
    r = pick(x, layout, order).astype(np.float32) if size is None else pick(np.stack([resize32(im, size) for im in x]), "nhwc", order)
    y = r * kk[:, :, None, None] + bb[:, :, None, None]
    assert y.dtype == np.float32
    return y

"""numpy mirror of pl_peaks_f32: the 3 x 3 local maxima above a threshold of every plane of float32 heat maps
(N, K, H, W), counted, and the best max_peaks of each plane as [x, y, score] rows.  Everything is exact: floats compare as bits.

`peak_mask` pads with -inf and compares shifted views; `peaks_ref` orders a plane's peaks with a stable sort of the negated
scores over the ascending raster indices (tests/test_peaks_ref.py holds both to independent formulations).  The pattern
generators return float32 (N, K, H, W)."""
import numpy as np

F32, I32 = np.float32, np.int32
NINF = F32(-np.inf)


def peak_mask(x, threshold=0.0, ties="all"):
    """bool like x (N, K, H, W): pixel p is a peak iff x[p] > threshold and, against each neighbour q of its plane, x[p] >= x[q]
    ("all"), or x[p] > x[q] where q < p in raster order and x[p] >= x[q] where q > p ("first").  float32 comparisons."""
    x = np.asarray(x)
    assert x.dtype == F32 and x.ndim == 4 and ties in ("all", "first")
    n, k, h, w = x.shape
    pad = np.full((n, k, h + 2, w + 2), NINF, F32)        # -inf: every comparison against it holds where the pixel can be a peak
    pad[:, :, 1:h + 1, 1:w + 1] = x
    with np.errstate(invalid="ignore"):
        pk = x > F32(threshold)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy == 0 and dx == 0:
                    continue
                q = pad[:, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                before = dy < 0 or (dy == 0 and dx < 0)
                pk &= (x > q) if ties == "first" and before else (x >= q)
    return pk


def _nudge(v, idx, pos, extent, step):
    """The quarter-pixel offsets of the peaks at flat indices idx of plane v along one axis (pos: their coordinate there)."""
    d = np.zeros(idx.size, F32)
    inner = (pos > 0) & (pos < extent - 1)
    flat = v.ravel()
    lo, hi = flat[idx[inner] - step], flat[idx[inner] + step]
    with np.errstate(invalid="ignore"):
        d[inner] = np.where(hi > lo, F32(0.25), np.where(hi < lo, F32(-0.25), F32(0)))
    return d


def peaks_ref(x, threshold=0.0, ties="all", max_peaks=32, refine="none", stride=(1.0, 1.0)):
    """(peaks float32 (N, K, max_peaks, 3), num int32 (N, K)) of float32 x (N, K, H, W)."""
    x = np.asarray(x)
    assert refine in ("none", "quarter") and max_peaks >= 1
    n, k, h, w = x.shape
    sy, sx = (F32(s) for s in (stride if isinstance(stride, (tuple, list)) else (stride, stride)))
    pk = peak_mask(x, threshold, ties)
    peaks, num = np.zeros((n, k, max_peaks, 3), F32), np.zeros((n, k), I32)
    for i in range(n):
        for j in range(k):
            v = x[i, j]
            idx = np.flatnonzero(pk[i, j])                # ascending p
            num[i, j] = idx.size
            score = v.ravel()[idx]
            idx = idx[np.argsort(-score, kind="stable")][:max_peaks]      # (-(-0.0) == -(+0.0): they stay in raster order)
            py, px = idx // w, idx % w
            dy = dx = np.zeros(idx.size, F32)
            if refine == "quarter":
                dx, dy = _nudge(v, idx, px, w, 1), _nudge(v, idx, py, h, w)
            peaks[i, j, :idx.size, 0] = (px.astype(F32) + dx) * sx
            peaks[i, j, :idx.size, 1] = (py.astype(F32) + dy) * sy
            peaks[i, j, :idx.size, 2] = v.ravel()[idx]
    return peaks, num


# ---- patterns ---------------------------------------------------------------------------------------------------------------
def random_maps(n, k, h, w, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (n, k, h, w)).astype(F32)


def quantised(n, k, h, w, seed):
    """Four levels, -0.25 to 0.5: plateaus everywhere."""
    return (np.random.default_rng(seed).integers(0, 4, (n, k, h, w)).astype(F32) - 1) / F32(4)


def smooth_quantised(n, k, h, w, seed):
    """Four levels in blocks of 3 x 2 pixels: plateaus of several pixels, many of them across a seam."""
    q = quantised(n, k, -(-h // 3), -(-w // 2), seed)
    return np.ascontiguousarray(np.repeat(np.repeat(q, 3, 2), 2, 3)[:, :, :h, :w])


def constant(n, k, h, w, value=0.5):
    return np.full((n, k, h, w), value, F32)


def seams(n, k, h, w, th, tw, seed):
    """Noise below 0.5, and the value 1 on either side of every tile seam (pairs every fifth row or column) and on the 2 x 2
    pixels around every tile corner."""
    x = (np.random.default_rng(seed).uniform(0, 0.5, (n, k, h, w))).astype(F32)
    for s in range(tw, w, tw):
        x[:, :, 1::5, s - 1:s + 1] = 1
    for s in range(th, h, th):
        x[:, :, s - 1:s + 1, 2::5] = 1
    for sy in range(th, h, th):
        for sx in range(tw, w, tw):
            x[:, :, sy - 1:sy + 1, sx - 1:sx + 1] = 1
    return x


def borders(n, k, h, w):
    """-1 everywhere, distinct positive values in the plane's corners and in the middle of its edges."""
    x = np.full((n, k, h, w), -1, F32)
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)]
    for i, (y, xx) in enumerate(spots):
        x[:, :, y, xx] = np.maximum(x[:, :, y, xx], F32(1 + i / 8))
    return x


def with_nan(n, k, h, w, th, tw, seed):
    """Random values, one pixel in sixteen NaN, and NaN on either side of the tile seams every third row or column."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (n, k, h, w)).astype(F32)
    x[rng.random((n, k, h, w)) < 1 / 16] = np.nan
    for s in range(tw, w, tw):
        x[:, :, 0::3, s - 1] = np.nan
        x[:, :, 1::3, s] = np.nan
    for s in range(th, h, th):
        x[:, :, s - 1, 0::3] = np.nan
        x[:, :, s, 1::3] = np.nan
    return x


def with_inf(n, k, h, w, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (n, k, h, w)).astype(F32)
    r = rng.random((n, k, h, w))
    x[r < 0.05] = np.inf
    x[r > 0.9] = -np.inf
    return x


def zeros_mixed(n, k, h, w, seed):
    """-0.0 and +0.0 at random: one plateau."""
    x = np.zeros((n, k, h, w), F32)
    x[np.random.default_rng(seed).random((n, k, h, w)) < 0.5] = F32(-0.0)
    return x


def lattice(n, k, h, w, step=3):
    """0 everywhere, the value 1 on every step-th pixel of every step-th row: equal isolated peaks in every tile."""
    x = np.zeros((n, k, h, w), F32)
    x[:, :, ::step, ::step] = 1
    return x

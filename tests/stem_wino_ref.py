"""Host reference of the polyphase F(4,4) stem form (csrc/conv_stem_wino_kernel.h): its matrices, an emulation of its arithmetic
in a chosen precision, and the per-element error bound its tests use.

The 7x7 / stride 2 / pad 3 conv on 3 channels: conv column j reads padded columns 2 j + v, so taps v = 0, 2, 4, 6 are a 4-tap
stride-1 correlation over the even padded columns and v = 1, 3, 5 (+ a zero tap) one over the odd ones.  Both run as F(4,4) on the
nodes 0, 1, -1, 2, -2, 1/2, inf; the products are summed over k = (filter row, channel, phase) per frequency, then one A^T.

Bound of an output element, from the absolute values of everything that enters it (u = 2^-24):
    tol = lam * u * |scale| * W + 4 u (|scale| (conv(|x|, |K|) + |B|) + |shift|),   W = |A^T| sum_k (|G| |g_k|) * (|B^T| |d_k|)
LAMBDA is 4x the worst err / (u W) of the float32 emulation below over `calibration_cases` (the kernel sums in another order),
rounded up: the worst ratio is 0.846 (case "he224"; skewed operands 0.727, with an offset of 50 0.375), so LAMBDA = 3.5.
"""
import numpy as np

from oracle import planer_np as onp
from tests import ref64 as R

U = 2.0 ** -24
CONV = dict(group=1, strides=[2, 2], dilations=[1, 1], pads=[3, 3, 3, 3])
POOL = dict(w=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2])

AT = np.array([[1, 1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 1 / 2, 0], [0, 1, 1, 4, 4, 1 / 4, 0], [0, 1, -1, 8, -8, 1 / 8, 1]], float)
G = np.array([[-1 / 2, 0, 0, 0], [-1 / 3, -1 / 3, -1 / 3, -1 / 3], [1 / 9, -1 / 9, 1 / 9, -1 / 9], [1 / 36, 1 / 18, 1 / 9, 2 / 9],
              [-1 / 60, 1 / 30, -1 / 15, 2 / 15], [32 / 45, 16 / 45, 8 / 45, 4 / 45], [0, 0, 0, 1]], float)
BT = np.array([[-2, 4, 5 / 2, -5, -1 / 2, 1, 0], [0, 2, -2, -9 / 2, 1 / 2, 1, 0], [0, -2, 6, -7 / 2, -3 / 2, 1, 0],
               [0, 1, -3 / 2, -2, 3 / 2, 1, 0], [0, -1, 5 / 2, 0, -5 / 2, 1, 0], [0, 4, 0, -5, 0, 1, 0],
               [0, -2, 4, 5 / 2, -5, -1 / 2, 1]], float)
LAMBDA = 3.5


def filter_phases(K):
    """OIHW [Cout][3][7][7] -> g[Cout][c][fr][phase][4 taps]: even columns, odd columns + a zero."""
    K = np.asarray(K)
    g = np.zeros(K.shape[:3] + (2, 4), K.dtype)
    g[..., 0, :] = K[..., 0::2]
    g[..., 1, :3] = K[..., 1::2]
    return g


def filter_freq(K, dtype=np.float64, mat=G):
    """G g: [Cout][c][fr][phase][7 f]."""
    return np.einsum("fa,ocrpa->ocrpf", mat.astype(dtype), filter_phases(K).astype(dtype)).astype(dtype)


def _tiles(x):
    """d[N][c][padded row][phase][tile][7]: the input segments of every tile of 4 conv columns."""
    n, c, h, w = x.shape
    wo = (w + 6 - 7) // 2 + 1
    t = -(-wo // 4)
    xp = np.zeros((n, c, h + 6, 2 * (4 * t + 3)), x.dtype)
    xp[:, :, 3:3 + h, 3:3 + w] = x
    ph = np.stack([xp[..., 0::2], xp[..., 1::2]], axis=3)                     # [n][c][row][phase][column of the phase]
    idx = 4 * np.arange(t)[:, None] + np.arange(7)[None, :]
    return ph[..., idx], wo


def _rows(d, ho):
    """[n][c][row][...] -> [n][c][fr][conv row][...]: padded row 2 r + fr."""
    return d[:, :, np.arange(7)[:, None] + 2 * np.arange(ho)[None, :]]


def emulate(x, K, dtype=np.float32):
    """The conv as the kernel runs it, every transform and sum in `dtype` -> [N][Cout][Ho][Wo]."""
    x, K = np.asarray(x, dtype), np.asarray(K, dtype)
    ho = (x.shape[2] + 6 - 7) // 2 + 1
    d, wo = _tiles(x)
    v = np.einsum("fm,ncrptm->ncrptf", BT.astype(dtype), d).astype(dtype)
    u = filter_freq(K, dtype)
    m = np.einsum("ocrpf,ncrhptf->nohtf", u, _rows(v, ho)).astype(dtype)
    y = np.einsum("if,nohtf->nohti", AT.astype(dtype), m).astype(dtype)
    return y.reshape(y.shape[0], y.shape[1], ho, -1)[..., :wo]


def weight(x, K):
    """W of the module docstring, float64 -> [N][Cout][Ho][Wo]."""
    x, K = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(K, np.float64))
    ho = (x.shape[2] + 6 - 7) // 2 + 1
    d, wo = _tiles(x)
    v = np.einsum("fm,ncrptm->ncrptf", np.abs(BT), d)
    u = filter_freq(K, np.float64, np.abs(G))
    m = np.einsum("ocrpf,ncrhptf->nohtf", u, _rows(v, ho))
    y = np.einsum("if,nohtf->nohti", np.abs(AT), m)
    return y.reshape(y.shape[0], y.shape[1], ho, -1)[..., :wo]


def bound(x, K, B=None, scale=None, shift=None, lam=LAMBDA):
    """Per-element tolerance of the conv + fused tail (module docstring)."""
    s = np.abs(R._chan(scale)) if scale is not None else 1.0
    lin = R.conv64(np.abs(x), np.abs(K), **CONV)
    if B is not None:
        lin = lin + np.abs(R._chan(B))
    lin = s * lin
    if shift is not None:
        lin = lin + np.abs(R._chan(shift))
    return lam * U * s * weight(x, K) + 4 * U * lin


def pooled(a):
    """The oracle's max-pool (3x3 / stride 2 / pad 1, zero padding, running maximum from -1e4) of a float64 map; of a bound:
    the largest bound in each window."""
    return onp.maxpool(np.asarray(a, np.float64), **POOL)


def calibration_cases():
    """(name, x, K): N(0,1) images under He-normal filters at real size, and the skewed operands of the conv bound tests."""
    rng = np.random.default_rng(4404)
    x = rng.standard_normal((2, 3, 224, 224)).astype(np.float32)
    K = (rng.standard_normal((64, 3, 7, 7)) * np.sqrt(2.0 / 147)).astype(np.float32)
    yield "he224", x, K
    for dc in (0.0, 50.0):
        xs, Ks, _ = R.skewed_operands(rng, (1, 3, 40, 224), (36, 3, 7, 7), dc=dc)
        yield "skewed dc %g" % dc, xs, Ks


def emulation_ratio(x, K):
    """Worst err / (u W) of the float32 emulation against the float64 conv."""
    err = np.abs(emulate(x, K).astype(np.float64) - R.conv64(x, K, **CONV))
    return float((err / (U * weight(x, K))).max())

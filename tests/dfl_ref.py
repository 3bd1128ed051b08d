"""Anchor-free heads and prototype masks: float64 mirrors of pl_dfl_decode_f32 and pl_proto_masks_f32.  numpy only;
the order, NMS and tolerance helpers are tests/detect_ref.py's.

`decode64`: head h is float32 (N, 4 R + C + Md, Gh, Gw); class = np.argmax of the C logits, score = s(logit[class]), a candidate
iff score > conf; per side d = sum_j j e_j / sum_j e_j with e_j = exp(t_j - fmax_j t_j); box = ((gx + .5 - d_l) sx,
(gy + .5 - d_t) sy, (gx + .5 + d_r) sx, (gy + .5 + d_b) sy).  Anchor index = heads in order, then gy Gw + gx.

The box bound, from the operation count (u = 2^-24; the test's logits are multiples of 1/4, so t_j - m is exact in float32):
every e_j is off by at most 2 ulp <= 4u of itself, fl(j e_j) adds u, each of the R additions of a sum adds u, and all terms are
non-negative, so the numerator is within rn = (1 + 4u)(1 + u)^(R + 1) - 1 of itself and the denominator within
rd = (1 + 4u)(1 + u)^R - 1; the division adds u:  |err d| <= rho d,  rho = (1 + rn)(1 + u) / (1 - rd) - 1, plus R^2 2^-126 for
terms that run out of exponent.  fl(g + 0.5) is exact; a = fl(g + .5 -+ d) adds sp(a), fl(a s) adds sp(box):
    tol = (rho d + sp(a)) s + sp(box)          (sp: detect_ref's float32 spacing, which covers one rounding)
A reference value that is not finite has no tolerance (detect_ref.close): that infinity, or a NaN for a NaN.

`masks64`: the crop is float32 arithmetic, reproduced exactly; inside it a bit is decided where the float64 logit exceeds the
worst float32 error of an Md-term dot product in any order, |logit| > gamma sum_k |coef proto|, gamma = (Md + 1) u / (1 - (Md + 1) u)."""
import numpy as np

from tests import detect_ref as R

F32, U = np.float32, 2.0 ** -24


def decode64(xs, heads, classes, md, conf):
    """heads[h] = (R, (sx, sy)).  -> dict over (N, total): score, cls, cand, and box, tol_box over (N, total, 4)."""
    out = {k: [] for k in ("score", "cls", "box", "tol_box")}
    with np.errstate(all="ignore"):
        for x, (r, (sx, sy)) in zip(xs, heads):
            n, ch, gh, gw = x.shape
            assert ch == 4 * r + classes + md
            x = np.asarray(x, F32).reshape(n, ch, gh * gw)
            logits = x[:, 4 * r:4 * r + classes]
            cls = np.argmax(logits, axis=1)                                     # numpy's rule on the float32 logits
            out["cls"].append(cls)
            out["score"].append(R.sigmoid64(np.take_along_axis(logits, cls[:, None], 1)[:, 0]))
            t = x[:, :4 * r].astype(np.float64).reshape(n, 4, r, gh * gw)
            e = np.exp(t - np.fmax.reduce(t, axis=2, keepdims=True))
            d = (np.arange(r)[None, None, :, None] * e).sum(2) / e.sum(2)       # (n, 4, cells)
            rn, rd = (1 + 4 * U) * (1 + U) ** (r + 1) - 1, (1 + 4 * U) * (1 + U) ** r - 1
            ed = ((1 + rn) * (1 + U) / (1 - rd) - 1) * d + r * r * 2.0 ** -126
            cell = np.arange(gh * gw)
            g = np.stack([cell % gw, cell // gw, cell % gw, cell // gw]) + 0.5
            a = g + np.array([-1.0, -1.0, 1.0, 1.0])[:, None] * d
            s = np.array([sx, sy, sx, sy], np.float64)[:, None]
            out["box"].append((a * s).transpose(0, 2, 1))
            out["tol_box"].append(((ed + R.sp(a)) * s + R.sp(a * s)).transpose(0, 2, 1))
    out = {k: np.concatenate(v, axis=1) for k, v in out.items()}
    out["cand"] = out["score"] > float(F32(conf))
    return out


def crop32(det, num, ph, pw, size):
    """(N, max_det, Ph, Pw) bool: d < num[n] and the pixel inside the box at prototype scale, in float32 as the kernel does it."""
    det = np.asarray(det, F32)
    kx, ky = F32(pw / size[1]), F32(ph / size[0])
    with np.errstate(all="ignore"):
        x1, y1, x2, y2 = ((det[:, :, j] * k)[:, :, None, None] for j, k in enumerate((kx, ky, kx, ky)))
        x, y = np.arange(pw, dtype=F32)[None, None, None, :], np.arange(ph, dtype=F32)[None, None, :, None]
        live = (np.arange(det.shape[1])[None, :] < np.asarray(num)[:, None])[:, :, None, None]
        return live & (x1 <= x) & (x < x2) & (y1 <= y) & (y < y2)


def masks64(det, num, coef, protos, size):
    """-> (inside, positive, decided), bool (N, max_det, Ph, Pw): the crop, the float64 sign, and where that sign binds."""
    n, md, ph, pw = protos.shape
    c, p = np.asarray(coef, np.float64), np.asarray(protos, np.float64).reshape(n, md, -1)
    logit, mag = np.einsum("ndk,nkp->ndp", c, p), np.einsum("ndk,nkp->ndp", np.abs(c), np.abs(p))
    gamma = (md + 1) * U / (1 - (md + 1) * U)
    shape = (n, c.shape[1], ph, pw)
    return crop32(det, num, ph, pw, size), (logit > 0).reshape(shape), (np.abs(logit) > gamma * mag).reshape(shape)

"""tests/peaks_ref.py, the numpy mirror of pl_peaks_f32, held to independent formulations: scipy's maximum filter
for ties="all", np.lexsort for the order, np.argmax for the single-peak case, a pixel loop for the contract's sentences."""
import numpy as np
import pytest

from tests import peaks_ref as R

F32 = np.float32
TH, TW = 4, 6                                   # (any seam positions serve the patterns here)


def maps():
    out = [("random", R.random_maps(2, 3, 9, 11, 1)), ("quantised", R.quantised(2, 2, 10, 13, 2)),
           ("smooth quantised", R.smooth_quantised(1, 2, 11, 9, 3)), ("constant", R.constant(1, 2, 5, 7)),
           ("seams", R.seams(1, 2, 11, 17, TH, TW, 4)), ("borders", R.borders(1, 1, 7, 9)), ("nan", R.with_nan(2, 2, 9, 14, TH, TW, 5)),
           ("inf", R.with_inf(2, 2, 9, 10, 6)), ("zeros", R.zeros_mixed(1, 2, 6, 7, 7)), ("lattice", R.lattice(1, 1, 10, 11)),
           ("one pixel", R.random_maps(1, 2, 1, 1, 8)), ("one row", R.quantised(1, 2, 1, 12, 9)), ("one column", R.quantised(1, 2, 12, 1, 10))]
    return out


def loop_mask(x, threshold, ties):
    """The contract's sentences, pixel by pixel, in Python floats (a float32 compares as its double)."""
    n, k, h, w = x.shape
    out = np.zeros(x.shape, bool)
    t = float(F32(threshold))
    for i in range(n):
        for j in range(k):
            v = x[i, j].tolist()
            for y in range(h):
                for xx in range(w):
                    c = v[y][xx]
                    ok = c > t
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            yy, xq = y + dy, xx + dx
                            if (dy, dx) == (0, 0) or not (0 <= yy < h and 0 <= xq < w):
                                continue
                            q = v[yy][xq]
                            if ties == "first" and yy * w + xq < y * w + xx:
                                ok = ok and c > q
                            else:
                                ok = ok and c >= q
                    out[i, j, y, xx] = ok
    return out


@pytest.mark.parametrize("ties", ["all", "first"])
def test_mask_equals_the_pixel_loop(ties):
    for name, x in maps():
        for t in (0.0, -1.0, -np.inf, 0.3):
            assert (R.peak_mask(x, t, ties) == loop_mask(x, t, ties)).all(), (name, t)


def test_all_is_the_maximum_filter_idiom():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, x in maps():
        if np.isnan(x).any():                   # (the filter's answer around a NaN depends on its scan order)
            continue
        for t in (0.0, -1.0, 0.3):
            with np.errstate(invalid="ignore"):
                want = np.stack([[(ndimage.maximum_filter(p, 3, mode="constant", cval=-np.inf) == p) & (p > F32(t)) for p in img] for img in x])
            assert (R.peak_mask(x, t, "all") == want).all(), (name, t)


@pytest.mark.parametrize("ties", ["all", "first"])
def test_order_is_lexsort_on_index_and_negated_score(ties):
    for name, x in maps():
        n, k, h, w = x.shape
        for mp in (1, 3, 200):
            peaks, num = R.peaks_ref(x, -1.0, ties, mp, "none", (1, 1))
            pk = R.peak_mask(x, -1.0, ties)
            for i in range(n):
                for j in range(k):
                    idx = np.flatnonzero(pk[i, j])
                    score = x[i, j].ravel()[idx]
                    idx = idx[np.lexsort((idx, -score))][:mp]
                    assert num[i, j] == pk[i, j].sum()
                    m = idx.size
                    assert (peaks[i, j, :m, 0] == idx % w).all() and (peaks[i, j, :m, 1] == idx // w).all(), (name, mp)
                    assert peaks[i, j, :m, 2].tobytes() == x[i, j].ravel()[idx].tobytes(), (name, mp)        # the pixel's own bits
                    assert not peaks[i, j, m:].view(np.uint32).any(), (name, mp)                             # +0.0 behind
    assert not np.isnan(peaks).any()


def test_single_first_peak_is_argmax():
    for name, x in maps():
        if np.isnan(x).any() or not (x.max(axis=(2, 3)) > -np.inf).all():
            continue
        n, k, h, w = x.shape
        peaks, num = R.peaks_ref(x, -np.inf, "first", 1, "none", (1, 1))
        am = x.reshape(n, k, -1).argmax(2)
        assert (num >= 1).all(), name
        assert (peaks[:, :, 0, 0] == am % w).all() and (peaks[:, :, 0, 1] == am // w).all(), name
        assert peaks[:, :, 0, 2].tobytes() == np.take_along_axis(x.reshape(n, k, -1), am[..., None], 2).tobytes(), name


def test_first_is_a_subset_of_all_without_equal_neighbours():
    for name, x in maps():
        for t in (0.0, -1.0):
            a, f = R.peak_mask(x, t, "all"), R.peak_mask(x, t, "first")
            assert not (f & ~a).any(), name
            n, k, h, w = x.shape
            for i, j, y, xx in zip(*np.nonzero(f)):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        yy, xq = y + dy, xx + dx
                        if (dy, dx) != (0, 0) and 0 <= yy < h and 0 <= xq < w and f[i, j, yy, xq]:
                            assert x[i, j, yy, xq] != x[i, j, y, xx], (name, y, xx)
    # a constant plane: every pixel under "all", the first under "first"
    c = R.constant(1, 1, 5, 7)
    assert R.peak_mask(c, 0.0, "all").all() and np.flatnonzero(R.peak_mask(c, 0.0, "first")).tolist() == [0]


def test_refinement_and_stride_by_hand():
    x = np.zeros((1, 1, 5, 6), F32)
    x[0, 0, 2, 3], x[0, 0, 2, 4], x[0, 0, 1, 3] = 2, 1, 0.5           # right > left: +0.25; below (0) < above (0.5): -0.25
    x[0, 0, 4, 0] = 3                                                  # on the border: no nudge along either axis it borders
    x[0, 0, 4, 1] = 1
    peaks, num = R.peaks_ref(x, 0.0, "all", 4, "quarter", (7.5, 3.3))
    assert num.tolist() == [[2]]
    assert peaks[0, 0, 0].tolist() == [0.0, float(F32(4) * F32(7.5)), 3.0]
    assert peaks[0, 0, 1].tolist() == [float(F32(3.25) * F32(3.3)), float(F32(1.75) * F32(7.5)), 2.0]
    assert not peaks[0, 0, 2:].view(np.uint32).any()
    plain = R.peaks_ref(x, 0.0, "all", 4, "none", 4)[0]
    assert plain[0, 0, :2].tolist() == [[0.0, 16.0, 3.0], [12.0, 8.0, 2.0]]
    # a NaN neighbour decides nothing; -0.0 keeps its sign in the score and ties with +0.0 in the order
    x = np.array([[[[-0.0, -2, 0.0, -2, -0.0]]]], F32)
    peaks, num = R.peaks_ref(x, -1.0, "all", 3, "quarter", 1)
    assert num.tolist() == [[3]] and peaks[0, 0, :, 0].tolist() == [0, 2, 4]
    assert np.signbit(peaks[0, 0, :, 2]).tolist() == [True, False, True]

"""tests/components_ref.py against scipy.ndimage where it is installed, and on hand-worked maps.  No GPU."""
import numpy as np
import pytest

from tests import components_ref as R

STRUCT = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: [[1, 1, 1]] * 3}
SHAPES = [(1, 1), (5, 7), (31, 63), (33, 65), (40, 9)]


def _binary_maps(h, w):
    yield from (R.random_binary(1, h, w, d, 3)[0] for d in (0.3, 0.5, 0.6))
    for f in (R.checkerboard, R.serpentine, R.comb, R.diagonal, R.row_ends, R.image_ends):
        yield (f(1, h, w)[0] > 0).astype(np.uint8)
    yield np.zeros((h, w), np.uint8)
    yield np.ones((h, w), np.uint8)


def _renumber(stacked):
    """Labellings of disjoint pixel sets (0 elsewhere), each numbered from 1 -> one numbering by first raster pixel."""
    key = np.zeros(stacked[0].shape, np.int64)
    for i, lab in enumerate(stacked):
        key = np.where(lab > 0, lab.astype(np.int64) + (i << 32), key)
    flat = key.ravel()
    ids, first = np.unique(flat[flat > 0], return_index=True)
    pos = np.flatnonzero(flat > 0)[first]
    rank = np.empty(len(ids), np.int64)
    rank[np.argsort(pos)] = np.arange(1, len(ids) + 1)
    out = np.zeros(flat.shape, np.int32)
    out[flat > 0] = rank[np.searchsorted(ids, flat[flat > 0])]
    return out.reshape(key.shape)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_binary_maps_equal_scipy_label(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    for h, w in SHAPES:
        for m in _binary_maps(h, w):
            want, count = ndimage.label(m, structure=STRUCT[connectivity])
            labels, num = R.label_ref(m, connectivity, 0)
            assert num == count and labels.dtype == np.int32
            np.testing.assert_array_equal(labels, want)                   # the labels, not merely the partition


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("background", [0, 2, -1])
def test_class_maps_equal_scipy_per_class_renumbered(connectivity, background):
    ndimage = pytest.importorskip("scipy.ndimage")
    for h, w in SHAPES:
        for m in (R.random_classes(1, h, w, 3, 5)[0], R.rings(1, h, w)[0], R.comb(1, h, w)[0]):
            per_class = [ndimage.label(m == c, structure=STRUCT[connectivity])[0] for c in range(256) if c != background and (m == c).any()]
            want = _renumber(per_class) if per_class else np.zeros(m.shape, np.int32)
            labels, num = R.label_ref(m, connectivity, background)
            np.testing.assert_array_equal(labels, want)
            assert num == want.max()


def test_hand_worked_map():
    m = np.array([[1, 0, 2, 2],
                  [0, 1, 0, 2],
                  [3, 0, 1, 0]], np.uint8)
    l8, n8 = R.label_ref(m, 8, 0)
    assert n8 == 3 and l8.tolist() == [[1, 0, 2, 2], [0, 1, 0, 2], [3, 0, 1, 0]]
    l4, n4 = R.label_ref(m, 4, 0)
    assert n4 == 5 and l4.tolist() == [[1, 0, 2, 2], [0, 3, 0, 2], [4, 0, 5, 0]]
    lb, nb = R.label_ref(m, 4, -1)                                         # the zeros are objects too: five of them
    assert nb == 10 and lb.tolist() == [[1, 2, 3, 3], [4, 5, 6, 3], [7, 8, 9, 10]]
    objects, centroids = R.regions_ref(m[None], l8[None], 4)
    assert objects[0].tolist() == [[1, 3, 0, 0, 3, 3], [2, 3, 0, 2, 2, 4], [3, 1, 2, 0, 3, 1], [0] * 6]
    assert centroids[0].tolist() == [[1, 1], [np.float32(1 / 3), np.float32(8 / 3)], [2, 0], [0, 0]]
    assert centroids.dtype == np.float32 and not np.signbit(centroids).any()
    objects, _ = R.regions_ref(m[None], l4[None], 2)                       # objects above max_objects have no row
    assert objects[0].tolist() == [[1, 1, 0, 0, 1, 1], [2, 3, 0, 2, 2, 4]]
    assert R.regions_ref(m[None], l4[None], 0)[0].shape == (1, 0, 6)


def test_patterns_and_answers():
    for h, w in ((33, 65), (7, 1), (1, 9), (2, 2), (66, 131)):
        labels, num = R.label_ref(R.serpentine(1, h, w)[0], 4, 0)
        assert num == 1 and (labels > 0).sum() == (h + 1) // 2 * w + h // 2
        assert R.label_ref(R.comb(1, h, w)[0], 4, 0)[1] == 1
        for m, labels, num in (R.lattice(h, w), R.stripes(h, w), R.serpentine_answer(h, w)):
            for connectivity in (4, 8):
                got, count = R.label_ref(m, connectivity, 0)
                np.testing.assert_array_equal(got, labels)
                assert (count == num).all()
    assert R.label_ref(R.checkerboard(1, 5, 7)[0], 4, 0)[1] == 18 and R.label_ref(R.checkerboard(1, 5, 7)[0], 8, 0)[1] == 1
    assert R.label_ref(R.diagonal(1, 9, 12)[0], 8, 0)[1] == 1 and R.label_ref(R.diagonal(1, 9, 12)[0], 4, 0)[1] == 9
    assert R.label_ref(R.row_ends(1, 6, 5)[0], 8, 0)[1] == 6               # rows do not join across the row break
    labels, num = R.label_ref(R.image_ends(3, 4, 5), 4, 0)
    assert num.tolist() == [2, 2, 2] and labels[:, 0].max() == 1 and labels[:, 3].min() == 2      # numbering restarts per image
    labels, num = R.label_ref(R.bridge(1, 9, 70, 64)[0], 4, 0)
    assert num == 1
    assert R.label_ref(R.bridge(1, 9, 70, 64)[0][:, :64], 4, 0)[1] == 2    # without the post: two bars

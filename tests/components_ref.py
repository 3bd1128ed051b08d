"""numpy mirror of pl_components_u8_i32: connected components of a uint8 class map, numbered per image by the
raster position of their first pixel, and the region table.  Everything is exact.

`label_ref` is the classic two-pass union-find with a Python loop over the pixels: for the small maps of the tests.  Maps too
large for that come with their answer (`lattice`, `stripes`, `serpentine` return the labels they must get); `regions_ref` is
vectorised and serves both."""
import numpy as np

I32 = np.int32


def _find(parent, i):
    r = i
    while parent[r] != r:
        r = parent[r]
    while parent[i] != r:
        parent[i], i = r, parent[i]
    return r


def _label_plane(m, connectivity, background):
    h, w = m.shape
    rows = m.tolist()
    parent = list(range(h * w))
    fg = [[c != background for c in row] for row in rows]
    steps = ((0, -1), (-1, 0)) if connectivity == 4 else ((0, -1), (-1, -1), (-1, 0), (-1, 1))
    for y in range(h):
        for x in range(w):
            if not fg[y][x]:
                continue
            c = rows[y][x]
            for dy, dx in steps:
                v, u = y + dy, x + dx
                if v < 0 or u < 0 or u >= w or rows[v][u] != c:
                    continue
                a, b = _find(parent, y * w + x), _find(parent, v * w + u)
                if a != b:                                # the smaller index stays the root: the object's first pixel
                    parent[max(a, b)] = min(a, b)
    root = np.array([_find(parent, i) for i in range(h * w)], np.int64).reshape(h, w)
    mask = np.array(fg, bool).reshape(h, w)
    labels = np.zeros((h, w), I32)
    firsts, inverse = np.unique(root[mask], return_inverse=True)      # ascending first pixels: the numbering
    labels[mask] = inverse + 1
    return labels, len(firsts)


def label_ref(m, connectivity=8, background=0):
    """(labels int32 like m, num int32 (N,)) of a uint8 class map (N, H, W) or (H, W) (then num is a number)."""
    m = np.asarray(m)
    assert m.dtype == np.uint8 and m.ndim in (2, 3) and connectivity in (4, 8) and -1 <= background <= 255
    if m.ndim == 2:
        labels, num = _label_plane(m, connectivity, background)
        return labels, I32(num)
    out = [_label_plane(p, connectivity, background) for p in m]
    labels = np.stack([o[0] for o in out]) if len(out) else np.zeros(m.shape, I32)
    return labels.reshape(m.shape), np.array([o[1] for o in out], I32)


def regions_ref(m, labels, max_objects):
    """(objects int32 (N, max_objects, 6), centroids float32 (N, max_objects, 2)) of class map m and its labels, both (N, H, W):
    row j is object j + 1, [class, area, y0, x0, y1, x1] and float32(float64(sum y) / float64(area)); unused rows are zero."""
    m, labels = np.asarray(m), np.asarray(labels)
    n, h, w = m.shape
    objects, centroids = np.zeros((n, max_objects, 6), I32), np.zeros((n, max_objects, 2), np.float32)
    for i in range(n):
        ys, xs = np.nonzero((labels[i] > 0) & (labels[i] <= max_objects))
        j = labels[i][ys, xs].astype(np.int64) - 1
        k = int(j.max()) + 1 if len(j) else 0
        area, sy, sx = (np.zeros(k, np.int64) for _ in range(3))
        np.add.at(area, j, 1), np.add.at(sy, j, ys), np.add.at(sx, j, xs)          # int64: exact
        y0, x0 = np.full(k, h, np.int64), np.full(k, w, np.int64)
        y1, x1 = np.zeros(k, np.int64), np.zeros(k, np.int64)
        np.minimum.at(y0, j, ys), np.minimum.at(x0, j, xs), np.maximum.at(y1, j, ys + 1), np.maximum.at(x1, j, xs + 1)
        cls = np.zeros(k, np.int64)
        cls[j] = m[i][ys, xs]
        assert (area > 0).all() and sy.max(initial=0) < 2 ** 53 and sx.max(initial=0) < 2 ** 53
        objects[i, :k] = np.stack([cls, area, y0, x0, y1, x1], 1)
        centroids[i, :k, 0] = (sy.astype(np.float64) / area.astype(np.float64)).astype(np.float32)
        centroids[i, :k, 1] = (sx.astype(np.float64) / area.astype(np.float64)).astype(np.float32)
    return objects, centroids


def components_ref(m, connectivity=8, background=0, max_objects=256):
    """The four arrays of the chain for m (N, H, W)."""
    labels, num = label_ref(m, connectivity, background)
    return (labels, num) + regions_ref(m, labels, max_objects)


# ---- patterns: uint8 (n, h, w) ---------------------------------------------------------------------------------------------
def random_binary(n, h, w, density, seed):
    return (np.random.default_rng(seed).random((n, h, w)) < density).astype(np.uint8)


def random_classes(n, h, w, classes, seed):
    return np.random.default_rng(seed).integers(0, classes, (n, h, w)).astype(np.uint8)


def full(n, h, w, value):
    return np.full((n, h, w), value, np.uint8)


def checkerboard(n, h, w):
    y, x = np.mgrid[:h, :w]
    return np.broadcast_to(((y + x) % 2 == 0).astype(np.uint8), (n, h, w)).copy()


def serpentine(n, h, w):
    """Every other row in full, joined alternately at the right and the left end: one object, area ceil(h / 2) w + h // 2."""
    m = np.zeros((n, h, w), np.uint8)
    m[:, 0::2] = 1
    for y in range(1, h, 2):
        m[:, y, w - 1 if (y // 2) % 2 == 0 else 0] = 1
    return m


def comb(n, h, w):
    """Teeth on every other column that meet only in the last row."""
    m = np.zeros((n, h, w), np.uint8)
    m[:, :, 0::2] = 3
    m[:, h - 1] = 3
    return m


def rings(n, h, w):
    y, x = np.mgrid[:h, :w]
    d = np.minimum(np.minimum(y, h - 1 - y), np.minimum(x, w - 1 - x))
    return np.broadcast_to((d % 2 + 1).astype(np.uint8), (n, h, w)).copy()


def diagonal(n, h, w):
    """The main diagonal, wrapping at the right edge (the wrap is no neighbourhood where w > 2)."""
    m = np.zeros((n, h, w), np.uint8)
    y = np.arange(h)
    m[:, y, y % w] = 1
    return m


def row_ends(n, h, w):
    """Even rows end in foreground, odd rows begin in it: raster neighbours across the row break, and no neighbours."""
    m = np.zeros((n, h, w), np.uint8)
    m[:, 0::2, w - 1] = 1
    m[:, 1::2, 0] = 1
    return m


def image_ends(n, h, w):
    """The last row of an image and the first row of the next in foreground."""
    m = np.zeros((n, h, w), np.uint8)
    m[:, 0] = 1
    m[:, h - 1] = 1
    return m


def bridge(n, h, w, tw):
    """Two bars in the first tile column that are joined only by a post in the second (w > tw, h >= 7)."""
    m = np.zeros((n, h, w), np.uint8)
    m[:, 2, 10:tw + 1] = 1
    m[:, 6, 10:tw + 1] = 1
    m[:, 2:7, tw] = 1
    return m


# ---- large maps with their answers -----------------------------------------------------------------------------------------
def lattice(h, w):
    """Isolated pixels on the even rows and columns: labels are their raster rank.  (m, labels, num), (1, h, w)."""
    m = np.zeros((1, h, w), np.uint8)
    m[:, 0::2, 0::2] = 1
    y, x = np.mgrid[:h, :w]
    cols = (w + 1) // 2
    labels = np.where(m[0] > 0, (y // 2) * cols + x // 2 + 1, 0).astype(I32)[None]
    return m, labels, np.array([((h + 1) // 2) * cols], I32)


def stripes(h, w):
    """Every other row in full: object k + 1 is row 2 k."""
    m = np.zeros((1, h, w), np.uint8)
    m[:, 0::2] = 7
    labels = np.where(m[0] > 0, np.arange(h)[:, None] // 2 + 1, 0).astype(I32)[None]
    return m, labels, np.array([(h + 1) // 2], I32)


def serpentine_answer(h, w):
    m = serpentine(1, h, w)
    return m, (m > 0).astype(I32), np.array([1], I32)

"""numpy mirror of pl_flow_instances_f32: instance masks by flow following.  The float32 operations of the step are
rounded one by one (numpy float32 arrays: one IEEE operation per expression, nothing contracted), everything behind them is
integer arithmetic.  The components step is tests/components_ref.py's.

`flow_ref` takes the planes as (N, C, H, W); the pattern generators below return such arrays with C == 3 (dy, dx, prob)."""
import numpy as np

from tests import components_ref as CR

F32, I32 = np.float32, np.int32


def _sign(v):
    return (v > 0).astype(np.int64) - (v < 0).astype(np.int64)


def step_ref(dy, dx, prob, level, min_flow):
    """(next int64 (H W,), fg bool (H W,)) of float32 planes (H, W): rule 1 and 2."""
    h, w = prob.shape
    dy, dx, prob = (np.ascontiguousarray(a, F32) for a in (dy, dx, prob))
    with np.errstate(all="ignore"):
        fg = prob > F32(level)                            # (a NaN compares false)
        ay, ax = dy * dy, dx * dx                         # float32 * float32 -> float32: one rounding each
        l2 = ay + ax
        g2 = F32(min_flow) * F32(min_flow)
        moves = fg & (l2 > g2)
        sy = np.where(F32(3) * ay >= ax, _sign(dy), 0)
        sx = np.where(F32(3) * ax >= ay, _sign(dx), 0)
    assert ay.dtype == F32 and l2.dtype == F32 and g2.dtype == F32
    y, x = np.mgrid[:h, :w]
    t = (np.clip(y + sy, 0, h - 1) * w + np.clip(x + sx, 0, w - 1)).ravel()
    p = np.arange(h * w, dtype=np.int64)
    fg = fg.ravel()
    return np.where(moves.ravel() & fg[t], t, p), fg


def table_ref(masks, max_instances):
    """(instances int32 (N, M, 5), centres float32 (N, M, 2)) of the final label maps (N, H, W): row j is instance j + 1,
    [area, y0, x0, y1, x1] and float32(float64(sum) / float64(area)); unused rows are zero."""
    n, h, w = masks.shape
    instances, centres = np.zeros((n, max_instances, 5), I32), np.zeros((n, max_instances, 2), F32)
    for i in range(n):
        ys, xs = np.nonzero((masks[i] > 0) & (masks[i] <= max_instances))
        j = masks[i][ys, xs].astype(np.int64) - 1
        k = int(j.max()) + 1 if len(j) else 0
        area, sy, sx = (np.zeros(k, np.int64) for _ in range(3))
        np.add.at(area, j, 1), np.add.at(sy, j, ys), np.add.at(sx, j, xs)
        y0, x0, y1, x1 = np.full(k, h, np.int64), np.full(k, w, np.int64), np.zeros(k, np.int64), np.zeros(k, np.int64)
        np.minimum.at(y0, j, ys), np.minimum.at(x0, j, xs), np.maximum.at(y1, j, ys + 1), np.maximum.at(x1, j, xs + 1)
        assert (area > 0).all()                           # numbers are consecutive: every row up to the largest is used
        instances[i, :k] = np.stack([area, y0, x0, y1, x1], 1)
        centres[i, :k, 0] = (sy.astype(np.float64) / area.astype(np.float64)).astype(F32)
        centres[i, :k, 1] = (sx.astype(np.float64) / area.astype(np.float64)).astype(F32)
    return instances, centres


def follow_plane(dy, dx, prob, level, min_flow, rounds, min_size):
    """(masks int32 (H, W), num) of one image: rules 1 to 6."""
    h, w = prob.shape
    end, fg = step_ref(dy, dx, prob, level, min_flow)
    for _ in range(rounds):
        end = end[end]                                    # a fresh array from the old one: no in-place doubling
    cnt = np.bincount(end[fg], minlength=h * w)
    S, raw_num = CR.label_ref((cnt > 0).astype(np.uint8).reshape(h, w), 8, 0)
    raw = np.where(fg, S.ravel()[end], 0)
    vol = np.bincount(raw[fg], minlength=int(raw_num) + 1)[1:]
    keep = vol >= min_size
    new = np.concatenate([[0], np.where(keep, np.cumsum(keep), 0)])
    return new[raw].astype(I32).reshape(h, w), int(keep.sum())


def flow_ref(x, level=0.0, min_flow=0.0, rounds=10, min_size=15, max_instances=256, planes=(0, 1, 2)):
    """The four arrays of the chain for float32 x (N, C, H, W)."""
    x = np.asarray(x)
    assert x.dtype == F32 and x.ndim == 4
    n, _, h, w = x.shape
    out = [follow_plane(x[i, planes[0]], x[i, planes[1]], x[i, planes[2]], level, min_flow, rounds, min_size) for i in range(n)]
    masks = np.stack([o[0] for o in out]) if n else np.zeros((0, h, w), I32)
    return (masks, np.array([o[1] for o in out], I32)) + table_ref(masks, max_instances)


# ---- patterns: float32 (n, 3, h, w), planes dy, dx, prob ---------------------------------------------------------------------
def _pack(dy, dx, prob, n):
    x = np.stack([np.asarray(a, F32) for a in (dy, dx, prob)])
    return np.broadcast_to(x, (n,) + x.shape).copy()


def random_flows(n, h, w, seed):
    """Full-mantissa flows of every magnitude and a probability plane around 0."""
    rng = np.random.default_rng(seed)
    mag = np.exp2(rng.integers(-4, 4, (n, 2, h, w))).astype(F32)
    flows = (rng.standard_normal((n, 2, h, w)).astype(F32) * mag).astype(F32)
    prob = (rng.standard_normal((n, 1, h, w)) + 0.7).astype(F32)
    return np.ascontiguousarray(np.concatenate([flows, prob], 1))


def discs(n, h, w, seed=0, noise=0.0, pitch=12, radius=4.5):
    """Discs on a grid with flows that point at their centres; outside them background.  Clean flows (noise 0) give one
    instance per disc.  -> (x, number of discs per image)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:h, :w]
    cy, cx = (y // pitch) * pitch + pitch // 2, (x // pitch) * pitch + pitch // 2
    inside = ((y - cy) ** 2 + (x - cx) ** 2 <= radius ** 2) & (cy + radius < h) & (cx + radius < w)
    dy, dx = np.where(inside, cy - y, 0).astype(F32), np.where(inside, cx - x, 0).astype(F32)
    out = _pack(dy, dx, np.where(inside, 1.0, -1.0), n)
    if noise:
        out[:, :2] += (rng.standard_normal((n, 2, h, w)) * noise).astype(F32)
    count = len(set(zip(cy[inside].tolist(), cx[inside].tolist())))
    return out, count


def all_background(n, h, w):
    return _pack(np.ones((h, w)), np.ones((h, w)), np.full((h, w), -1.0), n)


def all_foreground_still(n, h, w):
    return _pack(np.zeros((h, w)), np.zeros((h, w)), np.ones((h, w)), n)


def lattice(n, h, w):
    """Foreground on the even rows and columns only, zero flow: ceil(h / 2) ceil(w / 2) instances of one pixel."""
    prob = np.full((h, w), -1.0)
    prob[0::2, 0::2] = 1.0
    return _pack(np.zeros((h, w)), np.zeros((h, w)), prob, n)


def outward(n, h, w):
    """All foreground, the flow points away from the centre: out of every border."""
    y, x = np.mgrid[:h, :w]
    dy, dx = np.where(2 * y >= h, 1.0, -1.0), np.where(2 * x >= w, 1.0, -1.0)
    return _pack(dy, dx, np.ones((h, w)), n)


def into_background(n, h, w):
    """Foreground columns in pairs with a background column between; the flow points right: every second one into background."""
    x = np.mgrid[:h, :w][1]
    return _pack(np.zeros((h, w)), np.ones((h, w)), np.where(x % 3 == 2, -1.0, 1.0), n)


def serpentine(n, h, w):
    """One path through every other row, joined alternately at the right and the left end; each pixel points at the next one
    and the last at itself.  -> (x, length of the path)"""
    path, right = [], True
    for y in range(0, h, 2):
        xs = range(w) if right else range(w - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + 1 < h:
            path.append((y + 1, path[-1][1]))
        right = not right
    dy, dx, prob = np.zeros((h, w)), np.zeros((h, w)), np.full((h, w), -1.0)
    for (y0, x0), (y1, x1) in zip(path, path[1:]):
        dy[y0, x0], dx[y0, x0] = y1 - y0, x1 - x0
    for y, x in path:
        prob[y, x] = 1.0
    return _pack(dy, dx, prob, n), len(path)


def two_cycles(n, h, w, offset):
    """Pairs of horizontal neighbours that point at each other, the pairs starting at columns offset, offset + 2, ..."""
    x = np.mgrid[:h, :w][1]
    return _pack(np.zeros((h, w)), np.where((x - offset) % 2 == 0, 1.0, -1.0), np.ones((h, w)), n)


def vortices(n, h, w, offset):
    """2 x 2 blocks whose pixels point round the block (4-cycles), the blocks starting at rows and columns offset, offset + 2, ..."""
    y, x = np.mgrid[:h, :w]
    a, b = (y - offset) % 2, (x - offset) % 2
    dy = np.where((a == 0) & (b == 1), 1.0, np.where((a == 1) & (b == 0), -1.0, 0.0))
    dx = np.where((a == 0) & (b == 0), 1.0, np.where((a == 1) & (b == 1), -1.0, 0.0))
    return _pack(dy, dx, np.ones((h, w)), n)


def specials(n, h, w, seed):
    """Random flows with NaN, +inf and -inf planted in each of the three planes."""
    x = random_flows(n, h, w, seed)
    rng = np.random.default_rng(seed + 1)
    flat = x.reshape(n, 3, -1)
    for plane in range(3):
        for v in (np.nan, np.inf, -np.inf):
            idx = rng.integers(0, h * w, max(1, h * w // 12))
            flat[:, plane, idx] = v
    return x


def direction_edges(n, h, w, seed):
    """All foreground; (dy, dx) pairs on the boundaries between two of the eight directions: for random a, b runs over the
    float32 within 2 ulp of the one nearest sqrt(3) |a|, as (a, b) and as (b, a), all signs."""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(h * w).astype(F32) * np.exp2(rng.integers(-6, 6, h * w)).astype(F32)).astype(F32)
    b = (np.sqrt(3.0) * np.abs(a.astype(np.float64))).astype(F32)
    k = np.arange(h * w) % 5 - 2
    for step in range(2):
        b = np.where(k > step, np.nextafter(b, F32(np.inf)), np.where(k < -step, np.nextafter(b, F32(0)), b)).astype(F32)
    b = b * np.where(rng.random(h * w) < 0.5, -1, 1).astype(F32)
    swap = (np.arange(h * w) // 5) % 2 == 1
    dy, dx = np.where(swap, b, a), np.where(swap, a, b)
    return _pack(dy.reshape(h, w), dx.reshape(h, w), np.ones((h, w)), n)


MIN_FLOW_EDGE = 2.0


def length_edges(n, h, w):
    """All foreground, for min_flow = 2 (g2 = 4): dx around 2 and dy so small that l2 is exactly g2 (stays), rounds to g2 on a tie
    (stays), is one ulp above (moves right), or below (stays), column by column."""
    tiny = F32(2.0 ** -11)
    rows = [(0.0, 2.0), (tiny, 2.0), (np.nextafter(tiny, F32(1)), 2.0), (0.0, np.nextafter(F32(2), F32(3))),
            (0.0, np.nextafter(F32(2), F32(0)))]
    x = np.mgrid[:h, :w][1] % len(rows)
    dy = np.array([r[0] for r in rows], F32)[x]
    dx = np.array([r[1] for r in rows], F32)[x]
    return _pack(dy, dx, np.ones((h, w)), n)


def disc_grid(h, w, pitch=16, radius=6):
    """A grid of discs with centre-pointing flows for a large map, with its answer: (x (1, 3, h, w), count, area of each disc)."""
    y, x = np.mgrid[:h, :w]
    cy, cx = (y // pitch) * pitch + pitch // 2, (x // pitch) * pitch + pitch // 2
    inside = ((y - cy) ** 2 + (x - cx) ** 2 <= radius ** 2) & (cy + radius < h) & (cx + radius < w)
    out = _pack(np.where(inside, cy - y, 0), np.where(inside, cx - x, 0), np.where(inside, 1.0, -1.0), 1)
    v, u = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    area = int((v * v + u * u <= radius * radius).sum())
    rows, cols = (h - radius - 1 - pitch // 2) // pitch + 1, (w - radius - 1 - pitch // 2) // pitch + 1
    return out, rows * cols, area

"""tests/flow_ref.py, the numpy mirror the GPU tests of the flow-following chain compare against, held to an
independent statement of the rule: a per-pixel Python loop that walks 2^rounds single steps, scipy.ndimage.label with a 3 x 3
structure, and np.bincount.  CPU only."""
import numpy as np
import pytest

from tests import flow_ref as R

ndimage = pytest.importorskip("scipy.ndimage")
F32, I32 = np.float32, np.int32


def plain(x, level, min_flow, rounds, min_size, max_instances, planes=(0, 1, 2)):
    """The rule, pixel by pixel."""
    n, _, h, w = x.shape
    level, g2 = F32(level), F32(min_flow) * F32(min_flow)
    all_masks, nums = [], []
    for img in x:
        dy, dx, prob = (img[p] for p in planes)
        fg = [[bool(prob[y, u] > level) for u in range(w)] for y in range(h)]
        nxt = {}
        with np.errstate(all="ignore"):
            for y in range(h):
                for u in range(w):
                    nxt[y, u] = (y, u)
                    if not fg[y][u]:
                        continue
                    ay, ax = F32(dy[y, u] * dy[y, u]), F32(dx[y, u] * dx[y, u])
                    if not F32(ay + ax) > g2:
                        continue
                    sy = int(np.sign(dy[y, u])) if F32(F32(3) * ay) >= ax else 0
                    sx = int(np.sign(dx[y, u])) if F32(F32(3) * ax) >= ay else 0
                    t = min(max(y + sy, 0), h - 1), min(max(u + sx, 0), w - 1)
                    if fg[t[0]][t[1]]:
                        nxt[y, u] = t
        end = {}
        for p in nxt:
            q = p
            for _ in range(2 ** rounds):
                q = nxt[q]
            end[p] = q
        sink = np.zeros((h, w), bool)
        for p, q in end.items():
            if fg[p[0]][p[1]]:
                sink[q] = True
        S, _ = ndimage.label(sink, structure=np.ones((3, 3)))
        raw = np.array([[S[end[y, u]] if fg[y][u] else 0 for u in range(w)] for y in range(h)], np.int64).reshape(h, w)
        vol = np.bincount(raw.ravel())
        masks, k = np.zeros((h, w), I32), 0
        for j in range(1, len(vol)):
            if vol[j] >= min_size and vol[j] > 0:
                k += 1
                masks[raw == j] = k
        all_masks.append(masks)
        nums.append(k)
    masks = np.stack(all_masks)
    instances, centres = np.zeros((n, max_instances, 5), I32), np.zeros((n, max_instances, 2), F32)
    for i in range(n):
        for j in range(min(nums[i], max_instances)):
            ys, xs = np.nonzero(masks[i] == j + 1)
            instances[i, j] = [len(ys), ys.min(), xs.min(), ys.max() + 1, xs.max() + 1]
            centres[i, j] = [F32(np.float64(ys.sum()) / np.float64(len(ys))), F32(np.float64(xs.sum()) / np.float64(len(ys)))]
    return masks, np.array(nums, I32), instances, centres


def same(got, want, what):
    for name, g, r in zip(("masks", "num", "instances", "centres"), got, want):
        assert g.shape == r.shape and g.dtype == r.dtype, (what, name, g.shape, r.shape, g.dtype, r.dtype)
        assert g.tobytes() == r.tobytes(), (what, name)


def patterns(n, h, w):
    return [("random", R.random_flows(n, h, w, h + w)), ("discs", R.discs(n, h, w)[0]), ("noisy discs", R.discs(n, h, w, 3, 0.8)[0]),
            ("background", R.all_background(n, h, w)), ("still", R.all_foreground_still(n, h, w)), ("lattice", R.lattice(n, h, w)),
            ("outward", R.outward(n, h, w)), ("into background", R.into_background(n, h, w)), ("serpentine", R.serpentine(n, h, w)[0]),
            ("2-cycles", R.two_cycles(n, h, w, 1)), ("vortices", R.vortices(n, h, w, 1)), ("specials", R.specials(n, h, w, 5)),
            ("direction edges", R.direction_edges(n, h, w, 9)), ("length edges", R.length_edges(n, h, w))]


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 5, 7), (1, 17, 30), (1, 40, 70)], ids=str)
def test_mirror_equals_the_plain_rule(shape):
    n, h, w = shape
    for i, (name, x) in enumerate(patterns(n, h, w)):
        rounds = i % 7 if h * w < 1000 else i % 4         # 0 to 6; the largest map walks up to 8 steps per pixel
        kw = dict(level=0.0, min_flow=R.MIN_FLOW_EDGE if name == "length edges" else 0.25 * (i % 3), rounds=rounds,
                  min_size=(0, 1, 3, 15)[i % 4], max_instances=(0, 5, 64)[i % 3])
        same(R.flow_ref(x, **kw), plain(x, **kw), (shape, name, kw))


def test_rounds_up_to_six_on_a_long_path():
    x, length = R.serpentine(1, 9, 20)
    assert length > 2 ** 6
    for rounds in range(7):
        kw = dict(level=0.0, min_flow=0.0, rounds=rounds, min_size=0, max_instances=8)
        got = R.flow_ref(x, **kw)
        same(got, plain(x, **kw), rounds)
        # the pixels further than 2^rounds from the end are still on their way: the sinks are the rest of the path
        assert got[2][0, 0, 0] == length and got[1][0] == 1
    y = np.ascontiguousarray(x[:, [2, 1, 0]])                             # planes (prob, dx, dy)
    same(R.flow_ref(y, rounds=3, min_size=0, planes=(2, 1, 0)), R.flow_ref(x, rounds=3, min_size=0), "planes")


def test_discs_with_clean_flows_give_one_instance_each():
    x, count = R.discs(1, 96, 160)
    masks, num, instances, centres = R.flow_ref(x)
    assert count == 8 * 13 and num[0] == count
    y, u = np.mgrid[:96, :160]
    for j in range(count):                                # one instance per disc: its pixels are the disc's, its centre the disc's
        cy, cx = centres[0, j] if j < 256 else (0, 0)
        assert cy == (instances[0, j, 1] + instances[0, j, 3] - 1) / 2 and cx == (instances[0, j, 2] + instances[0, j, 4] - 1) / 2
        assert ((masks[0] == j + 1) == (((y - cy) ** 2 + (u - cx) ** 2 <= 4.5 ** 2))).all()
    assert (masks[0] > 0).sum() == (x[0, 2] > 0).sum()
    grid, count, area = R.disc_grid(64, 96)
    masks, num, instances, _ = R.flow_ref(grid, max_instances=32)
    assert num[0] == count == 24 and (instances[0, :24, 0] == area).all() and (np.bincount(masks.ravel())[1:] == area).all()


def test_the_patterns_are_what_they_claim():
    h, w = 11, 14
    kw = dict(min_size=0, max_instances=4)
    masks, num, instances, _ = R.flow_ref(R.lattice(1, h, w), **kw)
    assert num[0] == 6 * 7 and (instances[0, :, 0] == 1).all() and masks.max() == 42
    assert R.flow_ref(R.all_background(2, h, w), **kw)[1].tolist() == [0, 0]
    assert R.flow_ref(R.all_foreground_still(1, h, w), **kw)[2][0, 0].tolist() == [h * w, 0, 0, h, w]
    assert R.flow_ref(R.outward(1, h, w), **kw)[1][0] == 4                       # the four corners
    masks = R.flow_ref(R.into_background(1, h, w), **kw)[0]
    assert (masks[0, :, 2::3] == 0).all() and (masks[0, :, 0::3] > 0).all()
    # a 2-cycle swaps at rounds 0 and is back at rounds 1; either way each pair is its own sink region ... joined to the next
    a, b = (R.flow_ref(R.two_cycles(1, 4, 8, 0), rounds=r, **kw) for r in (0, 1))
    assert a[1][0] == b[1][0] == 1
    # dropped instances leave 0 in the masks and the rest is renumbered
    x, count = R.discs(1, 30, 40)
    full = R.flow_ref(x, min_size=0)
    vol = int(full[2][0, 0, 0])
    assert R.flow_ref(x, min_size=vol)[1][0] == count and R.flow_ref(x, min_size=vol + 1)[1][0] == 0
    # NaN probability is background; NaN flow does not move
    x = R.all_foreground_still(1, 3, 3)
    x[0, 2, 1, 1] = np.nan
    x[0, 0, 0, 0] = np.nan
    masks = R.flow_ref(x, min_size=0)[0]
    assert masks[0, 1, 1] == 0 and masks[0, 0, 0] == 1

"""Net.tiled without a GPU: the numpy mirrors of its two kernels (tests/tile_net_ref.py) reproduce what the
reference's own util.tile did (tests/golden/tile_net.npz, written by tools/capture_tile_net_golden.py) EXACTLY; the host geometry of
the product (util._Tiling, util.BlendGeometry) is the mirror's; and the refusals that need no device."""
import os

import numpy as np
import pytest

from tests import tile_net_ref as T
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "tile_net.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _nchw(rsts):
    return np.ascontiguousarray(rsts.transpose(0, 3, 1, 2))


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_mirror_equals_the_reference_exactly(gold, name):
    case = T.CASES[name]
    img, rsts, want = gold[name + "/img"], gold[name + "/rsts"], gold[name + "/out"]
    assert img.dtype == np.uint8 and tuple(img.shape[:2]) == case["size"]
    geo = T.Geometry(img.shape[0], img.shape[1], **case["tile"])
    assert len(geo.windows) == len(rsts)
    image = img.astype(np.float32)
    # the windows f was given: the mirror's cut of the (resampled) working image
    cut = T.cut_ref(image, geo.windows, work=geo.work)
    assert cut.shape == (len(rsts), img.shape[2]) + geo.win
    if name + "/wins" in gold.files:
        assert geo.resampled
        np.testing.assert_array_equal(T.canonical(cut.transpose(0, 2, 3, 1)), T.canonical(gold[name + "/wins"]))
    else:
        assert not geo.resampled
    # the blend, and the whole run with f = the recorded results
    calls = []
    got = T.tiled_ref(lambda x: _nchw(rsts), image, progress=lambda i, n: calls.append((i, n)), **case["tile"])
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_array_equal(T.canonical(got), T.canonical(want))
    np.testing.assert_array_equal(np.asarray(calls, np.int32).reshape(-1, 2), gold[name + "/progress"])
    assert rsts.shape[1] / geo.win[0] == case["k"]
    # the fixture carries what the blend must keep: NaN, infinities and a -0.0 that survives
    assert np.isnan(rsts).any() and np.isinf(rsts).any()
    if name in "ac":
        assert (np.signbit(want) & (want == 0)).any()


def test_fixture_geometries_are_the_ones_the_issue_names():
    g = {n: T.Geometry(*c["size"], **c["tile"]) for n, c in T.CASES.items()}
    assert (len(g["a"].rows), len(g["a"].cols)) == (3, 4)
    assert [r.start for r in g["b"].rows] == [0, 5, 10, 15, 21]
    cover = np.zeros(37, int)
    for r in g["b"].rows:
        cover[r] += 1
    assert cover.max() == 4                                       # four windows over one pixel per axis, sixteen in all
    assert g["c"].margin == 0 and g["c"].scaled(1)[2] == 0
    assert len(g["d"].windows) == 1 and g["d"].work == [16, 16] and g["d"].resampled
    assert g["e"].work == [50, 61] and g["e"].resampled
    r0, c0, ramp, size = g["g"].scaled(0.5)
    assert any(r.start % 2 for r in g["g"].rows) and any(c.start % 2 for c in g["g"].cols)
    assert (ramp, size) == (2, (18, 22)) and max(r0) + 8 == 18 and max(c0) + 8 == 22


@pytest.mark.parametrize("oh, ow, ramp", [(16, 16, 4), (16, 16, 10), (16, 16, 0), (32, 32, 8), (8, 8, 2), (7, 12, 5), (5, 5, 9)])
def test_weight_formula_is_the_reference_loop(oh, ow, ramp):
    """min(distance to the nearest edge, ramp) + 1 is what util.py:327-332 leaves in `weights`, ramps above half the window
    included (the descending loop's later, smaller writes win)."""
    weights = np.zeros((oh, ow), "uint16")
    weights += ramp + 1
    for i in range(ramp, 0, -1):
        if i > min(oh, ow):
            continue                                              # (the reference would index outside the window here)
        weights[i - 1, :] = weights[-i, :] = i
        weights[:, i - 1] = weights[:, -i] = i
    np.testing.assert_array_equal(weights, T.weights_formula(oh, ow, ramp))


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_host_geometry_equals_the_mirror(name):
    from planer_amd import util
    case = T.CASES[name]
    kw = dict(dict(sample=1, glob=1, window=1024, margin=0.1), **case["tile"])
    mine = util._Tiling(case["size"][0], case["size"][1], kw["sample"], kw["glob"], kw["window"], kw["margin"])
    ref = T.Geometry(*case["size"], **case["tile"])
    assert mine.windows == ref.windows and mine.work == ref.work and mine.margin == ref.margin
    assert (mine.win_h, mine.win_w) == ref.win and mine.resampled == ref.resampled
    k = case["k"]
    oh, ow = int(ref.win[0] * k), int(ref.win[1] * k)
    geo = util.BlendGeometry(mine.windows, k, mine.margin, mine.work, oh, ow)
    r0, c0, ramp, size = ref.scaled(k)
    r, c, h, w = util._window_origins(mine.windows)
    assert r.tolist() == [a.start for a, _ in ref.windows] and c.tolist() == [b.start for _, b in ref.windows]
    assert (h, w) == ref.win and r.dtype == c.dtype == np.int32
    assert (geo.gr, geo.gc) == (len(ref.rows), len(ref.cols)) and geo.n == len(ref.windows)
    if geo.n == 1:
        assert geo.R0.tolist() == [0] and geo.C0.tolist() == [0] and geo.ramp == 0 and (geo.OH, geo.OW) == (oh, ow)
    else:
        assert geo.R0.tolist() == r0 and geo.C0.tolist() == c0 and geo.ramp == ramp and (geo.OH, geo.OW) == size
    assert geo.R0.dtype == geo.C0.dtype == np.int32


def test_blend_geometry_refusals():
    from planer_amd import util
    geo = util._Tiling(37, 45, 1, 1, 16, 4)
    with pytest.raises(ValueError, match="scales"):               # k = 0.3: rows [0, 16) scale to 4 pixels, rows [21, 37) to 5
        util.BlendGeometry(geo.windows, 0.3, geo.margin, geo.work, 4, 4)
    with pytest.raises(ValueError, match="65535"):                # weights of 8193 on 3 x 3 windows
        big = util._Tiling(3 * 8192, 3 * 8192, 1, 1, 8192 + 4096, 8192)
        util.BlendGeometry(big.windows, 1, big.margin, big.work, 8192 + 4096, 8192 + 4096)
    with pytest.raises(ValueError, match="row-major grid"):
        util.BlendGeometry(geo.windows[1:] + geo.windows[:1], 1, geo.margin, geo.work, 16, 16)
    with pytest.raises(ValueError, match="covered by no window"):
        rows, cols = [slice(0, 16), slice(20, 36)], [slice(0, 16)]
        util.BlendGeometry([(r, c) for r in rows for c in cols], 1, 0, (36, 16), 16, 16)
    with pytest.raises(ValueError, match="size"):
        util._window_origins([(slice(0, 16), slice(0, 16)), (slice(0, 15), slice(0, 16))])
    with pytest.raises(ValueError, match="at least one"):
        util._window_origins([])


def _net():
    import planer_amd
    net = planer_amd.Net(ctx=object())                            # (no device: only the checks in front of any device work)
    net.input = ["x"]
    return net


def test_net_tiled_refusals_before_any_device_work():
    net = _net()
    u8, f32 = np.zeros((37, 45, 3), np.uint8), np.zeros((37, 45, 3), np.float32)
    with pytest.raises(ValueError, match="image_input"):
        net.tiled(u8, window=16)
    with pytest.raises(ValueError, match="uint8 or float32"):
        net.tiled(np.zeros((2, 3, 37, 45), np.float32), window=16)
    with pytest.raises(ValueError, match="batch"):
        net.tiled(f32, window=16, batch=0)
    net.label_output()
    with pytest.raises(NotImplementedError, match="different product"):
        net.tiled(f32, window=16, sample=(50, 61))
    with pytest.raises(NotImplementedError, match="different product"):
        net.tiled(f32[:12, :14], window=16, glob=8)               # grown to 16 x 16: resampled too
    net.float_output().image_output(1.0, 0.0)
    with pytest.raises(NotImplementedError, match="different product"):
        net.tiled(f32, window=16, sample=0.5)
    net.float_output().detection_output([([(10, 13)], 8)], classes=2)
    with pytest.raises(ValueError, match="detections"):
        net.tiled(f32, window=16)
    two = _net()
    two.input = ["x", "y"]
    with pytest.raises(ValueError, match="one input"):
        two.tiled(f32, window=16)

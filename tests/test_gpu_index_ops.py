"""The operators that do index arithmetic instead of arithmetic, at their block and grid boundaries on a real MI355X: TopK,
NonZero, Gather (and the shifted nearest Resize on its kernel), ScatterND, Cast, Equal / Greater / GreaterOrEqual, Where, Erf,
Slice / Pad / Tile / Expand / Split, Transpose and general-broadcast Add / Sub / Mul / Div / Pow.

Each has an exact answer in numpy (tests/ref_index.py), so every comparison is exact: integers and bools by value, dtype and
shape, float32 by bit pattern (NaN matching NaN; -0 is not +0).  Pow alone keeps the ULP["pow"] allowance of
tests/ref64_ops.py against float64.  What the shapes are for:

  * "past the grid": the streaming launch caps the grid at cu_count * 8 blocks of 256 threads and loops; an element count above
    twice that many threads makes every thread take a second trip.  Every such case asserts the inequality for the part it
    runs on (`_past_grid`).
  * NonZero: 2048 elements per block ("B"), 1024 blocks per chunk of the offset scan ("C" = 2 097 152 elements); from C + 1
    elements on the scan carries a running total from chunk to chunk.
  * TopK: rows up to 16 384 are sorted in LDS (padded to a power of two; from n = 4097 the launch raises the dynamic-LDS limit),
    longer rows take k selection rounds.  The order is exact: ascending value, NaN last, equal values (+0 / -0) by ascending
    index -- a stable argsort.

All calls go through the public layer functions; nothing is wrapped in try / except -- an input outside a kernel's domain is a
case of its own with pytest.raises.  Run with -s for the pool size at the end.
"""
import numpy as np
import pytest

from oracle import planer_np as onp
from tests import ref_index as R
from tests.cases import layer_cases
from tests.ref64_ops import ulp_bound

pytestmark = pytest.mark.gpu

F32 = np.float32
I64 = lambda *v: np.array(v, np.int64)


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _past_grid(pa, count, what):
    need = R.past_grid(pa.hip.context().cu_count)
    assert count > need, "%s: %d elements do not pass the grid (%d)" % (what, count, need)


def _dev(pa, a):
    """Host -> device WITHOUT a host mirror: a small integer / bool tensor made by `asarray` keeps one and would be evaluated on
    the host (layer._shape_domain), not by the kernel under test."""
    a = np.require(a, requirements="C")
    d = pa.hip.empty(a.shape, a.dtype)
    d.set(a)
    assert d.host is None
    return d


# ==== a. TopK ================================================================================================================
def _topk_check(pa, x, axis, ks, what):
    topk = pa.layer_map["topk"]
    dx = pa.asarray(x)
    order = np.argsort(x, axis=axis, kind="stable")
    for k in ks:
        for largest in (1, 0):
            wv, wi = R.topk_ref(x, k, axis, largest, order=order)
            gv, gi = topk(dx, I64(k), axis=axis, largest=largest)
            tag = "topk %s k=%d largest=%d" % (what, k, largest)
            R.assert_same(gi.get(), wi, tag + " indices")
            R.assert_same(gv.get(), wv, tag + " values")


@pytest.mark.parametrize("n", R.TOPK_SORT_N + R.TOPK_SELECT_N)
def test_topk_every_data_class(pa, n):
    """Three rows of every data class at every k of the path, both directions."""
    for cls in R.TOPK_CLASSES:
        _topk_check(pa, R.topk_data(cls, 3, n), -1, R.topk_ks(n), "%s n=%d" % (cls, n))


def _topk_mixed_rows(rows, n):
    """Rows of ties and of specials alternating (the two classes where a nearly right index shows)."""
    x = R.topk_data("ties", rows, n, seed=1)
    x[1::2] = R.topk_data("specials", rows, n, seed=1)[1::2]
    return x


@pytest.mark.parametrize("n", R.TOPK_SORT_N + R.TOPK_SELECT_N)
def test_topk_layouts(pa, n):
    """Axis last with 1 and 300 rows (more rows than CUs), a middle axis with inner extents 1, 7 and 130 (inner <= 7 above
    n = 4096)."""
    ks = [7, 300] if n > R.TOPK_LDS_MAX else sorted({min(n, 7), n})
    for rows in (1, 300):
        _topk_check(pa, _topk_mixed_rows(rows, n), -1, ks, "(%d, %d)" % (rows, n))
    for inner in ((1, 7, 130) if n <= 4096 else (1, 7)):
        x = np.ascontiguousarray(_topk_mixed_rows(3 * inner, n).reshape(3, inner, n).transpose(0, 2, 1))
        for axis in ((1, -2) if inner == 7 else (1,)):
            _topk_check(pa, x, axis, ks, "(3, %d, %d) axis %d" % (n, inner, axis))


def test_topk_refusals(pa):
    topk = pa.layer_map["topk"]
    x = pa.asarray(R.topk_data("ties", 2, 9))
    with pytest.raises(NotImplementedError):
        topk(x, I64(3), largest=2)
    with pytest.raises(IndexError):
        topk(x, I64(10))
    with pytest.raises(ValueError):
        topk(x, I64(3), axis=2)
    with pytest.raises(ValueError):
        topk(x, I64(3), axis=-3)


# ==== b. NonZero =============================================================================================================
def _nonzero_check(pa, x, what):
    got = pa.layer_map["nonzero"](_dev(pa, x)).get()
    R.assert_same(got, R.nonzero_ref(x), "nonzero " + what)


@pytest.mark.parametrize("size", R.NONZERO_SIZES)
def test_nonzero_patterns_1d(pa, size):
    """Every pattern at every 1-D size in float32 (NaN and subnormals are non-zero, -0.0 is zero); the other dtypes on the
    density-0.5 and the carry-only patterns."""
    ran = 0
    for p in R.NONZERO_PATTERNS:
        m = R.nonzero_mask(p, size)
        if m is None:                        # the pattern needs more than one block / chunk
            continue
        _nonzero_check(pa, R.nonzero_input(m, F32), "%s float32 %d" % (p, size))
        if p in ("half", "beyond_chunk"):
            for dt in (np.int32, np.int64, np.bool_):
                _nonzero_check(pa, R.nonzero_input(m, dt), "%s %s %d" % (p, np.dtype(dt), size))
        ran += 1
    assert ran >= 6 and (ran == 8) == (size > R.NZ_CHUNK)


def test_nonzero_float_specials(pa):
    x = np.array([0.0, -0.0, np.nan, R.TINY, -R.TINY, 2.0 ** -127, np.inf, -np.inf, 1.0, -0.0, 0.0, -np.nan], F32)
    got = pa.layer_map["nonzero"](pa.asarray(x)).get()
    R.assert_same(got, np.array([[2, 3, 4, 5, 6, 7, 8, 11]], np.int64), "nonzero specials")


@pytest.mark.parametrize("shape", R.NONZERO_SHAPES, ids=["x".join(map(str, s)) for s in R.NONZERO_SHAPES])
def test_nonzero_coordinate_decode(pa, shape):
    """Rank 2, 3 and 8 above C elements: the coordinates of a non-zero decode from its flat position axis by axis."""
    size = int(np.prod(shape))
    assert size > R.NZ_CHUNK
    m = R.nonzero_mask("half", size)
    m[-1] = m[0] = True
    _nonzero_check(pa, R.nonzero_input(m, F32).reshape(shape), str(shape))
    m = R.nonzero_mask("sparse", size)
    m[-1] = True
    _nonzero_check(pa, R.nonzero_input(m, np.int32).reshape(shape), "sparse int32 %s" % (shape,))


def test_nonzero_nine_axes_refused(pa):
    with pytest.raises(NotImplementedError):
        pa.layer_map["nonzero"](pa.asarray(np.ones((1, 2, 1, 2, 1, 2, 1, 2, 1), F32)))


# ==== c. Gather ==============================================================================================================
def _gather_check(pa, x, dx, idx, axis, what):
    got = pa.layer_map["gather"](dx, idx, axis=axis)
    R.assert_same(got.get(), np.take(x, idx, axis=axis), "gather %s axis %d idx %s" % (what, axis, np.shape(idx)))


IDX_SHAPES = [(), (1,), (5,), (4097,), (17, 241), (1, 5)]


@pytest.mark.parametrize("inner", [1, 3, 1000])
def test_gather_inner_extents_and_index_counts(pa, inner):
    """x viewed as (outer, axis_len, inner) = (3, 11, inner): 1, 5 and 4097 indices in tensors of rank 0, 1 and 2."""
    rng = np.random.default_rng(inner)
    x = rng.standard_normal((3, 11, inner)).astype(F32)
    dx = pa.asarray(x)
    assert int(np.prod(IDX_SHAPES[4])) == 4097
    for shp in IDX_SHAPES:
        idx = R.gather_indices(11, shp)
        for axis in (1, -2):
            _gather_check(pa, x, dx, idx, axis, str(x.shape))


def test_gather_axis_first_middle_last(pa):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((11, 5, 7)).astype(F32)
    dx = pa.asarray(x)
    for axis in (0, 1, 2, -1, -2, -3):
        alen = x.shape[axis]
        for shp in ((), (5,), (2, 3)):
            _gather_check(pa, x, dx, R.gather_indices(alen, shp), axis, str(x.shape))
    v = rng.standard_normal(13).astype(F32)                     # a vector: outer = inner = 1
    _gather_check(pa, v, pa.asarray(v), R.gather_indices(13, (40,)), 0, "(13,)")


def test_gather_past_the_grid(pa):
    x = np.random.default_rng(4).standard_normal((7, 50, 37)).astype(F32)
    idx = R.gather_indices(50, (4097,))
    _past_grid(pa, 7 * 4097 * 37, "gather")
    _gather_check(pa, x, pa.asarray(x), idx, 1, str(x.shape))


def test_gather_out_of_bounds_refused(pa):
    dx = pa.asarray(np.zeros((3, 11, 2), F32))
    for bad in (11, -12):
        with pytest.raises(IndexError):
            pa.layer_map["gather"](dx, I64(0, bad, 1), axis=1)


def _resize_mode_pairs():
    pairs = []
    for _, kind, _, p in layer_cases():
        if kind == "resize" and p.get("mode") == "nearest":
            pair = (p.get("coordinate_transformation_mode", "half_pixel"), p.get("nearest_mode", "round_prefer_floor"))
            if pair not in pairs:
                pairs.append(pair)
    return pairs


RESIZE_PAIRS = _resize_mode_pairs()


def _resize_check(pa, x, k, tm, rm):
    kk = np.array([1, 1] + list(k), F32)
    roi = np.zeros(0, F32)
    para = dict(mode="nearest", coordinate_transformation_mode=tm, nearest_mode=rm)
    want = onp.resize(x.copy(), roi, kk, **para)
    got = pa.layer_map["resize"](pa.asarray(x), roi, kk, **para)
    R.assert_same(got.get(), want, "resize %s x %s (%s, %s)" % (x.shape, k, tm, rm))


@pytest.mark.parametrize("pair", RESIZE_PAIRS, ids=["-".join(p) for p in RESIZE_PAIRS])
def test_resize_shifted_nearest_on_the_gather_kernel(pa, pair):
    """Every (coordinate mode, rounding mode) pair of tests/cases.py at an odd map and at one past the grid; then two geometries
    that share factors and shifts but differ in h and w, interleaved, and the first again -- a wrong key of the map cache shows."""
    assert len(RESIZE_PAIRS) >= 8
    rng = np.random.default_rng(len(pair[0]) * 31 + len(pair[1]))
    a = rng.standard_normal((2, 3, 37, 53)).astype(F32)
    b = rng.standard_normal((1, 2, 300, 301)).astype(F32)
    _past_grid(pa, 2 * 600 * 903, "resize")
    _resize_check(pa, a, (3, 2), *pair)
    _resize_check(pa, b, (2, 3), *pair)
    c = rng.standard_normal((2, 3, 53, 37)).astype(F32)         # h and w swapped: same element count, same factors and shifts
    d = rng.standard_normal((1, 1, 36, 54)).astype(F32)
    for x in (a, c, d, a, c):
        _resize_check(pa, x, (3, 2), *pair)


# ==== d. ScatterND ===========================================================================================================
def _scatter_check(pa, data, idx, upd, what):
    d = pa.asarray(data)
    got = pa.layer_map["scatternd"](d, idx, pa.asarray(upd))
    R.assert_same(got.get(), R.scatternd_ref(data, idx, upd), "scatternd " + what)
    R.assert_same(d.get(), data, "scatternd %s: data after the call" % what)


# 70 000 updates of 4099 floats would be 1.1 GB; the largest tensors here stay near 50 MB, so that one pair is left out -- both
# values still run against every other value of the other parameter
SCATTER_ROWS = [(L, n) for L in (1, 5, 4099) for n in (1, 1000, 70000) if L * n <= 12 << 20]


@pytest.mark.parametrize("row_len,n", SCATTER_ROWS)
def test_scatternd_rows_last_write_wins(pa, row_len, n):
    """Index tuples of length 1 into (4000, row_len): the updates are drawn from a quarter of the rows, negative indices among
    them, so most rows are written several times."""
    assert (4099, 1000) in SCATTER_ROWS and (5, 70000) in SCATTER_ROWS and len(SCATTER_ROWS) == 8
    rng = np.random.default_rng([row_len, n])
    rows = 4000
    data = rng.standard_normal((rows, row_len)).astype(F32)
    quarter = rng.permutation(rows)[:rows // 4]
    r = rng.choice(quarter, n)
    r = np.where(rng.random(n) < 0.5, r - rows, r)              # the same row under both of its names
    if n >= 1000:
        assert len(set((r % rows).tolist())) < n and (r < 0).any() and (r >= 0).any()
    idx = r.reshape(1, n, 1).astype(np.int64)
    upd = rng.standard_normal((1, n, row_len)).astype(F32)
    _scatter_check(pa, data, idx, upd, "rows (%d, %d) n=%d" % (rows, row_len, n))


def test_scatternd_tuples_of_two_into_3d(pa):
    rng = np.random.default_rng(21)
    data = rng.standard_normal((30, 40, 33)).astype(F32)
    n = 5000
    idx = np.stack([rng.integers(-30, 30, n), rng.integers(-40, 40, n)], 1).reshape(1, n, 2).astype(np.int64)
    upd = rng.standard_normal((1, n, 33)).astype(F32)
    _scatter_check(pa, data, idx, upd, "(30, 40, 33) tuples of 2")


def test_scatternd_full_rank_past_the_grid(pa):
    """1 200 000 single-element updates into (1500, 1000): 1 100 000 different places -- what the kernel copies, past the grid --
    and 100 000 of them written a second time later on."""
    rng = np.random.default_rng(22)
    cells = rng.permutation(1500 * 1000)[:1100000]
    flat = np.concatenate([cells, rng.choice(cells, 100000)])
    flat = flat[rng.permutation(flat.size)]
    assert flat.size == 1200000 and len(np.unique(flat)) == 1100000
    _past_grid(pa, 1100000, "scatternd")
    r, c = np.divmod(flat, 1000)
    r = np.where(rng.random(flat.size) < 0.3, r - 1500, r)
    idx = np.stack([r, c], 1).reshape(1, -1, 2).astype(np.int64)
    data = rng.standard_normal((1500, 1000)).astype(F32)
    upd = rng.standard_normal((1, flat.size)).astype(F32)
    _scatter_check(pa, data, idx, upd, "(1500, 1000) full rank")


def test_scatternd_extra_updates_are_ignored(pa):
    rng = np.random.default_rng(23)
    data = rng.standard_normal((9, 6)).astype(F32)
    idx = I64(3, 0, 3, -1).reshape(1, 4, 1)
    _scatter_check(pa, data, idx, rng.standard_normal((1, 7, 6)).astype(F32), "7 updates, 4 indices")


def test_scatternd_refusals(pa):
    scat = pa.layer_map["scatternd"]
    data = pa.asarray(np.zeros((9, 6), F32))
    with pytest.raises(NotImplementedError):
        scat(data, I64(3, 0, 3, 1).reshape(1, 4, 1), pa.asarray(np.zeros((1, 3, 6), F32)))
    for bad in (9, -10):
        with pytest.raises(IndexError):
            scat(data, I64(3, bad).reshape(1, 2, 1), pa.asarray(np.zeros((1, 2, 6), F32)))


# ==== e. Cast ================================================================================================================
@pytest.mark.parametrize("dst", R.CAST_TYPES)
@pytest.mark.parametrize("src", R.CAST_TYPES)
def test_cast_every_pair(pa, src, dst):
    """All sixteen pairs at 1, 255, 257 and 1 200 003 elements against astype.  float -> integer of NaN, +-inf or an out-of-range
    value is left out on purpose (undefined in C++; numpy's answer is the host CPU's): DESIGN 4.14."""
    _past_grid(pa, R.CAST_SIZES[-1], "cast")
    for n in R.CAST_SIZES:
        x = R.cast_source(src, dst, n)
        with np.errstate(invalid="ignore"):
            want = x.astype(dst)
        got = pa.layer_map["cast"](_dev(pa, x), dtype=dst)
        R.assert_same(got.get(), want, "cast %s -> %s n=%d" % (src, dst, n))


# ==== f. comparisons and Where ===============================================================================================
COMPARES = [("equal", np.equal), ("greater", np.greater), ("greaterorequal", np.greater_equal)]


@pytest.mark.parametrize("kind,ref", COMPARES, ids=[c[0] for c in COMPARES])
def test_compare_sizes_and_single_value_operands(pa, kind, ref):
    op = pa.layer_map[kind]
    _past_grid(pa, R.COMPARE_SIZES[-1], kind)
    for n in R.COMPARE_SIZES:
        a, b = R.compare_pair(n)
        da, db = pa.asarray(a), pa.asarray(b)
        R.assert_same(op(da, db).get(), ref(a, b), "%s full n=%d" % (kind, n))
        for s in (0.0, -0.0, 2.0, np.nan, np.inf):
            one = np.array([s], F32)
            R.assert_same(op(da, one).get(), ref(a, one), "%s host scalar %r on the right n=%d" % (kind, s, n))
            R.assert_same(op(one, db).get(), ref(one, b), "%s host scalar %r on the left n=%d" % (kind, s, n))
        one = np.array([1.0], F32)
        R.assert_same(op(da, pa.asarray(one)).get(), ref(a, one), "%s device scalar on the right n=%d" % (kind, n))
        R.assert_same(op(pa.asarray(one), db).get(), ref(one, b), "%s device scalar on the left n=%d" % (kind, n))
        R.assert_same(op(da, 1.0).get(), ref(a, F32(1.0)), "%s python scalar n=%d" % (kind, n))


@pytest.mark.parametrize("mask", R.WHERE_MASKS)
def test_where_passes_every_bit_pattern(pa, mask):
    where = pa.layer_map["where"]
    _past_grid(pa, R.COMPARE_SIZES[-1], "where")
    for n in R.COMPARE_SIZES:
        m = R.where_mask(mask, n)
        a, b = R.where_operand(n, 1), R.where_operand(n, 2)
        dm, da, db = _dev(pa, m), pa.asarray(a), pa.asarray(b)
        R.assert_same(where(dm, da, db).get(), np.where(m, a, b), "where %s full n=%d" % (mask, n))
        for s in (-0.0, np.nan, R.TINY):
            one = np.array([s], F32)
            R.assert_same(where(dm, one, db).get(), np.where(m, one, b), "where %s host %r left n=%d" % (mask, s, n))
            R.assert_same(where(dm, da, one).get(), np.where(m, a, one), "where %s host %r right n=%d" % (mask, s, n))
            R.assert_same(where(dm, pa.asarray(one), db).get(), np.where(m, one, b), "where %s device %r left n=%d" % (mask, s, n))
            R.assert_same(where(dm, da, pa.asarray(one)).get(), np.where(m, a, one), "where %s device %r right n=%d" % (mask, s, n))
        R.assert_same(where(dm, np.array([-0.0], F32), np.array([np.nan], F32)).get(),
                      np.where(m, F32(-0.0), F32(np.nan)).astype(F32), "where %s two single values n=%d" % (mask, n))


def test_where_refusals(pa):
    where = pa.layer_map["where"]
    a = pa.asarray(np.zeros(300, F32))
    with pytest.raises(TypeError):
        where(pa.asarray(np.ones(300, F32)), a, a)
    with pytest.raises(TypeError):
        where(_dev(pa, np.ones(300, np.int32)), a, a)
    with pytest.raises(NotImplementedError):
        where(_dev(pa, np.ones(300, bool)), a, pa.asarray(np.zeros(150, F32)))


def test_compare_refusal(pa):
    with pytest.raises(NotImplementedError):
        pa.layer_map["equal"](pa.asarray(np.zeros(300, F32)), pa.asarray(np.zeros(150, F32)))


# ==== g. Erf =================================================================================================================
def test_erf_table_boundaries_and_clobbered_input(pa):
    x = R.erf_points()
    _past_grid(pa, x.size, "erf")
    clobbered = x.copy()
    want = onp.erf(clobbered)                                   # overwrites its argument, like the reference
    dx = pa.asarray(x)
    got = pa.layer_map["erf"](dx)
    R.assert_same(got.get(), want.astype(F32), "erf")
    R.assert_same(dx.get(), clobbered, "erf: the input after the call")


# ==== h. strided-map family and Transpose ====================================================================================
BIG6 = (5, 6, 7, 8, 9, 100)


@pytest.fixture(scope="module")
def big6(pa):
    x = np.random.default_rng(60).standard_normal(BIG6).astype(F32)
    return x, pa.asarray(x)


def _slice_check(pa, x, dx, cuts, what):
    """cuts: {axis: (start, end, step)}"""
    axes = sorted(cuts)
    sl = [slice(None)] * x.ndim
    for a in axes:
        sl[a] = slice(*cuts[a])
    want = x[tuple(sl)]
    args = [I64(*[cuts[a][0] for a in axes]), I64(*[cuts[a][1] for a in axes]), I64(*axes), I64(*[cuts[a][2] for a in axes])]
    got = pa.layer_map["slice"](dx, *args)
    R.assert_same(got.get(), np.ascontiguousarray(want), "slice %s %s" % (what, cuts))
    return want.size


def test_slice_six_axes_every_step(pa, big6):
    x, dx = big6
    _past_grid(pa, x.size, "slice input")
    INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
    full = _slice_check(pa, x, dx, {0: (0, 5, 1), 1: (-1, INT_MIN, -1), 2: (0, INT_MAX, 1), 3: (7, -9, -1), 4: (-9, 9, 1),
                                    5: (99, -101, -1)}, "whole, three axes reversed")
    _past_grid(pa, full, "slice output")
    _slice_check(pa, x, dx, {0: (1, 5, 2), 1: (5, 0, -2), 2: (0, 7, 3), 3: (-1, -9, -1), 4: (2, 100, 1), 5: (-1, -200, -2)},
                 "steps 2, -2, 3, -1, 1, -2; bounds that clamp")
    _slice_check(pa, x, dx, {0: (-3, -1, 1), 1: (-100, 3, 1), 2: (-2, -8, -1), 3: (1, -1, 3), 4: (-1, 0, -2), 5: (-50, -1, 3)},
                 "negative bounds")
    for empty_axis, cut in ((0, (3, 3, 1)), (3, (2, 5, -1)), (5, (100, 200, 1)), (4, (-20, -10, 1))):
        _slice_check(pa, x, dx, {0: (0, 2, 1), empty_axis: cut}, "an empty axis")
    rng = np.random.default_rng(61)
    for _ in range(6):
        cuts = {}
        for a in range(6):
            n = BIG6[a]
            cuts[a] = (int(rng.integers(-n - 2, n + 3)), int(rng.integers(-n - 2, n + 3)), int(rng.choice([1, 2, 3, -1, -2])))
        _slice_check(pa, x, dx, cuts, "random")


PAD_MODES = ["constant", "wrap", "edge", "reflect", "symmetric"]


def _pad_check(pa, x, pads, mode, value=0.0):
    """pads: [(before, after)] per axis"""
    para = {"constant_values": value} if mode == "constant" else {}
    want = np.pad(x, pads, mode=mode, **para)
    flat = I64(*([p[0] for p in pads] + [p[1] for p in pads]))
    para = {"constant_value": value} if mode == "constant" else {}
    got = pa.layer_map["pad"](pa.asarray(x), flat, mode=mode, **para)
    R.assert_same(got.get(), want, "pad %s %s %s" % (mode, x.shape, pads))


@pytest.mark.parametrize("mode", PAD_MODES)
def test_pad_short_axes_wide_pads_every_rank(pa, mode):
    """Axes of extent 1, 2, 3 and 7 padded by 0 .. 10 on either side -- wrap, reflect and symmetric fold back several times -- in
    1-D through 6-D (from 4-D on two axes take the wide pads and the others 0 .. 1, which keeps the result small); every
    (extent, before, after) with before, after in {0, 3, 10} once in 1-D; one case past the grid."""
    rng = np.random.default_rng(PAD_MODES.index(mode))
    for ext in (1, 2, 3, 7):
        x = rng.standard_normal(ext).astype(F32)
        for before in (0, 3, 10):
            for after in (0, 3, 10):
                _pad_check(pa, x, [(before, after)], mode, -1.5)
    for nd in range(1, 7):
        for trial in range(3):
            shape = tuple(int(rng.choice([1, 2, 3, 7])) for _ in range(nd))
            wide = set(range(nd)) if nd <= 3 else set(rng.choice(nd, 2, replace=False).tolist())
            pads = [(int(rng.integers(0, 11)), int(rng.integers(0, 11))) if d in wide else
                    (int(rng.integers(0, 2)), int(rng.integers(0, 2))) for d in range(nd)]
            _pad_check(pa, rng.standard_normal(shape).astype(F32), pads, mode, float(trial) - 0.5)
    x = rng.standard_normal((3, 5, 260, 270)).astype(F32)
    _past_grid(pa, 3 * 5 * 267 * 277, "pad")
    _pad_check(pa, x, [(0, 0), (0, 0), (3, 4), (5, 2)], mode, 2.5)


def test_pad_refusals(pa):
    x = pa.asarray(np.zeros((2, 3), F32))
    with pytest.raises(NotImplementedError):
        pa.layer_map["pad"](x, I64(1, 1, 1, 1), mode="mean")
    with pytest.raises(ValueError):
        pa.layer_map["pad"](x, I64(1, -1, 1, 1))


def test_tile_repeat_lengths(pa):
    rng = np.random.default_rng(62)
    tile = pa.layer_map["tile"]
    x = rng.standard_normal((3, 5, 7)).astype(F32)
    dx = pa.asarray(x)
    for rep in ((2,), (3, 2), (2, 1, 3), (1, 1, 1), (2, 1, 3, 2), (2, 2, 1, 1, 2, 1)):       # shorter, equal, longer than the rank
        R.assert_same(tile(dx, I64(*rep)).get(), np.tile(x, rep), "tile %s by %s" % (x.shape, rep))
    v = rng.standard_normal(1).astype(F32)
    R.assert_same(tile(pa.asarray(v), I64(300)).get(), np.tile(v, 300), "tile (1,) by 300")
    y = rng.standard_normal((37, 41)).astype(F32)
    _past_grid(pa, 3 * 37 * 30 * 41 * 9, "tile")
    R.assert_same(tile(pa.asarray(y), I64(3, 30, 9)).get(), np.tile(y, (3, 30, 9)), "tile (37, 41) by (3, 30, 9)")


def test_expand_every_position_and_rank_extension(pa):
    rng = np.random.default_rng(63)
    expand = pa.layer_map["expand"]
    full = (3, 4, 5, 6)

    def check(xs, shp):
        x = rng.standard_normal(xs).astype(F32)
        want = np.ascontiguousarray(np.broadcast_to(x, np.broadcast_shapes(tuple(shp), xs)))
        R.assert_same(expand(pa.asarray(x), I64(*shp)).get(), want, "expand %s to %s" % (xs, shp))
    for p in range(4):
        check(tuple(1 if d == p else full[d] for d in range(4)), full)                      # one size-1 axis at every position
        check(tuple(full[d] if d == p else 1 for d in range(4)), full)                      # all but one
    check((1, 1, 1, 1), full)
    check(full, full)
    check((5, 6), full)                                                                     # rank extension through x ...
    check((5, 1), (2,) + full)
    check((1,), (2, 3) + full)                                                              # ... to six axes
    check(full, (1, 1, 5, 1))                                                               # the shape argument broadcasts too
    check((3, 1, 5, 1), (4, 1, 6))
    x = rng.standard_normal((1100, 1)).astype(F32)
    _past_grid(pa, 1100 * 1000, "expand")
    R.assert_same(expand(pa.asarray(x), I64(1100, 1000)).get(), np.ascontiguousarray(np.broadcast_to(x, (1100, 1000))), "expand past the grid")


def test_split_uneven_parts_and_the_leading_slice_quirk(pa):
    """np.split(x[:sum(parts)], cumsum(parts)[:-1], axis): the leading slice is along axis 0 whatever `axis` is, so on another
    axis it shortens axis 0 and the last part takes what is left of `axis`."""
    rng = np.random.default_rng(64)
    split = pa.layer_map["split"]
    x = rng.standard_normal((9, 7, 5)).astype(F32)
    dx = pa.asarray(x)
    for axis, parts in ((0, [2, 3, 4]), (0, [1, 1, 5]), (1, [1, 2, 4]), (1, [1, 2]), (2, [1, 4]), (2, [2, 1]), (-1, [4, 1]), (1, [3, 4, 2]),
                        (1, [6, 6])):
        seg = np.cumsum(parts).tolist()
        want = np.split(x[:seg[-1]], seg[:-1], axis)
        got = split(dx, split=parts, axis=axis)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            R.assert_same(g.get(), np.ascontiguousarray(w), "split %s axis %d part %d" % (parts, axis, i))
    assert np.split(x[:3], [1], 1)[1].shape == (3, 6, 5)                                    # the quirk, spelt out


TRANSPOSE_PERMS = {"identity": (0, 1, 2, 3, 4, 5), "reversal": (5, 4, 3, 2, 1, 0), "rotation": (1, 2, 3, 4, 5, 0),
                   "inner swap": (0, 1, 2, 3, 5, 4)}


@pytest.mark.parametrize("name", list(TRANSPOSE_PERMS))
def test_transpose_six_axes(pa, big6, name):
    x, dx = big6
    perm = TRANSPOSE_PERMS[name]
    _past_grid(pa, x.size, "transpose")
    tr = pa.layer_map["transpose"]
    R.assert_same(tr(dx, axis=list(perm)).get(), np.ascontiguousarray(x.transpose(perm)), "transpose %s" % name)
    ones = x.reshape(1, 30, 7, 1, 72, 100)                                                  # size-1 axes sprinkled in
    R.assert_same(tr(dx.reshape(ones.shape), axis=list(perm)).get(), np.ascontiguousarray(ones.transpose(perm)),
                  "transpose %s with size-1 axes" % name)


def test_transpose_2d_odd(pa):
    x = np.random.default_rng(65).standard_normal((1031, 1033)).astype(F32)
    _past_grid(pa, x.size, "transpose 2-D")
    R.assert_same(pa.layer_map["transpose"](pa.asarray(x), axis=[1, 0]).get(), np.ascontiguousarray(x.T), "transpose (1031, 1033)")


def test_seven_axes_refused(pa):
    x7 = pa.asarray(np.zeros((2, 1, 2, 1, 2, 1, 2), F32))
    with pytest.raises(NotImplementedError):
        pa.layer_map["slice"](x7, I64(0), I64(1), I64(0), I64(1))
    with pytest.raises(NotImplementedError):
        pa.layer_map["pad"](x7, I64(*([0] * 14)))
    with pytest.raises(NotImplementedError):
        pa.layer_map["tile"](x7, I64(*([1] * 7)))
    with pytest.raises(NotImplementedError):
        pa.layer_map["expand"](x7, I64(2, 1, 2, 1, 2, 1, 2))
    with pytest.raises(NotImplementedError):
        pa.layer_map["transpose"](x7, axis=[6, 5, 4, 3, 2, 1, 0])
    with pytest.raises(NotImplementedError):
        pa.layer_map["add"](x7, pa.asarray(np.zeros((1, 2, 1, 2, 1, 2, 1), F32)))


# ==== i. general broadcasting ================================================================================================
BCAST_OPS = [("add", np.add), ("sub", np.subtract), ("mul", np.multiply), ("div", np.divide), ("pow", np.power)]


@pytest.fixture(scope="module")
def bcast_pairs():
    return R.broadcast_pairs()


@pytest.mark.parametrize("kind,fn", BCAST_OPS, ids=[o[0] for o in BCAST_OPS])
def test_general_broadcasting_sixty_pairs(pa, bcast_pairs, kind, fn):
    """Sixty seeded shape pairs, ranks 0-6 on each side, extents from {1, 2, 3, 7, 16, 40}: at least fifteen results past the
    grid, at least ten that keep four or more axes after merging.  Add / Sub / Mul / Div bit for bit against numpy; Pow
    (positive bases) within ULP["pow"] of float64."""
    need = R.past_grid(pa.hip.context().cu_count)
    large = deep = 0
    for i, (sa, sb) in enumerate(bcast_pairs):
        a, b = R.broadcast_operands(i, sa, sb, positive=kind == "pow")
        if kind == "div":
            b = (np.abs(b) + F32(0.5)).astype(F32)
        got = pa.layer_map[kind](pa.asarray(a), pa.asarray(b))
        what = "%s pair %d %s %s" % (kind, i, sa, sb)
        if kind == "pow":
            ref = np.power(a.astype(np.float64), b.astype(np.float64))
            g = got.get()
            assert g.shape == ref.shape, what
            err = np.abs(g.astype(np.float64) - ref)
            tol = ulp_bound(ref, "pow")
            assert (err <= tol).all(), "%s: %.3g ulp-bounds at worst" % (what, float((err / tol).max()))
        else:
            R.assert_same(got.get(), fn(a, b), what)
        large += got.size > need
        deep += R.merged_axes(sa, sb) >= 4
    assert large >= 15, large
    assert deep >= 10, deep


def test_broadcast_that_cannot_merge_below_seven_axes_refused(pa):
    a, b = np.zeros((2, 1, 2, 1, 2, 1, 2), F32), np.zeros((1, 2, 1, 2, 1, 2, 1), F32)
    assert R.merged_axes(a.shape, b.shape) == 7
    for kind in ("add", "sub", "mul", "div", "pow"):
        with pytest.raises(NotImplementedError):
            pa.layer_map[kind](pa.asarray(a), pa.asarray(b))


def test_zz_pool_size(pa):
    """Runs last (file order): the pool after the whole module, for DESIGN 4.14."""
    reserved, used = pa.hip.context().pool_stats()
    print("\nindex ops: pool reserved %.1f MiB, in use %.1f MiB" % (reserved / 2.0 ** 20, used / 2.0 ** 20))

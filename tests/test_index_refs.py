"""The references and generators of tests/ref_index.py, pinned on the CPU: small hand-written inputs with their answers written
out literally, and for every generator the boundary it claims to cross (sizes, not kernels)."""
import numpy as np
import pytest

from tests import ref_index as R

F32 = np.float32
nan, inf = np.nan, np.inf


# ---- TopK: ties, NaN and +-0 ------------------------------------------------------------------------------------------------
#                  0    1    2     3    4    5     6    7    8
ROW = np.array([1.0, nan, 0.0, -0.0, 1.0, inf, -inf, nan, 0.0], F32)
# ascending, NaN last, equal values (+0 == -0) by index:  -inf(6)  0(2) -0(3) 0(8)  1(0) 1(4)  inf(5)  nan(1) nan(7)
ROW_ORDER = [6, 2, 3, 8, 0, 4, 5, 1, 7]


def test_topk_ref_order_is_value_then_nan_last_then_index():
    assert np.argsort(ROW, kind="stable").tolist() == ROW_ORDER
    assert R.topk_order_lexsort(ROW).tolist() == ROW_ORDER
    rng = np.random.default_rng(1)
    for n in (1, 2, 50, 1000):
        x = R.topk_data("specials", 1, n)[0]
        assert np.array_equal(np.argsort(x, kind="stable"), R.topk_order_lexsort(x))
        x = rng.integers(-2, 3, n).astype(F32)
        assert np.array_equal(np.argsort(x, kind="stable"), R.topk_order_lexsort(x))


def test_topk_ref_largest_takes_the_order_from_its_end():
    v, i = R.topk_ref(ROW, 5, axis=0, largest=1)
    assert i.dtype == np.int64 and i.tolist() == [7, 1, 5, 4, 0]                   # of two NaNs / two ones the HIGHER index first
    assert R.same_bits(v, np.array([nan, nan, inf, 1.0, 1.0], F32))
    v, i = R.topk_ref(ROW, 9, axis=0, largest=1)
    assert i.tolist() == ROW_ORDER[::-1]
    assert R.same_bits(v, np.array([nan, nan, inf, 1.0, 1.0, 0.0, -0.0, 0.0, -inf], F32))       # index 8, 3, 2: +0, -0, +0
    assert not R.same_bits(v, np.array([nan, nan, inf, 1.0, 1.0, 0.0, 0.0, 0.0, -inf], F32))    # -0 is not +0
    v, i = R.topk_ref(ROW, 0, axis=0, largest=1)
    assert v.shape == (0,) and i.shape == (0,)


def test_topk_ref_smallest_is_k_copies_of_the_first():
    v, i = R.topk_ref(ROW, 3, axis=0, largest=0)
    assert i.tolist() == [6, 6, 6] and v.tolist() == [-inf, -inf, -inf]
    z = np.array([0.0, -0.0, 0.0], F32)
    v, i = R.topk_ref(z, 2, axis=0, largest=0)
    assert i.tolist() == [0, 0] and R.same_bits(v, np.array([0.0, 0.0], F32))
    z = np.array([-0.0, 0.0, nan], F32)
    v, i = R.topk_ref(z, 2, axis=0, largest=0)
    assert i.tolist() == [0, 0] and R.same_bits(v, np.array([-0.0, -0.0], F32))
    v, i = R.topk_ref(np.array([nan, nan], F32), 1, axis=0, largest=0)
    assert i.tolist() == [0]


def test_topk_ref_along_a_middle_axis():
    x = np.array([[[3, 1], [3, 2], [0, 2]]], F32)                                  # (1, 3, 2)
    v, i = R.topk_ref(x, 2, axis=1, largest=1)
    assert i.tolist() == [[[1, 2], [0, 1]]] and v.tolist() == [[[3, 2], [3, 2]]]


# ---- ScatterND ----------------------------------------------------------------------------------------------------------
def test_scatternd_ref_last_write_wins():
    data = np.zeros((3, 2), F32)
    idx = np.array([[[1], [0], [1], [-1], [1]]], np.int64)
    upd = np.arange(1, 11, dtype=F32).reshape(1, 5, 2)
    out = R.scatternd_ref(data, idx, upd)
    assert out.tolist() == [[3, 4], [9, 10], [7, 8]]
    assert not data.any()                                                          # a copy: data stays
    idx = np.array([[[0, 0], [2, 1], [0, 0]]], np.int64)
    out = R.scatternd_ref(data, idx, np.array([[5, 6, 7, 99]], F32))               # a fourth update without an index is ignored
    assert out.tolist() == [[7, 0], [0, 0], [0, 6]]


# ---- same_bits ----------------------------------------------------------------------------------------------------------
def test_same_bits_is_strict():
    assert R.same_bits(np.array([nan, 0.0], F32), np.array([nan, 0.0], F32))
    assert not R.same_bits(np.array([0.0], F32), np.array([-0.0], F32))
    assert not R.same_bits(np.array([1], np.int32), np.array([1], np.int64))
    assert not R.same_bits(np.zeros((2, 1), bool), np.zeros((2,), bool))
    assert R.same_bits(np.array([[1, 2]], np.int64), np.array([[1, 2]], np.int64))
    with pytest.raises(AssertionError):
        R.assert_same(np.array([1, 2], np.int64), np.array([1, 3], np.int64), "x")


# ---- Cast: the table, literally -------------------------------------------------------------------------------------------
T62 = 4611686018427387904
CAST_EXPECTED = {
    ("float32", "int32"): [0, 0, 0, 0, 0, 0, 0, 1, -2, 16777215, 16777216, -16777216, 16777218, 2147483520, -2147483520],
    ("float32", "int64"): [0, 0, 0, 0, 0, 0, 0, 1, -2, 16777215, 16777216, -16777216, 16777218, 2147483520, -2147483648, 4294967296,
                           T62, -T62],
    ("float32", "bool"): [True, True, True, True, False, True, True, True, True, True, True, True, True, True, True, True, True, False],
    ("int32", "float32"): [0.0, 1.0, -1.0, -2147483648.0, 2147483648.0, 16777216.0, -16777220.0, 123456792.0],
    ("int32", "int64"): [0, 1, -1, -2147483648, 2147483647, 16777217, -16777219, 123456789],
    ("int32", "bool"): [False, True, True, True, True, True, True, True],
    # odd values just above 2^24 and 2^53 round to nearest even
    ("int64", "float32"): [0.0, 1.0, -1.0, 16777216.0, 16777220.0, -16777216.0, 9007199254740992.0, 9007199254740992.0, 2147483648.0,
                           2147483648.0, -2147483648.0, 4294967296.0, -1099511627776.0, 4.611686018427388e+18, 4294967296.0],
    # beyond +-2^31: the low 32 bits
    ("int64", "int32"): [0, 1, -1, 16777217, 16777219, -16777217, 1, 3, -2147483648, -2147483643, 2147483647, 7, 3, 0, 0],
    ("int64", "bool"): [False] + [True] * 14,
    ("bool", "float32"): [0.0, 1.0, 1.0, 0.0],
    ("bool", "int32"): [0, 1, 1, 0],
    ("bool", "int64"): [0, 1, 1, 0],
}


@pytest.mark.parametrize("src", R.CAST_TYPES)
@pytest.mark.parametrize("dst", R.CAST_TYPES)
def test_cast_table_against_literal_values(src, dst):
    sp = R.cast_specials(src, dst)
    assert sp.dtype == np.dtype(src)
    got = sp.astype(dst)
    if src == dst:
        assert R.same_bits(got, sp)
        return
    want = np.array(CAST_EXPECTED[(src, dst)], dst)
    assert R.same_bits(got, want), (src, dst, got.tolist())


def test_cast_sources_hold_what_the_table_claims():
    f = R.cast_specials("float32", "int32")
    assert np.isfinite(f).all() and np.abs(f).max() == 2.0 ** 31 - 128
    assert {0.5, -0.5, R.ONE_M, -R.ONE_M} <= set(f.tolist()) and np.signbit(f[f == 0]).any()
    assert ((np.abs(f) > 0) & (np.abs(f) < 2.0 ** -126)).sum() >= 2                # subnormals
    assert np.abs(R.cast_specials("float32", "int64")).max() == 2.0 ** 62
    b = R.cast_specials("float32", "bool")
    assert np.isnan(b).any() and np.isposinf(b).any() and np.isneginf(b).any()
    for dst in ("int32", "int64", "float32"):
        assert not np.isnan(R.cast_specials("float32", dst)).any() and not np.isinf(R.cast_specials("float32", dst)).any()
    i = R.cast_specials("int32", "float32")
    assert i.min() == -2 ** 31 and i.max() == 2 ** 31 - 1
    for src in R.CAST_TYPES:
        for dst in R.CAST_TYPES:
            for n in R.CAST_SIZES:
                x = R.cast_source(src, dst, n)
                assert x.shape == (n,) and x.dtype == np.dtype(src)
                if src == "float32" and dst in ("int32", "int64"):
                    lim = 2.0 ** 31 - 128 if dst == "int32" else 2.0 ** 62
                    assert np.isfinite(x).all() and np.abs(x).max() <= lim
                if n >= 18:
                    sp = R.cast_specials(src, dst)
                    assert R.same_bits(x[:sp.size], sp)


# ---- the generators reach the boundaries they claim -------------------------------------------------------------------------
def test_grid_sizes_for_256_cus():
    assert R.grid_threads(256) == 524288 and R.past_grid(256) == 1048576
    for n in (R.COMPARE_SIZES[-1], R.CAST_SIZES[-1], R.ERF_SIZE, 7 * 4097 * 37, 1200000, 2 * 2 * 600 * 903):
        assert n > R.past_grid(256)


def test_topk_rows_cross_every_lds_boundary():
    lds = {n: R.topk_lds_bytes(n) for n in R.TOPK_SORT_N + R.TOPK_SELECT_N}
    assert lds[4096] == 32 * 1024 <= R.TOPK_STATIC_LDS                             # the last row on the static limit
    assert lds[4097] == lds[8192] == 64 * 1024 > R.TOPK_STATIC_LDS                 # the first that raises it
    assert lds[8193] == lds[16383] == lds[16384] == 128 * 1024
    assert all(lds[n] is None for n in R.TOPK_SELECT_N) and min(R.TOPK_SELECT_N) == R.TOPK_LDS_MAX + 1
    for n in (63, 65, 255, 257, 1023, 1025):
        assert lds[n] // 8 > n                                                     # padded
    assert R.topk_ks(1) == [0, 1] and R.topk_ks(257) == [0, 1, 7, 257] and R.topk_ks(1025) == [0, 1, 7, 257, 1000, 1025]
    assert R.topk_ks(65537) == [1, 7, 300]
    assert max(R.topk_ks(16384)) > R.TPB                                           # more results than threads in the block


@pytest.mark.parametrize("n", [1, 3, 65, 1025, 20000])
def test_topk_data_classes(n):
    d = {c: R.topk_data(c, 3, n) for c in R.TOPK_CLASSES}
    assert all(len(set(r.tolist())) == n for r in d["distinct"]) and np.isfinite(d["distinct"]).all()
    assert set(d["ties"].reshape(-1).tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert (d["equal"] == d["equal"][0, 0]).all()
    if n > 1:
        assert (np.diff(d["ascending"], axis=1) > 0).all() and (np.diff(d["descending"], axis=1) < 0).all()
    if n >= 65:
        s = d["specials"]
        for r in s:
            assert np.isnan(r).sum() >= 2 and np.isposinf(r).any() and np.isneginf(r).any()
            z = r[r == 0]
            assert np.signbit(z).any() and (~np.signbit(z)).any() and (r == 1).sum() >= 2
        assert len(set(np.unique(d["ties"][0], return_counts=True)[1].tolist())) >= 1 and (d["ties"][0] == 2).sum() > 1


def test_nonzero_sizes_and_patterns():
    B, C = R.NZ_BLOCK, R.NZ_CHUNK
    assert (B, C) == (2048, 2097152)
    assert R.NONZERO_SIZES == [1, 2047, 2048, 2049, C - 1, C, C + 1, 2 * C + 5, 3 * C + B + 1]
    blocks = lambda n: -(-n // B)
    assert blocks(C) == 1024 and blocks(C + 1) == 1025                             # the first size whose scan takes a second chunk
    assert blocks(2 * C + 5) == 2049 and blocks(3 * C + B + 1) == 3074             # three and four chunks
    for size in (1, B + 1, C + 1):
        for p in R.NONZERO_PATTERNS:
            m = R.nonzero_mask(p, size)
            if m is None:
                assert (p == "odd_blocks" and size <= B) or (p == "beyond_chunk" and size <= C)
                continue
            assert m.shape == (size,) and m.dtype == bool
            if p == "none":
                assert not m.any()
            if p == "all":
                assert m.all()
            if p == "first":
                assert m[0] and m.sum() == 1
            if p == "last":
                assert m[-1] and m.sum() == 1
            if p == "odd_blocks":
                assert not m[:B].any() and m[B:min(2 * B, size)].all()
            if p == "beyond_chunk":
                assert not m[:C].any() and m[C:].any()
    m = R.nonzero_mask("half", 4096)
    for dt in (F32, np.int32, np.int64, np.bool_):
        x = R.nonzero_input(m, dt)
        assert x.dtype == np.dtype(dt) and np.array_equal(x != 0, m)
    x = R.nonzero_input(m, F32)
    assert np.isnan(x).any() and (np.abs(x[m]) < 2.0 ** -126).any() and np.signbit(x[~m]).any()
    for shp in R.NONZERO_SHAPES:
        assert int(np.prod(shp)) > C
    assert len(R.NONZERO_SHAPES[-1]) == 8


def test_gather_indices_cover_the_range():
    for alen, shape in ((1, ()), (5, (5,)), (50, (4097,)), (7, (3, 4))):
        idx = R.gather_indices(alen, shape)
        assert idx.shape == shape and idx.dtype == np.int64 and idx.min() >= -alen and idx.max() < alen
        if idx.size >= 2:
            assert idx.min() == -alen and idx.max() == alen - 1
        if idx.size >= 4:
            assert len(set(idx.reshape(-1).tolist())) < idx.size
    assert set(R.gather_indices(50, (4097,)).tolist()) == set(range(-50, 50))


def test_compare_and_where_data():
    for n in R.COMPARE_SIZES:
        a, b = R.compare_pair(n)
        assert a.shape == b.shape == (n,)
        if n >= 256:
            na, nb = np.isnan(a), np.isnan(b)
            assert (na & ~nb).any() and (~na & nb).any() and (na & nb).any()
            z = (a == 0) & (b == 0)
            assert (np.signbit(a[z]) != np.signbit(b[z])).any()
            assert (np.isinf(a) & (a == b)).any() and (np.isinf(a) & np.isinf(b) & (a != b)).any()
            assert (a == b).any() and (a > b).any() and (a < b).any()
            assert np.isnan(a[-13:]).any()                                         # specials in the last trip too
    seen = set()
    for n in (13, 26, 39):                                                         # a one-element input is not always the same pair
        seen.add(repr(R.compare_pair(n + 1)[0][:1].tolist()))
    for k in R.WHERE_MASKS:
        m = R.where_mask(k, 1048579)
        assert m.dtype == bool and m.shape == (1048579,)
    assert not R.where_mask("false", 9).any() and R.where_mask("true", 9).all()
    m = R.where_mask("blocks", 1024)
    assert m[:256].all() and not m[256:512].any() and m[512:768].all()
    x = R.where_operand(257, 1)
    assert np.isnan(x).any() and np.signbit(x[x == 0]).any() and ((x != 0) & (np.abs(x) < 2.0 ** -126)).any()


def test_erf_points_hold_every_table_boundary():
    x = R.erf_points()
    assert x.shape == (R.ERF_SIZE,) and x.dtype == F32 and x.min() >= -3 and x.max() <= 3
    have = set(x.tolist())
    for i in range(-512, 513):
        m = F32(i / 256.0)
        assert float(m) in have and float(np.nextafter(m, F32(4))) in have and float(np.nextafter(m, F32(-4))) in have
    assert (x > 2).any() and (x < -2).any()


def test_broadcast_pairs_counts():
    pairs = R.broadcast_pairs()
    assert len(pairs) == 60 and pairs == R.broadcast_pairs()
    assert all(len(a) <= 6 and len(b) <= 6 and set(a) | set(b) <= set(R.BCAST_EXTENTS) for a, b in pairs)
    assert {len(s) for p in pairs for s in p} == set(range(7))                     # ranks 0 .. 6
    sizes = [int(np.prod(np.broadcast_shapes(a, b), dtype=np.int64)) for a, b in pairs]
    assert sum(s > R.past_grid(256) for s in sizes) >= 15
    assert max(sizes) <= R.BCAST_LARGE_RANGE[1]
    merged = [R.merged_axes(a, b) for a, b in pairs]
    assert sum(m >= 4 for m in merged) >= 10 and max(merged) <= 6
    assert R.merged_axes((2, 1, 2, 1, 2, 1, 2), (1, 2, 1, 2, 1, 2, 1)) == 7
    assert R.merged_axes((4, 5, 6), (4, 5, 6)) == 1 and R.merged_axes((4, 1, 6), (1, 5, 1)) == 3
    assert R.merged_axes((2, 3, 4, 5), (4, 1)) == 3                                # (6, 4, 5): the two outer axes merge

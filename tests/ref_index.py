"""References and data generators for the index and selection operators (TopK, NonZero, Gather, ScatterND, Cast, the
comparisons, Where, Erf, the strided-map family, Transpose and general broadcasting): DESIGN 4.14.

Every one of these operators has an exact answer in numpy, so the references are plain numpy, never call the code under test,
and are compared without a tolerance (`same_bits`).  The generators build inputs that cross one structural boundary of a kernel
each -- a second trip of a grid-stride loop, a second chunk of the NonZero scan, the LDS sizes of the TopK sort -- and carry data
that separates a right index from a nearly right one (ties, NaN, +-0, duplicates).  tests/test_index_refs.py pins all of this on
the CPU; tests/test_gpu_index_ops.py runs the kernels against it.
"""
import numpy as np

from oracle import planer_np as onp
from tests.test_gpu_special_values import mismatch

F32 = np.float32
TPB = 256                           # threads of a streaming block (PL_STREAM_TPB)
BLOCKS_PER_CU = 8                   # pl_stream_grid's cap
NZ_BLOCK = 2048                     # elements one NonZero block counts (PL_NONZERO_BLOCK): "B"
NZ_CHUNK = NZ_BLOCK * 1024          # elements one chunk of the NonZero scan covers: "C"
TOPK_LDS_MAX = 16384                # rows up to this length are sorted in LDS, longer ones take selection rounds
TOPK_STATIC_LDS = 48 * 1024         # above this the launch raises the dynamic-LDS limit
TINY = float(F32(2.0 ** -149))


def grid_threads(cu_count):
    """Threads of the largest streaming grid."""
    return cu_count * BLOCKS_PER_CU * TPB


def past_grid(cu_count):
    """An element count above this makes every thread of the capped grid take a second (and some a third) trip."""
    return 2 * grid_threads(cu_count)


# ---- references ---------------------------------------------------------------------------------------------------------
def topk_ref(x, k, axis=-1, largest=1, order=None):
    """layer.TopK with the documented order: ascending value, NaN last, equal values (+0 / -0 included) by ascending index --
    which is exactly what a STABLE argsort gives.  The index list is the reference's own (largest = 0: k zeros).  `order`: that
    argsort, computed once by a caller that asks for several k."""
    order = np.argsort(x, axis=axis, kind="stable") if order is None else order
    idk = np.arange(int(k)) * -largest - (largest > 0)
    idx = np.take(order, idk, axis=axis).astype(np.int64)
    return np.take_along_axis(x, idx, axis=axis), idx


def topk_order_lexsort(row):
    """The same order spelt out for one row: by (isnan, value, index)."""
    nan = np.isnan(row)
    return np.lexsort((np.arange(row.size), np.where(nan, 0, row), nan))


nonzero_ref = lambda a: np.array(np.nonzero(a))


def scatternd_ref(data, indices, updates):
    """The reference's sequential loop (a later update of the same place wins)."""
    return onp.scatternd(data, indices, updates)


def same_bits(got, want):
    """Exact equality, dtype and shape included.  float32: as uint32 patterns with NaN matching NaN, so -0 is not +0."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype == F32:
        return not mismatch(got, want).any()
    return bool(np.array_equal(got, want))


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s, want %s %s" % (what, got.dtype, got.shape, want.dtype,
                                                                                          want.shape)
    if same_bits(got, want):
        return
    bad = mismatch(got, want) if got.dtype == F32 else got != want
    at = np.argwhere(bad)[:4]
    raise AssertionError("%s: %d of %d elements differ, e.g. %s" % (what, int(bad.sum()), bad.size, "; ".join(
        "%s: %r want %r" % (tuple(int(v) for v in j), got[tuple(j)], want[tuple(j)]) for j in at)))


# ---- TopK ---------------------------------------------------------------------------------------------------------------
TOPK_SORT_N = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 4097, 8192, 8193, 16383, 16384]
TOPK_SELECT_N = [16385, 20000, 65537]
TOPK_CLASSES = ["distinct", "ties", "equal", "ascending", "descending", "specials"]


def topk_lds_bytes(n):
    """Dynamic LDS of the sort kernel for a row of n (None on the selection path): keys + indices, padded to a power of two."""
    if n > TOPK_LDS_MAX:
        return None
    npad = 2
    while npad < n:
        npad <<= 1
    return npad * 8


def topk_ks(n):
    if n > TOPK_LDS_MAX:
        return [1, 7, 300]
    return sorted(set([0, 1, min(n, 7), n] + [k for k in (257, 1000) if k <= n]))


def topk_data(cls, rows, n, seed=0):
    """(rows, n) float32 of one data class."""
    rng = np.random.default_rng([seed, rows, n, TOPK_CLASSES.index(cls)])
    if cls == "distinct":                                   # a permutation per row: no two values equal, all normal
        x = np.stack([rng.permutation(n) for _ in range(rows)]).astype(F32) - F32(n // 2) + F32(0.25)
    elif cls == "ties":
        x = rng.integers(-2, 3, (rows, n)).astype(F32)
    elif cls == "equal":
        x = np.full((rows, n), 1.5, F32)
    elif cls == "ascending":
        x = np.broadcast_to(np.arange(n, dtype=F32), (rows, n)).copy()
    elif cls == "descending":
        x = np.broadcast_to(np.arange(n, 0, -1, dtype=F32), (rows, n)).copy()
    else:                                                   # NaNs, +-inf and both zeros interleaved among ties
        pool = np.array([np.nan, np.nan, np.inf, -np.inf, 0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 1.0, 2.0], F32)
        x = pool[(np.arange(rows * n) % pool.size).reshape(rows, n)]
        x = np.stack([r[rng.permutation(n)] if n > pool.size else r for r in x])
    assert x.shape == (rows, n) and x.dtype == F32
    return x


# ---- NonZero ------------------------------------------------------------------------------------------------------------
_B, _C = NZ_BLOCK, NZ_CHUNK
NONZERO_SIZES = [1, _B - 1, _B, _B + 1, _C - 1, _C, _C + 1, 2 * _C + 5, 3 * _C + _B + 1]
NONZERO_PATTERNS = ["none", "all", "half", "sparse", "first", "last", "odd_blocks", "beyond_chunk"]
NONZERO_SHAPES = [(70001, 31), (3, 1025, 683), (2, 1, 3, 1, 5, 7, 11, 913)]


def nonzero_mask(pattern, size):
    """bool (size,) of one pattern, or None where the pattern needs a larger input."""
    m = np.zeros(size, bool)
    rng = np.random.default_rng([NONZERO_PATTERNS.index(pattern), size])
    if pattern == "all":
        m[:] = True
    elif pattern == "half":
        m = rng.random(size) < 0.5
    elif pattern == "sparse":
        m = rng.random(size) < 1e-4
    elif pattern == "first":
        m[0] = True
    elif pattern == "last":
        m[-1] = True
    elif pattern == "odd_blocks":
        if size <= _B:
            return None
        m = (np.arange(size) // _B) % 2 == 1
    elif pattern == "beyond_chunk":                         # the first scan chunk sums to zero: everything rides on the carry
        if size <= _C:
            return None
        m[_C:] = rng.random(size - _C) < 0.5
        m[-1] = True
    return m


def nonzero_input(mask, dtype, seed=0):
    """An array of `dtype` that is non-zero exactly where `mask` is; the values vary (negative ones, large ones, and for float32
    NaN and subnormals as non-zeros, -0.0 as a zero)."""
    dtype = np.dtype(dtype)
    if dtype == np.bool_:
        return mask.copy()
    if dtype == F32:
        pool = np.array([1.0, -1.0, np.nan, TINY, -TINY, np.inf, 2.0 ** -127, 0.5], F32)
        zeros = np.array([0.0, -0.0], F32)
    else:
        pool = np.array([1, -1, 7, np.iinfo(dtype).min, np.iinfo(dtype).max, 256, -65536, 1 << 24], dtype)
        zeros = np.zeros(2, dtype)
    pick = (np.arange(mask.size) + seed) % 8                # (a fixed rotation through the values: quick at 6 M elements)
    return np.where(mask, pool[pick], zeros[pick % 2]).astype(dtype)


# ---- Gather -------------------------------------------------------------------------------------------------------------
def gather_indices(axis_len, shape, seed=0):
    """int64 indices of `shape` over the whole range [-axis_len, axis_len) with repeats; -axis_len and axis_len - 1 are in
    whenever there is room for them."""
    rng = np.random.default_rng([seed, axis_len, int(np.prod(shape, dtype=np.int64))])
    idx = rng.integers(-axis_len, axis_len, shape).astype(np.int64)
    flat = idx.reshape(-1)
    if flat.size >= 1:
        flat[0] = -axis_len
    if flat.size >= 2:
        flat[-1] = axis_len - 1
    if flat.size >= 4:
        flat[1] = flat[2]                                   # a repeat for certain
    return idx


# ---- Cast ---------------------------------------------------------------------------------------------------------------
CAST_TYPES = ["float32", "int32", "int64", "bool"]
CAST_SIZES = [1, 255, 257, 1200003]
_F = lambda *v: np.array(v, F32)
ONE_M = float(np.nextafter(F32(1), F32(0)))                 # 0.99999994


def cast_specials(src, dst):
    """The edge values of one (source, destination) pair.  float32 -> integer leaves out NaN, +-inf and out-of-range values
    (undefined in C++; numpy's answer is the host CPU's)."""
    if src == "float32":
        base = [0.5, -0.5, ONE_M, -ONE_M, -0.0, TINY, -1e-40, 1.5, -2.5, 16777215.0, 16777216.0, -16777216.0, 16777218.0]
        if dst == "int32":
            base += [2147483520.0, -2147483520.0]           # 2^31 - 128: the largest float32 below 2^31
        elif dst == "int64":
            base += [2147483520.0, -2147483648.0, 4294967296.0, 2.0 ** 62, -2.0 ** 62]
        elif dst == "bool":
            base += [np.nan, np.inf, -np.inf, 2.0 ** 62, 0.0]
        else:
            base += [2.0 ** 62, 3.0e38, 0.0]
        return _F(*base)
    if src == "int64":
        return np.array([0, 1, -1, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), 2 ** 53 + 1, 2 ** 53 + 3, 2 ** 31, 2 ** 31 + 5,
                         -2 ** 31 - 1, 2 ** 32 + 7, -2 ** 40 + 3, 2 ** 62, 2 ** 32], np.int64)
    if src == "int32":
        return np.array([0, 1, -1, -2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, -(2 ** 24 + 3), 123456789], np.int32)
    return np.array([False, True, True, False], bool)


def cast_source(src, dst, n, seed=0):
    """(n,) of dtype `src`: the specials of the pair first (rotated by n, so that a one-element input is not always the same
    value), then random values inside the destination's range."""
    sp = cast_specials(src, dst)
    rng = np.random.default_rng([seed, n, CAST_TYPES.index(src), CAST_TYPES.index(dst)])
    if src == "float32":
        body = (rng.standard_normal(n) * 1000).astype(F32)
        body[rng.random(n) < 0.2] = 0
    elif src == "bool":
        body = rng.random(n) < 0.5
    else:
        lim = 2 ** 31 - 1 if src == "int32" else 2 ** 62
        body = rng.integers(-lim, lim, n).astype(src)
        body[rng.random(n) < 0.2] = 0
    out = np.concatenate([np.roll(sp, -(n % sp.size)), body])[:n] if n < sp.size else np.concatenate([sp, body[sp.size:]])
    assert out.shape == (n,) and out.dtype == np.dtype(src)
    return out


# ---- comparisons / Where ------------------------------------------------------------------------------------------------
COMPARE_SIZES = [1, 256, 257, 1048579]
_CMP = _F(np.nan, 1.0, np.nan, 0.0, -0.0, np.inf, -np.inf, np.inf, 2.0, 2.0, 3.0, -1.0, TINY)
_CMQ = _F(1.0, np.nan, np.nan, -0.0, 0.0, np.inf, -np.inf, -np.inf, 2.0, 3.0, 2.0, -1.0, -TINY)


def compare_pair(n, seed=0):
    """Two (n,) float32 operands: NaN on either or both sides, +0 against -0, +-inf, equal and unequal finite values, then
    small integers (about one pair in five equal)."""
    rng = np.random.default_rng([seed, n])
    a, b = rng.integers(-2, 3, n).astype(F32), rng.integers(-2, 3, n).astype(F32)
    k = min(n, _CMP.size)
    shift = n % _CMP.size
    a[:k], b[:k] = np.roll(_CMP, -shift)[:k], np.roll(_CMQ, -shift)[:k]
    if n > 2 * _CMP.size:                                   # and once more at the very end (the last trip of the loop)
        a[-k:], b[-k:] = _CMP, _CMQ
    return a, b


WHERE_MASKS = ["false", "true", "blocks", "random"]


def where_mask(kind, n, seed=0):
    if kind == "false":
        return np.zeros(n, bool)
    if kind == "true":
        return np.ones(n, bool)
    if kind == "blocks":
        return (np.arange(n) // TPB) % 2 == 0
    return np.random.default_rng([seed, n, 9]).random(n) < 0.5


def where_operand(n, seed):
    """(n,) float32 with NaN, -0 and subnormals among ordinary values: Where must pass every bit pattern through."""
    rng = np.random.default_rng([seed, n, 5])
    pool = _F(np.nan, -0.0, 0.0, TINY, -TINY, 2.0 ** -127, np.inf, -np.inf, 1.0, -3.5)
    x = rng.standard_normal(n).astype(F32)
    m = rng.random(n) < 0.3
    x[m] = pool[rng.integers(0, pool.size, int(m.sum()))]
    k = min(n, pool.size)
    x[:k] = np.roll(pool, -(n + seed) % pool.size)[:k]
    return x


# ---- Erf ----------------------------------------------------------------------------------------------------------------
ERF_SIZE = 1200003


def erf_points():
    """(ERF_SIZE,) float32 over [-3, 3]: every multiple of 1/256 in [-2, 2] -- the table-index boundaries -- with its two
    float32 neighbours, then uniform draws; shuffled, so the boundaries land in every part of the grid."""
    m = (np.arange(-512, 513) / 256.0).astype(F32)
    edge = np.concatenate([m, np.nextafter(m, F32(-4)), np.nextafter(m, F32(4))])
    rng = np.random.default_rng(4014)
    x = np.concatenate([edge, rng.uniform(-3, 3, ERF_SIZE - edge.size).astype(F32)])
    return x[rng.permutation(x.size)]


# ---- general broadcasting -----------------------------------------------------------------------------------------------
BCAST_EXTENTS = [1, 2, 3, 7, 16, 40]
BCAST_SEED = 20261017
BCAST_PAIRS = 60
BCAST_LARGE = 20                    # the first BCAST_LARGE pairs are drawn until the result has BCAST_LARGE_RANGE elements
BCAST_LARGE_RANGE = (1200000, 3000000)
BCAST_DEEP = 14                     # the next BCAST_DEEP are drawn until four or more axes are left after merging
BCAST_SMALL_MAX = 150000


def merged_axes(sa, sb):
    """Axes the broadcast of shapes sa, sb keeps after merging neighbours that both operands walk the same way (the rule of
    layer._binary_general, restated here independently from numpy strides)."""
    out = np.broadcast_shapes(tuple(sa), tuple(sb))
    nd = len(out)

    def strides(s):
        a = np.broadcast_to(np.empty(s, np.int8), out)
        return list(a.strides)
    dims = [(out[d], strides(sa)[d], strides(sb)[d]) for d in range(nd) if out[d] != 1] or [(1, 0, 0)]
    merged = [list(dims[0])]
    for n, a, b in dims[1:]:
        m = merged[-1]
        if m[1] == a * n and m[2] == b * n:
            merged[-1] = [m[0] * n, a, b]
        else:
            merged.append([n, a, b])
    return len(merged)


def broadcast_pairs(seed=BCAST_SEED, count=BCAST_PAIRS):
    """`count` shape pairs, ranks 0-6 on each side, extents from BCAST_EXTENTS, each operand keeping a random number of the
    result's trailing axes with extents of 1 sprinkled in.  The first BCAST_LARGE are redrawn until the result is past the
    streaming grid of a 256-CU part (and small enough for a quick test), the next BCAST_DEEP until the pair is small and keeps
    four or more axes after merging, the rest until it is small."""
    rng = np.random.default_rng(seed)
    pairs = []
    while len(pairs) < count:
        nd = int(rng.integers(1, 7))
        full = [int(rng.choice(BCAST_EXTENTS)) for _ in range(nd)]

        def operand():
            keep = int(rng.integers(0, nd + 1))
            return tuple(d if rng.random() < 0.6 else 1 for d in full[nd - keep:])
        sa, sb = operand(), operand()
        size = int(np.prod(np.broadcast_shapes(sa, sb), dtype=np.int64))
        if len(pairs) < BCAST_LARGE:
            ok = BCAST_LARGE_RANGE[0] <= size <= BCAST_LARGE_RANGE[1]
        elif len(pairs) < BCAST_LARGE + BCAST_DEEP:
            ok = size <= BCAST_SMALL_MAX and merged_axes(sa, sb) >= 4
        else:
            ok = size <= BCAST_SMALL_MAX
        if ok:
            pairs.append((sa, sb))
    return pairs


def broadcast_operands(i, sa, sb, positive=False):
    rng = np.random.default_rng([BCAST_SEED, i])
    a, b = rng.standard_normal(sa).astype(F32), rng.standard_normal(sb).astype(F32)
    if positive:
        a = (np.abs(a) + F32(0.1)).astype(F32)
    return a, b

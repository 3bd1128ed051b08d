"""pl_topk_select_f32 on a real MI355X: the k greatest of every row by radix selection, against
np.argsort(kind="stable") read from its end.  Indices are compared exactly and values as uint32 patterns; nothing has a
tolerance.  The C entry is called directly, on a scratch block full of 0xA5 and on outputs with one spare row of sentinels on
either side, so the small shapes do not depend on routing.  C is the chunk a workgroup takes."""
import numpy as np
import pytest

from planer_amd import _lib
from tests import ref_index as R
from tests.head_kit import EINVAL, EUNSUPPORTED, OK, SENT

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
C, MAX_K = _lib.TOPK_SELECT_CHUNK, _lib.TOPK_SELECT_MAX_K


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _filled(pa, words):
    buf = pa.hip.empty((words,), U32)
    buf.set(np.full(words, SENT, U32))
    return buf


def select(pa, x, k):
    """pl_topk_select_f32 on host x (outer, n, inner) -> (status, values, indices, whether the spare rows are intact)."""
    outer, n, inner = x.shape
    spare = k * inner
    dx = pa.hip.asarray(np.ascontiguousarray(x))
    vals, idx = _filled(pa, (outer + 2) * spare), _filled(pa, (outer + 2) * spare * 2)
    scratch = _filled(pa, pa.util._topk_select_scratch_bytes(outer * inner, n, k) // 4 + 2)
    rc = _lib.load().pl_topk_select_f32(pa.hip.context().handle, dx.ptr, outer, n, inner, k, scratch.ptr, vals.ptr + 4 * spare,
                                        idx.ptr + 8 * spare)
    v, i = vals.get(), idx.get()
    intact = all((w[:e] == SENT).all() and (w[-e:] == SENT).all() for w, e in ((v, spare), (i, 2 * spare)))
    return rc, v[spare:-spare].reshape(outer, k, inner), i[2 * spare:-2 * spare].view(np.int64).reshape(outer, k, inner), intact


def check(pa, x, ks, what):
    """x (outer, n, inner) at every k of ks against the stable argsort along axis 1."""
    order = np.argsort(x, axis=1, kind="stable")
    for k in ks:
        wv, wi = R.topk_ref(x, k, 1, 1, order=order)
        rc, gv, gi, intact = select(pa, x, k)
        assert rc == OK and intact, (what, k, rc, intact)
        R.assert_same(gi, wi, "%s k=%d indices" % (what, k))
        R.assert_same(gv, wv.view(U32), "%s k=%d values" % (what, k))


@pytest.mark.parametrize("n", [1, 2, 65, C - 1, C, C + 1, 2 * C + 1, 16385])
def test_every_data_class(pa, n):
    """Three rows of every class: one chunk, the chunk seam, a ragged last chunk; rows 1 and 2 start off a 16-byte boundary
    where n % 4 != 0."""
    for cls in R.TOPK_CLASSES:
        check(pa, R.topk_data(cls, 3, n)[:, :, None], sorted({1, min(n, 7), min(n, 300), min(n, MAX_K)}), "%s n=%d" % (cls, n))


@pytest.mark.parametrize("kind", ["number", "nan", "zeros"])
def test_the_cut_among_equal_values(pa, kind):
    """n = 2C + 1.  Row 0 is one repeated value: nothing is above the threshold and every output is a tie.  Row 1 has five other
    elements (greater ones, or for NaN lesser ones: nothing is greater), none in the last chunk, which is a single tie.  The
    cuts: that one tie (r = 1, all of the last chunk), part of the middle chunk, exactly up to the seam and one past it, and
    every tie (k = n).  zeros: +0 and -0 mixed share a key, and their bits come back."""
    n = 2 * C + 1
    fill = {"number": np.full(n, 1.5, F32), "nan": np.full(n, np.nan, F32),
            "zeros": np.where(np.random.default_rng(3).random(n) < 0.5, F32(0.0), F32(-0.0)).astype(F32)}[kind]
    x = np.stack([fill, fill])
    x[1, [3, C - 1, C, C + 5, 2 * C - 1]] = [2.0, 3.0, 2.0, np.inf, 2.5]
    ties_mid = C - 3
    check(pa, x[:, :, None], [1, 5, 5 + 1, 5 + 1 + 100, 5 + 1 + ties_mid, 5 + 1 + ties_mid + 1, n - 5, n], kind)


def _consecutive(first_bits, count):
    """`count` consecutive float32 upwards from the one with bits `first_bits`, by np.nextafter."""
    out = [np.array(first_bits, U32).view(F32)[()]]
    for _ in range(count - 1):
        out.append(np.nextafter(out[-1], F32(np.inf)))
    return np.array(out, F32)


@pytest.mark.parametrize("first", [0x3F800000, 0x3F800000 - 1500, 0x80000000 + 1500], ids=["above 1.0", "across 1.0", "across zero"])
def test_neighbouring_floats(pa, first):
    """3000 consecutive floats, shuffled (no 3000 neighbours fit one 1024-wide bin of the last digit).  Upwards from 1.0 they
    share the top 11-bit digit of the key and cross two edges of the second, so the last two digits decide; across 1.0 the top
    digit changes in the middle; from -1500 denormal steps through -0 to +1499 the sign flip of the key decides."""
    x = _consecutive(first, 3000)
    assert np.unique(x).size == 3000
    x = x[np.random.default_rng(first).permutation(3000)]
    check(pa, x[None, :, None], [1, 7, 1500, 3000], hex(first))


@pytest.mark.parametrize("shape", [(2, C + 1, 7), (300, C + 1, 1)])
def test_layouts(pa, shape):
    """A strided axis, and more rows than a grid row of chunks; the spare output rows around stay sentinels (select)."""
    outer, n, inner = shape
    x = R.topk_data("ties", outer * inner, n, seed=1)
    x[1::2] = R.topk_data("specials", outer * inner, n, seed=1)[1::2]
    check(pa, np.ascontiguousarray(x.reshape(outer, inner, n).transpose(0, 2, 1)), [7], str(shape))


def test_refusals_leave_the_outputs_untouched(pa):
    lib, h = _lib.load(), pa.hip.context().handle
    x = pa.hip.asarray(R.topk_data("ties", 6, 5000))
    vals, idx, scratch = _filled(pa, 6 * 4096), _filled(pa, 6 * 4096 * 2), _filled(pa, pa.util._topk_select_scratch_bytes(6, 5000, 4096) // 4)
    ok = dict(x=x.ptr, outer=6, n=5000, inner=1, k=9, scratch=scratch.ptr, values=vals.ptr, indices=idx.ptr)
    bad = [(dict(x=None), EINVAL), (dict(scratch=None), EINVAL), (dict(values=None), EINVAL), (dict(indices=None), EINVAL),
           (dict(n=0), EINVAL), (dict(n=-5), EINVAL), (dict(k=0), EINVAL), (dict(k=-1), EINVAL), (dict(k=5001), EINVAL),
           (dict(outer=-1), EINVAL), (dict(inner=-1), EINVAL), (dict(k=MAX_K + 1), EUNSUPPORTED),
           (dict(outer=1 << 16, inner=1 << 15, n=9), EUNSUPPORTED), (dict(outer=1 << 16, inner=1, n=1 << 15), EUNSUPPORTED)]
    for change, code in bad:
        assert lib.pl_topk_select_f32(h, *dict(ok, **change).values()) == code, change
        assert lib.pl_last_error(), change
    assert lib.pl_topk_select_f32(None, *ok.values()) == EINVAL
    assert lib.pl_topk_select_f32(h, *dict(ok, outer=0).values()) == OK                     # nothing to do, nothing launched
    pa.hip.context().synchronize()
    assert all((b.get() == SENT).all() for b in (vals, idx, scratch))
    assert lib.pl_topk_select_f32(h, *ok.values()) == OK and (idx.get()[:6 * 9 * 2] != SENT).any()


def test_routing_gives_the_same_bits(pa, monkeypatch):
    """layer.TopK and util.nms with PLANER_HIP_TOPK_SELECT=0 and =force: other entries, equal results."""
    rng = np.random.default_rng(5)
    x = pa.asarray(R.topk_data("ties", 3, 20000) + rng.integers(0, 2, (3, 20000)).astype(F32) / 2)
    corner = rng.uniform(0, 600, (1, 20000, 2)).astype(F32)
    boxes = pa.hip.asarray(np.concatenate([corner, corner + rng.uniform(5, 60, (1, 20000, 2)).astype(F32)], -1))
    scores = pa.hip.asarray(rng.integers(0, 4000, (1, 20000)).astype(F32) / 4000)
    seen, got = [], {}
    monkeypatch.setattr(_lib, "_recorder", lambda name, args: seen.append(name))
    for switch in ("0", "force"):
        monkeypatch.setenv("PLANER_HIP_TOPK_SELECT", switch)
        del seen[:]
        got[switch] = [a.get() for a in pa.layer_map["topk"](x, np.int64(300)) + pa.util.nms(boxes, scores, iou=0.5, max_det=100)]
        assert seen.count("pl_topk_select_f32") == (2 if switch == "force" else 0) and seen.count("pl_topk_f32") == (0 if switch == "force" else 2)
    for a, b in zip(got["0"], got["force"]):
        R.assert_same(a.view(U32) if a.dtype == F32 else a, b.view(U32) if b.dtype == F32 else b, "routing")

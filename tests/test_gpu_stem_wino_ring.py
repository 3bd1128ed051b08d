"""The ring of k-quads in the F(4,4) stem + max-pool kernel (csrc/conv_stem_wino_kernel.h): V holds absolute k-quad Q at ring
position Q mod 20, a step transforms only its 4 new input rows and the conv rows read their 11 filter quads from position
(6 t + 3 rsel) mod 20 on.  6 t mod 20 has a period of 10 steps: strips of 15 steps run it once and a half.

* the kernel under the per-element bound of tests/stem_wino_ref.py (LAMBDA = 3.5, as tests/test_gpu_stem_wino.py) on shapes
  with long strips; worst err / tol measured on an MI355X: 0.341 on (1, 56, 32), 0.223 and 0.252 on the others;
* strips of 7 and of 14 pooled rows give the same bits: a conv row's sums do not depend on where its strip starts or where its
  quads sit in the ring, so any ring-offset error shows here.  The commit before the ring (V rebuilt whole in every step) passes
  this test too, as it does the others of this file: there the two strip sizes were already equal bit for bit;
* a NaN or an inf in input row h changes no bit of a pooled row that does not read h (rows 4 q - 5 .. 4 q + 5), however many
  steps later its ring quads are reused or lie under the two dead k values of a conv row's last quad; the pooled rows that do
  read h are non-finite in the columns of the poisoned tile.  For a NaN that is every such element.  An inf reaches the
  frequencies with both signs, so a pixel is NaN or +-inf, and a -inf loses the max-pool to a finite neighbour (another tile's
  pixel, another conv row, the pool's zero padding or its -1e4 start): there the test asks for a non-finite value in every such
  pooled row, not in every element.
  With k = 6 a + 2 c + phase (a: input row of the strip, image row h = 4 p0 - 5 + a under first pooled row p0; c: channel) the
  dead k values of step t hold: for conv row 0 (k = 24 t + 42, 43) row a = 4 t + 7 of channel 0, which the other conv row reads
  but pooled row t - 1 of the strip, fed by conv row 0, does not; for conv row 1 (k = 24 t + 54, 55) row a = 4 t + 9 of channel
  0 once the step's transform has written it -- pooled row t reads that row anyway -- and before that the stale k - 80: row
  a = 4 t - 5 of channel 2, which pooled row t does not read.  The rows of the issue's list never land there (a = 3 mod 4 and
  channel 0 or 2 are needed), and with finite data the zero filter values hide the slot, so DEAD adds rows that do: they are
  what fails if `cut` stops holding for either conv row."""
import numpy as np
import pytest

from tests import ref64 as R
from tests import stem_wino_ref as S
from tests.ref64 import ACT_NONE
from tests.test_gpu_stem_wino import TAILS, _run

pytestmark = pytest.mark.gpu
# one 14-row strip of 15 steps, 4 tiles; three 7-row strips (the last of 2 pooled rows) or a whole and a partial 14-row strip;
# two column chunks under a 15-step strip
SHAPES = [(1, 56, 32), (1, 64, 40), (1, 60, 300)]
IDS = ["%dx%dx%d" % s for s in SHAPES]
_CASES = {}


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _cases(shape):
    """[(tail index, cout, operands, act, pooled reference, pooled bound)]: all three tails on the first shape, scale + shift + ReLU
    on the others; Cout 64 and 36 (a partial 64-channel block).  Made once per shape."""
    if shape not in _CASES:
        from tests.test_gpu_conv_bounds import _operands
        n, h, w = shape
        out = []
        for t, tail in enumerate(TAILS):
            if t != 1 and shape != SHAPES[0]:
                continue
            for cout, dc in ((64, 0.0), (36, 50.0)):
                ops, act, want = _operands("stem-wino-ring", (n, 3, h, w), (cout, 3, 7, 7), tail, dc, **S.CONV)
                x, K, B, sc, sh, _ = ops
                out.append((t, cout, (x, K, B, sc, sh), act, S.pooled(want), S.pooled(S.bound(x, K, B, sc, sh))))
        _CASES[shape] = out
    return _CASES[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_ring_wrap_within_the_bound(pa, shape):
    worst = 0.0
    for t, cout, ops, act, want, tol in _cases(shape):
        for strip_rows in (0, 14):
            y, plan, ext = _run(pa, *ops, act, strip_rows)
            assert ext[0] == 7 and ext[3] == 44, ext
            worst = max(worst, R.check(y, want, tol, "stem ring %s cout %d tail %d strip_rows %d" % (shape, cout, t, strip_rows), plan))
    print("ratio stem-wino-ring %.3g %s" % (worst, shape))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_strip_size_does_not_change_a_bit(pa, shape):
    for t, cout, ops, act, _, _ in _cases(shape):
        y7, plan7, _ = _run(pa, *ops, act, 7)
        y14, plan14, _ = _run(pa, *ops, act, 14)
        assert "of 7 rows" in plan7 and "of 14 rows" in plan14, (plan7, plan14)
        same = y7.view(np.uint32) == y14.view(np.uint32)
        assert same.all(), "%s cout %d tail %d: %d of %d values differ, first at %s" % (
            shape, cout, t, (~same).sum(), same.size, tuple(int(v) for v in np.argwhere(~same)[0]))


# (channel, input row h) that lie under a dead k at H = 56 with strips of 7 and of 14 pooled rows alike (the strips start at
# pooled rows 0 and 7: a = h + 5 or h - 23).  Conv row 0: a = 11 = 4 * 1 + 7 and, 8 steps or one strip later, h = 34.  Conv row 1,
# stale: a = 7 = 4 * 3 - 5 and, 7 steps or one strip later, h = 30
DEAD = [(0, 6), (0, 34), (2, 2), (2, 30)]


def _dead_k_readers(c, h, prows, Hq):
    """Pooled rows that do not read input row h of channel c, but are fed by a conv row that finds it under a dead k."""
    out = []
    for p0 in range(0, Hq, prows):
        steps = min(prows, Hq - p0) + 1
        a = h + 5 - 4 * p0
        for t in range(steps):
            if c == 0 and a == 4 * t + 7 and t >= 1:                # conv row 0 of step t: pooled rows t - 1 and t of the strip
                out.append(p0 + t - 1)
            if c == 2 and a == 4 * t - 5 and t < steps - 1:         # conv row 1 of step t (stale quad): pooled row t of the strip
                out.append(p0 + t)
    return out


@pytest.mark.parametrize("strip_rows", [7, 14])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_non_finite_input_stays_in_the_rows_that_read_it(pa, bad, strip_rows):
    n, H, W = SHAPES[0]
    t, cout, (x, K, B, sc, sh), act, _, _ = _cases(SHAPES[0])[0]
    assert (B, sc, sh) == (None, None, None) and act == ACT_NONE       # no tail: nothing between the sums and the pool
    clean, plan, _ = _run(pa, x, K, None, None, None, act, strip_rows)
    assert "of %d rows" % strip_rows in plan, plan
    assert np.isfinite(clean).all()
    Hq = clean.shape[2]
    q = np.arange(Hq)
    wcol, cols = 12, slice(2, 5)        # input column 12 is read by tile 1 alone (its columns 5 .. 18): conv columns 4 .. 7, pooled 2 .. 4
    for c, h in [(1, h) for h in (0, 7, 8, 27, H - 1)] + DEAD:
        xp = x.copy()
        xp[0, c, h, wcol] = bad
        y, _, _ = _run(pa, xp, K, None, None, None, act, strip_rows)
        reads = (4 * q - 5 <= h) & (h <= 4 * q + 5)
        assert reads.any() and not reads.all()
        if (c, h) in DEAD:              # the value does meet a dead k of a conv row whose pooled row must not change
            seen = _dead_k_readers(c, h, strip_rows, Hq)
            assert seen and not reads[seen].any(), (c, h, seen)
        same = y[:, :, ~reads].view(np.uint32) == clean[:, :, ~reads].view(np.uint32)
        assert same.all(), "channel %d row %d: pooled rows %s changed" % (c, h, sorted(set(q[~reads][np.argwhere(~same)[:, 2]].tolist())))
        hit = ~np.isfinite(y[:, :, reads][..., cols])
        if np.isnan(bad):
            assert hit.all(), "channel %d row %d: %d finite values in the pooled rows %s" % (c, h, (~hit).sum(), q[reads].tolist())
        else:
            assert hit.any(axis=(0, 1, 3)).all(), "channel %d row %d: an all-finite pooled row among %s" % (c, h, q[reads].tolist())

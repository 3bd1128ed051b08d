"""Keypoints as net output on a real MI355X (pl_peaks_f32, util.heatmap_peaks, util.KeypointSpec, Net.keypoint_output;
DESIGN 4.27).

Everything is exact: peaks and num equal tests/peaks_ref.py's bit for bit, which tests/test_peaks_ref.py holds to scipy's maximum
filter, np.lexsort and np.argmax.  The two launches write into outputs framed by sentinel words that must survive, from a scratch
block filled with a poison pattern; one pass over the whole case list runs with the pool in hygiene mode, where scratch read
before it is written shows up as a wrong answer and a write past a block as a dirty guard.  Shapes come from the tile extent, the
merge capacity and the row limit the header states.  Then nets: every call form against the reference applied to what a second,
undeclared instance returns."""
import functools

import numpy as np
import pytest

from tests import head_kit as K
from tests import peaks_ref as R
from tests.head_kit import EINVAL, EUNSUPPORTED, F32, I32, OK, Framed

pytestmark = pytest.mark.gpu

NAMES = ("peaks", "num")
TIES, REFINE = {"all": 0, "first": 1}, {"none": 0, "quarter": 1}

_C = K.header_constants("PL_PEAKS_")
TH, TW, MERGE_KEYS, MAX_PEAKS, MAX_EXTENT = (_C["PL_PEAKS_" + k] for k in ("TILE_H", "TILE_W", "MERGE_KEYS", "MAX_PEAKS", "MAX_EXTENT"))

MULTI_ROUND = (1, 1, TH, (MERGE_KEYS // MAX_PEAKS + 1) * TW)                   # tiles x MAX_PEAKS candidates > MERGE_KEYS
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 1, TH, TW), (1, 2, TH - 1, TW - 1), (2, 1, TH + 1, TW + 1), (1, 1, 2 * TH + 3, 3 * TW + 5),
          (1, 1, 1, 4 * TW + 1), (1, 1, 4 * TH + 1, 1), (1, 3, TH + 2, TW + 1), MULTI_ROUND, (1, 2, TH + 3, 2 * TW + 4)]
MAX_PEAKS_CYCLE = (1, 3, MAX_PEAKS)
STRIDES = ((1, 1), (4, 4), (7.5, 3.3))


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def scratch_bytes(n, k, h, w, max_peaks):
    """PL_PEAKS_SCRATCH_BYTES"""
    return n * k * (-(-h // TH)) * (-(-w // TW)) * (max_peaks * 8 + 4)


@functools.lru_cache(maxsize=None)
def cases(shape):
    """[(name, x, threshold, ties, max_peaks, refine, stride, (peaks, num))] for one shape: computed once, shared, read-only.
    Every pattern under both `ties` and both `refine`; max_peaks and stride cycle through their values along the list, and the
    random maps get all three max_peaks."""
    n, k, h, w = shape
    seed = h * 1000 + w
    maps = [("random, max_peaks %d" % mp, R.random_maps(n, k, h, w, seed + i), 0.0, mp) for i, mp in enumerate(MAX_PEAKS_CYCLE)]
    maps += [("quantised", R.quantised(n, k, h, w, seed), -0.125, None), ("smooth quantised", R.smooth_quantised(n, k, h, w, seed), 0.0, None),
             ("constant", R.constant(n, k, h, w), 0.0, None), ("seams", R.seams(n, k, h, w, TH, TW, seed), 0.0, None),
             ("borders", R.borders(n, k, h, w), 0.0, None), ("NaN", R.with_nan(n, k, h, w, TH, TW, seed), -0.5, None),
             ("inf", R.with_inf(n, k, h, w, seed), 0.0, None), ("inf, threshold -inf", R.with_inf(n, k, h, w, seed + 1), -np.inf, None),
             ("zeros of both signs", R.zeros_mixed(n, k, h, w, seed), -1.0, None), ("below threshold", R.random_maps(n, k, h, w, seed + 5), 1.0, None),
             ("threshold +inf", R.with_inf(n, k, h, w, seed + 2), np.inf, None), ("lattice, cut in a tie", R.lattice(n, k, h, w), 0.0, 3),
             ("lattice", R.lattice(n, k, h, w), 0.0, MAX_PEAKS)]
    out, c = [], 0
    for name, x, t, mp in maps:
        for ties in ("all", "first"):
            for refine in ("none", "quarter"):
                mp_c = mp or MAX_PEAKS_CYCLE[c % 3]
                stride = STRIDES[(c // 3) % 3]
                c += 1
                ref = R.peaks_ref(x, t, ties, mp_c, refine, stride)
                for a in (x,) + ref:
                    a.setflags(write=False)
                out.append(("%s %s, %s, %s, max_peaks %d, stride %s" % (shape, name, ties, refine, mp_c, stride), x, t, ties, mp_c, refine,
                            stride, ref))
    return out


def chain(pa, x, threshold, ties, max_peaks, refine, stride):
    """pl_peaks_f32 through the C interface on framed outputs and a poisoned scratch block.
    -> (status, (peaks, num), every frame intact)."""
    ctx = pa.hip.context()
    n, k, h, w = x.shape
    dev = pa.hip.asarray(x) if x.size else pa.hip.empty(x.shape, F32)
    peaks, num = Framed(pa, n * k * max_peaks * 3), Framed(pa, n * k)
    scratch = Framed(pa, scratch_bytes(n, k, h, w, max_peaks) // 4 + 2)        # (PAD = 16 words: the block stays 8-byte aligned)
    rc = pa._lib.load().pl_peaks_f32(ctx.handle, dev.ptr, n, k, h, w, float(threshold), TIES[ties], max_peaks, REFINE[refine],
                                     float(stride[0]), float(stride[1]), scratch.ptr, peaks.ptr, num.ptr)
    p, ok_p = peaks.get(F32, (n, k, max_peaks, 3))
    c, ok_c = num.get(I32, (n, k))
    return rc, (p, c), ok_p and ok_c and scratch.get(np.uint32, (-1,))[1]


def same(got, want, what):
    K.same(got, want, NAMES, what)


def test_the_case_list_covers_what_it_claims():
    """On the reference alone: the random maps include planes with more peaks than rows and planes with fewer (and some), the
    multi-round shape needs more than one merge round, the lattice's cut falls between equal scores of different tiles."""
    more = fewer = 0
    for shape in SHAPES:
        for what, x, t, ties, mp, refine, stride, (peaks, num) in cases(shape):
            assert not np.isnan(peaks).any(), what
            if "random" in what:
                more += int((num > mp).sum())
                fewer += int(((num > 0) & (num < mp)).sum())
            if "constant" in what:
                assert (num == (x.shape[2] * x.shape[3] if ties == "all" else 1)).all(), what
            if "below" in what or "+inf" in what:
                assert not num.any() and not peaks.view(np.uint32).any(), what
    assert more >= 20 and fewer >= 20, (more, fewer)
    n, k, h, w = MULTI_ROUND
    assert (-(-h // TH)) * (-(-w // TW)) * MAX_PEAKS > MERGE_KEYS
    full = [c for c in cases(MULTI_ROUND) if c[4] == MAX_PEAKS and (c[7][1] > MAX_PEAKS).all()]
    assert len(full) >= 4, len(full)                                          # ... and with every tile's candidates in use
    for what, x, t, ties, mp, refine, stride, (peaks, num) in cases((1, 1, 2 * TH + 3, 3 * TW + 5)):
        if "cut in a tie" in what:
            assert mp == 3 and (num > 100).all() and (peaks[..., 2] == 1).all()
    x = R.lattice(*MULTI_ROUND)
    peaks, num = R.peaks_ref(x, 0.0, "all", MAX_PEAKS, "none", (1, 1))
    assert num[0, 0] > MAX_PEAKS and (peaks[0, 0, :, 2] == 1).all() and len({int(v) // TW for v in peaks[0, 0, :, 0]}) > 1
    assert peaks[0, 0, -1, 1] < x.shape[2] - 3                                # the cut leaves equal peaks of the same tiles out


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_chain_equals_the_reference(pa, shape):
    for i, (what, x, t, ties, mp, refine, stride, ref) in enumerate(cases(shape)):
        rc, got, intact = chain(pa, x, t, ties, mp, refine, stride)
        assert rc == OK and intact, what
        same(got, ref, what)
        if i % 7 == 0:                                                         # two runs of one input: identical bytes
            again = chain(pa, x, t, ties, mp, refine, stride)[1]
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), what


def test_hygiene_pass_over_every_case(pa):
    """util.heatmap_peaks on every case with the pool in hygiene mode: fresh blocks are poisoned and guarded."""
    K.hygiene_pass(pa, [case for shape in SHAPES for case in cases(shape)],
                   lambda x, *spec: pa.util.heatmap_peaks(pa.hip.asarray(x), *spec), NAMES, 500)


def test_heatmap_peaks_on_two_three_and_four_dimensions(pa):
    x = R.smooth_quantised(2, 3, TH + 3, TW + 9, 11)
    spec = dict(threshold=-0.125, ties="first", max_peaks=40, refine="quarter", stride=(4, 2))
    ref = R.peaks_ref(x, **spec)
    got = pa.util.heatmap_peaks(pa.hip.asarray(x), **spec)
    assert [a.shape for a in got] == [(2, 3, 40, 3), (2, 3)]
    same(tuple(a.get() for a in got), ref, "4-d")
    got = pa.util.heatmap_peaks(pa.hip.asarray(x[1]), **spec)
    assert [a.shape for a in got] == [(3, 40, 3), (3,)]
    same(tuple(a.get() for a in got), (ref[0][1], ref[1][1]), "3-d")
    got = pa.util.heatmap_peaks(pa.hip.asarray(x[1, 2]), **spec)
    assert [a.shape for a in got] == [(40, 3), ()]
    same(tuple(a.get() for a in got), (ref[0][1, 2], ref[1][1, 2]), "2-d")
    # the defaults
    same(tuple(a.get() for a in pa.util.heatmap_peaks(pa.hip.asarray(x))), R.peaks_ref(x), "defaults")
    # max_peaks = 1, ties = "first", threshold = -inf: numpy's argmax of each plane
    x = R.random_maps(2, 5, 2 * TH + 1, TW + 7, 12)
    x[0, 0, 7, 5] = x[0, 0, TH + 2, TW + 1] = 2                              # equal maxima in different tiles: the first
    peaks, num = (a.get() for a in pa.util.heatmap_peaks(pa.hip.asarray(x), -np.inf, "first", 1))
    am = x.reshape(2, 5, -1).argmax(2)
    assert (peaks[:, :, 0, 0] == am % x.shape[3]).all() and (peaks[:, :, 0, 1] == am // x.shape[3]).all() and (num >= 1).all()
    assert (peaks[0, 0, 0] == [5, 7, 2]).all() and (peaks[:, :, 0, 2] == x.max(axis=(2, 3))).all()
    # an empty plane, an empty batch
    peaks, num = pa.util.heatmap_peaks(pa.hip.empty((2, 2, 0, 5), F32), max_peaks=3)
    assert peaks.shape == (2, 2, 3, 3) and not num.get().any() and not peaks.get().view(np.uint32).any()
    peaks, num = pa.util.heatmap_peaks(pa.hip.empty((0, 4, 5, 5), F32))
    assert peaks.shape == (0, 4, 32, 3) and num.shape == (0, 4)


def test_refusals_leave_the_outputs_untouched(pa):
    ctx = pa.hip.context()
    lib = pa._lib.load()
    x = pa.hip.asarray(R.random_maps(2, 3, 9, 11, 1))
    peaks, num = Framed(pa, 2 * 3 * 4 * 3), Framed(pa, 2 * 3)
    scratch = Framed(pa, scratch_bytes(2, 3, 9, 11, 4) // 4 + 2)
    nan = float("nan")
    ok = dict(x=x.ptr, N=2, K=3, H=9, W=11, threshold=0.0, ties=0, max_peaks=4, refine=1, sy=4.0, sx=4.0, scratch=scratch.ptr,
              peaks=peaks.ptr, num=num.ptr)
    bad = [(dict(x=None), EINVAL), (dict(scratch=None), EINVAL), (dict(peaks=None), EINVAL), (dict(num=None), EINVAL),
           (dict(N=-1), EINVAL), (dict(K=-1), EINVAL), (dict(H=-1), EINVAL), (dict(W=-2), EINVAL), (dict(max_peaks=0), EINVAL),
           (dict(max_peaks=-3), EINVAL), (dict(ties=2), EINVAL), (dict(ties=-1), EINVAL), (dict(refine=2), EINVAL), (dict(refine=-1), EINVAL),
           (dict(threshold=nan), EINVAL), (dict(sy=nan), EINVAL), (dict(sx=nan), EINVAL),
           (dict(max_peaks=MAX_PEAKS + 1), EUNSUPPORTED), (dict(N=1, K=1, H=1, W=MAX_EXTENT + 1), EUNSUPPORTED),
           (dict(N=1, K=1, H=MAX_EXTENT + 1, W=1), EUNSUPPORTED), (dict(N=1, K=1, H=46341, W=46341), EUNSUPPORTED),
           (dict(N=1 << 6, K=1 << 5, H=1 << 10, W=1 << 10), EUNSUPPORTED), (dict(N=1 << 16, K=1 << 12, H=1, W=1, max_peaks=3), EUNSUPPORTED)]
    for change, code in bad:
        args = dict(ok, **change)
        assert lib.pl_peaks_f32(ctx.handle, *args.values()) == code, change
        assert lib.pl_last_error(), change
    assert lib.pl_peaks_f32(None, *ok.values()) == EINVAL
    for change in (dict(N=0), dict(K=0), dict(N=0, H=0)):                     # nothing to do: PL_OK without a launch
        assert lib.pl_peaks_f32(ctx.handle, *dict(ok, **change).values()) == OK, change
    ctx.synchronize()
    assert peaks.untouched() and num.untouched() and scratch.untouched()
    # an empty plane: num = 0 and every row +0.0, written
    assert lib.pl_peaks_f32(ctx.handle, *dict(ok, H=0).values()) == OK
    p, intact = peaks.get(np.uint32, (-1,))
    c, intact2 = num.get(I32, (-1,))
    assert intact and intact2 and not p.any() and not c.any() and scratch.untouched()
    assert lib.pl_peaks_f32(ctx.handle, *ok.values()) == OK                   # ... and the arguments they were derived from run
    assert num.get(I32, (-1,))[0].any()


def test_chain_replays_from_a_captured_graph(pa):
    """No host wait and no host-computed value: the two launches captured once answer for whatever is in their input at launch."""
    n, k, h, w, mp = 2, 2, TH + 5, 2 * TW + 4, 20
    maps = [R.random_maps(n, k, h, w, 21), R.constant(n, k, h, w), R.with_nan(n, k, h, w, TH, TW, 22), R.smooth_quantised(n, k, h, w, 23)]
    x = pa.hip.empty((n, k, h, w), F32)
    peaks, num = pa.hip.empty((n, k, mp, 3), F32), pa.hip.empty((n, k), I32)
    scratch = pa.hip.empty(((scratch_bytes(n, k, h, w, mp) + 7) // 8,), np.int64)
    K.replay_from_captured_graph(
        pa, lambda: pa._lib.load().pl_peaks_f32(pa.hip.context().handle, x.ptr, n, k, h, w, -0.5, 1, mp, 1, 4.0, 4.0, scratch.ptr, peaks.ptr, num.ptr),
        x, (peaks, num), maps, lambda host: R.peaks_ref(host, -0.5, "first", mp, "quarter", (4, 4)), NAMES)


def test_a_large_map_with_a_known_answer(pa):
    """Several hundred tiles and many merge rounds; the answer by construction: distinct values on a lattice, the largest last."""
    h, w = 16 * TH + 7, 20 * TW + 9
    x = np.zeros((1, 1, h, w), F32)
    ys, xs = np.meshgrid(np.arange(1, h, 4), np.arange(2, w, 4), indexing="ij")
    values = (1 + np.arange(ys.size, dtype=np.int64) * 3 % 1021).astype(F32)   # many equal scores across tiles
    x[0, 0, ys.ravel(), xs.ravel()] = values
    order = np.lexsort((ys.ravel() * w + xs.ravel(), -values))[:MAX_PEAKS]
    peaks, num = (a.get() for a in pa.util.heatmap_peaks(pa.hip.asarray(x), max_peaks=MAX_PEAKS, stride=4))
    assert num.tolist() == [[ys.size]] and ys.size > 20 * MAX_PEAKS
    assert (peaks[0, 0, :, 0] == xs.ravel()[order] * 4).all() and (peaks[0, 0, :, 1] == ys.ravel()[order] * 4).all()
    assert (peaks[0, 0, :, 2] == values[order]).all()
    same((peaks, num), R.peaks_ref(x, 0.0, "all", MAX_PEAKS, "none", 4), "large")
    # a constant plane: every pixel under "all", one under "first"; everything below the threshold: nothing
    c = R.constant(1, 1, h, w)
    for ties in ("all", "first"):
        same(tuple(a.get() for a in pa.util.heatmap_peaks(pa.hip.asarray(c), 0.0, ties, 7, "quarter")), R.peaks_ref(c, 0.0, ties, 7, "quarter"),
             "constant, " + ties)
    peaks, num = (a.get() for a in pa.util.heatmap_peaks(pa.hip.asarray(c), 0.5, "all", 7))
    assert not num.any() and not peaks.view(np.uint32).any()


# ---- nets -------------------------------------------------------------------------------------------------------------------
SPEC = dict(threshold=0.0, ties="first", max_peaks=64, refine="quarter", stride=(2, 2))


def _want(maps):
    ref = R.peaks_ref(maps, **SPEC)
    assert ref[1].min() >= 2 and (ref[1] > SPEC["max_peaks"]).any() and (ref[1] < SPEC["max_peaks"]).any(), ref[1]
    return ref


@pytest.mark.parametrize("streams", [None, "pipe2"])
def test_tiny_net_every_call_form(pa, streams):
    K.check_every_call_form(pa, streams, lambda net, **at: net.keypoint_output(**at, **SPEC), _want, NAMES)


def test_one_output_net_and_uint8_input(pa):
    def mirror(maps):
        ref = R.peaks_ref(maps, **SPEC)
        assert ref[1].min() >= 1
        return ref

    net, x = K.check_one_output_net_and_uint8_input(pa, lambda net: net.keypoint_output(**SPEC), mirror, NAMES, [(2, 3, 64, 3), (2, 3)],
                                                    pa.util.KeypointSpec(**SPEC))
    # Net.tiled says that it does not take the declaration
    with pytest.raises(ValueError, match="keypoint output is declared"):
        net.tiled(x[0], window=16)
    pa.hip.trim_side_contexts()


def test_posenet_at_batch_two(pa):
    from planer_amd.irgen import posenet
    g, b = posenet.build()
    x = posenet.make_input(2)
    net = pa.from_graph(g, b)
    maps = net(x)                                                            # the same instance, so the same plan and the same maps
    assert maps.shape == (2, posenet.JOINTS, 64, 48)
    before = dict(net._plans)
    net.keypoint_output(threshold=float(np.median(maps)), max_peaks=16, refine="quarter", stride=posenet.STRIDE)
    got = net(x)
    assert all(net._plans[key] is before[key] for key in before)
    ref = R.peaks_ref(maps, float(np.median(maps)), "all", 16, "quarter", posenet.STRIDE)
    same(got, ref, "posenet")
    same(net.submit(x).get(), ref, "posenet, submit")
    net.keypoint_output(threshold=-np.inf, ties="first", max_peaks=1, stride=posenet.STRIDE)      # the single-person read-out
    peaks, num = net(x)
    am = maps.reshape(2, posenet.JOINTS, -1).argmax(2)
    assert (peaks[:, :, 0, 0] == am % 48 * 4).all() and (peaks[:, :, 0, 1] == am // 48 * 4).all()
    print("posenet: peaks per plane %s" % ref[1].tolist())
    pa.hip.trim_side_contexts()

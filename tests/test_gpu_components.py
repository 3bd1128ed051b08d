"""Objects as net output on a real MI355X (pl_components_u8_i32, util.connected_components, util.ObjectSpec,
Net.object_output, Net.tiled).

Everything is exact: labels, num, objects and centroids equal tests/components_ref.py's, which tests/test_components_ref.py holds
to scipy.ndimage.  The kernel chain writes into outputs framed by sentinel words that must survive, from a scratch block filled
with a poison pattern; one pass over the whole case list runs with the pool in hygiene mode, where scratch read before it is
written shows up as a wrong answer and a write past a block as a dirty guard.  Shapes come from the tile extent the header
states.  Then nets: every call form against the reference applied to the argmax of what a second, undeclared instance returns."""
import functools

import numpy as np
import pytest

from tests import components_ref as R
from tests import head_kit as K
from tests.head_kit import EINVAL, EUNSUPPORTED, F32, I32, OK, Framed

pytestmark = pytest.mark.gpu

NAMES = ("labels", "num", "objects", "centroids")

_C = K.header_constants("PL_CC_")
TH, TW, BLOCK, SCAN_STEP, MAX_OBJECTS = (_C["PL_CC_" + k] for k in ("TILE_H", "TILE_W", "BLOCK", "SCAN_STEP", "MAX_OBJECTS"))

SHAPES = [(1, 1, 1), (2, 5, 7), (1, TH, TW), (1, TH - 1, TW - 1), (2, TH + 1, TW + 1), (1, 2 * TH + 3, 3 * TW + 5), (1, 1, 4 * TW + 1),
          (1, 4 * TH + 1, 1), (3, TH + 2, TW + 2)]


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def scratch_bytes(n, h, w, max_objects):
    """PL_CC_SCRATCH_BYTES"""
    return n * max_objects * 16 + n * h * w * 4 + n * ((h * w + BLOCK - 1) // BLOCK) * 4


@functools.lru_cache(maxsize=None)
def cases(shape):
    """[(name, m, connectivity, background, max_objects, reference's four arrays)] for one shape: computed once, shared, read-only."""
    n, h, w = shape
    seed = h * 1000 + w
    maps = []
    for c in (4, 8):
        maps += [("binary %.1f" % d, R.random_binary(n, h, w, d, seed + i), c, 0, 256) for i, d in enumerate((0.3, 0.5, 0.6))]
        maps += [("classes", R.random_classes(n, h, w, 3, seed), c, 0, 256), ("checkerboard", R.checkerboard(n, h, w), c, 0, 7),
                 ("diagonal", R.diagonal(n, h, w), c, 0, 256), ("rings", R.rings(n, h, w), c, 0 if c == 8 else -1, 256)]
    maps += [("classes, background 2", R.random_classes(n, h, w, 3, seed + 1), 4, 2, 256),
             ("classes, no background", R.random_classes(n, h, w, 3, seed + 2), 8, -1, 256),
             ("all foreground", R.full(n, h, w, 5), 8, 0, 256), ("all foreground, class 0", R.full(n, h, w, 0), 4, -1, 3),
             ("all background", R.full(n, h, w, 9), 4, 9, 256), ("serpentine", R.serpentine(n, h, w), 4, 0, 256),
             ("serpentine", R.serpentine(n, h, w), 8, 0, 2), ("comb", R.comb(n, h, w), 4, 0, 256), ("row ends", R.row_ends(n, h, w), 8, 0, 256),
             ("image ends", R.image_ends(n, h, w), 4, 0, 256)]
    if w > TW and h >= 7:
        maps.append(("bridge", R.bridge(n, h, w, TW), 4, 0, 256))
    out = []
    for name, m, c, bg, mo in maps:
        ref = R.components_ref(m, c, bg, mo)
        for a in (m,) + ref:
            a.setflags(write=False)
        out.append(("%s %s, %d-connected" % (shape, name, c), m, c, bg, mo, ref))
    return out


def chain(pa, m, connectivity, background, max_objects, null_tables=False):
    """pl_components_u8_i32 through the C interface on framed outputs and a poisoned scratch block.
    -> (status, (labels, num, objects, centroids), every frame intact, the Framed outputs)."""
    ctx = pa.hip.context()
    n, h, w = m.shape
    dev = pa.hip.asarray(m) if m.size else pa.hip.empty(m.shape, np.uint8)
    frames = [Framed(pa, n * h * w), Framed(pa, n), Framed(pa, n * max_objects * 6), Framed(pa, n * max_objects * 2)]
    scratch = Framed(pa, scratch_bytes(n, h, w, max_objects) // 4 + 2)
    args = [f.ptr for f in frames]
    if null_tables:
        args[2] = args[3] = None
    rc = pa._lib.load().pl_components_u8_i32(ctx.handle, dev.ptr, n, h, w, connectivity, background, max_objects, scratch.ptr, *args)
    got, intact = [], scratch.get(np.uint32, (-1,))[1]
    for f, dt, shape in zip(frames, (I32, I32, I32, F32), ((n, h, w), (n,), (n, max_objects, 6), (n, max_objects, 2))):
        a, ok = f.get(dt, shape)
        got.append(a)
        intact = intact and ok
    return rc, tuple(got), intact, frames


def same(got, want, what):
    K.same(got, want, NAMES, what)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_chain_equals_the_reference(pa, shape):
    for what, m, c, bg, mo, ref in cases(shape):
        rc, got, intact, _ = chain(pa, m, c, bg, mo)
        assert rc == OK and intact, what
        same(got, ref, what)
        if "binary 0.6" in what or "classes," in what:                       # two runs of one input: identical bytes
            again = chain(pa, m, c, bg, mo)[1]
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), what


def test_the_patterns_are_what_they_claim(pa):
    """The properties the case list is there for, asserted on the device's own answers."""
    shape = (1, 2 * TH + 3, 3 * TW + 5)
    n, h, w = shape
    by_name = {what: (m, c, bg, mo, ref) for what, m, c, bg, mo, ref in cases(shape)}

    def run(name, c):
        m, c, bg, mo, ref = by_name["%s %s, %d-connected" % (shape, name, c)]
        rc, got, intact, _ = chain(pa, m, c, bg, mo)
        assert rc == OK and intact
        same(got, ref, name)
        return m, mo, got

    m, mo, (labels, num, objects, _) = run("checkerboard", 4)
    assert num[0] == (h * w + 1) // 2 > mo == 7                               # more objects than rows: the first seven have one
    assert labels.max() == num[0] and (objects[0, :, 1] == 1).all() and objects[0, :, 3].tolist() == [0, 2, 4, 6, 8, 10, 12]
    assert run("checkerboard", 8)[2][1][0] == 1
    m, _, (labels, num, objects, _) = run("serpentine", 4)
    assert num[0] == 1 and objects[0, 0].tolist() == [1, (h + 1) // 2 * w + h // 2, 0, 0, h, w]
    assert run("comb", 4)[2][1][0] == 1
    assert run("diagonal", 8)[2][1][0] == 1 and run("diagonal", 4)[2][1][0] == h
    assert run("row ends", 8)[2][1][0] == h
    assert run("all foreground", 8)[2][2][0, 0].tolist() == [5, h * w, 0, 0, h, w]
    assert run("all background", 4)[2][1][0] == 0
    assert run("bridge", 4)[2][1][0] == 1
    # images do not join and the numbering restarts
    for what, m, c, bg, mo, ref in cases((3, TH + 2, TW + 2)):
        if "image ends" in what:
            labels, num = chain(pa, m, c, bg, mo)[1][:2]
            assert num.tolist() == [2, 2, 2] and (labels[:, 0] == 1).all() and (labels[:, -1] == 2).all()


def test_hygiene_pass_over_every_case(pa):
    """util.connected_components on every case with the pool in hygiene mode: fresh blocks are poisoned and guarded."""
    K.hygiene_pass(pa, [case for shape in SHAPES for case in cases(shape)],
                   lambda m, c, bg, mo: pa.util.connected_components(pa.hip.asarray(m), c, bg, mo), NAMES, 200)


def test_one_plane_and_no_table(pa):
    m = R.random_classes(1, TH + 3, TW + 9, 4, 11)
    ref = R.components_ref(m, 8, 1, 40)
    got = pa.util.connected_components(pa.hip.asarray(m[0]), background=1, max_objects=40)
    assert [a.shape for a in got] == [(TH + 3, TW + 9), (1,), (1, 40, 6), (1, 40, 2)]
    same(tuple(a.get() for a in got), (ref[0][0],) + ref[1:], "(H, W)")
    # max_objects == 0: no table, and the chain takes null pointers for it
    rc, got, intact, frames = chain(pa, m, 8, 1, 0, null_tables=True)
    assert rc == OK and intact and (got[0] == ref[0]).all() and (got[1] == ref[1]).all()
    labels, num, objects, centroids = pa.util.connected_components(pa.hip.asarray(m), background=1, max_objects=0)
    assert objects.shape == (1, 0, 6) and centroids.shape == (1, 0, 2) and (labels.get() == ref[0]).all() and (num.get() == ref[1]).all()
    # an empty plane, an empty batch
    labels, num, objects, centroids = pa.util.connected_components(pa.hip.empty((2, 0, 5), np.uint8), max_objects=3)
    assert labels.shape == (2, 0, 5) and num.get().tolist() == [0, 0] and not objects.get().any() and not centroids.get().view(np.uint32).any()
    assert pa.util.connected_components(pa.hip.empty((0, 4, 5), np.uint8))[1].shape == (0,)


def test_refusals_leave_the_outputs_untouched(pa):
    ctx = pa.hip.context()
    lib = pa._lib.load()
    m = pa.hip.asarray(R.random_binary(2, 9, 11, 0.5, 1))
    frames = [Framed(pa, 2 * 9 * 11), Framed(pa, 2), Framed(pa, 2 * 4 * 6), Framed(pa, 2 * 4 * 2)]
    scratch = Framed(pa, scratch_bytes(2, 9, 11, 4) // 4 + 2)
    ok = dict(m=m.ptr, N=2, H=9, W=11, connectivity=8, background=0, max_objects=4, scratch=scratch.ptr, labels=frames[0].ptr,
              num=frames[1].ptr, objects=frames[2].ptr, centroids=frames[3].ptr)
    bad = [(dict(m=None), EINVAL), (dict(scratch=None), EINVAL), (dict(labels=None), EINVAL), (dict(num=None), EINVAL),
           (dict(objects=None), EINVAL), (dict(centroids=None), EINVAL), (dict(N=-1), EINVAL), (dict(H=-1), EINVAL), (dict(W=-2), EINVAL),
           (dict(max_objects=-1), EINVAL), (dict(connectivity=6), EINVAL), (dict(connectivity=0), EINVAL), (dict(background=-2), EINVAL),
           (dict(background=256), EINVAL), (dict(H=46341, W=46341), EUNSUPPORTED), (dict(N=1 << 11, H=1 << 10, W=1 << 10), EUNSUPPORTED),
           (dict(max_objects=MAX_OBJECTS + 1), EUNSUPPORTED)]
    for change, code in bad:
        args = dict(ok, **change)
        assert lib.pl_components_u8_i32(ctx.handle, *args.values()) == code, change
        assert lib.pl_last_error(), change
    assert lib.pl_components_u8_i32(None, *ok.values()) == EINVAL
    for change in (dict(N=0), dict(H=0), dict(W=0)):                         # nothing to do: PL_OK without a launch
        assert lib.pl_components_u8_i32(ctx.handle, *dict(ok, **change).values()) == OK, change
    ctx.synchronize()
    assert all(f.untouched() for f in frames) and scratch.untouched()
    assert lib.pl_components_u8_i32(ctx.handle, *ok.values()) == OK          # ... and the arguments they were derived from run
    assert not frames[1].untouched()


def test_chain_replays_from_a_captured_graph(pa):
    """No host wait and no host-computed value: the chain captured once answers for whatever map is in its input at launch."""
    n, h, w, mo = 2, TH + 5, 2 * TW + 3, 20
    maps = [R.random_classes(n, h, w, 3, 21), R.serpentine(n, h, w), R.random_binary(n, h, w, 0.55, 22)]
    m = pa.hip.empty((n, h, w), np.uint8)
    labels, num = pa.hip.empty((n, h, w), I32), pa.hip.empty((n,), I32)
    objects, centroids = pa.hip.empty((n, mo, 6), I32), pa.hip.empty((n, mo, 2), F32)
    scratch = pa.hip.empty(((scratch_bytes(n, h, w, mo) + 7) // 8,), np.int64)
    K.replay_from_captured_graph(
        pa, lambda: pa._lib.load().pl_components_u8_i32(pa.hip.context().handle, m.ptr, n, h, w, 4, 0, mo, scratch.ptr, labels.ptr, num.ptr,
                                                        objects.ptr, centroids.ptr),
        m, (labels, num, objects, centroids), maps, lambda host: R.components_ref(host, 4, 0, mo), NAMES)


def test_large_maps_with_known_answers(pa):
    """More root counts per image than one step of the scan's workgroup takes; answers by construction."""
    h, w = 1449, 1501
    assert (h * w + BLOCK - 1) // BLOCK > SCAN_STEP
    for name, (m, labels, num) in (("lattice", R.lattice(h, w)), ("stripes", R.stripes(h, w)), ("serpentine", R.serpentine_answer(h, w))):
        want = (labels, num) + R.regions_ref(m, labels, 300)
        for c in (4, 8):
            got = tuple(a.get() for a in pa.util.connected_components(pa.hip.asarray(m), c, 0, 300))
            same(got, want, "%s, %d-connected" % (name, c))
    assert want[1][0] == 1 and want[2][0, 0].tolist() == [1, (h + 1) // 2 * w + h // 2, 0, 0, h, w]


# ---- nets -------------------------------------------------------------------------------------------------------------------
SPEC = dict(connectivity=4, background=1, max_objects=40)


def _want(scores):
    m = np.argmax(scores, 1).astype(np.uint8)
    ref = R.components_ref(m, **SPEC)
    assert 3 <= ref[1].min() and ref[2][:, :, 1].max() > 8, ref[1]              # several objects, some of them large
    return ref


@pytest.mark.parametrize("streams", [None, "pipe2"])
def test_tiny_net_every_call_form(pa, streams):
    K.check_every_call_form(pa, streams, lambda net, **at: net.object_output(**at, **SPEC), _want, NAMES)


def test_one_output_net_and_uint8_input(pa):
    K.check_one_output_net_and_uint8_input(pa, lambda net: net.object_output(**SPEC), _want, NAMES,
                                           [(2, 32, 32), (2,), (2, 40, 6), (2, 40, 2)], pa.util.ObjectSpec(**SPEC))


def test_fpn_at_64(pa):
    from planer_amd.irgen import fpn
    g, b = fpn.build()
    x = fpn.make_input(2, size=64)
    net = pa.from_graph(g, b)
    scores = net(x)                                                          # the same instance, so the same plan and the same scores
    assert scores.shape == (2, 21, 64, 64)
    before = dict(net._plans)
    net.object_output(max_objects=64)
    got = net(x)
    assert all(net._plans[key] is before[key] for key in before)
    ref = R.components_ref(np.argmax(scores, 1).astype(np.uint8), 8, 0, 64)
    same(got, ref, "fpn")
    same(net.submit(x).get(), ref, "fpn, submit")
    print("fpn at 64: %s objects" % ref[1].tolist())
    pa.hip.trim_side_contexts()


# ---- Net.tiled --------------------------------------------------------------------------------------------------------------
def test_net_tiled_objects_of_the_scan(pa):
    from tests import tile_net_ref as T
    case = T.CASES["a"]
    geo = T.Geometry(*case["size"], **case["tile"])
    g, b, _ = T.exact_net(3, 3, case["k"])
    net = pa.from_graph(g, b)
    net.image_input(np.ones(3, F32), np.zeros(3, F32))
    img = np.random.default_rng(41).integers(0, 256, (5, 6, 3), dtype=np.uint8)
    img = np.ascontiguousarray(np.repeat(np.repeat(img, 8, 0), 8, 1)[:case["size"][0], :case["size"][1]])
    net.label_output()
    m = net.tiled(img, **case["tile"])
    assert m.dtype == np.uint8 and m.shape == case["size"]
    net.object_output(connectivity=4, background=-1, max_objects=50)
    ref = R.components_ref(m[None], 4, -1, 50)
    want = (ref[0][0],) + ref[1:]
    got = net.tiled(img, **case["tile"])
    assert isinstance(got, tuple) and all(isinstance(a, np.ndarray) for a in got)
    same(got, want, "tiled, host")
    dev = net.tiled(pa.hip.asarray(img), batch=5, **case["tile"])
    assert all(isinstance(a, pa.hip.DeviceArray) for a in dev)
    same(K.host(dev), want, "tiled, device")
    # at least one object lies on both sides of a line where a window begins
    starts = [s.start for s in geo.rows if s.start]
    boxes = ref[2][0][:min(int(ref[1][0]), 50)]
    assert len(geo.windows) > 1 and any(y0 < s < y1 for s in starts for _, _, y0, _, y1, _ in boxes.tolist())
    with pytest.raises(NotImplementedError, match="different product"):      # resampled working sizes: refused as for labels
        net.tiled(img, window=16, sample=(50, 61))
    pa.hip.trim_side_contexts()

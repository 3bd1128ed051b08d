"""Instances as net output on a real MI355X (pl_flow_instances_f32, util.follow_flows, util.FlowSpec, Net.flow_output, Net.tiled;
DESIGN 4.28).

Everything is exact: masks, num, instances and centres equal tests/flow_ref.py's, which tests/test_flow_ref.py holds to a
per-pixel statement of the rule.  The kernel chain writes into outputs framed by sentinel words that must survive, from a scratch
block filled with a poison pattern; one pass over the whole case list runs with the pool in hygiene mode, where scratch read
before it is written shows up as a wrong answer and a write past a block as a dirty guard.  Shapes come from the tile extent the
header states (the table pass takes the components tile; the chain adds no tile extent of its own).  Then nets: every call form
against the mirror applied to what a second, undeclared instance returns."""
import functools

import numpy as np
import pytest

from tests import flow_ref as R
from tests import head_kit as K
from tests import image_input_ref as RI
from tests.head_kit import EINVAL, EUNSUPPORTED, F32, I32, OK, Framed

pytestmark = pytest.mark.gpu

NAMES = ("masks", "num", "instances", "centres")

_C = K.header_constants("PL_(?:CC|FLOW)_")
TH, TW, BLOCK = _C["PL_CC_TILE_H"], _C["PL_CC_TILE_W"], _C["PL_CC_BLOCK"]
SCAN_STEP, MAX_ROUNDS, MAX_INSTANCES = _C["PL_FLOW_SCAN_STEP"], _C["PL_FLOW_MAX_ROUNDS"], _C["PL_FLOW_MAX_INSTANCES"]

SHAPES = [(1, 1, 1), (2, 5, 7), (1, TH, TW), (1, TH - 1, TW - 1), (2, TH + 1, TW + 1), (1, 2 * TH + 3, 3 * TW + 5), (1, 1, 4 * TW + 1),
          (1, 4 * TH + 1, 1)]
DEFAULT = dict(level=0.0, min_flow=0.0, rounds=10, min_size=15, max_instances=256, planes=(0, 1, 2))


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def scratch_bytes(n, h, w, m):
    """PL_FLOW_SCRATCH_BYTES"""
    def align(b):
        return (b + 15) // 16 * 16
    cc = n * h * w * 4 + n * ((h * w + BLOCK - 1) // BLOCK) * 4
    return 16 + n * m * 16 + 4 * align(n * h * w * 4) + align(n * ((h + 1) // 2) * ((w + 1) // 2) * 4) + align(n * 4) + align(n * h * w) + cc


def _kw(**change):
    return dict(DEFAULT, **change)


@functools.lru_cache(maxsize=None)
def cases(shape):
    """[(name, x (N, C, H, W), arguments, the mirror's four arrays)] for one shape: computed once, shared, read-only."""
    n, h, w = shape
    seed = h * 1000 + w
    small = _kw(min_size=0, max_instances=40)
    discs, noisy = R.discs(n, h, w)[0], R.discs(n, h, w, seed, 0.7)[0]
    vol = int(R.flow_ref(discs, **small)[2][0, 0, 0])                        # the first disc's pixel count (0: no disc fits)
    spare = np.concatenate([R.random_flows(n, h, w, seed + 7)[:, :2], R.discs(n, h, w, seed, 0.4)[0]], 1)     # five planes
    items = [("random", R.random_flows(n, h, w, seed), small), ("random, defaults", R.random_flows(n, h, w, seed + 1), _kw()),
             ("random, level and min_flow", R.random_flows(n, h, w, seed + 2), _kw(level=0.5, min_flow=1.25, min_size=2, rounds=5)),
             ("discs", discs, _kw()), ("noisy discs", noisy, _kw(min_size=3)),
             ("all background", R.all_background(n, h, w), _kw()), ("all foreground, still", R.all_foreground_still(n, h, w), _kw()),
             ("lattice", R.lattice(n, h, w), _kw(min_size=1, max_instances=7)), ("outward", R.outward(n, h, w), small),
             ("into background", R.into_background(n, h, w), small),
             ("2-cycles", R.two_cycles(n, h, w, 0), _kw(rounds=0, min_size=0)), ("2-cycles across seams", R.two_cycles(n, h, w, 1), small),
             ("vortices", R.vortices(n, h, w, 0), _kw(rounds=1, min_size=0)), ("vortices across seams", R.vortices(n, h, w, 1), small),
             ("vortices across seams, one step", R.vortices(n, h, w, 1), _kw(rounds=0, min_size=0)),
             ("specials", R.specials(n, h, w, seed + 3), small), ("specials, min_flow", R.specials(n, h, w, seed + 4), _kw(min_flow=0.5, min_size=2)),
             ("direction edges", R.direction_edges(n, h, w, seed + 5), _kw(rounds=1, min_size=0)),
             ("length edges", R.length_edges(n, h, w), _kw(min_flow=R.MIN_FLOW_EDGE, rounds=1, min_size=0)),
             ("min_size at vol", discs, _kw(min_size=vol)), ("min_size above vol", discs, _kw(min_size=vol + 1)),
             ("min_size 0", noisy, _kw(min_size=0)), ("no table", noisy, _kw(min_size=2, max_instances=0)),
             ("fewer rows than instances", noisy, _kw(min_size=0, max_instances=2)),
             ("other planes", spare, _kw(planes=(4, 1, 3), min_size=2))]
    items += [("serpentine, rounds %d" % r, R.serpentine(n, h, w)[0], _kw(rounds=r, min_size=0, max_instances=8)) for r in (0, 1, 3)]
    out = []
    for name, x, kw in items:
        ref = R.flow_ref(x, **kw)
        for a in (x,) + ref:
            a.setflags(write=False)
        out.append(("%s %s" % (shape, name), x, kw, ref))
    return out


def chain(pa, x, kw, hwc=False, null_tables=False):
    """pl_flow_instances_f32 through the C interface on framed outputs and a poisoned scratch block; hwc: the same data as
    (N, H, W, C), read through pixel_stride = C.  -> (status, (masks, num, instances, centres), every frame intact)."""
    ctx = pa.hip.context()
    n, c, h, w = x.shape
    m = kw["max_instances"]
    if hwc:
        dev, strides = pa.hip.asarray(np.ascontiguousarray(x.transpose(0, 2, 3, 1))), (h * w * c, c) + tuple(kw["planes"])
    else:
        dev, strides = pa.hip.asarray(np.ascontiguousarray(x)), (c * h * w, 1) + tuple(p * h * w for p in kw["planes"])
    frames = [Framed(pa, n * h * w), Framed(pa, n), Framed(pa, n * m * 5), Framed(pa, n * m * 2)]
    scratch = Framed(pa, scratch_bytes(n, h, w, m) // 4 + 2)
    args = [f.ptr for f in frames]
    if null_tables:
        args[2] = args[3] = None
    rc = pa._lib.load().pl_flow_instances_f32(ctx.handle, dev.ptr, n, h, w, *strides, kw["level"], kw["min_flow"], kw["rounds"],
                                              kw["min_size"], m, scratch.ptr, *args)
    got, intact = [], scratch.get(np.uint32, (-1,))[1]
    for f, dt, shape in zip(frames, (I32, I32, I32, F32), ((n, h, w), (n,), (n, m, 5), (n, m, 2))):
        a, ok = f.get(dt, shape)
        got.append(a)
        intact = intact and ok
    return rc, tuple(got), intact


def same(got, want, what):
    K.same(got, want, NAMES, what)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_chain_equals_the_mirror(pa, shape):
    for what, x, kw, ref in cases(shape):
        null = kw["max_instances"] == 0
        rc, got, intact = chain(pa, x, kw, null_tables=null)
        assert rc == OK and intact, what
        same(got, ref, what)
        if "random" in what or "noisy" in what or "specials" in what:        # the same data through the HWC strides; and two runs
            rc, again, intact = chain(pa, x, kw, hwc=True, null_tables=null)     # of one input give identical bytes
            assert rc == OK and intact, what
            same(again, ref, what + ", hwc")
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, chain(pa, x, kw, null_tables=null)[1])), what


def test_the_patterns_are_what_they_claim(pa):
    """The properties the case list is there for, asserted on the device's own answers."""
    shape = (1, 2 * TH + 3, 3 * TW + 5)
    n, h, w = shape
    by_name = {what: (x, kw, ref) for what, x, kw, ref in cases(shape)}

    def run(name):
        x, kw, ref = by_name["%s %s" % (shape, name)]
        rc, got, intact = chain(pa, x, kw, null_tables=kw["max_instances"] == 0)
        assert rc == OK and intact
        same(got, ref, name)
        return got

    masks, num, instances, _ = run("lattice")
    assert num[0] == ((h + 1) // 2) * ((w + 1) // 2) > 7                      # the volume table's bound, and more than the rows
    assert masks.max() == num[0] and (instances[0, :, 0] == 1).all() and instances[0, :, 2].tolist() == [0, 2, 4, 6, 8, 10, 12]
    assert run("all background")[1][0] == 0 and not run("all background")[0].any()
    assert run("all foreground, still")[2][0, 0].tolist() == [h * w, 0, 0, h, w]
    assert run("outward")[1][0] == 4                                          # the four corners, through the clamp
    masks = run("into background")[0]
    assert (masks[0, :, 2::3] == 0).all() and (masks[0, :, 0::3] > 0).all()
    count = R.discs(n, h, w)[1]
    assert run("discs")[1][0] == count == run("min_size at vol")[1][0] and run("min_size above vol")[1][0] == 0
    assert count == (h // 12) * (w // 12)
    length = R.serpentine(n, h, w)[1]
    assert length > 2 ** 3
    sinks = [int((run("serpentine, rounds %d" % r)[0] > 0).sum()) for r in (0, 1, 3)]
    assert sinks == [length] * 3                                              # one path, one instance, whatever the rounds
    a, b = run("vortices across seams, one step"), run("vortices across seams")
    assert a[1][0] == b[1][0] == 1 and (a[0] == b[0]).all()
    x, kw, _ = by_name["%s length edges" % (shape,)]
    nxt = R.step_ref(x[0, 0], x[0, 1], x[0, 2], 0.0, R.MIN_FLOW_EDGE)[0].reshape(h, w) - np.arange(h * w).reshape(h, w)
    assert nxt[0, :10].tolist() == [0, 0, 1, 1, 0] * 2                        # exactly g2 and the tie stay, one ulp above moves
    assert run("no table")[1][0] > 2 and run("fewer rows than instances")[1][0] > 2


def test_hygiene_pass_over_every_case(pa):
    """util.follow_flows on every case with the pool in hygiene mode: fresh blocks are poisoned and guarded."""
    K.hygiene_pass(pa, [case for shape in SHAPES for case in cases(shape)],
                   lambda x, kw: pa.util.follow_flows(pa.hip.asarray(np.ascontiguousarray(x)), **kw), NAMES, 200)


def test_one_image_and_empty_inputs(pa):
    x = R.discs(1, TH + 3, TW + 9, 2, 0.5)[0]
    ref = R.flow_ref(x, **_kw(max_instances=40))
    got = pa.util.follow_flows(pa.hip.asarray(x[0]), max_instances=40)
    assert [a.shape for a in got] == [(TH + 3, TW + 9), (1,), (1, 40, 5), (1, 40, 2)]
    same(tuple(a.get() for a in got), (ref[0][0],) + ref[1:], "(C, H, W)")
    masks, num, instances, centres = pa.util.follow_flows(pa.hip.asarray(x), max_instances=0)
    assert instances.shape == (1, 0, 5) and centres.shape == (1, 0, 2) and (masks.get() == ref[0]).all() and (num.get() == ref[1]).all()
    # an empty plane, an empty batch
    masks, num, instances, centres = pa.util.follow_flows(pa.hip.empty((2, 3, 0, 5), F32), max_instances=3)
    assert masks.shape == (2, 0, 5) and num.get().tolist() == [0, 0] and not instances.get().any() and not centres.get().view(np.uint32).any()
    assert pa.util.follow_flows(pa.hip.empty((0, 3, 4, 5), F32))[1].shape == (0,)


def test_refusals_leave_the_outputs_untouched(pa):
    ctx = pa.hip.context()
    lib = pa._lib.load()
    x = pa.hip.asarray(R.random_flows(2, 9, 11, 1))
    frames = [Framed(pa, 2 * 9 * 11), Framed(pa, 2), Framed(pa, 2 * 4 * 5), Framed(pa, 2 * 4 * 2)]
    scratch = Framed(pa, scratch_bytes(2, 9, 11, 4) // 4 + 2)
    ok = dict(x=x.ptr, N=2, H=9, W=11, image_stride=297, pixel_stride=1, off_dy=0, off_dx=99, off_prob=198, level=0.0, min_flow=0.0,
              rounds=4, min_size=2, max_instances=4, scratch=scratch.ptr, masks=frames[0].ptr, num=frames[1].ptr, instances=frames[2].ptr,
              centres=frames[3].ptr)
    bad = [(dict(x=None), EINVAL), (dict(scratch=None), EINVAL), (dict(masks=None), EINVAL), (dict(num=None), EINVAL),
           (dict(instances=None), EINVAL), (dict(centres=None), EINVAL), (dict(N=-1), EINVAL), (dict(H=-1), EINVAL), (dict(W=-2), EINVAL),
           (dict(max_instances=-1), EINVAL), (dict(rounds=-1), EINVAL), (dict(min_size=-1), EINVAL), (dict(image_stride=0), EINVAL),
           (dict(pixel_stride=0), EINVAL), (dict(pixel_stride=-1), EINVAL), (dict(H=46341, W=46341), EUNSUPPORTED),
           (dict(N=1 << 11, H=1 << 10, W=1 << 10), EUNSUPPORTED), (dict(rounds=MAX_ROUNDS + 1), EUNSUPPORTED),
           (dict(max_instances=MAX_INSTANCES + 1), EUNSUPPORTED)]
    for change, code in bad:
        args = dict(ok, **change)
        assert lib.pl_flow_instances_f32(ctx.handle, *args.values()) == code, change
        assert lib.pl_last_error(), change
    assert lib.pl_flow_instances_f32(None, *ok.values()) == EINVAL
    for change in (dict(N=0), dict(H=0), dict(W=0)):                         # nothing to do: PL_OK without a launch
        assert lib.pl_flow_instances_f32(ctx.handle, *dict(ok, **change).values()) == OK, change
    ctx.synchronize()
    assert all(f.untouched() for f in frames) and scratch.untouched()
    assert lib.pl_flow_instances_f32(ctx.handle, *ok.values()) == OK         # ... and the arguments they were derived from run
    assert not frames[1].untouched()


def test_chain_replays_from_a_captured_graph(pa):
    """No host wait and no host-computed value: the chain captured once answers for whatever planes are in its input at launch."""
    n, h, w, m = 2, TH + 5, 2 * TW + 3, 20
    kw = _kw(rounds=3, min_size=2, max_instances=m)
    inputs = [R.random_flows(n, h, w, 21), R.serpentine(n, h, w)[0], R.discs(n, h, w, 22, 0.6)[0], R.vortices(n, h, w, 1)]
    x = pa.hip.empty((n, 3, h, w), F32)
    masks, num = pa.hip.empty((n, h, w), I32), pa.hip.empty((n,), I32)
    instances, centres = pa.hip.empty((n, m, 5), I32), pa.hip.empty((n, m, 2), F32)
    scratch = pa.hip.empty(((scratch_bytes(n, h, w, m) + 7) // 8,), np.int64)
    K.replay_from_captured_graph(
        pa, lambda: pa._lib.load().pl_flow_instances_f32(pa.hip.context().handle, x.ptr, n, h, w, 3 * h * w, 1, 0, h * w, 2 * h * w, kw["level"],
                                                         kw["min_flow"], kw["rounds"], kw["min_size"], m, scratch.ptr, masks.ptr, num.ptr,
                                                         instances.ptr, centres.ptr),
        x, (masks, num, instances, centres), inputs, lambda host: R.flow_ref(host, **kw), NAMES)


def test_a_large_map_with_a_known_answer(pa):
    """A grid of discs on 1024 x 1536: more raw instances than one step of the renumbering workgroup takes; the count and every
    area come from the construction."""
    h, w = 1024, 1536
    x, count, area = R.disc_grid(h, w)
    assert count == 64 * 96 > SCAN_STEP
    masks, num, instances, centres = (a.get() for a in pa.util.follow_flows(pa.hip.asarray(x), max_instances=count))
    assert num[0] == count and (instances[0, :, 0] == area).all()
    assert (np.bincount(masks.ravel(), minlength=count + 1)[1:] == area).all() and ((masks[0] > 0) == (x[0, 2] > 0)).all()
    j = np.arange(count)                                                     # numbered in raster order of the discs' first pixels
    cy, cx = (j // 96) * 16 + 8, (j % 96) * 16 + 8
    assert (centres[0, :, 0] == cy).all() and (centres[0, :, 1] == cx).all()
    assert (instances[0, :, 1] == cy - 6).all() and (instances[0, :, 4] == cx + 7).all()
    assert (masks[0, cy, cx] == j + 1).all()
    # one more than the discs: the last row is unused
    _, num, instances, centres = (a.get() for a in pa.util.follow_flows(pa.hip.asarray(x), min_size=area, max_instances=count + 1))
    assert num[0] == count and not instances[0, count].any() and not centres[0, count].view(np.uint32).any()
    assert pa.util.follow_flows(pa.hip.asarray(x), min_size=area + 1)[1].get()[0] == 0


# ---- nets -------------------------------------------------------------------------------------------------------------------
SPEC = dict(level=0.0, min_flow=0.5, rounds=6, min_size=2, max_instances=40)


def _want(planes):
    ref = R.flow_ref(planes, **SPEC)
    assert ref[1].min() >= 1, ref[1]                                         # something to find in every image
    return ref


@pytest.mark.parametrize("streams", [None, "pipe2"])
def test_tiny_net_every_call_form(pa, streams):
    K.check_every_call_form(pa, streams, lambda net, **at: net.flow_output(**at, **SPEC), _want, NAMES)


def test_one_output_net_and_uint8_input(pa):
    K.check_one_output_net_and_uint8_input(pa, lambda net: net.flow_output(**SPEC), _want, NAMES,
                                           [(2, 32, 32), (2,), (2, 40, 5), (2, 40, 2)], pa.util.FlowSpec(**SPEC))


def test_cellnet_at_64(pa):
    from planer_amd.irgen import cellnet
    g, b = cellnet.build()
    x = cellnet.make_input(2, size=64)
    net = pa.from_graph(g, b)
    planes = net(x)                                                          # the same instance, so the same plan and the same planes
    assert planes.shape == (2, 3, 64, 64)
    before = dict(net._plans)
    kw = dict(min_size=4, max_instances=64, planes=cellnet.PLANES)
    net.flow_output(**kw)
    got = net(x)
    assert all(net._plans[key] is before[key] for key in before)
    ref = R.flow_ref(planes, **kw)
    same(got, ref, "cellnet")
    same(net.submit(x).get(), ref, "cellnet, submit")
    print("cellnet at 64: %s instances" % ref[1].tolist())
    pa.hip.trim_side_contexts()


# ---- Net.tiled --------------------------------------------------------------------------------------------------------------
def test_net_tiled_instances_of_the_scan(pa):
    from tests import tile_net_ref as T
    case = T.CASES["a"]
    geo = T.Geometry(*case["size"], **case["tile"])
    g, b, _ = T.exact_net(3, 3, case["k"])
    net = pa.from_graph(g, b)
    net.image_input(np.ones(3, F32), np.zeros(3, F32))
    img = np.random.default_rng(41).integers(0, 256, (5, 6, 3), dtype=np.uint8)
    img = np.ascontiguousarray(np.repeat(np.repeat(img, 8, 0), 8, 1)[:case["size"][0], :case["size"][1]])
    blend = net.tiled(img, **case["tile"])                                   # the float blend of the same net: (OH, OW, 3)
    assert blend.dtype == F32 and blend.shape == case["size"] + (3,) and len(geo.windows) > 1
    kw = dict(level=0.0, min_flow=0.25, rounds=5, min_size=2, max_instances=50, planes=(1, 2, 0))
    net.flow_output(**kw)
    ref = R.flow_ref(np.ascontiguousarray(blend.transpose(2, 0, 1))[None], **kw)
    want = (ref[0][0],) + ref[1:]
    got = net.tiled(img, **case["tile"])
    assert isinstance(got, tuple) and all(isinstance(a, np.ndarray) for a in got)
    same(got, want, "tiled, host")
    dev = net.tiled(pa.hip.asarray(img), batch=5, **case["tile"])
    assert all(isinstance(a, pa.hip.DeviceArray) for a in dev)
    same(K.host(dev), want, "tiled, device")
    assert ref[1][0] >= 1
    with pytest.raises(NotImplementedError, match="different product"):      # resampled working sizes: refused as for labels
        net.tiled(img, window=16, sample=(50, 61))
    net.float_output()
    assert RI.same_bits(net.tiled(img, **case["tile"]), blend)
    pa.hip.trim_side_contexts()

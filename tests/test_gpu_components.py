"""Objects as net output on a real MI355X (pl_components_u8_i32, util.connected_components, util.ObjectSpec,
Net.object_output, Net.tiled).

Everything is exact: labels, num, objects and centroids equal tests/components_ref.py's, which tests/test_components_ref.py holds
to scipy.ndimage.  The kernel chain writes into outputs framed by sentinel words that must survive, from a scratch block filled
with a poison pattern; one pass over the whole case list runs with the pool in hygiene mode, where scratch read before it is
written shows up as a wrong answer and a write past a block as a dirty guard.  Shapes come from the tile extent the header
states.  Then nets: every call form against the reference applied to the argmax of what a second, undeclared instance returns."""
import functools
import os
import re

import numpy as np
import pytest

from tests import components_ref as R
from tests import image_input_ref as RI
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

F32, I32 = np.float32, np.int32
PAD = 16                                    # sentinel words on either side of an output
SENT = np.uint32(0xA5A5A5A5)
OK, EINVAL, EUNSUPPORTED = 0, 1, 2

_H = open(os.path.join(ROOT, "include", "planer_hip.h")).read()
_C = {k: int(v) for k, v in re.findall(r"#define (PL_CC_[A-Z_]+) (\d+)", _H)}
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


class Framed:
    """`words` 32-bit words on the device between two runs of PAD sentinel words, all of it the sentinel to begin with."""

    def __init__(self, pa, words):
        self.words = words
        self.buf = pa.hip.empty((PAD + words + PAD,), np.uint32)
        self.buf.set(np.full(self.buf.shape, SENT, np.uint32))
        self.ptr = self.buf.ptr + 4 * PAD

    def get(self, dtype, shape):
        """(the words as `dtype`, whether both sentinel runs are intact)"""
        raw = self.buf.get()
        intact = bool((raw[:PAD] == SENT).all() and (raw[PAD + self.words:] == SENT).all())
        return raw[PAD:PAD + self.words].view(dtype).reshape(shape), intact

    def untouched(self):
        return bool((self.buf.get() == SENT).all())


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
    for name, g, r in zip(("labels", "num", "objects", "centroids"), got, want):
        assert g.shape == r.shape and g.dtype == r.dtype, (what, name, g.shape, r.shape, g.dtype, r.dtype)
        bad = np.flatnonzero((g.view(np.uint32) if g.dtype == F32 else g).ravel() != (r.view(np.uint32) if r.dtype == F32 else r).ravel())
        assert bad.size == 0, "%s: %s differs at %d places, first flat index %d: got %r, want %r" % (
            what, name, bad.size, bad[0], g.ravel()[bad[0]], r.ravel()[bad[0]])


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
    ctx = pa.hip.context()
    ctx.synchronize()
    ctx.pool_debug(pa.hip.POOL_GUARD_BYTES, 0xFF)
    try:
        got = [tuple(a.get() for a in pa.util.connected_components(pa.hip.asarray(m), c, bg, mo))
               for shape in SHAPES for _, m, c, bg, mo, _ in cases(shape)]
        dirty, report = ctx.pool_debug_check()
    finally:
        ctx.pool_debug(0)
    assert dirty == 0, report
    want = [(what, ref) for shape in SHAPES for what, _, _, _, _, ref in cases(shape)]
    assert len(got) == len(want) > 200
    for g, (what, ref) in zip(got, want):
        same(g, ref, what)


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
    from planer_amd import _lib
    ctx = pa.hip.context()
    n, h, w, mo = 2, TH + 5, 2 * TW + 3, 20
    maps = [R.random_classes(n, h, w, 3, 21), R.serpentine(n, h, w), R.random_binary(n, h, w, 0.55, 22)]
    m = pa.hip.empty((n, h, w), np.uint8)
    labels, num = pa.hip.empty((n, h, w), I32), pa.hip.empty((n,), I32)
    objects, centroids = pa.hip.empty((n, mo, 6), I32), pa.hip.empty((n, mo, 2), F32)
    scratch = pa.hip.empty(((scratch_bytes(n, h, w, mo) + 7) // 8,), np.int64)
    ctx.synchronize()
    _lib.call("pl_capture_begin", ctx.handle)
    graph = _lib.c_void_p()
    try:
        rc = _lib.load().pl_components_u8_i32(ctx.handle, m.ptr, n, h, w, 4, 0, mo, scratch.ptr, labels.ptr, num.ptr, objects.ptr, centroids.ptr)
    finally:
        end = _lib.load().pl_capture_end(ctx.handle, _lib.byref(graph))
    assert rc == OK
    _lib.check(end)
    try:
        for i, host in enumerate(maps):
            m.set(host)
            _lib.call("pl_graph_launch", graph)
            same(tuple(a.get() for a in (labels, num, objects, centroids)), R.components_ref(host, 4, 0, mo), "replay %d" % i)
    finally:
        _lib.check(_lib.load().pl_graph_destroy(graph))


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


def tiny_net(outputs, seed=4):
    """x (N, 3, 32, 32) -> conv 3x3 (8) + relu = f -> conv 3x3 (3) = s, the scores.  Small-integer filters and biases: with integer
    inputs every partial sum is an exact float32, so two instances agree bit for bit whichever kernels they pick (the trick of
    tests/test_gpu_conv_exact.py), and equal scores are common: the argmax takes the first."""
    from planer_amd.irgen.builder import GraphBuilder
    rng = np.random.default_rng(seed)
    g = GraphBuilder(["x"])
    g.init("K0", rng.integers(-2, 3, (8, 3, 3, 3)).astype(F32))
    g.init("B0", rng.integers(-3, 4, 8).astype(F32))
    g.op("conv", ["x", "K0", "B0"], "c0", name="conv0", group=1, strides=[1, 1], dilations=[1, 1], pads=[1, 1, 1, 1])
    g.op("relu", "c0", "f", name="relu0")
    g.init("K1", rng.integers(-2, 3, (3, 8, 3, 3)).astype(F32))
    g.init("B1", rng.integers(-3, 4, 3).astype(F32))
    g.op("conv", ["f", "K1", "B1"], "s", name="conv1", group=1, strides=[1, 1], dilations=[1, 1], pads=[1, 1, 1, 1])
    return g.finish(outputs)


def tiny_input(seed=7):
    """Integers, and smooth enough that the argmax has objects of more than a few pixels."""
    x = np.random.default_rng(seed).integers(-3, 4, (2, 3, 8, 8)).astype(F32)
    return np.ascontiguousarray(np.repeat(np.repeat(x, 4, 2), 4, 3))


def _host(y):
    return tuple(v.get() if hasattr(v, "get") else v for v in y)


def _want(scores):
    m = np.argmax(scores, 1).astype(np.uint8)
    ref = R.components_ref(m, **SPEC)
    assert 3 <= ref[1].min() and ref[2][:, :, 1].max() > 8, ref[1]              # several objects, some of them large
    return ref


@pytest.mark.parametrize("streams", [None, "pipe2"])
def test_tiny_net_every_call_form(pa, streams):
    g, b = tiny_net(["f", "s"])
    x = tiny_input()
    net, plain = pa.from_graph(g, b), pa.from_graph(g, b)
    if streams:
        net.streams = plain.streams = streams
    feat, scores = plain(x)
    assert feat.shape == (2, 8, 32, 32) and scores.shape == (2, 3, 32, 32)
    ref = _want(scores)

    def check(y, what, on_device=False):
        assert isinstance(y, tuple) and len(y) == 5, what
        assert all(isinstance(v, pa.hip.DeviceArray if on_device else np.ndarray) for v in y), what
        y = _host(y)
        assert RI.same_bits(y[0], feat), what                                # the other output: untouched
        same(y[1:], ref, what)

    base = net(x)                                                            # a plan exists before the declaration
    assert len(base) == 2 and RI.same_bits(base[1], scores)
    before = dict(net._plans)
    assert net.object_output(index=1, **SPEC) is net
    check(net(x), "host")
    check(net(pa.asarray(x)), "device", True)
    check(net({net.input[0]: x}), "dict")
    check(net.submit(x).get(), "submit")
    check(net.submit(pa.asarray(x)).result(), "submit device", True)
    pend = [net.submit(x) for _ in range(3)]                                 # several in flight
    for p in pend:
        check(p.get(), "submits in flight")
    net.compile(pa.asarray(x))
    check(net(pa.asarray(x)), "compile + replay", True)
    assert all(net._plans[key] is before[key] for key in before)             # the declaration touched no plan
    for got, want in zip(plain.submit(x).get(), (feat, scores)):            # (the plain net's throughput plan: the same scores)
        assert RI.same_bits(got, want)
    assert sorted(net._plans, key=repr) == sorted(plain._plans, key=repr)
    for how in ("debug", "eager"):                                           # the eager routes
        if how == "eager":
            net.use_graph = False
        check(net(x, debug=True) if how == "debug" else net(x), how)
    net.use_graph = True
    # float_output restores the float tensor
    assert net.float_output(1) is net
    for got, want in zip(net(x), (feat, scores)):
        assert RI.same_bits(got, want)
    for got, want in zip(net.submit(x).get(), (feat, scores)):
        assert RI.same_bits(got, want)
    # checks come before anything is launched: a tensor the label kernel does not take, a position the net does not have
    net.object_output(index=2, **SPEC)
    for call in (lambda: net(x), lambda: net(pa.asarray(x)), lambda: net.submit(x), lambda: net(x, debug=True)):
        with pytest.raises(ValueError, match="returns 2"):
            call()
    pa.hip.trim_side_contexts()


def test_one_output_net_and_uint8_input(pa):
    g, b = tiny_net(["s"])
    net, plain = pa.from_graph(g, b), pa.from_graph(g, b)
    k, bb = np.ones(3, F32), np.zeros(3, F32)                               # the bytes as they are: integers
    net.image_input(k, bb).object_output(**SPEC)
    i = np.arange(2 * 8 * 8 * 3, dtype=np.int64)
    x = ((i * 37 + i // 192 * 53 + 11) % 256).astype(np.uint8).reshape(2, 8, 8, 3)
    x = np.ascontiguousarray(np.repeat(np.repeat(x, 4, 1), 4, 2))
    ref = _want(plain(RI.decode32(x, k, bb)))
    for what, y in (("host", net(x)), ("device", net(pa.asarray(x))), ("submit", net.submit(x).get()), ("float in", net(RI.decode32(x, k, bb)))):
        assert len(y) == 4, what
        same(_host(y), ref, what)
    labels, num, objects, centroids = net(x)
    assert labels.shape == (2, 32, 32) and num.shape == (2,) and objects.shape == (2, 40, 6) and centroids.shape == (2, 40, 2)
    # util.ObjectSpec on its own, on the float scores
    scores = plain(RI.decode32(x, k, bb))
    same(_host(pa.util.ObjectSpec(**SPEC).encode(pa.asarray(scores))), ref, "ObjectSpec.encode")
    pa.hip.trim_side_contexts()


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
    same(_host(dev), want, "tiled, device")
    # at least one object lies on both sides of a line where a window begins
    starts = [s.start for s in geo.rows if s.start]
    boxes = ref[2][0][:min(int(ref[1][0]), 50)]
    assert len(geo.windows) > 1 and any(y0 < s < y1 for s in starts for _, _, y0, _, y1, _ in boxes.tolist())
    with pytest.raises(NotImplementedError, match="different product"):      # resampled working sizes: refused as for labels
        net.tiled(img, window=16, sample=(50, 61))
    pa.hip.trim_side_contexts()

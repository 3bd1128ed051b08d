"""What the GPU tests of the output heads share (test_gpu_components.py, test_gpu_peaks.py, test_gpu_flow.py and, for `Framed`
and `host`, test_gpu_detection_output.py): framed device outputs, the bitwise compare, the constants of include/planer_hip.h, the
tiny net every head is declared on, and the checks that are the same for every head but for the declaration, the number of
arrays that come back and the mirror they are held to.  A plain module: no fixtures, and nothing here knows a head by name."""
import os
import re

import numpy as np
import pytest

from tests import image_input_ref as RI
from tests.conftest import ROOT

F32, I32 = np.float32, np.int32
PAD = 16                                    # sentinel words on either side of an output
SENT = np.uint32(0xA5A5A5A5)
OK, EINVAL, EUNSUPPORTED = 0, 1, 2


def header_constants(prefix):
    """{name: value} of the integer #defines of include/planer_hip.h whose names match the regex `prefix` and then [A-Z_]+."""
    header = open(os.path.join(ROOT, "include", "planer_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define (%s[A-Z_]+) (\d+)" % prefix, header)}


class Framed:
    """`words` 32-bit words on the device between two runs of PAD sentinel words, all of it the sentinel to begin with."""

    def __init__(self, pa, words):
        self.words = words
        self.buf = pa.hip.empty((PAD + words + PAD,), np.uint32)
        self.buf.set(np.full(self.buf.shape, SENT, np.uint32))
        self.ptr = self.buf.ptr + 4 * PAD

    def get(self, dtype=np.uint32, shape=None):
        """(the words as `dtype`, flat or of `shape`; whether both sentinel runs are intact)"""
        raw = self.buf.get()
        intact = bool((raw[:PAD] == SENT).all() and (raw[PAD + self.words:] == SENT).all())
        words = raw[PAD:PAD + self.words].view(dtype)
        return (words if shape is None else words.reshape(shape)), intact

    def untouched(self):
        """Every word, the sentinel runs included, is still the sentinel."""
        return bool((self.buf.get() == SENT).all())


def framed_call(pa, shape, dtype, off, call, pad=64):
    """call(pointer to an output of `shape` and `dtype`), the output `off` elements into a block with `pad` elements on either
    side, every byte of the block 0xA5 to begin with (test_gpu_image_output.py, test_gpu_tile_net.py: byte outputs at odd
    addresses).  -> (what call returned, the output, whether every byte around it still holds 0xA5)."""
    dtype = np.dtype(dtype)
    lo, size = (pad + off) * dtype.itemsize, int(np.prod(shape)) * dtype.itemsize
    frame = pa.hip.empty((lo + size + pad * dtype.itemsize,), np.uint8)
    frame.set(np.full(frame.shape, 0xA5, np.uint8))
    result = call(frame.ptr + lo)
    got = frame.get()
    intact = bool((got[:lo] == 0xA5).all() and (got[lo + size:] == 0xA5).all())
    return result, got[lo:lo + size].view(dtype).reshape(shape), intact


def _bits(a):
    return a.view(np.uint32) if a.dtype == F32 else a


def same(got, want, names, what):
    """The arrays `got` equal `want` in shape, dtype and every bit; `names` name them in the message."""
    for name, g, r in zip(names, got, want):
        assert g.shape == r.shape and g.dtype == r.dtype, (what, name, g.shape, r.shape, g.dtype, r.dtype)
        bad = np.flatnonzero(_bits(g).ravel() != _bits(r).ravel())
        assert bad.size == 0, "%s: %s differs at %d places, first flat index %d: got %r, want %r" % (
            what, name, bad.size, bad[0], g.ravel()[bad[0]], r.ravel()[bad[0]])


def host(y):
    return tuple(v.get() if hasattr(v, "get") else v for v in y)


def hygiene_pass(pa, cases, call, names, least):
    """call(*case[1:-1]) -> device arrays for every case (name, ..., the mirror's arrays), all of them with the pool in hygiene
    mode, where fresh blocks are poisoned and guarded: no guard is dirty and every answer is the mirror's.  More than `least`
    cases."""
    ctx = pa.hip.context()
    ctx.synchronize()
    ctx.pool_debug(pa.hip.POOL_GUARD_BYTES, 0xFF)
    try:
        got = [tuple(a.get() for a in call(*case[1:-1])) for case in cases]
        dirty, report = ctx.pool_debug_check()
    finally:
        ctx.pool_debug(0)
    assert dirty == 0, report
    assert len(got) == len(cases) > least
    for g, case in zip(got, cases):
        same(g, case[-1], names, case[0])


def replay_from_captured_graph(pa, enqueue, feed, outputs, inputs, mirror, names):
    """enqueue() -> status puts the chain on the context's stream under capture, reading the DeviceArray `feed` and writing the
    DeviceArrays `outputs`; the graph then answers mirror(host) for each of `inputs` set into `feed` before a launch."""
    from planer_amd import _lib
    ctx = pa.hip.context()
    ctx.synchronize()
    _lib.call("pl_capture_begin", ctx.handle)
    graph = _lib.c_void_p()
    try:
        rc = enqueue()
    finally:
        end = _lib.load().pl_capture_end(ctx.handle, _lib.byref(graph))
    assert rc == OK
    _lib.check(end)
    try:
        for i, x in enumerate(inputs):
            feed.set(x)
            _lib.call("pl_graph_launch", graph)
            same(tuple(a.get() for a in outputs), mirror(x), names, "replay %d" % i)
    finally:
        _lib.check(_lib.load().pl_graph_destroy(graph))


# ---- nets -------------------------------------------------------------------------------------------------------------------
def tiny_net(outputs, seed=4):
    """x (N, 3, 32, 32) -> conv 3x3 (8) + relu = f -> conv 3x3 (3) = s, what a head reads: scores, heat maps or flow planes.
    Small-integer filters and biases: with integer inputs every partial sum is an exact float32, so two instances agree bit for
    bit whichever kernels they pick (the trick of tests/test_gpu_conv_exact.py), and equal values are common: the argmax takes
    the first, and there are plateaus and ties in the order."""
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


def check_every_call_form(pa, streams, declare, mirror, names):
    """The tiny net with outputs (f, s): declare(net, index=1) puts a head on s, whose len(names) arrays then come back in s's
    place from every call route, bit for bit mirror(s) of the s a second, undeclared instance returns, and f beside them as it
    was.  declare returns the net."""
    g, b = tiny_net(["f", "s"])
    x = tiny_input()
    net, plain = pa.from_graph(g, b), pa.from_graph(g, b)
    if streams:
        net.streams = plain.streams = streams
    feat, s = plain(x)
    assert feat.shape == (2, 8, 32, 32) and s.shape == (2, 3, 32, 32)
    ref = mirror(s)

    def check(y, what, on_device=False):
        assert isinstance(y, tuple) and len(y) == 1 + len(names), what
        assert all(isinstance(v, pa.hip.DeviceArray if on_device else np.ndarray) for v in y), what
        y = host(y)
        assert RI.same_bits(y[0], feat), what                                # the other output: untouched
        same(y[1:], ref, names, what)

    base = net(x)                                                            # a plan exists before the declaration
    assert len(base) == 2 and RI.same_bits(base[1], s)
    before = dict(net._plans)
    assert declare(net, index=1) is net
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
    check(net(pa.asarray(x)), "replay again", True)
    assert all(net._plans[key] is before[key] for key in before)             # the declaration touched no plan
    for got, want in zip(plain.submit(x).get(), (feat, s)):                  # (the plain net's throughput plan: the same s)
        assert RI.same_bits(got, want)
    assert sorted(net._plans, key=repr) == sorted(plain._plans, key=repr)
    for how in ("debug", "eager"):                                           # the eager routes
        if how == "eager":
            net.use_graph = False
        check(net(x, debug=True) if how == "debug" else net(x), how)
    net.use_graph = True
    # float_output restores the float tensor
    assert net.float_output(1) is net
    for got, want in zip(net(x), (feat, s)):
        assert RI.same_bits(got, want)
    for got, want in zip(net.submit(x).get(), (feat, s)):
        assert RI.same_bits(got, want)
    # checks come before anything is launched: a position the net does not have
    declare(net, index=2)
    for call in (lambda: net(x), lambda: net(pa.asarray(x)), lambda: net.submit(x), lambda: net(x, debug=True)):
        with pytest.raises(ValueError, match="returns 2"):
            call()
    pa.hip.trim_side_contexts()


def check_one_output_net_and_uint8_input(pa, declare, mirror, names, shapes, spec):
    """The tiny net with the one output s behind a uint8 image input: declare(net) puts the head on it, and the arrays that come
    back, of `shapes`, are bit for bit mirror(s) of the float s a second instance returns for the decoded bytes; so is
    spec.encode on that s.  -> (net, x) for what a head has to add."""
    g, b = tiny_net(["s"])
    net, plain = pa.from_graph(g, b), pa.from_graph(g, b)
    k, bb = np.ones(3, F32), np.zeros(3, F32)                               # the bytes as they are: integers
    declare(net.image_input(k, bb))
    i = np.arange(2 * 8 * 8 * 3, dtype=np.int64)
    x = ((i * 37 + i // 192 * 53 + 11) % 256).astype(np.uint8).reshape(2, 8, 8, 3)
    x = np.ascontiguousarray(np.repeat(np.repeat(x, 4, 1), 4, 2))
    s = plain(RI.decode32(x, k, bb))
    ref = mirror(s)
    for what, y in (("host", net(x)), ("device", net(pa.asarray(x))), ("submit", net.submit(x).get()), ("float in", net(RI.decode32(x, k, bb)))):
        assert len(y) == len(names), what
        same(host(y), ref, names, what)
    assert [a.shape for a in net(x)] == list(shapes)
    same(host(spec.encode(pa.asarray(s))), ref, names, type(spec).__name__ + ".encode")      # the spec on its own, on the float s
    pa.hip.trim_side_contexts()
    return net, x

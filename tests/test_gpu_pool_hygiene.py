"""The pool's hygiene mode itself (pl_pool_debug / pl_pool_debug_check) on a real MI355X: that the caching pool
really masks stale data and slack, that a hygiene block is [guard][exactly the requested bytes, poisoned][guard] on a
256-byte aligned payload, that a write into either guard -- planted with pl_memset INSIDE the block's own allocation, so
nothing faults -- is reported with its side, offsets and byte count, once, for live and for freed blocks, and that an output
element nobody wrote fails `assert_close` under both poison bytes."""
import ctypes
import re

import numpy as np
import pytest

from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

GUARD = 64 << 10
SIZES = [1, 3, 4, 511, 512, 513, (1 << 20) - 4, (1 << 20) + 4]


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


@pytest.fixture
def ctx(pa):
    """A context of its own: its pool statistics start at zero and nothing else allocates from it."""
    c = pa.hip.Context(pa.hip.context().device)
    yield c
    c.close()


def _alloc(ctx, nbytes):
    from planer_amd import _lib
    p = ctypes.c_void_p()
    _lib.call("pl_alloc", ctx.handle, nbytes, ctypes.byref(p))
    return p.value


def _free(ctx, p):
    from planer_amd import _lib
    _lib.call("pl_free", ctx.handle, ctypes.c_void_p(p))


def _memset(ctx, p, byte, nbytes):
    from planer_amd import _lib
    _lib.call("pl_memset", ctx.handle, ctypes.c_void_p(p), byte, nbytes)


def _read(ctx, p, nbytes):
    from planer_amd import _lib
    out = np.empty(nbytes, np.uint8)
    _lib.call("pl_d2h", ctx.handle, out.ctypes.data, ctypes.c_void_p(p), nbytes)
    return out


def _block(ctx, p):
    from planer_amd import _lib
    base, size = ctypes.c_void_p(), ctypes.c_size_t()
    _lib.call("pl_pool_block", ctx.handle, ctypes.c_void_p(p), ctypes.byref(base), ctypes.byref(size))
    return base.value, size.value


def test_the_pool_masks_stale_data_and_the_mode_unmasks_it(ctx):
    a = _alloc(ctx, 4000)
    _memset(ctx, a, 0x3C, 4000)
    _free(ctx, a)
    b = _alloc(ctx, 4000)
    assert b == a and (_read(ctx, b, 4000) == 0x3C).all()          # the same block with the previous tenant's bytes
    assert _block(ctx, b)[1] == 4096                               # ... and 96 bytes of slack nobody looks at
    for poison in (0xFF, 0x7F):
        ctx.pool_debug(GUARD, poison)
        c = _alloc(ctx, 4000)
        assert c != a and (_read(ctx, c, 4000) == poison).all()
        _memset(ctx, c, 0x3C, 4000)
        _free(ctx, c)
        d = _alloc(ctx, 4000)
        assert d not in (a, c) and (_read(ctx, d, 4000) == poison).all()
        _free(ctx, d)
        assert ctx.pool_debug_check()[0] == 0
        ctx.pool_debug(0)
    assert ctx.pool_stats() == (4096, 4096)                        # nothing of the mode is left
    _free(ctx, b)


@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("poison", [0xFF, 0x7F])
def test_layout(ctx, nbytes, poison):
    start = ctx.pool_stats()
    ctx.pool_debug(GUARD, poison)
    p = _alloc(ctx, nbytes)
    assert p % 256 == 0
    assert (_read(ctx, p, nbytes) == poison).all()
    assert ctx.pool_stats() == (start[0] + 2 * GUARD + nbytes, start[1] + nbytes)
    assert _block(ctx, p) == (p, nbytes) and _block(ctx, p + nbytes - 1) == (p, nbytes)
    # the guards are there, filled with one byte that is not the poison, right up to the payload on both sides
    front, back = _read(ctx, p - GUARD, GUARD), _read(ctx, p + nbytes, GUARD)
    assert front[0] != poison and (front == front[0]).all() and (back == front[0]).all()
    assert ctx.pool_debug_check() == (0, "")
    _free(ctx, p)
    assert ctx.pool_stats() == (start[0] + 2 * GUARD + nbytes, start[1])       # kept as evidence until the check
    assert ctx.pool_debug_check() == (0, "")
    assert ctx.pool_stats() == start
    ctx.pool_debug(0)


# (name, offset of the 4 planted bytes from the payload start as f(nbytes), side, first, last) -- offsets as the report counts
# them: end+k is k bytes past the payload's last byte, start-k is k bytes before its first
PLANTS = [("just past the end", lambda n: n, "back", "end+0", "end+3"),
          ("just before the start", lambda n: -4, "front", "start-4", "start-1"),
          ("the last bytes of the back guard", lambda n: n + GUARD - 4, "back", "end+%d" % (GUARD - 4), "end+%d" % (GUARD - 1))]


@pytest.mark.parametrize("freed", [False, True], ids=["live", "freed"])
@pytest.mark.parametrize("plant", PLANTS, ids=[p[0] for p in PLANTS])
@pytest.mark.parametrize("nbytes", [513, 4096])
def test_planted_violations_are_reported_once(ctx, nbytes, plant, freed):
    from tests.test_gpu_hygiene_sweep import hygiene
    _, where, side, first, last = plant
    keep = []
    with pytest.raises(AssertionError, match="written outside their payload"):
        with hygiene(0xFF, ctx, GUARD):
            _free(ctx, _alloc(ctx, 100))                            # serial 1: a clean neighbour
            p = _alloc(ctx, nbytes)                                 # serial 2
            _memset(ctx, p + where(nbytes), 0x11, 4)
            keep.append(p)
            if freed:
                _free(ctx, p)
    ctx.pool_debug(GUARD, 0xFF)
    q = _alloc(ctx, nbytes)
    _memset(ctx, q + where(nbytes), 0x11, 4)
    if freed:
        _free(ctx, q)
    n, report = ctx.pool_debug_check()
    assert n == 1, report
    m = re.fullmatch(r"block #(\d+) \((\d+) bytes, (live|freed)\): (front|back) guard dirty, (\d+) bytes, first at (\S+), last at (\S+)\n",
                     report)
    assert m, report
    assert m.groups()[1:] == (str(nbytes), "freed" if freed else "live", side, "4", first, last), report
    assert ctx.pool_debug_check() == (0, "")                       # reported once
    if not freed:
        _free(ctx, q)
        _free(ctx, keep[0])
    assert ctx.pool_debug_check() == (0, "")
    ctx.pool_debug(0)
    assert ctx.pool_stats() == (0, 0)


@pytest.mark.parametrize("poison", [0xFF, 0x7F])
def test_an_unwritten_output_element_fails_the_comparison(pa, ctx, poison):
    from planer_amd import _lib
    want = np.random.default_rng(1).standard_normal(1000).astype(np.float32)
    src = pa.asarray(want, ctx=ctx)
    ctx.pool_debug(GUARD, poison)
    dst = pa.hip.empty((1000,), ctx=ctx)
    _lib.call("pl_d2d", ctx.handle, dst.ptr, src.ptr, want.nbytes - 4)
    got = dst.get()
    np.testing.assert_array_equal(got[:-1], want[:-1])
    assert got[-1:].tobytes() == bytes([poison]) * 4
    with pytest.raises(AssertionError, match="rel err"):
        assert_close(got, want)
    del dst
    assert ctx.pool_debug_check()[0] == 0
    ctx.pool_debug(0)


def test_mixed_lifetimes(ctx):
    old = _alloc(ctx, 3000)                                        # an ordinary block from before the switch
    _memset(ctx, old, 0x3C, 3000)
    ctx.pool_debug(GUARD, 0x7F)
    assert ctx.pool_stats() == (3072, 3072)
    h = _alloc(ctx, 3000)
    ctx.pool_debug(0)
    plain = _alloc(ctx, 3000)                                      # after the switch-off: the caching pool again
    assert ctx.pool_stats() == (3072 + 2 * GUARD + 3000 + 3072, 3072 + 3000 + 3072)
    assert (_read(ctx, old, 3000) == 0x3C).all() and (_read(ctx, h, 3000) == 0x7F).all()
    _free(ctx, h)                                                  # a hygiene block freed with the mode off
    _free(ctx, old)
    _free(ctx, plain)
    assert ctx.pool_stats() == (3072 + 2 * GUARD + 3000 + 3072, 0)
    assert ctx.pool_debug_check() == (0, "")
    assert ctx.pool_stats() == (2 * 3072, 0)                       # the ordinary blocks are cached, the hygiene block is gone
    assert _alloc(ctx, 3000) in (old, plain)
    ctx.trim()


def test_trim_and_destroy_with_hygiene_blocks_present(pa):
    c = pa.hip.Context(pa.hip.context().device)
    cached = _alloc(c, 2000)
    _free(c, cached)                                               # an ordinary block on the free list
    c.pool_debug(GUARD, 0xFF)
    assert c.pool_stats() == (0, 0)
    live, gone = _alloc(c, 2000), _alloc(c, 70000)
    _free(c, gone)                                                 # quarantined
    before = c.pool_stats()
    assert before == (4 * GUARD + 72000, 2000)
    c.trim()                                                       # neither a live nor a quarantined hygiene block is a cached block
    assert c.pool_stats() == before and _block(c, live) == (live, 2000)
    c.close()                                                      # pl_ctx_destroy releases both, guards and all


def test_capture_allocates_as_with_the_mode_off(ctx):
    from planer_amd import _lib

    def captured():
        """reserved / in-use deltas after the capture and after its graph is gone"""
        ctx.trim()
        s0 = ctx.pool_stats()
        _lib.call("pl_capture_begin", ctx.handle)
        a = _alloc(ctx, 5000)
        _memset(ctx, a, 1, 5000)
        b = _alloc(ctx, 70000)
        _memset(ctx, b, 2, 70000)
        _free(ctx, a)
        c = _alloc(ctx, 5000)                                      # inside a capture a freed block is handed out again
        _memset(ctx, c, 3, 5000)
        g = ctypes.c_void_p()
        _lib.call("pl_capture_end", ctx.handle, ctypes.byref(g))
        s1 = ctx.pool_stats()
        _lib.call("pl_graph_launch", g)
        ctx.synchronize()
        same = c == a
        _free(ctx, b)
        _free(ctx, c)
        _lib.call("pl_graph_destroy", g)
        s2 = ctx.pool_stats()
        return same, (s1[0] - s0[0], s1[1] - s0[1]), (s2[0] - s0[0], s2[1] - s0[1])

    off = captured()
    ctx.pool_debug(GUARD, 0xFF)
    on = captured()
    assert ctx.pool_debug_check() == (0, "")
    ctx.pool_debug(0)
    assert on == off and off[0] is True, (off, on)

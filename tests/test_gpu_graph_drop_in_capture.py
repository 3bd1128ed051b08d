"""A captured graph dropped while the same context's stream is capturing another one.

`Net` plans are released by Python's collector, which runs when it likes -- also in the middle of the next plan's capture on the
shared default context.  pl_graph_destroy synchronises the context's stream before it frees the graph; on a capturing stream that
call is illegal and invalidates the capture, and the next launch fails with "operation failed due to a previous error during
capture".  The library therefore keeps such a graph until the capture has ended (csrc/runtime.hip, `cap_doomed`)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _capture(ctx, body):
    from planer_amd import _lib
    _lib.call("pl_capture_begin", ctx.handle)
    g = _lib.c_void_p()
    try:
        body()
    finally:
        rc = _lib.load().pl_capture_end(ctx.handle, _lib.byref(g))
    _lib.check(rc)
    return g


def test_a_graph_dropped_during_another_capture_leaves_that_capture_valid():
    import planer_amd
    from planer_amd import _lib, hip
    ctx = hip.context()
    n = 1024
    host = (np.arange(n, dtype=np.float32) - 512) / 8
    x = planer_amd.asarray(host, ctx=ctx)
    y, z = hip.empty((n,), ctx=ctx), hip.empty((n,), ctx=ctx)
    old = _capture(ctx, lambda: _lib.call("pl_relu_f32", ctx.handle, x.ptr, y.ptr, n))
    _lib.call("pl_graph_launch", old)
    ctx.synchronize()

    def body():
        _lib.call("pl_relu_f32", ctx.handle, x.ptr, z.ptr, n)
        _lib.check(_lib.load().pl_graph_destroy(old))             # what _Plan.__del__ does when the collector runs here
        _lib.call("pl_leakyrelu_f32", ctx.handle, z.ptr, y.ptr, n, 0.5)
    new = _capture(ctx, body)
    _lib.call("pl_graph_launch", new)
    ctx.synchronize()
    want = np.maximum(host, 0)
    assert np.array_equal(z.get(), want) and np.array_equal(y.get(), want)      # leakyrelu of a relu'd tensor changes nothing
    # the pool is usable and a second capture works: the deferred graph went away with the first
    again = _capture(ctx, lambda: _lib.call("pl_leakyrelu_f32", ctx.handle, x.ptr, y.ptr, n, 0.5))
    _lib.call("pl_graph_launch", again)
    ctx.synchronize()
    assert np.array_equal(y.get(), np.where(host > 0, host, host * np.float32(0.5)))
    for g in (new, again):
        _lib.check(_lib.load().pl_graph_destroy(g))

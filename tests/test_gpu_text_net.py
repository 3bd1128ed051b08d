"""Text as net output on a real MI355X, through nets (Net.text_output): every call form of the tiny net of
tests/head_kit.py, and the CRNN of irgen/crnn.py in the forms that ship, the declared net's four arrays against the mirror of the
float output taken by the same route."""
import numpy as np
import pytest

from tests import head_kit as K
from tests import text_ref as R

pytestmark = pytest.mark.gpu

NAMES = ("text", "length", "conf", "spans")
TINY = dict(layout="nchw", blank=0, merge_repeated=True, confidence="value", max_len=64)


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def _tiny_mirror(s):
    """The tiny net's (2, 3, 32, 32) s: 64 lines of 32 frames over 3 classes, integers with many ties."""
    ref = R.ctc_greedy(s, "nchw", 0, True, "value", 64)
    assert ref[1].shape == (2, 32) and ref[1].max() >= 2 and len(np.unique(ref[0])) >= 2       # symbols, and rows behind them
    return ref


@pytest.mark.parametrize("streams", [None, "pipe2"])
def test_tiny_net_every_call_form(pa, streams):
    K.check_every_call_form(pa, streams, lambda net, index: net.text_output(index=index, **TINY), _tiny_mirror, NAMES)


def test_one_output_net_and_uint8_input(pa):
    net, x = K.check_one_output_net_and_uint8_input(pa, lambda net: net.text_output(**TINY), _tiny_mirror, NAMES,
                                                    [(2, 32, 64), (2, 32), (2, 32, 64), (2, 32, 64, 2)], pa.util.TextSpec(**TINY))
    with pytest.raises(ValueError, match="text output is declared"):
        net.tiled(x[0], window=16)
    pa.hip.trim_side_contexts()


def test_lstm_with_init_states_under_submit(pa):
    """`lstm` alone in a Net, its initial states inits and not zero, so the first step's h R^T matters: `submit` (a throughput
    plan captured on a replica's stream, in another context than the inits) answers what `net(x)` answers, bit for bit, however
    the pools are churned between the passes, and both are the numpy oracle's LSTM.  Before layer.LSTM viewed the initial state
    from X's context, the first step's GEMM was enqueued on the net's own stream, outside the replica's graph, and replays read
    its freed output block."""
    from oracle import planer_np as onp
    from planer_amd.irgen.builder import GraphBuilder
    T, N, D, H = 6, 2, 16, 8
    rng = np.random.default_rng(17)
    w = [rng.standard_normal(s).astype(np.float32) * 0.5 for s in ((2, 4 * H, D), (2, 4 * H, H), (2, 8 * H), (2, N, H), (2, N, H))]
    g = GraphBuilder(["x"])
    for name, a in zip(("W", "R", "B", "h0", "c0"), w):
        g.init(name, a)
    g.init("lens", np.zeros(N, np.int64))
    g.op("lstm", ["x", "W", "R", "B", "lens", "h0", "c0"], ["Y", "Yh", "Yc"], name="lstm", hidden_size=H, direction="bidirectional")
    graph, blob = g.finish(["Y"])
    net = pa.from_graph(graph, blob)
    x = rng.standard_normal((T, N, D)).astype(np.float32)
    want = net(x)
    assert want.shape == (T, 2, N, H)
    ref = onp.lstm(x, w[0], w[1], w[2], np.zeros(N, np.int64), w[3], w[4], hidden_size=H, direction="bidirectional")[0]
    np.testing.assert_allclose(want, ref, rtol=1e-4, atol=1e-5)
    for i in range(4):
        junk = [pa.asarray(rng.standard_normal(n).astype(np.float32)) for n in (N * 4 * H, 64, 4096)]      # churn the net's pool
        got = net.submit(x).get()
        assert got.tobytes() == want.tobytes(), "submit %d differs from net(x) at %d places" % (
            i, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        del junk
    pa.hip.trim_side_contexts()


ALPHABET = "-0123456789"


@pytest.mark.parametrize("recurrent", [False, True], ids=["convolutional", "recurrent"])
def test_crnn_text_equals_the_mirror_of_its_float_output(pa, recurrent):
    """irgen.crnn at (2, 3, 32, 64), hidden 32, 11 classes.  The softmax confidence is the one inexact output: it is held to the
    float64 value of the logits within text_ref's bound; the value-mode run is bit for bit throughout.  The logits are the
    net's own float output by the same route, taken before the declaration (which touches no plan).  A second, undeclared
    instance is held to 1e-4 only: run alone, two instances of this float-weight net agree bit for bit by every route, but
    behind the rest of the GPU suite, in one process with it, their float outputs were seen to differ in the last place at 330
    of 352 values (the context's conv picks are measured and move while other tests run), so the second instance cannot be the
    bit-for-bit reference here that it is for the tiny net's integers."""
    from planer_amd.irgen import crnn
    g, b = crnn.build(classes=11, hidden=32, channels=3, recurrent=recurrent, batch=2)
    x = crnn.make_input(2, size=(32, 64), channels=3)
    layout, shape = ("tnc", (16, 2, 11)) if recurrent else ("nchw", (2, 11, 1, 16))
    net, plain = pa.from_graph(g, b), pa.from_graph(g, b)
    logits = plain(x)
    assert logits.shape == shape and np.isfinite(logits).all()
    form = "time" if layout == "nchw" else "rows"
    dev = pa.asarray(x)
    routes = [("host", lambda n: n(x), False), ("device", lambda n: n(dev), True), ("submit", lambda n: n.submit(x).get(), False),
              ("submit device", lambda n: n.submit(dev).result(), True), ("compile + replay", lambda n: n.compile(dev) and n(dev), True),
              ("replay again", lambda n: n(dev), True)]
    for confidence in ("value", "softmax"):
        for what, route, on_device in routes:
            floats = K.host((route(net.float_output()),))[0]                  # the float output by the same route
            assert floats.shape == shape, what
            np.testing.assert_allclose(floats, K.host((route(plain),))[0], rtol=1e-4, atol=1e-4, err_msg=what)
            net.text_output(layout, confidence=confidence, max_len=16)
            ref = R.ctc_greedy(floats, layout, 0, True, confidence, 16)
            assert ref[1].min() >= 1, what
            y = route(net)
            assert isinstance(y, tuple) and len(y) == 4, what
            assert all(isinstance(v, pa.hip.DeviceArray if on_device else np.ndarray) for v in y), what
            y = K.host(y)
            if confidence == "value":
                K.same(y, ref, NAMES, what)
                continue
            K.same((y[0], y[1], y[3]), (ref[0], ref[1], ref[3]), ("text", "length", "spans"), what)
            _, seq = R.frames_of(floats, layout)
            conf, spans, length = y[2].reshape(-1, 16), ref[3].reshape(-1, 16, 2), ref[1].reshape(-1)
            for s in range(conf.shape[0]):
                n = min(int(length[s]), 16)
                rows = seq[s, spans[s, :n, 0]]
                assert (np.abs(conf[s, :n] - R.frame_conf64(rows)) <= R.conf_bound(rows, form)).all(), what
                assert not conf[s, n:].view(np.uint32).any(), what
    text, length = net(x)[:2]
    strings = pa.util.text_strings(text, length, ALPHABET)
    flat = strings if recurrent else [s for line in strings for s in line]
    assert len(flat) == 2 and all(isinstance(s, str) and 1 <= len(s) <= 16 and "-" not in s for s in flat)
    assert [len(s) for s in flat] == np.minimum(length.reshape(-1), 16).tolist()
    assert net.float_output() is net                                         # the float tensor again
    np.testing.assert_allclose(net(x), logits, rtol=1e-4, atol=1e-4)
    print("crnn %s: %r" % ("recurrent" if recurrent else "convolutional", flat))
    pa.hip.trim_side_contexts()


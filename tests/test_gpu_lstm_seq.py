"""pl_lstm_seq_f32 and layer.LSTM on top of it, on a real MI355X.  The reference of the bitwise tests is built here
from the unchanged ABI: pl_gemm_f32 (trans_b) + pl_lstm_cell_f32 per step and direction, the chain layer.LSTM ran before the
fused step kernel existed."""
import numpy as np
import pytest

from tests import head_kit as K
from tests import ref64_ops as R64

pytestmark = pytest.mark.gpu

F32 = np.float32
SIGNS = {"forward": [1], "reverse": [-1], "bidirectional": [1, -1]}
NAMES = ("Y", "c")


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def operands(seed, L, N, H, nd, spread=4.0):
    """-> (gx [nd x (L N, 4H)], R (nd, 4H, H), B (nd, 8H), h0, c0 (nd, N, H)): gates spread so that sigmoid and tanh see their
    range, h R^T of the gates' own size, initial states not zero."""
    rng = np.random.default_rng(seed)
    gx, B = [], []
    for _ in range(nd):
        g, _, b, _ = R64.lstm_operands(rng, L * N, H, spread)
        gx.append(g)
        B.append(b)
    Rw = (rng.standard_normal((nd, 4 * H, H)) * (spread / np.sqrt(H))).astype(F32)
    h0 = rng.uniform(-1, 1, (nd, N, H)).astype(F32)
    c0 = np.stack([R64.lstm_operands(rng, N, H, spread)[3] for _ in range(nd)])
    return gx, Rw, np.stack(B), h0, c0


def chain(pa, ops, L, N, H, signs, gates_h=None, plans=None):
    """The per-step chain on the default context -> (Y (L, nd, N, H), final c (nd, N, H)).  gates_h: [nd x (N, 4H)] fed to the
    cell instead of the GEMM's result (L == 1).  plans: a list that collects the GEMMs' launch plans."""
    from planer_amd import _lib
    ctx = pa.hip.context()
    gx, Rw, B, h0, c0 = ops
    nd = len(signs)
    d_gx, d_R, d_B, d_h0, d_c0 = [pa.asarray(g) for g in gx], pa.asarray(Rw), pa.asarray(B), pa.asarray(h0), pa.asarray(c0)
    Y = pa.hip.zeros((L, nd, N, H))
    finals = []
    for i, sign in enumerate(signs):
        h, c = d_h0[i], d_c0[i]
        for t in range(L)[::sign]:
            if gates_h is None:
                gh = pa.hip.empty((N, 4 * H))
                _lib.call("pl_gemm_f32", ctx.handle, h.ptr, N, H, d_R[i].ptr, 4 * H, 1, None, gh.ptr)
                if plans is not None:
                    plans.append(ctx.last_conv_plan())
            else:
                gh = pa.asarray(gates_h[i])
            h_new, c_new = Y[t][i], pa.hip.empty((N, H))
            _lib.call("pl_lstm_cell_f32", ctx.handle, d_gx[i].rows(t * N, (t + 1) * N).ptr, gh.ptr, d_B[i].ptr, c.ptr, h_new.ptr,
                      c_new.ptr, N, H)
            h, c = h_new, c_new
        finals.append(c.get())
    return Y.get(), np.stack(finals)


def seq_rc(ctx, ptrs, L, N, H, nd, sign0):
    """The raw call: ptrs = (gx0, gx1 or None, R, B, h0, c0, Y, c) as integers -> status."""
    from planer_amd import _lib
    return _lib.load().pl_lstm_seq_f32(ctx.handle, *ptrs, L, N, H, nd, sign0)


def fused(pa, ops, L, N, H, signs, ctx=None, out=None, c_is_c0=False):
    """pl_lstm_seq_f32 on `ctx` -> (Y, c) device arrays; out = (Y pointer, c pointer) writes there instead and returns None;
    c_is_c0: the state buffer is the device copy of c0 itself."""
    from planer_amd import _lib
    ctx = ctx or pa.hip.context()
    gx, Rw, B, h0, c0 = ops
    nd = len(signs)
    d = [pa.asarray(g, ctx=ctx) for g in gx] + [pa.asarray(a, ctx=ctx) for a in (Rw, B, h0, c0)]
    Y, c = (None, None) if out else (pa.hip.empty((L, nd, N, H), ctx=ctx), pa.hip.empty((nd, N, H), ctx=ctx))
    if c_is_c0:
        c = d[-1]
    ptrs = (d[0].ptr, d[1].ptr if nd == 2 else None) + tuple(a.ptr for a in d[nd:]) + (out or (Y.ptr, c.ptr))
    _lib.check(seq_rc(ctx, ptrs, L, N, H, nd, signs[0]))
    ctx.synchronize()                                            # the operands stay alive until the launches are done
    return None if out else (Y, c)


# ---- 1. bit for bit against the per-step chain, where its GEMM is dense_small_kernel --------------------------------------------
@pytest.mark.parametrize("direction", ["forward", "reverse", "bidirectional"])
@pytest.mark.parametrize("H", [64, 72, 128])
def test_bits_of_the_per_step_chain(pa, H, direction):
    """H = 72: 9 K steps over four waves is 3, 3, 3, 0 -- wave 3 has none.  N = 33 and 64: two row blocks, the second ragged or
    full."""
    signs = SIGNS[direction]
    for N in (1, 31, 32, 33, 64):
        for L in (1, 2, 5):
            ops = operands(1000 * H + 10 * N + L, L, N, H, len(signs))
            plans = []
            want = chain(pa, ops, L, N, H, signs, plans=plans)
            assert len(plans) == L * len(signs) and all(p.startswith("dense32x32") for p in plans), plans
            got = fused(pa, ops, L, N, H, signs)
            K.same(K.host(got), want, NAMES, "H %d N %d L %d %s" % (H, N, L, direction))
            assert np.isfinite(want[0]).all() and len(np.unique(want[0])) > want[0].size // 4       # gates that say something


# ---- 2. outside that domain --------------------------------------------------------------------------------------------------
OUTSIDE = [(8, 1), (8, 33), (16, 1), (16, 33), (40, 1), (40, 33), (64, 65), (64, 97)]


# inside the dense_small domain too: there the bitwise reference shares dense_tile.h with the kernel under test, and numpy's exact
# gates_h does not.  H = 72: the uneven split of the K steps over the waves; N = 33, 64: two row blocks
INSIDE = [(72, 1), (72, 33), (128, 31), (128, 64)]


@pytest.mark.parametrize("H, N", OUTSIDE + INSIDE)
def test_exact_on_integer_recurrence(pa, H, N):
    """R and h0 small integers: h R^T is exact in float32 in any order (|sum| <= 64 H), so the fused step equals the cell kernel
    fed the exact gates_h, whatever GEMM the per-step chain would have picked here."""
    for direction in ("forward", "bidirectional"):
        signs = SIGNS[direction]
        gx, _, B, _, c0 = operands(7 * H + N, 1, N, H, len(signs))
        rng = np.random.default_rng(H * 100 + N)
        Rw = rng.integers(-8, 9, (len(signs), 4 * H, H)).astype(F32)
        h0 = rng.integers(-8, 9, (len(signs), N, H)).astype(F32)
        gh = [(h0[i].astype(np.float64) @ Rw[i].astype(np.float64).T) for i in range(len(signs))]
        assert all(np.abs(g).max() < 2 ** 24 and np.abs(g).max() > 8 for g in gh)
        ops = (gx, Rw, B, h0, c0)
        want = chain(pa, ops, 1, N, H, signs, gates_h=[g.astype(F32) for g in gh])
        K.same(K.host(fused(pa, ops, 1, N, H, signs)), want, NAMES, "H %d N %d %s" % (H, N, direction))


@pytest.mark.parametrize("H, N", OUTSIDE)
def test_float_sequence_against_the_numpy_oracle(pa, H, N):
    """L = 5, bidirectional, float operands against oracle.planer_np.lstm at the tolerance test_lstm_with_init_states_under_submit
    holds this size to.  The oracle gets the gates through W = the two halves of an identity, which is exact."""
    from oracle import planer_np as onp
    L, rng = 5, np.random.default_rng(31 * H + N)
    gx = [rng.standard_normal((L * N, 4 * H)).astype(F32) * F32(0.5) for _ in range(2)]
    Rw, B, h0, c0 = (rng.standard_normal(s).astype(F32) * F32(0.5) for s in ((2, 4 * H, H), (2, 8 * H), (2, N, H), (2, N, H)))
    X = np.concatenate(gx, axis=1).reshape(L, N, 8 * H)
    eye = np.eye(8 * H, dtype=F32)
    W = np.stack([eye[:4 * H], eye[4 * H:]])
    ref_Y, _, ref_c = onp.lstm(X, W, Rw, B, np.zeros(N, np.int64), h0, c0, hidden_size=H, direction="bidirectional")
    Y, c = K.host(fused(pa, (gx, Rw, B, h0, c0), L, N, H, [1, -1]))
    np.testing.assert_allclose(Y, ref_Y, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(c[1], ref_c[0], rtol=1e-4, atol=1e-5)                # the oracle keeps the last direction's


def test_state_buffer_may_be_c0_itself(pa):
    """include/planer_hip.h: "c may be c0 itself" -- the thread that owns (n, j) reads c0 before it writes c."""
    for H, N, L, direction in ((64, 33, 3, "bidirectional"), (8, 5, 2, "reverse")):
        signs = SIGNS[direction]
        ops = operands(H + L, L, N, H, len(signs))
        want = K.host(fused(pa, ops, L, N, H, signs))
        K.same(K.host(fused(pa, ops, L, N, H, signs, c_is_c0=True)), want, NAMES, "c is c0, H %d" % H)


# ---- 3. special values -------------------------------------------------------------------------------------------------------
def test_special_values_equal_the_chain(pa):
    H, N, L, signs = 64, 33, 2, [1, -1]
    gx, Rw, B, h0, c0 = operands(5, L, N, H, 2)
    specials = [F32(np.nan), F32(np.inf), F32(-np.inf), F32(-0.0)]
    rng = np.random.default_rng(9)
    for arr in gx + [h0[0], h0[1], c0[0], c0[1]]:
        flat = arr.reshape(-1)
        at = rng.choice(flat.size, 3 * len(specials), replace=False)
        flat[at] = np.tile(specials, 3)
    h0[1, N - 1, H - 1], c0[0, 32, 0], gx[1][0, 0] = np.nan, -np.inf, -0.0           # the ragged row block and the corners
    ops = (gx, Rw, B, h0, c0)
    want = chain(pa, ops, L, N, H, signs)
    assert np.isnan(want[0]).any() and np.isfinite(want[0]).any() and np.isnan(want[1]).any()
    K.same(K.host(fused(pa, ops, L, N, H, signs)), want, NAMES, "special values")


# ---- 4. writes only what it owns ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, N, L, direction", [(72, 33, 2, "bidirectional"), (8, 1, 3, "reverse"), (64, 31, 1, "forward")])
def test_framed_outputs(pa, H, N, L, direction):
    signs = SIGNS[direction]
    nd = len(signs)
    ops = operands(77 + H, L, N, H, nd)
    Y, c = K.Framed(pa, L * nd * N * H), K.Framed(pa, nd * N * H)
    fused(pa, ops, L, N, H, signs, out=(Y.ptr, c.ptr))
    (gy, y_ok), (gc, c_ok) = Y.get(F32, (L, nd, N, H)), c.get(F32, (nd, N, H))
    assert y_ok and c_ok, "a write outside Y or c"
    assert not (gy.view(np.uint32) == K.SENT).any() and not (gc.view(np.uint32) == K.SENT).any()      # and all of both written
    if H >= 64:
        K.same((gy, gc), chain(pa, ops, L, N, H, signs), NAMES, "framed")


def test_under_pool_hygiene(pa):
    shapes = [(64, 33, 2, "bidirectional"), (72, 1, 3, "reverse"), (128, 64, 1, "forward"), (64, 31, 5, "bidirectional")]
    kept, cases = {}, []
    for H, N, L, direction in shapes:
        ops = operands(H + N + L, L, N, H, len(SIGNS[direction]))
        kept[(H, N, L, direction)] = ops
        cases.append(("H %d N %d L %d %s" % (H, N, L, direction), (H, N, L, direction), chain(pa, ops, L, N, H, SIGNS[direction])))
    K.hygiene_pass(pa, cases, lambda key: fused(pa, kept[key], key[2], key[1], key[0], SIGNS[key[3]]), NAMES, 3)


# ---- 5. reproducible ---------------------------------------------------------------------------------------------------------
def test_two_contexts_give_the_same_bits_at_hidden_8(pa):
    """The layer at H = 8, where the per-step GEMM went through a measured conv pick and two instances differed in the last
    place.  X and W are small integers, so the input GEMM is exact whatever it picks; everything recurrent is float."""
    L, N, D, H = 6, 2, 16, 8
    rng = np.random.default_rng(17)
    X, W = rng.integers(-3, 4, (L, N, D)).astype(F32), rng.integers(-2, 3, (2, 4 * H, D)).astype(F32)
    Rw, B, h0, c0 = (rng.standard_normal(s).astype(F32) * F32(0.5) for s in ((2, 4 * H, H), (2, 8 * H), (2, N, H), (2, N, H)))
    ctxs = [pa.hip.context(), pa.hip.side_context(pa.hip.context().device, 1)]
    runs = []
    for ctx in ctxs + ctxs:
        d = [pa.asarray(a, ctx=ctx) for a in (X, W, Rw, B)] + [np.zeros(N, np.int64)] + [pa.asarray(a, ctx=ctx) for a in (h0, c0)]
        runs.append(K.host(pa.layer_map["lstm"](*d, hidden_size=H, direction="bidirectional")))
    for other in runs[1:]:
        K.same(other, runs[0], ("Y", "H", "C"), "another context or run")
    pa.hip.trim_side_contexts()


# ---- 6. through the layer and the net ----------------------------------------------------------------------------------------
def _layer_operands(seed, L, N, D, H, nd):
    rng = np.random.default_rng(seed)
    shapes = ((L, N, D), (nd, 4 * H, D), (nd, 4 * H, H), (nd, 8 * H), (nd, N, H), (nd, N, H))
    return [rng.standard_normal(s).astype(F32) * F32(0.5) for s in shapes]


def _calls_of(pa, fn):
    """fn() with every C-ABI call's name collected -> (result, names)."""
    from planer_amd import _lib
    names = []
    _lib._recorder = lambda name, args: names.append(name)
    try:
        return fn(), names
    finally:
        _lib._recorder = None


@pytest.mark.parametrize("direction", ["forward", "reverse", "bidirectional"])
def test_layer_shapes_and_switch(pa, direction, monkeypatch):
    from oracle import planer_np as onp
    L, N, D, H, nd = 5, 3, 24, 64, len(SIGNS[direction])
    x, W, Rw, B, h0, c0 = _layer_operands(3, L, N, D, H, nd)

    def run():
        d = [pa.asarray(a) for a in (x, W, Rw, B)] + [np.zeros(N, np.int64), pa.asarray(h0), pa.asarray(c0)]
        return K.host(pa.layer_map["lstm"](*d, hidden_size=H, direction=direction))

    monkeypatch.delenv("PLANER_HIP_LSTM_FUSED", raising=False)
    got, names = _calls_of(pa, run)
    assert names.count("pl_lstm_seq_f32") == 1 and "pl_lstm_cell_f32" not in names and names.count("pl_gemm_f32") == nd
    ref = onp.lstm(x, W, Rw, B, np.zeros(N, np.int64), h0, c0, hidden_size=H, direction=direction)
    assert [a.shape for a in got] == [a.shape for a in ref] == [(L, nd, N, H), (N, H), (1, N, H)]
    for g, r in zip(got, ref):
        np.testing.assert_allclose(g, r, rtol=1e-4, atol=1e-5)
    monkeypatch.setenv("PLANER_HIP_LSTM_FUSED", "0")                                   # read at call time
    old, names = _calls_of(pa, run)
    assert "pl_lstm_seq_f32" not in names and names.count("pl_lstm_cell_f32") == L * nd
    K.same(got, old, ("Y", "H", "C"), "fused against PLANER_HIP_LSTM_FUSED=0")


def test_layer_keeps_the_per_step_program_where_the_rule_says_no(pa):
    """H = 12 and L = 0: no fused call, and the per-step program's results as they were."""
    for L, H in ((3, 12), (0, 8)):
        x, W, Rw, B, h0, c0 = _layer_operands(4, L, 2, 16, H, 1)
        d = [pa.asarray(a) for a in (x, W, Rw, B)] + [np.zeros(2, np.int64), pa.asarray(h0), pa.asarray(c0)]
        got, names = _calls_of(pa, lambda: pa.layer_map["lstm"](*d, hidden_size=H, direction="forward"))
        assert "pl_lstm_seq_f32" not in names and names.count("pl_lstm_cell_f32") == L
        assert got[0].shape == (L, 1, 2, H) and (not L or [a.shape for a in got[1:]] == [(2, H), (1, 2, H)])


def test_one_op_net_every_route_agrees(pa):
    """`lstm` alone in a Net at H = 64, initial states inits and not zero: net(x), submit (a graph replayed on a replica, in
    another context than the inits), the compiled plan and a plan file replayed through ctypes agree bit for bit while the
    pools are churned between the calls."""
    from planer_amd.export import export_plan
    from planer_amd.irgen.builder import GraphBuilder
    from tests.test_gpu_plan_file import _bind, _run_plan
    T, N, D, H = 5, 3, 24, 64
    x, *w = _layer_operands(11, T, N, D, H, 2)
    g = GraphBuilder(["x"])
    for name, a in zip(("W", "R", "B", "h0", "c0"), w):
        g.init(name, a)
    g.init("lens", np.zeros(N, np.int64))
    g.op("lstm", ["x", "W", "R", "B", "lens", "h0", "c0"], ["Y", "Yh", "Yc"], name="lstm", hidden_size=H, direction="bidirectional")
    graph, blob = g.finish(["Y"])
    net = pa.from_graph(graph, blob)
    want = net(x)
    assert want.shape == (T, 2, N, H)
    d = [pa.asarray(a) for a in [x] + w[:3]] + [np.zeros(N, np.int64), pa.asarray(w[3]), pa.asarray(w[4])]
    K.same((want,), K.host(pa.layer_map["lstm"](*d, hidden_size=H, direction="bidirectional"))[:1], ("Y",), "net(x) against the layer")
    rng = np.random.default_rng(2)
    dev = pa.asarray(x)
    net.compile(dev)
    for i in range(3):
        junk = [pa.asarray(rng.standard_normal(n).astype(F32)) for n in (N * 4 * H, 64, 4096)]      # churn the net's pool
        K.same((net.submit(x).get(),), (want,), ("Y",), "submit %d" % i)
        K.same((net(dev).get(),), (want,), ("Y",), "compiled plan %d" % i)
        K.same((net(x),), (want,), ("Y",), "net(x) %d" % i)
        del junk
    plan = export_plan(net, x)
    assert b"pl_lstm_seq_f32" in plan and b"pl_lstm_cell_f32" not in plan
    out, = _run_plan(_bind(), plan, [x])
    K.same((out,), (want,), ("Y",), "plan file")
    pa.hip.trim_side_contexts()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what, code, message", [("H12", K.EUNSUPPORTED, "multiple of 8"), ("ndir3", K.EINVAL, "ndir = 3"),
                                                 ("L0", K.EINVAL, "L = 0"), ("R+4", K.EINVAL, "16-byte aligned")])
def test_refusals_launch_nothing(pa, what, code, message):
    from planer_amd import _lib
    ctx = pa.hip.context()
    L, N, H, nd = (0 if what == "L0" else 2), 3, (12 if what == "H12" else 16), (3 if what == "ndir3" else 2)
    room = pa.hip.zeros((4 * 4 * H * H + 3 * 8 * H + 2 * 4 * N * 4 * H + 64,))      # every operand fits in it, whatever is read
    Y, c = K.Framed(pa, 2 * 3 * N * H), K.Framed(pa, 3 * N * H)
    ptrs = (room.ptr, room.ptr, room.ptr + (4 if what == "R+4" else 0), room.ptr, room.ptr, room.ptr, Y.ptr, c.ptr)
    assert seq_rc(ctx, ptrs, L, N, H, nd, 1) == code
    assert "pl_lstm_seq_f32" in _lib.load().pl_last_error().decode() and message in _lib.load().pl_last_error().decode()
    ctx.synchronize()
    assert Y.untouched() and c.untouched()

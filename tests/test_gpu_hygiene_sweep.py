"""The kernels under the pool's hygiene mode (Context.pool_debug) on a real MI355X: WHERE they write, and whether
a result depends on bytes nobody wrote.

Every body below is an existing test body (imported, not copied) or the same loop over other shapes.  `sweep` runs it three
times on the default context: once with the mode off (the warm-up that fixes launch plans and algorithm picks), once with
every fresh block filled with 0xFF (every float a NaN, every integer -1) and once with 0x7F (3.39e38: finite, so it survives
`x > 0 ? x : 0`, which swallows a NaN), each allocation -- library workspaces included -- a block of its own between two
64 KiB guards.  Three things must hold:
  (a) the body's own comparison with the oracle / float64 passes under both poisons;
  (b) every host array the two poisoned runs read back is bit-identical between them (no tolerance: a result may not depend
      on bytes the program never wrote);
  (c) no guard byte changed (`hygiene` asserts it, with the library's report of block, side, offsets and byte count).
The last test of the module asserts what the sweep reached: the w_layouts, a split-K plan, both dense paths, the chain and
conv1x1 + Winograd-in kernels -- coverage is a condition.  Run with -s for seconds per group, mode off and on, and the peak
pool size.

Group "index ops" (test_index_ops_at_their_boundaries): a kept subset of tests/test_gpu_index_ops.py, one case per family across
its boundary -- TopK at n = 8193 and n = 16385, NonZero at 2C + 5 with density 0.5, the 70 000-update ScatterND, Gather past the
grid, Where at 1 048 579 and Cast at 1 200 003 elements, one comparison and Erf: 0.3 s mode off, 0.8 s for the two poisoned
runs."""
import contextlib
import ctypes
import gc
import re
import time

import numpy as np
import pytest

from oracle import planer_np as onp
from tests.conftest import RTOL, assert_close

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x7F)
# the library entry point of each conv family -> its w_layout (planer_amd/conv_layouts.py)
ENTRY_LAYOUT = {"pl_conv2d_q4_f32": 2, "pl_conv2d_winograd_q4_f32": 4, "pl_conv2d_rowpack_q4_f32": 6, "pl_conv2d_rowpacked_q4_f32": 6,
                "pl_conv2d_winograd4_q4_f32": 7, "pl_wino4_gemm_q4_f32": 7, "pl_conv2d_w1d4_q4_f32": 8, "pl_conv2d_wf4_q4_f32": 9,
                "pl_conv2d_rowpacked_pool_q4_f32": 10, "pl_conv2d_winograd43_q4_f32": 11, "pl_wino43_gemm_q4_f32": 11,
                "pl_conv2d_stem_pool_nchw_q4_f32": 12, "pl_conv2d_dw_q4_f32": 13, "pl_conv2d_convt_q4_f32": 14}
PLANNED = set(ENTRY_LAYOUT) | {"pl_conv2d_f32", "pl_conv2d_fused_f32", "pl_gemm_f32", "pl_conv2d_q4_pair_f32"}
REACHED = {"layouts": set(), "plans": set(), "dense": set(), "entries": set()}          # under the mode only
STATS = {}                                                              # group -> [seconds off, seconds on (two runs), peak reserved]
_STATE = {"on": False, "peak": 0}


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


@contextlib.contextmanager
def hygiene(poison, ctx=None, guard=None):
    """Hygiene mode on for `ctx` (default: the process-wide context) around the body; afterwards every guard of every block the
    body allocated, freed ones included, must be untouched."""
    from planer_amd import hip
    ctx = ctx or hip.context()
    ctx.pool_debug(hip.POOL_GUARD_BYTES if guard is None else guard, poison)
    _STATE["on"] = True
    try:
        yield ctx
        gc.collect()
        _STATE["peak"] = max(_STATE["peak"], ctx.pool_stats()[0])
        n, report = ctx.pool_debug_check()
        assert n == 0, "%d block(s) written outside their payload (poison %#x):\n%s" % (n, poison, report)
    finally:
        _STATE["on"] = False
        ctx.pool_debug(0)
        ctx.pool_debug_check()              # (after a failure in the body: releases what it freed)


@contextlib.contextmanager
def _watch(sink):
    """Collect every host array `DeviceArray.get()` returns (Winograd-domain tensors apart: their padded GEMM rows are never
    written and never used) and note which conv entry points ran and how they were launched."""
    from planer_amd import _lib, hip
    from planer_amd.net import Net
    get, call, pick = hip.DeviceArray.get, _lib.call, Net._pick_conv_algo

    def get_and_keep(self):
        a = get(self)
        if self.meta is None:
            sink[0].append(a.copy())
        return a

    def call_and_note(name, *args):
        call(name, *args)
        if _STATE["on"]:
            REACHED["entries"].add(name)
            if name in PLANNED:
                buf = ctypes.create_string_buffer(160)
                _lib.load().pl_conv2d_last_plan(args[0], buf, 160)
                REACHED["dense" if name == "pl_gemm_f32" else "plans"].add(buf.value.decode())
                if name in ENTRY_LAYOUT:
                    REACHED["layouts"].add(ENTRY_LAYOUT[name])

    picks = {}

    def pick_once(self, cands, K, srcs, para, shapes, q4=False):
        # a Net times its conv candidates anew; the three runs of a body must run the same kernels, so the warm-up's pick stays
        if self.force_algo is not None:
            return pick(self, cands, K, srcs, para, shapes, q4)
        key = (tuple(cands), tuple(K.shape), tuple(shapes[srcs[0].split("@")[0]]), tuple(srcs[2:6]), para.get("act", 0), q4,
               self._pick_mode)
        if key not in picks:
            picks[key] = pick(self, cands, K, srcs, para, shapes, q4)
        return picks[key]

    hip.DeviceArray.get, _lib.call, Net._pick_conv_algo = get_and_keep, call_and_note, pick_once
    try:
        yield
    finally:
        hip.DeviceArray.get, _lib.call, Net._pick_conv_algo = get, call, pick


def _identical(a, b, what):
    assert len(a) == len(b), "%s: %d host arrays under 0xFF, %d under 0x7F" % (what, len(a), len(b))
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and u.dtype == v.dtype, (what, i, u.shape, v.shape)
        if u.tobytes() != v.tobytes():
            diff = np.flatnonzero(u.view(np.uint8).reshape(-1) != v.view(np.uint8).reshape(-1)) // max(u.itemsize, 1)
            raise AssertionError("%s: host array %d of the run %s differs between poison 0xFF and 0x7F in %d elements, first at "
                                 "flat index %d (%r vs %r): the result depends on bytes nobody wrote"
                                 % (what, i, u.shape, len(set(diff.tolist())), diff[0], u.reshape(-1)[diff[0]], v.reshape(-1)[diff[0]]))


def sweep(group, body, what=""):
    from planer_amd import hip
    ctx = hip.context()
    sink, runs = [None], {}
    stat = STATS.setdefault(group, [0.0, 0.0, 0])
    with _watch(sink):
        for poison in (None,) + POISONS:
            sink[0] = runs[poison] = []
            t0 = time.perf_counter()
            if poison is None:
                body()
                ctx.synchronize()
            else:
                with hygiene(poison):
                    body()
            stat[0 if poison is None else 1] += time.perf_counter() - t0
    stat[2] = max(stat[2], _STATE["peak"])
    _identical(runs[0xFF], runs[0x7F], what or group)


# ---- operators: the seeded sweeps of tests/test_gpu_fuzz.py ---------------------------------------------------------------
@pytest.mark.parametrize("seed", range(120))
def test_fuzz_conv_every_family(pa, seed):
    from tests import test_gpu_fuzz as F
    sweep("fuzz conv", lambda: F.test_random_conv_every_eligible_kernel_family(pa, seed), "fuzz conv seed %d" % seed)


@pytest.mark.parametrize("seed", range(40))
def test_fuzz_pointwise(pa, seed):
    from tests import test_gpu_fuzz as F
    sweep("fuzz pointwise", lambda: F.test_random_pointwise_layers_nchw_and_q4_are_bit_exact(pa, seed), "fuzz pointwise seed %d" % seed)


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_dense(pa, seed):
    from tests import test_gpu_fuzz as F
    sweep("fuzz dense", lambda: F.test_random_dense_small_batch_and_general(pa, seed), "fuzz dense seed %d" % seed)


@pytest.mark.parametrize("seed", range(60))
def test_fuzz_second_wave(pa, seed):
    from tests import test_gpu_fuzz as F
    sweep("fuzz second wave", lambda: F.test_random_second_wave_ops_match_the_oracle(pa, seed), "fuzz second wave seed %d" % seed)


# ---- tile edges under every launch plan -----------------------------------------------------------------------------------
# Cout in {1, 33, 70, 130} x maps {1x1, 5x7, 13x29} x Cin in {3, 20}: every tile configuration (32 .. 128 rows, 32 .. 256
# columns, K chunks of 8 .. 32) gets a partial last row tile, column tile and K chunk; K = 180 (Cin 20) really splits.  The
# Cin 32 shape lets the tap-major configurations (Cin % 16 == 0) in.
_P1 = dict(strides=[1, 1], pads=[1, 1, 1, 1])
EDGES = [((2, 3, 1, 1), (1, 3, 3, 3), _P1), ((2, 20, 5, 7), (33, 20, 3, 3), _P1), ((1, 20, 13, 29), (70, 20, 3, 3), _P1),
         ((2, 3, 13, 29), (130, 3, 3, 3), _P1), ((3, 20, 5, 7), (130, 20, 1, 1), dict(strides=[1, 1], pads=[0, 0, 0, 0])),
         ((1, 20, 13, 29), (1, 20, 3, 3), dict(strides=[2, 2], pads=[1, 1, 1, 1])), ((2, 3, 5, 7), (70, 3, 3, 3), _P1),
         ((1, 20, 1, 1), (33, 20, 3, 3), _P1), ((2, 32, 5, 7), (33, 32, 3, 3), _P1)]


@pytest.mark.parametrize("shape", EDGES, ids=["%s-%s" % ("x".join(map(str, s[0])), "x".join(map(str, s[1]))) for s in EDGES])
def test_tile_edges_every_config_and_split(pa, shape):
    """The loops of test_gpu_layers.test_conv_every_tile_config_and_split_k and test_gpu_q4.test_q4_conv_every_tile_config_and_split_k
    on the edge shapes: here the split-K slabs and the reduce / reduce4 / Q4 reduce kernels get guards."""
    from planer_amd import q4
    from tests.test_gpu_layers import _cfg_names
    xs, ks, p = shape
    rng = np.random.default_rng(sum(xs) + sum(ks))
    x = rng.standard_normal(xs).astype(np.float32)
    k = (rng.standard_normal(ks) * 0.1).astype(np.float32)
    b = rng.standard_normal(ks[0]).astype(np.float32)
    ref = np.ascontiguousarray(onp.conv2d(x, k, b, **p))
    names = _cfg_names(pa)
    ctx = pa.hip.context()

    def body():
        dx, dk, db = pa.asarray(x), pa.asarray(k), pa.asarray(b)
        dkt = pa.prepare_conv_weights(dk) if ks[1] % 16 == 0 else None
        xq, kq = q4.to_q4(dx), q4.prepare_q4_weights(dk, 1)
        try:
            for cfg, name in enumerate(names):
                if name.startswith("q") or name.startswith("k"):
                    for split in ((1,) if name.startswith("k") else (1, 3)):
                        ctx.set_conv_config(cfg, split)
                        y = q4.from_q4(q4.ConvQ4(xq, kq, db, **p)).get()
                        assert_close(y, ref, RTOL, "q4 cfg %s split %d %s [%s]" % (name, split, xs, ctx.last_conv_plan()))
                if name.startswith("q"):
                    continue
                tap = name.startswith("t")
                if tap and (dkt is None or ks[1] % int(name.split("x")[-1])):
                    continue
                for split in (1, 3):
                    ctx.set_conv_config(cfg, split)
                    y = pa.ConvFused(dx, dkt if tap else dk, db, w_layout=int(tap), **p).get()
                    assert_close(y, ref, RTOL, "cfg %s split %d %s [%s]" % (name, split, xs, ctx.last_conv_plan()))
        finally:
            ctx.set_conv_config(-1, 0)

    sweep("tile edges", body, "tile edges %s" % (shape,))


# ---- Winograd families at maps that are not whole tiles -------------------------------------------------------------------
WINO_MAPS = [(2, 1, 1), (2, 3, 5), (1, 6, 6), (2, 7, 7), (1, 14, 14), (1, 15, 17)]
WINO_CH = [(4, 4), (20, 36), (68, 132)]          # the 64- and 128-channel GEMM blocks and the quad chunk loops are partial
WINO = [(n, ci, h, w, co) for ci, co in WINO_CH for n, h, w in WINO_MAPS]


@pytest.mark.parametrize("shape", WINO, ids=["x".join(map(str, s)) for s in WINO])
def test_winograd_families_on_partial_tiles(pa, shape, monkeypatch):
    """w_layout 4 and 8 against the oracle here; 7 (one call and staged, LDS transforms), the chain kernel, 9, 11 (7 / 14-pixel
    maps) and conv1x1 + Winograd-in through their own tests' bodies."""
    from planer_amd import q4
    from tests import test_gpu_conv1x1_wino as C1
    from tests import test_gpu_wf4 as WF
    from tests import test_gpu_wino43 as W43
    from tests import test_gpu_wino_chain as WC
    n, cin, h, w, cout = shape
    tail = ("b", "bn", "leaky", "res", "after")
    host = WC._operands(pa, np.random.default_rng(sum(shape)), n, cin, h, w, cout, tail)[0]
    want = WC._oracle(host, tail)

    def body():
        dev = {key: (None if v is None else pa.asarray(v)) for key, v in host.items()}
        xq, rq = q4.to_q4(dev["x"]), q4.to_q4(dev["res"])
        for lay, prep in ((4, q4.prepare_winograd_q4_weights), (8, q4.prepare_w1d4_q4_weights)):
            y = q4.ConvQ4(xq, prep(dev["k"]), dev["b"], dev["scale"], dev["shift"], rq, pads=(1, 1, 1, 1), act=WC._act(tail), alpha=0.1,
                          w_layout=lay)
            assert_close(q4.from_q4(y).get(), want, RTOL, "w_layout %d %s [%s]" % (lay, shape, pa.hip.context().last_conv_plan()))
        WC.test_stages_equal_the_one_call_pipeline_bit_for_bit(pa, shape, "2", monkeypatch)
        WC.test_chained_pair_equals_two_one_call_convs_bit_for_bit(pa, shape)
        WF.test_fused_f4x4_conv_vs_oracle(pa, shape, "1", monkeypatch)
        if h in (7, 14) and w in (7, 14):
            W43.test_mixed_tile_conv_matches_oracle_and_its_stages(pa, shape)
            W43.test_mixed_tile_chain_equals_two_convs_bit_for_bit(pa, shape)
        C1.test_conv1x1_wino_in_matches_conv_then_transform(pa, shape, "bn+leaky")

    sweep("winograd", body, "winograd %s" % (shape,))


# ---- the other special kernels --------------------------------------------------------------------------------------------
def test_stem_maxpool_every_block_count(pa):
    """Stem + max-pool, w_layout 12 (NB = 1 .. 7 pixel blocks, two and three chunks a row) and 10, odd heights, bit for bit."""
    from planer_amd import q4
    from tests import ref64 as R
    from tests import test_gpu_stem_kpack as S
    from tests.test_gpu_conv_exact import _case, _dev, _exact
    tails = [(False, True, False, R.ACT_RELU), (True, False, False, R.ACT_NONE), (True, True, False, R.ACT_LEAKY)]
    cases = []
    for i, (w, nb) in enumerate(S.WIDTHS):
        n, h, cout = (2, 37, 12) if i % 2 else (1, 29, 36)
        ops, act, want = _case("hygiene-stem", (n, 3, h, w), (cout, 3, 7, 7), tails[i % 3], **S.CONV)
        cases.append((ops, act, onp.maxpool(want.astype(np.float32), **S.POOL), nb, (n, h, w, cout)))

    def body():
        for (x, K, B, sc, sh, _), act, want, nb, what in cases:
            y, plan, ext = S._run(pa, x, K, B, sc, sh, act, R.ALPHA, 0)
            assert " x %dpx," % (16 * nb) in plan and ext[3] == 148, (plan, ext)
            _exact(y, want, "stem nchw %s" % (what,), plan)
            y = q4.ConvPoolQ4(_dev(pa, x), q4.prepare_rowpack_weights(_dev(pa, K)), _dev(pa, B), _dev(pa, sc), _dev(pa, sh), act=act,
                              alpha=R.ALPHA, **S.CONV)
            plan = pa.hip.context().last_conv_plan()
            assert plan.startswith("stem+maxpool "), plan
            _exact(q4.from_q4(y).get(), want, "stem rowpacked %s" % (what,), plan)

    sweep("special", body, "stem + max-pool")


def test_rowpack_and_small_cin(pa, monkeypatch):
    from tests import test_gpu_conv_exact as CE

    def body():
        CE.test_rowpack_every_tail(pa)
        CE.test_small_cin_mfma_and_valu_kernels(pa, monkeypatch)

    sweep("special", body, "rowpack / small Cin")


def _dw_cases():
    from tests import test_gpu_depthwise as D
    return [c for c in D.CASES if c[4] in (6, 10)]


@pytest.mark.parametrize("i", range(6))
def test_depthwise_partial_quad(pa, i):
    """C = 6 and 10: the last channel quad is half full, NCHW and Q4 (w_layout 13)."""
    from tests import test_gpu_depthwise as D
    cases = _dw_cases()
    assert len(cases) >= 6 and any(c[4] == 6 for c in cases)
    case = cases[i * len(cases) // 6]
    sweep("special", lambda: D.test_depthwise_nchw_and_q4_match_the_oracle(pa, case), "depthwise %s" % (case[:8],))


def _convt_chunks():
    """Chunks of test_gpu_convtranspose's geometry sweep that hold a stride-2 and a stride-3 geometry with output_padding."""
    from tests import test_gpu_convtranspose as T
    picked = []
    for stride in (2, 3):
        for gi in range(0, len(T.GEOMS), 8):
            if gi not in picked and any(stride in s and max(op) > 0 for _, s, _, op in T.GEOMS[gi:gi + 8]):
                picked.append(gi)
                break
    return picked


def test_convtranspose_by_phase(pa):
    from tests import test_gpu_convtranspose as T
    chunks = _convt_chunks()
    assert len(chunks) == 2, chunks

    def body():
        for gi in chunks:
            T.test_geometry_sweep_exact_both_entries_every_tail(pa, gi)
        for ci, co in ((5, 5), (13, 1), (3, 8)):
            T.test_channels_exact_k3_and_k2(pa, ci, co)

    sweep("special", body, "convtranspose")


@pytest.mark.parametrize("case", [(2, 8, 9, 11, 12, 2), (1, 6, 7, 7, 5, 3)], ids=["2x8x9x11x12s2", "1x6x7x7x5s3"])
def test_sibling_pair(pa, case):
    from tests import test_gpu_pair as P
    sweep("special", lambda: P.test_pair_equals_the_two_convs(pa, case), "pair %s" % (case,))


def test_reductions_softmax_instancenorm_resize(pa):
    """GAP (NCHW and Q4, C % 4 != 0), softmax, instance norm, linear upsample and fractional resize on rows of 1 .. 65537."""
    from tests import test_gpu_ops_bounds as O

    def body():
        O.test_gap_past_grid_cap_and_partial_quads(pa)
        O.test_softmax(pa, 0)
        O.test_instancenorm(pa, 50.0)
        O.test_upsample_linear_and_resize(pa, 0.0)

    sweep("special", body, "reductions / softmax / instance norm / resize")


def test_tile_blend_transpose_and_copies(pa, golden_layers):
    """util.tile's blend buffers (tile_accumulate / tile_normalise, HWC resize), transposes and the 2-D copies of concat / pad /
    slice / tile on the reference's odd-sized vectors."""
    from tests import test_gpu_layers as L
    from tests import test_tile as T
    golden = np.load(T.os.path.join(T.ROOT, "tests", "golden", "tile.npz"))
    names = ["transpose_0231", "transpose_10", "concat_axis1", "concat_axis0_3", "pad_hw", "pad_reflect_hw", "slice_step_neg", "tile_2d",
             "expand_channel", "split_axis1", "resize_linear_frac", "add_bcast_channel"]

    def body():
        for case in T.CASES[:2]:
            T.test_device_tile_matches_reference(case, False, golden)
        T.test_device_tile_matches_reference(T.CASES[-1], True, golden)
        T.test_device_resize_matches_oracle()
        for name in names:
            L.test_copy_and_compare_ops_are_bit_exact(pa, name, golden_layers)

    sweep("special", body, "tile / transpose / copies")


# ---- index and selection operators: outputs and scratch whose size depends on the data ------------------------------------
def test_index_ops_at_their_boundaries(pa):
    """A kept subset of tests/test_gpu_index_ops.py, one case per family, each across its boundary: TopK at n = 8193
    (128 KiB of LDS; every data class, ties among them) and at n = 16385 (selection rounds, k = 1, 7, 300), NonZero at 2C + 5 with
    density 0.5 (the scan's carry; scratch of 2050 counts, an output sized by the count), the 70 000-update ScatterND, Gather past
    the grid, Where at 1 048 579 and Cast at 1 200 003 elements, one comparison and Erf."""
    from tests import ref_index as R
    from tests import test_gpu_index_ops as I
    size = 2 * R.NZ_CHUNK + 5
    nz = R.nonzero_input(R.nonzero_mask("half", size), np.float32)

    def body():
        I.test_topk_every_data_class(pa, 8193)
        I.test_topk_every_data_class(pa, 16385)
        I._nonzero_check(pa, nz, "half float32 %d" % size)
        I.test_scatternd_rows_last_write_wins(pa, 5, 70000)
        I.test_gather_past_the_grid(pa)
        I.test_where_passes_every_bit_pattern(pa, "random")
        I.test_cast_every_pair(pa, "float32", "int64")
        I.test_cast_every_pair(pa, "int64", "float32")
        I.test_compare_sizes_and_single_value_operands(pa, "greater", np.greater)
        I.test_erf_table_boundaries_and_clobbered_input(pa)

    sweep("index ops", body)
    assert {"pl_topk_f32", "pl_nonzero_count", "pl_nonzero_write", "pl_scatter_rows_f32", "pl_gather_f32", "pl_where_f32", "pl_cast",
            "pl_compare_f32", "pl_erf_lut_f32"} <= REACHED["entries"], sorted(REACHED["entries"])


# ---- whole programs, eagerly: the float64 step audit of tests/test_gpu_plan_audit.py with guards and poison ----------------
@pytest.fixture
def _plan_switches(monkeypatch):
    from tests.test_conv_layouts import SWITCHES
    for k in SWITCHES + ("PLANER_HIP_CONV_ALGO", "PLANER_HIP_STREAMS", "PLANER_HIP_Q4"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("seed", range(20))
def test_random_nets_audited(pa, seed, _plan_switches):
    from tests import test_gpu_plan_audit as A
    from tests.random_nets import random_net
    g, b, xs = random_net(40000 + seed)

    def body():
        A.run_audit(pa, g, b, xs[0], "random %d" % seed, graph=False)
        A.run_audit(pa, g, b, xs[1], "random %d q4 forced" % seed, q4="force", graph=False)

    sweep("programs", body, "random net %d" % seed)


@pytest.mark.parametrize("seed", range(0, 24, 3))
def test_real_scale_random_nets_audited(pa, seed, monkeypatch, _plan_switches):
    from tests import test_gpu_plan_audit as A
    from tests.random_nets import random_net_real
    g, b, xs = random_net_real(seed)

    def body():
        A.run_audit(pa, g, b, xs[0], "real %d" % seed, graph=False)
        for algo in A.FORCED:
            monkeypatch.setenv("PLANER_HIP_CONV_ALGO", str(algo))
            try:
                A.run_audit(pa, g, b, xs[0], "real %d algo %d" % (seed, algo), graph=False)
            except ValueError as e:
                if "does not apply" not in str(e):
                    raise
            finally:
                monkeypatch.delenv("PLANER_HIP_CONV_ALGO")

    sweep("programs", body, "real-scale random net %d" % seed)


# ---- plan files: pl_plan_build's eager pass on a zeroed and on a poisoned arena --------------------------------------------
@pytest.mark.parametrize("name", ["resnet18", "yolov3", "customnet"])
def test_plan_files_do_not_rely_on_the_zeroed_arena(name):
    """pl_plan_build + pl_plan_run (ctypes only, tests/test_gpu_plan_file._run_plan) with the mode off -- the arena cleared to
    zero, as shipped -- and under each poison: guards clean, outputs bit-identical in all three."""
    import planer_amd
    from planer_amd import hip
    from planer_amd.export import export_plan
    from planer_amd.irgen import customnet, resnet18, yolov3
    from tests import test_gpu_plan_file as PF
    mod, x = {"resnet18": (resnet18, resnet18.make_input(2)), "yolov3": (yolov3, yolov3.make_input(1, size=160)),
              "customnet": (customnet, customnet.make_input(2))}[name]
    g, b = mod.build()
    net = planer_amd.from_graph(g, b)
    blob = export_plan(net, x)
    del net
    lib = PF._bind()
    stat = STATS.setdefault("plan files", [0.0, 0.0, 0])
    outs = {}
    for poison in (None,) + POISONS:
        t0 = time.perf_counter()
        outs[poison] = PF._run_plan(lib, blob, [x], hygiene=None if poison is None else (hip.POOL_GUARD_BYTES, poison))
        stat[0 if poison is None else 1] += time.perf_counter() - t0
    for poison in POISONS:
        _identical(outs[None], outs[poison], "%s plan file, zeroed arena vs poison %#x" % (name, poison))


# ---- what the sweep reached -----------------------------------------------------------------------------------------------
def test_zz_coverage_and_times(pa):
    """Runs last (file order): needs the whole module to have run."""
    for group, (off, on, peak) in sorted(STATS.items()):
        print("%-16s mode off %6.1f s   mode on (two poisons) %6.1f s   peak pool %7.1f MiB" % (group, off, on, peak / 2.0 ** 20))
    lay, plans, entries = REACHED["layouts"], REACHED["plans"], REACHED["entries"]
    print("w_layouts under the mode: %s" % sorted(lay))
    assert {2, 4, 6, 7, 8, 9, 11, 13, 14} <= lay and {10, 12} & lay, sorted(lay)
    assert any(re.search(r"split=([2-9]|\d\d)", p) for p in plans), "no split-K plan ran under the mode"
    dense = REACHED["dense"]
    assert any(p.startswith("dense32x32") for p in dense), "the small-batch dense kernel did not run under the mode"
    assert any(not p.startswith("dense32x32") for p in dense), "the generic dense path did not run under the mode"
    assert {"pl_wino4_chain_q4_f32", "pl_wino43_chain_q4_f32", "pl_conv1x1_wino_in_q4_f32"} <= entries, sorted(entries)

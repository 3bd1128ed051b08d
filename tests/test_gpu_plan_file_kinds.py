"""Plan files for every net kind: export_plan -> pl_plan_build / pl_plan_run (ctypes only, tests/test_gpu_plan_file._run_plan)
against the live net, bit for bit.  A plan file is the same calls in the same order, so nothing here has a tolerance.

  A  the ten generator nets of tests/plan_programs.NETS at 64 px and batch 2, crnn (fused LSTM steps at H = 8, the per-step
     program at H = 12), cellnet and posenet, under PICKS["first"] and PICKS["last"] in place of the conv timing: live net(x) ==
     three replays == a run from the caller's pointers, a second batch on the same built plan == net(x2), and the recorded
     block life times put no two live blocks on one byte (tests/test_plan_file_arena.check_placement on the real event list).
  B  24 graphs of tests/random_nets.random_net, seeds 40000 .. 40023, layouts forced (the maps are tiny): the same comparison.
     Each seed's program is walked on the host first (plan_audit.cpu_front): no step of the nonzero class in any of them (0 of
     24), so none may refuse.  Three graphs of random_net_q4ops, three plain NCHW programs and a mixed-tile Winograd chain add
     the kinds those do not hold.
  C  output heads declared on head_kit.tiny_net, a uint8 image input, and the refusals.
  D  every kind with trait W of plan.KINDS fed by the graph input, directly and through a view: the plan's input is written
     once and must survive three runs.
  F  what the files reached.

Both sides run with the launch-plan tuner off (PLANER_HIP_AUTOTUNE=0, no shipped database: the static heuristic): a plan file
holds calls, not launch plans, and a host that tunes for itself may split K otherwise than the recording net did.  The live
nets run on a context of their own, made under those switches.

Findings (what these tests exposed, and what became of it):
  * export_plan ignored Net.image_output / label_output / object_output / keypoint_output / flow_output / text_output /
    detection_output: the file of a net with a declared head returned the float tensor.  Every encoder is a chain of device
    calls with tables of a DECLARED size (max_objects, max_peaks, max_det ...; counts stay on the device), so none needs the
    host: export_plan now records Net._hand_back behind the pass, and the file returns the head's arrays at their dtypes.
  * export_plan took a uint8 batch of a Net.image_input net for the tensor itself.  The decode kernel is now the file's first
    call and the plan's input is the uint8 batch (dtype code 3).
  * export_plan's private list of in-place kinds lacked clip, erf and the norms (plan.KINDS has them), and no list followed a
    view: x -> reshape -> erf rewrote the recorded input block.  The kinds now come from plan._IN_PLACE, and what they rewrite
    is read off the pointers of the warm pass, so a view of the input counts whatever made it.
  * _run_plan read every output as float32 and refused a non-float input; it now honours the records' dtype codes, and checks
    that a run leaves the caller's input buffers as they were.
  Not real: LSTM initial states are read, never written (pl_lstm_seq_f32 writes a cell block of its own); the life times of
  Q4 copies and views held on every net here.  A net with net.streams > 1 exports: the recorded pass is the one-context
  program whatever the live net fans out to; the "another context" refusal is reached by a call on a side context only.
"""
import contextlib
import ctypes
import struct
import time

import numpy as np
import pytest

from tests import head_kit as K
from tests import plan_programs as PP
from tests.test_gpu_plan_file import _bind, _run_plan
from tests.test_plan_file_arena import check_placement

pytestmark = pytest.mark.gpu

F32 = np.float32
REACHED = {"live": set(), "file": set(), "kinds": set(), "refused": set(), "secs": {}, "largest": (0, ""), "nets": set()}
EXTRA = ("crnn", "crnn_h12", "cellnet", "posenet")
RANDOM_SEEDS = range(40000, 40024)


@pytest.fixture(scope="module")
def quiet():
    """-> a context of its own for the live nets, made with the launch-plan tuner off, as every ctypes context of the module is."""
    from planer_amd import hip
    mp = pytest.MonkeyPatch()
    mp.setenv("PLANER_HIP_AUTOTUNE", "0")
    mp.setenv("PLANER_HIP_TUNED", "0")
    try:
        yield hip.Context(hip.context().device)          # (left to the process: arrays of dropped nets still name it)
    finally:
        mp.undo()


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def calls_of(blob):
    """The entry-point names of a plan file's call records, in order (the layout csrc/plan_exec.hip documents)."""
    assert blob[:8] == b"PLPLAN1\0"
    _, _, n_in, n_out, ncalls, _ = struct.unpack_from("<QQIIII", blob, 8)
    p, names = 40 + (n_in + n_out) * 56, []
    for _ in range(ncalls):
        n, = struct.unpack_from("<I", blob, p)
        names.append(blob[p + 4:p + 4 + n].decode())
        p += 4 + n + (-n) % 4
        nargs, = struct.unpack_from("<I", blob, p)
        p += 4
        for _ in range(nargs):
            kind, _, payload = struct.unpack_from("<IIQ", blob, p)
            p += 16 + ((payload + 7) // 8 * 8 if kind == 5 else 0)
    return names


def replayable(name):
    """A call the recorder keeps: not a query, not pool / event bookkeeping, not what it refuses."""
    from planer_amd import _lib, export
    sig = _lib.SIGNATURES.get(name)
    if not sig or sig[0] is not ctypes.c_void_p or name.endswith(export._QUERIES) or name in export._IGNORED:
        return False
    return name not in ("pl_alloc", "pl_h2d", "pl_d2h", "pl_sync") and not name.startswith(
        ("pl_ctx_", "pl_comm_", "pl_graph_", "pl_capture_", "pl_stream_", "pl_plan_", "pl_nonzero", "pl_tune_", "pl_pool_", "pl_event_"))


@contextlib.contextmanager
def noting_calls(into):
    from planer_amd import _lib
    call = _lib.call

    def call_and_note(name, *args):
        call(name, *args)
        into.add(name)
    _lib.call = call_and_note
    try:
        yield
    finally:
        _lib.call = call


@contextlib.contextmanager
def watching_place(into):
    """export._place as it is, its arguments and results kept."""
    from planer_amd import export
    place = export._place

    def place_and_keep(events, pinned):
        offsets, arena = place(events, pinned)
        into.append((list(events), set(pinned), dict(offsets), arena))
        return offsets, arena
    export._place = place_and_keep
    try:
        yield
    finally:
        export._place = place


def as_list(y):
    return [np.asarray(a) for a in (y if isinstance(y, (tuple, list)) else (y,))]


def hooks_are_off():
    from planer_amd import _lib, hip
    return _lib._recorder is None and hip._free_hook is None


def three_way(net, xs, xs2, what, live=True):
    """net(x) == three replays of its file == a run from the caller's pointers, and net(x2) == a run of x2 on the same plan.
    -> the file.  `live`: note the fused program's kinds and the calls of one eager pass of it for `test_what_the_files_reached`."""
    from planer_amd import hip
    from planer_amd.export import export_plan
    from tests.plan_audit import program
    t0 = time.perf_counter()
    want, want2 = as_list(net(*xs)), as_list(net(*xs2))
    if live:
        dev = [hip.asarray(x, ctx=net.ctx) for x in xs]
        prog, _ = program(net, dev)
        REACHED["kinds"].update(obj.name for obj in prog.objs.values())
        seen, work = set(), [d.copy() for d in dev]
        with noting_calls(seen):
            net._interpret(prog, work)
        del work
        net.ctx.synchronize()
        REACHED["live"].update(n for n in seen if replayable(n))
    placed = []
    with watching_place(placed):
        blob = export_plan(net, *xs)
    assert hooks_are_off() and len(placed) == 1
    events, pinned, offsets, arena = placed[0]
    check_placement(events, pinned, offsets, arena, what)
    names = tuple("output %d" % i for i in range(len(want)))
    lib, stats = _bind(), {}
    got, (got2,) = _run_plan(lib, blob, xs, then=[xs2], stats=stats)
    assert stats["arena"] == arena and stats["calls"] == len(calls_of(blob))
    K.same(got, want, names, what + ": plan file")
    K.same(got2, want2, names, what + ": second batch on the same plan")
    K.same(_run_plan(lib, blob, xs, through_pointers=True), want, names, what + ": from the caller's pointers")
    REACHED["file"].update(calls_of(blob))
    REACHED["secs"][what] = time.perf_counter() - t0
    REACHED["largest"] = max(REACHED["largest"], (len(blob), what))
    return blob


def install(net, pick):
    """PICKS[pick] in place of the conv timing, installed where plan_programs.net_record installs it, but not the same pick: every
    candidate but the first is launched once on operands of the step's shape, and PICKS[pick] chooses among those whose kernel
    took it -- "last" is the last candidate that RUNS.  Net._pick_conv_algo's own loop skips a candidate that answers
    NotImplementedError in the same way (the fused F(4x4,3x3) kernel refuses these 64-px maps), and a program with such a step
    runs nowhere, live or from a file.  Nothing is timed."""
    from planer_amd import hip, q4
    from planer_amd.conv_layouts import LAYOUTS
    from planer_amd.layer import ConvFused
    runs = {}

    def takes(lay, K, xs, has, para, quad):
        key = (lay, quad, xs, tuple(K.shape), has, repr(sorted(para.items())))
        if key not in runs:
            rng = np.random.default_rng(1234)
            x = hip.asarray(rng.standard_normal(xs).astype(F32), ctx=net.ctx)
            cout = K.shape[0]
            chan = hip.asarray(rng.uniform(0.5, 1.5, (1, cout, 1, 1)).astype(F32), ctx=net.ctx)
            res = hip.asarray(rng.standard_normal((xs[0], cout, xs[2], xs[3])).astype(F32), ctx=net.ctx) if has[3] else None
            if quad:
                x, res = q4.to_q4(x), (q4.to_q4(res) if res is not None else None)
            args = [hip.zeros((cout,), F32, net.ctx) if has[0] else None, chan if has[1] else None, chan if has[2] else None, res]
            try:
                (q4.ConvQ4 if quad else ConvFused)(x, LAYOUTS[lay].prepare(K), *args, w_layout=lay,
                                                   **{k: v for k, v in para.items() if k != "w_layout"})
                runs[key] = True
            except (NotImplementedError, ValueError):
                runs[key] = False
        return runs[key]

    def choose(cands, K, srcs, para, shapes, q4=False):
        xs = tuple(shapes[srcs[0].split("@")[0]])
        has = tuple(i < len(srcs) and srcs[i] != "None" for i in range(2, 6))
        ok = [lay for lay in cands if len(cands) == 1 or lay == cands[0] or takes(lay, K, xs, has, para, q4)]
        return PP.PICKS[pick](ok)
    net._pick_conv_algo = choose
    return net


def second(x, seed=99):
    """Another batch of x's shape and dtype."""
    r = np.random.default_rng(seed)
    return r.integers(0, 256, x.shape).astype(np.uint8) if x.dtype == np.uint8 else r.standard_normal(x.shape).astype(x.dtype)


def load(name):
    """-> (graph, blob, x) of a net of A at batch 2 and its smallest legal input."""
    from planer_amd.irgen import cellnet, crnn, posenet
    if name in PP.NETS:
        return PP.load(name, batch=2)
    if name.startswith("crnn"):
        # height 8, width 16: T = 4 frames behind the two 2 x 2 pools; H = 8 is the smallest the fused rule takes
        # (layer.lstm_fused_eligible), H = 12 is refused by it and records the per-step program
        g, b = crnn.build(classes=5, height=8, hidden=12 if name.endswith("h12") else 8, batch=2)
        return g, b, crnn.make_input(2, size=(8, 16))
    mod = {"cellnet": cellnet, "posenet": posenet}[name]
    g, b = mod.build()
    return g, b, mod.make_input(2, size=64 if name == "cellnet" else (64, 64))


# ---- A. the generator nets ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pick", ["first", "last"])
@pytest.mark.parametrize("name", list(PP.NETS) + list(EXTRA))
def test_generator_net_replays_bit_for_bit(quiet, name, pick):
    """drn also folds its dilated convs (net.fold_dilated = "force": the folds and refolds are plan kinds like any other).  No
    candidate is forced away: the split-K plans of these kernels reduce slabs in a fixed order (test_gpu_layers.
    test_hybrid_split_k_plans_are_deterministic), and with the tuner off both sides take the same one."""
    import planer_amd
    from planer_amd.layer import lstm_fused_eligible
    g, b, x = load(name)
    net = install(planer_amd.from_graph(g, b, ctx=quiet), pick)
    if name == "drn":
        net.fold_dilated = "force"
    REACHED["nets"].add(name)                             # (the census wants every case of A to have RUN; a failure is this case's)
    blob = three_way(net, [x], [second(x)], "%s/%s" % (name, pick))
    if name.startswith("crnn"):
        fused = lstm_fused_eligible(4, 2, 12 if name.endswith("h12") else 8, 2)
        assert fused == (not name.endswith("h12"))
        assert (b"pl_lstm_seq_f32" in blob) == fused and (b"pl_lstm_cell_f32" in blob) == (not fused)
    planer_amd.hip.trim_side_contexts()


# ---- B. random programs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(RANDOM_SEEDS))
def test_random_program_replays_bit_for_bit(quiet, seed):
    """Shared tensors, in-place ReLU on forked values, several outputs, the Q4 pointwise kinds (net.use_q4 = "force", as
    plan_programs.stage_digests forces layouts).  None of the 24 may refuse: see the module docstring."""
    import planer_amd
    from tests.random_nets import random_net
    from tests.plan_audit import cpu_front
    g, b, xs = random_net(seed)
    body, _, _, _ = cpu_front(g, b, xs[0], force=True)            # the walk on the host: no step of the nonzero class
    assert not [step for step in body if step[1] in ("nonzero", "topk", "where", "gather", "scatternd")]
    net = install(planer_amd.from_graph(g, b, ctx=quiet), "last" if seed % 2 else "first")
    net.use_q4 = "force"
    three_way(net, [xs[0]], [xs[1]], "random %d" % seed)
    planer_amd.hip.trim_side_contexts()


# the kinds the nets of A and B do not hold, forced: linear and nearest resizes in Q4 and NCHW, the fused add behind one, an NCHW
# pixel shuffle (tests/random_nets.random_net_q4ops, seeds chosen on the host by the kinds tests.plan_audit.cpu_program gives)
@pytest.mark.parametrize("seed", [10, 24, 29])
def test_q4ops_program_replays_bit_for_bit(quiet, seed):
    import planer_amd
    from tests.random_nets import random_net_q4ops
    g, b, xs = random_net_q4ops(seed)
    net = install(planer_amd.from_graph(g, b, ctx=quiet), "first")
    net.use_q4 = "force"
    three_way(net, [xs[0]], [second(xs[0])], "q4ops %d" % seed)
    want = {10: {"resize_q4", "resize_add_q4"}, 24: {"resize", "resize_q4", "resize_add_q4"}, 29: {"pixelshuffle"}}[seed]
    assert want <= REACHED["kinds"], sorted(want - REACHED["kinds"])
    planer_amd.hip.trim_side_contexts()


@pytest.mark.parametrize("name, fuse", [("unet", False), ("yolov3", False), ("edsr", True)])
def test_nchw_program_replays_bit_for_bit(quiet, name, fuse):
    """The plain NCHW programs (net.use_q4 = False; `fuse` False: no conv epilogues either): conv, batchnorm, leakyrelu and the
    NCHW transposed conv as steps of their own, edsr's pixel shuffle as reshape / transpose / reshape."""
    import planer_amd
    g, b, x = load(name)
    net = install(planer_amd.from_graph(g, b, ctx=quiet), "first")
    net.use_q4, net.use_fusion = False, fuse
    three_way(net, [x], [second(x)], "%s nchw%s" % (name, "" if fuse else " unfused"))
    want = {"unet": {"conv", "batchnorm", "convt_fused"}, "yolov3": {"leakyrelu", "batchnorm"}, "edsr": {"transpose", "reshape"}}[name]
    assert want <= REACHED["kinds"], sorted(want - REACHED["kinds"])
    planer_amd.hip.trim_side_contexts()


def test_mixed_tile_winograd_stages_replay_bit_for_bit(quiet):
    """Three 3x3 convs 128 -> 128 on 21-pixel maps at batch 8, where conv_layouts.candidates offers the mixed-tile F(4,3) layout
    last: its input transform, GEMM, chain and output stages from a file."""
    import planer_amd
    from planer_amd.irgen.builder import GraphBuilder
    r = np.random.default_rng(3)
    g = GraphBuilder(["x"])
    src = "x"
    for i in range(3):
        g.init("K%d" % i, (r.standard_normal((128, 128, 3, 3)) * 0.03).astype(F32))
        src = g.op("relu", g.op("conv", [src, "K%d" % i], "c%d" % i, name="conv%d" % i, group=1, strides=[1, 1], dilations=[1, 1],
                                pads=[1, 1, 1, 1]), "r%d" % i, name="relu%d" % i)
    graph, b = g.finish([src])
    x = r.standard_normal((8, 128, 21, 21)).astype(F32)
    net = install(planer_amd.from_graph(graph, b, ctx=quiet), "last")
    net.use_q4 = "force"
    three_way(net, [x], [second(x)], "wino43 stages")
    want = {"wino43_in", "wino43_gemm", "wino43_out", "wino43_chain"}
    assert want <= REACHED["kinds"], sorted(want - REACHED["kinds"])
    planer_amd.hip.trim_side_contexts()


# ---- C. heads and refusals --------------------------------------------------------------------------------------------------------
# Every head's encoder (planer_amd/util.py: *Spec.encode) allocates tables of a declared size and makes device calls only --
# "nothing waits for the host" -- so every head EXPORTS; none is a refusal.  (declaration, outputs of tiny_net, arrays back)
HEADS = {
    "image": (lambda n: n.image_output([1.0], [8.0]), ["s"], 1),
    "label": (lambda n: n.label_output(), ["s"], 1),
    "objects": (lambda n: n.object_output(max_objects=16), ["s"], 4),
    "keypoints": (lambda n: n.keypoint_output(max_peaks=8), ["s"], 2),
    "instances": (lambda n: n.flow_output(rounds=4, min_size=2, max_instances=16), ["s"], 4),
    "text": (lambda n: n.text_output("nchw", max_len=8), ["s"], 4),
    "detections": (lambda n: n.detection_output([([(4, 4)], 1.0)], 3, conf=0.0, max_det=16), ["f"], 2),
    "dfl": (lambda n: n.detection_output([("dfl", 1.0, 1)], 4, conf=0.0, max_det=16), ["f"], 2),
    # DFL detections with masks: a prototype tensor has 4 planes at least, so the tiny net's twin with a 12-plane head (4 bins,
    # 4 classes, 4 coefficients) and 4 prototype planes: det, num, masks (uint8)
    "dfl+masks": (lambda n: n.detection_output([("dfl", 1.0, 1)], 4, conf=0.0, max_det=16, size=(32, 32), protos=1), ["f", "p"], 3),
}


def proto_net(outputs, seed=4):
    """head_kit.tiny_net's twin for a head with prototype masks: x (N, 3, 32, 32) -> conv 3x3 (12) + relu = f -> conv 3x3 (4) = p,
    small-integer filters and biases like it."""
    from planer_amd.irgen.builder import GraphBuilder
    rng = np.random.default_rng(seed)
    g = GraphBuilder(["x"])
    g.init("K0", rng.integers(-2, 3, (12, 3, 3, 3)).astype(F32))
    g.init("B0", rng.integers(-3, 4, 12).astype(F32))
    g.op("conv", ["x", "K0", "B0"], "c0", name="conv0", group=1, strides=[1, 1], dilations=[1, 1], pads=[1, 1, 1, 1])
    g.op("relu", "c0", "f", name="relu0")
    g.init("K1", rng.integers(-2, 3, (4, 12, 3, 3)).astype(F32))
    g.init("B1", rng.integers(-3, 4, 4).astype(F32))
    g.op("conv", ["f", "K1", "B1"], "p", name="conv1", group=1, strides=[1, 1], dilations=[1, 1], pads=[1, 1, 1, 1])
    return g.finish(outputs)


@pytest.mark.parametrize("head", list(HEADS))
def test_declared_head_replays_with_its_dtypes(quiet, head):
    """The file of a net with a declared head returns the head's arrays, integer ones at their dtype, for two inputs."""
    import planer_amd
    declare, outputs, places = HEADS[head]
    g, b = proto_net(outputs) if "p" in outputs else K.tiny_net(outputs)
    net = install(planer_amd.from_graph(g, b, ctx=quiet), "first")
    declare(net)
    x = K.tiny_input()
    assert len(as_list(net(x))) == places
    blob = three_way(net, [x], [K.tiny_input(seed=8)], "head " + head, live=False)
    REACHED["heads"] = REACHED.get("heads", set()) | {head}
    assert len(calls_of(blob)) > 2
    if head == "dfl+masks":
        assert {"pl_dfl_decode_f32", "pl_nms_rows_f32", "pl_dfl_coefficients_f32", "pl_proto_masks_f32"} <= set(calls_of(blob))
    planer_amd.hip.trim_side_contexts()


def test_uint8_image_input_is_the_plans_input(quiet):
    """Net.image_input with a resize (the sampling tables are constants of the file) in front of the tiny net and a label output
    behind it: uint8 in, uint8 out."""
    import planer_amd
    g, b = K.tiny_net(["s"])
    net = planer_amd.from_graph(g, b, ctx=quiet)
    net.image_input(np.ones(3, F32), np.zeros(3, F32), size=(32, 32)).label_output()
    i = np.arange(2 * 24 * 20 * 3, dtype=np.int64)
    x = ((i * 37 + i // 192 * 53 + 11) % 256).astype(np.uint8).reshape(2, 24, 20, 3)
    blob = three_way(net, [x], [second(x)], "uint8 input", live=False)
    assert calls_of(blob)[0] == "pl_image_u8_nchw_f32" and calls_of(blob)[-1] == "pl_labels_f32_u8"
    planer_amd.hip.trim_side_contexts()


def _one_op(kind, outputs=("y",), **para):
    from planer_amd.irgen.builder import GraphBuilder
    g = GraphBuilder(["x"])
    g.op(kind, "x", "y", name=kind + "0", **para)
    return g.finish(list(outputs))


def refused(net, x, tmp_path, match):
    """export_plan refuses with `match` in the message, writes nothing, leaves the hooks off and the net as it answered before."""
    from planer_amd.export import export_plan
    before = as_list(net(x))
    path = tmp_path / "refused.plplan"
    with pytest.raises(NotImplementedError, match=match):
        export_plan(net, x, path=str(path))
    assert not path.exists() and hooks_are_off()
    K.same(as_list(net(x)), before, ["output %d" % i for i in range(len(before))], "after the refusal")


def test_a_nonzero_net_is_refused_by_name(quiet, tmp_path):
    import planer_amd
    g, b = _one_op("nonzero")
    net = planer_amd.from_graph(g, b, ctx=quiet)
    x = (np.arange(24).reshape(2, 3, 4) % 3).astype(F32)
    refused(net, x, tmp_path, "pl_nonzero|host value|pl_h2d|pl_d2h|pl_sync")
    REACHED["refused"].add("nonzero")


def test_a_result_that_is_a_view_is_refused(quiet, tmp_path):
    """A net that returns one of its inits beside a computed tensor: that result is a view into the block of the weights, a
    constant of the file and no arena block.  Nothing is written, the hooks are off again and the net answers as before.  (The
    other half of the message, a view of the middle of an arena block, no graph reaches: layer.Split and layer.Slice
    materialise their parts, and the LSTM copies the states it hands back.)"""
    import planer_amd
    from planer_amd.export import export_plan
    from planer_amd.irgen.builder import GraphBuilder
    g = GraphBuilder(["x"])
    g.init("c", np.arange(6, dtype=F32))
    g.op("relu", "x", "y", name="relu0")
    graph, b = g.finish(["y", "c"])
    net = planer_amd.from_graph(graph, b, ctx=quiet)
    path, x = tmp_path / "view.plplan", np.arange(-3, 3, dtype=F32).reshape(2, 3)
    before = as_list(net(x))
    with pytest.raises(NotImplementedError, match="a result that is a view of a constant"):
        export_plan(net, x, path=str(path))
    assert not path.exists() and hooks_are_off()
    K.same(as_list(net(x)), before, ("y", "c"), "after the refusal")


def test_a_call_on_another_context_is_refused_and_streams_do_not_matter(quiet):
    """The recorder refuses a call whose context is not the net's ("side streams are not exported"); a net with streams > 1 still
    exports, because export_plan records the one-context program: its file equals the fanned-out live net (integer data: every
    partial sum is exact, whichever kernels the sub-batches pick)."""
    import planer_amd
    from planer_amd import export, hip
    rec = export._Recorder(quiet)
    with pytest.raises(NotImplementedError, match="pl_memset runs on another context"):
        rec.on_call("pl_memset", (hip.context().handle, ctypes.c_void_p(256), 0, 4))
    assert rec.events == []
    g, b = K.tiny_net(["f", "s"])
    net = planer_amd.from_graph(g, b, ctx=quiet)
    net.streams = 2
    three_way(net, [K.tiny_input()], [K.tiny_input(seed=8)], "streams = 2", live=False)
    planer_amd.hip.trim_side_contexts()


# ---- D. in-place kinds on the graph input, constants the pass writes ----------------------------------------------------------------
def _w_kinds():
    from planer_amd import plan
    return [k for k, traits in plan.KINDS.items() if plan.W in traits]


# how a graph makes the input feed each W kind: the NCHW kinds read x itself ("direct") or x under another shape ("view": a
# reshape to the same extents, which layer.Reshape hands on as the same memory); a "_q4" form reads a conv's output -- to_q4
# stands between the input and any Q4 step, so no graph input feeds one -- which a second step reads too, so that the conv's
# epilogue does not absorb the relu
def _w_net(kind, how="direct"):
    from planer_amd.irgen.builder import GraphBuilder
    r = np.random.default_rng(5)
    g = GraphBuilder(["x"])
    c = 8
    base = kind[:-3] if kind.endswith("_q4") else kind
    src = "x"
    if kind.endswith("_q4"):
        g.init("K", (r.standard_normal((c, c, 3, 3)) * 0.2).astype(F32))
        src = g.op("conv", ["x", "K"], "c0", name="conv0", group=1, strides=[1, 1], dilations=[1, 1], pads=[1, 1, 1, 1])
    elif how == "view":
        g.init("shp", np.array([0, 0, 12, 12], np.int64))
        src = g.op("reshape", ["x", "shp"], "xv", name="reshape0")
    if base == "relu":
        y = g.op("relu", src, "y", name="relu0")
    elif base == "clip":
        y = g.op("clip", src, "y", name="clip0", min=-0.5, max=0.5)
    elif base == "erf":
        y = g.op("erf", src, "y", name="erf0")
    elif base == "instancenormalization":
        g.init("s", r.uniform(0.5, 1.5, c).astype(F32))
        g.init("t", (r.standard_normal(c) * 0.1).astype(F32))
        y = g.op("instancenormalization", [src, "s", "t"], "y", name="in0", epsilon=1e-5)
    elif base == "groupnorm":
        from tests.groupnorm_ref import five_steps

        class S:
            pass
        S.g = g
        y = five_steps(S, src, (1, c, 12, 12), 2, tag="gn", mid="4d", affine="both", lead=False, seed=3)
    else:
        raise AssertionError("plan.KINDS has a new in-place kind, %r: say here how a graph input feeds it" % kind)
    # a second step reads the result, so that the in-place step is not the program's last
    g.init("one", np.ones(1, F32))
    out = g.op("add", [y, "one"], "z", name="add0")
    # (y is NOT a result: layer.ReLU, Clip and InstanceNormalization hand x itself on, and a result that points into the input
    # makes export_plan copy the input by its other rule, whatever the in-place table says)
    outs = [out]
    if kind == "relu_q4":
        outs.append(g.op("leakyrelu", src, "w", name="leaky0", alpha=0.1))        # a second reader of the conv's output
    return g.finish(outs), r.standard_normal((2, c, 12, 12)).astype(F32)


def _w_cases():
    return [(k, "direct") for k in _w_kinds()] + [(k, "view") for k in _w_kinds() if not k.endswith("_q4") and k != "groupnorm"]


@pytest.mark.parametrize("kind, how", _w_cases())
def test_in_place_kind_on_the_graph_input_leaves_the_input_alone(quiet, kind, how):
    """Every kind with trait W of plan.KINDS (the table is iterated), fed by the input itself and by a view of it.  The fused
    program holds the kind.  The plan's own input buffer is written ONCE and the plan run three times with no further upload:
    every run equals the live net, so no run rewrote the recorded input block (a file whose pass works on the input block
    itself gives kind(kind(x)) on the second run).  Then the usual comparison, from pointers the caller owns too."""
    import planer_amd
    from planer_amd import hip
    from planer_amd.export import export_plan
    from tests.plan_audit import program
    (g, b), x = _w_net(kind, how)
    net = install(planer_amd.from_graph(g, b, ctx=quiet), "first")
    net.use_q4 = "force" if kind.endswith("_q4") else net.use_q4
    prog, _ = program(net, [hip.asarray(x, ctx=net.ctx)])
    held = [obj.name for obj in prog.objs.values()]
    assert kind in held and (how != "view" or "reshape" in held), held
    want = as_list(net(x))
    got = _run_plan(_bind(), export_plan(net, x), [x], write_once=True)
    K.same(got, want, ["output %d" % i for i in range(len(want))], "input -> %s (%s), the input written once" % (kind, how))
    three_way(net, [x], [second(x)], "input -> %s (%s)" % (kind, how))
    planer_amd.hip.trim_side_contexts()


def test_export_takes_its_in_place_kinds_from_the_plan_table():
    from planer_amd import export, plan
    assert export._IN_PLACE is plan._IN_PLACE
    assert not [name for name, v in vars(export).items()                    # and no other collection of kind names
                if isinstance(v, (tuple, list, set, frozenset)) and v is not plan._IN_PLACE and set(v) & set(plan.KINDS)]


@pytest.mark.parametrize("name", ["crnn", "lstm", "erf"])
def test_constants_are_not_written_by_the_pass(quiet, name):
    """Every pool block the file holds as a constant (export._Recorder.consts: weights, prepared filters, tables, LSTM initial
    states -- here not zero) has, after the recorded pass and after two more passes, the bytes it had BEFORE export's warm
    pass (its second pass, the first of the fused program): the file carries what the net was loaded with, not end-of-run
    state.  The copy from before is taken of every pool block a live DeviceArray of the context points into, when export._warm
    is entered; a constant that is not among them was made by the warm pass itself and fails the test.  Read with the pool's
    own queries (pl_pool_block, pl_d2h)."""
    import gc
    import planer_amd
    from planer_amd import _lib, export, hip
    from planer_amd.irgen.builder import GraphBuilder
    if name == "crnn":
        g, b, x = load("crnn")
        raw = np.array(b, copy=True)
        from tests.plan_audit import _offsets
        for (key, shape, dt), off in zip(g["inits"], _offsets(g["inits"])):          # initial states that are not zero
            if key.endswith(("_h0", "_c0")):
                n = int(np.prod(shape)) * 4
                raw[off:off + n] = (np.random.default_rng(len(key)).standard_normal(n // 4) * 0.5).astype(F32).view(np.uint8)
        b = raw
    elif name == "lstm":
        from tests.test_gpu_lstm_seq import _layer_operands
        T, N, D, H = 5, 3, 24, 64
        x, *w = _layer_operands(11, T, N, D, H, 2)
        gb = GraphBuilder(["x"])
        for key, a in zip(("W", "R", "B", "h0", "c0"), w):
            gb.init(key, a)
        gb.init("lens", np.zeros(N, np.int64))
        gb.op("lstm", ["x", "W", "R", "B", "lens", "h0", "c0"], ["Y", "Yh", "Yc"], name="lstm", hidden_size=H, direction="bidirectional")
        g, b = gb.finish(["Y", "Yh", "Yc"])
    else:
        (g, b), x = _w_net("erf")
    net = planer_amd.from_graph(g, b, ctx=quiet)
    kept, early = [], {}
    init, warm = export._Recorder.__init__, export._warm

    def init_and_keep(self, ctx):
        init(self, ctx)
        kept.append(self)

    def snapshot_and_warm(*args):
        quiet.synchronize()
        for o in gc.get_objects():
            if isinstance(o, hip.DeviceArray) and o.ctx is quiet:
                base, size = ctypes.c_void_p(), ctypes.c_size_t()
                ptr = getattr(o, "ptr", None)               # (an array under construction has none yet)
                if not ptr or _lib.load().pl_pool_block(quiet.handle, ctypes.c_void_p(ptr), ctypes.byref(base), ctypes.byref(size)):
                    continue                                # no memory of its own, or none of this pool's: not a block to copy
                if base.value not in early:
                    early[base.value] = np.empty(size.value, np.uint8)
                    _lib.call("pl_d2h", quiet.handle, early[base.value].ctypes.data, base.value, size.value)
        return warm(*args)
    export._Recorder.__init__, export._warm = init_and_keep, snapshot_and_warm
    try:
        blob = export.export_plan(net, x)
    finally:
        export._Recorder.__init__, export._warm = init, warm
    rec, = kept
    assert rec.const_order and hooks_are_off()

    def read():
        quiet.synchronize()
        out = []
        for base in rec.const_order:
            host = np.empty(rec.consts[base][1], np.uint8)
            _lib.call("pl_d2h", quiet.handle, host.ctypes.data, base, host.nbytes)
            out.append(host)
        return out
    before = read()
    for base, host in zip(rec.const_order, before):
        assert base in early, "constant block %#x (%d bytes) did not exist before the warm pass" % (base, host.size)
        assert np.array_equal(early[base], host), "a pass of export_plan wrote constant block %#x (%d bytes) of %s" % (base, host.size, name)
    # the file's constants are those bytes
    const_bytes, = struct.unpack_from("<Q", blob, 8)
    tail = np.frombuffer(blob[len(blob) - const_bytes:], np.uint8)
    pos = 0
    for base, host in zip(rec.const_order, before):
        assert np.array_equal(tail[pos:pos + host.size], host), "constant block %#x differs from the file's copy" % base
        pos += host.size + (-host.size) % export._ALIGN
    want = as_list(net(x))
    for rep in range(2):
        for i, (a, c) in enumerate(zip(before, read())):
            assert np.array_equal(a, c), "pass %d wrote constant block %d (%d bytes) of %s" % (rep, i, a.size, name)
        net(x)
    names = ["output %d" % i for i in range(len(want))]
    K.same(_run_plan(_bind(), blob, [x]), want, names, name + ": plan file")
    REACHED["file"].update(calls_of(blob))
    planer_amd.hip.trim_side_contexts()


# ---- F. what the files reached ---------------------------------------------------------------------------------------------------
# the kinds of plan.KINDS that no exported program of this module holds, each with its reason.  A kind that IS held may not be
# listed (the test fails), so a kind that stops appearing is noticed.
_WAVE2 = "second-wave operator: no net generator and no random program is made of it; its kernel has tests/test_gpu_ops_bounds.py"
NOT_IN_A_FILE = {
    "nonzero": "refused at export time: test_a_nonzero_net_is_refused_by_name",
    "batchnorm_q4": "a BatchNorm behind a conv is folded into it, and nothing else makes a Q4 tensor in front of one here",
    "convtranspose": "every ConvTranspose of these nets is taken by the phase-decomposed kernel (convt_fused, convt_q4)",
    "identity": "no generator writes one; layer.Identity launches nothing",
    "cast": _WAVE2, "const": _WAVE2, "constantofshape": _WAVE2, "div": _WAVE2, "equal": _WAVE2, "exp": _WAVE2, "expand": _WAVE2,
    "gather": _WAVE2, "greater": _WAVE2, "greaterorequal": _WAVE2, "hardsigmoid": _WAVE2, "log": _WAVE2, "logsoftmax": _WAVE2,
    "mul": _WAVE2, "pow": _WAVE2, "range": _WAVE2, "reciprocal": _WAVE2, "reducemax": _WAVE2, "reducemean": _WAVE2,
    "reducemin": _WAVE2, "reducesum": _WAVE2, "scatternd": _WAVE2, "shape": _WAVE2, "slice": _WAVE2, "softmax": _WAVE2,
    "split": _WAVE2, "sqrt": _WAVE2, "sub": _WAVE2, "tanh": _WAVE2, "tile": _WAVE2, "topk": _WAVE2, "unsqueeze": _WAVE2,
    "where": _WAVE2,
}


def test_what_the_files_reached(capsys):
    """(1) every entry point a live pass of this module called is in some replayed file; (2) every kind of plan.KINDS was in an
    exported program or is in NOT_IN_A_FILE with its reason, and none is both; (3) the census under -s: distinct thunks
    replayed, seconds per net, the largest file."""
    from planer_amd import plan
    assert REACHED["nets"] >= set(PP.NETS) | set(EXTRA), "the census counts what the cases of this module left in REACHED: run it with them (the whole module, one session), not alone or under -k"
    assert REACHED["live"] and REACHED["live"] <= REACHED["file"], sorted(REACHED["live"] - REACHED["file"])
    missing = sorted(set(plan.KINDS) - REACHED["kinds"])
    excused = set(NOT_IN_A_FILE)
    assert excused <= set(plan.KINDS)
    slowest = sorted(REACHED["secs"].items(), key=lambda kv: -kv[1])
    with capsys.disabled():
        print("\nplan files: %d distinct thunks replayed (%d names in live passes); largest file %d bytes (%s); slowest: %s"
              % (len(REACHED["file"]), len(REACHED["live"]), REACHED["largest"][0], REACHED["largest"][1],
                 ", ".join("%s %.1f s" % kv for kv in slowest[:6])))
        print("kinds in exported programs: %d of %d; not in any: %s" % (len(REACHED["kinds"] & set(plan.KINDS)), len(plan.KINDS), missing))
    assert REACHED["refused"] >= {"nonzero"}
    assert set(missing) == excused, (sorted(set(missing) - excused), sorted(excused - set(missing)))
    # the kinds these nets are made of: each family the issue names went through a recorded call
    for kind in ("conv_q4", "convt_q4", "instancenormalization_q4", "groupnorm_q4", "pad_q4", "upsample_add_q4", "pixelshuffle_q4",
                 "refold_q4", "lstm", "relu_q4", "to_q4", "from_q4", "dense", "conv_fused"):
        assert kind in REACHED["kinds"], kind

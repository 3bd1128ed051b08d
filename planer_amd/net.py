"""planer's graph executor (`Net`) on MI355X.

Public surface and IR semantics are the reference's (net.py:5-101):
`load_json(inputs, inits, body, flow)`, `load_weights(uint8 blob)`,
`forward`, `__call__` (dict or positional inputs, host ndarray in -> host
ndarray out, the `rst[0] if len(rst)==1` unwrapping), `run`, `timeit`,
`timer`, liveness-based freeing of intermediates, chained layers and
multi-output steps.

What is new underneath (MI355X-first, no counterpart in the reference):
  * weights live in ONE device allocation (256-byte aligned slots) so the
    multi-GPU weight exchange is a single RCCL broadcast;
  * `forward` enqueues one hand-written HIP kernel per layer on the context
    stream and never synchronises;
  * `__call__` on device-resident inputs runs a *compiled plan*: the flow is
    peephole-fused (conv -> batchnorm -> [add] -> [relu|leakyrelu] become one
    MFMA kernel with a fused epilogue), executed once to warm the memory
    pool, then captured into a hipGraph that is replayed with a single C call
    per forward pass.
"""
import os
import time

import numpy

from . import _lib
from . import hip
from .hip import DeviceArray
from . import q4 as _q4
from .conv_layouts import DIRECT_Q4, IGEMM_NCHW, LAYOUTS, STEM_POOL, STEM_POOL_NCHW, WINO4_Q4, WINO43_Q4, experiment, suffix
from .layer import layer_map, wrap
from .plan import compile_front, fuse_upsample_concat, lower
from .util import BlendGeometry, DetectionSpec, FlowSpec, ImageFeed, ImageOutSpec, ImageSpec, KeypointSpec, LabelSpec, ObjectSpec, TextSpec, WindowFeed, _Tiling
from .util import blend_windows as _blend_windows, resize as _resize

STEM_WINO_DEFAULT = 1      # whether the stem + max-pool step takes the F(4,4) form where it applies

_q4.register(layer_map)

_ALIGN = 256

# w_layout code -> what runs (for run reports; conv_layouts.LAYOUTS)
W_LAYOUT_NAMES = {code: lay.name for code, lay in LAYOUTS.items()}


def _as_list(v):
    return list(v) if isinstance(v, (list, tuple)) else [v]


class _Program:
    """A flow ready to interpret: layer objects, steps and last-use table."""

    def __init__(self, body, flow):
        self.objs = {name: wrap(layer_map[kind], kind)(**para) for name, kind, para in body}
        self.flow = flow
        self.life = {}
        for i, step in enumerate(flow):
            for k in _as_list(step[0]):
                self.life[k] = i                     # net.py:16-19


def prog_body(prog):
    return [(name, obj.name) for name, obj in prog.objs.items()]


def graph_tag_of(layers, flow, init_shapes):
    """crc32 over layer kinds and parameters, flow wiring and init shapes (Net.graph_tag)."""
    import json
    import zlib

    def plain(v):
        # numpy scalars / arrays print differently across numpy versions (np.float32(0.1) vs 0.1): hash plain Python values
        if isinstance(v, numpy.ndarray):
            return v.tolist()
        if isinstance(v, numpy.generic):
            return v.item()
        if isinstance(v, dict):
            return {str(k): plain(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [plain(x) for x in v]
        return v
    text = json.dumps(plain([layers, flow, [list(map(int, s)) for s in init_shapes]]), sort_keys=True, default=repr)
    return "%08x" % (zlib.crc32(text.encode()) & 0xffffffff)


def _feed_static(ctx, dst, a, always=False):
    """A new batch `a` (a device tensor) into a captured plan's static input `dst`, on `ctx`'s stream.  Where the plan's
    only reader of that input is the row-packed stem conv (Net._capture, `dst.packed`), the batch is re-laid straight
    into the packed image the graph reads -- that pass replaces the copy -- and the NCHW tensor is left alone.  Where that
    reader is the stem + max-pool kernel that takes NCHW itself (`dst.prefed`), the kernel runs HERE, from the caller's batch
    into the pooled tensor the captured pass starts from: no copy and no re-layout at all.
    A uint8 image batch (`ImageFeed`, Net.image_input) is decoded straight into `dst`; the feed-time part then runs from there."""
    if isinstance(a, ImageFeed):
        a.decode_into(dst.ptr, ctx)
        a, always = dst, False
    if dst.prefed is not None:
        if a.ptr % 16:                                   # (a view that starts off a 16-byte boundary: through the static tensor)
            _lib.call("pl_d2d", ctx.handle, dst.ptr, a.ptr, dst.nbytes)
            a = dst
        dst.prefed[0](a.ptr, ctx)
    elif dst.packed is not None:
        _q4.pack_rows(dst, src_ptr=a.ptr, ctx=ctx)
    elif always or a is not dst:
        _lib.call("pl_d2d", ctx.handle, dst.ptr, a.ptr, dst.nbytes)


class _Plan:
    """One captured forward pass for one input signature."""

    def __init__(self, inputs, outputs, graph, ctx, fused_steps):
        self.inputs, self.outputs, self.graph, self.ctx = inputs, outputs, graph, ctx
        self.fused_steps, self.ms, self.streams = fused_steps, None, "1x1"
        self.algos = []              # per conv step: kernel family + launch plan (filled by Net._capture)
        # bounded host run-ahead: launch k waits (on the host) for launch k - max_in_flight of this plan's stream.
        # A free-running loop otherwise queues every batch it is asked for at once; eight batches keep the GPU fed
        # for milliseconds, and tools that intercept dispatches (rocprofv3) crash with ~2000 of them outstanding.
        self.max_in_flight, self._ring = 8, []
        self._held = []              # per ring slot: what that launch's feed read (Net.submit), released with the slot
        self.host_in, self.fed = None, None      # Net.submit with host batches: this replica's own upload buffers + "feed has read them"
        self._fed = False            # a feed has run since the last launch (else launch() runs the feed-time part itself)

    def feed(self, xs):
        """Copy new inputs into the plan's static input buffers (on the plan's stream)."""
        for s, a in zip(self.inputs, xs):
            _feed_static(self.ctx, s, a)
        self._fed = True

    def launch(self, join=True, hold=None):
        """`hold`: objects the feed of THIS launch read on this plan's stream (the caller's input arrays).  They stay
        referenced until the host has seen a marker behind this launch complete: a block the caller drops right after
        submitting must not go back to its pool -- and be overwritten through another stream -- before the asynchronous
        feed has read it.
        A launch that no `feed` preceded takes what the caller wrote into `plan.inputs[i]` itself: where part of the pass
        runs at feed time (the stem + max-pool kernel in front of the captured graph, `DeviceArray.prefed`; the row-packed
        copy, `.packed`) that part runs here from the static tensor -- the graph alone would read the previous batch's
        pooled tensor (round-5 advisor)."""
        if not self._fed:
            for s in self.inputs:
                if s.prefed is not None or s.packed is not None:
                    _feed_static(self.ctx, s, s)
        self._fed = False
        _lib.call("pl_graph_launch", self.graph)
        if self.max_in_flight:
            if len(self._ring) >= self.max_in_flight:
                ev = self._ring.pop(0)
                ev.synchronize()
                self._held.pop(0)
            else:
                ev = hip.Event(self.ctx)
            self._ring.append(ev.record())
            self._held.append(hold)
        elif hold is not None:       # no ring to tie the references to: wait for the launch instead
            self.ctx.synchronize()

    def join(self):
        pass

    def __del__(self):
        try:
            self.outputs = self.inputs = None      # drop buffers before their graph
            if self.graph is not None:
                _lib.load().pl_graph_destroy(self.graph)
        except Exception:
            pass


class _NotSplittable(Exception):
    """An output does not carry the batch on axis 0, so sub-batch streams cannot be used."""


class _MultiPlan:
    """A forward pass fanned out over several streams: sub-batch i is its own captured graph on
    side stream i (kernels of different streams run concurrently and fill CUs that one small
    grid leaves idle); the net's own stream forks before and joins after."""

    def __init__(self, inputs, outputs, subs, ctx, fused_steps):
        self.inputs, self.outputs, self.subs, self.ctx = inputs, outputs, subs, ctx
        self.fused_steps, self.ms = fused_steps, None
        self.streams = "%dx%d" % (len(subs), len(subs))
        self.algos = subs[0].algos

    def feed(self, xs):
        """Per-stream input copy: stream i copies ITS rows, ordered behind its own previous
        sub-graph, so consecutive forward passes may overlap across streams without a join."""
        n = self.inputs[0].shape[0] // len(self.subs)
        for i, sp in enumerate(self.subs):
            for dst, a in zip(sp.inputs, xs):
                _feed_static(sp.ctx, dst, a.rows(i * n, (i + 1) * n), always=True)
            sp._fed = True

    def launch(self, join=True):
        """join=True: fork from / join into the net's own stream (what Net.__call__ needs: inputs
        written and outputs read on the main stream).  join=False: throughput mode -- the streams
        free-run and pipeline across passes; call join() before reading outputs."""
        if join:
            for c in {id(sp.ctx): sp.ctx for sp in self.subs}.values():
                c.wait_for(self.ctx)           # fork FIRST: inputs were written on the main stream
        for sp in sorted(self.subs, key=lambda q: q.ctx is self.ctx):   # main-stream graphs last
            sp.launch()
        if join:
            self.join()

    def join(self):
        """Gather every sub-batch's outputs into the full output (on its own stream, outside the
        graphs: memcpy nodes inside the sub-graphs serialised the streams), then join."""
        for sp, rows in zip(self.subs, self.out_rows):
            outs = sp.outputs if isinstance(sp.outputs, tuple) else (sp.outputs,)
            for o, d in zip(outs, rows):
                _lib.call("pl_d2d", sp.ctx.handle, d.ptr, o.ptr, o.nbytes)
        for c in {id(sp.ctx): sp.ctx for sp in self.subs}.values():
            self.ctx.wait_for(c)


class _PipelinePlan:
    """Throughput mode only: R full-batch graphs ("replicas"), each on its own stream, used round
    robin -- consecutive forward passes run on different streams, so one batch's kernel tails,
    launch ramps and small kernels hide under the next batch's convs while every kernel keeps the
    full batch (better tile efficiency than sub-batch graphs).  `outputs` are those of the replica
    launched last; a replica's buffers are rewritten R launches later."""

    def __init__(self, replicas, ctx, fused_steps):
        self.replicas, self.ctx, self.fused_steps, self.ms = replicas, ctx, fused_steps, None
        self.streams = "pipe%d" % len(replicas)
        for rp in replicas:                  # the host's run-ahead is bounded over the whole pipeline, not per replica
            rp.max_in_flight = max(2, 24 // len(replicas))
        self.algos = replicas[0].algos
        self.turn, self.last = 0, replicas[0]
        self.stream_probe = None             # {"shift": s, "ms_per_pass": [...]} once Net._probe_streams has placed the replicas

    @property
    def inputs(self):
        return self.last.inputs

    @property
    def outputs(self):
        return self.last.outputs

    def feed(self, xs):
        rp = self.replicas[self.turn]
        for dst, a in zip(rp.inputs, xs):
            _feed_static(rp.ctx, dst, a, always=True)                           # on the replica's stream
        rp._fed = True

    def launch(self, join=True, hold=None):
        rp = self.replicas[self.turn]
        self.turn = (self.turn + 1) % len(self.replicas)
        self.last = rp
        if join:
            rp.ctx.wait_for(self.ctx)
        rp.launch(hold=hold)
        if join:
            self.join()

    def join(self):
        for rp in self.replicas:
            if rp.ctx is not self.ctx:
                self.ctx.wait_for(rp.ctx)


class Pending:
    """Handle of a forward pass submitted with `Net.submit`: the pass runs on one of the net's replica streams while the
    caller goes on (submits the next batch, prepares inputs).  `result()` hands the outputs to the net's own stream --
    device arrays, private to this handle, ordered behind the pass (no host wait); `get()` returns host arrays.  Both
    unwrap like `Net.__call__` (net.py:101)."""

    def __init__(self, net, outs, event, to_host, final=False, tickets=None):
        self.net, self._outs, self._event, self._to_host, self._final = net, outs, event, to_host, final
        # host-array submits: the device -> pinned-host copies of the outputs were enqueued at submit time (one ticket per
        # output, None where no pinned buffer was free); get() only waits for them
        self._tickets = tickets

    def done(self):
        """Host-side wait for this pass alone (not for passes submitted after it)."""
        if self._event is not None:
            self._event.synchronize()
        return self

    def result(self):
        if self._event is not None:
            self.net.ctx.wait_event(self._event)
            self.net._events.append(self._event)
            self._event = None
        rst = self._outs
        if self._final:                               # Net.__call__ ran the pass (flows that cannot be captured): as it returned
            return rst
        if self._to_host:
            tk, self._tickets = self._tickets, None
            if tk is not None:
                seq = rst if isinstance(rst, tuple) else (rst,)
                got = tuple(o.get_finish(t) if isinstance(o, DeviceArray) else o for o, t in zip(seq, tk))
                rst = got if isinstance(rst, tuple) else got[0]
            else:
                rst = tuple(i.get() for i in rst) if isinstance(rst, tuple) else rst.get()
        return rst[0] if len(rst) == 1 else rst

    def __del__(self):
        try:
            tk, self._tickets = self._tickets, None
            if tk is not None:                        # dropped without get(): hand the pinned buffers back
                seq = self._outs if isinstance(self._outs, tuple) else (self._outs,)
                for o, t in zip(seq, tk):
                    if isinstance(o, DeviceArray):
                        o.get_cancel(t)
        except Exception:
            pass

    def get(self):
        if self._final:
            rst = self._outs
            if isinstance(rst, tuple):
                return tuple(i.get() if isinstance(i, DeviceArray) else i for i in rst)
            return rst.get() if isinstance(rst, DeviceArray) else rst
        self._to_host = True
        return self.result()


class Net:
    def __init__(self, ctx=None):
        self.weights, self.body, self.flow = [], [], []
        self.life, self.timer = {}, {}
        self.input, self.inits, self.layer = [], [], []
        self.ctx = ctx
        self.use_graph = os.environ.get("PLANER_HIP_GRAPH", "1") != "0"
        self.use_fusion = os.environ.get("PLANER_HIP_FUSE", "1") != "0"
        self.profile = os.environ.get("PLANER_HIP_PROFILE", "0") == "1"
        # compiled plans keep activations channel-quad (Q4) between layers that have Q4 kernels
        # "force": channel-quad layout wherever a Q4 kernel exists, whatever the conversion-cost estimate says (tests)
        self.use_q4 = {"0": False, "force": "force"}.get(os.environ.get("PLANER_HIP_Q4", "1"), True)
        # dilated 3x3 convs folded by pixel phase onto the Winograd kernels (plan.fold_dilated): False (the default:
        # the program of a compiler without the pass), True = where it measures faster (_fold_worth), "force" = every eligible conv
        self.fold_dilated = {"1": True, "force": "force"}.get(os.environ.get("PLANER_HIP_DILATED_FOLD", "0"), False)
        self.dilated_folds = 0       # dilated convs the last plan runs folded
        self.refolds = 0             # refold_q4 steps of the last plan
        self._fold_pick = {}         # (x shape, filter shape, dilation) -> fold or not, as measured (_fold_worth)
        # streams: how many sub-batch graphs a forward pass is fanned out to ("auto" measures 1/2/4)
        self.streams = os.environ.get("PLANER_HIP_STREAMS", "auto")
        self._side = []
        self._events = []            # recycled stream markers of finished Pending handles (Net.submit)
        self.device_timer = {}       # kind -> ms of device time (profile mode)
        self.last_events = []        # [(layer name, kind, ms)] of the last profiled forward
        self._blob = None
        self._slots = []             # (offset, nbytes) per weight inside the blob
        self._program = None
        self._eager_prog = {}        # input signature -> fused program, for nets whose flow cannot be captured (Net.__call__)
        self._plans = {}
        self._extra = {}             # derived constant tensors (tap-major / Winograd filters)
        self._algo = {}              # conv shape signature -> chosen w_layout
        self._algo_tp = {}           # the same for THROUGHPUT plans where the pipeline's judge differs from the isolated one
        self._pick_mode = None       # "throughput" while a throughput plan's program is being fused (Net.picking)
        self.wino_chains = 0         # F(4x4,3x3) output / input transform pairs the last plan runs as one kernel
        self.conv_pairs = 0          # sibling conv pairs the last plan runs as one launch
        self.conv_wino_fused = 0     # 1x1 convs the last plan runs inside the next conv's Winograd input transform
        self.instnorm_fused = 0      # add / relu steps the last plan runs inside a channel-quad instance norm
        self.linear_adds_fused = 0   # add steps the last plan runs inside a channel-quad linear upsample / resize
        self.pixel_shuffles_fused = 0  # reshape / transpose / reshape trios the last plan runs as one pixelshuffle step
        self.groupnorms_fused = 0    # reshape / instance norm / reshape / mul / add runs the last plan runs as one groupnorm step
        # force_algo: w_layout (int) every eligible 3x3/s1/p1 conv must use, or None = pick by timing
        fa = os.environ.get("PLANER_HIP_CONV_ALGO")
        self.force_algo = int(fa) if fa else None
        # choices persist next to the C library's launch-plan cache, so a second run (profiling!)
        # launches no trial kernels and reproduces the first run's kernels exactly; the database shipped in
        # planer_amd/tuned/ (hip.Context.tuned_db) holds the picks for the BASELINE workloads on this device
        tc = os.environ.get("PLANER_HIP_TUNE_CACHE")
        self.algo_cache = tc + ".algo.json" if tc else None
        self._algo_loaded = False
        self._streams_pick = {}      # compile key -> stream plan ("pipe3", "2x2", ...) chosen by measurement
        self.algo_misses = 0         # conv algorithm picks that had to be measured (no cached choice)
        self.stream_misses = 0       # stream-plan picks that had to be measured
        self._image_in = {}          # input key (None: the first input) -> util.ImageSpec: uint8 batches that input also takes
        self._image_out = {}         # output position -> util.ImageOutSpec / util.LabelSpec: that output comes back as uint8;
                                     # util.ObjectSpec: as labels, num, objects, centroids in its place; util.KeypointSpec: as
                                     # peaks, num; util.FlowSpec: as masks, num, instances, centres; util.TextSpec: as text,
                                     # length, conf, spans (a spec's `places` says how many arrays it hands back)
        self._detect = None          # (util.DetectionSpec, positions of its heads or None: every output): they come back as det, num

    # ---- loading ----------------------------------------------------------------
    def load_json(self, inputs, inits, body, flow, debug=False):
        """net.py:10-24.  Unknown layer kinds raise KeyError like the reference."""
        self.ctx = self.ctx or hip.context()
        if debug:
            for i in body:
                print(i)
        self._program = _Program(body, flow)
        self.body = list(self._program.objs.items())
        self.life = self._program.life
        self.input, self.inits = inputs, [i[0] for i in inits]
        self.layer, self.flow = body, flow
        # one device allocation for every weight; slots padded to 256 B
        self._slots, off = [], 0
        for _, shape, dt in inits:
            nbytes = int(numpy.prod(shape, dtype=numpy.int64)) * numpy.dtype(dt).itemsize
            self._slots.append((off, nbytes))
            off += (nbytes + _ALIGN - 1) // _ALIGN * _ALIGN
        self._blob = hip.zeros((max(off, 1),), numpy.uint8, self.ctx)
        self._host = numpy.zeros(max(off, 1), numpy.uint8)
        self.weights = []
        for (o, nbytes), (_, shape, dt) in zip(self._slots, inits):
            host = self._host[o:o + nbytes].view(dt).reshape(shape)
            self.weights.append(DeviceArray(shape, dt, self.ctx, self._blob.ptr + o, self._blob, host))
        self._plans = {}

    def load_weights(self, data):
        """net.py:83-88: `data` holds the raw bytes of every init back to back."""
        raw = numpy.ascontiguousarray(data).view(numpy.uint8).ravel()
        need = sum(n for _, n in self._slots)
        if raw.size < need:
            raise ValueError("weight blob has %d bytes, the graph needs %d" % (raw.size, need))
        pos = 0
        for o, n in self._slots:
            self._host[o:o + n] = raw[pos:pos + n]
            pos += n
        self._blob.set(self._host)
        self._plans, self._extra, self._eager_prog = {}, {}, {}

    def weight_blob(self):
        """The single device allocation holding all weights (RCCL broadcast unit)."""
        return self._blob

    def refresh_host_mirror(self):
        """Re-read the host mirror after the device blob was written by a broadcast."""
        self._host[:] = self._blob.get()
        self._plans, self._extra = {}, {}

    def image_input(self, k, b, layout="nhwc", size=None, order=None, key=None):
        """Input `key` (default: the first) also takes uint8 image batches, host ndarray or DeviceArray, (N, H, W, C) for
        layout "nhwc" or (N, C, H, W) for "nchw": the net then reads fl(fl(x * k[c]) + b[c]) as float32 NCHW (k, b per channel
        from util.image_affine), channel c taken from source channel order[c], resized to `size` by util.resize's rule where
        the batch's H x W differs.  The decode is one kernel (pl_image_u8_nchw_f32) in front of the pass; a uint8 batch runs the
        plan of the float32 tensor it decodes to.  float32 inputs are taken as before.  Calling it again replaces the
        declaration."""
        self._image_in[key] = ImageSpec(k, b, layout, size, order)
        u8 = lambda sig: any(dt == "uint8" for _, dt in sig)        # noqa: E731
        self._plans = {s: p for s, p in self._plans.items() if not u8(s[1:])}
        self._eager_prog = {s: p for s, p in self._eager_prog.items() if not u8(s)}
        return self

    def image_output(self, k, b, layout="nhwc", order=None, rounding="nearest", index=0):
        """Output number `index` (its position in what the net returns), a float32 (N, C, H, W) tensor, comes back as uint8
        images, (N, H, W, Co) for layout "nhwc" or (N, Co, H, W) for "nchw": the byte of fl(fl(v * k[c]) + b[c]) (k, b per channel
        from util.image_affine_inverse), v taken from plane order[c]; NaN -> 0, clamped to [0, 255], rounded to nearest even or
        truncated ("truncate": what astype(uint8) does).  One kernel (pl_image_f32_u8) behind the pass, in place of the private
        copy of that output: plans are not touched.  A later declaration for the same index replaces this one."""
        spec = ImageOutSpec(k, b, layout, order, rounding)
        self._image_out[self._unclaimed(index)] = spec
        return self

    def label_output(self, threshold=0.0, index=0):
        """Output number `index`, float32 (N, C, H, W) scores, comes back as the uint8 label map (N, H, W): numpy's argmax over
        the C planes (2 to 256), for C == 1 the comparison x > threshold (pl_labels_f32_u8).  See `image_output`."""
        spec = LabelSpec(threshold)
        self._image_out[self._unclaimed(index)] = spec
        return self

    def object_output(self, threshold=0.0, connectivity=8, background=0, max_objects=256, index=0):
        """Output number `index`, float32 (N, C, H, W) scores, comes back as its objects, four arrays in its place: labels int32
        (N, H, W), num int32 (N,), objects int32 (N, max_objects, 6) rows [class, area, y0, x0, y1, x1] and centroids float32
        (N, max_objects, 2) rows [cy, cx] -- the connected components (`connectivity` 4 or 8, class `background` left out, -1:
        none) of `label_output`'s map, numbered per image by the raster position of their first pixel (util.ObjectSpec:
        pl_labels_f32_u8, then pl_components_u8_i32).  For a one-output net: labels, num, objects, centroids = net(x).  See
        `image_output`."""
        spec = ObjectSpec(threshold, connectivity, background, max_objects)
        self._image_out[self._unclaimed(index)] = spec
        return self

    def keypoint_output(self, threshold=0.0, ties="all", max_peaks=32, refine="none", stride=1.0, index=0):
        """Output number `index`, float32 (N, K, H, W) heat maps, comes back as points, two arrays in its place: peaks float32
        (N, K, max_peaks, 3), per plane the best `max_peaks` 3 x 3 local maxima above `threshold` as rows [x, y, score] by
        descending score (equal scores by raster position; +0.0 in unused rows), x and y scaled by `stride` (a number or
        (sy, sx)) and with refine="quarter" moved a quarter pixel towards the higher neighbour; and num int32 (N, K), all peaks
        of the plane, which may exceed max_peaks.  ties "all" keeps every pixel of a plateau, "first" its first
        (util.KeypointSpec: pl_peaks_f32).  For a one-output net: peaks, num = net(x).  With max_peaks=1, ties="first",
        threshold=-inf, row 0 is numpy's argmax of each plane (on planes without NaN, maximum above -inf).  `Net.tiled` refuses
        a net with this declared.  See `image_output`."""
        spec = KeypointSpec(threshold, ties, max_peaks, refine, stride)
        self._image_out[self._unclaimed(index)] = spec
        return self

    def flow_output(self, level=0.0, min_flow=0.0, rounds=10, min_size=15, max_instances=256, planes=(0, 1, 2), index=0):
        """Output number `index`, float32 (N, C, H, W) with a flow field (dy, dx) and a probability in the planes `planes`, comes
        back as instance masks by flow following, four arrays in its place: masks int32 (N, H, W), num int32 (N,), instances
        int32 (N, max_instances, 5) rows [area, y0, x0, y1, x1] and centres float32 (N, max_instances, 2) rows [cy, cx].  A pixel
        is foreground iff prob > level; it follows the flow (where longer than min_flow) for 2^rounds steps inside the
        foreground, and the pixels that meet at one 8-connected sink region are one instance; instances below `min_size`
        pixels are dropped (util.FlowSpec: pl_flow_instances_f32).  For a one-output net: masks, num, instances, centres =
        net(x).  `Net.tiled` follows the flows of the blended scan.  See `image_output`."""
        spec = FlowSpec(level, min_flow, rounds, min_size, max_instances, planes)
        self._image_out[self._unclaimed(index)] = spec
        return self

    def text_output(self, layout="tnc", blank=0, merge_repeated=True, confidence="softmax", max_len=64, index=0):
        """Output number `index`, a float32 sequence tensor -- `layout` "tnc" (T, N, C), "ntc" (N, T, C), or "nchw" (N, C, H, W)
        with one sequence per (n, h) and time along W -- comes back as text by greedy CTC decoding, four arrays in its place,
        `lead` being (N,) or for "nchw" (N, H): text int32 lead + (max_len,), the labels of the first `max_len` symbols and -1
        behind them; length int32 lead, all symbols of the sequence, which may exceed max_len; conf float32 lead + (max_len,),
        the confidence of each symbol's first frame; spans int32 lead + (max_len, 2), [start, end) in frames.  A frame's label
        is numpy's argmax over the classes; a symbol starts where the label is not `blank` and, with `merge_repeated`, differs
        from the frame in front.  `confidence` "softmax": 1 / sum exp(x - max); "value": x at the argmax; "none": +0.0
        (util.TextSpec: pl_ctc_greedy_f32).  For a one-output net: text, length, conf, spans = net(x); util.text_strings makes
        strings of the first two.  `Net.tiled` refuses a net with this declared.  See `image_output`."""
        spec = TextSpec(layout, blank, merge_repeated, confidence, max_len)
        self._image_out[self._unclaimed(index)] = spec
        return self

    def float_output(self, index=0):
        """Output number `index` comes back as the float32 tensor again; if it is a head of a detection declaration, so do all
        of that declaration's heads."""
        index = self._out_index(index)
        self._image_out.pop(index, None)
        if self._detect is not None and (self._detect[1] is None or index in self._detect[1]):
            self._detect = None
        return self

    def detection_output(self, heads, classes, conf=0.25, iou=0.45, max_det=100, max_candidates=1024, class_aware=True, size=None,
                         indices=None):
        """The outputs at positions `indices` (in head order; default: every output, in order) are YOLO-style heads, float32
        (N, A (5 + classes), Gh, Gw), head h with anchors and stride heads[h] = (anchors, stride or None).  In their place the
        net returns det, float32 (N, max_det, 6) rows [x1, y1, x2, y2, score, class] in input pixels by descending score (+0.0
        in unused rows), and num, int32 (N,), inserted where the lowest of those positions was; the other outputs keep their
        order.  Decode, top-k and NMS run behind the pass on the stream that owns the outputs (util.DetectionSpec): plans are
        not touched.  Declaring again replaces the declaration; `float_output` on one of the positions removes it."""
        spec = DetectionSpec(heads, classes, conf, iou, max_det, max_candidates, class_aware, size)
        if indices is not None:
            indices = tuple(self._out_index(i) for i in indices)
            if len(indices) != len(spec.heads) or len(set(indices)) != len(indices):
                raise ValueError("detection output: indices names one distinct output position per head (%d), got %r"
                                 % (len(spec.heads), indices))
        taken = sorted(self._image_out if indices is None else set(indices) & set(self._image_out))
        if taken:
            raise ValueError("detection output: output %d is already declared an image or label output" % taken[0])
        self._detect = (spec, indices)
        return self

    def tiled(self, image, window=1024, margin=0.1, sample=1, glob=1, batch=None, progress=None):
        """Whole-image inference, util.tile's job as a mode of the net: `image`, (H, W[, C]) as a host ndarray or a DeviceArray,
        is cut into overlapping windows (util.tile's geometry: `sample`, `glob`, `window`, `margin` as there), the windows go
        through the net in chunks of `batch` (default: all of them, one pass) and the results are blended with util.tile's
        border-distance weights -- bit for bit the reference's float32 loop.  One gather kernel in front of each pass
        (pl_tile_windows_*_nchw_f32) writes the plan's NCHW input, one blend kernel behind the last (pl_tile_blend_*) reads the
        plan's NCHW results: no per-window launches, no transposes, no blend buffers.
        A uint8 image needs a declared `image_input`, whose k, b and order are used (its `size` and `layout` are not: the image
        is one (H, W, C) array and the working size is `sample`'s); a float32 image is taken as it is.  Returns float32
        (OH, OW, Co); with `label_output` declared on output 0 the uint8 label map (OH, OW); with `image_output` the uint8 image in
        its layout: (OH, OW, Co') or (Co', OH, OW); with `object_output` the objects of the blended label map, labels (OH, OW),
        num (1,), objects (1, max_objects, 6) and centroids (1, max_objects, 2); with `flow_output` the instances of the blended flow and
        probability planes (the windows are blended as floats, then one chain follows the whole map), masks (OH, OW), num (1,),
        instances (1, max_instances, 5) and centres (1, max_instances, 2).  Host image in, host array out; device in, device out.
        A declared `keypoint_output` raises ValueError: peaks of a blended scan are not built; so does a declared `text_output`.
        Every chunk runs the plan of ONE signature, (batch, Co, h, w): a short last chunk is padded with its last window.
        `progress(i, n)` is called after each chunk with the number of its last window (not at all for a single window).
        Where the working size differs from the image's (`sample`, or an image smaller than the window grown to `glob`), the
        gather kernel resamples on the way in and the float32 result goes through util.resize on the way out; a declared uint8
        or label output then raises NotImplementedError.  All n window results stay resident until the blend:
        n Co oh ow 4 bytes.  Nets with several inputs or outputs, or with `detection_output` declared, raise ValueError."""
        if len(self.input) != 1:
            raise ValueError("Net.tiled: a net with one input, this one has %d" % len(self.input))
        if self._detect is not None:
            raise ValueError("Net.tiled: detections of windows cannot be blended; `float_output` removes the declaration")
        host_in = isinstance(image, numpy.ndarray)
        if host_in and image.dtype != numpy.uint8:
            image = numpy.ascontiguousarray(image, dtype=numpy.float32)
        if not isinstance(image, (numpy.ndarray, DeviceArray)) or image.ndim not in (2, 3) or image.dtype not in (numpy.uint8, numpy.float32):
            raise ValueError("Net.tiled: an (H, W[, C]) image, uint8 or float32, host ndarray or DeviceArray, got %r" % (image,))
        spec = None
        if image.dtype == numpy.uint8:
            spec = self._image_spec(0)
            if spec is None:
                raise ValueError("Net.tiled: a uint8 image needs `image_input` declared (its k, b and order are used)")
        out_spec = self._image_out.get(0)
        if isinstance(out_spec, TextSpec):
            raise ValueError("Net.tiled: a text output is declared, and a blended scan is no sequence tensor; "
                             "`float_output` removes the declaration")
        if isinstance(out_spec, KeypointSpec):
            raise ValueError("Net.tiled: a keypoint output is declared, and the peaks of a blended scan are not built; "
                             "`float_output` removes the declaration, `util.heatmap_peaks` takes the blended heat maps")
        geo = _Tiling(image.shape[0], image.shape[1], sample, glob, window, margin)
        if geo.resampled and out_spec is not None:
            raise NotImplementedError("Net.tiled: the working size %s differs from the image's %s, so the blended result is resampled "
                                      "back -- and the argmax or the bytes of a resampled blend are a different product from the "
                                      "resampled label map or image; use `float_output` and encode the result" % (geo.work, geo.src))
        n = len(geo.windows)
        batch = n if batch is None else int(batch)
        if batch < 1:
            raise ValueError("Net.tiled: batch is a count >= 1, got %r" % (batch,))
        batch = min(batch, n)
        dev = hip.asarray(image, ctx=self.ctx)
        feeds = WindowFeed(dev, geo.windows, spec, geo.work)
        results = shape = blend = None
        for lo in range(0, n, batch):
            hi = min(lo + batch, n)
            out = self._run_windows(feeds.chunk(lo, batch))
            if shape is None:
                shape = tuple(out.shape)
                if out.dtype != numpy.float32 or len(shape) != 4:
                    raise ValueError("Net.tiled: the net's result is no float32 (N, C, H, W) tensor: %s %s" % (out.dtype, shape))
                k = shape[2] / geo.win_h                 # output pixels per working pixel
                blend = BlendGeometry(geo.windows, k, geo.margin, geo.work, shape[2], shape[3])
                if out_spec is not None:
                    out_spec.geometry((n,) + shape[1:])
            if batch == n:
                results = out                            # one pass: the blend reads the plan's own buffer
            else:
                if results is None:
                    results = hip.empty((n,) + shape[1:], ctx=self.ctx)
                results.rows(lo, hi).copy_from(out.rows(0, hi - lo))
            if progress is not None and n > 1:
                progress(hi, n)
        objects, flows = isinstance(out_spec, ObjectSpec), isinstance(out_spec, FlowSpec)
        rst = _blend_windows(results, geo.windows, blend.k, geo.margin, geo.work,
                             out_spec.labels if objects else "float" if flows or out_spec is None else out_spec)
        if flows:                                        # the instances of the scan: one chain on the blended (OH, OW, C) map
            masks, num, table, centres = out_spec.encode_hwc(rst)
            rst = masks.reshape(masks.shape[1:]), num, table, centres
            return tuple(a.get() for a in rst) if host_in else rst
        if objects:                                      # the objects of the scan, not of the windows: one chain on the whole map
            labels, num, table, centroids = out_spec.components(rst.reshape((1,) + tuple(rst.shape)))
            rst = labels.reshape(labels.shape[1:]), num, table, centroids
            return tuple(a.get() for a in rst) if host_in else rst
        if geo.resampled:
            rst = _resize(rst, geo.back_size(blend.k))
        return rst.get() if host_in else rst

    def _run_windows(self, feed):
        """The net's single float32 result for the windows of `feed`, as the pass left it (a plan's own output buffer)."""
        out = None
        if self.use_graph and not self.profile:
            try:
                plan = self.compile(feed)
                if isinstance(plan.outputs, tuple) and len(plan.outputs) != 1:      # (before anything is launched)
                    raise ValueError("Net.tiled: a net with one output, this one returns %d" % len(plan.outputs))
                out = self._launch([feed], declared=False).outputs
            except _lib.NotCapturable:
                self.use_graph = False
        if out is None:
            x = feed.materialise()
            out = self._interpret(self._eager_program([x]), [x]) if self._eager_prog else self.forward(x)
        if isinstance(out, (tuple, list)):
            if len(out) != 1:
                raise ValueError("Net.tiled: a net with one output, this one returns %d" % len(out))
            out = out[0]
        if not isinstance(out, DeviceArray):
            raise ValueError("Net.tiled: the net's result is no device tensor: %s" % type(out).__name__)
        return out

    def _unclaimed(self, index):
        index = self._out_index(index)
        if self._detect is not None and (self._detect[1] is None or index in self._detect[1]):
            raise ValueError("output %d is a head of the declared detection output" % index)
        return index

    @staticmethod
    def _out_index(index):
        if not isinstance(index, (int, numpy.integer)) or index < 0:
            raise ValueError("output index is a position in what the net returns (0, 1, ...), got %r" % (index,))
        return int(index)

    def _check_outputs(self, out):
        """ValueError unless every declared output is a float32 device tensor of the shape its encoder takes.  Returns the positions of
        the detection heads (None: none declared)."""
        seq = out if isinstance(out, tuple) else (out,)
        for i, spec in self._image_out.items():
            if i >= len(seq):
                raise ValueError("output %d is declared uint8, the net returns %d output(s)" % (i, len(seq)))
            if not isinstance(seq[i], DeviceArray):
                raise ValueError("output %d is declared uint8 and is no device tensor: %s" % (i, type(seq[i]).__name__))
            spec.check(seq[i])
        if self._detect is None:
            return None
        spec, idx = self._detect
        if idx is None:
            idx = tuple(range(len(seq)))
            if len(idx) != len(spec.heads):
                raise ValueError("detection output: %d heads declared, the net returns %d output(s)" % (len(spec.heads), len(seq)))
        for i in idx:
            if i >= len(seq):
                raise ValueError("output %d is declared a detection head, the net returns %d output(s)" % (i, len(seq)))
            if not isinstance(seq[i], DeviceArray):
                raise ValueError("output %d is declared a detection head and is no device tensor: %s" % (i, type(seq[i]).__name__))
        spec.check([seq[i] for i in idx])
        return idx

    def _hand_back(self, out, private):
        """What a pass hands to the caller: a declared output encoded into a fresh uint8 array on the stream that owns it, the
        others as private copies (`private`: the plan's buffers are rewritten by the next pass) or as they are."""
        if not self._image_out and self._detect is None and not private:
            return out
        heads = self._check_outputs(out)
        seq = out if isinstance(out, tuple) else (out,)
        rst = [self._image_out[i].encode(o) if i in self._image_out else
               o.copy() if private and isinstance(o, DeviceArray) and not (heads and i in heads) else o for i, o in enumerate(seq)]
        # a spec says how many places its arrays take: an object output's four, a keypoint output's two
        places = [tuple(r) if i in self._image_out and self._image_out[i].places > 1 else (r,) for i, r in enumerate(rst)]
        if heads is None:
            flat = tuple(a for p in places for a in p)
            return flat if isinstance(out, tuple) or len(flat) > 1 else flat[0]
        # det, num where the lowest head was; the heads themselves are not handed back (nor copied)
        first = min(heads)
        det_num = self._detect[0].encode([seq[i] for i in heads])
        return tuple(r for i, p in enumerate(places) for r in (det_num if i == first else () if i in heads else p))

    def _image_spec(self, pos):
        name = self.input[pos] if pos < len(self.input) else None
        return self._image_in.get(name, self._image_in.get(None) if pos == 0 else None)

    def _image_feeds(self, xs):
        """uint8 batches of inputs declared with `image_input` (host arrays are uploaded as they are) -> ImageFeeds."""
        xs = list(xs)
        for i, a in enumerate(xs if self._image_in else ()):
            spec = self._image_spec(i)
            if spec is not None and isinstance(a, (DeviceArray, numpy.ndarray)) and a.dtype == numpy.uint8:
                xs[i] = spec.bind(hip.asarray(a, ctx=self.ctx))
        return xs

    def _signature(self, xs):
        """(shape, dtype) per input as a plan is keyed: a declared uint8 batch counts as the float32 tensor it decodes to."""
        sig = []
        for i, a in enumerate(xs):
            spec = self._image_spec(i) if self._image_in else None
            if spec is not None and not isinstance(a, ImageFeed) and a.dtype == numpy.uint8:
                sig.append((spec.geometry(a.shape)[1], "float32"))
            else:
                sig.append((tuple(a.shape), str(a.dtype)))
        return tuple(sig)

    def half(self):
        raise NotImplementedError("planer_amd computes the hot path in float32 only (BASELINE metric)")

    def show(self):
        raise NotImplementedError("plot_net is missing from the reference snapshot too (net.py:90-92)")

    def info(self, obj):
        if isinstance(obj, (list, tuple)):
            return [self.info(i) for i in obj]
        return obj.shape if hasattr(obj, "shape") else obj

    # ---- eager interpreter ---------------------------------------------------------
    def _interpret(self, prog, xs, debug=False, shapes=None, profile=False, record=None, repeat=1):
        """net.py:37-72: one kernel launch (or view) per layer, in flow order.  `record` (a list)
        receives one dict per convolution / dense step: which kernel family and launch plan ran.  `profile` brackets the
        steps with stream markers; with `repeat` = R > 1 every step is launched R times between its markers (the time per
        launch is what gets recorded: a marker costs about as much as a small kernel, R launches dilute it)."""
        env = {"None": None}
        env.update(zip(self.inits, self.weights))
        env.update(self._extra)
        env.update(zip(self.input, xs))
        events, out_key = [], None
        for i, (src, names, dst) in enumerate(prog.flow):
            for pos, name in enumerate(_as_list(names)):
                keys = src if pos == 0 else dst                  # chained layers
                args = [env[keys]] if isinstance(keys, str) else [env.get(k) for k in keys]
                for k in set(_as_list(src)):
                    if k in env and prog.life[k] <= i:
                        del env[k]                               # release dead inputs
                obj = prog.objs[name]
                if debug:
                    print(name, obj.name, ":", obj.para())
                    print("\t--> ", keys, ":", self.info(args))
                t0 = time.time()
                if profile and not events:
                    events.append((None, None, hip.Event(self.ctx).record()))
                val = obj(*args)
                for _ in range(repeat - 1 if profile else 0):
                    val = obj(*args)
                if profile:                                  # ONE marker per step boundary: step time = marker to marker
                    events.append((name, obj.name, hip.Event(self.ctx).record()))
                if record is not None and obj.name in ("conv", "conv_fused", "conv_q4", "dense", "matmul", "wino4_gemm", "wino43_gemm",
                                                       "conv_q4_pair", "conv_pool_q4", "conv1x1_wino_in", "convt_q4", "convt_fused"):
                    lay = (obj.para().get("w_layout", DIRECT_Q4 if obj.name in ("conv_q4_pair", "conv1x1_wino_in") else IGEMM_NCHW)
                           if obj.name != "conv" else IGEMM_NCHW)
                    lname = name
                    if obj.name in ("wino4_gemm", "wino43_gemm"):       # the GEMM stage of a staged Winograd conv
                        lay, lname = (WINO4_Q4 if obj.name == "wino4_gemm" else WINO43_Q4), name[:-len("@gemm")]
                    ctx_ = args[0].ctx if isinstance(args[0], DeviceArray) else self.ctx
                    xshape = (args[0].meta if args[0].meta is not None else
                              _q4.logical_shape(args[0]) if _q4.is_q4(args[0]) else args[0].shape)
                    record.append({"layer": lname, "kind": obj.name, "w_layout": lay,
                                   "algo": W_LAYOUT_NAMES.get(lay, str(lay)), "plan": ctx_.last_conv_plan(),
                                   "extents": list(ctx_.last_conv_extents()), "x": list(xshape)})
                    if getattr(args[0], "fold", None) is not None:       # a conv on a folded tensor: `x` is the folded shape
                        record[-1]["fold"] = list(args[0].fold)
                if record is not None and obj.name in ("instancenormalization_q4", "groupnorm_q4"):
                    # the form taken ("instnorm-q4 one-wg" / "instnorm-q4 chunks=S", "groupnorm-q4 wide one-wg" ...), as the entry
                    # point left it
                    record.append({"layer": name, "kind": obj.name, "w_layout": None, "algo": "instnorm-q4" if obj.name == "instancenormalization_q4" else "groupnorm-q4",
                                   "plan": args[0].ctx.last_conv_plan() if args[0].size else "", "extents": [],
                                   "x": list(_q4.logical_shape(args[0]))})
                del args
                if isinstance(dst, str):
                    env[dst] = val
                else:
                    env.update(zip(dst, val))
                if debug:
                    for k in _as_list(dst):
                        print("\t<-- ", k, ":", self.info(env[k]))
                if shapes is not None:
                    for k in _as_list(dst):
                        shapes[k] = getattr(env[k], "shape", None)
                self.timer[obj.name] = self.timer.get(obj.name, 0) + time.time() - t0
                del val
            out_key = dst
        if profile:
            self.last_events = []
            for (_, _, e0), (name, kind, e1) in zip(events, events[1:]):
                ms = e0.elapsed_ms(e1) / max(1, repeat)
                self.last_events.append((name, kind, ms))
                self.device_timer[kind] = self.device_timer.get(kind, 0.0) + ms
        return env[out_key]

    def forward(self, *x, debug=False):
        """Per-layer execution of the flow exactly as written (no fusion)."""
        return self._interpret(self._program, x, debug=debug, profile=self.profile)

    def timeit(self, status="start"):
        """net.py:74-77"""
        if status == "start":
            self.timer, self.device_timer = {}, {}
        if status == "end":
            for k in self.timer:
                print(k, self.timer[k])

    def run(self, output=None, input={}):
        """onnxruntime-style entry (net.py:79-81)"""
        rst = self(input)
        return rst if isinstance(rst, tuple) else (rst,)

    # ---- plan compiler -----------------------------------------------------------------
    def _fuse(self, shapes, fuse=True):
        """Plan program: fused epilogues + tap-major filter copies for the fast conv kernel.  The passes and their order are
        plan.compile_front's and plan.lower's; this reads the switches, answers what needs the device or the weights, and keeps
        the counters."""
        wmap = dict(zip(self.inits, self.weights))
        worth = None
        if self.fold_dilated:
            worth = (lambda xs, ks, para: True) if self.fold_dilated == "force" else self._fold_worth
        body, flow, counts = compile_front(self.layer, self.flow, self.inits, shapes, fuse=fuse, q4=self.use_q4, worth=worth,
                                           values=lambda key: wmap[key].host if key in wmap else None)
        if self.use_q4:
            self.pixel_shuffles_fused = counts.get("fuse_pixel_shuffle", 0)
            self.groupnorms_fused = counts.get("fuse_groupnorm", 0)
            self.instnorm_fused, self.linear_adds_fused = counts["fuse_instnorm_q4"], counts["fuse_linear_add"]
        if "fold_dilated" in counts:
            self.dilated_folds = sum(len(r["heads"]) for r in counts["fold_dilated"])
            refold_layers = {b[0] for b in body if b[1] == "refold_q4"}
            self.refolds = sum(1 for f in flow if f[1][0] in refold_layers)
        if os.environ.get("PLANER_HIP_TAPMAJOR", "1") != "0":
            body, flow = self._prepare_filters(body, flow, shapes)
        return _Program(body, flow), counts.get("fuse_flow", 0)

    def _prepare_filters(self, body, flow, shapes):
        """Give every eligible conv a prepared copy of its (constant) filter: tap-major for the
        fast implicit-GEMM kernel, or Winograd-domain where that measures faster for this shape."""
        wmap = dict(zip(self.inits, self.weights))
        env = lambda name, default="1": os.environ.get("PLANER_HIP_" + name, default)          # noqa: E731

        def kshape(key):
            # an init or a prepared copy of one; a filter that is not float32 is left to the kernel that converts it
            K = wmap.get(key, self._extra.get(key))
            return K.shape if K is not None and K.dtype == numpy.float32 else None

        stem_form = {"wino": False}     # what `stem_pool` chose for the stem whose filter `prepare` is asked for next

        def prepare(lay, init, para):
            key = init + suffix(lay, para)
            if key not in self._extra:
                self._extra[key] = LAYOUTS[lay].prepare(wmap[init], **para)
            if lay == STEM_POOL_NCHW:
                # the F(4,4) form of the stem kernel is neither a layout nor a step parameter (recorded programs stay as they
                # are): its filter rides on the direct form's, and the step runs it where it finds one (q4.ConvPoolQ4)
                _q4.attach_stem_wino(self._extra[key], wmap[init] if stem_form["wino"] else None)
            return key

        def stem_pool(xs, ks, para):
            if not _q4.stem_pool_eligible(xs, ks, **para):
                return None
            # W % 4 == 0: the kernel reads the NCHW batch itself; PLANER_HIP_STEM_NCHW=0 keeps the row-packed copy
            if env("STEM_NCHW") == "0" or not _q4.stem_pool_nchw_eligible(xs, ks, **para):
                return STEM_POOL, {}
            extra = {}
            if self._pick_mode == "throughput" and env("STEM_ROWS14") != "0":
                # throughput plans: strips of 14 pooled rows where that still leaves half a chip of workgroups -- 15
                # conv-row pairs instead of 2 x 8, on half the CUs for longer (160 against 91 us alone; +0.8 ... +1.2 % on
                # seven replicas: the other replicas' kernels take the rest of the chip)
                hq = ((xs[2] + 6 - 7) // 2 + 1 + 1) // 2
                if xs[0] * (-(-hq // 14)) * (-(-ks[0] // 64)) * 2 >= self.ctx.cu_count:
                    extra["strip_rows"] = 14
            # the polyphase F(4,4) form of the kernel (csrc/conv_stem_wino_kernel.h); PLANER_HIP_EXPERIMENT=stem_wino=0 / 1
            stem_form["wino"] = bool(experiment("stem_wino", STEM_WINO_DEFAULT)) and _q4.stem_pool_wino_eligible(xs, ks, **para)
            return STEM_POOL_NCHW, extra

        def fits(key):
            # whole planes per workgroup: the plane must fit the LDS kernel, and there must be enough (image,
            # channel quad) planes to fill the chip (a batch-1 detection net has 32-256 of them: not worth it)
            shp = shapes.get(key.split("@")[0])
            return (shp is not None and len(shp) == 4 and shp[0] * (shp[1] // 4) >= self.ctx.cu_count // 2
                    and _q4.wino4_chain_supported(tuple(shp), self.ctx))

        lim = env("CONV1X1_WINO", "4096")            # =0 turns the 1x1 -> Winograd input transform step off, =<tiles> moves the limit

        def small(key):
            shp = shapes.get(key.split("@")[0])
            return shp is not None and len(shp) == 4 and shp[0] * (-(-shp[2] // 4)) * (-(-shp[3] // 4)) <= int(lim)

        body, flow, counts = lower(
            body, flow, self.inits, shapes, kshape=kshape, prepare=prepare, fits=fits, small=small if lim != "0" else None,
            pick=lambda cands, kind, srcs, para: self._pick_conv_algo(cands, wmap[srcs[1]], srcs, para, shapes, q4=kind == "conv_q4"),
            stem_pool=stem_pool if env("STEM_POOL") != "0" else None, pair=env("PAIR") != "0", wino_chain=env("WINO_CHAIN"))
        for name, attr in (("pair_sibling_convs", "conv_pairs"), ("chain_winograd", "wino_chains"),
                           ("fuse_conv1x1_wino_in", "conv_wino_fused")):
            if name in counts:                       # (a pass switched off leaves its counter as it was)
                setattr(self, attr, counts[name])
        return body, flow

    _fuse_upsample_concat = staticmethod(fuse_upsample_concat)      # the name callers outside the package know it by

    def _pick_conv_algo(self, cands, K, srcs, para, shapes, q4=False):
        """Time the candidate w_layouts (conv_layouts.candidates) for this conv's real shape and epilogue; the first is the
        fallback and wins ties.  Cached per shape signature (and persisted, see `algo_cache`); `force_algo` bypasses the
        measurement."""
        from .layer import ConvFused
        xs = tuple(shapes[srcs[0].split("@")[0]])
        has = [i < len(srcs) and srcs[i] != "None" for i in range(2, 6)]       # B, scale, shift, res
        sig = (q4, xs, tuple(K.shape), tuple(has), para.get("act", 0))
        if self.force_algo is not None:
            if self.force_algo not in cands:
                raise ValueError("force_algo=%r does not apply to conv %s k%s" % (self.force_algo, xs, tuple(K.shape)))
            return self.force_algo
        self._load_algo_cache()
        # Throughput plans first ask the table of picks made UNDER the pipeline (tools/pipeline_search.py): a kernel that holds
        # a fraction of the CUs for longer loses an isolated timing and can win there -- the other replicas' kernels take the rest
        # of the chip (ResNet-18 layer2 at batch 32: the fused F(4x4,3x3) kernel on 128 workgroups, 63 us against 43 us staged, and
        # +1.9 % on seven replicas).  Latency plans (net(x) one call at a time) keep the isolated picks.
        if self._pick_mode == "throughput" and self._algo_tp.get(sig) in cands:
            return self._algo_tp[sig]
        if sig in self._algo and self._algo[sig] in cands:      # (a stored pick this run's switches exclude is ignored)
            return self._algo[sig]
        self.algo_misses += 1
        ctx = self.ctx
        # random operands: zero tensors clock ~19 % higher (DVFS) and would bias the pick towards
        # the MFMA-heavy candidates (MI355X guide, "DVFS give-back")
        rng = numpy.random.default_rng(1234)
        x = hip.asarray(rng.standard_normal(xs).astype(numpy.float32), ctx=ctx)
        cout = K.shape[0]
        chan = hip.asarray(rng.uniform(0.5, 1.5, (1, cout, 1, 1)).astype(numpy.float32), ctx=ctx)
        out_shape = (xs[0], cout, xs[2], xs[3])
        res = hip.asarray(rng.standard_normal(out_shape).astype(numpy.float32), ctx=ctx) if has[3] else None
        if q4:
            x, res = _q4.to_q4(x), (_q4.to_q4(res) if res is not None else None)
        args = [hip.zeros((cout,), numpy.float32, ctx) if has[0] else None, chan if has[1] else None,
                chan if has[2] else None, res]
        kw = {k: v for k, v in para.items() if k != "w_layout"}
        conv = _q4.ConvQ4 if q4 else ConvFused
        best, best_ms = cands[0], None
        for lay in cands:
            try:
                Kp = LAYOUTS[lay].prepare(K)
                run = lambda: conv(x, Kp, *args, w_layout=lay, **kw)
                for _ in range(3):
                    run()                              # first call autotunes the MFMA plan(s)
                ms = None
                for _ in range(3):                     # best of three bursts of 8
                    e0 = hip.Event(ctx).record()
                    for _ in range(8):
                        run()
                    e1 = hip.Event(ctx).record()
                    t = e0.elapsed_ms(e1) / 8
                    ms = t if ms is None else min(ms, t)
            except (NotImplementedError, ValueError, MemoryError):
                continue
            if os.environ.get("PLANER_CONV_TUNE_LOG"):
                import sys
                print("[planer_amd] conv %s k%s tail %s: w_layout %d = %.1f us" % (xs, tuple(K.shape), has, lay, ms * 1e3),
                      file=sys.stderr)
            if best_ms is None or ms < best_ms:
                best, best_ms = lay, ms
        self._algo[sig] = best
        self._algo_dirty = True
        return best

    def _fold_worth(self, xs, ks, para):
        """plan.fold_dilated's `worth` under PLANER_HIP_DILATED_FOLD=1: is the dilated conv of input `xs` and filter `ks` faster
        folded?  Times (a) the conv as it stands -- the direct kernel at its own shape -- against (b) refold in, the picked
        candidate at the folded shape, refold out, by the burst protocol of _pick_conv_algo.  Both refolds are charged to the
        one conv although a run of folded convs shares them: deliberately conservative.  The verdict is cached per (input,
        filter, dilation) beside the algorithm picks (table "dilated_fold" of the algo cache file)."""
        from .conv_layouts import candidates
        fold = tuple(int(v) for v in para["dilations"])
        sig = ("fold", tuple(xs), tuple(ks), fold)
        self._load_algo_cache()
        if sig in self._fold_pick:
            return self._fold_pick[sig]
        self.algo_misses += 1
        ctx = self.ctx
        rng = numpy.random.default_rng(1234)
        x = _q4.to_q4(hip.asarray(rng.standard_normal(xs).astype(numpy.float32), ctx=ctx))
        K = hip.asarray((rng.standard_normal(ks) * 0.05).astype(numpy.float32), ctx=ctx)
        geo = {k: v for k, v in para.items() if k in ("group", "strides", "dilations", "pads")}
        one = dict(geo, dilations=[1, 1], pads=[1, 1, 1, 1])
        fxs = _q4.folded_shape(xs, *fold)
        cands = candidates(True, tuple(ks), one, fxs)
        lay = cands[0] if len(cands) == 1 else self._pick_conv_algo(cands, K, ["~fold_probe", "~k"], one, {"~fold_probe": fxs}, q4=True)
        Kd, Kf = LAYOUTS[DIRECT_Q4].prepare(K, **geo), LAYOUTS[lay].prepare(K, **one)

        def folded():
            y = _q4.ConvQ4(_q4.refold_q4(x, *fold), Kf, w_layout=lay, **one)
            return _q4.refold_q4(y, 1, 1)
        ms = []
        for run in (lambda: _q4.ConvQ4(x, Kd, w_layout=DIRECT_Q4, **geo), folded):
            for _ in range(3):
                run()
            best = None
            for _ in range(3):                     # best of three bursts of 8
                e0 = hip.Event(ctx).record()
                for _ in range(8):
                    run()
                e1 = hip.Event(ctx).record()
                t = e0.elapsed_ms(e1) / 8
                best = t if best is None else min(best, t)
            ms.append(best)
        if os.environ.get("PLANER_CONV_TUNE_LOG"):
            import sys
            print("[planer_amd] dilated conv %s k%s d%s: direct %.1f us, folded on w_layout %d (with both refolds) %.1f us"
                  % (tuple(xs), tuple(ks), fold, ms[0] * 1e3, lay, ms[1] * 1e3), file=sys.stderr)
        self._fold_pick[sig] = ms[1] < ms[0]
        self._algo_dirty = True
        return self._fold_pick[sig]

    @staticmethod
    def _sig_key(sig):
        return repr(sig)

    def _device_tag(self):
        ctx = self.ctx or hip.context()
        return "%s cu%d lib%d" % (ctx.arch.split(":")[0], ctx.cu_count, _lib.load().pl_version())

    def _load_algo_cache(self):
        """Shipped database first (planer_amd/tuned/<arch>_cu<N>.algo.json), then the user's cache on top.  A file
        written for another device or library version is ignored."""
        if self._algo_loaded:
            return
        self._algo_loaded = True
        import ast
        import json
        ctx = self.ctx or hip.context()
        shipped = ctx.tuned_db + ".algo.json" if getattr(ctx, "tuned_db", None) else None
        for path in (shipped, self.algo_cache):
            if not path:
                continue
            try:
                with open(path) as f:
                    stored = json.load(f)
            except (OSError, ValueError):
                continue
            if "algo" not in stored:                       # round-2 files: a flat {signature: layout} table
                stored = {"device": None, "algo": stored, "streams": {}}
            if stored.get("device") not in (None, self._device_tag()):
                continue
            for table, dst in (("algo", self._algo), ("algo_throughput", self._algo_tp)):
                for k, v in stored.get(table, {}).items():
                    try:
                        dst[ast.literal_eval(k)] = int(v)
                    except (ValueError, SyntaxError):
                        pass
            self._streams_pick.update({str(k): str(v) for k, v in stored.get("streams", {}).items()})
            for k, v in stored.get("dilated_fold", {}).items():
                try:
                    self._fold_pick[ast.literal_eval(k)] = bool(v)
                except (ValueError, SyntaxError):
                    pass

    def save_algo_cache(self, path=None):
        """Persist the per-shape conv algorithm choices and the stream-plan choices (next to PLANER_HIP_TUNE_CACHE
        by default): written to a temporary file and renamed, by rank 0 only."""
        path = path or self.algo_cache
        if not path or os.environ.get("RANK", "0") != "0":
            return
        import json
        data = {"device": self._device_tag(),
                "algo": {self._sig_key(k): v for k, v in sorted(self._algo.items(), key=repr)},
                "algo_throughput": {self._sig_key(k): v for k, v in sorted(self._algo_tp.items(), key=repr)},
                "streams": dict(sorted(self._streams_pick.items()))}
        if self._fold_pick:
            data["dilated_fold"] = {self._sig_key(k): bool(v) for k, v in sorted(self._fold_pick.items(), key=repr)}
        tmp = "%s.%d.tmp" % (path, os.getpid())
        with open(tmp, "w") as f:
            json.dump(data, f, indent=1)
        os.replace(tmp, path)

    def graph_tag(self):
        """A short structural hash of the loaded graph: stored stream-plan picks are keyed by it, so that another net with
        the same input shape and step count cannot take them."""
        return graph_tag_of(self.layer, self.flow, [w.shape for w in self.weights])

    def tune_source(self):
        """Where this net's kernel choices came from, for run reports: "shipped" (every launch plan, algorithm and
        stream plan was in the database shipped for this device), "cache", or what had to be measured."""
        ctx = self.ctx
        _, plan_misses = ctx.tune_stats()
        for c in self._side:
            plan_misses += c.tune_stats()[1]
        base = "shipped" if getattr(ctx, "tuned_db", None) else None
        if ctx.tune_cache and os.path.exists(ctx.tune_cache):
            base = (base + " + cache") if base else "cache"
        miss = plan_misses + self.algo_misses + self.stream_misses
        if not miss:
            return base or "static heuristics (autotune off)"
        what = "autotuned: %d launch plans, %d conv algorithms, %d stream plans" % (plan_misses, self.algo_misses, self.stream_misses)
        return "%s; %s" % (base, what) if base else what

    def picking(self, mode):
        """Context: programs fused inside take the conv algorithms of `mode` ("throughput": the pipeline-judged table first)."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            prev, self._pick_mode = self._pick_mode, mode
            try:
                yield self
            finally:
                self._pick_mode = prev
        return cm()

    def compile(self, *xs, mode="latency"):
        """(see _compile: the plan's program is fused under this mode's conv algorithm tables)"""
        with self.picking(mode):
            return self._compile(*self._image_feeds(xs), mode=mode)

    def _compile(self, *xs, mode="latency"):
        """Build (or fetch) the captured plan for these device inputs.  `mode` only affects how
        the number of sub-batch streams is chosen: "latency" measures fork/join passes (what
        __call__ does), "throughput" measures free-running back-to-back passes."""
        key = (mode,) + tuple((a.shape, str(a.dtype)) for a in xs)
        plan = self._plans.get(key)
        if plan is not None:
            self._ensure_streams(plan)
            return plan
        xs = [a.materialise() if isinstance(a, ImageFeed) else a for a in xs]      # (a uint8 batch: compiled on its decoded form)
        ctx = self.ctx
        shapes = {k: a.shape for k, a in zip(self.input, xs)}
        shapes.update({k: w.shape for k, w in zip(self.inits, self.weights)})
        # unfused eager pass: validates the graph and records every shape.
        # ReLU works in place, so feed it copies, never the caller's arrays.
        timer = dict(self.timer)
        self._interpret(self._program, [a.copy() for a in xs], shapes=shapes)
        batch = xs[0].shape[0] if xs and xs[0].ndim else 0
        # A plan is (Q, P): the batch is cut into P sub-batches, each its own captured graph,
        # dealt round-robin onto Q streams.  Q > 1 lets two kernels overlap (one's tail and ramp
        # under the other's body); P > Q keeps per-kernel grids small enough to interleave well.
        splittable = batch > 0 and all(a.ndim and a.shape[0] == batch for a in xs)
        want = str(self.streams)
        if want == "auto":
            cands = [(1, 1)] + [(q, p_) for q, p_ in ((2, 2), (2, 4), (4, 4))
                                if splittable and batch % p_ == 0 and batch // p_ >= 4]
        elif want.startswith("pipe"):
            cands = []
        else:
            q, _, p_ = want.partition("x")
            q, p_ = int(q), int(p_ or q)
            cands = [(q, p_) if splittable and p_ >= q >= 1 and batch % p_ == 0 else (1, 1)]
        # throughput mode pipelines whole batches over R streams (R full-batch graphs); sub-batch plans
        # are dominated there (28.4 k vs 34.8 k img/s on ResNet-18), so they are not even tried
        # (depths: 3, 7 and 15 replicas interleave best -- depths that are multiples of the four hardware queues the runtime
        #  maps streams onto lose 3-8 %: ResNet-18 at batch 32 in steady state 52.3 / 53.1 / 53.6 k img/s at 3 / 7 / 15 against
        #  48.4 / 50.8 k at 4 / 8; YOLO-v3 at batch 1 1.54 / 1.60 / 1.64 k; a lone write-bound conv is best at 3)
        pipes = [2, 3, 7, 15] if (mode == "throughput" and want == "auto") else []
        if pipes:
            cands = [(1, 1)]
        if want.startswith("pipe"):
            cands, pipes = [], [int(want[4:] or 2)]
        # a stream plan chosen for this (mode, inputs, graph) before -- shipped database or the user's cache -- is taken
        # without measuring, so that consecutive runs time the same thing
        self._load_algo_cache()
        pick_key = repr((mode, [tuple(a.shape) for a in xs], "%d:%s" % (len(self.flow), self.graph_tag()), want))
        stored = self._streams_pick.get(pick_key) if want == "auto" else None
        if stored and stored.startswith("pipe") and mode == "throughput":
            cands, pipes = [], [int(stored[4:])]
        elif stored and "x" in stored:
            q, _, p_ = stored.partition("x")
            if (int(q), int(p_)) in cands:
                cands, pipes = [(int(q), int(p_))], []
        progs = {}

        def program_for(P):
            """The fused program with conv algorithms (direct vs Winograd) picked for the shapes a
            sub-batch of batch/P images really has."""
            if P not in progs:
                sub = dict(shapes)
                if P > 1:
                    for k, shp in shapes.items():
                        if k not in self.inits and shp and len(shp) >= 1 and shp[0] == batch:
                            sub[k] = (batch // P,) + tuple(shp[1:])
                progs[P] = self._fuse(sub, self.use_fusion)
            return progs[P]
        best = None
        todo = [("sub", c) for c in cands] + [("pipe", r) for r in pipes]
        for how, c in todo:
            if how == "sub":
                Q, P = c
                prog, nfused = program_for(P)
                try:
                    cand = self._build_plan(prog, xs, Q, P, nfused)
                except _NotSplittable:
                    continue
                except _lib.NotCapturable:
                    self._eager_prog[key[1:]] = program_for(1)[0]      # Net.__call__ runs this one eagerly
                    self.timer = timer
                    raise
            else:
                prog, nfused = program_for(1)
                reps = []
                try:
                    for r in range(c):
                        cx = self._side_context(r)
                        reps.append(self._capture(prog, [DeviceArray(a.shape, a.dtype, cx).copy_from(a) for a in xs],
                                                  cx, nfused))
                        ctx.synchronize()
                except MemoryError:
                    # a deep pipeline is R full copies of the activations: a candidate the device has no room for is
                    # skipped (a depth that was asked for by name is not)
                    if len(todo) == 1 or best is None:
                        raise
                    del reps
                    continue
                cand = _PipelinePlan(reps, ctx, nfused)
                self._probe_streams(cand, xs)
            if len(todo) == 1:
                best = cand
                break
            def burst(k):
                for _ in range(k):
                    if mode == "throughput":
                        cand.feed(xs)
                    cand.launch(join=mode != "throughput")
                cand.join()
                ctx.synchronize()
            burst(5)
            cand.ms = None
            # latency plans: best of five bursts of 10 passes.  Pipelined (throughput) plans are judged in steady
            # state -- best of three runs of 100 passes -- because a 10-pass burst is mostly pipeline fill and drain
            # and under-rates the deeper pipeline (host run-ahead is bounded by _Plan.max_in_flight)
            reps, depth = (3, 100) if how == "pipe" else (5, 10)
            for _ in range(reps):
                t0 = time.perf_counter()
                burst(depth)
                ms = (time.perf_counter() - t0) / depth * 1e3
                cand.ms = ms if cand.ms is None else min(cand.ms, ms)
            if os.environ.get("PLANER_PLAN_LOG"):
                import sys
                print("[planer_amd] plan candidate %s: %.4f ms/pass" % (cand.streams, cand.ms), file=sys.stderr)
            if best is None or cand.ms < best.ms:
                best = cand
        if len(todo) > 1 and want == "auto":
            self.stream_misses += 1
            self._streams_pick[pick_key] = best.streams
            self._algo_dirty = True
        self.timer = timer
        self._plans[key] = best
        # every pipeline candidate's probe rotated the process-wide side-stream pool for ITS depth: what is left is the last
        # candidate's assignment, not the winner's -- re-apply the one the winner was measured (and picked) under
        self._ensure_streams(best)
        if getattr(self, "_algo_dirty", False):
            self.save_algo_cache()
            self._algo_dirty = False
        return best

    def _probe_streams(self, plan, xs):
        """Which hardware queue the runtime put a stream on follows the order in which the process created its streams, and a
        pipeline's rate depends on where its replicas land (depth 7: 53.1 k img/s or 50.4 k) -- a host that
        created streams of its own first, or RCCL at world > 1, shifts the map.  So the replicas are not tied to the streams they
        were captured on: with three spare side streams behind the ones the pipeline needs, every rotation of the assignment
        (hip.set_side_stream_shift, 0..3 = one period of the four queues) runs the plan for a few milliseconds and the fastest
        stays.  PLANER_HIP_STREAM_PROBE=0 keeps creation order, =<s> forces a shift."""
        want = os.environ.get("PLANER_HIP_STREAM_PROBE", "auto")
        nrep = len(plan.replicas)
        if want == "0" or nrep < 2:
            return
        nside = nrep - 1 + 3
        dev, ctx = self.ctx.device, self.ctx

        def run(rounds):
            for _ in range(rounds * nrep):
                plan.feed(xs)
                plan.launch(join=False)
            plan.join()
            ctx.synchronize()
        if want != "auto":
            hip.set_side_stream_shift(dev, nside, int(want))
            plan.stream_probe = {"shift": int(want), "forced": True}
            return
        ms = []
        for s_ in range(4):
            hip.set_side_stream_shift(dev, nside, s_)
            run(1)
            best = None
            for _ in range(2):
                t0 = time.perf_counter()
                run(3)
                t = (time.perf_counter() - t0) / (3 * nrep) * 1e3
                best = t if best is None else min(best, t)
            ms.append(round(best, 5))
        pick = min(range(4), key=lambda i: ms[i])
        if ms[0] <= ms[pick] * 1.01:             # creation order unless another assignment is clearly (> 1 %) faster
            pick = 0
        hip.set_side_stream_shift(dev, nside, pick)
        plan.stream_probe = {"shift": pick, "ms_per_pass": ms}

    def _ensure_streams(self, plan):
        """The side-stream assignment is process-wide state (hip.set_side_stream_perm): another candidate's probe, or another
        Net's throughput plan compiled since, may have rotated it.  A pipeline plan carries the assignment it was measured
        under (`stream_probe`: shift over nrep + 2 side streams) and puts it back before it runs -- a few stream syncs, and only
        when something else changed it."""
        sp = getattr(plan, "stream_probe", None)
        if not isinstance(plan, _PipelinePlan) or not sp or "shift" not in sp:
            return
        n = len(plan.replicas) - 1 + 3
        want = [(i + int(sp["shift"])) % n for i in range(n)]
        if hip.side_stream_perm(self.ctx.device)[:n] != want:
            hip.set_side_stream_shift(self.ctx.device, n, sp["shift"])

    def _side_context(self, i):
        """Extra stream (context) number i of this net's device; 0 is the net's own."""
        while len(self._side) < i:              # the device's shared pool, in index order (hip.side_context)
            self._side.append(hip.side_context(self.ctx.device, len(self._side) + 1))
        return self.ctx if i == 0 else self._side[i - 1]

    def _build_plan(self, prog, xs, Q, S, nfused):
        """Q streams, S sub-batch graphs (S >= Q)."""
        if S == 1:
            return self._capture(prog, [DeviceArray(a.shape, a.dtype, self.ctx).copy_from(a) for a in xs],
                                 self.ctx, nfused)
        # S sub-batches on S streams: full-size static inputs/outputs live on the net's own
        # context; every sub-graph copies its input rows in and its output rows out itself.
        ctx0 = self.ctx
        full_in = [DeviceArray(a.shape, a.dtype, ctx0).copy_from(a) for a in xs]
        ctx0.synchronize()
        n = xs[0].shape[0] // S
        state = {"full_out": None}

        def dst_views(i, warm):
            outs = warm if isinstance(warm, tuple) else (warm,)
            if any(not isinstance(o, DeviceArray) or not o.ndim or o.shape[0] != n for o in outs):
                raise _NotSplittable()
            if state["full_out"] is None:
                state["full_out"] = [DeviceArray((n * S,) + o.shape[1:], o.dtype, ctx0) for o in outs]
            return [f.rows(i * n, (i + 1) * n) for f in state["full_out"]]

        subs = []
        for i in range(S):
            c = self._side_context(i % Q)
            # the sub-plan reads its rows of the full input in place: an alias view that belongs
            # to the side context, so every op that consumes it runs on the side stream
            statics = []
            for f in full_in:
                v = f.rows(i * n, (i + 1) * n)
                statics.append(DeviceArray(v.shape, v.dtype, c, v.ptr, f))
            subs.append(self._capture(prog, statics, c, nfused))
            dst_views(i, subs[-1].outputs)
        outs = state["full_out"]
        was_tuple = isinstance(subs[0].outputs, tuple)
        plan = _MultiPlan(full_in, tuple(outs) if was_tuple else outs[0], subs, ctx0, nfused)
        plan.streams = "%dx%d" % (Q, S)
        plan.out_rows = [[f.rows(i * n, (i + 1) * n) for f in outs] for i in range(S)]
        return plan

    def _capture(self, prog, statics, ctx, nfused, srcs=None, make_dsts=None):
        """Warm the pool / tuner with one eager pass of `prog` on `ctx`, then capture it."""
        def fill():
            if srcs is not None:
                for s_, v in zip(statics, srcs):
                    _lib.call("pl_d2d", ctx.handle, s_.ptr, v.ptr, s_.nbytes)
        fill()
        algos = []
        warm = self._interpret(prog, [s_.copy() for s_ in statics], record=algos)
        dsts = make_dsts(warm) if make_dsts else None
        del warm
        ctx.synchronize()
        # A static input is only copied first if a step could overwrite it in place.
        kinds = {b[0]: b[1] for b in prog_body(prog)}
        inplace = set()
        for src, names, dst in prog.flow:
            if kinds.get(_as_list(names)[0]) in ("relu", "relu_q4", "flatten", "identity", "return"):
                inplace.update(_as_list(src))
        self._pack_static_inputs(prog, statics, inplace)
        _lib.call("pl_capture_begin", ctx.handle)
        try:
            fill()
            work = []
            for k, s_ in zip(self.input, statics):
                if k in inplace:
                    s_ = DeviceArray(s_.shape, s_.dtype, ctx).copy_from(s_)
                work.append(s_)
            out = self._interpret(prog, work)
            del work
            if dsts is not None:
                for o, d in zip(out if isinstance(out, tuple) else (out,), dsts):
                    _lib.call("pl_d2d", ctx.handle, d.ptr, o.ptr, o.nbytes)
        except Exception:
            g = _lib.c_void_p()
            _lib.load().pl_capture_end(ctx.handle, _lib.byref(g))
            if g.value:
                _lib.load().pl_graph_destroy(g)
            raise
        g = _lib.c_void_p()
        _lib.call("pl_capture_end", ctx.handle, _lib.byref(g))
        plan = _Plan(statics, out, g, ctx, nfused)
        plan.algos = algos
        return plan

    def _pack_static_inputs(self, prog, statics, inplace):
        """A graph input whose ONLY reader is the row-packed stem conv (w_layout 6) gets its row-packed image
        as a persistent buffer beside it (`static.packed`): the captured conv reads that image, the re-layout kernel stays
        out of the graph and runs when the plan is fed (`_feed_static`) -- as the copy that brings the batch in.
        PLANER_HIP_FEED_PACK=0 keeps the re-layout inside the graph."""
        if os.environ.get("PLANER_HIP_FEED_PACK", "1") == "0":
            return
        for k, s_ in zip(self.input, statics):
            readers = [(src, names) for src, names, dst in prog.flow if k in _as_list(src)]
            if len(readers) != 1 or k in inplace or s_.packed is not None or len(s_.shape) != 4 or s_.base is not None:
                continue
            src, names = readers[0]
            obj = prog.objs[_as_list(names)[0]]
            para = obj.para()
            if (obj.name == "conv_pool_q4" and para.get("w_layout") == 12 and _as_list(src)[0] == k and _as_list(src).count(k) == 1
                    and s_.prefed is None and s_.ptr % 16 == 0 and os.environ.get("PLANER_HIP_FEED_STEM", "1") != "0"):
                # the stem + max-pool kernel reads NCHW itself: it leaves the graph and runs when the plan is fed, straight
                # from the caller's batch; the captured pass starts from its (persistent) pooled tensor
                env = {"None": None}
                env.update(zip(self.inits, self.weights))
                env.update(self._extra)
                args = [env.get(a) for a in (_as_list(src)[1:5] + ["None"] * 4)[:4]]
                fpara = {a: b for a, b in para.items() if a != "w_layout"}
                pooled = _q4.ConvPoolQ4(s_, *args, w_layout=12, **fpara)
                s_.prefed = (_q4.stem_pool_feeder(s_.shape, args[0], args[1], args[2], args[3], fpara.get("act", 0),
                                                  fpara.get("alpha", 0.0), pooled, fpara.get("strip_rows", 0)), pooled)
                continue
            if (obj.name not in ("conv_q4", "conv_pool_q4") or para.get("w_layout") not in (6, 10) or _as_list(src)[0] != k
                    or _as_list(src).count(k) != 1):
                continue
            kw = self._shape_of_init(_as_list(src)[1])[3]
            strides, pads = para.get("strides", (1, 1)), para.get("pads", (0, 0, 0, 0))
            _q4.pack_rows(s_, geom=(int(kw), int(strides[1]), int(pads[0]), int(pads[1])))

    def _shape_of_init(self, key):
        v = dict(zip(self.inits, self.weights)).get(key)
        if v is None:
            v = self._extra[key]
        return v.shape

    def _replay(self, xs, private=True):
        # private copies (the plan's buffers are rewritten by the next replay) unless the caller copies to the host right away;
        # a declared uint8 output is encoded into a fresh array either way
        return self._hand_back(self._launch(xs).outputs, private)

    def _launch(self, xs, declared=True):
        """One pass of the plan for `xs`, joined into the net's own stream; the plan (its outputs are the plan's own buffers).
        `declared`: the outputs are checked against the declared output forms before anything is launched."""
        plan = self.compile(*xs)
        if declared and (self._image_out or self._detect is not None):
            self._check_outputs(plan.outputs)          # (before anything is launched)
        if isinstance(plan, _PipelinePlan):
            # the replica whose turn it is gets the inputs (plan.inputs are those of the replica launched LAST);
            # its stream first waits for the main stream, where the caller produced xs
            plan.replicas[plan.turn].ctx.wait_for(self.ctx)
            plan.feed(xs)
        else:
            self._feed_on_main(plan, xs)
        plan.launch()
        return plan

    def _feed_on_main(self, plan, xs):
        """Inputs of a one-graph or sub-batch plan, copied on the net's OWN stream (where the caller produced them);
        `launch()` forks the side streams behind that point."""
        for s, a in zip(plan.inputs, xs):
            if isinstance(a, ImageFeed):                 # decoded into the static tensor, then the feed pass from there
                _feed_static(self.ctx, s, a)
            elif isinstance(plan, _MultiPlan) or not isinstance(a, DeviceArray):
                if a is not s:
                    s.copy_from(a)
                if s.prefed is not None or s.packed is not None:        # (a host array: through the static tensor, then the feed pass)
                    _feed_static(self.ctx, s, s)
            else:
                _feed_static(self.ctx, s, a)
        for sp in (plan.subs if isinstance(plan, _MultiPlan) else (plan,)):
            sp._fed = True

    def submit(self, *x):
        """Asynchronous form of `net(x)` (net.py:94-101): enqueue one forward pass and return a `Pending` handle at once.
        Consecutive submits rotate over the replicas of the throughput plan (R full-batch graphs on R streams,
        `compile(mode="throughput")`), so one batch's tails and memory-bound layers run under the next one's convs --
        a loop of submits reaches the rate `bench.py` reports for the plan API.  Each handle owns private copies of its
        outputs (the replica's buffers are rewritten R submits later)."""
        if type(x[0]) is dict:
            x = [x[0][i] for i in self.input]
        host = [isinstance(i, numpy.ndarray) for i in x]
        plan = None
        route = os.environ.get("PLANER_HIP_HOST_ROUTE", "direct")          # direct | staged | plain (A/B: tools/host_submit_probe.py)
        direct = False
        if any(host) and self.use_graph and not self.profile and route != "plain":
            # a pipeline compiled for this signature: a host batch goes straight into an input buffer that belongs to the
            # replica whose turn it is -- a synchronous DMA on NO stream (pl_h2d_direct: the host waits 0.35 ms for a 19 MB
            # batch while the other replicas compute; a copy enqueued on a stream would hold that stream's hardware queue, and
            # the replica that shares it, for as long).  The buffer is free once the replica's previous feed has read it.
            hx = [numpy.require(i, requirements="C") if b else i for i, b in zip(x, host)]
            plan = self._plans.get(("throughput",) + self._signature(hx))
            if isinstance(plan, _PipelinePlan) and route == "staged":       # pinned ring + DMA on the replica's stream (pl_h2d_staged)
                self._ensure_streams(plan)
                xs = self._image_feeds(hip.asarray(i, ctx=self.ctx, consumer=plan.replicas[plan.turn].ctx) if b else i
                                       for i, b in zip(hx, host))
            elif isinstance(plan, _PipelinePlan):
                self._ensure_streams(plan)
                rp, direct = plan.replicas[plan.turn], True
                if rp.host_in is None:
                    rp.host_in, rp.fed = [None] * len(hx), hip.Event(rp.ctx)
                else:
                    rp.fed.synchronize()              # (recorded R submits ago)
                xs = []
                for i, (a, b) in enumerate(zip(hx, host)):
                    if b:
                        d = rp.host_in[i]
                        if d is None or d.shape != a.shape or d.dtype != a.dtype:
                            d = rp.host_in[i] = DeviceArray(a.shape, a.dtype, rp.ctx)
                            rp.ctx.synchronize()      # (a fresh pool block: its previous reader was enqueued on this stream)
                        if a.nbytes:
                            _lib.call("pl_h2d_direct", rp.ctx.handle, d.ptr, a.ctypes.data, a.nbytes)
                        a = d
                    xs.append(a)
                xs = self._image_feeds(xs)            # (a uint8 batch is decoded out of the replica's upload buffer)
            else:
                plan = None
        if plan is None:
            xs = self._image_feeds(hip.asarray(i, ctx=self.ctx) if b else i for i, b in zip(x, host))
            if self.use_graph and not self.profile:
                try:
                    plan = self.compile(*xs, mode="throughput")
                except _lib.NotCapturable:
                    self.use_graph = False
        if plan is None:                              # flows that need the host between kernels: run now, hand back a finished handle
            return Pending(self, self(*x), None, any(host), final=True)
        if self._image_out or self._detect is not None:
            self._check_outputs(plan.outputs)         # (before anything is launched)
        if isinstance(plan, _PipelinePlan):
            rp = plan.replicas[plan.turn]
            if not (direct and all(host)):
                rp.ctx.wait_for(self.ctx)             # the caller produced xs on the net's own stream
            plan.feed(xs)
            if direct:
                rp.fed.record()                       # the replica's upload buffers are free again behind this point
            # what the feed read stays referenced until the replica has read it (the replica's own upload buffers live on anyway)
            keep = [a for a, b in zip(xs, host) if not (direct and b)]
            plan.launch(join=False, hold=keep or None)
            cx, out = rp.ctx, rp.outputs
        else:
            # sub-batch plans ("QxP"): the copy runs on the net's own stream, the sub-streams fork behind it and join
            # back into it (the feed of _MultiPlan.feed on the side streams could read xs before the main stream wrote them)
            self._feed_on_main(plan, xs)
            plan.launch()
            cx, out = self.ctx, plan.outputs
        # private copies (declared uint8 outputs: encoded) on the replica's stream, then the marker result() waits for
        outs = self._hand_back(out, True)
        ev = self._events.pop() if self._events else hip.Event(cx)      # a marker can be recorded on any stream of its device
        _lib.call("pl_event_record", cx.handle, ev.handle)
        tickets = None
        if any(host):                                 # host in -> host out: the copies back start now, behind this pass
            seq = outs if isinstance(outs, tuple) else (outs,)
            tickets = [o.get_begin(producer=cx) if isinstance(o, DeviceArray) else None for o in seq]
        return Pending(self, outs, ev, any(host), tickets=tickets)

    def _eager_program(self, xs):
        """The fused program for THESE input shapes (conv algorithms, Winograd chaining, row packing and the fusions are
        all decided per shape, so a program fused for one image size must not run another): built on first sight of a
        signature like a plan is, from an unfused pass that records every shape."""
        sig = tuple((a.shape, str(a.dtype)) for a in xs)
        prog = self._eager_prog.get(sig)
        if prog is None:
            shapes = {k: a.shape for k, a in zip(self.input, xs)}
            shapes.update({k: w.shape for k, w in zip(self.inits, self.weights)})
            timer = dict(self.timer)
            self._interpret(self._program, [a.copy() for a in xs], shapes=shapes)     # ReLU works in place: copies
            self.timer = timer
            prog = self._eager_prog[sig] = self._fuse(shapes, self.use_fusion)[0]
        return prog

    # ---- entry point ---------------------------------------------------------------------
    def __call__(self, *x, **key):
        """net.py:94-101."""
        if type(x[0]) is dict:
            x = [x[0][i] for i in self.input]
        host = [isinstance(i, numpy.ndarray) for i in x]
        need = any(host)
        if need:
            x = [hip.asarray(i, ctx=self.ctx) if b else i for i, b in zip(x, host)]
        x = self._image_feeds(x)
        graphable = (self.use_graph and not key.get("debug") and not self.profile
                     and all(isinstance(i, (DeviceArray, ImageFeed)) for i in x))
        if graphable:
            try:
                rst = self._replay(list(x), private=not need)          # host in -> host out: .get() reads the plan's buffers
            except _lib.NotCapturable:
                # post-processing graphs (NonZero, uploads of host-computed index lists) need the host between
                # kernels: the FUSED program (same kernels, layouts and algorithm picks as the plan) is launched
                # step by step from here on
                self.use_graph = graphable = False
        if not graphable:
            x = [i.materialise() if isinstance(i, ImageFeed) else i for i in x]      # eager routes: a fresh decoded array
            if self._eager_prog and not key.get("debug") and not self.profile and all(isinstance(i, DeviceArray) for i in x):
                rst = self._interpret(self._eager_program(list(x)), list(x))
            else:
                rst = self.forward(*x, **key)
            if self._image_out or self._detect is not None:
                rst = self._hand_back(rst, False)
        if need:
            rst = tuple(i.get() for i in rst) if isinstance(rst, tuple) else rst.get()
        return rst[0] if len(rst) == 1 else rst

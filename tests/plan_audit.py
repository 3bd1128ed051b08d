"""Step-by-step float64 audit of a compiled plan program.

The per-family tests (tests/ref64.py, tests/ref64_ops.py) call each kernel on operands the test built; a forward pass runs
them on operands the plan compiler built (plan.compile_front and plan.lower: fuse_flow, assign_layouts, conv_layouts.choose,
pair_sibling_convs, chain_winograd, fuse_conv1x1_wino_in, the stem + max-pool and upsample/concat peepholes).  The audit runs the program a
captured plan runs, step by step, and checks every step against float64 computed from the inputs that step really read:

* `capture(net, xs, mode)` builds the program exactly as Net._compile does for one sub-batch (under `net.picking(mode)`) and
  interprets it eagerly (Net._interpret), recording each step's inputs BEFORE the call (ReLU and Clip rewrite theirs in
  place) and its outputs after it, copied to the host for the images `sample(N)` = {0, N - 1} only: every op of these nets
  is per image, and the last image is where indexing goes wrong;
* `audit(trace, inits)` walks the recorded steps:
  - every channel-quad (Q4) output must have exact zeros in the padding lanes of a partial last quad;
  - every input must be what its producer wrote (or what an in-place step made of it since);
  - conv steps: tests/ref64.ref64 + ref64.bound with the lam of the step's w_layout family, from the layer's own inputs and
    the ORIGINAL OIHW filter (the init key without its @... suffix); ConvTranspose through the zero-stuffed form of
    tests/test_gpu_convtranspose.py; stem + max-pool: the pooled reference, the bound pooled the same way;
  - the staged Winograd stages X@in -> X@gemm -> X@out are one conv from X@in's input to X@out's output, X@chain closes one
    conv and opens the next, conv1x1_wino_in (@v4) is the 1x1 conv followed by its 3x3 conv, A&B is two convs on one input.
    A tensor the plan never writes (keep_y False, the 1x1 output inside @v4) is computed in float64 from its producer's
    inputs, and its bound is carried into the next conv as |scale| * conv(tol, |K|) (ReLU / leaky are 1-Lipschitz);
  - ops that round once (ReLU, leaky, max / average pool, add, concat, nearest upsample, batchnorm, clip, layout
    conversions, flatten) must equal the oracle's float32 op on the same inputs bit for bit; GAP, sigmoid and dense are
    checked against tests/ref64_ops bounds.
  A failure names the step, its kind, w_layout and launch plan, and the worst element (n, c, y, x) with its err / tol.
  -> {family: worst err / tol}, plus the census of w_layouts the program ran.

The CPU tests (tests/test_plan_audit.py) feed the same audit a trace made by `cpu_trace`: the program built by the same
two functions with the host's answers (`cpu_program`) and interpreted with numpy stand-ins (the oracle's float32 ops, Q4
values packed by numpy)."""
import collections

import numpy as np

from oracle import planer_np as onp
from planer_amd import conv_layouts as cl
from tests import ref64 as R
from tests import ref64_ops as RO

# w_layout code -> lam family of tests/ref64.py
FAMILY = {0: "direct", 1: "direct", 2: "direct", 6: "direct", 10: "direct", 12: "direct", 13: "direct", 14: "direct",
          3: "f2x2", 4: "f2x2", 7: "f4x4", 9: "f4x4", 8: "w1d4", 11: "wino43"}
STAGED = {"wino4": cl.WINO4_Q4, "wino43": cl.WINO43_Q4}
CONV_KINDS = ("conv", "conv_fused", "conv_q4")
CONVT_KINDS = ("convtranspose", "convt_fused", "convt_q4")
EXACT = ("relu", "leakyrelu", "maxpool", "averagepool", "add", "concat", "upsample", "batchnorm", "clip", "flatten")
IN_PLACE = ("relu", "relu_q4", "clip", "clip_q4")


class Q4Host:
    """A channel-quad tensor on the host: data (n, ceil(c/4), h, w, 4), `chan` = c."""

    def __init__(self, data, chan):
        self.data, self.chan = data, int(chan)

    def nchw(self):
        n, cq, h, w, _ = self.data.shape
        return np.ascontiguousarray(self.data.transpose(0, 1, 4, 2, 3).reshape(n, cq * 4, h, w)[:, :self.chan])


def pack_q4(x):
    n, c, h, w = x.shape
    cq = -(-c // 4)
    buf = np.zeros((n, cq * 4, h, w), np.float32)
    buf[:, :c] = x
    return Q4Host(np.ascontiguousarray(buf.reshape(n, cq, 4, h, w).transpose(0, 1, 3, 4, 2)), c)


def nchw(v):
    return v.nchw() if isinstance(v, Q4Host) else v


def sample(n):
    return sorted({0, n - 1})


class Step:
    """One executed layer: kind, para, source / destination keys, the host values it read and wrote (None for constants
    and Winograd-domain tensors), and the launch plan string of a conv."""

    def __init__(self, name, kind, para, src, dst, ins, outs, plan=""):
        self.name, self.kind, self.para, self.src, self.dst = name, kind, dict(para), list(src), list(dst)
        self.ins, self.outs, self.plan = ins, outs, plan


def _as_list(v):
    return list(v) if isinstance(v, (list, tuple)) else [v]


def _steps_of(prog):
    for src, names, dst in prog.flow:
        for pos, name in enumerate(_as_list(names)):
            yield name, (src if pos == 0 else dst), dst


# ---- capture on the GPU ----------------------------------------------------------------------------------------------------
def program(net, xs, mode="latency"):
    """The fused program a captured plan of these device inputs runs (Net._compile, one sub-batch) -> (prog, shapes)."""
    shapes = {k: a.shape for k, a in zip(net.input, xs)}
    shapes.update({k: w.shape for k, w in zip(net.inits, net.weights)})
    net._interpret(net._program, [a.copy() for a in xs], shapes=shapes)
    with net.picking(mode):
        prog, _ = net._fuse(shapes, net.use_fusion)
    return prog, shapes


def capture(net, xs, mode="latency"):
    """-> (trace, output of the eager run as host arrays).  xs: device arrays."""
    from planer_amd import q4
    from planer_amd.hip import DeviceArray
    prog, _ = program(net, xs, mode)
    consts = set(net.inits) | set(net._extra)
    batch = xs[0].shape[0]
    idx = sample(batch)

    def host(a, key):
        if not isinstance(a, DeviceArray) or key in consts or key.endswith(("@V", "@M")) or a.meta is not None:
            return None
        v = a.get()
        if v.ndim and v.shape[0] == batch:
            v = np.ascontiguousarray(v[idx])
        return Q4Host(v, a.chan) if q4.is_q4(a) else v

    order = list(_steps_of(prog))
    trace, pos = [], [0]

    class Probe:
        def __init__(self, obj):
            self.obj, self.name = obj, obj.name

        def para(self):
            return self.obj.para()

        def __call__(self, *args):
            name, keys, dst = order[pos[0]]
            pos[0] += 1
            keys = _as_list(keys)
            ins = [host(a, k) for a, k in zip(args, keys)]
            val = self.obj(*args)
            outs = [host(v, k) for v, k in zip(_as_list(val), _as_list(dst))]
            plan = net.ctx.last_conv_plan() if "conv" in self.name or "wino" in self.name or self.name == "dense" else ""
            trace.append(Step(name, self.name, self.obj.para(), keys, _as_list(dst), ins, outs, plan))
            return val

    prog.objs = {name: Probe(obj) for name, obj in prog.objs.items()}
    out = net._interpret(prog, list(xs))
    out = tuple(o.get() for o in out) if isinstance(out, tuple) else (out.get(),)
    return trace, out


def host_inits(net):
    return {k: (w.host if w.host is not None else w.get()) for k, w in zip(net.inits, net.weights)}


# ---- the checks ----------------------------------------------------------------------------------------------------------
class AuditError(AssertionError):
    pass


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def _conv_para(para):
    return dict(group=int(para.get("group", 1)), strides=list(para.get("strides", (1, 1))),
                dilations=list(para.get("dilations", (1, 1))), pads=list(para.get("pads", (0, 0, 0, 0))))


class _Layer:
    """A logical conv: input (observed values, or a float64 reference with the bound it carries), filter and tail."""

    def __init__(self, x, x_tol, K, B, scale, shift, res, para, w_layout, transposed=False):
        self.x, self.x_tol, self.K, self.B, self.scale, self.shift, self.res = x, x_tol, K, B, scale, shift, res
        self.para, self.w_layout, self.transposed = para, w_layout, transposed

    def expect(self):
        """-> (float64 reference, per-element tolerance)."""
        p = self.para
        act, alpha = int(p.get("act", 0)), float(p.get("alpha", 0.0))
        lam = R.LAMBDA[FAMILY[self.w_layout]]
        x, K = _f64(self.x), _f64(self.K)
        if self.transposed:
            from tests.test_gpu_convtranspose import stuffed
            x, K = stuffed(x, K, list(p.get("strides", (2, 2))), list(p.get("pads", (0, 0, 0, 0))),
                           list(p.get("output_padding", (0, 0))))
            conv = {}
        else:
            conv = _conv_para(p)
        ref = R.ref64(x, K, self.B, self.scale, self.shift, self.res, act=act, alpha=alpha, **conv)
        tol = R.bound(x, K, self.B, self.scale, self.shift, self.res, lam=lam, **conv)
        if self.x_tol is not None:
            s = np.abs(_f64(self.scale)).reshape(1, -1, 1, 1) if self.scale is not None else 1.0
            xt = self.x_tol
            if self.transposed:
                xt = stuffed(xt, K, list(p.get("strides", (2, 2))), list(p.get("pads", (0, 0, 0, 0))),
                             list(p.get("output_padding", (0, 0))))[0]
            tol = tol + s * R.conv64(xt, np.abs(K), **conv)
        return ref, tol


class Audit:
    def __init__(self, inits):
        self.inits = inits
        self.worst = collections.defaultdict(float)
        self.census = collections.Counter()
        self.produced = {}          # key -> NCHW values its producer wrote (updated by in-place steps)
        self.vsrc = {}              # Winograd-domain key -> (input values, carried tolerance or None)
        self.open = {}              # staged conv base name -> its _Layer under construction

    # -- helpers
    def const(self, key):
        if key == "None":
            return None
        base = key.split("@")[0]
        return self.inits[key] if key in self.inits else self.inits[base]

    def fail(self, step, msg):
        raise AuditError("step %s (%s, w_layout %s, plan %r): %s" % (step.name, step.kind, step.para.get("w_layout"),
                                                                     step.plan, msg))

    def record(self, fam, worst):
        self.worst[fam] = max(self.worst[fam], float(worst))

    def compare(self, step, what, fam, got, ref, tol):
        try:
            self.record(fam, R.check(got, ref, tol, "%s %s" % (step.name, what), step.plan))
        except AssertionError as e:
            self.fail(step, "%s family %s: %s" % (what, fam, e))

    def exact(self, step, what, got, want):
        got, want = np.asarray(got), np.asarray(want, np.float32)
        if got.shape != want.shape:
            self.fail(step, "%s: shape %s != %s" % (what, got.shape, want.shape))
        bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        if bad.any():
            i = tuple(int(v) for v in np.argwhere(bad)[0])
            self.fail(step, "%s: element %s = %r, want %r bit for bit (%d elements differ)"
                      % (what, i, float(got[i]), float(want[i]), int(bad.sum())))
        self.record("exact", 0.0)

    def arg(self, step, i):
        """Input i of a step: observed values (NCHW) or a constant."""
        if i >= len(step.src) or step.src[i] == "None":
            return None
        v = step.ins[i]
        return nchw(v) if v is not None else self.const(step.src[i])

    # -- the walk
    def run(self, trace):
        for step in trace:
            self.inputs_are_what_was_written(step)
            self.padding(step)
            self.check(step)
            for k, v in zip(step.dst, step.outs):
                if v is not None:
                    self.produced[k] = nchw(v)
            if step.kind in IN_PLACE and step.outs[0] is not None:
                self.produced[step.src[0]] = nchw(step.outs[0])
        return dict(self.worst), self.census

    def inputs_are_what_was_written(self, step):
        for i, (k, v) in enumerate(zip(step.src, step.ins)):
            if v is None or k not in self.produced:
                continue
            want, got = self.produced[k], nchw(v)
            if got.shape != want.shape or not ((got == want) | (np.isnan(got) & np.isnan(want))).all():
                self.fail(step, "input %d (%s) is not what its producer wrote" % (i, k))

    def padding(self, step):
        for k, v in zip(step.dst, step.outs):
            if isinstance(v, Q4Host) and v.chan % 4:
                pad = v.data[:, -1, :, :, v.chan % 4:]
                if (pad != 0).any() or np.isnan(pad).any():
                    n, y, x, lane = (int(t) for t in np.argwhere((pad != 0) | np.isnan(pad))[0])
                    self.fail(step, "output %s (C=%d): padding lane %d of the last quad is %r at (n %d, y %d, x %d)"
                              % (k, v.chan, v.chan % 4 + lane, float(pad[n, y, x, lane]), n, y, x))

    def conv_check(self, step, layer, got, what="output"):
        ref, tol = layer.expect()
        self.census[layer.w_layout] += 1
        self.compare(step, what, FAMILY[layer.w_layout], nchw(got), ref, tol)

    def layer(self, step, off, para, w_layout, x=None, x_tol=None, transposed=False, res=True):
        """_Layer from step inputs [x?, K, B, scale, shift, res] starting at `off` (x at off - 1 unless given)."""
        if x is None:
            x = self.arg(step, off - 1)
        tail = [self.arg(step, off + j) for j in range(1, 5 if res else 4)] + ([] if res else [None])
        return _Layer(x, x_tol, self.const(step.src[off]), *tail, para=para, w_layout=w_layout, transposed=transposed)

    def check(self, step):
        k, p = step.kind, step.para
        base = k[:-3] if k.endswith("_q4") else k
        if k in CONV_KINDS:
            lay = int(p.get("w_layout", cl.IGEMM_NCHW))
            self.conv_check(step, self.layer(step, 1, p, lay), step.outs[0])
        elif k in CONVT_KINDS:
            self.conv_check(step, self.layer(step, 1, p, int(p.get("w_layout", cl.CONVT_Q4)), transposed=True), step.outs[0])
        elif k == "conv_pool_q4":
            L = self.layer(step, 1, p, int(p["w_layout"]), res=False)
            ref, tol = L.expect()
            pool = dict(w=[3, 3], strides=[2, 2], pads=[1, 1, 1, 1])
            self.census[L.w_layout] += 1
            self.compare(step, "pooled output", FAMILY[L.w_layout], nchw(step.outs[0]), onp.maxpool(ref, **pool),
                         onp.maxpool(tol, **pool))
        elif k == "conv_q4_pair":
            x = self.arg(step, 0)
            for j, (pk, out) in enumerate(zip(("para1", "para2"), step.outs)):
                L = self.layer(step, 1 + 4 * j, p[pk], int(p[pk].get("w_layout", cl.DIRECT_Q4)), x=x, res=False)
                self.conv_check(step, L, out, "output %d" % (j + 1))
        elif k in ("wino4_in", "wino43_in"):
            self.vsrc[step.dst[0]] = (self.arg(step, 0), None)
        elif k in ("wino4_gemm", "wino43_gemm"):
            x, x_tol = self.vsrc.pop(step.src[0])
            self.open[step.name[:-len("@gemm")]] = (x, x_tol, self.const(step.src[1]), STAGED[k[:-len("_gemm")]])
        elif k in ("wino4_out", "wino43_out", "wino4_chain", "wino43_chain"):
            x, x_tol, K, lay = self.open.pop(step.name.rsplit("@", 1)[0])
            L = _Layer(x, x_tol, K, *[self.arg(step, j) for j in range(1, 5)], para=dict(p, pads=[1, 1, 1, 1]), w_layout=lay)
            if k.endswith("_out") or p.get("keep_y", True):
                self.conv_check(step, L, step.outs[0])
                if k.endswith("_chain"):
                    self.vsrc[step.dst[1]] = (nchw(step.outs[0]), None)
            else:                                          # y is never written: its reference and bound go to the next conv
                self.census[lay] += 1
                self.vsrc[step.dst[0]] = L.expect()
        elif k == "conv1x1_wino_in":
            L = self.layer(step, 1, dict(p), cl.DIRECT_Q4, res=False)
            self.census[cl.DIRECT_Q4] += 1
            self.vsrc[step.dst[0]] = L.expect()
        elif k in ("to_q4", "from_q4"):
            self.exact(step, "conversion", nchw(step.outs[0]), self.arg(step, 0))
        elif k == "upconcat_q4":
            up = onp.upsample(self.arg(step, 0).copy(), self.arg(step, 1), mode="nearest")
            self.exact(step, "upsample + concat", nchw(step.outs[0]), onp.concat(up, self.arg(step, 2), axis=1))
        elif base in EXACT:
            if base == "upsample" and p.get("mode", "nearest") != "nearest":
                self.fail(step, "no audit for upsample mode %r" % p.get("mode"))
            args = [None if a is None else np.array(a, np.float32) for a in (self.arg(step, i) for i in range(len(step.src)))]
            self.exact(step, "output", nchw(step.outs[0]), onp.OPS[base](*args, **p))
        elif base == "gap":
            x = _f64(self.arg(step, 0))
            n, c = x.shape[:2]
            rows = x.reshape(n * c, -1)
            self.compare(step, "output", "gap", nchw(step.outs[0]), RO.reduce64(rows, 1).reshape(n, c, 1, 1),
                         RO.mean_bound(rows).reshape(n, c, 1, 1))
        elif base == "sigmoid":
            ref = 1.0 / (1.0 + np.exp(-_f64(self.arg(step, 0))))
            self.compare(step, "output", "sigmoid", nchw(step.outs[0]), ref, RO.ulp_bound(ref, "sigmoid"))
        elif k == "dense":
            x, K, B = _f64(self.arg(step, 0)), _f64(self.arg(step, 1)), _f64(self.arg(step, 2))
            n, o = x.shape[0], K.shape[0]
            x4, K4 = x.reshape(n, -1, 1, 1), K.reshape(o, -1, 1, 1)
            self.compare(step, "output", "dense", step.outs[0], (x @ K.T + B).reshape(n, o),
                         R.bound(x4, K4, B).reshape(n, o))
        elif k == "return":
            pass
        else:
            self.fail(step, "no audit for this kind")


def audit(trace, inits):
    """-> ({family: worst err / tol}, Counter of w_layouts).  Raises AuditError on the first step that is wrong."""
    return Audit(inits).run(trace)


# ---- the same program on the host (CPU tests) ------------------------------------------------------------------------------
def _conv_np(x, K, B=None, scale=None, shift=None, res=None, act=0, alpha=0.0, **para):
    from tests.test_plan_fusion import conv_fused_np
    conv = _conv_para(para)
    return conv_fused_np(np.asarray(x, np.float32), K, B, scale, shift, res, act, alpha, **conv)


def cpu_front(graph, blob, x, force=False, **kw):
    """plan.compile_front on this graph, as Net._fuse calls it: shapes from one oracle pass, `values` from the blob; `kw`: its
    `stop`, `worth`, `fuse`.  -> (body, flow, counts, shapes)"""
    from planer_amd.plan import compile_front
    from tests.test_plan_fusion import shapes_of
    shapes = shapes_of(graph, blob, x)
    body, flow, counts = compile_front(graph["layers"], graph["flow"], [i[0] for i in graph["inits"]], shapes,
                                       q4="force" if force else True, values=blob_inits(graph, blob).get, **kw)
    return body, flow, counts, shapes


def cpu_program(graph, blob, x, pick=lambda cands: cands[0], force_q4=False):
    """The program Net compiles for this graph, on the host: plan.compile_front, then plan.lower with `pick` in place of the
    timing and the host's answers for the rest (no stem + max-pool kernel, every map fits the chained transform).
    -> (body, flow, shapes)"""
    from planer_amd.plan import lower
    body, flow, _, shapes = cpu_front(graph, blob, x, force_q4)
    body, flow, _ = lower(body, flow, [i[0] for i in graph["inits"]], shapes, pick=lambda cands, *_: pick(cands))
    return body, flow, shapes


def steps_of(body, flow):
    """[(kind, para, srcs, dst, name)] in flow order."""
    k = {b[0]: b for b in body}
    return [(k[names[0]][1], k[names[0]][2], _as_list(src), dst, names[0]) for src, names, dst in flow]


def kinds_of(body, flow):
    return [s[0] for s in steps_of(body, flow)]


def run_on_oracle(graph, blob, x, body, flow, **standins):
    """The program (body, flow) on the numpy oracle: plan-internal kinds as their NCHW operators (test_plan_fusion._q4_standins),
    plus the stand-ins given by kind."""
    from tests.test_plan_fusion import _q4_standins
    saved = dict(onp.OPS)
    onp.OPS.update(_q4_standins())
    onp.OPS.update(standins)
    try:
        net = onp.OracleNet()
        net.load_json(graph["input"], graph["inits"], body, flow)
    finally:
        onp.OPS.clear()
        onp.OPS.update(saved)
    net.load_weights(blob)
    return net(x.copy())


Q4_OUT = ("conv_q4", "convt_q4", "conv_pool_q4", "upconcat_q4", "to_q4", "wino4_out", "wino43_out", "wino4_chain", "wino43_chain")


def cpu_trace(graph, blob, x, body, flow, fault=None, conv=None):
    """Interpret (body, flow) with numpy stand-ins and record a trace for `audit`, sampled like `capture`.  Channel-quad
    kinds produce Q4Host values packed by numpy; a Winograd-domain tensor is carried as the NCHW values it stands for.
    `fault(step, outs) -> outs` may change what a step writes (planted faults); `conv` replaces the conv stand-in.
    -> (trace, outputs)"""
    conv = conv or (lambda step, *a, **kw: _conv_np(*a, **kw))
    env = {"None": None}
    env.update(blob_inits(graph, blob))
    inits = {k for k, _, _ in graph["inits"]}
    env[graph["input"][0]] = x.copy()
    kinds = {b[0]: b for b in body}
    idx = sample(x.shape[0])
    batch = x.shape[0]

    def get(k):
        if k in env:
            return env[k]
        return env[k.split("@")[0]]                      # a prepared filter: the stand-ins use the OIHW init

    def host(v, k):
        if (k in inits or (k != "None" and k.split("@")[0] in inits) or k.endswith(("@V", "@M")) or v is None
                or isinstance(v, tuple)):
            return None
        if isinstance(v, Q4Host):
            return Q4Host(np.ascontiguousarray(v.data[idx]).copy(), v.chan)
        v = np.asarray(v)
        return np.ascontiguousarray(v[idx]) if v.ndim and v.shape[0] == batch else v.copy()

    trace, out_key = [], None
    for src, names, dst in flow:
        for pos, name in enumerate(_as_list(names)):
            keys = _as_list(src if pos == 0 else dst)
            _, kind, para = kinds[name]
            args = [get(k) for k in keys]
            ins = [host(a, k) for a, k in zip(args, keys)]
            step = Step(name, kind, para, keys, _as_list(dst), ins, [])
            outs = _standin(step, args, conv)
            if fault is not None:
                outs = fault(step, outs)
            for k, v in zip(step.dst, outs):
                env[k] = v
            step.outs = [host(v, k) for v, k in zip(outs, step.dst)]
            trace.append(step)
        out_key = dst
    outs = tuple(nchw(v) for k in _as_list(out_key) for v in (env[k] if isinstance(env[k], tuple) else (env[k],)))
    return trace, outs


def _offsets(inits):
    out, o = [], 0
    for _, s, dt in inits:
        out.append(o)
        o += int(np.prod(s, dtype=np.int64)) * np.dtype(dt).itemsize
    return out


def _standin(step, args, conv):
    k, p = step.kind, step.para
    a = [nchw(v) if isinstance(v, Q4Host) else v for v in args]
    q4 = k in Q4_OUT or (k.endswith("_q4") and k not in ("gap_q4", "from_q4"))
    cp = {key: v for key, v in p.items() if key not in ("w_layout", "rowpack", "strip_rows", "keep_y", "wino")}
    if k in ("relu_q4", "clip_q4") or k in ("relu", "clip"):
        v = args[0]
        buf = v.data if isinstance(v, Q4Host) else v
        buf[...] = onp.OPS[k.replace("_q4", "")](buf.copy(), **p)          # in place, like the kernels
        return [v]
    if k in CONV_KINDS:
        y = conv(step, *a[:1], a[1], *(a[2:] + [None] * (6 - len(a)))[:4], **cp)
    elif k in CONVT_KINDS:
        from tests.test_plan_convtranspose import convt_fused_np
        y = convt_fused_np(*a, **cp)
    elif k == "conv_q4_pair":
        y1 = conv(step, a[0], a[1], a[2], a[3], a[4], **_strip(p["para1"]))
        y2 = conv(step, a[0], a[5], a[6], a[7], a[8], **_strip(p["para2"]))
        return [pack_q4(y1), pack_q4(y2)]
    elif k in ("wino4_in", "wino43_in"):
        return [a[0]]
    elif k in ("wino4_gemm", "wino43_gemm"):
        return [(a[0], a[1])]                            # the conv closes at @out / @chain with its tail
    elif k in ("wino4_out", "wino43_out", "wino4_chain", "wino43_chain"):
        x, K = args[0]
        y = conv(step, x, K, *(a[1:] + [None] * 4)[:4], pads=[1, 1, 1, 1], **{key: v for key, v in cp.items() if key in ("act", "alpha")})
        if k.endswith("_chain"):
            return [pack_q4(y), y] if p.get("keep_y", True) else [y]
    elif k == "conv1x1_wino_in":
        return [conv(step, a[0], a[1], a[2], a[3], a[4], **cp)]
    elif k == "to_q4":
        y = a[0].copy()
    elif k == "from_q4":
        return [a[0].copy()]
    elif k == "return":
        return [tuple(a)]
    elif k == "upconcat_q4":
        y = onp.concat(onp.upsample(a[0].copy(), a[1], mode="nearest"), a[2], axis=1)
    else:
        base = k[:-3] if k.endswith("_q4") else k
        y = onp.OPS[base](*[v.copy() if isinstance(v, np.ndarray) else v for v in a], **p)
    if isinstance(y, tuple):
        return list(y)
    return [pack_q4(np.asarray(y, np.float32)) if q4 else y]


def _strip(para):
    return {k: v for k, v in para.items() if k not in ("w_layout", "rowpack")}


def blob_inits(graph, blob):
    """{init key: array} of a graph's weight blob."""
    raw = np.asarray(blob).view(np.uint8).ravel()
    return {k: np.frombuffer(raw, dtype=dt, count=int(np.prod(s)), offset=o).reshape(s).copy()
            for (k, s, dt), o in zip(graph["inits"], _offsets(graph["inits"]))}

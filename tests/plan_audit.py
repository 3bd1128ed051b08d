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
    checked against tests/ref64_ops bounds;
  - the kinds behind the convs, NCHW and _q4 form alike: instance norm and group norm (with the residual and ReLU the plan
    folds in) against tests/groupnorm_ref.reference; pad (np.pad), pixel shuffle (numpy's reshape / transpose / reshape,
    nchw_out included), nearest resize and refold_q4 (tests/fold_ref.refold_np, zero-fill cells included) bit for bit; linear
    upsample / resize and their fused adds against ref64_ops.upsample_linear64 / resize_linear64 and their bounds;
  - steps on tensors folded by pixel phase (plan.fold_dilated; the fold comes from the key and DeviceArray.fold): a conv is
    checked in the UNFOLDED domain (_Layer.expect), a pointwise step on the folded arrays as observed; the input of a folded
    3x3 conv has exact zeros in its zero-fill cells, a tensor with a junk key is read by refold_q4 only (Audit.folds);
  - a kind without an arm fails the audit, and the census counts the audited steps by kind: `assert_every_step_audited`
    compares that with the kinds of the program's flow.
  A failure names the step, its kind, w_layout and launch plan, and the worst element (n, c, y, x) with its err / tol.
  -> {family: worst err / tol}, plus the census of w_layouts the program ran.

The CPU tests (tests/test_plan_audit.py) feed the same audit a trace made by `cpu_trace`: the program built by the same
two functions with the host's answers (`cpu_program`) and interpreted with numpy stand-ins (the oracle's float32 ops, Q4
values packed by numpy)."""
import collections

import numpy as np

from oracle import planer_np as onp
from planer_amd import conv_layouts as cl
from planer_amd import plan as P
from tests import fold_ref as FR
from tests import ref64 as R
from tests import ref64_ops as RO

# w_layout code -> lam family of tests/ref64.py
FAMILY = {0: "direct", 1: "direct", 2: "direct", 6: "direct", 10: "direct", 12: "direct", 13: "direct", 14: "direct",
          3: "f2x2", 4: "f2x2", 7: "f4x4", 9: "f4x4", 8: "w1d4", 11: "wino43"}
STAGED = {"wino4": cl.WINO4_Q4, "wino43": cl.WINO43_Q4}
CONV_KINDS = ("conv", "conv_fused", "conv_q4")
CONVT_KINDS = ("convtranspose", "convt_fused", "convt_q4")
EXACT = ("relu", "leakyrelu", "maxpool", "averagepool", "add", "concat", "upsample", "batchnorm", "clip", "flatten")
IN_PLACE = tuple(k for k, traits in P.KINDS.items() if P.W in traits)      # the kinds that rewrite srcs[0]: plan.KINDS' W rows


class Q4Host:
    """A channel-quad tensor on the host: data (n, ceil(c/4), h, w, 4), `chan` = c.  `fold`: None, or (dh, dw, H, W) of a tensor
    folded by pixel phase (plan.fold_dilated, DeviceArray.fold) -- n counts folded images, h x w is the folded map, H x W the
    unfolded one."""

    def __init__(self, data, chan, fold=None):
        self.data, self.chan = data, int(chan)
        self.fold = None if fold is None else tuple(int(v) for v in fold)

    def nchw(self):
        n, cq, h, w, _ = self.data.shape
        return np.ascontiguousarray(self.data.transpose(0, 1, 4, 2, 3).reshape(n, cq * 4, h, w)[:, :self.chan])


def pack_q4(x, fold=None):
    n, c, h, w = x.shape
    cq = -(-c // 4)
    buf = np.zeros((n, cq * 4, h, w), np.float32)
    buf[:, :c] = x
    return Q4Host(np.ascontiguousarray(buf.reshape(n, cq, 4, h, w).transpose(0, 1, 3, 4, 2)), c, fold)


def nchw(v):
    return v.nchw() if isinstance(v, Q4Host) else v


def sample(n):
    return sorted({0, n - 1})


def fold_sample(idx, dh, dw):
    """The images of a tensor folded by (dh, dw) that hold the unfolded images `idx`: every phase of each."""
    return [(n * dh + i) * dw + j for n in idx for i in range(dh) for j in range(dw)]


def key_fold(key):
    """((dh, dw), junk) where `key` names a folded tensor (plan.folded_key), else None."""
    base = key.split("@")[0]
    if P.FOLD_SEP not in base:
        return None
    tag = base.rsplit(P.FOLD_SEP, 1)[1]
    dh, dw = tag.rstrip("j").split("x")
    return (int(dh), int(dw)), tag.endswith("j")


def fold_of(v):
    return v.fold if isinstance(v, Q4Host) else None


class Trace(list):
    """The recorded steps; `flow_kinds`: kind -> number of steps of the program's flow, counted before anything ran."""

    def __init__(self, flow_kinds):
        super().__init__()
        self.flow_kinds = collections.Counter(flow_kinds)


class Census(collections.Counter):
    """w_layout -> convs audited.  `kinds`: kind -> steps audited; `assert_every_step_audited` compares it with the flow.
    `folded`: kind -> steps (refold_q4 apart) that read a folded tensor; `joined_1x1`: 1x1 convs among them; `junk`: tensors
    written under a junk key; `nearest`: kind -> nearest resizes checked; `plans`: (kind, launch plan) of the steps that gave one."""

    def __init__(self):
        super().__init__()
        self.kinds, self.folded, self.nearest = collections.Counter(), collections.Counter(), collections.Counter()
        self.joined_1x1, self.junk, self.plans = 0, 0, []


def assert_every_step_audited(trace, census):
    """Every step of the program's flow went through an arm of Audit.check: no step left out, none the trace did not record."""
    assert census.kinds == trace.flow_kinds, ("steps audited != steps of the flow", sorted((census.kinds - trace.flow_kinds).items()),
                                               sorted((trace.flow_kinds - census.kinds).items()))


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
        if a.fold is not None:                           # a folded tensor: the phases of the sampled images
            v = np.ascontiguousarray(v[fold_sample(idx, a.fold[0], a.fold[1])])
        elif v.ndim and v.shape[0] == batch:
            v = np.ascontiguousarray(v[idx])
        return Q4Host(v, a.chan, a.fold) if q4.is_q4(a) else v

    order = list(_steps_of(prog))
    trace, pos = Trace(prog.objs[name].name for name, _, _ in order), [0]

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
            plan = net.ctx.last_conv_plan() if any(t in self.name for t in ("conv", "wino", "norm_q4", "normalization_q4")) or self.name == "dense" else ""
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


CLOBBERED = object()            # in Audit.produced: a tensor a step rewrote with values the trace does not hold


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def _conv_para(para):
    return dict(group=int(para.get("group", 1)), strides=list(para.get("strides", (1, 1))),
                dilations=list(para.get("dilations", (1, 1))), pads=list(para.get("pads", (0, 0, 0, 0))))


class _Layer:
    """A logical conv: input (observed values, or a float64 reference with the bound it carries), filter and tail."""

    def __init__(self, x, x_tol, K, B, scale, shift, res, para, w_layout, transposed=False, fold=None):
        self.x, self.x_tol, self.K, self.B, self.scale, self.shift, self.res = x, x_tol, K, B, scale, shift, res
        self.para, self.w_layout, self.transposed, self.fold = para, w_layout, transposed, fold

    def expect(self):
        """-> (float64 reference, per-element tolerance).  A conv on folded tensors (`fold` = (dh, dw, H, W)) is computed in the
        UNFOLDED domain -- input, residual and carried bound unfolded, a 3x3 filter with the dilation and pads the fold stands
        for (plan.fold_dilated's rewrite undone), a 1x1 filter as it is -- and the reference and the bound are folded again, so
        the folded program is checked against the conv the fold stands for, not against itself.  Their zero-fill cells are 0:
        compare outside fold_ref.tail_mask.  The dilation and pads come from the fold alone: a step-local check cannot see
        whether the ORIGINAL conv had them (a head taken with other pads or strides); that is what the flow-preservation tests
        (test_rewrites_preserve_the_flow_*, the end-to-end comparisons) and tests/test_plan_dilated_fold.py are for."""
        if self.fold is None:
            return self._expect(self.x, self.x_tol, self.res, self.para)
        dh, dw, h, w = self.fold
        unfold = lambda a: None if a is None else FR.unfold_np(np.asarray(a), dh, dw, h, w)            # noqa: E731
        para = dict(self.para)
        if tuple(np.shape(self.K)[2:]) == (3, 3):
            para.update(dilations=[dh, dw], pads=[dh, dw, dh, dw])
        ref, tol = self._expect(unfold(self.x), unfold(self.x_tol), unfold(self.res), para)
        return FR.fold_np(ref, dh, dw), FR.fold_np(np.ascontiguousarray(np.broadcast_to(tol, ref.shape)), dh, dw)

    def _expect(self, x, x_tol, res, p):
        act, alpha = int(p.get("act", 0)), float(p.get("alpha", 0.0))
        lam = R.LAMBDA[FAMILY[self.w_layout]]
        x, K = _f64(x), _f64(self.K)
        if self.transposed:
            from tests.test_gpu_convtranspose import stuffed
            x, K = stuffed(x, K, list(p.get("strides", (2, 2))), list(p.get("pads", (0, 0, 0, 0))),
                           list(p.get("output_padding", (0, 0))))
            conv = {}
        else:
            conv = _conv_para(p)
        ref = R.ref64(x, K, self.B, self.scale, self.shift, res, act=act, alpha=alpha, **conv)
        tol = R.bound(x, K, self.B, self.scale, self.shift, res, lam=lam, reach=R.REACH[FAMILY[self.w_layout]], **conv)
        if x_tol is not None:
            s = np.abs(_f64(self.scale)).reshape(1, -1, 1, 1) if self.scale is not None else 1.0
            xt = x_tol
            if self.transposed:
                xt = stuffed(xt, K, list(p.get("strides", (2, 2))), list(p.get("pads", (0, 0, 0, 0))),
                             list(p.get("output_padding", (0, 0))))[0]
            tol = tol + s * R.conv64(xt, np.abs(K), **conv)
        return ref, tol


class Audit:
    def __init__(self, inits):
        self.inits = inits
        self.worst = collections.defaultdict(float)
        self.census = Census()
        self.produced = {}          # key -> NCHW values its producer wrote (updated by in-place steps)
        self.vsrc = {}              # Winograd-domain key -> (input values, carried tolerance or None, fold or None)
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
            self.folds(step)
            self.check(step)
            self.census.kinds[step.kind] += 1
            if step.plan:
                self.census.plans.append((step.kind, step.plan))
            for k, v in zip(step.dst, step.outs):
                if v is not None:
                    self.produced[k] = nchw(v)
            if step.kind in IN_PLACE:
                if step.kind == "groupnorm":
                    # layer.GroupNorm leaves the un-affined norm in x, which no trace records: plan.fuse_groupnorm only makes the
                    # step where nothing else reads x, and a later reader of it fails (inputs_are_what_was_written)
                    self.produced[step.src[0]] = CLOBBERED
                elif step.outs[0] is not None:
                    self.produced[step.src[0]] = nchw(step.outs[0])
        return dict(self.worst), self.census

    def folds(self, step):
        """What a fold adds to the contract: a key says how its tensor is folded; a tensor with a junk key (the output of a conv
        that folds alone, junk in its zero-fill cells) is read by refold_q4 only; a step other than refold_q4 writes the fold it
        read."""
        for i, (k, v) in enumerate(zip(step.src, step.ins)):
            f = key_fold(k)
            if f is not None and f[1] and step.kind != "refold_q4":
                self.fail(step, "input %d (%s) has a junk key: only refold_q4 may read it" % (i, k))
            if isinstance(v, Q4Host) and (v.fold[:2] if v.fold else None) != (f[0] if f else None):
                self.fail(step, "input %d (%s) is folded by %s" % (i, k, v.fold and v.fold[:2]))
        self.census.junk += sum(1 for k in step.dst if key_fold(k) is not None and key_fold(k)[1])
        if step.kind == "refold_q4":
            return
        self.census.folded[step.kind] += any(key_fold(k) is not None for k in step.src)
        if not any(isinstance(v, Q4Host) for v in step.ins):
            return
        have = next((f for f in (fold_of(v) for v in step.ins) if f is not None), None)
        for k, v in zip(step.dst, step.outs):
            if isinstance(v, Q4Host) and v.fold != have:
                self.fail(step, "output %s is folded by %s, the input by %s" % (k, v.fold, have))
            if isinstance(v, Q4Host) and v.fold and (v.fold[2] % v.fold[0] or v.fold[3] % v.fold[1]) and not (key_fold(k) or (0, 0))[1]:
                self.fail(step, "output %s has zero-fill cells this step wrote into: it needs a junk key" % k)

    def zero_fill(self, step, v=None, key=None):
        """The input of a folded 3x3 conv (operand 0 unless given): exact zeros in the zero-fill cells, which the conv reads as
        its padding."""
        if v is None:
            v, key = step.ins[0], step.src[0]
        if fold_of(v) is None:
            return
        dh, dw, h, w = v.fold
        a = v.nchw()
        bad = FR.tail_mask((a.shape[0] // (dh * dw), a.shape[1], h, w), dh, dw) & ~(a == 0)
        if bad.any():
            at = tuple(int(t) for t in np.argwhere(bad)[0])
            self.fail(step, "conv input %s: zero-fill cell %s = %r (%d cells are not zero)" % (key, at, float(a[at]), int(bad.sum())))

    def inputs_are_what_was_written(self, step):
        for i, (k, v) in enumerate(zip(step.src, step.ins)):
            if v is None or k not in self.produced:
                continue
            want, got = self.produced[k], nchw(v)
            if want is CLOBBERED:
                self.fail(step, "input %d (%s) was rewritten by an NCHW groupnorm step: nothing may read it after that" % (i, k))
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
        if layer.fold is not None and fold_of(got) != layer.fold:
            self.fail(step, "%s is folded by %s, the conv's input by %s" % (what, fold_of(got), layer.fold))
        got = nchw(got)
        if layer.fold is not None and got.shape == ref.shape:      # what the conv writes into the zero-fill cells is not its result
            dh, dw, h, w = layer.fold
            got = np.where(FR.tail_mask((ref.shape[0] // (dh * dw), ref.shape[1], h, w), dh, dw), ref, got)
        self.compare(step, what, FAMILY[layer.w_layout], got, ref, tol)

    def layer(self, step, off, para, w_layout, x=None, x_tol=None, transposed=False, res=True, fold=None):
        """_Layer from step inputs [x?, K, B, scale, shift, res] starting at `off` (x at off - 1 unless given, with its `fold`)."""
        if x is None:
            x, fold = self.arg(step, off - 1), fold_of(step.ins[off - 1])
        tail = [self.arg(step, off + j) for j in range(1, 5 if res else 4)] + ([] if res else [None])
        K = self.const(step.src[off])
        if fold is not None:
            # what a conv on folded tensors may be: a head rewritten to 3x3 / stride 1 / dilation 1 / pad 1, or a joined 1x1 /
            # stride 1 / pad 0 conv (plan.fold_dilated); anything else has no meaning on pixel phases
            geo = _conv_para(para)
            want = dict(geo, strides=[1, 1], dilations=[1, 1], pads=[1, 1, 1, 1] if tuple(K.shape[2:]) == (3, 3) else [0, 0, 0, 0])
            if tuple(K.shape[2:]) not in ((3, 3), (1, 1)) or geo != want:
                self.fail(step, "a %dx%d conv with %s on a tensor folded by %s" % (K.shape[2], K.shape[3], geo, fold[:2]))
            self.census.joined_1x1 += tuple(K.shape[2:]) == (1, 1)
            if tuple(K.shape[2:]) == (3, 3) and step.ins[0] is not None:
                self.zero_fill(step)
        return _Layer(x, x_tol, K, *tail, para=para, w_layout=w_layout, transposed=transposed, fold=fold)

    def refold(self, step):
        """refold_q4: fold_ref.refold_np of the observed input, bit for bit, the zero-fill cells (exact zeros) included."""
        v, out, p = step.ins[0], step.outs[0], step.para
        named = key_fold(step.src[0])
        src = tuple(int(t) for t in p["from"]) if p.get("from") is not None else named[0] if named else (1, 1)
        to = tuple(int(t) for t in p["to"])
        if ((v.fold or (1, 1))[:2]) != src:
            self.fail(step, "the input is folded by %s, the plan says %s" % (v.fold and v.fold[:2], src))
        a = v.nchw()
        h, w = v.fold[2:] if v.fold else a.shape[2:]
        want_fold = None if to == (1, 1) else to + (h, w)
        if fold_of(out) != want_fold:
            self.fail(step, "the output is folded by %s, want %s" % (fold_of(out), want_fold))
        self.exact(step, "refold %s -> %s" % (src, to), nchw(out), FR.refold_np(a, src, to, h, w))

    def norm(self, step, base):
        """instancenormalization / groupnorm, NCHW or Q4, with the tail plan.fuse_instnorm_q4 folds in: groupnorm_ref.reference
        (ref64_ops.instancenorm64 and instancenorm_bound on the rows, + U |ref| per further rounding).  An instance norm is the
        group norm of C groups without gamma and beta."""
        from tests.groupnorm_ref import reference
        p = step.para
        x = self.arg(step, 0)
        if x.size == 0:
            return self.exact(step, "output", nchw(step.outs[0]), x)
        if base == "groupnorm":
            gamma, beta, res, groups = self.arg(step, 3), self.arg(step, 4), self.arg(step, 5), int(p["groups"])
        else:
            gamma, beta, res, groups = None, None, self.arg(step, 3), x.shape[1]
        ref, tol = reference(_f64(x), self.arg(step, 1), self.arg(step, 2), gamma, beta, res, int(p.get("act", 0)), groups,
                             p.get("epsilon", 1e-5))
        self.compare(step, "output", base, nchw(step.outs[0]), ref, tol)

    def linear(self, step, base):
        """Linear upsample / resize and their fused adds: whole factors -> ref64_ops.upsample_linear64, others -> resize_linear64
        at round(factor * size), the dispatch of layer._upsample_linear; the fused add is one more rounding."""
        x = _f64(self.arg(step, 0))
        n, c, h, w = x.shape
        fused = base.endswith("_add")
        if base.startswith("upsample"):
            kv = np.asarray(self.const(step.src[1])).reshape(-1)
            f = (float(int(kv[-2])), float(int(kv[-1])))                       # truncated, as layer.UpSample reads them
            res = self.arg(step, 2) if fused else None
        else:
            f = P.resize_factors(step.src, x.shape, lambda key: np.zeros(0, np.float32) if key == "None" else np.asarray(self.const(key)))
            res = self.arg(step, 4) if fused else None
            if f is None:
                self.fail(step, "the factors of this resize are not constants")
        if f[0] == int(f[0]) and f[1] == int(f[1]):
            fh, fw = int(f[0]), int(f[1])
            fam = "upsample_linear"
            ref, tol = (x, 0.0 * x) if fh == fw == 1 else (RO.upsample_linear64(x, fh, fw), RO.upsample_linear_bound(x, fh, fw))
        else:
            oh, ow = int(round(f[0] * h)), int(round(f[1] * w))
            fam = "resize_linear"
            ref, tol = RO.resize_linear64(x, oh, ow), RO.resize_linear_bound(x, oh, ow)
        if fused:
            ref = ref + _f64(res)
            tol = tol + RO.U * np.abs(ref)
        self.compare(step, "output", fam + ("_add" if fused else ""), nchw(step.outs[0]), ref, tol)

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
            x, fold = self.arg(step, 0), fold_of(step.ins[0])
            for j, (pk, out) in enumerate(zip(("para1", "para2"), step.outs)):
                L = self.layer(step, 1 + 4 * j, p[pk], int(p[pk].get("w_layout", cl.DIRECT_Q4)), x=x, res=False, fold=fold)
                self.conv_check(step, L, out, "output %d" % (j + 1))
        elif k in ("wino4_in", "wino43_in"):
            self.zero_fill(step)
            self.vsrc[step.dst[0]] = (self.arg(step, 0), None, fold_of(step.ins[0]))
        elif k in ("wino4_gemm", "wino43_gemm"):
            x, x_tol, fold = self.vsrc.pop(step.src[0])
            self.open[step.name[:-len("@gemm")]] = (x, x_tol, self.const(step.src[1]), STAGED[k[:-len("_gemm")]], fold)
        elif k in ("wino4_out", "wino43_out", "wino4_chain", "wino43_chain"):
            x, x_tol, K, lay, fold = self.open.pop(step.name.rsplit("@", 1)[0])
            L = _Layer(x, x_tol, K, *[self.arg(step, j) for j in range(1, 5)], para=dict(p, pads=[1, 1, 1, 1]), w_layout=lay,
                       fold=fold)
            if k.endswith("_out") or p.get("keep_y", True):
                self.conv_check(step, L, step.outs[0])
                if k.endswith("_chain"):
                    self.zero_fill(step, step.outs[0], step.dst[0])      # the next conv's input
                    self.vsrc[step.dst[1]] = (nchw(step.outs[0]), None, fold)
            else:                                          # y is never written: its reference and bound go to the next conv
                self.census[lay] += 1
                self.vsrc[step.dst[0]] = L.expect() + (fold,)
        elif k == "conv1x1_wino_in":
            L = self.layer(step, 1, dict(p), cl.DIRECT_Q4, res=False)
            self.census[cl.DIRECT_Q4] += 1
            self.vsrc[step.dst[0]] = L.expect() + (L.fold,)
        elif k in ("to_q4", "from_q4"):
            self.exact(step, "conversion", nchw(step.outs[0]), self.arg(step, 0))
        elif k == "refold_q4":
            self.refold(step)
        elif k == "upconcat_q4":
            up = onp.upsample(self.arg(step, 0).copy(), self.arg(step, 1), mode="nearest")
            self.exact(step, "upsample + concat", nchw(step.outs[0]), onp.concat(up, self.arg(step, 2), axis=1))
        elif base in ("instancenormalization", "groupnorm"):
            self.norm(step, base)
        elif base == "pad":
            x, pads, value = self.arg(step, 0), self.arg(step, 1), self.arg(step, 2)
            kw = {"mode": p.get("mode", "constant")}
            if kw["mode"] == "constant":
                kw["constant_values"] = np.float32(p.get("constant_value", 0) if value is None else np.asarray(value).reshape(-1)[0])
            self.exact(step, "output", nchw(step.outs[0]), np.pad(x, np.asarray(pads).reshape(2, -1).T.astype(int).tolist(), **kw))
        elif base == "pixelshuffle":
            from tests.pixel_shuffle_ref import shuffle_np
            if k.endswith("_q4") and bool(p.get("nchw_out")) == isinstance(step.outs[0], Q4Host):
                self.fail(step, "nchw_out %r, the output is %s" % (p.get("nchw_out"), type(step.outs[0]).__name__))
            self.exact(step, "output", nchw(step.outs[0]), shuffle_np(self.arg(step, 0), **p))
        elif P.is_linear(base, p):
            self.linear(step, base)
        elif base == "resize":                              # nearest: the oracle's replication (and shift)
            args = [np.zeros(0, np.float32) if a is None else np.array(a) for a in (self.arg(step, i) for i in range(len(step.src)))]
            self.exact(step, "output", nchw(step.outs[0]), onp.OPS[base](*args, **p))
            self.census.nearest[k] += 1
        elif k in ("reshape", "transpose", "mul"):           # what a group norm or a pixel shuffle is with its pass switched off
            self.exact(step, "output", step.outs[0], onp.OPS[k](*[np.array(self.arg(step, i)) for i in range(len(step.src))], **p))
        elif base in EXACT:
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
    """-> ({family: worst err / tol}, Census: Counter of w_layouts, `.kinds` the steps audited by kind).  Raises AuditError on the
    first step that is wrong."""
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


def cpu_program(graph, blob, x, pick=lambda cands: cands[0], force_q4=False, **kw):
    """The program Net compiles for this graph, on the host: plan.compile_front, then plan.lower with `pick` in place of the
    timing and the host's answers for the rest (no stem + max-pool kernel, every map fits the chained transform).  `kw`: to
    cpu_front (`worth`: fold_dilated's callback, as Net gives it with net.fold_dilated set).
    -> (body, flow, shapes)"""
    from planer_amd.plan import lower
    body, flow, _, shapes = cpu_front(graph, blob, x, force_q4, **kw)
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
            images = idx if v.fold is None else fold_sample(idx, v.fold[0], v.fold[1])
            return Q4Host(np.ascontiguousarray(v.data[images]).copy(), v.chan, v.fold)
        v = np.asarray(v)
        return np.ascontiguousarray(v[idx]) if v.ndim and v.shape[0] == batch else v.copy()

    trace = Trace(kinds[name][1] for _, names, _ in flow for name in _as_list(names))
    out_key, folds = None, {}                            # folds: key -> (dh, dw, H, W) of a folded tensor, Winograd-domain ones too
    for src, names, dst in flow:
        for pos, name in enumerate(_as_list(names)):
            keys = _as_list(src if pos == 0 else dst)
            _, kind, para = kinds[name]
            args = [get(k) for k in keys]
            ins = [host(a, k) for a, k in zip(args, keys)]
            step = Step(name, kind, para, keys, _as_list(dst), ins, [])
            fold = next((folds[k] for k in keys if folds.get(k) is not None), None)
            outs = _standin(step, args, conv, fold)
            if fault is not None:
                outs = fault(step, outs)
            for k, v in zip(step.dst, outs):
                env[k] = v
                folds[k] = v.fold if isinstance(v, Q4Host) else fold if kind != "return" else None
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


def _tail32(y, res, act):
    """The tail plan.fuse_instnorm_q4 / fuse_linear_add folds in, in float32, each operation rounded on its own."""
    if res is not None:
        y = (np.asarray(y, np.float32) + np.asarray(res, np.float32)).astype(np.float32)
    return np.maximum(y, np.float32(0)) if act else y


def _standin(step, args, conv, fold=None):
    """`fold`: (dh, dw, H, W) where an input is folded by pixel phase -- a position-independent step (plan.KINDS' F rows, a conv
    rewritten to dilation 1) runs on the folded arrays as they are and writes a tensor folded the same way."""
    k, p = step.kind, step.para
    base = k[:-3] if k.endswith("_q4") else k
    a = [nchw(v) if isinstance(v, Q4Host) else v for v in args]
    q4 = k in Q4_OUT or (k.endswith("_q4") and k not in ("gap_q4", "from_q4") and not p.get("nchw_out"))
    cp = {key: v for key, v in p.items() if key not in ("w_layout", "rowpack", "strip_rows", "keep_y", "wino")}
    if k in ("relu_q4", "clip_q4") or k in ("relu", "clip"):
        v = args[0]
        buf = v.data if isinstance(v, Q4Host) else v
        buf[...] = onp.OPS[k.replace("_q4", "")](buf.copy(), **p)          # in place, like the kernels
        return [v]
    if base in ("instancenormalization", "groupnorm"):
        from tests.groupnorm_ref import groupnorm_np
        v, s, b = args[0], a[1].copy(), a[2].copy()                         # (the oracle's norm reshapes s and b in place)
        x = a[0] if k == "groupnorm" else a[0].copy()                       # layer.GroupNorm: x is left as the inner norm made it
        if base == "groupnorm":
            res = a[5] if len(a) > 5 else None
            y = groupnorm_np(x, s, b, a[3], a[4], res, groups=p["groups"], epsilon=p.get("epsilon", 1e-5), act=p.get("act", 0))
            if k == "groupnorm":
                return [y]
        else:
            y = _tail32(onp.OPS[base](x, s, b, epsilon=p.get("epsilon", 1e-5)), a[3] if len(a) > 3 else None, p.get("act", 0))
        if isinstance(v, Q4Host):                                           # in place, like the kernels
            v.data[...] = pack_q4(y).data
        else:
            v[...] = y
        return [v]
    if k == "refold_q4":
        v, to = args[0], tuple(int(t) for t in p["to"])
        dh, dw, h, w = v.fold if v.fold is not None else (1, 1) + a[0].shape[2:]
        return [pack_q4(FR.refold_np(a[0], (dh, dw), to, h, w), None if to == (1, 1) else to + (h, w))]
    if base == "pad":
        value = p.get("constant_value", 0) if len(a) < 3 or a[2] is None else np.asarray(a[2]).reshape(-1)[0]
        y = onp.OPS["pad"](a[0], np.asarray(a[1]), value, p.get("mode", "constant")).astype(np.float32)
        return [pack_q4(y) if q4 else y]
    if base == "pixelshuffle":
        from tests.pixel_shuffle_ref import shuffle_np
        y = shuffle_np(a[0], **p)
        return [pack_q4(y) if q4 else y]
    if base in ("upsample_add", "resize_add"):
        y = _tail32(onp.OPS[base[:-4]](*[np.zeros(0, np.float32) if v is None else v.copy() for v in a[:-1]], **p), a[-1], 0)
        return [pack_q4(y)]
    if base == "resize":
        y = onp.OPS[base](*[np.zeros(0, np.float32) if v is None else v.copy() for v in a], **p)
        return [pack_q4(np.asarray(y, np.float32)) if q4 else y]
    if k in CONV_KINDS:
        y = conv(step, *a[:1], a[1], *(a[2:] + [None] * (6 - len(a)))[:4], **cp)
    elif k in CONVT_KINDS:
        from tests.test_plan_convtranspose import convt_fused_np
        y = convt_fused_np(*a, **cp)
    elif k == "conv_q4_pair":
        y1 = conv(step, a[0], a[1], a[2], a[3], a[4], **_strip(p["para1"]))
        y2 = conv(step, a[0], a[5], a[6], a[7], a[8], **_strip(p["para2"]))
        return [pack_q4(y1, fold), pack_q4(y2, fold)]
    elif k in ("wino4_in", "wino43_in"):
        return [a[0]]
    elif k in ("wino4_gemm", "wino43_gemm"):
        return [(a[0], a[1])]                            # the conv closes at @out / @chain with its tail
    elif k in ("wino4_out", "wino43_out", "wino4_chain", "wino43_chain"):
        x, K = args[0]
        y = conv(step, x, K, *(a[1:] + [None] * 4)[:4], pads=[1, 1, 1, 1], **{key: v for key, v in cp.items() if key in ("act", "alpha")})
        if k.endswith("_chain"):
            return [pack_q4(y, fold), y] if p.get("keep_y", True) else [y]
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
        y = onp.OPS[base](*[v.copy() if isinstance(v, np.ndarray) else v for v in a], **p)
    if isinstance(y, tuple):
        return list(y)
    return [pack_q4(np.asarray(y, np.float32), fold) if q4 else y]


def _strip(para):
    return {k: v for k, v in para.items() if k not in ("w_layout", "rowpack")}


def blob_inits(graph, blob):
    """{init key: array} of a graph's weight blob."""
    raw = np.asarray(blob).view(np.uint8).ravel()
    return {k: np.frombuffer(raw, dtype=dt, count=int(np.prod(s)), offset=o).reshape(s).copy()
            for (k, s, dt), o in zip(graph["inits"], _offsets(graph["inits"]))}

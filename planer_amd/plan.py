"""Plan compiler: peephole fusion of a planer flow (pure host logic, no GPU).

The reference interprets the flow one layer at a time (net.py:37-72).  On
MI355X the HBM-bound layers that follow a convolution -- folded BatchNorm
(layer.py:125-127), residual Add (layer.py:93-95), ReLU / LeakyReLU
(layer.py:44-51) -- cost more than the bytes they compute on, so the plan
folds each chain  conv -> batchnorm -> [add] -> [relu|leakyrelu] -> [add]  into
the conv kernel's epilogue (`conv_fused`; the residual goes before the
activation in ResNet's blocks and after it in YOLO-v3's, never both).  A
transposed conv that the phase-decomposed kernel runs heads the same chains
(`convt_fused`: a U-Net's up-step followed by BatchNorm / ReLU).  A link is absorbed only when the
intermediate tensor has exactly one reader and one writer, so nothing a user
could observe disappears; the fused step sits where the LAST link of its
chain was, so a residual operand produced after the conv is still available.

Programs pass from pass to pass as (body, flow).  Inside a pass they are read through `Steps` -- one step per layer, who reads
and writes each key, the two predicates that make moving a read sound (`only_reader`, `clobbered`) and the one epilogue that
rebuilds a body (`emit`) -- and what a kind does to its operands is looked up in one table, `KINDS`.
"""
import os

from .conv_layouts import (CONVT_KINDS, DIRECT_Q4, ROWPACK_Q4, STAGED_LAYOUTS, STEM_POOL, STEM_POOL_NCHW, choose, conv_para,
                           convt_phase_eligible, dw_q4_eligible, q4_conv_eligible, suffix)
from .layer import PIXEL_SHUFFLE_AXES, _nearest_shift, pixel_shuffle_shapes

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
ACT_RES_AFTER = 16      # OR-ed into `act`: the residual is added after the activation


def _as_list(v):
    return list(v) if isinstance(v, (list, tuple)) else [v]


# ---- what a kind does to its operands: ONE table, every list of kinds below is read off it ---------------------------------------
# W    rewrites srcs[0] in place and hands it on (layer.py:46, 217-226, 250-258): a read of that tensor may not move across it
# R    only reads its inputs: a Winograd input transform may be hoisted over it (chain_winograd)
# F    position-independent: runs unchanged on tensors folded by pixel phase (fold_dilated)
# Q..  has a channel-quad kernel, kind + "_q4" (planer_amd/q4.py: Q4_LAYERS); QI and QL are those a switch takes out again
# A kind with none of them is none of these: it writes a tensor of its own, nothing is hoisted over it, it reads unfolded NCHW.
# Every kind a plan can hold has a row (tests/test_plan_kinds.py), so a new kind states whether it writes in place.
W, R, F, Q, QI, QL = "in place", "pure reader", "folds", "q4", "q4/PLANER_HIP_INSTNORM_Q4", "q4/PLANER_HIP_LINEAR_Q4"
KINDS = {
    # the reference's operators (layer.layer_map)
    "maxpool": (Q,), "averagepool": (Q,), "gap": (Q,), "upsample": (Q,), "batchnorm": (Q,), "relu": (W, Q), "leakyrelu": (Q,),
    "sigmoid": (Q,), "add": (Q,), "concat": (Q,), "clip": (W, Q), "instancenormalization": (W, QI), "pad": (QI,), "resize": (QL,),
    "erf": (W,), "dense": (), "conv": (), "convtranspose": (), "flatten": (), "matmul": (), "identity": (), "return": (),
    "sub": (), "mul": (), "div": (), "pow": (), "exp": (), "log": (), "tanh": (), "sqrt": (), "reciprocal": (), "hardsigmoid": (),
    "softmax": (), "logsoftmax": (), "reducesum": (), "reducemean": (), "reducemax": (), "reducemin": (), "transpose": (),
    "reshape": (), "squeeze": (), "unsqueeze": (), "slice": (), "tile": (), "expand": (), "split": (), "shape": (), "const": (),
    "constantofshape": (), "range": (), "cast": (), "equal": (), "greater": (), "greaterorequal": (), "where": (), "gather": (),
    "scatternd": (), "nonzero": (), "topk": (), "lstm": (),
    # what the passes in front of assign_layouts make
    "conv_fused": (), "convt_fused": (), "pixelshuffle": (Q,), "groupnorm": (W, Q),
    # the channel-quad forms
    "maxpool_q4": (R,), "averagepool_q4": (R,), "gap_q4": (R,), "upsample_q4": (R,), "batchnorm_q4": (R, F), "relu_q4": (W, F),
    "leakyrelu_q4": (R, F), "sigmoid_q4": (R, F), "add_q4": (R, F), "concat_q4": (R, F), "clip_q4": (W, F),
    "instancenormalization_q4": (W,), "pad_q4": (R,), "resize_q4": (R,), "pixelshuffle_q4": (R,), "groupnorm_q4": (W,),
    # plan-internal (q4.register)
    "to_q4": (), "from_q4": (R,), "refold_q4": (R,), "conv_q4": (R,), "convt_q4": (R,), "conv_q4_pair": (R,), "conv_pool_q4": (),
    "upconcat_q4": (R,), "upsample_add_q4": (R,), "resize_add_q4": (R,), "conv1x1_wino_in": (R,),
    "wino4_in": (R,), "wino4_gemm": (R,), "wino4_out": (R,), "wino4_chain": (R,),
    "wino43_in": (R,), "wino43_gemm": (R,), "wino43_out": (R,), "wino43_chain": (R,),
}


def _kinds_with(*traits):
    return tuple(k for k, t in KINDS.items() if any(x in t for x in traits))


_IN_PLACE, _PURE_READERS, _FOLD_POINTWISE = _kinds_with(W), _kinds_with(R), _kinds_with(F)
# (instancenormalization_q4 never joins a fold; fold_dilated's list has named it since the norm got its Q4 form, and keeps it)
_FOLD_IN_PLACE = tuple(k for k in _FOLD_POINTWISE if k in _IN_PLACE) + ("instancenormalization_q4",)


class Steps:
    """The view every pass takes of a (body, flow) program.  `steps`: one [srcs list, name, dst] per layer, chained steps
    [x, [l1, l2], y] taken apart (net.py:46-50).  `layers`: name -> (kind, para).  `readers`, `writers`: key -> the indices of
    the steps that read / write it, each once and in order."""

    def __init__(self, body, flow):
        self.layers = {b[0]: (b[1], b[2]) for b in body}
        self.steps = [[_as_list(src if pos == 0 else dst), name, dst]
                      for src, names, dst in flow for pos, name in enumerate(_as_list(names))]
        self.readers, self.writers = {}, {}
        for i, (srcs, _, dst) in enumerate(self.steps):
            for k in set(srcs):
                self.readers.setdefault(k, []).append(i)
            for k in _as_list(dst):
                self.writers.setdefault(k, []).append(i)

    def kind(self, i):
        return self.layers[self.steps[i][1]][0]

    def step(self, i):
        """Step i as passes emit it: (srcs, name, kind, para, dst)."""
        srcs, name, dst = self.steps[i]
        return (srcs, name) + tuple(self.layers[name]) + (dst,)

    def each(self):
        return [self.step(i) for i in range(len(self.steps))]

    def only_reader(self, i, dst):
        """The one step that reads `dst`, a single tensor written once (by step i), where it comes later; else None.  What lets
        a pass absorb the reader into step i: nothing a user could observe disappears with `dst`."""
        if not isinstance(dst, str) or len(self.readers.get(dst, ())) != 1 or len(self.writers.get(dst, ())) != 1:
            return None
        return self.readers[dst][0] if self.readers[dst][0] > i else None

    def clobbers(self, t, key, in_place=_IN_PLACE, writes=True):
        """Step t reads `key` and is of a kind in `in_place` (None: any reader counts), or -- with `writes` -- writes `key`."""
        srcs, _, dst = self.steps[t]
        return (key in srcs and (in_place is None or self.kind(t) in in_place)) or (writes and key in _as_list(dst))

    def clobbered(self, key, lo, hi, skip=(), **rule):
        """A step strictly between lo and hi, those in `skip` apart, clobbers `key`: a read of it may not move from lo to hi."""
        return any(self.clobbers(t, key, **rule) for t in range(lo + 1, hi) if t not in skip)

    def spliced(self, at, dropped=()):
        """-> [(srcs, name, kind, para, dst)]: the steps with `at[i]` in place of step i and those in `dropped` gone."""
        return [at[i] if i in at else self.step(i) for i in range(len(self.steps)) if i in at or i not in dropped]

    @staticmethod
    def emit(out):
        """[(srcs, name, kind, para, dst)] -> (body, flow): each layer once, in the order of first use; one layer per step."""
        body, seen = [], set()
        for srcs, name, kind, para, dst in out:
            if name not in seen:
                seen.add(name)
                body.append([name, kind, para])
        return body, [[srcs, [name], dst] for srcs, name, kind, para, dst in out]


def convt_ok(srcs, para, inits, shapes):
    """A convtranspose step the phase-decomposed kernel takes: constant 4-D filter, 4-D input, and a geometry
    layer.convt_phase_eligible accepts (group 1, dilation 1, pads within the kernel reach)."""
    return (len(srcs) >= 2 and srcs[1] in inits and _is4d(shapes, srcs[1]) and _is4d(shapes, srcs[0])
            and convt_phase_eligible(shapes[srcs[1]], **para))


def fuse_flow(layers, flow, init_names, shapes):
    """-> (layers', flow', number_of_absorbed_steps).

    `shapes` maps tensor keys to shapes (from one eager pass); a residual add
    is folded only when both operands have the same known shape.
    """
    view = Steps(layers, flow)
    steps, inits = view.steps, set(init_names)
    consumed, fused_at, nfused = set(), {}, 0
    for i, (srcs, name, dst) in enumerate(steps):
        kind, para = view.layers[name]
        if i in consumed or not isinstance(dst, str):
            continue
        if kind != "conv" and not (kind == "convtranspose" and convt_ok(srcs, para, inits, shapes)):
            continue
        chain, cur, stage = [i], dst, 0
        extra = {"scale": "None", "shift": "None", "res": "None", "act": ACT_NONE, "alpha": 0.0}
        while stage < 4:
            j = view.only_reader(chain[-1], cur)
            if j is None or j in consumed or not isinstance(steps[j][2], str):
                break
            jsrcs, jname, jdst = steps[j]
            jkind, jpara = view.layers[jname]
            # an in-place relu on one of the conv's inputs between here and j would
            # change what the delayed conv reads (layer.py:46 mutates its input)
            if any(view.clobbered(k, chain[-1], j, chain, in_place=("relu",), writes=False) for k in srcs):
                break
            if (jkind == "batchnorm" and stage < 1 and len(jsrcs) == 3 and jsrcs[0] == cur
                    and jsrcs[1] in inits and jsrcs[2] in inits):
                extra["scale"], extra["shift"], stage = jsrcs[1], jsrcs[2], 1
            elif (jkind == "add" and (stage < 2 or (stage == 3 and extra["res"] == "None"))
                  and len(jsrcs) == 2 and jsrcs.count(cur) == 1
                  and shapes.get(jsrcs[0]) is not None
                  and tuple(shapes.get(jsrcs[0])) == tuple(shapes.get(jsrcs[1]) or ())):
                extra["res"] = jsrcs[1 - jsrcs.index(cur)]
                if stage == 3:
                    extra["act"] |= ACT_RES_AFTER
                stage = 2 if stage < 2 else 4
            elif jkind == "relu" and stage < 3:
                extra["act"], stage = ACT_RELU, 3
            elif jkind == "leakyrelu" and stage < 3:
                extra["act"], extra["alpha"], stage = ACT_LEAKY, jpara.get("alpha", 0.2), 3
            else:
                break
            chain.append(j)
            cur = jdst
        if len(chain) > 1:
            consumed.update(chain)
            args = [srcs[0], srcs[1], srcs[2] if len(srcs) > 2 else "None", extra["scale"], extra["shift"], extra["res"]]
            fused_at[chain[-1]] = (args, name + "+", "conv_fused" if kind == "conv" else "convt_fused",
                                   dict(para, act=extra["act"], alpha=extra["alpha"]), cur)
            nfused += len(chain) - 1
    return view.emit(view.spliced(fused_at, consumed)) + (nfused,)


# ---- activation layout assignment -------------------------------------------------------------
# Kinds that have a channel-quad (Q4) kernel besides conv (planer_amd/q4.py).  A step of one of
# these kinds runs in Q4 when one of its activation inputs already is Q4 -- layouts are "sticky"
# downstream of a conv -- and everything else reads NCHW, with a conversion step inserted where a
# value is needed in the layout it was not produced in (converted copies are cached per value).
Q4_POINTWISE = _kinds_with(Q, QI, QL)
# the kinds of instance-normalised generators (fast-neural-style, CycleGAN ...): PLANER_HIP_INSTNORM_Q4=0 takes them out again,
# which gives the program of a compiler without them
INSTNORM_Q4_KINDS = _kinds_with(QI)
PAD_MODES = ("constant", "wrap", "edge", "reflect", "symmetric")
TO_Q4, FROM_Q4 = "@to_q4", "@from_q4"


# bilinear interpolation between convs (FPN top-down paths, segmentation decoders): PLANER_HIP_LINEAR_Q4=0 takes linear
# `upsample` and the WHOLE of `resize` out again -- nearest `resize` too, although the switch is named after the linear kernels:
# no `resize` ran in Q4 before them, and the switch's contract is the program of a compiler without this change
LINEAR_Q4_KINDS = _kinds_with(QL)


def linear_q4_enabled():
    return os.environ.get("PLANER_HIP_LINEAR_Q4", "1") != "0"


def q4_pointwise_kinds():
    """Q4_POINTWISE as the environment leaves it."""
    kinds = Q4_POINTWISE
    if os.environ.get("PLANER_HIP_INSTNORM_Q4", "1") == "0":
        kinds = tuple(k for k in kinds if k not in INSTNORM_Q4_KINDS)
    if not linear_q4_enabled():
        kinds = tuple(k for k in kinds if k not in LINEAR_Q4_KINDS)
    return kinds


def _copy_of(body, flow):
    """A program as it came, in its own form: what a pass hands back where nothing matched."""
    return [list(b) for b in body], [[list(s) if isinstance(s, (list, tuple)) else s, n, d] for s, n, d in flow]


def _shape(shapes, key):
    """The shape of a tensor by its key (a converted copy, key@q4, has its tensor's), as a tuple, or None."""
    s = shapes.get(key.split("@")[0])
    return None if s is None else tuple(s)


def _is4d(shapes, key):
    s = shapes.get(key)
    return s is not None and len(s) == 4


def q4_conv_ok(srcs, para, inits, shapes):
    """A conv step can take the Q4 kernel: constant 4-D filter (and constant bias / scale / shift),
    4-D input, symmetric pads, and groups that do not split a channel quad (conv_layouts.q4_conv_eligible) -- or one input
    and one output channel per group (a depthwise conv: conv_layouts.dw_q4_eligible)."""
    if len(srcs) < 2 or srcs[1] not in inits or not _is4d(shapes, srcs[1]) or not _is4d(shapes, srcs[0]):
        return False
    if any(k != "None" and k not in inits for k in srcs[2:5]):
        return False
    group = int(para.get("group", 1))
    pads = list(para.get("pads", (0, 0, 0, 0)))
    if len(pads) == 4 and (pads[0] != pads[2] or pads[1] != pads[3]):
        return False
    return dw_q4_eligible(shapes[srcs[1]], group) or q4_conv_eligible(shapes[srcs[1]], group)


def pad_q4_ok(c, pads, constant_value=0, mode="constant", **_):
    """PadQ4 pads pixels only -- (N, C, H, W) pads as ONNX orders them, all begins then all ends, N and C entries zero -- and in
    constant mode keeps the zero padding lanes of a partial last quad only when the value is 0 (the rule of clip_q4_ok)."""
    pads = [int(v) for v in pads]
    if len(pads) != 8 or any(p < 0 for p in pads) or any(pads[i] for i in (0, 1, 4, 5)) or mode not in PAD_MODES:
        return False
    return mode != "constant" or c % 4 == 0 or float(constant_value) == 0.0


def groupnorm_q4_ok(c, groups):
    """GroupNormQ4 takes the channels-per-group counts that do not split a channel quad unevenly: a multiple of 4 (a group is whole
    quad planes), 2 (two groups per quad) or 1 (the instance norm's geometry).  3, 6, 10 ... have no channel-quad form."""
    c, groups = int(c), int(groups)
    if groups < 1 or c < 1 or c % groups:
        return False
    cpg = c // groups
    return cpg % 4 == 0 or cpg in (1, 2)


def _linear_factors_ok(fh, fw, h, w):
    """The geometries the linear channel-quad kernels take (q4._upsample_linear_q4): integer factors other than 1 x 1 with at
    most 64 weights, or fractional ones on a map of at least 2 x 2 pixels."""
    if fh == int(fh) and fw == int(fw):
        return fh >= 1 and fw >= 1 and 1 < int(fh) * int(fw) <= 64
    return h >= 2 and w >= 2 and int(round(fh * h)) >= 1 and int(round(fw * w)) >= 1


def resize_factors(srcs, shape, values):
    """(fh, fw) of a resize step as layer.Resize reads them -- scales, or sizes over the input's -- or None where they are not
    constants whose numbers are known."""
    if values is None or len(srcs) < 3:
        return None
    kv = values(srcs[2])
    if kv is None:
        return None
    kv = kv.reshape(-1)
    if kv.size == 0:
        sz = values(srcs[3]) if len(srcs) > 3 else None
        if sz is None or sz.reshape(-1).size < 2 or not shape[2] or not shape[3]:
            return None
        sz = sz.reshape(-1)
        return float(sz[-2]) / shape[2], float(sz[-1]) / shape[3]
    return (float(kv[-2]), float(kv[-1])) if kv.size >= 2 else None


def resize_nearest_q4_ok(fh, fw, trans_mode="half_pixel", round_mode="round_prefer_floor"):
    """A nearest `resize` by (fh, fw), truncated as layer.Resize truncates them, has a channel-quad form: up-scaling, and a
    (transform, rounding) pair that does not shift the replicated map (layer._nearest_shift is 0 on both axes)."""
    fh, fw = int(fh), int(fw)
    return fh >= 1 and fw >= 1 and _nearest_shift(fh, trans_mode, round_mode) == 0 and _nearest_shift(fw, trans_mode, round_mode) == 0


def is_linear(kind, para):
    """A step that interpolates linearly: `upsample` / `resize` (or their channel-quad kinds) with mode "linear"."""
    return kind.split("_")[0] in ("upsample", "resize") and para.get("mode", "nearest") == "linear"


def _q4_pointwise_ok(kind, srcs, para, inits, shapes, values=None):
    acts = [k for k in srcs if k != "None" and k not in inits]
    if not acts or not all(_is4d(shapes, k) for k in acts):
        return False
    c = shapes[acts[0]][1]
    if kind == "instancenormalization":     # constant scale and bias
        return len(srcs) == 3 and len(acts) == 1 and acts[0] == srcs[0] and srcs[1] in inits and srcs[2] in inits
    if kind == "groupnorm":                 # constant scale, bias, gamma and beta; a group count that keeps quads whole
        return (len(srcs) == 5 and acts == [srcs[0]] and all(k in inits for k in srcs[1:3])
                and all(k == "None" or k in inits for k in srcs[3:5]) and groupnorm_q4_ok(c, para.get("groups", 0)))
    if kind == "pad":                       # constant pads (and value): their numbers decide, so the caller must supply them
        if values is None or len(srcs) not in (2, 3) or acts != [srcs[0]] or srcs[1] not in inits:
            return False
        pv = values(srcs[1])
        cv = para.get("constant_value", 0)
        if len(srcs) == 3 and srcs[2] != "None":
            cv = values(srcs[2])
            cv = None if cv is None or len(cv.reshape(-1)) != 1 else float(cv.reshape(-1)[0])
        return pv is not None and cv is not None and pad_q4_ok(c, list(pv.reshape(-1)), cv, para.get("mode", "constant"))
    if kind == "pixelshuffle":              # CRD for any channel count; DCR where every narrow quad is one aligned wide quad
        r = int(para.get("r", 0))
        narrow = c if para.get("inverse") else c // max(1, r * r)
        return (list(srcs) == acts and r in PIXEL_SHUFFLE_R and (para.get("order") == "crd" or (para.get("order") == "dcr" and narrow % 4 == 0))
                and pixel_shuffle_shapes(shapes[acts[0]], r, para.get("order"), para.get("inverse")) is not None)
    if kind == "add":
        return len(srcs) == 2 and len(acts) == 2 and tuple(shapes[srcs[0]]) == tuple(shapes[srcs[1]])
    if kind == "concat":
        return para.get("axis", 0) in (1, -3) and len(acts) == len(srcs) and all(shapes[k][1] % 4 == 0 for k in srcs)
    if kind == "sigmoid":
        return c % 4 == 0
    if kind == "clip":                    # clip(0) must be 0 where a partial last quad has padding lanes
        return c % 4 == 0 or float(para.get("min", 0)) <= 0.0 <= float(para.get("max", 1))
    if kind == "batchnorm":
        return len(srcs) == 3 and srcs[1] in inits and srcs[2] in inits
    if kind == "upsample":
        if len(srcs) != 2 or srcs[1] not in inits:
            return False
        if para.get("mode", "nearest") == "nearest":
            return True
        if para.get("mode") != "linear" or not linear_q4_enabled() or values is None or values(srcs[1]) is None:
            return False
        kv = values(srcs[1]).reshape(-1)
        if kv.size < 2:
            return False
        n, _, h, w = shapes[srcs[0]]
        return _linear_factors_ok(int(kv[-2]), int(kv[-1]), h, w)          # truncated, layer.py:82
    if kind == "resize":                  # constant scales / sizes: their numbers decide
        if acts != [srcs[0]] or any(k != "None" and k not in inits for k in srcs[1:]):
            return False
        f = resize_factors(srcs, shapes[srcs[0]], values)
        if f is None:
            return False
        n, _, h, w = shapes[srcs[0]]
        if para.get("mode", "nearest") == "linear":
            return _linear_factors_ok(f[0], f[1], h, w)
        return (para.get("mode", "nearest") == "nearest" and int(f[0]) * int(f[1]) != 1
                and resize_nearest_q4_ok(f[0], f[1], para.get("coordinate_transformation_mode", "half_pixel"),
                                         para.get("nearest_mode", "round_prefer_floor")))
    return len(acts) == 1


# Rough device rates for the go / no-go estimate below: the Q4 conv kernel saves ~15 % of a conv's
# time at ~100 TFLOP/s; a layout conversion reads and writes its tensor once at ~4 TB/s.
_Q4_CONV_GAIN_S_PER_FLOP = 0.15 / 100e12
_CONVERT_S_PER_BYTE = 2.0 / 4e12


def _nbytes(shape):
    n = 4
    for d in shape:
        n *= d
    return n


def assign_layouts(body, flow, init_names, shapes, force=False, values=None):
    """-> (body', flow', number of Q4 steps).  `values(key)` gives the host array of a constant (or None): `pad` goes Q4 only
    where its pads are known numbers.  Rewrites conv / conv_fused steps to `conv_q4`, the transposed convs
    the phase-decomposed kernel takes (convtranspose / convt_fused) to `convt_q4`, and the
    HBM-bound layers that follow them to their `*_q4` kinds, inserting `to_q4` / `from_q4` steps at
    the edges.  The program's observable values (its last step's outputs) stay NCHW.

    Unless `force`, the rewrite is dropped (-> the input program, 0) when the conversions it needs
    would cost more than the convs gain -- e.g. a lone conv whose large output has to be handed
    back as NCHW right away."""
    view = Steps(body, flow)
    kinds, steps, inits = view.layers, view.steps, set(init_names)
    q4 = set()          # keys whose primary copy is Q4
    copies = {}         # (key, layout) -> key of the cached converted copy
    out, nq4 = [], 0    # out: (srcs, name, kind, para, dst)

    def convert(key, to_q4, dst):
        name = TO_Q4 if to_q4 else FROM_Q4
        out.append(([key], name, name[1:], {}, dst))

    est = {"gain": 0.0, "cost": 0.0}

    def need(key, want_q4):
        if key == "None" or key in inits or (key in q4) == want_q4:
            return key
        ck = copies.get((key, want_q4))
        if ck is None:
            if shapes.get(key.split("@")[0]) is not None:
                est["cost"] += _nbytes(shapes[key.split("@")[0]]) * _CONVERT_S_PER_BYTE
            ck = key + ("@q4" if want_q4 else "@nchw")
            convert(key, want_q4, ck)
            copies[(key, want_q4)] = ck
            if want_q4:
                q4.add(ck)
        return ck

    def drop_copies(key):
        for lay in (True, False):
            copies.pop((key, lay), None)

    last = len(steps) - 1
    pointwise = q4_pointwise_kinds()

    def ends_program(i, dst):
        """Step i is the program's last, or what it writes is handed out by the closing `return`."""
        return i == last or (kinds[steps[last][1]][0] == "return" and dst in steps[last][0]
                             and not any(dst in s_ for s_, _, _ in steps[i + 1:last]))
    for i, (srcs, name, dst) in enumerate(steps):
        kind, para = kinds[name]
        single = isinstance(dst, str)
        as_q4 = False
        if kind in ("conv", "conv_fused") and single and q4_conv_ok(srcs, para, inits, shapes):
            as_q4 = True
            full = list(srcs) + ["None"] * (6 - len(srcs))
            res = full[5]
            if res != "None" and (res in inits or not _is4d(shapes, res)):
                as_q4 = False
            else:
                # 1..3 input channels arriving as NCHW (the stem): the row-packed kernel reads a padded
                # NHWC copy it makes itself -- K without the 4th padding channel, no to_q4 step
                k = shapes[srcs[1]]
                rowpack = (os.environ.get("PLANER_HIP_ROWPACK", "1") != "0"
                           and full[0] not in q4 and k[1] < 4 and int(para.get("group", 1)) == 1
                           and list(para.get("dilations", (1, 1))) == [1, 1])
                args = [need(full[0], not rowpack)] + full[1:5] + [need(res, True)]
                new_kind = "conv_q4"
                if rowpack:
                    para = dict(para, rowpack=True)
                if shapes.get(dst) is not None:
                    k = shapes[srcs[1]]
                    est["gain"] += 2.0 * (_nbytes(shapes[dst]) / 4) * k[1] * k[2] * k[3] * _Q4_CONV_GAIN_S_PER_FLOP
        elif (kind in ("convtranspose", "convt_fused") and single and convt_ok(srcs, para, inits, shapes)
              and all(k == "None" or k in inits for k in srcs[2:5])
              and (len(srcs) < 6 or srcs[5] == "None" or (srcs[5] not in inits and _is4d(shapes, srcs[5])))):
            # the NCHW entry converts its input and output itself (layer.ConvTransposeFused): in Q4 those two passes go
            as_q4 = True
            full = list(srcs) + ["None"] * (6 - len(srcs))
            args = [need(full[0], True)] + full[1:5] + [need(full[5], True)]
            new_kind = "convt_q4"
            for k in (srcs[0], dst):
                if shapes.get(k) is not None:
                    est["gain"] += _nbytes(shapes[k]) * _CONVERT_S_PER_BYTE
        elif kind in pointwise and single and _q4_pointwise_ok(kind, srcs, para, inits, shapes, values) \
                and any(k in q4 for k in srcs) and not (is_linear(kind, para) and ends_program(i, dst)):
            # (a linear upsample that ends the program stays NCHW behind a from_q4 of its small input: the result has to be NCHW
            # anyway, and converting the large tensor costs more than converting the small one)
            as_q4 = True
            args = [need(k, True) for k in srcs]
            new_kind = kind + "_q4"
            if kind == "pixelshuffle" and not para.get("inverse") and ends_program(i, dst):
                # a shuffle that ends the program (an ESPCN tail) writes NCHW itself: no Q4 result, no from_q4 behind it
                para = dict(para, nchw_out=True)
        if not as_q4:
            args = [need(k, False) for k in srcs]
            new_kind = kind
        if kind in _IN_PLACE and kind in Q4_POINTWISE:   # (layer.py:46, 217-226, 250-251): cached copies of the input go stale
            drop_copies(srcs[0])                         # (not for `erf`, the in-place kind without a Q4 form: DESIGN, asymmetries)
        out_key = dst
        produces_q4 = as_q4 and kind != "gap" and not (kind == "pixelshuffle" and para.get("nchw_out"))
        if produces_q4 and i == last:
            out_key = dst + "@q4"                # the program's result is handed back as NCHW below
        out.append((args, name, new_kind, para, out_key))
        if kind == "clip" and not as_q4 and srcs[0] in q4 and i != last:
            # clipped in place on its NCHW copy (a partial quad that clip would dirty): later readers of the input must
            # see the clipped values, so the Q4 primary is made again from that copy
            convert(args[0], True, srcs[0])
        if (kind == "instancenormalization" and not as_q4 and srcs[0] in q4
                and any(srcs[0] in s_ for s_, _, _ in steps[i + 1:])):
            # likewise for an instance norm that stays NCHW (a scale computed by the graph, or the switch off) where the tensor it
            # rewrote has later readers
            convert(args[0], True, srcs[0])
        for k in _as_list(dst):
            q4.discard(k)
            drop_copies(k)
        if produces_q4:
            q4.add(out_key)
            nq4 += 1
            if i == last:
                convert(out_key, False, dst)
                if shapes.get(dst) is not None:
                    est["cost"] += _nbytes(shapes[dst]) * _CONVERT_S_PER_BYTE
        elif as_q4:
            nq4 += 1
    if not force and est["cost"] > est["gain"]:
        return [list(b) for b in body], [[list(srcs), [name], dst] for srcs, name, dst in steps], 0
    return view.emit(out) + (nq4,)


# ---- instance norm and group norm tails ------------------------------------------------------------------
# the channel-quad norms whose kernels take [+ res] [relu] in their write pass -> the number of sources of an unfused step
_NORM_Q4_SRCS = {"instancenormalization_q4": 3, "groupnorm_q4": 5}


def fuse_instnorm_q4(body, flow, shapes):
    """-> (body', flow', number of absorbed steps).  Runs on assign_layouts' program (one layer per step).  Folds
    instancenormalization_q4 -> [add_q4 with an operand of the same shape] -> [relu_q4]  into ONE instancenormalization_q4 step
    with `res` and `act` set (q4.InstanceNormQ4: the tail goes into the kernel's write pass), and groupnorm_q4 likewise
    (q4.GroupNormQ4: `res` behind gamma and beta).  The order is fixed -- residual,
    then activation -- so a relu that comes first ends the chain and the add behind it stays a step of its own.  As in
    fuse_flow a link is absorbed only when the tensor between has one reader and one writer, and the fused step sits where the
    last link was.  The norm works in place, so it is only moved when nothing else ever reads the tensor it rewrites."""
    view = Steps(body, flow)
    steps, readers, writers = view.steps, view.readers, view.writers
    consumed, fused_at, nfused = set(), {}, 0
    for i, (srcs, name, dst) in enumerate(steps):
        kind, para = view.layers[name]
        if _NORM_Q4_SRCS.get(kind) != len(srcs) or i in consumed or not isinstance(dst, str):
            continue
        if readers.get(srcs[0]) != [i] or len(writers.get(srcs[0], ())) > 1:
            continue
        chain, cur, res, act = [i], dst, "None", ACT_NONE
        while act == ACT_NONE:
            j = view.only_reader(chain[-1], cur)
            if j is None or j in consumed or not isinstance(steps[j][2], str):
                break
            jsrcs, jname, jdst = steps[j]
            jkind = view.kind(j)
            if (jkind == "add_q4" and res == "None" and len(jsrcs) == 2 and jsrcs.count(cur) == 1
                    and _shape(shapes, jsrcs[0]) is not None and _shape(shapes, jsrcs[0]) == _shape(shapes, jsrcs[1])):
                res = jsrcs[1 - jsrcs.index(cur)]
            elif jkind == "relu_q4" and jsrcs == [cur]:
                # the residual is now read at j: nothing may rewrite it between the add and here
                if res != "None" and view.clobbered(res, chain[-1], j):
                    break
                act = ACT_RELU
            else:
                break
            chain.append(j)
            cur = jdst
        if len(chain) > 1:
            consumed.update(chain)
            fused_at[chain[-1]] = (srcs + [res], name + "+", kind, dict(para, act=act), cur)
            nfused += len(chain) - 1
    return view.emit(view.spliced(fused_at, consumed)) + (nfused,)


# ---- linear upsample + add ---------------------------------------------------------------------------
LINEAR_ADD_KINDS = {"upsample_q4": "upsample_add_q4", "resize_q4": "resize_add_q4"}


def fuse_linear_add(body, flow, shapes):
    """-> (body', flow', number of absorbed adds).  Runs on assign_layouts' program (one layer per step).  A linear `upsample_q4`
    / `resize_q4` whose result has one reader and one writer, that reader an `add_q4` of two equal known shapes, becomes ONE
    `upsample_add_q4` / `resize_add_q4` step (q4.UpSampleAddQ4 / ResizeAddQ4: the add's other operand, in either position, goes
    into the kernel's write pass as a rounding of its own).  The fused step sits where the add was, so the upsample now reads its
    source there: not fused where a step between the two rewrites that source in place (`_IN_PLACE`) or writes it, or writes the
    other operand.  fuse_flow has already put an add behind a conv into that conv's epilogue; this takes what is left -- the
    second and later terms of a sum of upsampled maps."""
    view = Steps(body, flow)
    steps, consumed, fused_at = view.steps, set(), {}
    for i, (srcs, name, dst) in enumerate(steps):
        kind, para = view.layers[name]
        if kind not in LINEAR_ADD_KINDS or not is_linear(kind, para):
            continue
        j = view.only_reader(i, dst)
        if j is None or j in consumed:
            continue
        jsrcs, jname, jdst = steps[j]
        if (view.kind(j) != "add_q4" or not isinstance(jdst, str) or len(jsrcs) != 2 or jsrcs.count(dst) != 1
                or _shape(shapes, jsrcs[0]) is None or _shape(shapes, jsrcs[0]) != _shape(shapes, jsrcs[1])):
            continue
        res = jsrcs[1 - jsrcs.index(dst)]
        if view.clobbered(srcs[0], i, j) or view.clobbered(res, i, j, in_place=()):
            continue
        if kind == "upsample_q4":
            args = [srcs[0], srcs[1], res]
        else:
            args = (srcs + ["None"] * 4)[:4] + [res]
        consumed.update((i, j))
        fused_at[j] = (args, name + "+", LINEAR_ADD_KINDS[kind], para, jdst)
    return view.emit(view.spliced(fused_at, consumed)) + (len(fused_at),)


# ---- pixel shuffle / unshuffle ---------------------------------------------------------------------------------------------------
# planer has no depth-to-space kind (the operator table is the reference's): a sub-pixel convolution's shuffle arrives as what an
# exporter writes, reshape -> transpose (6-D) -> reshape.  As three steps it drops out of Q4 -- from_q4, the 6-D transpose, to_q4
# -- on the largest tensors of a super-resolution net.  fuse_pixel_shuffle names the trio (`pixelshuffle`, layer.PixelShuffle: the
# same three steps) so that assign_layouts can give it its one-pass Q4 kernel (q4.PixelShuffleQ4).
# PLANER_HIP_PIXEL_SHUFFLE_Q4=0 skips the pass: the program of a compiler without it.
PIXEL_SHUFFLE_R = (2, 3, 4)


def pixel_shuffle_enabled():
    return os.environ.get("PLANER_HIP_PIXEL_SHUFFLE_Q4", "1") != "0"


def match_pixel_shuffle(s_in, s_mid, axis, s_out):
    """-> {"r", "order", "inverse"} where reshape(s_in -> s_mid), transpose(axis), reshape(-> s_out) is a pixel shuffle or
    unshuffle by r = 2, 3, 4 (the four forms of layer.PIXEL_SHUFFLE_AXES, both r extents equal, every shape as the form has it),
    else None."""
    if s_in is None or s_mid is None or s_out is None or len(s_in) != 4 or len(s_mid) != 6 or len(s_out) != 4:
        return None
    for (order, inverse), ax in PIXEL_SHUFFLE_AXES.items():
        if [int(a) for a in axis] != ax:
            continue
        r = int(s_mid[3] if inverse else s_mid[2] if order == "crd" else s_mid[1])
        if r not in PIXEL_SHUFFLE_R:
            return None
        want = pixel_shuffle_shapes(s_in, r, order, inverse)
        if want is None or tuple(s_mid) != want[0] or tuple(s_out) != want[1]:
            return None
        return {"r": r, "order": order, "inverse": inverse}
    return None


def fuse_pixel_shuffle(body, flow, shapes):
    """-> (body', flow', number of trios).  Runs on fuse_flow's program, in front of assign_layouts.  A `reshape` of a 4-D tensor
    to 6-D, a `transpose` of that by one of the four permutations, and a `reshape` back to 4-D become ONE `pixelshuffle` step
    {r, order, inverse} where the traced `shapes` say so (match_pixel_shuffle) -- the shapes alone, so a shape operand computed by
    shape-domain steps is as good as a constant one -- and both intermediates have exactly one writer and one reader.  The step
    sits where the last reshape was and reads the first reshape's input there: not fused where a step between rewrites that input
    in place or writes it.  Steps that only fed the reshapes' shape operands stay where they are."""
    view = Steps(body, flow)
    kinds, steps = view.layers, view.steps

    def only_reader(i, dst, kind):
        """view.only_reader where that step is of `kind` with `dst` its first operand and writes one tensor."""
        j = view.only_reader(i, dst)
        if j is None:
            return None
        jsrcs, _, jdst = steps[j]
        return j if view.kind(j) == kind and jsrcs[0] == dst and jsrcs.count(dst) == 1 and isinstance(jdst, str) else None

    consumed, fused_at, names = set(), {}, {b[0] for b in body}
    for i, (srcs, name, dst) in enumerate(steps):
        if kinds[name][0] != "reshape" or i in consumed or len(srcs) != 2:
            continue
        j = only_reader(i, dst, "transpose")
        if j is None or j in consumed or len(steps[j][0]) != 1:
            continue
        k = only_reader(j, steps[j][2], "reshape")
        if k is None or k in consumed or len(steps[k][0]) != 2:
            continue
        x, out = srcs[0], steps[k][2]
        form = match_pixel_shuffle(shapes.get(x), shapes.get(dst), kinds[steps[j][1]][1].get("axis", ()), shapes.get(out))
        if form is None or tuple(shapes.get(steps[j][2]) or ()) != tuple(shapes[dst][a] for a in PIXEL_SHUFFLE_AXES[(form["order"], form["inverse"])]):
            continue
        if view.clobbered(x, i, k, skip=(j,)):
            continue
        new = steps[j][1] + "+"
        while new in names:                      # a transpose layer that serves several steps: one pixelshuffle layer per trio
            new += "+"
        names.add(new)
        consumed.update((i, j, k))
        fused_at[k] = ([x], new, "pixelshuffle", form, out)
    return view.emit(view.spliced(fused_at, consumed)) + (len(fused_at),)


# ---- group normalisation -----------------------------------------------------------------------------------------------------------
# planer has no group-norm kind (the operator table is the reference's): below opset 18 an exporter writes one as reshape (N, G, -1)
# -> instancenormalization (G scales / biases, ones and zeros) -> reshape back -> mul gamma (C, 1, 1) -> add beta (C, 1, 1).  reshape
# and mul have no channel-quad kind and add only for equal shapes, so between two convs the five steps ran NCHW between a from_q4 and
# a to_q4.  fuse_groupnorm names them (`groupnorm`, layer.GroupNorm: the same five steps) so that assign_layouts can give the norm
# its one-launch Q4 kernel (q4.GroupNormQ4).  PLANER_HIP_GROUPNORM_Q4=0 skips the pass: the program of a compiler
# without it.
def groupnorm_enabled():
    return os.environ.get("PLANER_HIP_GROUPNORM_Q4", "1") != "0"


def _per_channel(shape, c):
    """An operand that squeezes to c values on the channel axis of an NCHW tensor: (c, 1, 1) or (1, c, 1, 1)."""
    return shape is not None and tuple(int(v) for v in shape) in ((c, 1, 1), (1, c, 1, 1))


def fuse_groupnorm(body, flow, shapes, init_names=None):
    """-> (body', flow', number of norms).  Runs on fuse_flow's program, in front of assign_layouts.  A `reshape` of a 4-D
    (N, C, H, W) tensor x to (N, G, *rest) with G | C, an `instancenormalization` of that with constant scale and bias of G values, a
    `reshape` back to exactly x's shape, then optionally a `mul` and optionally an `add` whose other operand -- in either position
    -- is a constant of C values shaped (C, 1, 1) or (1, C, 1, 1), become ONE `groupnorm` step {groups, epsilon} with sources
    [x, scale, bias, gamma | "None", beta | "None"].  Matched on the traced `shapes`, so a shape operand computed by shape-domain
    steps is as good as a constant one.  Every intermediate has one writer and one reader; the norm rewrites x in place, so x must
    have no reader but the first reshape, and nothing may write it between the first step and the last.  A constant is a key no
    step writes (and one of `init_names` where they are given).  The step sits where the last link was; steps that only fed the
    reshapes' shape operands stay where they are."""
    view = Steps(body, flow)
    kinds, steps, readers, writers = view.layers, view.steps, view.readers, view.writers
    inits = None if init_names is None else set(init_names)

    def const(key):
        return key != "None" and key not in writers and (inits is None or key in inits)

    def only_reader(i, dst):
        """view.only_reader where that step is not part of an earlier pattern and writes one tensor."""
        j = view.only_reader(i, dst)
        return j if j is not None and j not in consumed and isinstance(steps[j][2], str) else None

    def channel_operand(j, cur, kind, c):
        """The constant per-channel operand of step j where that is a `kind` of `cur` and such a constant, else None."""
        if j is None:
            return None
        jsrcs, jname, _ = steps[j]
        if kinds[jname][0] != kind or len(jsrcs) != 2 or jsrcs.count(cur) != 1:
            return None
        other = jsrcs[1 - jsrcs.index(cur)]
        return other if const(other) and _per_channel(shapes.get(other), c) else None

    consumed, fused_at, names = set(), {}, {b[0] for b in body}
    for i, (srcs, name, dst) in enumerate(steps):
        if kinds[name][0] != "reshape" or i in consumed or len(srcs) != 2:
            continue
        x = srcs[0]
        sx, sm = shapes.get(x), shapes.get(dst)
        if sx is None or sm is None or len(sx) != 4 or len(sm) < 3 or readers.get(x) != [i] or len(writers.get(x, ())) > 1:
            continue
        n, c = int(sx[0]), int(sx[1])
        g = int(sm[1])
        if int(sm[0]) != n or g < 1 or c % g:
            continue
        j = only_reader(i, dst)
        if j is None or kinds[steps[j][1]][0] != "instancenormalization":
            continue
        nsrcs, nname, ndst = steps[j]
        if (len(nsrcs) != 3 or nsrcs[0] != dst or not all(const(k) and tuple(shapes.get(k) or ()) == (g,) for k in nsrcs[1:])):
            continue
        k = only_reader(j, ndst)
        if (k is None or kinds[steps[k][1]][0] != "reshape" or len(steps[k][0]) != 2 or steps[k][0][0] != ndst
                or tuple(shapes.get(steps[k][2]) or ()) != tuple(sx)):
            continue
        chain, cur, gamma, beta = [i, j, k], steps[k][2], "None", "None"
        m = only_reader(k, cur)
        got = channel_operand(m, cur, "mul", c)
        if got is not None:
            chain, cur, gamma = chain + [m], steps[m][2], got
            m = only_reader(m, cur)
        got = channel_operand(m, cur, "add", c)
        if got is not None:
            chain, cur, beta = chain + [m], steps[m][2], got
        if view.clobbered(x, i, chain[-1] + 1, chain, in_place=()):
            continue
        new = nname + "+"
        while new in names:                      # a norm layer that serves several steps: one groupnorm layer per pattern
            new += "+"
        names.add(new)
        consumed.update(chain)
        para = {"groups": g, "epsilon": kinds[nname][1].get("epsilon", 1e-5)}
        fused_at[chain[-1]] = ([x, nsrcs[1], nsrcs[2], gamma, beta], new, "groupnorm", para, cur)
    if not fused_at:
        return _copy_of(body, flow) + (0,)
    return view.emit(view.spliced(fused_at, consumed)) + (len(fused_at),)


# ---- Winograd chaining ------------------------------------------------------------------------------
# A conv_q4 step that runs F(4x4,3x3) (w_layout 7) is three kernels: input transform (x -> V), the 36
# grouped GEMMs (V, U -> M) and output transform + fused tail (M -> y).  When the y of one such conv
# feeds another, "M -> y -> V'" can be ONE kernel that keeps y on chip (csrc/wino4_chain_kernel.h), and
# when nothing else reads y it is never written at all.  `chain_winograd` makes the stages explicit plan
# steps and merges the out / in pairs.  A Winograd input transform may be hoisted over the kinds that only read their inputs
# (`_PURE_READERS`: no in-place update).


def chain_winograd(body, flow, supported=lambda key: True, chain=True):
    """-> (body', flow', number of chained pairs).  `flow` holds one layer per step (as made by
    assign_layouts / lower); `supported(key)` says whether the LDS transform kernel
    can take the activation `key` (whole planes must fit a workgroup's LDS)."""
    view = Steps(body, flow)
    steps = []                      # [srcs, name, kind, para, dst]: the view's steps with the staged convs taken apart
    for srcs, name, kind, para, dst in view.each():
        if kind == "conv_q4" and para.get("w_layout") in STAGED_LAYOUTS and isinstance(dst, str):
            full = srcs + ["None"] * (6 - len(srcs))
            tail = {k: para[k] for k in ("act", "alpha") if k in para}
            pre = STAGED_LAYOUTS[para["w_layout"]]
            steps.append([[full[0]], name + "@in", pre + "_in", {}, name + "@V"])
            steps.append([[name + "@V", full[1]], name + "@gemm", pre + "_gemm", {}, name + "@M"])
            steps.append([[name + "@M"] + full[2:6], name + "@out", pre + "_out", tail, dst])
        else:
            steps.append([srcs, name, kind, para, dst])
    nchained = 0
    if chain:
        last_dsts = set(_as_list(steps[-1][4])) if steps else set()
        i = 0
        while i < len(steps):
            srcs, name, kind, para, dst = steps[i]
            if kind in ("wino4_out", "wino43_out") and (kind == "wino43_out" or supported(dst)):
                pre = kind[:-len("_out")]
                readers = [j for j in range(i + 1, len(steps)) if dst in steps[j][0]]
                # overwritten later under the same key?  then only readers before that point count
                rewrite = [j for j in range(i + 1, len(steps)) if dst in _as_list(steps[j][4])]
                stop = rewrite[0] if rewrite else len(steps)
                readers = [j for j in readers if j <= stop]
                j = next((j for j in readers if steps[j][2] == pre + "_in" and steps[j][0] == [dst]), None)
                if j is not None and all(steps[k][2] in _PURE_READERS for k in readers if k < j):
                    vkey = steps[j][4]
                    keep = len(readers) > 1 or dst in last_dsts
                    base = name[:-len("@out")]
                    steps[i] = [srcs, base + "@chain", pre + "_chain", dict(para, keep_y=keep), [dst, vkey] if keep else vkey]
                    del steps[j]
                    nchained += 1
            i += 1
    return view.emit(steps) + (nchained,)


# ---- 1x1 conv -> staged Winograd conv ----------------------------------------------------------------------
def fuse_conv1x1_wino_in(body, flow, kshape=lambda key: None, small=lambda key: True):
    """-> (body', flow', number of fused pairs).  A direct channel-quad 1x1 conv (w_layout 2, stride 1, no padding, group 1,
    no residual) whose ONLY reader is the input-transform stage of a staged F(4x4,3x3) conv (`wino4_in`, made explicit by
    chain_winograd) becomes one `conv1x1_wino_in` step that writes that stage's V (q4.Conv1x1WinoIn): the 1x1 -> 3x3 pairs of a
    Darknet block.  `small(key)` says whether the activation is small enough for the launch saved to matter (the fused kernel
    computes the 1x1 conv on overlapping patches: 1.9x its multiplies)."""
    view = Steps(body, flow)
    steps, readers, writers = view.steps, view.readers, view.writers
    last_dsts = set(_as_list(steps[-1][2])) if steps else set()
    drop, repl, nfused = set(), {}, 0
    for i, (srcs, name, dst) in enumerate(steps):
        if view.kind(i) != "wino4_in" or len(srcs) != 1:
            continue
        y = srcs[0]
        if len(writers.get(y, [])) != 1 or readers.get(y, []) != [i] or y in last_dsts:
            continue
        j = writers[y][0]
        csrcs, cname, cdst = steps[j]
        ckind, cpara = view.layers[cname]
        full = csrcs + ["None"] * (6 - len(csrcs))
        if j >= i or j in drop or ckind != "conv_q4" or cpara.get("w_layout") != DIRECT_Q4 or not isinstance(cdst, str) or full[5] != "None":
            continue
        k = kshape(full[1])
        if (k is None or tuple(k[2:]) != (1, 1) or k[0] % 4 or int(cpara.get("group", 1)) != 1
                or [int(v) for v in cpara.get("strides", (1, 1))] != [1, 1] or [int(v) for v in cpara.get("dilations", (1, 1))] != [1, 1]
                or any(int(v) for v in cpara.get("pads", (0, 0, 0, 0))) or int(cpara.get("act", 0)) & ~3 or not small(y)):
            continue
        fname = cname + "@v4"
        repl[j] = (full[:5], fname, "conv1x1_wino_in", {"act": int(cpara.get("act", 0)), "alpha": float(cpara.get("alpha", 0.0)), "wino": 4}, dst)
        drop.add(i)
        nfused += 1
    return view.emit(view.spliced(repl, drop)) + (nfused,)


# ---- sibling convolutions --------------------------------------------------------------------------------
# Where a graph forks into two direct channel-quad convs on the same tensor -- a ResNet block that changes resolution:
# the stride-2 3x3 conv and the 1x1 stride-2 projection -- both run in ONE launch (q4.ConvQ4Pair,
# csrc/conv_q4_kernel.h conv_q4_pair_kernel).  The second conv moves up to the first one's place; it only needs the
# shared input and constants, so that is legal unless something rewrites the input in place (`_IN_PLACE`) in between.


def pair_sibling_convs(body, flow, kshape=lambda key: None):
    """-> (body', flow', number of pairs).  One layer per step, as made by lower.  `kshape(key)` gives
    the OIHW shape of a filter key; only the projection pattern is paired -- equal strides > 1, one of the two a 1x1 --
    because both convs then have the same output map and neither wants a split-K plan of its own."""
    view = Steps(body, flow)
    steps = view.steps

    def direct(i):
        srcs, name, kind, para, dst = view.step(i)
        full = srcs + ["None"] * (6 - len(srcs))
        return (kind == "conv_q4" and para.get("w_layout") == DIRECT_Q4 and isinstance(dst, str) and full[5] == "None"
                and int(para.get("group", 1)) == 1 and [int(v) for v in para.get("dilations", (1, 1))] == [1, 1]
                and not para.get("rowpack") and not (int(para.get("act", 0)) & ~3))

    used, npairs, out = set(), 0, []
    for i in range(len(steps)):
        if i in used:
            continue
        srcs, name, dst = steps[i]
        j = None
        if direct(i):
            for k in range(i + 1, len(steps)):
                ks, kname, kdst = steps[k]
                if view.clobbers(k, srcs[0]):
                    break                                   # the shared input is rewritten: later readers see other values
                # the flow's LAST step defines the program's result (net.py:72): hoisting it would make another step last
                if k not in used and k != len(steps) - 1 and i != len(steps) - 1 and direct(k) and ks[0] == srcs[0]:
                    p1, p2 = view.layers[name][1], view.layers[kname][1]
                    k1, k2 = kshape(srcs[1]), kshape(ks[1])
                    st1, st2 = [int(v) for v in p1.get("strides", (1, 1))], [int(v) for v in p2.get("strides", (1, 1))]
                    if (k1 is not None and k2 is not None and st1 == st2 and min(st1) > 1
                            and min(k1[2] * k1[3], k2[2] * k2[3]) == 1):
                        j = k
                        break
        if j is None:
            out.append(view.step(i))
            continue
        s2, n2, d2 = steps[j]
        f1, f2 = srcs + ["None"] * (6 - len(srcs)), s2 + ["None"] * (6 - len(s2))
        pname = name + "&" + n2
        out.append(([f1[0]] + f1[1:5] + f2[1:5], pname, "conv_q4_pair",
                    {"para1": dict(view.layers[name][1]), "para2": dict(view.layers[n2][1])}, [dst, d2]))
        used.add(j)
        npairs += 1
    return view.emit(out) + (npairs,)


# ---- dilated 3x3 convs on the Winograd kernels: pixel-phase folding ------------------------------------------------------------
# A 3x3 / stride 1 conv with dilation (dh, dw) and pads (dh, dw, dh, dw) is dh * dw independent 3x3 / pad 1 convs, one per pixel
# phase x[:, :, i::dh, j::dw].  With the phases moved into the batch axis (q4.refold_q4: the tensor "folded by (dh, dw)") it is
# an ordinary conv on (N dh dw, C, ceil(H/dh), ceil(W/dw)) that every Winograd layout takes.  Where dh | H and dw | W the folded
# tensor has no zero-fill cells and position-independent steps run on it as they are, so a run of dilated convs is folded once
# on the way in and unfolded once on the way out.  On other maps the conv leaves junk in the zero-fill cells -- the next
# folded conv would read it as padding -- so it folds alone: in, conv, out.
FOLD_SEP = "~"
REFOLD = "@refold_q4"


def folded_key(key, fold, junk=False):
    """The key of tensor `key` folded by `fold`: the part before the first "@" -- what every pass looks shapes up by -- gets the
    fold, so the folded tensor has a shape entry of its own.  `junk`: the output of a conv that folds alone, whose zero-fill
    cells hold junk -- a key of its own, so that a clean folded copy of the same tensor can exist beside it."""
    if tuple(fold) == (1, 1):
        return key
    base = key.split("@")[0]
    return "%s%s%dx%d%s%s" % (base, FOLD_SEP, fold[0], fold[1], "j" if junk else "", key[len(base):])


def _folded_shape(shape, fold):
    n, c, h, w = shape
    return (n * fold[0] * fold[1], c, -(-h // fold[0]), -(-w // fold[1]))


def _act_positions(kind, srcs):
    """Positions of the activation operands of a step that can run on folded tensors (the others are constants)."""
    if kind == "conv_q4":
        return [0] + ([5] if len(srcs) > 5 and srcs[5] != "None" else [])
    if kind == "batchnorm_q4":
        return [0]
    return [i for i, k in enumerate(srcs) if k != "None"]


def fold_dilated(body, flow, shapes, worth=lambda x_shape, k_shape, para: True):
    """-> (body', flow', regions).  Runs on assign_layouts' program (one layer per step).  A `conv_q4` step is a HEAD when it
    has a constant 4-D 3x3 filter, strides [1, 1], dilations [dh, dw] with dh * dw > 1, pads [dh, dw, dh, dw], is neither
    depthwise nor row-packed, would be w1d_q4_eligible at dilation 1 / pad 1, and `worth(x_shape, k_shape, para)` agrees.  It is
    rewritten to dilation 1 / pad 1 on its input folded by (dh, dw) -- same filter key, so prepared filters are shared with
    undilated users.  Where dh | H and dw | W, steps of position-independent kinds that read a tensor folded by (dh, dw) JOIN:
    other heads of that dilation, 1x1 / stride 1 / pad 0 convs, relu / leakyrelu / clip / sigmoid / batchnorm / add and concat
    along channels; all their activation operands are brought to the fold.  Everything else reads unfolded tensors, and the
    program's result is unfolded.  One fold state per key as in assign_layouts' `need`: `refold_q4` steps are inserted where a
    value is needed in a fold it does not have (fold to fold directly), converted copies are cached per (key, fold) and dropped
    when a step rewrites their tensor in place.  Folded tensors get keys of their own (`folded_key`) and `shapes` gains their
    shapes.  `regions`: one {"fold", "dividing", "heads", "steps"} per run of steps that share folded tensors."""
    from .conv_layouts import w1d_q4_eligible
    view = Steps(body, flow)
    steps = view.steps
    forms = {}            # key -> the folds it exists in, the one it was produced in first; absent: unfolded only
    region_of = {}        # key -> index of the region that produced it folded
    copy_region = {}      # (key, fold) -> index of the region a folded copy of an operand was first made for
    out, regions = [], []

    def shape(key):
        s = shapes.get(key.split("@")[0])
        return tuple(s) if s is not None and len(s) == 4 else None

    def refold(key, src, fold, dst):                     # one layer per (from, to) pair: a layer's parameters are its own
        out.append(([key], "%s:%dx%d>%dx%d" % ((REFOLD,) + src + fold), "refold_q4", {"to": list(fold), "from": list(src)}, dst))

    def need(key, fold):
        if key == "None":
            return key
        have = forms.setdefault(key, [(1, 1)])
        if fold not in have:
            src = have[0]
            refold(folded_key(key, src), src, fold, folded_key(key, fold))
            have.append(fold)
            if fold != (1, 1) and shape(key) is not None:
                shapes[folded_key(key, fold).split("@")[0]] = _folded_shape(shape(key), fold)
        return folded_key(key, fold)

    def head_fold(kind, para, srcs):
        if kind != "conv_q4" or para.get("rowpack") or len(srcs) < 2:
            return None
        k, x = shapes.get(srcs[1]), shape(srcs[0])
        d = [int(v) for v in para.get("dilations", (1, 1))]
        if k is None or x is None or len(k) != 4 or len(d) != 2 or d[0] * d[1] <= 1 or min(d) < 1:
            return None
        group = int(para.get("group", 1))
        if ([int(v) for v in para.get("pads", (0, 0, 0, 0))] != [d[0], d[1], d[0], d[1]] or dw_q4_eligible(tuple(k), group)
                or not w1d_q4_eligible(tuple(k), group, para.get("strides", (1, 1)), (1, 1), (1, 1, 1, 1))):
            return None
        return (d[0], d[1]) if worth(x, tuple(k), dict(para)) else None

    def joins(kind, para, srcs, fold):
        """A position-independent step with an operand whose tensor is folded by `fold` (and, for a conv, the right geometry)."""
        if not any(forms.get(srcs[p], [(1, 1)])[0] == fold for p in _act_positions(kind, srcs)):
            return False
        if kind == "conv_q4":
            k = shapes.get(srcs[1])
            return (not para.get("rowpack") and k is not None and len(k) == 4 and tuple(k[2:]) == (1, 1)
                    and [int(v) for v in para.get("strides", (1, 1))] == [1, 1] and not any(int(v) for v in para.get("pads", (0, 0, 0, 0))))
        if kind == "concat_q4":
            return int(para.get("axis", 0)) in (1, -3)
        return kind in _FOLD_POINTWISE

    last = len(steps) - 1
    for i, (srcs, name, dst) in enumerate(steps):
        kind, para = view.layers[name]
        fold, head = None, False
        if isinstance(dst, str):
            fold = head_fold(kind, para, srcs)
            head = fold is not None
            if not head:
                # the folds its operands are in, in operand order: the step joins the first it can run in
                for p in (_act_positions(kind, srcs) if kind == "conv_q4" or kind in _FOLD_POINTWISE else []):
                    f = forms.get(srcs[p], [(1, 1)])[0]
                    if f != (1, 1) and joins(kind, para, srcs, f):
                        fold = f
                        break
        if fold is None:
            args = [need(k, (1, 1)) if k in forms else k for k in srcs]
            out.append((args, name, kind, para, dst))
            if kind in _IN_PLACE and srcs:
                forms[srcs[0]] = [(1, 1)]
            for k in _as_list(dst):
                forms[k] = [(1, 1)]
                region_of.pop(k, None)
            continue
        x = shape(srcs[0])
        dividing = x is not None and x[2] % fold[0] == 0 and x[3] % fold[1] == 0
        acts = _act_positions(kind, srcs)
        # the region: that of an operand already folded this way, else a new one
        reg = next((region_of[srcs[p]] for p in acts if srcs[p] in region_of and forms.get(srcs[p], [None])[0] == fold), None)
        if reg is None:                                 # ... or that of the step a cached folded copy of an operand was made for
            reg = next((copy_region[(srcs[p], fold)] for p in acts
                        if (srcs[p], fold) in copy_region and fold in forms.get(srcs[p], [])), None)
        if reg is None or not dividing:
            regions.append({"fold": list(fold), "dividing": bool(dividing), "heads": [], "steps": []})
            reg = len(regions) - 1
        args = list(srcs)
        for p in acts:
            args[p] = need(srcs[p], fold)
            if dividing:
                copy_region.setdefault((srcs[p], fold), reg)
        if head:
            para = dict(para, dilations=[1, 1], pads=[1, 1, 1, 1])
            regions[reg]["heads"].append(name)
        regions[reg]["steps"].append(name)
        fdst = folded_key(dst, fold, junk=not dividing)
        out.append((args, name, kind, para, fdst))
        if kind in _FOLD_IN_PLACE:
            forms[srcs[0]] = [fold]                     # rewritten in this fold: the other copies are stale
        ys = shape(dst)
        if ys is not None:
            shapes[fdst.split("@")[0]] = _folded_shape(ys, fold)
        forms[dst] = [fold]
        region_of[dst] = reg
        if not dividing or i == last:
            # zero-fill cells hold junk behind the conv: nothing may read this tensor folded.  (And a program ends unfolded.)
            refold(fdst, fold, (1, 1), dst)
            forms[dst] = [(1, 1)]
            region_of.pop(dst, None)
    if not regions:
        return _copy_of(body, flow) + ([],)
    return view.emit(out) + (regions,)


# ---- peepholes behind the filter choice (`body` is {name: entry} there and is rewritten in place) ---------------------------------
def fuse_upsample_concat(body, flow):
    """upsample_q4 whose only reader is a two-input concat_q4 (axis 1) that takes it FIRST -> one upconcat_q4 step
    (detection-net routes: the upsampled tensor is written once, into its place in the concatenation)."""
    view = Steps(body.values(), flow)                    # (one layer per step: step i is flow[i])
    drop, out = set(), {}
    for i, (src, names, dst) in enumerate(flow):
        entry = body[names[0]]
        if (entry[1] == "upsample_q4" and isinstance(dst, str) and isinstance(src, list) and len(src) == 2
                and entry[2].get("mode", "nearest") == "nearest" and len(view.readers.get(dst, [])) == 1):
            j = view.readers[dst][0]
            csrc, cnames, cdst = flow[j]
            ce = body[cnames[0]]
            if (ce[1] == "concat_q4" and len(cnames) == 1 and isinstance(csrc, list) and len(csrc) == 2 and csrc[0] == dst != csrc[1]
                    and int(ce[2].get("axis", 0)) == 1 and i < j
                    # the upsample now reads its source at step j: nobody may read it in between (in-place ReLU)
                    and not view.clobbered(src[0], i, j, in_place=None, writes=False)):
                body[cnames[0]] = [ce[0], "upconcat_q4", {"mode": "nearest", "axis": 1}]
                out[j] = [[src[0], src[1], csrc[1]], cnames, cdst]
                drop.add(i)
    return [out.get(i, f) for i, f in enumerate(flow) if i not in drop]


def fuse_stem_pool(body, flow, shapes, kshape, eligible, prepare):
    """conv_q4 (row-packed stem, w_layout 6, no residual) whose only reader is maxpool_q4(w=3x3, strides 2, pads 1) -> one
    conv_pool_q4 step: the full-resolution tensor is never written.  `eligible(x shape, filter shape, para)` -> None, or the
    w_layout that takes the conv and its extra parameters (lower's `stem_pool`); STEM_POOL_NCHW reads the NCHW batch itself (no
    row-packed copy) with the filter in its own k order, which `prepare` makes."""
    readers = Steps(body.values(), flow).readers
    drop, out = set(), []
    for i, (src, names, dst) in enumerate(flow):
        entry = body[names[0]]
        if (entry[1] == "conv_q4" and entry[2].get("w_layout") == ROWPACK_Q4 and isinstance(dst, str)
                and (len(src) < 6 or src[5] == "None") and len(readers.get(dst, [])) == 1 and i != len(flow) - 1):
            j = readers[dst][0]
            psrc, pnames, pdst = flow[j]
            pe = body[pnames[0]]
            xs, ks = shapes.get(src[0].split("@")[0]), kshape(src[1])
            para = conv_para(entry[2])
            got = None
            if (pe[1] == "maxpool_q4" and len(pnames) == 1 and (psrc == dst or psrc == [dst]) and xs is not None
                    and [int(v) for v in pe[2].get("w", (2, 2))] == [3, 3]
                    and [int(v) for v in pe[2].get("strides", (2, 2))] == [2, 2]
                    and [int(v) for v in pe[2].get("pads", (0, 0, 0, 0))] == [1, 1, 1, 1]
                    and int(entry[2].get("act", 0)) in (0, 1, 2)):
                got = eligible(tuple(xs), tuple(ks), para)
            if got is not None:
                (lay, extra), fsrc, packed = got, list(src[:5]), suffix(ROWPACK_Q4, para)
                if lay == STEM_POOL_NCHW and src[1].endswith(packed):
                    fsrc[1] = prepare(lay, src[1][:-len(packed)], para)
                elif lay == STEM_POOL_NCHW:
                    lay, extra = STEM_POOL, {}
                body[names[0]] = [entry[0], "conv_pool_q4", dict(entry[2], w_layout=lay, **extra)]
                out.append([fsrc, names, pdst])
                drop.add(j)
                continue
        if i not in drop:
            out.append([src, names, dst])
    return out


# ---- the compiler: the passes in the order they run ------------------------------------------------------------------------------
# Net._fuse and the host tests both compile through compile_front and lower, so the order is written here only.  What needs a
# device or the weights -- timing conv candidates, preparing filters, kernel limits -- comes in through the caller; the defaults
# are what a host without either answers.
FRONT = ("fuse_flow", "fuse_pixel_shuffle", "fuse_groupnorm", "assign_layouts", "fuse_instnorm_q4", "fuse_linear_add", "fold_dilated")


def compile_front(layers, flow, inits, shapes, fuse=True, q4=True, values=None, worth=None, stop=None):
    """The front half of a compile: the passes of FRONT in that order, up to and including `stop` (a name in FRONT; None: all).
    -> (body, flow, {pass that ran: the third value it returned}).  fuse: epilogue fusion (fuse_flow).  q4: channel-quad
    activations, False / True / "force" (assign_layouts' `force`); without it only fuse_flow runs.  values: key -> host array of
    an init, or None.  worth: fold_dilated's callback; None leaves dilated convs as they are.  PLANER_HIP_PIXEL_SHUFFLE_Q4 and
    PLANER_HIP_GROUPNORM_Q4 are read here, at each call."""
    run = {
        "fuse_flow": fuse and (lambda b, f: fuse_flow(b, f, inits, shapes)),
        # reshape -> transpose -> reshape that is a pixel shuffle / unshuffle as one step, which has a one-pass Q4 kernel
        "fuse_pixel_shuffle": q4 and pixel_shuffle_enabled() and (lambda b, f: fuse_pixel_shuffle(b, f, shapes)),
        # reshape -> instancenormalization -> reshape -> [mul] -> [add] that is a group norm as one step, which has a Q4 kernel
        "fuse_groupnorm": q4 and groupnorm_enabled() and (lambda b, f: fuse_groupnorm(b, f, shapes, inits)),
        "assign_layouts": q4 and (lambda b, f: assign_layouts(b, f, inits, shapes, force=q4 == "force", values=values)),
        # instancenormalization_q4 -> [add_q4] -> [relu_q4] as one step: the tail goes into the norm's write pass
        "fuse_instnorm_q4": q4 and (lambda b, f: fuse_instnorm_q4(b, f, shapes)),
        # linear upsample_q4 / resize_q4 -> add_q4 as one step: the add goes into the upsample's write pass
        "fuse_linear_add": q4 and (lambda b, f: fuse_linear_add(b, f, shapes)),
        # dilated 3x3 convs folded by pixel phase onto the Winograd kernels, where `worth` agrees
        "fold_dilated": q4 and worth is not None and (lambda b, f: fold_dilated(b, f, shapes, worth)),
    }
    body, flow, counts = [list(b) for b in layers], [list(f) for f in flow], {}
    for name in FRONT[:FRONT.index(stop) + 1 if stop else None]:
        if run[name]:
            body, flow, counts[name] = run[name](body, flow)
    return body, flow, counts


def lower(body, flow, inits, shapes, kshape=None, pick=lambda cands, kind, srcs, para: cands[0], prepare=None, stem_pool=None,
          pair=True, wino_chain="1", fits=lambda key: True, small=lambda key: True):
    """The back half of a compile: every eligible conv gets a w_layout and the key of its prepared filter (conv_layouts.choose),
    then the stem-pool and upsample/concat peepholes, pair_sibling_convs, chain_winograd and fuse_conv1x1_wino_in.
    -> (body, flow, {pass that ran: the third value it returned}).  The answers of the caller:
      kshape(key)                        the OIHW shape of a filter key, None for what no kernel takes as a filter
                                         (host: the shape of the init the key was made from);
      pick(cands, kind, srcs, para)      the w_layout of a conv several apply to (host: the first; Net times them);
      prepare(w_layout, init key, para)  -> the key of the init's filter prepared for that layout (host: key + suffix; Net makes
                                         the copy);
      stem_pool(x shape, filter shape, para) -> None, or (STEM_POOL or STEM_POOL_NCHW, extra parameters such as strip_rows) where
                                         the stem + max-pool kernel takes the conv (host, and PLANER_HIP_STEM_POOL=0: None);
      pair                               sibling convs in one launch (PLANER_HIP_PAIR);
      wino_chain                         "1" staged Winograd convs chained, "stages" explicit stages only, "0" one call per conv
                                         (PLANER_HIP_WINO_CHAIN);
      fits(key)                          whether the chained transform kernel takes that activation (host: yes);
      small(key)                         whether a 1x1 conv on that activation is small enough to run inside the next conv's input
                                         transform (host: yes; None, PLANER_HIP_CONV1X1_WINO=0: no such step)."""
    inits = set(inits)
    kshape = kshape or (lambda key: shapes.get(key.split("@")[0]) if key.split("@")[0] in inits else None)
    prepare = prepare or (lambda lay, key, para: key + suffix(lay, para))
    view = Steps(body, flow)
    out_body = {b[0]: list(b) for b in body}
    out_flow = []
    for srcs, name, kind, para, dst in view.each():
        ks = kshape(srcs[1]) if len(srcs) >= 2 and srcs[1] in inits else None
        if ks is not None:
            # (an NCHW conv looks its input up by key: one on a converted copy, key@nchw, is not timed)
            xs = shapes.get(srcs[0].split("@")[0] if kind == "conv_q4" else srcs[0])
            got = choose(kind, ks, para, xs, para.get("rowpack"), lambda cands: pick(cands, kind, srcs, para))
            if got is not None:
                srcs[1] = prepare(got[0], srcs[1], para)
                new_kind = kind if kind in ("conv_q4", "convt_q4") else "convt_fused" if kind in CONVT_KINDS else "conv_fused"
                out_body[name] = [name, new_kind, dict(para, w_layout=got[0])]
        out_flow.append([srcs, [name], dst])
    # the row-packed stem conv whose only reader is maxpool(3x3 / s2 / p1): one kernel that writes the pooled tensor only
    # (csrc/conv_stem_pool_kernel.h)
    if stem_pool is not None:
        out_flow = fuse_stem_pool(out_body, out_flow, shapes, kshape, stem_pool, prepare)
    out_flow = fuse_upsample_concat(out_body, out_flow)
    used = {n for _, names, _ in out_flow for n in names}
    body, flow, counts = [out_body[b[0]] for b in body if b[0] in used], out_flow, {}
    # two direct convs on one tensor (a resolution-changing ResNet block) -> one launch
    if pair:
        body, flow, counts["pair_sibling_convs"] = pair_sibling_convs(body, flow, kshape)
    # F(4x4,3x3) convs as explicit stages, consecutive ones sharing a transform kernel
    if wino_chain != "0":
        body, flow, counts["chain_winograd"] = chain_winograd(body, flow, fits, chain=wino_chain != "stages")
        # a 1x1 conv whose only reader is such a conv's input transform writes V itself (detection nets at small maps: one
        # launch less per 3x3 conv)
        if small is not None:
            body, flow, counts["fuse_conv1x1_wino_in"] = fuse_conv1x1_wino_in(body, flow, kshape, small)
    return body, flow, counts

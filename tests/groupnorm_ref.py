"""Shared pieces of the group-norm tests (tests/test_plan_groupnorm.py on the host, tests/test_gpu_groupnorm.py on the GPU): the
five steps an exporter writes -- reshape (N, G, -1), instancenormalization, reshape back, mul gamma, add beta -- as conv -> norm ->
conv graphs, the compiler's front half up to fuse_linear_add, the oracle stand-in, and the
float64 reference with its per-element bound.

The bound is tests/ref64_ops.instancenorm_bound on the rows (N G, cpg HW) -- a group is contiguous in NCHW -- carried through the
two roundings behind the instance norm:
    y1 = IN(x)            |err| <= bound_IN
    y2 = fl(y1 gamma)     |err| <= |gamma| bound_IN + U |gamma IN64|
    y3 = fl(y2 + beta)    |err| <= ... + U |y64|,  y64 = gamma IN64 + beta
    y4 = fl(y3 + res)     |err| <= ... + U |y64 + res|
relu is exact and 1-Lipschitz.  A term is there only where its operation is.  No constant of its own."""
import numpy as np

from oracle import planer_np as onp
from tests import plan_audit as PA
from tests import ref64_ops as R
from tests.linear_q4_ref import Small
from tests.plan_audit import cpu_front, kinds_of, steps_of      # noqa: F401

F32 = np.float32


# ---- graphs ---------------------------------------------------------------------------------------------------------------------
def five_steps(s, y, shape, groups, tag="gn", mid="3d", via_const=False, affine="both", swap_mul=False, swap_add=False, lead=False,
               merge=None, gamma_shape=None, seed=5):
    """reshape -> instancenormalization -> reshape -> [mul] -> [add] on tensor `y` of 4-D `shape` (batch axis written as 0) into a
    tests.linear_q4_ref.Small.  mid: "3d" (0, G, -1) or "4d" (0, G, cpg, -1); via_const: the shape operands from `const` steps;
    affine: "both", "mul" or "none"; swap_*: the constant as the FIRST operand; lead: constants shaped (1, C, 1, 1), else (C, 1, 1);
    merge: the second reshape's target where it is not the input's shape."""
    _, c, h, w = shape
    rng = np.random.default_rng(seed)
    split = [0, groups, -1] if mid == "3d" else [0, groups, c // groups, -1]
    merge = [0, c, h, w] if merge is None else list(merge)
    if via_const:
        s.g.op("const", [], tag + "_s3", name=tag + "_shape3", value=split, dtype="int64")
        s.g.op("const", [], tag + "_s4", name=tag + "_shape4", value=merge, dtype="int64")
    else:
        s.g.init(tag + "_s3", np.array(split, np.int64))
        s.g.init(tag + "_s4", np.array(merge, np.int64))
    s.g.init(tag + "_ones", rng.uniform(0.5, 1.5, groups).astype(F32))       # honoured whatever they hold
    s.g.init(tag + "_zeros", (rng.standard_normal(groups) * 0.1).astype(F32))
    cshape = gamma_shape or ((1, c, 1, 1) if lead else (c, 1, 1))
    y = s.g.op("reshape", [y, tag + "_s3"], tag + "_g", name=tag + "_split")
    y = s.g.op("instancenormalization", [y, tag + "_ones", tag + "_zeros"], tag + "_n", name=tag + "_in", epsilon=1e-5)
    y = s.g.op("reshape", [y, tag + "_s4"], tag + "_m", name=tag + "_merge")
    if affine in ("both", "mul"):
        s.g.init(tag + "_gamma", rng.uniform(0.5, 1.5, cshape).astype(F32))
        y = s.g.op("mul", [tag + "_gamma", y] if swap_mul else [y, tag + "_gamma"], tag + "_k", name=tag + "_mul")
    if affine == "both":
        s.g.init(tag + "_beta", (rng.standard_normal((1, c, 1, 1) if lead else (c, 1, 1)) * 0.1).astype(F32))
        y = s.g.op("add", [tag + "_beta", y] if swap_add else [y, tag + "_beta"], tag + "_b", name=tag + "_shift")
    return y


def sandwich(c=8, groups=2, hw=(6, 7), **kw):
    """x (N, 4, h, w) -> conv (c channels) -> the five steps -> conv -> return.  -> (graph, blob)."""
    s = Small()
    y = s.conv("x", "a", cin=4, cout=c)
    y = five_steps(s, y, (1, c) + tuple(hw), groups, **kw)
    return s.finish(s.conv(y, "z", cin=c))


def make_x(n=2, hw=(6, 7), seed=3):
    return np.random.default_rng(seed).standard_normal((n, 4) + tuple(hw)).astype(F32)


def compile_plan(g, b, x, force=True):
    """plan.compile_front up to fuse_linear_add.  -> (body, flow, number of norms fused, shapes)."""
    body, flow, counts, shapes = cpu_front(g, b, x, force, stop="fuse_linear_add")
    return body, flow, counts.get("fuse_groupnorm", 0), shapes


def groupnorm_np(x, s, bias, gamma=None, beta=None, res=None, groups=1, epsilon=1e-5, act=0, mid="3d"):
    """`groupnorm` / `groupnorm_q4` on the oracle: the five oracle operators the step stands for, then the fused tail.  `mid` is
    not the step's: numpy's mean over one axis of n values and over two axes of the same n values add in another order, so the
    stand-in for a graph written with the 4-D middle shape splits as that graph does (on the device both are one kernel on rows)."""
    ops = onp.OPS
    y = ops["reshape"](x, np.array([0, groups, -1] if mid == "3d" else [0, groups, x.shape[1] // groups, -1], np.int64))
    y = ops["instancenormalization"](y, s, bias, epsilon=epsilon)
    y = ops["reshape"](y, np.array(x.shape, np.int64))
    if gamma is not None:
        y = ops["mul"](y, gamma)
    if beta is not None:
        y = ops["add"](y, beta)
    if res is not None:
        y = ops["add"](y, res)
    return ops["relu"](y) if act else y


def run_on_oracle(g, b, x, body, flow, mid="3d"):
    """The program (body, flow) on the numpy oracle: plan-internal kinds as their NCHW operators, groupnorm[_q4] as the five steps."""
    from functools import partial
    return PA.run_on_oracle(g, b, x, body, flow, groupnorm=partial(groupnorm_np, mid=mid), groupnorm_q4=partial(groupnorm_np, mid=mid))


# ---- float64 reference, bound, float32 emulation -------------------------------------------------------------------------------
def _rows(x, gs, gb, groups):
    n, c = x.shape[:2]
    return x.reshape(n * groups, -1), np.tile(np.asarray(gs).reshape(-1), n), np.tile(np.asarray(gb).reshape(-1), n)


def _chan(v):
    return None if v is None else np.asarray(v, np.float64).reshape(1, -1, 1, 1)


def reference(x, gs, gb, gamma=None, beta=None, res=None, act=0, groups=1, eps=1e-5):
    """-> (float64 reference, per-element bound), both shaped like the NCHW x."""
    rows, sr, br = _rows(x, gs, gb, groups)
    ref = R.instancenorm64(rows, sr, br, eps).reshape(x.shape)
    tol = R.instancenorm_bound(rows, sr, br, eps).reshape(x.shape)
    if gamma is not None:
        ref = ref * _chan(gamma)
        tol = tol * np.abs(_chan(gamma)) + R.U * np.abs(ref)
    if beta is not None:
        ref = ref + _chan(beta)
        tol = tol + R.U * np.abs(ref)
    if res is not None:
        ref = ref + np.asarray(res, np.float64)
        tol = tol + R.U * np.abs(ref)
    if act:
        ref = np.maximum(ref, 0.0)
    return ref, tol


def emulate(x, gs, gb, gamma=None, beta=None, res=None, act=0, groups=1, eps=1e-5, two_pass=True):
    """The kernel's order of operations in float32 numpy: emulate_instancenorm on the group rows, then each further operation
    rounded on its own.  two_pass=False: the E[x^2] - mean^2 mutation."""
    rows, sr, br = _rows(np.asarray(x, F32), gs, gb, groups)
    y = R.emulate_instancenorm(rows, sr, br, eps, two_pass=two_pass).reshape(x.shape)
    if gamma is not None:
        y = (y * np.asarray(gamma, F32).reshape(1, -1, 1, 1)).astype(F32)
    if beta is not None:
        y = (y + np.asarray(beta, F32).reshape(1, -1, 1, 1)).astype(F32)
    if res is not None:
        y = (y + np.asarray(res, F32)).astype(F32)
    return np.maximum(y, F32(0)) if act else y


def operands(rng, xs, groups, dc=0.0, res=False, gamma=True, beta=True):
    """Skewed operands as the instance-norm tests draw them: every (image, channel) plane scaled by 2^U(-10, 6), plus a DC offset."""
    n, c = xs[:2]
    x = (rng.standard_normal(xs) * 2.0 ** rng.uniform(-10, 6, (n, c, 1, 1)) + dc).astype(F32)
    gs = (rng.choice([-1, 1], groups) * 2.0 ** rng.uniform(-3, 3, groups)).astype(F32)
    gb = rng.standard_normal(groups).astype(F32)
    ga = (rng.choice([-1, 1], c) * 2.0 ** rng.uniform(-4, 4, c)).astype(F32) if gamma else None
    be = rng.standard_normal(c).astype(F32) if beta else None
    r = rng.standard_normal(xs).astype(F32) if res else None
    return x, gs, gb, ga, be, r

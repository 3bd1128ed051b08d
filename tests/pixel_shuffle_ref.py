"""Shared pieces of the pixel shuffle / unshuffle tests (tests/test_plan_pixel_shuffle.py on the host,
tests/test_gpu_pixel_shuffle.py on the GPU): numpy's own reshape / transpose / reshape as the reference, the four forms as
conv -> trio -> conv graphs, and the compiler's front half up to fuse_linear_add."""
import numpy as np

from tests import plan_audit as PA
from tests.linear_q4_ref import Small
from tests.plan_audit import cpu_front, kinds_of, steps_of      # noqa: F401

# (order, inverse) -> the 6-D permutation, as the issue's table has them
AXES = {("crd", False): [0, 1, 4, 2, 5, 3], ("dcr", False): [0, 3, 4, 1, 5, 2],
        ("crd", True): [0, 1, 3, 5, 2, 4], ("dcr", True): [0, 3, 5, 1, 2, 4]}
FORMS = [("crd", False), ("dcr", False), ("crd", True), ("dcr", True)]
FORM_IDS = ["shuffle-crd", "shuffle-dcr", "unshuffle-crd", "unshuffle-dcr"]


def mid_shape(shape, r, order, inverse):
    """The 6-D shape of the trio on the 4-D `shape`."""
    n, c, h, w = shape
    if inverse:
        return (n, c, h // r, r, w // r, r)
    cn = c // (r * r)
    return (n, cn, r, r, h, w) if order == "crd" else (n, r, r, cn, h, w)


def out_shape(shape, r, inverse):
    n, c, h, w = shape
    return (n, c * r * r, h // r, w // r) if inverse else (n, c // (r * r), h * r, w * r)


def shuffle_np(x, r, order="crd", inverse=False, **_):
    """numpy's own reshape -> transpose -> reshape on the NCHW tensor."""
    return np.ascontiguousarray(x.reshape(mid_shape(x.shape, r, order, inverse)).transpose(AXES[(order, bool(inverse))])
                                .reshape(out_shape(x.shape, r, inverse)))


def trio(s, y, shape, r, order, inverse, tag="ps", axis=None, mid=None, via_const=False):
    """reshape -> transpose -> reshape on tensor `y` of 4-D `shape` (batch axis written as 0), into a tests.linear_q4_ref.Small."""
    mid = [0] + list(mid_shape(shape, r, order, inverse))[1:] if mid is None else list(mid)
    out = [0] + list(out_shape(shape, r, inverse))[1:]
    if via_const:               # the shape operands as results of `const` steps, not inits
        s.g.op("const", [], tag + "_s6", name=tag + "_shape6", value=mid, dtype="int64")
        s.g.op("const", [], tag + "_s4", name=tag + "_shape4", value=out, dtype="int64")
    else:
        s.g.init(tag + "_s6", np.array(mid, np.int64))
        s.g.init(tag + "_s4", np.array(out, np.int64))
    y = s.g.op("reshape", [y, tag + "_s6"], tag + "_6", name=tag + "_split")
    y = s.g.op("transpose", y, tag + "_t", name=tag + "_perm", axis=list(AXES[(order, inverse)] if axis is None else axis))
    return s.g.op("reshape", [y, tag + "_s4"], tag, name=tag + "_merge")


def sandwich(order, inverse, r=2, narrow=4, hw=(6, 8), via_const=False, tail=True, n_in=4, **kw):
    """x (N, 4, h, w) -> conv -> trio -> [conv] -> return; `narrow`: the channel count of the narrow side.  -> (graph, blob)."""
    s = Small()
    cmid = narrow if inverse else narrow * r * r
    y = s.conv("x", "a", cin=n_in, cout=cmid)
    y = trio(s, y, (1, cmid) + tuple(hw), r, order, inverse, via_const=via_const, **kw)
    if tail:
        y = s.conv(y, "z", cin=narrow * r * r if inverse else narrow)
    return s.finish(y)


def make_x(n=2, hw=(6, 8), seed=3):
    return np.random.default_rng(seed).standard_normal((n, 4) + tuple(hw)).astype(np.float32)


def compile_plan(g, b, x, force=True):
    """plan.compile_front up to fuse_linear_add.  -> (body, flow, number of trios fused, shapes)."""
    body, flow, counts, shapes = cpu_front(g, b, x, force, stop="fuse_linear_add")
    return body, flow, counts.get("fuse_pixel_shuffle", 0), shapes


def run_on_oracle(g, b, x, body, flow):
    """The program (body, flow) on the numpy oracle: plan-internal kinds as their NCHW operators, pixelshuffle[_q4] as numpy's trio."""
    return PA.run_on_oracle(g, b, x, body, flow, pixelshuffle=shuffle_np, pixelshuffle_q4=shuffle_np)

"""Shared pieces of the tests of linear upsample / resize in channel-quad (Q4) plans (tests/test_plan_linear_q4.py on the host,
tests/test_gpu_linear_q4.py on the GPU): the compiler's front half up to fuse_linear_add, small graphs, the bit-pattern
comparison, and a per-step check against the NCHW kernels (tests/plan_audit.py checks the same steps against float64).
"""
import numpy as np

from oracle import planer_np as onp
from planer_amd.irgen.builder import GraphBuilder
from tests import plan_audit as PA
from tests.plan_audit import cpu_front, kinds_of, nchw, steps_of      # noqa: F401

LINEAR_KINDS = ("upsample_q4", "resize_q4", "upsample_add_q4", "resize_add_q4")
CONV = dict(group=1, strides=[1, 1], dilations=[1, 1], pads=[1, 1, 1, 1])


def compile_plan(g, b, x, force=True):
    """plan.compile_front up to fuse_linear_add.  -> (body, flow, number of adds fuse_linear_add absorbed, shapes)."""
    body, flow, counts, shapes = cpu_front(g, b, x, force, stop="fuse_linear_add")
    return body, flow, counts["fuse_linear_add"], shapes


def run_on_oracle(g, b, x, body, flow):
    """The program (body, flow) on the numpy oracle, plan-internal kinds replaced by their NCHW operators."""
    return PA.run_on_oracle(g, b, x, body, flow, resize_q4=onp.OPS["resize"],
                            upsample_add_q4=lambda x, k, res, **kw: onp.OPS["upsample"](x, k, **kw) + res,
                            resize_add_q4=lambda x, roi, k, size, res, **kw: onp.OPS["resize"](x, roi, k, size, **kw) + res)


class Small:
    """x (N, 4, H, W) -> conv `a` (8 channels) -> ... -> return, filters seeded; `conv(src, tag)` adds a 3x3 / pad 1 conv 8 -> 8."""

    def __init__(self, seed=11):
        self.rng = np.random.default_rng(seed)
        self.g = GraphBuilder(["x"])
        self.g.init("scales2", np.array([1, 1, 2, 2], np.float32))
        self.g.init("roi", np.zeros(0, np.float32))
        self.g.init("none", np.zeros(0, np.float32))

    def conv(self, src, tag, cin=8, cout=8):
        self.g.init(tag + "_w", (self.rng.standard_normal((cout, cin, 3, 3)) * 0.2).astype(np.float32))
        return self.g.op("conv", [src, tag + "_w"], tag, name=tag + "_conv", **CONV)

    def finish(self, y):
        return self.g.finish([y])


def sandwich(step):
    """conv -> `step(small, conv output)` -> conv -> return."""
    s = Small()
    y = s.conv("x", "a", cin=4)
    y = step(s, y)
    y = s.conv(y, "z")
    return s.finish(y)


def make_x(n=1, h=6, w=7, seed=3):
    return np.random.default_rng(seed).standard_normal((n, 4, h, w)).astype(np.float32)


# ---- bit patterns ----------------------------------------------------------------------------------------------------------
def assert_same_bits(got, want, what=""):
    """Equal as uint32 bit patterns; NaNs are compared as positions (a NaN's payload is not part of the contract)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN positions differ" % what
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    bad = (gb != wb) & ~gn
    assert not bad.any(), "%s: %d of %d elements differ in bits, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def padding_lanes(raw, c):
    """The padding lanes of a raw Q4 buffer (n, cq, h, w, 4) that holds c channels, as uint32."""
    n, cq, h, w, _ = raw.shape
    lanes = raw.transpose(0, 1, 4, 2, 3).reshape(n, cq * 4, h, w)[:, c:]
    return np.ascontiguousarray(lanes).view(np.uint32)


# ---- per-step check on the GPU --------------------------------------------------------------------------------------------
def check_linear_steps(pa, trace, inits):
    """Every upsample_q4 / resize_q4 / *_add_q4 step of a plan_audit.capture trace: its output equals, bit for bit, the NCHW
    layer (and layer.Add for a fused add) applied on the device to the step's own captured inputs.  `inits`: key -> host array
    (plan_audit.host_inits).  -> number of steps checked."""
    from planer_amd import layer
    n = 0
    for st in trace:
        if st.kind not in LINEAR_KINDS:
            continue
        x = pa.hip.asarray(nchw(st.ins[0]))
        const = lambda key: None if key == "None" else inits[key]           # noqa: E731
        fused = st.kind.endswith("_add_q4")
        if st.kind.startswith("upsample"):
            want = layer.UpSample(x, const(st.src[1]), **st.para)
        else:
            srcs = st.src[:-1] if fused else st.src
            want = layer.Resize(x, *[const(k) for k in srcs[1:]], **st.para)
        if fused:
            want = layer.Add(want, pa.hip.asarray(nchw(st.ins[-1])))
        assert_same_bits(nchw(st.outs[0]), want.get(), "%s (%s)" % (st.name, st.kind))
        n += 1
    return n

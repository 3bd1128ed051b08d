"""The plan audit (tests/plan_audit.py) on a real MI355X: every step of the programs the captured plans run, checked in
float64 against the inputs it really read, for the generator nets, the random nets and the real-scale random nets; and the
audited eager run must be bit-identical to the captured graph (latency plan "1x1", throughput plan "pipe2").  Run with -s
for the worst err / tol per net and family and the w_layout census."""
import numpy as np
import pytest

from planer_amd.irgen import customnet, mobilenetv2, resnet18, unet, yolov3
from tests import plan_audit as PA
from tests.random_nets import random_net, random_net_real
from tests.test_conv_layouts import SWITCHES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for k in SWITCHES + ("PLANER_HIP_CONV_ALGO", "PLANER_HIP_STREAMS", "PLANER_HIP_Q4"):
        monkeypatch.delenv(k, raising=False)


def _same(got, want, what):
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i)
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        assert same.all(), "%s output %d: %d elements differ from the audited eager run, first at %s" % (
            what, i, int((~same).sum()), tuple(int(v) for v in np.argwhere(~same)[0]))


def run_audit(pa, g, b, x, label, mode="latency", q4=None, graph=True):
    net = pa.from_graph(g, b)
    if q4 is not None:
        net.use_q4 = q4
    trace, eager = PA.capture(net, [pa.asarray(x)], mode)
    worst, census = PA.audit(trace, PA.host_inits(net))
    if graph:
        net.streams = "1x1" if mode == "latency" else "pipe2"
        got = net(x.copy()) if mode == "latency" else net.submit(x.copy()).get()
        _same(got, eager, "%s: captured %s plan" % (label, net.streams))
    print("%-32s %-10s %s  census %s" % (label, mode, " ".join("%s %.3f" % kv for kv in sorted(worst.items())),
                                          dict(sorted(census.items()))))
    return worst, census


# (module, batch, size, build kwargs, picking mode, w_layouts the audit must have reached -- the shipped picks of
#  planer_amd/tuned and the fixed choices test_conv_layouts.py pins: direct 2, row-packed stem 6, stem + pool 10 / 12,
#  wf4 9, F(4x4) staged 7, wino43 11, F(2x2) 4, depthwise 13, ConvTranspose 14)
NETS = {
    "resnet18 b32@224 latency": (resnet18, 32, 224, {}, "latency", {2, 7, 9, 11}),
    "resnet18 b32@224 throughput": (resnet18, 32, 224, {}, "throughput", {2, 7, 9, 11}),
    "resnet18 b2@224": (resnet18, 2, 224, {}, "latency", {2}),
    "yolov3 b1@416": (yolov3, 1, 416, {}, "latency", {2, 4, 6, 7}),
    "yolov3 b1@160": (yolov3, 1, 160, {}, "latency", {2, 6}),
    "mobilenetv2 b8@224": (mobilenetv2, 8, 224, {}, "latency", {2, 6, 13}),
    "unet-k2 b2@256": (unet, 2, 256, {"up": "k2"}, "latency", {2, 6, 14}),
    "unet-k3 b2@256": (unet, 2, 256, {"up": "k3"}, "latency", {2, 6, 14}),
    "customnet b1@64": (customnet, 1, 64, {}, "latency", set()),
}


@pytest.mark.parametrize("name", list(NETS))
def test_generator_nets(pa, name):
    mod, batch, size, kw, mode, want = NETS[name]
    g, b = mod.build(**kw)
    x = mod.make_input(batch, size=size) if mod is not customnet else mod.make_input(batch)
    _, census = run_audit(pa, g, b, x, name, mode)
    assert want <= set(census), (name, dict(census))
    if name.startswith("resnet18 b32"):
        assert {10, 12} & set(census), "the stem + max-pool kernel was not audited"


@pytest.mark.parametrize("seed", range(60))
def test_random_nets(pa, seed):
    g, b, xs = random_net(40000 + seed)
    run_audit(pa, g, b, xs[0], "random %d" % seed)
    run_audit(pa, g, b, xs[1], "random %d q4 forced" % seed, q4="force")


# staged F(2x2) and F(4x4), 1-D F(4,3), wf4, wino43: forced one at a time where every 3x3 / s1 conv of the net can take it
FORCED = (4, 7, 8, 9, 11)


@pytest.mark.parametrize("seed", range(24))
def test_real_scale_random_nets(pa, seed, monkeypatch):
    g, b, xs = random_net_real(seed)
    run_audit(pa, g, b, xs[0], "real %d" % seed)
    if seed % 3:
        return
    for algo in FORCED:
        monkeypatch.setenv("PLANER_HIP_CONV_ALGO", str(algo))
        try:
            run_audit(pa, g, b, xs[0], "real %d algo %d" % (seed, algo))
        except ValueError as e:
            if "does not apply" not in str(e):
                raise

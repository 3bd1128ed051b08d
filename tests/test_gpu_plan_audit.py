"""The plan audit (tests/plan_audit.py) on a real MI355X: every step of the programs the captured plans run, checked in
float64 against the inputs it really read, for the generator nets, the random nets and the real-scale random nets; and the
audited eager run must be bit-identical to the captured graph (latency plan "1x1", throughput plan "pipe2").  Run with -s
for the worst err / tol per net and family and the w_layout census."""
import os
import subprocess
import sys

import numpy as np
import pytest

from planer_amd.irgen import customnet, drn, edsr, fpn, mobilenetv2, resnet18, resnet_gn, stylenet, unet, yolov3
from tests import plan_audit as PA
from tests.audit_nets import SWITCHED_OFF, TINY_EDSR, TINY_GN
from tests.random_nets import random_net, random_net_q4ops, random_net_real
from tests.test_conv_layouts import SWITCHES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for k in SWITCHES + ("PLANER_HIP_CONV_ALGO", "PLANER_HIP_STREAMS", "PLANER_HIP_Q4") + tuple(SWITCHED_OFF):
        monkeypatch.delenv(k, raising=False)


def _same(got, want, what):
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i)
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        assert same.all(), "%s output %d: %d elements differ from the audited eager run, first at %s" % (
            what, i, int((~same).sum()), tuple(int(v) for v in np.argwhere(~same)[0]))


def run_audit(pa, g, b, x, label, mode="latency", q4=None, graph=True, fold=None):
    net = pa.from_graph(g, b)
    if q4 is not None:
        net.use_q4 = q4
    if fold is not None:
        net.fold_dilated = fold
    trace, eager = PA.capture(net, [pa.asarray(x)], mode)
    worst, census = PA.audit(trace, PA.host_inits(net))
    PA.assert_every_step_audited(trace, census)          # every step of the flow went through an arm of the audit
    if graph:
        net.streams = "1x1" if mode == "latency" else "pipe2"
        got = net(x.copy()) if mode == "latency" else net.submit(x.copy()).get()
        _same(got, eager, "%s: captured %s plan" % (label, net.streams))
    folds = "  refolds %d, folded steps %d (1x1 convs %d), junk keys %d" % (
        census.kinds["refold_q4"], sum(census.folded.values()), census.joined_1x1, census.junk) if census.kinds["refold_q4"] else ""
    if census.nearest:
        folds += "  nearest resizes %s" % dict(census.nearest)
    print("%-32s %-10s %s  census %s%s" % (label, mode, " ".join("%s %.3f" % kv for kv in sorted(worst.items())),
                                            dict(sorted(census.items())), folds))
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
    # the nets of the kinds behind the convs; a seventh entry: run_audit's q4 / fold, `kinds` the audit must have gone through at
    # the least, `plans` launch-plan strings (kind, part of the plan) it must have met.  One throughput ("pipe2") row per family.
    "stylenet b2@32": (stylenet, 2, 32, {}, "latency", set(), dict(
        kinds={"instancenormalization_q4": 15, "pad_q4": 15}, plans=[("instancenormalization_q4", "one-wg")])),
    "stylenet b2@32 throughput": (stylenet, 2, 32, {}, "throughput", set(), dict(kinds={"instancenormalization_q4": 15, "pad_q4": 15})),
    "stylenet b1@96": (stylenet, 1, 96, {}, "latency", set(), dict(
        kinds={"instancenormalization_q4": 15, "pad_q4": 15}, plans=[("instancenormalization_q4", "chunks=")])),
    "drn b2@64 folded": (drn, 2, 64, {}, "latency", set(), dict(fold="force", kinds={"refold_q4": 5}, folded=8, joined_1x1=2, junk=0)),
    "drn b2@64 folded throughput": (drn, 2, 64, {}, "throughput", set(), dict(fold="force", kinds={"refold_q4": 5})),
    "drn b1@40 folded": (drn, 1, 40, {}, "latency", set(), dict(fold="force", kinds={"refold_q4": 16}, junk=7)),
    "fpn-upsample b2@64": (fpn, 2, 64, {"via": "upsample"}, "latency", set(), dict(kinds={"upsample_q4": 7, "upsample_add_q4": 2})),
    "fpn-resize b2@64": (fpn, 2, 64, {"via": "resize"}, "latency", set(), dict(kinds={"resize_q4": 7, "resize_add_q4": 2})),
    "fpn-upsample b2@64 throughput": (fpn, 2, 64, {"via": "upsample"}, "throughput", set(), dict(kinds={"upsample_add_q4": 2})),
    "edsr-x2 tiny": (edsr, 2, TINY_EDSR["size"], dict(TINY_EDSR, scale=2), "latency", set(), dict(q4="force", kinds={"pixelshuffle_q4": 1})),
    "edsr-x4 tiny": (edsr, 2, TINY_EDSR["size"], dict(TINY_EDSR, scale=4), "latency", set(), dict(q4="force", kinds={"pixelshuffle_q4": 2})),
    "edsr-unshuffle-in tiny": (edsr, 2, TINY_EDSR["size"], dict(TINY_EDSR, scale=2, unshuffle_in=True), "latency", set(),
                               dict(q4="force", kinds={"pixelshuffle_q4": 1})),
    "edsr-x2 tiny throughput": (edsr, 2, TINY_EDSR["size"], dict(TINY_EDSR, scale=2), "throughput", set(),
                                dict(q4="force", kinds={"pixelshuffle_q4": 1})),
    "resnet_gn tiny": (resnet_gn, 2, TINY_GN["size"], TINY_GN, "latency", set(), dict(q4="force", kinds={"groupnorm_q4": 20})),
    "resnet_gn tiny throughput": (resnet_gn, 2, TINY_GN["size"], TINY_GN, "throughput", set(), dict(q4="force", kinds={"groupnorm_q4": 20})),
}


@pytest.mark.parametrize("name", list(NETS))
def test_generator_nets(pa, name):
    mod, batch, size, kw, mode, want = NETS[name][:6]
    extra = dict(NETS[name][6]) if len(NETS[name]) > 6 else {}
    g, b = mod.build(**kw)
    x = mod.make_input(batch, size=size) if mod is not customnet else mod.make_input(batch)
    _, census = run_audit(pa, g, b, x, name, mode, q4=extra.get("q4"), fold=extra.get("fold"))
    assert want <= set(census), (name, dict(census))
    if name.startswith("resnet18 b32"):
        assert {10, 12} & set(census), "the stem + max-pool kernel was not audited"
    for kind, n in extra.get("kinds", {}).items():
        assert census.kinds[kind] >= n, (name, kind, dict(census.kinds))
    for kind, part in extra.get("plans", ()):
        assert any(k == kind and part in plan for k, plan in census.plans), (name, kind, part, census.plans)
    assert sum(census.folded.values()) >= extra.get("folded", 0), (name, dict(census.folded))
    assert census.joined_1x1 >= extra.get("joined_1x1", 0), (name, census.joined_1x1)      # 1x1 convs that joined a fold
    if "junk" in extra:
        assert census.junk == extra["junk"], (name, census.junk)


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
    run_audit(pa, g, b, xs[0], "real %d fold=force" % seed, fold="force")      # its dilated convs folded by pixel phase
    for algo in FORCED:
        monkeypatch.setenv("PLANER_HIP_CONV_ALGO", str(algo))
        try:
            run_audit(pa, g, b, xs[0], "real %d algo %d" % (seed, algo))
        except ValueError as e:
            if "does not apply" not in str(e):
                raise


@pytest.mark.parametrize("seed", range(30))
def test_q4ops_random_nets(pa, seed):
    """Norms, pads, shuffles, linear steps and dilated convs at small odd sizes: as the plan compiler would run them, and with
    channel-quad activations and the pixel-phase fold forced (what the cost estimates decline on maps this small)."""
    g, b, xs = random_net_q4ops(seed)
    run_audit(pa, g, b, xs[0], "q4ops %d" % seed)
    run_audit(pa, g, b, xs[0], "q4ops %d q4 and fold forced" % seed, q4="force", fold="force")


CHILD = """
import sys
import planer_amd
from tests import plan_audit as PA
from tests.audit_nets import SWITCHED_OFF, small_net
name, has, has_not = SWITCHED_OFF[sys.argv[1]]
g, b, x = small_net(name)
net = planer_amd.from_graph(g, b)
net.use_q4 = "force"
trace, _ = PA.capture(net, [planer_amd.asarray(x)])
worst, census = PA.audit(trace, PA.host_inits(net))
PA.assert_every_step_audited(trace, census)
assert all(census.kinds[k] for k in has) and not any(census.kinds[k] for k in has_not), dict(census.kinds)
print("AUDIT", sys.argv[1], "= 0", name, " ".join("%s %.3f" % kv for kv in sorted(worst.items())), dict(census.kinds))
"""


@pytest.mark.parametrize("switch", sorted(SWITCHED_OFF))
def test_switched_off_programs(switch):
    """With a feature switch at 0 the steps run as the NCHW kinds: the same checks through their NCHW arms.  A fresh process, so
    that whatever reads the switch at import sees it."""
    r = subprocess.run([sys.executable, "-c", CHILD, switch], cwd=ROOT, env=dict(os.environ, **{switch: "0"}), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    print(r.stdout.strip())

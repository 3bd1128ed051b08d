"""The plan audit (tests/plan_audit.py) on the CPU: it passes on the oracle's own float32 run of each compiled program, it
fails on each kind of fault it is there to find, the real-scale random nets reach every plan pass, and those passes keep the
meaning of the flow."""
import collections

import numpy as np
import pytest

from oracle import planer_np as onp
from planer_amd.irgen import customnet, resnet18
from tests import plan_audit as PA
from tests.conftest import assert_close
from tests.random_nets import random_net_real
from tests.test_conv_layouts import SWITCHES

# conv algorithm pickers standing in for the timing: the step's own kind, the last candidate (wf4 / wino43), staged F(4x4)
PICKS = {"first": lambda c: c[0], "last": lambda c: c[-1], "staged": lambda c: 7 if 7 in c else c[-1]}


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _nets():
    out = [("customnet",) + customnet.build() + (customnet.make_input(1),),
           ("resnet18",) + resnet18.build() + (resnet18.make_input(2, size=64),)]
    for s in range(20):
        g, b, xs = random_net_real(s)
        out.append(("real%d" % s, g, b, xs[0]))
    return out


NETS = {n[0]: n[1:] for n in _nets()}


def _run(name, pick="staged", **kw):
    g, b, x = NETS[name]
    body, flow, _ = PA.cpu_program(g, b, x, PICKS[pick])
    trace, outs = PA.cpu_trace(g, b, x, body, flow, **kw)
    return trace, outs, PA.blob_inits(g, b)


@pytest.mark.parametrize("pick", sorted(PICKS))
@pytest.mark.parametrize("name", sorted(NETS))
def test_audit_passes_on_the_oracles_own_run(name, pick):
    """The oracle's float32 conv is an sgemm: a direct-family conv, within every family's bound."""
    trace, _, inits = _run(name, pick)
    worst, census = PA.audit(trace, inits)
    assert census and max(worst.values()) <= 1.0
    PA.assert_every_step_audited(trace, census)


def _conv_steps(trace):
    return [s for s in trace if s.kind == "conv_q4" and s.outs and s.outs[0] is not None]


def _bump(q, n, c, y, x, delta):
    q.data[n, c // 4, y, x, c % 4] += np.float32(delta)


def test_planted_fault_one_element_off_by_twice_its_tol():
    trace, clean, inits = _run("resnet18", "first")
    step = _conv_steps(trace)[len(_conv_steps(trace)) // 2]
    ref, tol = PA.Audit(inits).layer(step, 1, step.para, step.para["w_layout"]).expect()
    c, y, x = np.unravel_index(int(np.argmax(np.abs(ref[0]))), ref[0].shape)

    def fault(s, outs):
        if s.name == step.name:
            _bump(outs[0], 0, c, y, x, 2 * tol[0, c, y, x])
        return outs
    bad, outs, _ = _run("resnet18", "first", fault=fault)
    for o, w in zip(outs, clean):
        assert_close(o, w, 1e-4)                       # the old per-tensor check does not see it
    with pytest.raises(PA.AuditError, match=step.name):
        PA.audit(bad, inits)


def test_planted_fault_dirty_padding_lane():
    name = next(n for n in sorted(NETS) if any(isinstance(o, PA.Q4Host) and o.chan % 4 for s in _run(n, "first")[0]
                                                for o in s.outs))
    trace, _, _ = _run(name, "first")
    step = next(s for s in trace if s.outs and isinstance(s.outs[0], PA.Q4Host) and s.outs[0].chan % 4)

    def fault(s, outs):
        if s.name == step.name:
            outs[0].data[0, -1, 0, 0, 3] = 1e-3
        return outs
    bad, _, inits = _run(name, "first", fault=fault)
    with pytest.raises(PA.AuditError, match="padding lane 3"):
        PA.audit(bad, inits)


def test_planted_fault_residual_from_another_tensor_of_the_same_shape():
    full = {}

    def keep(s, outs):
        for k, v in zip(s.dst, outs):
            full[k] = PA.nchw(v) if isinstance(v, (PA.Q4Host, np.ndarray)) else None
        return outs
    trace, _, inits = _run("resnet18", "first", fault=keep)
    step = next(s for s in _conv_steps(trace) if len(s.src) > 5 and s.src[5] != "None")
    shape = full[step.src[5]].shape
    other = next(k for k, v in full.items() if v is not None and v.shape == shape and k != step.src[5]
                 and not np.array_equal(v, full[step.src[5]]))

    def conv(s, x, K, B=None, scale=None, shift=None, res=None, **kw):
        if s.name == step.name:
            res = full[other]
        return PA._conv_np(x, K, B, scale, shift, res, **kw)
    bad, _, _ = _run("resnet18", "first", conv=conv)
    with pytest.raises(PA.AuditError, match=step.name):
        PA.audit(bad, inits)


def test_planted_fault_inside_an_elided_tensor():
    """A chain step with keep_y False writes no y: an error there shows only in the next conv, through the carried bound."""
    trace, _, inits = _run("resnet18", "staged")
    step = next(s for s in trace if s.kind == "wino4_chain" and not s.para["keep_y"])
    assert all(v is None for v in step.outs)          # nothing of y is observed

    def fault(s, outs):
        if s.name == step.name:
            y = outs[0]
            y[0, 0, 1, 1] += 1e3 * (1 + np.abs(y).max())
        return outs
    bad, _, _ = _run("resnet18", "staged", fault=fault)
    with pytest.raises(PA.AuditError):
        PA.audit(bad, inits)


def test_real_scale_generator_reaches_every_plan_pass():
    seen = collections.Counter()
    for seed in range(24):
        g, b, xs = random_net_real(seed)
        for pick in PICKS.values():
            body, flow, shapes = PA.cpu_program(g, b, xs[0], pick)
            for name, kind, para in body:
                if "w_layout" in para or kind in ("wino4_gemm", "wino43_gemm"):       # (staged convs: their GEMM stage)
                    seen["w_layout %d" % para.get("w_layout", PA.STAGED[kind[:-len("_gemm")]] if "gemm" in kind else 0)] += 1
                if kind.endswith("_chain"):
                    seen["chain keep_y %s" % para["keep_y"]] += 1
                if kind in ("conv_q4_pair", "conv1x1_wino_in"):
                    seen[kind] += 1
            kinds = {e[0]: e[1] for e in body}
            for src, names, dst in flow:                 # a channel-quad conv output with a partial last quad
                s = shapes.get(dst.split("@")[0]) if isinstance(dst, str) else None
                if kinds[names[0]] in ("conv_q4", "convt_q4") and s is not None and len(s) == 4 and s[1] % 4:
                    seen["partial quad"] += 1
    want = ["w_layout %d" % c for c in (2, 6, 7, 9, 11, 13, 14)] + ["chain keep_y True", "chain keep_y False", "conv_q4_pair",
                                                                    "conv1x1_wino_in", "partial quad"]
    assert all(seen[k] >= 3 for k in want), [(k, seen[k]) for k in want if seen[k] < 3]


@pytest.mark.parametrize("pick", sorted(PICKS))
def test_rewrites_preserve_the_flow_on_real_scale_graphs(pick):
    """fuse_flow, assign_layouts, the conv choice, the upsample/concat peephole, pair_sibling_convs, chain_winograd and
    fuse_conv1x1_wino_in, interpreted with numpy stand-ins, give the tensors of the flow as written."""
    for seed in range(24):
        g, b, xs = random_net_real(seed)
        ref = onp.OracleNet()
        ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
        ref.load_weights(b)
        want = ref(xs[0].copy())
        want = want if isinstance(want, tuple) else (want,)
        body, flow, _ = PA.cpu_program(g, b, xs[0], PICKS[pick])
        _, got = PA.cpu_trace(g, b, xs[0], body, flow)
        assert len(got) == len(want)
        for o, w in zip(got, want):
            assert o.shape == w.shape, seed
            assert_close(np.ascontiguousarray(o), np.ascontiguousarray(w), 1e-5, "seed %d" % seed)

"""Dilated 3x3 convs folded by pixel phase onto the Winograd kernels on the GPU.

pl_refold_q4_f32 against tests/fold_ref.py bit for bit (it moves bits: NaN payloads, infinities, -0 and denormals included), with
the input's zero-fill cells poisoned where it has any, and under the pool's hygiene mode; a folded conv on every Winograd layout
that takes the shape against the float64 reference of the DILATED conv within that family's bound (tests/ref64.py, the
yardstick of tests/test_gpu_conv_bounds.py), and exactly on integer operands on the direct layout; the dilated ResNet-18
(planer_amd.irgen.drn) with every eligible conv folded against the oracle through net(x), the pipelined path and a plan file, on
maps the dilations divide (size 64: 8 x 8) and maps they do not (size 40: 5 x 5); and the switch -- off: no refold step, "1":
whatever the timing decides -- from fresh child processes.

Refold counts of DRN: 5 at size 64, 16 at size 40 (tests/test_plan_dilated_fold.py says why not 18)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import planer_np as onp
from tests import ref64 as R
from tests.conftest import ROOT, RTOL, assert_close
from tests.fold_ref import fold_np, folded_shape, tail_mask, to_q4_np, unfold_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
# (unfolded shape, fold of the input, fold of the output).  (2, 64, 96, 96) is 294 912 quads; the launch grid of a 256-CU device
# covers 524 288 per pass, so (2, 64, 160, 160) -- 819 200 quads -- is the case that takes the grid-stride loop round again.
REFOLD = [((2, 8, 8, 8), (1, 1), (2, 2)), ((2, 8, 8, 8), (2, 2), (1, 1)), ((1, 6, 7, 9), (1, 1), (2, 2)), ((1, 4, 3, 3), (1, 1), (4, 4)),
          ((2, 4, 12, 8), (1, 1), (4, 2)), ((1, 8, 12, 12), (2, 2), (4, 4)), ((1, 8, 12, 12), (2, 2), (3, 3)),
          ((2, 64, 96, 96), (1, 1), (2, 2)), ((2, 64, 160, 160), (1, 1), (2, 2)),
          # inputs WITH zero-fill cells (poisoned below): unfold, and fold to fold
          ((1, 6, 7, 9), (2, 2), (1, 1)), ((1, 6, 7, 9), (2, 2), (3, 3)), ((1, 4, 3, 3), (4, 4), (1, 1))]
SPECIAL = np.array([0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF], np.uint32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _case(shape, src, dst):
    """-> (host Q4 input folded by `src`, its fold attribute, expected Q4 output).  Values: normals with special bit patterns
    sprinkled in; the zero-fill cells of the input -- which a conv would have left junk in -- hold NaNs of another payload."""
    rng = np.random.default_rng(sum(shape) * 7 + src[0] * 3 + dst[1])
    x = rng.standard_normal(shape).astype(np.float32)
    at = rng.random(shape) < 0.05
    x.view(np.uint32)[at] = rng.choice(SPECIAL, int(at.sum()))
    xin = fold_np(x, *src)
    xin.view(np.uint32)[tail_mask(shape, *src)] = 0x7FCDEAD0
    want = to_q4_np(fold_np(x, *dst))
    return to_q4_np(xin), (src + shape[2:] if src != (1, 1) else None), want


def _upload(pa, q, chan, fold):
    d = pa.asarray(np.ascontiguousarray(q))
    d.chan, d.fold = chan, fold
    return d


def _ids(cases):
    return ["%s-%dx%d-to-%dx%d" % ("x".join(map(str, s)), a[0], a[1], b[0], b[1]) for s, a, b in cases]


@pytest.mark.parametrize("shape,src,dst", REFOLD, ids=_ids(REFOLD))
def test_refold_kernel_moves_bits_exactly(pa, shape, src, dst):
    from planer_amd import q4
    xin, fold, want = _case(shape, src, dst)
    y = q4.refold_q4(_upload(pa, xin, shape[1], fold), *dst)
    assert q4.logical_shape(y) == folded_shape(shape, *dst) and y.chan == shape[1]
    assert y.fold == (dst + shape[2:] if dst != (1, 1) else None)
    assert np.array_equal(_bits(y.get()), _bits(want))


HYGIENE = [c for c in REFOLD if c[0] != (2, 64, 160, 160)]


@pytest.mark.parametrize("shape,src,dst", HYGIENE, ids=_ids(HYGIENE))
def test_refold_kernel_writes_every_quad_and_nothing_else(pa, shape, src, dst):
    """Fresh blocks filled with 0xFF, then 0x7F, between guards: the result is the expected bits both times -- every quad is
    written, the zero-fill cells included -- and no guard byte changed."""
    from planer_amd import q4
    from tests.test_gpu_hygiene_sweep import POISONS, hygiene
    xin, fold, want = _case(shape, src, dst)
    got = []
    for poison in POISONS:
        with hygiene(poison):
            y = q4.refold_q4(_upload(pa, xin, shape[1], fold), *dst)
            got.append(_bits(y.get()).copy())
            del y
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], _bits(want))


def test_refold_entry_refuses_bad_arguments_before_touching_the_device(pa):
    from planer_amd import _lib, q4
    ctx = pa.hip.context()
    x = q4.to_q4(pa.asarray(np.zeros((1, 4, 4, 4), np.float32)))
    y = pa.hip.empty((4, 1, 2, 2, 4), ctx=ctx)
    for args, what in (((1, 4, 4, 4, 0, 1, 2, 2), "fold"), ((1, 4, 0, 4, 1, 1, 2, 2), "shape"),
                       ((1 << 20, 4, 1 << 10, 1, 1, 1, 1, 1), "2\\^29"), ((1, 4, 1 << 15, 1 << 15, 1, 1, 1 << 14, 1 << 14), "2\\^29")):
        with pytest.raises(Exception, match=what):
            _lib.call("pl_refold_q4_f32", ctx.handle, x.ptr, y.ptr, *args)
    with pytest.raises(ValueError, match="folded by"):
        q4.refold_q4(x, 2, 2, **{"from": [4, 4]})
    with pytest.raises(TypeError):
        q4.refold_q4(pa.asarray(np.zeros((1, 4, 4, 4), np.float32)), 2, 2)


# ---- a folded conv ------------------------------------------------------------------------------------------------------------
def _dev(pa, a):
    return None if a is None else pa.asarray(np.ascontiguousarray(a))


def _folded_conv(pa, x, K, B, sc, sh, r, d, lay, prep, act, alpha=0.0):
    """ConvQ4 at dilation 1 / pad 1 on `x` folded by `d`, the residual folded the same way; the result, unfolded, as NCHW."""
    from planer_amd import q4
    xq = q4.refold_q4(q4.to_q4(_dev(pa, x)), *d)
    rq = q4.refold_q4(q4.to_q4(_dev(pa, r)), *d) if r is not None else None
    yq = q4.ConvQ4(xq, prep(_dev(pa, K)), _dev(pa, B), _dev(pa, sc), _dev(pa, sh), rq, act=act, alpha=alpha, w_layout=lay,
                   group=1, strides=[1, 1], dilations=[1, 1], pads=[1, 1, 1, 1])
    assert yq.fold == tuple(d) + x.shape[2:] and q4.logical_shape(yq) == folded_shape((x.shape[0], K.shape[0]) + x.shape[2:], *d)
    return q4.from_q4(q4.refold_q4(yq, 1, 1)).get()


# (2, 16, 16, 16) dilated by 2: 8 x 8 maps.  (1, 16, 28, 28) dilated by 4: 7 x 7 maps, which the mixed-tile form takes.
WINO = [((2, 16, 16, 16), (2, 2)), ((1, 16, 28, 28), (4, 4))]


@pytest.mark.parametrize("xs,d", WINO, ids=["16x16-d2", "28x28-d4"])
def test_folded_conv_on_the_winograd_layouts_within_the_family_bound(pa, xs, d):
    from planer_amd import q4
    from tests.test_gpu_conv_bounds import ALPHA, FAM, LABEL, PLAN, TAILS, _check, _operands
    conv = dict(group=1, strides=[1, 1], dilations=list(d), pads=[d[0], d[1], d[0], d[1]])
    ks = (16, xs[1], 3, 3)
    ops, act, want = _operands("fold", xs, ks, TAILS[0], **conv)         # bias, scale / shift, residual, relu
    x, K, B, sc, sh, r = ops
    prep = {4: q4.prepare_winograd_q4_weights, 7: q4.prepare_winograd4_q4_weights, 9: q4.prepare_wf4_q4_weights,
            8: q4.prepare_w1d4_q4_weights, 11: q4.prepare_winograd43_q4_weights}
    fxs = folded_shape(xs, *d)
    ran = []
    for lay in (4, 7, 9, 8, 11):
        if not q4.LAYOUTS[lay].eligible(ks, fxs, group=1, strides=[1, 1], dilations=[1, 1], pads=[1, 1, 1, 1]):
            continue
        y = _folded_conv(pa, x, K, B, sc, sh, r, d, lay, prep[lay], act, ALPHA)
        assert pa.hip.context().last_conv_plan().startswith(PLAN[lay]), (lay, pa.hip.context().last_conv_plan())
        _check(pa, y, ops, want, FAM[lay], "%s folded by %s" % (xs, d), LABEL[lay] + " folded", **conv)
        ran.append(lay)
    assert ran == ([4, 7, 9, 8, 11] if fxs[2] == 7 else [4, 7, 9, 8])


@pytest.mark.parametrize("xs,d", WINO + [((1, 8, 7, 9), (2, 2)), ((2, 4, 5, 6), (3, 4))], ids=["16x16-d2", "28x28-d4", "7x9-d2", "5x6-d3x4"])
def test_folded_conv_on_the_direct_layout_is_exact_on_integers(pa, xs, d):
    from planer_amd import q4
    conv = dict(group=1, strides=[1, 1], dilations=list(d), pads=[d[0], d[1], d[0], d[1]])
    ks = (12, xs[1], 3, 3)
    rng = np.random.default_rng(xs[2] * 100 + d[0])
    x, K, B, sc, sh, r = R.int_operands(rng, xs, ks, bias=True, bn=True, res=True, **conv)
    R.assert_exact(x, K, B, sc, sh, r, **conv)
    want = R.ref64(x, K, B, sc, sh, r, act=R.ACT_RELU, **conv)
    y = _folded_conv(pa, x, K, B, sc, sh, r, d, 2, q4.prepare_q4_weights, R.ACT_RELU)
    assert np.array_equal(y.astype(np.float64), want)


# ---- the dilated ResNet-18 --------------------------------------------------------------------------------------------------------
CASES = {64: 2, 40: 1}          # size -> batch
REFOLDS = {64: 5, 40: 16}


def _model(size):
    from planer_amd.irgen import drn
    g, b = drn.build()
    x = drn.make_input(CASES[size], size=size)
    ref = onp.OracleNet()
    ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
    ref.load_weights(b)
    return size, g, b, x, ref(x.copy())


def _forced(pa, model):
    size, g, b, x, _ = model
    net = pa.from_graph(g, b)
    net.fold_dilated = "force"
    return net, net(pa.asarray(x)).get()


@pytest.fixture(scope="module", params=sorted(CASES), ids=["size%d" % s for s in sorted(CASES)])
def drn_model(request):
    """(size, graph, blob, input, the oracle's result), shared by the tests of one size."""
    return _model(request.param)


@pytest.fixture(scope="module")
def drn_net(pa, drn_model):
    """(the net compiled with every eligible conv folded, its result through net(x)), shared by the tests of one size and
    released with them."""
    return _forced(pa, drn_model)


@pytest.fixture(scope="module")
def drn64(pa):
    """The size-64 model and its forced net for the two switch tests."""
    model = _model(64)
    return model, _forced(pa, model)


def test_drn_folded_through_net_pipelined_and_plan_file(pa, drn_model, drn_net, tmp_path):
    from planer_amd.export import export_plan
    from tests.test_gpu_plan_file import _bind, _run_plan
    size, g, b, x, want = drn_model
    net, got = drn_net
    assert got.shape == (CASES[size], 21, size, size)
    assert_close(got, want, RTOL, "drn %d folded" % size)
    assert_close(net.submit(pa.asarray(x, ctx=net.ctx)).get(), want, RTOL, "drn %d folded, submit" % size)
    path = tmp_path / ("drn_%d.plplan" % size)
    blob = export_plan(net, x, path=str(path))
    assert blob.count(b"pl_refold_q4_f32") >= 1
    out, = _run_plan(_bind(), open(path, "rb").read(), [x])
    assert_close(out, want, RTOL, "drn %d folded, plan file" % size)


def test_drn_plan_facts(pa, drn_model, drn_net):
    size, g, b, x, want = drn_model
    net, _ = drn_net
    plan = net.compile(pa.asarray(x))
    folded = [a for a in plan.algos if a.get("fold")]
    heads = [a for a in folded if a["layer"][:4] in ("l30b", "l31a", "l31b", "l40a", "l40b", "l41a", "l41b")]
    assert len(heads) == 7 and net.dilated_folds == 7 and net.refolds == REFOLDS[size], (net.dilated_folds, net.refolds, plan.algos)
    m = size // 8
    for a in heads:
        d = 2 if a["layer"][:4] in ("l30b", "l31a", "l31b", "l40a") else 4
        assert a["fold"] == [d, d, m, m] and a["x"][0] == CASES[size] * d * d and a["x"][2:] == [-(-m // d)] * 2, a
    # on dividing maps the 1x1 projection of layer4.0 and the head conv run folded too; on the others nothing else does
    assert sorted(a["layer"][:4] for a in folded if a not in heads) == (["head", "l40d"] if size == 64 else [])


CHILD = """
import sys
import numpy as np
import planer_amd
from planer_amd.irgen import drn
size, batch, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
g, b = drn.build()
x = drn.make_input(batch, size=size)
net = planer_amd.from_graph(g, b)
y = net(planer_amd.asarray(x)).get()
plan = net.compile(planer_amd.asarray(x))
nfold = sum(1 for a in plan.algos if a.get("fold"))
print("FOLD", repr(net.fold_dilated), net.dilated_folds, net.refolds, nfold)
np.save(out, y)
"""


def _child(size, tmp_path, switch):
    out = str(tmp_path / "drn.npy")
    env = {k: v for k, v in os.environ.items() if k != "PLANER_HIP_DILATED_FOLD"}
    if switch is not None:
        env["PLANER_HIP_DILATED_FOLD"] = switch
    r = subprocess.run([sys.executable, "-c", CHILD, str(size), str(CASES[size]), out], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("FOLD ")][-1].split()
    return np.load(out), line[1], [int(v) for v in line[2:]]


def test_switch_unset_runs_the_unfolded_program(pa, drn64, tmp_path):
    (size, g, b, x, want), (_, forced) = drn64
    y, mode, (folds, refolds, nfold) = _child(size, tmp_path, None)
    assert mode == "False" and (folds, refolds, nfold) == (0, 0, 0)
    assert_close(y, want, RTOL, "drn %d, switch unset" % size)
    assert_close(forced, y, RTOL, "drn %d, folded against unfolded" % size)


def test_switch_one_matches_the_oracle_whatever_it_decides(pa, drn64, tmp_path):
    size, g, b, x, want = drn64[0]
    y, mode, (folds, refolds, nfold) = _child(size, tmp_path, "1")
    assert mode == "True" and 0 <= folds <= 7 and nfold >= folds and (refolds > 0) == (folds > 0)
    print("PLANER_HIP_DILATED_FOLD=1 at size %d: %d of 7 dilated convs folded, %d refold steps" % (size, folds, refolds))
    assert_close(y, want, RTOL, "drn %d, switch 1" % size)

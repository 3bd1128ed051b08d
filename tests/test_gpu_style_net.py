"""The fast-neural-style net (planer_amd.irgen.stylenet) as one channel-quad plan on the GPU: through Net, the pipelined path and
a plan file, against the oracle at the project's tolerance; and the program of PLANER_HIP_INSTNORM_Q4=0 (NCHW instance norms and
pads, a conversion around each) from a fresh child process against the same reference.

Size 32, batch 2: every instance norm takes the one-workgroup form.  Size 96, batch 1: 96 x 96 pixels are more than one
workgroup holds, so the first and the last norm run as chunk statistics + merge-and-apply."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import planer_np as onp
from tests.conftest import ROOT, RTOL, assert_close

pytestmark = pytest.mark.gpu

CASES = {32: 2, 96: 1}          # size -> batch


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


@pytest.fixture(scope="module", params=sorted(CASES), ids=["size%d" % s for s in sorted(CASES)])
def style_model(request):
    from planer_amd.irgen import stylenet
    size = request.param
    g, b = stylenet.build()
    x = stylenet.make_input(CASES[size], size=size)
    ref = onp.OracleNet()
    ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
    ref.load_weights(b)
    return size, g, b, x, ref(x.copy())


@pytest.fixture(scope="module")
def style_net(pa, style_model):
    """-> (the compiled net, its result through net(x)), shared by the tests of one size."""
    size, g, b, x, want = style_model
    net = pa.from_graph(g, b)
    return net, net(pa.asarray(x)).get()


def test_style_net_through_net_pipelined_and_plan_file(pa, style_model, style_net, tmp_path):
    from planer_amd import _lib
    from planer_amd.export import export_plan
    from tests.test_gpu_plan_file import _bind, _run_plan
    size, g, b, x, want = style_model
    net, got = style_net
    assert got.shape == (CASES[size], 3, size, size)
    assert_close(got, want, RTOL, "style %d" % size)
    plan = net.compile(pa.asarray(x))
    norms = [a for a in plan.algos if a["kind"] == "instancenormalization_q4"]
    assert len(norms) == 15 and net.instnorm_fused == 15, plan.algos
    forms = [a["plan"] for a in norms]
    if size * size <= _lib.INSTNORM_Q4_ONE_WG_PIXELS:
        assert forms == ["instnorm-q4 one-wg"] * 15, forms
    else:
        chunks = "instnorm-q4 chunks=%d" % -(-size * size // _lib.INSTNORM_Q4_CHUNK_PIXELS)
        assert forms == [chunks] + ["instnorm-q4 one-wg"] * 13 + [chunks], forms
    assert [a["x"][1:] for a in norms[:3]] == [[32, size, size], [64, size // 2, size // 2], [128, size // 4, size // 4]]
    assert_close(net.submit(pa.asarray(x, ctx=net.ctx)).get(), want, RTOL, "style %d submit" % size)
    path = tmp_path / ("style_%d.plplan" % size)
    blob = export_plan(net, x, path=str(path))
    assert b"pl_instancenorm_q4_f32" in blob and b"pl_instancenorm_f32" not in blob
    out, = _run_plan(_bind(), open(path, "rb").read(), [x])
    assert_close(out, want, RTOL, "style %d plan file" % size)


CHILD = """
import sys
import numpy as np
import planer_amd
from planer_amd.irgen import stylenet
size, batch, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
g, b = stylenet.build()
x = stylenet.make_input(batch, size=size)
net = planer_amd.from_graph(g, b)
y = net(planer_amd.asarray(x)).get()
plan = net.compile(planer_amd.asarray(x))
assert not any(a["kind"] == "instancenormalization_q4" for a in plan.algos), plan.algos
np.save(out, y)
"""


def test_switch_off_program_agrees(pa, style_model, style_net, tmp_path):
    size, g, b, x, want = style_model
    out = str(tmp_path / "nchw.npy")
    env = dict(os.environ, PLANER_HIP_INSTNORM_Q4="0")
    r = subprocess.run([sys.executable, "-c", CHILD, str(size), str(CASES[size]), out], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    eager = np.load(out)
    assert_close(eager, want, RTOL, "style %d, instance norm and pad as NCHW steps" % size)
    assert_close(style_net[1], eager, RTOL, "style %d, Q4 against NCHW norms" % size)

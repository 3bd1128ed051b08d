"""Net compiles the recorded programs on a real MI355X: the ten generator nets at batch 2 and 64 pixels, with the first and
the last conv candidate in place of the timing, as latency and as throughput plans, against
tests/golden/plan_programs_gpu.json -- every step's name, kind, sources and destination, the digest of the parameters, and the
counters a compile leaves on the Net.  No timing decides a program here, so the recording holds on every run."""
import json
import os

import pytest

from tests import plan_programs as PP
from tests.conftest import GOLDEN
from tests.test_conv_layouts import SWITCHES

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "plan_programs_gpu.json")) as f:
    RECORDED = json.load(f)


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for k in SWITCHES + ("PLANER_HIP_CONV_ALGO", "PLANER_HIP_STREAMS", "PLANER_HIP_Q4"):
        monkeypatch.delenv(k, raising=False)


_loaded = {}


def _net(pa, name):
    """One Net at a time: both picks of a net share its weights on the device."""
    if name not in _loaded:
        _loaded.clear()
        g, b, x = PP.load(name, batch=2)
        _loaded[name] = pa.from_graph(g, b), [pa.asarray(x)]
    return _loaded[name]


@pytest.mark.parametrize("name, pick", [(n, p) for n in PP.NETS for p in PP.PICKS])
def test_net_compiles_the_recorded_program(pa, name, pick):
    net, xs = _net(pa, name)
    for mode in ("latency", "throughput"):
        got, want = PP.net_record(net, xs, pick, mode), RECORDED["%s/%s/%s" % (name, pick, mode)]
        assert len(got["steps"]) == len(want["steps"]), (mode, len(got["steps"]), len(want["steps"]))
        for i, (a, b) in enumerate(zip(got["steps"], want["steps"])):
            assert a == b, "%s: step %d is %s, recorded %s" % (mode, i, a, b)
        assert got["paras"] == want["paras"], mode
        assert got["counters"] == want["counters"], mode

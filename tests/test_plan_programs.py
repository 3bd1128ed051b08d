"""The programs plan.compile_front and plan.lower give for the ten generator nets at 64 pixels are the recorded ones
(tests/golden/plan_programs.json: per net the step kinds in flow order and a sha256 of the canonical JSON of (body, flow),
after the front half and after lowering with the first and with the last conv candidate).  The recording was made with the
hand-written pass orders the tests had before the order lived in plan.py; tools/capture_plan_programs.py rewrites it."""
import json
import os

import pytest

from tests import plan_programs as PP
from tests.conftest import GOLDEN
from tests.test_conv_layouts import SWITCHES

with open(os.path.join(GOLDEN, "plan_programs.json")) as f:
    RECORDED = json.load(f)


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def test_every_net_is_recorded():
    assert all(set(RECORDED[stage]) == set(PP.NETS) for stage in ("front", "first", "last"))


@pytest.mark.parametrize("name", list(PP.NETS))
def test_compiled_programs_are_the_recorded_ones(name):
    got = PP.host_programs(name)
    for stage in ("front", "first", "last"):
        want = RECORDED[stage][name]
        assert got[stage]["kinds"] == want["kinds"], stage
        assert got[stage]["sha256"] == want["sha256"], stage

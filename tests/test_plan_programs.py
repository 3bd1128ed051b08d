"""The programs plan.compile_front and plan.lower give for the ten generator nets at 64 pixels are the recorded ones
(tests/golden/plan_programs.json: per net the step kinds in flow order and a sha256 of the canonical JSON of (body, flow),
after the front half and after lowering with the first and with the last conv candidate).  The recording was made with the
hand-written pass orders the tests had before the order lived in plan.py; tools/capture_plan_programs.py rewrites it.

tests/golden/plan_programs_random.json is a second recording, made before the passes were moved onto plan.Steps: a digest
after every pass of plan.FRONT and after plan.lower under seven settings (plan_programs.stages), for the ten nets and for the
150 random graphs test_plan_fusion's fuzz test walks -- shared tensors, in-place ReLU on forked values, several outputs."""
import json
import os

import pytest

from tests import plan_programs as PP
from tests.conftest import GOLDEN
from tests.test_conv_layouts import SWITCHES

with open(os.path.join(GOLDEN, "plan_programs.json")) as f:
    RECORDED = json.load(f)
with open(os.path.join(GOLDEN, "plan_programs_random.json")) as f:
    EVERY_PASS = json.load(f)
CHUNK = 15


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


def test_every_pass_is_recorded():
    assert EVERY_PASS["stages"] == PP.stages()
    assert set(EVERY_PASS["nets"]) == set(PP.NETS) and set(EVERY_PASS["random"]) == {str(s) for s in PP.RANDOM_SEEDS}
    rows = list(EVERY_PASS["nets"].values()) + list(EVERY_PASS["random"].values())
    assert all(len(r) == len(PP.stages()) and None not in r for r in rows)        # every pass ran on every graph


@pytest.mark.parametrize("name", list(PP.NETS))
def test_net_programs_after_every_pass_are_the_recorded_ones(name):
    assert dict(zip(PP.stages(), PP.stage_digests(*PP.load(name)))) == dict(zip(PP.stages(), EVERY_PASS["nets"][name]))


@pytest.mark.parametrize("first", list(PP.RANDOM_SEEDS)[::CHUNK])
def test_random_programs_are_the_recorded_ones(first):
    for seed in list(PP.RANDOM_SEEDS)[first:first + CHUNK]:
        got, want = PP.random_digests(seed), EVERY_PASS["random"][str(seed)]
        assert dict(zip(PP.stages(), got)) == dict(zip(PP.stages(), want)), seed

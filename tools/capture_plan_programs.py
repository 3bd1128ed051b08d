#!/usr/bin/env python3
"""Rewrite tests/golden/plan_programs.json: the programs plan.compile_front and plan.lower give on the host for the nets of
tests/plan_programs.py (what tests/test_plan_programs.py compares against).  Run it when a change to the plan compiler is
meant to change a program, and say in the commit which nets moved and why.

    python tools/capture_plan_programs.py [path]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import plan_programs as PP  # noqa: E402


def main(path=os.path.join(ROOT, "tests", "golden", "plan_programs.json")):
    out = {"front": {}, "first": {}, "last": {}}
    for name in PP.NETS:
        for stage, rec in PP.host_programs(name).items():
            out[stage][name] = rec
        print(name, len(out["front"][name]["kinds"]), "steps, lowered", len(out["first"][name]["kinds"]))
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(*sys.argv[1:2])

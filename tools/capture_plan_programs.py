#!/usr/bin/env python3
"""Rewrite tests/golden/plan_programs.json and plan_programs_random.json: the programs plan.compile_front and plan.lower give
on the host for the nets of tests/plan_programs.py, and the digest after every pass for those nets and for 150 random graphs
(what tests/test_plan_programs.py compares against).  Run it when a change to the plan compiler is meant to change a program,
and say in the commit which nets moved and why.

    python tools/capture_plan_programs.py [path [path of the random recording]]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import plan_programs as PP  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main(path=os.path.join(GOLDEN, "plan_programs.json"), random_path=os.path.join(GOLDEN, "plan_programs_random.json")):
    out = {"front": {}, "first": {}, "last": {}}
    every = {"stages": PP.stages(), "nets": {}, "random": {}}
    for name in PP.NETS:
        for stage, rec in PP.host_programs(name).items():
            out[stage][name] = rec
        every["nets"][name] = PP.stage_digests(*PP.load(name))
        print(name, len(out["front"][name]["kinds"]), "steps, lowered", len(out["first"][name]["kinds"]))
    for seed in PP.RANDOM_SEEDS:
        every["random"][str(seed)] = PP.random_digests(seed)
    print(len(every["random"]), "random graphs")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(random_path, "w") as f:                  # one row a line
        f.write('{\n "stages": %s,\n "nets": {\n%s\n },\n "random": {\n%s\n }\n}\n'
                % (json.dumps(every["stages"]), _rows(every["nets"]), _rows(every["random"])))


def _rows(d):
    return ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in d.items())


if __name__ == "__main__":
    main(*sys.argv[1:3])

"""Recorded plan programs (tests/golden/plan_programs.json on the host, plan_programs_gpu.json from Net on the device): the ten
generator nets at 64 pixels, the canonical form of a program and its digest.  tests/test_plan_programs.py and
tests/test_gpu_plan_programs.py compare against the recordings; tools/capture_plan_programs.py writes the host ones, the
second of which (plan_programs_random.json) holds a digest after every pass for the ten nets and 150 random graphs."""
import hashlib
import json

import numpy as np

from planer_amd.conv_layouts import STAGED_LAYOUTS
from planer_amd.irgen import customnet, drn, edsr, fpn, mobilenetv2, resnet18, resnet_gn, stylenet, unet, yolov3

# name -> (generator, build keywords).  Every input is 64 x 64.
NETS = {"customnet": (customnet, {}), "resnet18": (resnet18, {}), "yolov3": (yolov3, {}), "mobilenetv2": (mobilenetv2, {}),
        "unet": (unet, {}), "stylenet": (stylenet, {}), "drn": (drn, {}), "fpn": (fpn, {}),
        "edsr": (edsr, {"size": 64}), "resnet_gn": (resnet_gn, {"size": 64})}
PICKS = {"first": lambda cands: cands[0], "last": lambda cands: cands[-1]}
# what a compile leaves on the Net beside the program
COUNTERS = ("pixel_shuffles_fused", "groupnorms_fused", "instnorm_fused", "linear_adds_fused", "dilated_folds", "refolds",
            "conv_pairs", "wino_chains", "conv_wino_fused")


def load(name, batch=1):
    """-> (graph, blob, input) of a recorded net."""
    mod, kw = NETS[name]
    g, b = mod.build(**kw)
    return g, b, mod.make_input(batch) if mod is customnet else mod.make_input(batch, size=64)


def plain(v):
    """Numpy values as lists and Python numbers, tuples as lists: what json writes the same way everywhere."""
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, dict):
        return {str(k): plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v


def digest(obj):
    """sha256 of the canonical JSON of `obj`."""
    return hashlib.sha256(json.dumps(plain(obj), sort_keys=True).encode()).hexdigest()


def host_record(body, flow):
    """A (body, flow) program as recorded: its step kinds in flow order and the digest of all of it."""
    kinds = {b[0]: b[1] for b in body}
    return {"kinds": [kinds[names[0]] for _, names, _ in flow], "sha256": digest([body, flow])}


def net_record(net, xs, pick, mode):
    """The program `net` compiles for device inputs `xs` under `mode` with PICKS[pick] in place of the conv timing: its steps
    [name, kind, srcs, dst], the digest of their parameters, and the counters the compile left on the net."""
    from tests.plan_audit import program
    net._pick_conv_algo = lambda cands, K, srcs, para, shapes, q4=False: PICKS[pick](cands)
    prog, _ = program(net, xs, mode)
    steps, paras = [], []
    for src, names, dst in prog.flow:
        obj = prog.objs[names[0]]
        steps.append(plain([names[0], obj.name, src if isinstance(src, list) else [src], dst]))
        paras.append(obj.para())
    return {"steps": steps, "paras": digest(paras), "counters": {k: int(getattr(net, k)) for k in COUNTERS}}


# The second host recording (tests/golden/plan_programs_random.json): the digest after every pass, for the ten nets and for
# the random graphs of test_plan_fusion's fuzz test.  stages() is the order of a recorded row: the passes of plan.FRONT
# (compile_front(stop=...)), then plan.lower under each of LOWERINGS.
RANDOM_SEEDS = range(150)
# (the first candidate is the direct kernel and the last a fused one: the chain switches get the pick that takes a staged
# Winograd layout wherever one applies, which is what they act on)
_STAGED = {"pick": lambda cands, *_: next((c for c in cands if c in STAGED_LAYOUTS), cands[0])}
LOWERINGS = {"first": {"pick": lambda cands, *_: cands[0]}, "last": {"pick": lambda cands, *_: cands[-1]}, "staged": _STAGED,
             "stages": dict(_STAGED, wino_chain="stages"), "unchained": dict(_STAGED, wino_chain="0"), "unpaired": {"pair": False},
             "no_conv1x1": dict(_STAGED, small=None)}
DIGEST_CHARS = 16       # a row keeps this much of each sha256: 64 bits tell two programs apart, and the file stays small


def stages():
    from planer_amd.plan import FRONT
    return list(FRONT) + ["lower:" + k for k in LOWERINGS]


def stage_digests(g, b, x):
    """-> [digest after each stage of stages()] for this graph (None for a pass of FRONT that did not run).  The maps of the
    random graphs are tiny, so layouts are forced; `worth` always agrees, so that drn's dilated convs fold."""
    from planer_amd.plan import FRONT, lower
    from tests.plan_audit import cpu_front
    row = []
    for stop in FRONT:
        body, flow, counts, shapes = cpu_front(g, b, x, force=True, worth=lambda *_: True, stop=stop)
        row.append(digest([body, flow])[:DIGEST_CHARS] if stop in counts else None)
    for kw in LOWERINGS.values():
        row.append(digest(list(lower(body, flow, [i[0] for i in g["inits"]], shapes, **kw)[:2]))[:DIGEST_CHARS])
    return row


def random_digests(seed):
    from tests.random_nets import random_net
    g, b, xs = random_net(40000 + seed)
    return stage_digests(g, b, xs[0])


def host_programs(name):
    """A recorded net through plan.compile_front and plan.lower on the host -> {"front": record, pick: record of the lowered
    program under that pick}."""
    from planer_amd.plan import lower
    from tests.plan_audit import cpu_front
    g, b, x = load(name)
    body, flow, _, shapes = cpu_front(g, b, x)
    out = {"front": host_record(body, flow)}
    for pick, fn in PICKS.items():
        out[pick] = host_record(*lower(body, flow, [i[0] for i in g["inits"]], shapes, pick=lambda cands, *_, fn=fn: fn(cands))[:2])
    return out

"""Recorded plan programs (tests/golden/plan_programs.json on the host, plan_programs_gpu.json from Net on the device): the ten
generator nets at 64 pixels, the canonical form of a program and its digest.  tests/test_plan_programs.py and
tests/test_gpu_plan_programs.py compare against the recordings; tools/capture_plan_programs.py writes the host one."""
import hashlib
import json

import numpy as np

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

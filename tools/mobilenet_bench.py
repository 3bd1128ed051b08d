"""MobileNet-v2 (planer_amd/irgen/mobilenetv2.py) at batch 32, 224x224, fp32 on one GPU: one JSON line with
  pipelined_img_s   images/s on the pipelined feed / launch path bench.py times (median of --repeats regions of --steps steps)
  call_img_s        images/s of net(x), one call at a time (device synchronise after each)
  parity_rel_err    max|logits - oracle| / max|oracle| of the pipelined plan's output, first --check images
  convs             the algorithm every conv ran (net.W_LAYOUT_NAMES) and its launch plan
    python tools/mobilenet_bench.py [--root TREE] [--batch 32] [--steps 50] [--warmup 10] [--repeats 5] [--calls 10]
--root: the source tree whose planer_amd is measured (default: this one).  The graph, its weights and the oracle always come from
THIS tree, so the same script times two builds (e.g. a checkout of the parent commit) on the same work."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--check", type=int, default=2)
    args = ap.parse_args()
    root = os.path.abspath(args.root)

    # the workload, from this tree (pure numpy: nothing touches the GPU yet)
    sys.path.insert(0, HERE)
    from oracle import planer_np as onp
    from planer_amd.irgen import mobilenetv2
    g, blob = mobilenetv2.build()
    xs_host = [mobilenetv2.make_input(args.batch, seed=1 + i, size=args.size) for i in range(2)]
    ref = onp.OracleNet()
    ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
    ref.load_weights(blob)
    want = ref(xs_host[0][:args.check].copy())
    # ... measured on the package of --root
    for m in [m for m in sys.modules if m == "planer_amd" or m.startswith("planer_amd.")]:
        del sys.modules[m]
    sys.path.insert(0, root)
    import planer_amd
    from planer_amd import net as net_mod
    assert os.path.dirname(os.path.dirname(os.path.abspath(planer_amd.__file__))) == root, planer_amd.__file__

    ctx = planer_amd.hip.context()
    net = planer_amd.from_graph(g, blob)
    xs = [planer_amd.asarray(a, ctx=ctx) for a in xs_host]
    t0 = time.perf_counter()
    plan = net.compile(xs[0], mode="throughput")
    ctx.synchronize()
    compile_s = time.perf_counter() - t0
    state = {"i": 0}

    def step():
        plan.feed([xs[state["i"] & 1]])
        plan.launch(join=False)
        state["i"] += 1

    def sync():
        plan.join()
        ctx.synchronize()

    for _ in range(args.warmup):
        step()
    sync()
    spans = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        sync()
        spans.append(time.perf_counter() - t0)
    rates = sorted(args.batch * args.steps / t for t in spans)

    plan.feed([xs[0]])
    plan.launch(join=False)
    sync()
    out = plan.outputs
    got = (out[0] if isinstance(out, tuple) else out).get()
    parity = float(np.abs(got[:args.check].astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-30))

    for _ in range(2):
        net(xs[0])
    ctx.synchronize()
    calls = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        net(xs[0])
        ctx.synchronize()
        calls.append(time.perf_counter() - t0)
    call_rate = args.batch / sorted(calls)[len(calls) // 2]

    convs = [{"layer": a["layer"], "w_layout": a["w_layout"], "algo": net_mod.W_LAYOUT_NAMES.get(a["w_layout"], str(a["w_layout"])),
              "plan": a["plan"]} for a in plan.algos]
    print(json.dumps({"workload": "mobilenetv2", "batch": args.batch, "size": args.size, "dtype": "fp32", "root": root,
                      "pipelined_img_s": round(rates[len(rates) // 2], 1),
                      "pipelined_spread": [round(rates[0], 1), round(rates[-1], 1)],
                      "call_img_s": round(call_rate, 1), "parity_rel_err": parity, "parity_checked_images": args.check,
                      "compile_s": round(compile_s, 2), "steps": args.steps, "repeats": args.repeats, "convs": convs}))
    if not parity <= 1e-4:
        sys.exit("parity failure: %.3g" % parity)


if __name__ == "__main__":
    main()

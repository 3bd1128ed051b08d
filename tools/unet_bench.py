"""U-Net (planer_amd/irgen/unet.py) at batch 8, 256x256, fp32 on one GPU: one JSON line with
  pipelined_img_s   images/s on the pipelined feed / launch path bench.py times (median of --repeats regions of --steps steps)
  call_img_s        images/s of net(x), one call at a time (device synchronise after each)
  parity_rel_err    max|class map - oracle| / max|oracle| of the pipelined plan's output, first --check images
  convs             the algorithm every conv ran (net.W_LAYOUT_NAMES) and its launch plan (a build that runs transposed convs
                    outside the conv kernels lists only the others)
    python tools/unet_bench.py [--root TREE] [--up k2|k3] [--batch 8] [--size 256] [--steps 20] [--warmup 5] [--repeats 5]
                               [--calls 10]
--up: the up-step form (unet.build): k2 = ConvTranspose2d(k=2, s=2) + bias, k3 = ConvTranspose2d(k=3, s=2, p=1, op=1) + BN + ReLU.
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
    ap.add_argument("--up", default="k2", choices=["k2", "k3"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--check", type=int, default=1)
    args = ap.parse_args()
    root = os.path.abspath(args.root)

    # the workload, from this tree (pure numpy: nothing touches the GPU yet)
    sys.path.insert(0, HERE)
    from oracle import planer_np as onp
    from planer_amd.irgen import unet
    g, blob = unet.build(up=args.up)
    xs_host = [unet.make_input(args.batch, seed=1 + i, size=args.size) for i in range(2)]
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
    print(json.dumps({"workload": "unet-" + args.up, "batch": args.batch, "size": args.size, "dtype": "fp32", "root": root,
                      "pipelined_img_s": round(rates[len(rates) // 2], 1),
                      "pipelined_spread": [round(rates[0], 1), round(rates[-1], 1)],
                      "call_img_s": round(call_rate, 1), "parity_rel_err": parity, "parity_checked_images": args.check,
                      "compile_s": round(compile_s, 2), "steps": args.steps, "repeats": args.repeats, "convs": convs}))
    if not parity <= 1e-4:
        sys.exit("parity failure: %.3g" % parity)


if __name__ == "__main__":
    main()

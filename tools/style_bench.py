"""The fast-neural-style net (planer_amd/irgen/stylenet.py) at batch 8, 224x224, fp32 on one GPU, with instance norm and pad as
channel-quad steps (the default) and as NCHW steps (PLANER_HIP_INSTNORM_Q4=0), one after the other in the same session: one
JSON line with, per arm,
  pipelined_img_s   images/s on the pipelined feed / launch path bench.py times (median of --repeats regions of --steps steps)
  call_ms           milliseconds of net(x), one call at a time on one stream (device synchronise after each; median of --calls)
  parity_rel_err    max|image - oracle| / max|oracle| of the pipelined plan's output, first --check images
  norms             the form every instance norm took (plan.algos)
and `kernels`: per instance-norm shape of the net, the time of the Q4 launch(es) with the ReLU tail, the bytes they move (one
read + one write in the one-workgroup form, two reads + one write in the chunked form), the fraction of the 8 TB/s HBM peak that
is, and the NCHW kernel (plus the from_q4 / to_q4 it needs inside a Q4 plan) on the same tensor.
    python tools/style_bench.py [--batch 8] [--size 224] [--steps 20] [--warmup 5] [--repeats 5] [--calls 10]
Every arm is a fresh child process; the parent never opens the GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8e12


def arm(args):
    sys.path.insert(0, HERE)
    from oracle import planer_np as onp
    from planer_amd.irgen import stylenet
    import planer_amd
    g, blob = stylenet.build()
    xs_host = [stylenet.make_input(args.batch, seed=1 + i, size=args.size) for i in range(2)]
    want = None
    if args.check:
        ref = onp.OracleNet()
        ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
        ref.load_weights(blob)
        want = ref(xs_host[0][:args.check].copy())
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
    parity = None
    if want is not None:
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
    print(json.dumps({"instnorm_q4": os.environ.get("PLANER_HIP_INSTNORM_Q4", "1") != "0",
                      "pipelined_img_s": round(rates[len(rates) // 2], 1), "pipelined_spread": [round(rates[0], 1), round(rates[-1], 1)],
                      "call_ms": round(1e3 * sorted(calls)[len(calls) // 2], 3), "parity_rel_err": parity,
                      "compile_s": round(compile_s, 2), "streams": getattr(plan, "streams", None),
                      "norms": [a["plan"] for a in plan.algos if a["kind"] == "instancenormalization_q4"]}))
    if parity is not None and not parity <= 1e-4:
        sys.exit("parity failure: %.3g" % parity)


def kernels(args):
    sys.path.insert(0, HERE)
    import planer_amd
    from planer_amd import _lib, hip, q4
    from planer_amd.layer import InstanceNormalization
    ctx = hip.context()
    rng = np.random.default_rng(5)
    n, s = args.batch, args.size
    rows = []
    for c, side in ((32, s), (64, s // 2), (128, s // 4)):
        x = planer_amd.asarray(rng.standard_normal((n, c, side, side)).astype(np.float32), ctx=ctx)
        sc = planer_amd.asarray(rng.uniform(0.5, 1.5, c).astype(np.float32), ctx=ctx)
        bi = planer_amd.asarray(rng.standard_normal(c).astype(np.float32), ctx=ctx)
        xq = q4.to_q4(x)

        def timed(fn, bursts=5, reps=20):
            for _ in range(3):
                fn()
            best = None
            for _ in range(bursts):
                e0 = hip.Event(ctx).record()
                for _ in range(reps):
                    fn()
                e1 = hip.Event(ctx).record()
                t = e0.elapsed_ms(e1) / reps
                best = t if best is None else min(best, t)
            return best * 1e-3
        t_q4 = timed(lambda: q4.InstanceNormQ4(xq, sc, bi, act=1))
        form = ctx.last_conv_plan()
        t_nchw = timed(lambda: InstanceNormalization(x, sc, bi))
        t_conv = timed(lambda: q4.to_q4(q4.from_q4(xq)))
        nbytes = x.size * 4
        passes = 2 if side * side <= _lib.INSTNORM_Q4_ONE_WG_PIXELS else 3
        rows.append({"x": [n, c, side, side], "form": form, "q4_us": round(t_q4 * 1e6, 1), "q4_bytes": passes * nbytes,
                     "q4_gb_s": round(passes * nbytes / t_q4 / 1e9, 1), "q4_fraction_of_hbm_peak": round(passes * nbytes / t_q4 / HBM_PEAK, 3),
                     "nchw_us": round(t_nchw * 1e6, 1), "nchw_gb_s": round(3 * nbytes / t_nchw / 1e9, 1),
                     "from_q4_plus_to_q4_us": round(t_conv * 1e6, 1)})
    print(json.dumps({"kernels": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--check", type=int, default=1)
    ap.add_argument("--child", choices=["arm", "kernels"])
    args = ap.parse_args()
    if args.child:
        return arm(args) if args.child == "arm" else kernels(args)
    out = {"workload": "stylenet", "batch": args.batch, "size": args.size, "dtype": "fp32", "steps": args.steps, "repeats": args.repeats}
    passed = [a for a in sys.argv[1:]]
    for name, child, switch in (("q4", "arm", "1"), ("nchw", "arm", "0"), ("kernels", "kernels", "1")):
        env = dict(os.environ, PLANER_HIP_INSTNORM_Q4=switch)
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + passed + ["--child", child], env=env, capture_output=True,
                           text=True, timeout=900)
        if r.returncode != 0:
            sys.exit("%s arm failed (exit %d):\n%s" % (name, r.returncode, r.stderr[-3000:]))
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        out[name] = line["kernels"] if child == "kernels" else line
    out["pipelined_speedup"] = round(out["q4"]["pipelined_img_s"] / out["nchw"]["pipelined_img_s"], 3)
    out["call_speedup"] = round(out["nchw"]["call_ms"] / out["q4"]["call_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

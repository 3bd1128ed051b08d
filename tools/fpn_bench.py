"""The Panoptic-FPN segmentation net (planer_amd/irgen/fpn.py) at batch 32, 224x224, fp32 on one GPU, with its linear upsamples
as channel-quad steps (PLANER_HIP_LINEAR_Q4=1) and as NCHW steps between two layout conversions (=0: the program of a compiler
without the linear Q4 kernels), the two arms ALTERNATING --rounds times in one session so that the spread of the repeats is
visible next to the gain.  One JSON line per arm run, then one summary line.  Per arm run:
  pipelined_img_s   images/s on the pipelined feed / launch path bench.py times (median of --repeats regions of --steps steps)
  call_ms           milliseconds of net(x), one call at a time on one stream (device synchronise after each; median of --calls)
  parity_rel_err    max|y - oracle| / max|oracle| of the pipelined plan's output, first --check images
  steps             counts of upsample_q4 / resize_q4 / fused adds / to_q4 / from_q4 / NCHW upsample steps of the plan
and once (`kernels`), per distinct upsample shape of the net, with and without a residual: pl_upsample_linear_q4_f32's time and
bytes -- one read of the input, one write of the output, one read of the residual -- next to pl_upsample_nearest_q4_f32 at the
same shape (same store stream, one load per output instead of four), and the three-kernel route it replaces (pl_q4_to_nchw_f32,
pl_upsample_linear_f32, pl_nchw_to_q4_f32, and pl_add_f32 where there is a residual).  Each is the entry point called alone on
preallocated tensors, weight table marshalled once; `launch_floor_us` is the same loop on a one-quad tensor, and a figure within
1.5x of it is marked `launch_bound` and given no rate.
    python tools/fpn_bench.py [--batch 32] [--size 224] [--rounds 3] [--steps 20] [--warmup 5] [--repeats 5] [--calls 10] [--via upsample]
Every arm run is a fresh child process; the parent never opens the GPU.  The children share one tuning cache (a temporary file
unless PLANER_HIP_TUNE_CACHE names one), so every round after the first runs the kernels the first one picked."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8e12
COUNTED = ("upsample_q4", "resize_q4", "upsample_add_q4", "resize_add_q4", "add_q4", "to_q4", "from_q4", "upsample", "resize")


def arm(args):
    sys.path.insert(0, HERE)
    from oracle import planer_np as onp
    from planer_amd.irgen import fpn
    import planer_amd
    g, blob = fpn.build(via=args.via)
    xs_host = [fpn.make_input(args.batch, seed=1 + i, size=args.size) for i in range(2)]
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
    # the step kinds of the program this plan runs
    shapes = {k: a.shape for k, a in zip(net.input, xs[:1])}
    shapes.update({k: w.shape for k, w in zip(net.inits, net.weights)})
    net._interpret(net._program, [xs[0].copy()], shapes=shapes)
    with net.picking("throughput"):
        prog, _ = net._fuse(shapes, net.use_fusion)
    kinds = [prog.objs[names[0] if isinstance(names, list) else names].name for _, names, _ in prog.flow]
    steps = {k: kinds.count(k) for k in COUNTED}
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
    print(json.dumps({"linear_q4": os.environ.get("PLANER_HIP_LINEAR_Q4", "1"), "round": args.round, "via": args.via,
                      "pipelined_img_s": round(rates[len(rates) // 2], 1), "pipelined_spread": [round(rates[0], 1), round(rates[-1], 1)],
                      "call_ms": round(1e3 * sorted(calls)[len(calls) // 2], 3), "parity_rel_err": parity,
                      "compile_s": round(compile_s, 2), "streams": getattr(plan, "streams", None), "steps": steps,
                      "linear_adds_fused": net.linear_adds_fused, "tune_source": net.tune_source()}))
    if parity is not None and not parity <= 1e-4:
        sys.exit("parity failure: %.3g" % parity)


def kernels(args):
    """Device time per entry point.  Every timed closure is ONE C call on preallocated tensors: the weight table is built and
    marshalled once outside the loop and nothing is allocated inside it, so a burst measures launches and kernels, not Python.
    `launch_floor_us` is the same loop on a one-quad tensor: what a call costs when the kernel is nothing.  A figure at the floor
    is launch-bound, not a kernel time, and carries no rate."""
    sys.path.insert(0, HERE)
    import planer_amd
    from planer_amd import _lib, hip, q4
    from planer_amd.layer import _linear_weights
    ctx = hip.context()
    lib = _lib.load()
    h = ctx.handle
    rng = np.random.default_rng(5)
    n, s = args.batch, args.size
    w = _linear_weights(2, 2)
    tab = (_lib.c_float * w.size)(*w.reshape(-1).tolist())

    def timed(fn, bursts=5, reps=50):
        for _ in range(5):
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

    def ok(rc):
        _lib.check(rc)

    tx, ty = hip.zeros((1, 1, 1, 1, 4), ctx=ctx), hip.zeros((1, 1, 2, 2, 4), ctx=ctx)
    floors = {"nearest_q4": timed(lambda: ok(lib.pl_upsample_nearest_q4_f32(h, tx.ptr, ty.ptr, 1, 4, 1, 1, 2, 2))),
              "linear_q4": timed(lambda: ok(lib.pl_upsample_linear_q4_f32(h, tx.ptr, ty.ptr, None, 1, 4, 1, 1, 2, 2, tab)))}

    def move(t, nbytes, kind):
        out = {"us": round(t * 1e6, 1), "bytes": nbytes, "launch_bound": bool(t < 1.5 * floors[kind])}
        if not out["launch_bound"]:
            out.update(gb_s=round(nbytes / t / 1e9, 1), fraction_of_hbm_peak=round(nbytes / t / HBM_PEAK, 3))
        return out
    # the distinct (channels, input side) of the net's nine x2 steps: top-down 128 channels from 1/32, 1/16, 1/8; heads 64 channels
    # from 1/32, 1/16, 1/8
    rows = []
    for c in (128, 64):
        for div in (32, 16, 8):
            m = s // div
            x = planer_amd.asarray(rng.standard_normal((n, c, m, m)).astype(np.float32), ctx=ctx)
            r = planer_amd.asarray(rng.standard_normal((n, c, 2 * m, 2 * m)).astype(np.float32), ctx=ctx)
            xq, rq = q4.to_q4(x), q4.to_q4(r)
            yq, zq, y, xn = (hip.empty(rq.shape, ctx=ctx), hip.empty(rq.shape, ctx=ctx), hip.empty(r.shape, ctx=ctx),
                              hip.empty(x.shape, ctx=ctx))
            nin, nout = x.size * 4, r.size * 4
            t_lin = timed(lambda: ok(lib.pl_upsample_linear_q4_f32(h, xq.ptr, yq.ptr, None, n, c, m, m, 2, 2, tab)))
            t_res = timed(lambda: ok(lib.pl_upsample_linear_q4_f32(h, xq.ptr, yq.ptr, rq.ptr, n, c, m, m, 2, 2, tab)))
            t_near = timed(lambda: ok(lib.pl_upsample_nearest_q4_f32(h, xq.ptr, yq.ptr, n, c, m, m, 2, 2)))
            t_from = timed(lambda: ok(lib.pl_q4_to_nchw_f32(h, xq.ptr, xn.ptr, n, c, m * m)))
            t_up = timed(lambda: ok(lib.pl_upsample_linear_f32(h, x.ptr, y.ptr, n * c, m, m, 2, 2, tab)))
            t_to = timed(lambda: ok(lib.pl_nchw_to_q4_f32(h, y.ptr, yq.ptr, n, c, 4 * m * m)))
            t_add = timed(lambda: ok(lib.pl_add_f32(h, yq.ptr, rq.ptr, zq.ptr, yq.size)))
            row = {"x": [n, c, m, m], "factors": [2, 2], "linear_q4": move(t_lin, nin + nout, "linear_q4"),
                   "linear_q4_with_residual": move(t_res, nin + 2 * nout, "linear_q4"), "nearest_q4": move(t_near, nin + nout, "nearest_q4"),
                   "nchw_route_us": {"from_q4": round(t_from * 1e6, 1), "upsample_linear": round(t_up * 1e6, 1),
                                     "to_q4": round(t_to * 1e6, 1), "add": round(t_add * 1e6, 1),
                                     "three_kernels": round((t_from + t_up + t_to) * 1e6, 1),
                                     "four_kernels": round((t_from + t_up + t_to + t_add) * 1e6, 1)}}
            if not (row["linear_q4"]["launch_bound"] or row["nearest_q4"]["launch_bound"]):
                row["linear_over_nearest"] = round(t_lin / t_near, 3)
            rows.append(row)
            del x, r, xq, rq, yq, zq, y, xn
    print(json.dumps({"kernels": rows, "launch_floor_us": {k: round(v * 1e6, 1) for k, v in floors.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--check", type=int, default=1)
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--via", choices=["upsample", "resize"], default="upsample")
    ap.add_argument("--child", choices=["arm", "kernels"])
    args = ap.parse_args()
    if args.child:
        return arm(args) if args.child == "arm" else kernels(args)
    passed = [a for a in sys.argv[1:]]
    tmp = None
    cache = os.environ.get("PLANER_HIP_TUNE_CACHE")
    if not cache:
        tmp = tempfile.mkdtemp(prefix="fpn_bench_")
        cache = os.path.join(tmp, "tune.txt")

    def child(kind, switch, rnd):
        env = dict(os.environ, PLANER_HIP_LINEAR_Q4=switch, PLANER_HIP_TUNE_CACHE=cache)
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + passed + ["--child", kind, "--round", str(rnd)], env=env,
                           capture_output=True, text=True, timeout=1100)
        if r.returncode != 0:
            sys.exit("%s child, switch %s, round %d failed (exit %d):\n%s" % (kind, switch, rnd, r.returncode, r.stderr[-3000:]))
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    out = {"workload": "fpn-resnet18", "batch": args.batch, "size": args.size, "dtype": "fp32", "steps": args.steps,
           "repeats": args.repeats, "rounds": args.rounds, "via": args.via}
    out.update(child("kernels", "1", 0))
    print(json.dumps({"kernels": out["kernels"], "launch_floor_us": out["launch_floor_us"]}), flush=True)
    runs = {"1": [], "0": []}
    for rnd in range(args.rounds):
        for switch in ("1", "0"):
            line = child("arm", switch, rnd)
            runs[switch].append(line)
            print(json.dumps(line), flush=True)
    for switch, name in (("1", "linear_q4"), ("0", "nchw")):
        rates, calls = [r["pipelined_img_s"] for r in runs[switch]], [r["call_ms"] for r in runs[switch]]
        out[name] = {"pipelined_img_s": rates, "call_ms": calls, "median_img_s": sorted(rates)[len(rates) // 2],
                     "median_call_ms": sorted(calls)[len(calls) // 2], "img_s_spread": [min(rates), max(rates)],
                     "call_ms_spread": [min(calls), max(calls)], "steps": runs[switch][-1]["steps"],
                     "parity_rel_err": max(r["parity_rel_err"] or 0.0 for r in runs[switch])}
    out["pipelined_speedup"] = round(out["linear_q4"]["median_img_s"] / out["nchw"]["median_img_s"], 3)
    out["call_speedup"] = round(out["nchw"]["median_call_ms"] / out["linear_q4"]["median_call_ms"], 3)
    # the default follows the measurement: on unless the on arm's median is below the off arm's by more than the off arm's spread
    off = out["nchw"]
    out["keep_on"] = bool(out["linear_q4"]["median_img_s"] >= off["median_img_s"] - (off["img_s_spread"][1] - off["img_s_spread"][0]))
    print(json.dumps(out))
    if tmp:
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()

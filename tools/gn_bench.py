"""ResNet-18-GN (planer_amd/irgen/resnet_gn.py) at batch 32, 224x224, fp32 on one GPU, with its group norms as one-launch
channel-quad steps (PLANER_HIP_GROUPNORM_Q4=1) and as reshape / instancenormalization / reshape / mul / add between two layout
conversions (=0: the program of a compiler without plan.fuse_groupnorm), the two arms ALTERNATING --rounds times in one session so
that the spread of the repeats is visible next to the gain.  One JSON line per arm run, then one summary line.  Per arm run:
  pipelined_img_s   images/s on the pipelined feed / launch path bench.py times (median of --repeats regions of --steps steps)
  call_ms           milliseconds of net(x), one call at a time on one stream (device synchronise after each; median of --calls)
  parity_rel_err    max|y - oracle| / max|oracle| of the pipelined plan's output, first --check images
  steps             counts of the norm, conversion and tail steps of the plan
and once (`kernels`), per distinct norm shape of the net: pl_groupnorm_q4_f32's time alone and with the residual and relu in its
write pass, the five kernels it replaces (pl_q4_to_nchw_f32, pl_instancenorm_f32, the two broadcast pl_binary_f32, pl_nchw_to_q4_f32)
plus the pl_add_f32 and pl_relu_f32 of the tail, and pl_instancenorm_q4_f32 on the same tensor for its byte rate.  Bytes are one
read and one write of the tensor, plus one read of the residual; `launch_floor_us` is the same loop on a one-quad tensor, and a
figure within 1.5x of it is marked `launch_bound` and given no rate.
    python tools/gn_bench.py [--batch 32] [--size 224] [--groups 32] [--rounds 3] [--steps 10] [--warmup 3] [--repeats 5] [--calls 10]
Every arm run is a fresh child process under a timeout of its own; the parent never opens the GPU (it runs the numpy oracle once and
hands the result to the children).  The children share one tuning cache (a temporary file unless PLANER_HIP_TUNE_CACHE names one), so
every round after the first runs the kernels the first one picked."""
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
COUNTED = ("groupnorm_q4", "groupnorm", "to_q4", "from_q4", "reshape", "instancenormalization", "mul", "add", "add_q4", "relu", "relu_q4")


def build(args):
    sys.path.insert(0, HERE)
    from planer_amd.irgen import resnet_gn
    g, blob = resnet_gn.build(groups=args.groups, width=args.width, size=args.size)
    return resnet_gn, g, blob


def arm(args):
    gen, g, blob = build(args)
    import planer_amd
    xs_host = [gen.make_input(args.batch, seed=1 + i, size=args.size) for i in range(2)]
    want = np.load(args.want) if args.want else None
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
        k = want.shape[0]
        parity = float(np.abs(got[:k].astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-30))
    for _ in range(2):
        net(xs[0])
    ctx.synchronize()
    calls = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        net(xs[0])
        ctx.synchronize()
        calls.append(time.perf_counter() - t0)
    print(json.dumps({"groupnorm_q4": os.environ.get("PLANER_HIP_GROUPNORM_Q4", "1"), "round": args.round,
                      "pipelined_img_s": round(rates[len(rates) // 2], 1), "pipelined_spread": [round(rates[0], 1), round(rates[-1], 1)],
                      "call_ms": round(1e3 * sorted(calls)[len(calls) // 2], 3), "parity_rel_err": parity,
                      "compile_s": round(compile_s, 2), "streams": getattr(plan, "streams", None), "steps": steps,
                      "groupnorms_fused": net.groupnorms_fused, "tune_source": net.tune_source()}))
    if parity is not None and not parity <= 1e-4:
        sys.exit("parity failure: %.3g" % parity)


def norm_shapes(g, blob):
    """The distinct (C, H, W) of the graph's norms, read from the second reshapes' shape constants."""
    out, pos = [], 0
    for name, shape, dt in g["inits"]:
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
        if name.startswith("gn_merge_"):
            v = blob[pos:pos + nbytes].view(dt).tolist()
            if tuple(v[1:]) not in out:
                out.append(tuple(v[1:]))
        pos += nbytes
    return out


def kernels(args):
    """Device time per entry point.  Every timed closure is ONE C call on preallocated tensors, nothing allocated inside the
    loop, so a burst measures launches and kernels, not Python.  The norms work in place: a burst renormalises its own output,
    which stays finite."""
    _, g, blob = build(args)
    import planer_amd
    from planer_amd import _lib, hip, q4
    ctx = hip.context()
    lib = _lib.load()
    h = ctx.handle
    rng = np.random.default_rng(5)
    n, G = args.batch, args.groups

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

    def ok(rc):
        _lib.check(rc)

    one = planer_amd.asarray(np.ones(4, np.float32), ctx=ctx)
    tx = hip.zeros((1, 1, 1, 1, 4), ctx=ctx)
    floor = timed(lambda: ok(lib.pl_groupnorm_q4_f32(h, tx.ptr, one.ptr, one.ptr, one.ptr, one.ptr, None, 1, 4, 1, 1, 1e-5, 0)))

    def move(t, nbytes):
        out = {"us": round(t * 1e6, 1), "bytes": nbytes, "launch_bound": bool(t < 1.5 * floor)}
        if not out["launch_bound"]:
            out.update(gb_s=round(nbytes / t / 1e9, 1), fraction_of_hbm_peak=round(nbytes / t / HBM_PEAK, 3))
        return out

    rows = []
    for c, hh, ww in norm_shapes(g, blob):
        hw = hh * ww
        x = planer_amd.asarray(rng.standard_normal((n, c, hh, ww)).astype(np.float32), ctx=ctx)
        xq, rq = q4.to_q4(x), q4.to_q4(planer_amd.asarray(rng.standard_normal((n, c, hh, ww)).astype(np.float32), ctx=ctx))
        y = hip.empty(x.shape, ctx=ctx)
        gs, gb = planer_amd.asarray(np.ones(G, np.float32), ctx=ctx), planer_amd.asarray(np.zeros(G, np.float32), ctx=ctx)
        cs, cb = planer_amd.asarray(np.ones(c, np.float32), ctx=ctx), planer_amd.asarray(np.zeros(c, np.float32), ctx=ctx)
        ga = planer_amd.asarray(rng.uniform(0.5, 1.5, c).astype(np.float32), ctx=ctx)
        be = planer_amd.asarray((rng.standard_normal(c) * 0.1).astype(np.float32), ctx=ctx)
        nbytes = 2 * x.size * 4
        t_gn = timed(lambda: ok(lib.pl_groupnorm_q4_f32(h, xq.ptr, gs.ptr, gb.ptr, ga.ptr, be.ptr, None, n, c, hw, G, 1e-5, 0)))
        form = ctx.last_conv_plan()
        t_tail = timed(lambda: ok(lib.pl_groupnorm_q4_f32(h, xq.ptr, gs.ptr, gb.ptr, ga.ptr, be.ptr, rq.ptr, n, c, hw, G, 1e-5, 1)))
        t_in = timed(lambda: ok(lib.pl_instancenorm_q4_f32(h, xq.ptr, cs.ptr, cb.ptr, None, n, c, hw, 1e-5, 0)))
        t_from = timed(lambda: ok(lib.pl_q4_to_nchw_f32(h, xq.ptr, x.ptr, n, c, hw)))
        t_norm = timed(lambda: ok(lib.pl_instancenorm_f32(h, x.ptr, gs.ptr, gb.ptr, n * G, G, c // G * hw, 1e-5)))
        t_mul = timed(lambda: ok(lib.pl_binary_f32(h, x.ptr, ga.ptr, y.ptr, n, c, hw, 2, 0, 1)))
        t_add = timed(lambda: ok(lib.pl_binary_f32(h, y.ptr, be.ptr, x.ptr, n, c, hw, 0, 0, 1)))
        t_to = timed(lambda: ok(lib.pl_nchw_to_q4_f32(h, x.ptr, xq.ptr, n, c, hw)))
        t_res = timed(lambda: ok(lib.pl_add_f32(h, xq.ptr, rq.ptr, xq.ptr, xq.size)))
        t_relu = timed(lambda: ok(lib.pl_relu_f32(h, xq.ptr, xq.ptr, xq.size)))
        five = t_from + t_norm + t_mul + t_add + t_to
        rows.append({"x": [n, c, hh, ww], "groups": G, "cpg": c // G, "form": form,
                     "groupnorm_q4": move(t_gn, nbytes), "groupnorm_q4_res_relu": move(t_tail, nbytes + x.size * 4),
                     "instancenorm_q4_same_tensor": move(t_in, nbytes),
                     "nchw_route_us": {"from_q4": round(t_from * 1e6, 1), "instancenorm": round(t_norm * 1e6, 1),
                                       "mul": round(t_mul * 1e6, 1), "add": round(t_add * 1e6, 1), "to_q4": round(t_to * 1e6, 1),
                                       "five_kernels": round(five * 1e6, 1), "add_q4": round(t_res * 1e6, 1),
                                       "relu_q4": round(t_relu * 1e6, 1), "seven_kernels": round((five + t_res + t_relu) * 1e6, 1)},
                     "speedup_over_five_kernels": round(five / t_gn, 2),
                     "speedup_over_seven_kernels_with_tail": round((five + t_res + t_relu) / t_tail, 2)})
        del x, xq, rq, y
    print(json.dumps({"kernels": rows, "launch_floor_us": round(floor * 1e6, 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--check", type=int, default=1)
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=400, help="seconds one child may take")
    ap.add_argument("--want", default="")
    ap.add_argument("--child", choices=["arm", "kernels"])
    args = ap.parse_args()
    if args.child:
        return arm(args) if args.child == "arm" else kernels(args)
    passed = [a for a in sys.argv[1:]]
    tmp = tempfile.mkdtemp(prefix="gn_bench_")
    cache = os.environ.get("PLANER_HIP_TUNE_CACHE") or os.path.join(tmp, "tune.txt")
    want = []
    if args.check:
        gen, g, blob = build(args)
        from oracle import planer_np as onp
        ref = onp.OracleNet()
        ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
        ref.load_weights(blob)
        np.save(os.path.join(tmp, "want.npy"), ref(gen.make_input(args.batch, seed=1, size=args.size)[:args.check].copy()))
        want = ["--want", os.path.join(tmp, "want.npy")]

    def child(kind, switch, rnd):
        env = dict(os.environ, PLANER_HIP_GROUPNORM_Q4=switch, PLANER_HIP_TUNE_CACHE=cache)
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__)] + passed + want
        r = subprocess.run(cmd + ["--child", kind, "--round", str(rnd)], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("%s child, switch %s, round %d failed (exit %d):\n%s" % (kind, switch, rnd, r.returncode, r.stderr[-3000:]))
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    out = {"workload": "resnet18-gn", "batch": args.batch, "size": args.size, "groups": args.groups, "width": args.width,
           "dtype": "fp32", "steps": args.steps, "repeats": args.repeats, "rounds": args.rounds}
    out.update(child("kernels", "1", 0))
    print(json.dumps({"kernels": out["kernels"], "launch_floor_us": out["launch_floor_us"]}), flush=True)
    runs = {"1": [], "0": []}
    for rnd in range(args.rounds):
        for switch in ("1", "0"):
            line = child("arm", switch, rnd)
            runs[switch].append(line)
            print(json.dumps(line), flush=True)
    for switch, name in (("1", "groupnorm_q4"), ("0", "five_steps")):
        rates, calls = [r["pipelined_img_s"] for r in runs[switch]], [r["call_ms"] for r in runs[switch]]
        out[name] = {"pipelined_img_s": rates, "call_ms": calls, "median_img_s": sorted(rates)[len(rates) // 2],
                     "median_call_ms": sorted(calls)[len(calls) // 2], "img_s_spread": [min(rates), max(rates)],
                     "call_ms_spread": [min(calls), max(calls)], "steps": runs[switch][-1]["steps"],
                     "parity_rel_err": max(r["parity_rel_err"] or 0.0 for r in runs[switch])}
    out["pipelined_speedup"] = round(out["groupnorm_q4"]["median_img_s"] / out["five_steps"]["median_img_s"], 3)
    out["call_speedup"] = round(out["five_steps"]["median_call_ms"] / out["groupnorm_q4"]["median_call_ms"], 3)
    # the default follows the measurement: on only if the on arm beat the off arm in EVERY round, pipelined and per call
    out["keep_on"] = bool(all(a["pipelined_img_s"] > b["pipelined_img_s"] and a["call_ms"] < b["call_ms"]
                              for a, b in zip(runs["1"], runs["0"])))
    print(json.dumps(out))
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()

"""EDSR-baseline (planer_amd/irgen/edsr.py) at batch 8, 128x128 in, x4, fp32 on one GPU, with its pixel shuffles as one-pass
channel-quad steps (PLANER_HIP_PIXEL_SHUFFLE_Q4=1) and as reshape / transpose / reshape between two layout conversions (=0: the
program of a compiler without plan.fuse_pixel_shuffle), the two arms ALTERNATING --rounds times in one session so that the spread of
the repeats is visible next to the gain.  One JSON line per arm run, then one summary line.  Per arm run:
  pipelined_img_s   images/s on the pipelined feed / launch path bench.py times (median of --repeats regions of --steps steps)
  call_ms           milliseconds of net(x), one call at a time on one stream (device synchronise after each; median of --calls)
  parity_rel_err    max|y - oracle| / max|oracle| of the pipelined plan's output, first --check images
  steps             counts of pixelshuffle_q4 / pixelshuffle / to_q4 / from_q4 / transpose steps of the plan
and once (`kernels`), per distinct shuffle shape of the net: pl_pixel_shuffle_q4_f32's time as a shuffle, with nchw_out and as the
unshuffle back, and the three-kernel route it replaces (pl_q4_to_nchw_f32, the 6-D pl_transpose_f32, pl_nchw_to_q4_f32).  Bytes are one read of the input and one write of the
output; `launch_floor_us` is the same loop on a one-quad tensor, and a figure within 1.5x of it is marked `launch_bound` and given
no rate.
    python tools/sr_bench.py [--batch 8] [--size 128] [--scale 4] [--rounds 3] [--steps 10] [--warmup 3] [--repeats 5] [--calls 10]
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
COUNTED = ("pixelshuffle_q4", "pixelshuffle", "to_q4", "from_q4", "transpose", "reshape")


def build(args):
    sys.path.insert(0, HERE)
    from planer_amd.irgen import edsr
    g, blob = edsr.build(scale=args.scale, size=args.size, tail=args.tail, unshuffle_in=args.unshuffle_in)
    return edsr, g, blob


def arm(args):
    edsr, g, blob = build(args)
    import planer_amd
    xs_host = [edsr.make_input(args.batch, seed=1 + i, size=args.size) for i in range(2)]
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
    print(json.dumps({"pixel_shuffle_q4": os.environ.get("PLANER_HIP_PIXEL_SHUFFLE_Q4", "1"), "round": args.round,
                      "pipelined_img_s": round(rates[len(rates) // 2], 1), "pipelined_spread": [round(rates[0], 1), round(rates[-1], 1)],
                      "call_ms": round(1e3 * sorted(calls)[len(calls) // 2], 3), "parity_rel_err": parity,
                      "compile_s": round(compile_s, 2), "streams": getattr(plan, "streams", None), "steps": steps,
                      "pixel_shuffles_fused": net.pixel_shuffles_fused, "tune_source": net.tune_source()}))
    if parity is not None and not parity <= 1e-4:
        sys.exit("parity failure: %.3g" % parity)


def shuffle_shapes(g, blob):
    """The distinct (narrow C, r, wide H, wide W) of the graph's CRD shuffles, read from the first reshapes' shape constants."""
    out, pos = [], 0
    for name, shape, dt in g["inits"]:
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
        if name.endswith("_s6"):
            v = blob[pos:pos + nbytes].view(dt).tolist()
            if v[2] == v[3] and (v[1], v[2], v[4], v[5]) not in out:          # (0, C, r, r, H, W): a shuffle; unshuffles have r last
                out.append((v[1], v[2], v[4], v[5]))
        pos += nbytes
    return out


def kernels(args):
    """Device time per entry point.  Every timed closure is ONE C call on preallocated tensors, nothing allocated inside the
    loop, so a burst measures launches and kernels, not Python."""
    _, g, blob = build(args)
    import planer_amd
    from planer_amd import _lib, hip, q4
    ctx = hip.context()
    lib = _lib.load()
    h = ctx.handle
    rng = np.random.default_rng(5)
    n = args.batch

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

    tx, ty = hip.zeros((1, 4, 1, 1, 4), ctx=ctx), hip.zeros((1, 1, 2, 2, 4), ctx=ctx)
    floor = timed(lambda: ok(lib.pl_pixel_shuffle_q4_f32(h, tx.ptr, ty.ptr, 1, 4, 2, 2, 2, 0, 0, 0)))

    def move(t, nbytes):
        out = {"us": round(t * 1e6, 1), "bytes": nbytes, "launch_bound": bool(t < 1.5 * floor)}
        if not out["launch_bound"]:
            out.update(gb_s=round(nbytes / t / 1e9, 1), fraction_of_hbm_peak=round(nbytes / t / HBM_PEAK, 3))
        return out

    rows = []
    for c, r, hs, ws in shuffle_shapes(g, blob):
        x = planer_amd.asarray(rng.random((n, c * r * r, hs, ws), dtype=np.float32), ctx=ctx)
        xq = q4.to_q4(x)
        H, W = hs * r, ws * r
        yq = hip.empty((n, (c + 3) // 4, H, W, 4), ctx=ctx)
        y, xn = hip.empty((n, c, H, W), ctx=ctx), hip.empty(x.shape, ctx=ctx)
        nbytes = 2 * x.size * 4
        shp = (_lib.c_int * 6)(n, c, r, r, hs, ws)
        prm = (_lib.c_int * 6)(0, 1, 4, 2, 5, 3)
        t_reg = timed(lambda: ok(lib.pl_pixel_shuffle_q4_f32(h, xq.ptr, yq.ptr, n, c, H, W, r, 0, 0, 0)))
        t_nchw = timed(lambda: ok(lib.pl_pixel_shuffle_q4_f32(h, xq.ptr, y.ptr, n, c, H, W, r, 0, 0, 1)))
        t_inv = timed(lambda: ok(lib.pl_pixel_shuffle_q4_f32(h, yq.ptr, xq.ptr, n, c, H, W, r, 0, 1, 0)))
        t_from = timed(lambda: ok(lib.pl_q4_to_nchw_f32(h, xq.ptr, xn.ptr, n, c * r * r, hs * ws)))
        t_tr = timed(lambda: ok(lib.pl_transpose_f32(h, x.ptr, y.ptr, 6, shp, prm)))
        t_to = timed(lambda: ok(lib.pl_nchw_to_q4_f32(h, y.ptr, yq.ptr, n, c, H * W)))
        rows.append({"wide": [n, c * r * r, hs, ws], "narrow": [n, c, H, W], "r": r,
                     "pixel_shuffle_q4": move(t_reg, nbytes),
                     "nchw_out": move(t_nchw, nbytes), "unshuffle": move(t_inv, nbytes),
                     "nchw_route_us": {"from_q4": round(t_from * 1e6, 1), "transpose": round(t_tr * 1e6, 1), "to_q4": round(t_to * 1e6, 1),
                                       "three_kernels": round((t_from + t_tr + t_to) * 1e6, 1),
                                       "two_kernels_to_nchw": round((t_from + t_tr) * 1e6, 1)},
                     "speedup_over_three_kernels": round((t_from + t_tr + t_to) / t_reg, 2)})
        del x, xq, yq, y, xn
    print(json.dumps({"kernels": rows, "launch_floor_us": round(floor * 1e6, 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--tail", choices=["conv", "shuffle"], default="conv")
    ap.add_argument("--unshuffle-in", dest="unshuffle_in", action="store_true")
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
    tmp = tempfile.mkdtemp(prefix="sr_bench_")
    cache = os.environ.get("PLANER_HIP_TUNE_CACHE") or os.path.join(tmp, "tune.txt")
    want = []
    if args.check:
        edsr, g, blob = build(args)
        from oracle import planer_np as onp
        ref = onp.OracleNet()
        ref.load_json(g["input"], g["inits"], g["layers"], g["flow"])
        ref.load_weights(blob)
        np.save(os.path.join(tmp, "want.npy"), ref(edsr.make_input(args.batch, seed=1, size=args.size)[:args.check].copy()))
        want = ["--want", os.path.join(tmp, "want.npy")]

    def child(kind, switch, rnd):
        env = dict(os.environ, PLANER_HIP_PIXEL_SHUFFLE_Q4=switch, PLANER_HIP_TUNE_CACHE=cache)
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__)] + passed + want
        r = subprocess.run(cmd + ["--child", kind, "--round", str(rnd)], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("%s child, switch %s, round %d failed (exit %d):\n%s" % (kind, switch, rnd, r.returncode, r.stderr[-3000:]))
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    out = {"workload": "edsr-baseline", "batch": args.batch, "size": args.size, "scale": args.scale, "tail": args.tail,
           "unshuffle_in": args.unshuffle_in, "dtype": "fp32", "steps": args.steps, "repeats": args.repeats, "rounds": args.rounds}
    out.update(child("kernels", "1", 0))
    print(json.dumps({"kernels": out["kernels"], "launch_floor_us": out["launch_floor_us"]}), flush=True)
    runs = {"1": [], "0": []}
    for rnd in range(args.rounds):
        for switch in ("1", "0"):
            line = child("arm", switch, rnd)
            runs[switch].append(line)
            print(json.dumps(line), flush=True)
    for switch, name in (("1", "pixel_shuffle_q4"), ("0", "trio")):
        rates, calls = [r["pipelined_img_s"] for r in runs[switch]], [r["call_ms"] for r in runs[switch]]
        out[name] = {"pipelined_img_s": rates, "call_ms": calls, "median_img_s": sorted(rates)[len(rates) // 2],
                     "median_call_ms": sorted(calls)[len(calls) // 2], "img_s_spread": [min(rates), max(rates)],
                     "call_ms_spread": [min(calls), max(calls)], "steps": runs[switch][-1]["steps"],
                     "parity_rel_err": max(r["parity_rel_err"] or 0.0 for r in runs[switch])}
    out["pipelined_speedup"] = round(out["pixel_shuffle_q4"]["median_img_s"] / out["trio"]["median_img_s"], 3)
    out["call_speedup"] = round(out["trio"]["median_call_ms"] / out["pixel_shuffle_q4"]["median_call_ms"], 3)
    # the default follows the measurement: on only if the on arm beat the off arm in EVERY round
    out["keep_on"] = bool(all(a["pipelined_img_s"] > b["pipelined_img_s"] for a, b in zip(runs["1"], runs["0"])))
    print(json.dumps(out))
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()

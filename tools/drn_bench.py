"""The dilated ResNet-18 (planer_amd/irgen/drn.py) at batch 32, 224x224, fp32 on one GPU, with its dilated convs folded by pixel
phase where that measures faster (PLANER_HIP_DILATED_FOLD=1) and as they are (=0: the direct channel-quad kernel), the two arms
ALTERNATING --rounds times in one session so that the spread of the repeats is visible next to the gain.  One JSON line per arm
run, then one summary line.  Per arm run:
  pipelined_img_s   images/s on the pipelined feed / launch path bench.py times (median of --repeats regions of --steps steps)
  call_ms           milliseconds of net(x), one call at a time on one stream (device synchronise after each; median of --calls)
  parity_rel_err    max|y - oracle| / max|oracle| of the pipelined plan's output, first --check images
  convs             per conv step: layer, kernel family, input shape as the kernel sees it, fold (null: not folded)
  dilated_folds / refolds   heads folded and refold_q4 steps of the plan
and once (`kernels`), per dilated conv shape of the net: the direct kernel at the conv's own shape, the picked candidate at the
folded shape, each refold's time and bytes (one read + one write) and the fraction of the 8 TB/s HBM peak that is, next to
pl_nchw_to_q4_f32 on the same bytes; and the 2 -> 4 refold of layer4.0.
    python tools/drn_bench.py [--batch 32] [--size 224] [--rounds 3] [--steps 20] [--warmup 5] [--repeats 5] [--calls 10]
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


def arm(args):
    sys.path.insert(0, HERE)
    from oracle import planer_np as onp
    from planer_amd.irgen import drn
    import planer_amd
    g, blob = drn.build()
    xs_host = [drn.make_input(args.batch, seed=1 + i, size=args.size) for i in range(2)]
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
    folds, refolds = net.dilated_folds, net.refolds
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
    convs = [{"layer": a["layer"], "algo": a["algo"].split(" (")[0], "x": a["x"], "fold": a.get("fold")} for a in plan.algos]
    print(json.dumps({"dilated_fold": os.environ.get("PLANER_HIP_DILATED_FOLD", "0"), "round": args.round,
                      "pipelined_img_s": round(rates[len(rates) // 2], 1), "pipelined_spread": [round(rates[0], 1), round(rates[-1], 1)],
                      "call_ms": round(1e3 * sorted(calls)[len(calls) // 2], 3), "parity_rel_err": parity,
                      "compile_s": round(compile_s, 2), "streams": getattr(plan, "streams", None),
                      "dilated_folds": folds, "refolds": refolds, "tune_source": net.tune_source(), "convs": convs}))
    if parity is not None and not parity <= 1e-4:
        sys.exit("parity failure: %.3g" % parity)


def kernels(args):
    sys.path.insert(0, HERE)
    import planer_amd
    from planer_amd import hip, q4
    from planer_amd.conv_layouts import DIRECT_Q4, LAYOUTS, candidates
    from planer_amd.net import Net
    ctx = hip.context()
    rng = np.random.default_rng(5)
    n, m = args.batch, args.size // 8

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

    def move(t, nbytes):
        return {"us": round(t * 1e6, 1), "bytes": 2 * nbytes, "gb_s": round(2 * nbytes / t / 1e9, 1),
                "fraction_of_hbm_peak": round(2 * nbytes / t / HBM_PEAK, 3)}
    picker = Net(ctx=ctx)                      # (only its algorithm picker and caches are used)
    rows = []
    for cin, cout, d in ((256, 256, 2), (256, 512, 2), (512, 512, 4)):
        xs, ks = (n, cin, m, m), (cout, cin, 3, 3)
        x = planer_amd.asarray(rng.standard_normal(xs).astype(np.float32), ctx=ctx)
        K = planer_amd.asarray((rng.standard_normal(ks) * 0.05).astype(np.float32), ctx=ctx)
        geo = dict(group=1, strides=[1, 1], dilations=[d, d], pads=[d] * 4)
        one = dict(geo, dilations=[1, 1], pads=[1, 1, 1, 1])
        fxs = q4.folded_shape(xs, d, d)
        lay = picker._pick_conv_algo(candidates(True, ks, one, fxs), K, ["~probe", "~k"], one, {"~probe": fxs}, q4=True)
        xq = q4.to_q4(x)
        xf = q4.refold_q4(xq, d, d)
        Kd, Kf = LAYOUTS[DIRECT_Q4].prepare(K, **geo), LAYOUTS[lay].prepare(K, **one)
        t_direct = timed(lambda: q4.ConvQ4(xq, Kd, w_layout=DIRECT_Q4, **geo))
        plan_direct = ctx.last_conv_plan()
        t_folded = timed(lambda: q4.ConvQ4(xf, Kf, w_layout=lay, **one))
        yf = q4.ConvQ4(xf, Kf, w_layout=lay, **one)
        t_in, t_out = timed(lambda: q4.refold_q4(xq, d, d)), timed(lambda: q4.refold_q4(yf, 1, 1))
        t_conv = timed(lambda: q4.to_q4(x))
        verdict = picker._fold_worth(xs, ks, geo)
        rows.append({"x": list(xs), "k": list(ks), "dilation": d, "folded_x": list(fxs),
                     "direct_us": round(t_direct * 1e6, 1), "direct_plan": plan_direct,
                     "folded_us": round(t_folded * 1e6, 1), "folded_algo": LAYOUTS[lay].name.split(" (")[0],
                     "refold_in": move(t_in, x.size * 4), "refold_out": move(t_out, yf.size * 4),
                     "nchw_to_q4_same_bytes": move(t_conv, x.size * 4),
                     "folded_with_both_refolds_us": round((t_folded + t_in + t_out) * 1e6, 1), "worth": bool(verdict)})
    x = q4.refold_q4(q4.to_q4(planer_amd.asarray(rng.standard_normal((n, 512, m, m)).astype(np.float32), ctx=ctx)), 2, 2)
    rows.append({"x": [n, 512, m, m], "refold_2_to_4": move(timed(lambda: q4.refold_q4(x, 4, 4)), x.size * 4)})
    picker.save_algo_cache()                   # the arms take these picks and verdicts instead of measuring again
    print(json.dumps({"kernels": rows}))


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
    ap.add_argument("--child", choices=["arm", "kernels"])
    args = ap.parse_args()
    if args.child:
        return arm(args) if args.child == "arm" else kernels(args)
    passed = [a for a in sys.argv[1:]]
    tmp = None
    cache = os.environ.get("PLANER_HIP_TUNE_CACHE")
    if not cache:
        tmp = tempfile.mkdtemp(prefix="drn_bench_")
        cache = os.path.join(tmp, "tune.txt")

    def child(kind, switch, rnd):
        env = dict(os.environ, PLANER_HIP_DILATED_FOLD=switch, PLANER_HIP_TUNE_CACHE=cache)
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + passed + ["--child", kind, "--round", str(rnd)], env=env,
                           capture_output=True, text=True, timeout=1100)
        if r.returncode != 0:
            sys.exit("%s child, switch %s, round %d failed (exit %d):\n%s" % (kind, switch, rnd, r.returncode, r.stderr[-3000:]))
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    out = {"workload": "drn18", "batch": args.batch, "size": args.size, "dtype": "fp32", "steps": args.steps, "repeats": args.repeats,
           "rounds": args.rounds, "kernels": child("kernels", "1", 0)["kernels"]}
    print(json.dumps({"kernels": out["kernels"]}), flush=True)
    runs = {"1": [], "0": []}
    for rnd in range(args.rounds):
        for switch in ("1", "0"):
            line = child("arm", switch, rnd)
            runs[switch].append(line)
            print(json.dumps(line), flush=True)
    for switch, name in (("1", "fold"), ("0", "direct")):
        rates, calls = [r["pipelined_img_s"] for r in runs[switch]], [r["call_ms"] for r in runs[switch]]
        out[name] = {"pipelined_img_s": rates, "call_ms": calls, "median_img_s": sorted(rates)[len(rates) // 2],
                     "median_call_ms": sorted(calls)[len(calls) // 2], "dilated_folds": runs[switch][-1]["dilated_folds"],
                     "refolds": runs[switch][-1]["refolds"], "parity_rel_err": max(r["parity_rel_err"] or 0.0 for r in runs[switch])}
    out["pipelined_speedup"] = round(out["fold"]["median_img_s"] / out["direct"]["median_img_s"], 3)
    out["call_speedup"] = round(out["direct"]["median_call_ms"] / out["fold"]["median_call_ms"], 3)
    print(json.dumps(out))
    if tmp:
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()

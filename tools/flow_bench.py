"""What a caller who wants INSTANCE MASKS back gets from a flow-following cell net, fp32 on one GPU.
  cell-masks       irgen/cellnet.py (U-Net, 3 planes), batch 32, 224 x 224, host uint8 in (Net.image_input), Net.flow_output:
                   masks, num, instances, centres come back                                      (pl_flow_instances_f32)
  cell-planes      the same net without the declaration: the three float planes come back
  cell-planes-host the same, then per image the host mirror of the rule (numpy pointer jumping, bincount, scipy.ndimage.label,
                   bincount, look-up; tests/flow_ref.py's labelling where scipy is absent: the line says which) in the loop
  scan-masks       Net.tiled on a --scan x --scan uint8 scan (default 4096), window 512, margin 0.1, with flow_output
  scan-planes-host Net.tiled's float blend, then the host mirror on the whole map
Every arm run is a FRESH process under a timeout of its own; the arms alternate --rounds times and share one tuning cache.  Then
the chain alone (one more process): HIP events around --launches calls of pl_flow_instances_f32 on a batch of 32 maps of 224 x 224
and on one scan-sized map of noisy discs -- with rounds = 10 and 0, without the table, and
beside the label-map path of DESIGN 4.26 on the same shapes.  (With rounds = 0 nothing has converged and most of the foreground is
a sink, so that figure is a different workload, not the chain minus its rounds.)  With --trace one more process runs the chain
TRACE_CALLS times per map under rocprofv3 --kernel-trace, and the median device time of each kernel of the chain is reported
per map: which launch dominates.
One JSON line per step as it ends, then one summary line.  The tool stops at the first step that fails.
    python tools/flow_bench.py [--rounds 3] [--passes 20] [--arms ...] [--no-kernels] [--trace]
The parent process never opens the GPU."""
import argparse
import collections
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
ARMS = ["cell-masks", "cell-planes", "cell-planes-host", "scan-masks", "scan-planes-host"]
WINDOW, MARGIN = 512, 0.1
TRACE_CALLS = 12
SPEC = dict(level=0.0, min_flow=0.0, rounds=10, min_size=15, max_instances=256)

try:
    from scipy import ndimage
    HOST_STEP = "numpy + scipy.ndimage %s" % __import__("scipy").__version__
except ImportError:
    ndimage = None
    HOST_STEP = "numpy stand-in (tests/flow_ref.py)"


def host_masks(planes):
    """The rule on the host for float32 (N, 3, H, W): the masks a caller would compute.  -> number of instances."""
    from tests import flow_ref
    total = 0
    for dy, dx, prob in planes:
        if ndimage is None:
            total += flow_ref.follow_plane(dy, dx, prob, SPEC["level"], SPEC["min_flow"], SPEC["rounds"], SPEC["min_size"])[1]
            continue
        h, w = prob.shape
        end, fg = flow_ref.step_ref(dy, dx, prob, SPEC["level"], SPEC["min_flow"])
        for _ in range(SPEC["rounds"]):
            end = end[end]
        cnt = np.bincount(end[fg], minlength=h * w)
        S, raw = ndimage.label((cnt > 0).reshape(h, w), structure=np.ones((3, 3)))
        inst = np.where(fg, S.ravel()[end], 0)
        keep = np.bincount(inst[fg], minlength=raw + 1)[1:] >= SPEC["min_size"]
        new = np.concatenate([[0], np.where(keep, np.cumsum(keep), 0)])
        new[inst].astype(np.int32).reshape(h, w)
        total += int(keep.sum())
    return total


def arm_child(args):
    import planer_amd
    from planer_amd.irgen import cellnet
    what, how = args.arm.split("-", 1)
    rng = np.random.default_rng(3)
    g, blob = cellnet.build()
    net = planer_amd.from_graph(g, blob)
    net.image_input(*planer_amd.util.image_affine(MEAN, STD))
    if how == "masks":
        net.flow_output(planes=cellnet.PLANES, **SPEC)
    line = {"arm": args.arm, "round": args.round, "host_step": HOST_STEP if how == "planes-host" else None}
    if what == "scan":
        img = rng.integers(0, 256, (args.scan, args.scan, 3), dtype=np.uint8)
        tile = dict(window=WINDOW, margin=MARGIN, batch=args.batch)
        t0 = time.perf_counter()
        got = net.tiled(img, **tile)
        line["compile_and_warm_s"] = round(time.perf_counter() - t0, 2)
        ts = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            got = net.tiled(img, **tile)
            ts.append(time.perf_counter() - t0)
        line["tiled_ms"] = round(sorted(ts)[len(ts) // 2] * 1e3, 2)
        if how == "planes-host":
            t0 = time.perf_counter()
            line["instances"] = host_masks(np.ascontiguousarray(got.transpose(2, 0, 1))[None])
            line["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            line["tiled_ms_host_step_included"] = round(line["tiled_ms"] + line["host_ms"], 1)
        else:
            line["instances"] = int(got[1][0])
    else:
        n = 32
        batches = [rng.integers(0, 256, (n, 224, 224, 3), dtype=np.uint8) for _ in range(2)]
        window, pend = 8, collections.deque()

        def host_loop(count, finish=None):
            got = None
            for i in range(count):
                pend.append(net.submit(batches[i & 1]))
                if len(pend) > window:
                    got = pend.popleft().get()
                    finish and finish(got)
            while pend:
                got = pend.popleft().get()
                finish and finish(got)
            return got
        t0 = time.perf_counter()
        host_loop(10)
        line["compile_and_warm_s"] = round(time.perf_counter() - t0, 2)
        line["tune_source"] = net.tune_source()
        host_loop(10)
        t0 = time.perf_counter()
        got = host_loop(args.passes)
        line["img_s"] = round(n * args.passes / (time.perf_counter() - t0), 1)
        seq = got if isinstance(got, tuple) else (got,)
        line["output_bytes_per_batch"] = int(sum(a.nbytes for a in seq))
        if how == "planes-host":
            t0 = time.perf_counter()
            line["instances_per_batch"] = host_masks(got)
            line["host_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3, 1)
            t0 = time.perf_counter()
            host_loop(args.host_passes, host_masks)
            line["img_s_host_step_included"] = round(n * args.host_passes / (time.perf_counter() - t0), 1)
        elif how == "masks":
            line["instances_per_batch"] = int(got[1].sum())
    ctx = planer_amd.hip.context()
    if ctx.tune_cache:
        ctx.save_tune_cache()
    print(json.dumps(line), flush=True)


def bench_maps(args):
    from tests import flow_ref
    s = args.scan
    return [("batch 32 x 224 x 224, noisy discs", flow_ref.discs(32, 224, 224, 1, 0.5, 24, 9)[0], args.launches),
            ("scan %d x %d, noisy discs" % (s, s), flow_ref.discs(1, s, s, 2, 0.5, 24, 9)[0], max(args.launches // 5, 3))]


def trace_child(args):
    """The chain alone, TRACE_CALLS times per map, for the kernel trace: nothing else touches the GPU in this process."""
    from planer_amd import hip, util
    ctx = hip.context()
    spec = util.FlowSpec(**SPEC)
    for _, host, _ in bench_maps(args):
        x = hip.asarray(host)
        for _ in range(TRACE_CALLS):
            spec.encode(x)
        ctx.synchronize()


def trace_digest(directory, names):
    """Per map: the median over the chains of each kernel's device time in us (the launches of one kernel inside a chain summed),
    from a rocprofv3 kernel trace of trace_child.  A chain begins with step_kernel."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if "flow::" in r["Kernel_Name"] or "components::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    chains = []
    for r in rows:
        space, name = ("flow", r["Kernel_Name"].split("flow::")[1]) if "flow::" in r["Kernel_Name"] else \
            ("components", r["Kernel_Name"].split("components::")[1])
        name = name.split("(")[0].split("<")[0]
        if space == "flow" and name == "step_kernel":
            chains.append(collections.OrderedDict())
        if chains:
            key = "%s::%s" % (space, name)
            chains[-1][key] = chains[-1].get(key, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    out = collections.OrderedDict()
    for i, name in enumerate(names):
        mine = chains[i * TRACE_CALLS + 2:(i + 1) * TRACE_CALLS]          # (the first two of a map warm the caches)
        per = collections.OrderedDict()
        for c in mine:
            for k, us in c.items():
                per.setdefault(k, []).append(us)
        out[name] = {k: round(sorted(v)[len(v) // 2], 2) for k, v in per.items()}
        out[name]["sum"] = round(sum(out[name].values()), 2)
    out["chains_in_trace"], out["chains_expected"] = len(chains), len(names) * TRACE_CALLS
    return out


def kernels_child(args):
    from planer_amd import _lib, hip, util
    ctx = hip.context()

    def timed(fn, launches):
        for _ in range(3):
            fn()
        best = None
        for _ in range(3):
            e0 = hip.Event(ctx).record()
            for _ in range(launches):
                fn()
            e1 = hip.Event(ctx).record()
            t = e0.elapsed_ms(e1) / launches * 1e-3
            best = t if best is None else min(best, t)
        return best

    def chain(x, rounds, max_instances):
        """The entry point itself into fixed arrays: no allocation between the events."""
        n, c, h, w = x.shape
        masks, num = hip.empty((n, h, w), np.int32, ctx=ctx), hip.empty((n,), np.int32, ctx=ctx)
        table, centres = hip.empty((n, max_instances, 5), np.int32, ctx=ctx), hip.empty((n, max_instances, 2), np.float32, ctx=ctx)
        scratch = hip.empty((util._flow_scratch_bytes(n, h, w, max_instances) // 8 + 1,), np.int64, ctx=ctx)
        fn = lambda: _lib.call("pl_flow_instances_f32", ctx.handle, x.ptr, n, h, w, c * h * w, 1, 0, h * w, 2 * h * w, 0.0, 0.0, rounds,     # noqa: E731
                               15, max_instances, scratch.ptr, masks.ptr, num.ptr, table.ptr if max_instances else None,
                               centres.ptr if max_instances else None)
        return fn, num, (masks, table, centres, scratch)

    def objects(x):
        spec = util.ObjectSpec(0.0, 8, 0, 256)
        return lambda: spec.encode(x)
    for name, host, launches in bench_maps(args):
        x = hip.asarray(host)
        n, _, h, w = host.shape
        line = {"kernel": "pl_flow_instances_f32", "map": name, "shape": list(host.shape)}
        for key, rounds, m in (("us", 10, 256), ("us_rounds_0", 0, 256), ("us_no_table", 10, 0)):
            fn, num, keep = chain(x, rounds, m)
            line[key] = round(timed(fn, launches) * 1e6, 2)
            if key == "us":
                line["instances"] = int(num.get().sum())
            del keep
        line["pointer_round_bytes"] = 8 * n * h * w
        line["ns_per_pixel"] = round(line["us"] * 1e3 / (n * h * w), 4)
        # the label-map path of DESIGN 4.26 on the same planes (plane 2 thresholded, 8-connected components, 256 rows); its
        # arrays come from the pool, which the chain's timing above does not pay
        line["object_path_us"] = round(timed(objects(hip.asarray(np.ascontiguousarray(host[:, 2:3]))), launches) * 1e6, 2)
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=20, help="submits per timed loop")
    ap.add_argument("--host-passes", type=int, default=2, help="submits of the loop that includes the caller's host step")
    ap.add_argument("--calls", type=int, default=3, help="net.tiled calls timed")
    ap.add_argument("--launches", type=int, default=50, help="calls between the two events of a chain timing")
    ap.add_argument("--scan", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=9, help="windows per pass of Net.tiled")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--trace", action="store_true", help="the chain alone once more under rocprofv3 --kernel-trace")
    ap.add_argument("--cache", default=None, help="tuning cache file every process loads and saves")
    ap.add_argument("--timeout", type=int, default=300, help="seconds one child process may take")
    ap.add_argument("--child", choices=["arm", "kernels", "trace"])
    ap.add_argument("--arm")
    ap.add_argument("--round", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return {"arm": arm_child, "kernels": kernels_child, "trace": trace_child}[args.child](args)
    tmp = tempfile.TemporaryDirectory()
    if args.cache is None:
        args.cache = os.path.join(tmp.name, "tune.json")
    env = dict(os.environ, PLANER_HIP_TUNE_CACHE=os.path.abspath(args.cache))
    common = ["--passes", str(args.passes), "--host-passes", str(args.host_passes), "--calls", str(args.calls),
              "--launches", str(args.launches), "--scan", str(args.scan), "--batch", str(args.batch)]

    def step(extra, wrap=()):
        cmd = ["timeout", "-k", "10", str(args.timeout)] + list(wrap) + [sys.executable, os.path.abspath(__file__)] + extra + common
        r = subprocess.run(cmd, capture_output=True, text=True, env=env)
        if r.returncode != 0:                          # the first failing step ends the run: nothing more is started
            sys.exit("step %s failed (exit %d):\n%s\n%s" % (" ".join(extra), r.returncode, r.stdout[-2000:], r.stderr[-3000:]))
        lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        for ln in lines:
            print(json.dumps(ln), flush=True)
        return lines
    arms = [a for a in args.arms.split(",") if a]
    kernels = [] if args.no_kernels else step(["--child", "kernels"])
    runs = []
    for rnd in range(args.rounds):
        for arm in arms:
            runs += step(["--child", "arm", "--arm", arm, "--round", str(rnd)])
    out = {"dtype": "fp32", "rounds": args.rounds, "passes": args.passes, "arms": {}, "kernels": kernels}
    if args.trace:
        d = os.path.join(tmp.name, "trace")
        step(["--child", "trace"], wrap=["rocprofv3", "--kernel-trace", "-d", d, "-o", "flow", "--output-format", "csv", "--"])
        out["trace"] = trace_digest(d, ["batch 32 x 224 x 224", "scan %d x %d" % (args.scan, args.scan)])
    med = lambda v: sorted(v)[len(v) // 2] if v else None        # noqa: E731
    for arm in arms:
        mine = [r for r in runs if r["arm"] == arm]
        keys = [k for k, v in mine[0].items() if isinstance(v, (int, float)) and k != "round"]
        out["arms"][arm] = {"median_" + k: med([r[k] for r in mine]) for k in keys}
        out["arms"][arm]["host_step"] = mine[0].get("host_step")
    print(json.dumps(out))
    tmp.cleanup()


if __name__ == "__main__":
    main()

"""What a caller who wants OBJECTS back gets from a segmentation net, fp32 on one GPU.
  fpn-objects      FPN, batch 32, 224 x 224, 21 classes, host uint8 in (Net.image_input), Net.object_output: labels, num,
                   objects, centroids come back                                     (pl_labels_f32_u8 + pl_components_u8_i32)
  fpn-labels-host  the same net with Net.label_output, then per image and class scipy.ndimage.label / find_objects / coordinate
                   sums on the host (a numpy stand-in where scipy is absent: the line says which) -- timed alone and in the loop
  fpn-labels       Net.label_output alone: what the pass costs without any of it
  scan-objects     Net.tiled on a --scan x --scan uint8 scan (default 4096), window 512, margin 0.1, with object_output
  scan-labels-host Net.tiled with label_output, then the host step on the whole map
Every arm run is a FRESH process under a timeout of its own; the arms alternate --rounds times and share one tuning cache.  Then
the chain alone (one more process): HIP events around --launches launches of the label kernel and of pl_components_u8_i32 on
the batch's label map and on scan-sized maps -- random objects, one object that fills the map, a serpentine -- beside a one-tile
call (the launch floors).  With --trace that process runs once more under rocprofv3 --kernel-trace and the median device time of
each kernel of the chain is reported per map.
One JSON line per step as it ends, then one summary line.  The tool stops at the first step that fails.
    python tools/object_bench.py [--rounds 3] [--passes 60] [--arms ...] [--no-kernels] [--trace]
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
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
ARMS = ["fpn-objects", "fpn-labels-host", "fpn-labels", "scan-objects", "scan-labels-host"]
WINDOW, MARGIN, MAX_OBJECTS = 512, 0.1, 256

try:
    from scipy import ndimage
    HOST_STEP = "scipy.ndimage %s" % __import__("scipy").__version__
except ImportError:
    ndimage = None
    HOST_STEP = "numpy stand-in (tests/components_ref.py)"


def host_objects(maps):
    """Per image: every class but 0 labelled 8-connected, boxes and centroids of its objects.  -> number of objects."""
    total = 0
    for m in maps:
        if ndimage is None:
            sys.path.insert(0, HERE)
            from tests import components_ref
            labels, num = components_ref.label_ref(m, 8, 0)
            components_ref.regions_ref(m[None], labels[None], MAX_OBJECTS)
            total += int(num)
            continue
        for c in np.unique(m):
            if c == 0:
                continue
            labels, num = ndimage.label(m == c, structure=np.ones((3, 3)))
            ndimage.find_objects(labels)
            idx = np.arange(1, num + 1)
            ys, xs = np.indices(m.shape, sparse=True)
            area = ndimage.sum_labels(np.ones(m.shape), labels, idx)
            ndimage.sum_labels(np.broadcast_to(ys, m.shape), labels, idx) / area
            ndimage.sum_labels(np.broadcast_to(xs, m.shape), labels, idx) / area
            total += num
    return total


def arm_child(args):
    sys.path.insert(0, HERE)
    import planer_amd
    from planer_amd.irgen import fpn
    what, how = args.arm.split("-", 1)
    rng = np.random.default_rng(3)
    g, blob = fpn.build()
    net = planer_amd.from_graph(g, blob)
    net.image_input(*planer_amd.util.image_affine(MEAN, STD))
    if how == "objects":
        net.object_output(max_objects=MAX_OBJECTS)
    else:
        net.label_output()
    line = {"arm": args.arm, "round": args.round, "host_step": HOST_STEP if how == "labels-host" else None}
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
        if how == "labels-host":
            t0 = time.perf_counter()
            line["objects"] = host_objects(got[None])
            line["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            line["tiled_ms_host_step_included"] = round(line["tiled_ms"] + line["host_ms"], 1)
        else:
            line["objects"] = int(got[1][0])
    else:
        n = 32
        batches = [rng.integers(0, 256, (n, 224, 224, 3), dtype=np.uint8) for _ in range(2)]
        window, pend = 12, collections.deque()

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
        host_loop(20)
        line["compile_and_warm_s"] = round(time.perf_counter() - t0, 2)
        line["tune_source"] = net.tune_source()
        host_loop(20)
        t0 = time.perf_counter()
        got = host_loop(args.passes)
        line["img_s"] = round(n * args.passes / (time.perf_counter() - t0), 1)
        seq = got if isinstance(got, tuple) else (got,)
        line["output_bytes_per_batch"] = int(sum(a.nbytes for a in seq))
        for i in range(3):
            net(batches[i & 1])
        ts = []
        for i in range(args.calls):
            t0 = time.perf_counter()
            got = net(batches[i & 1])
            ts.append(time.perf_counter() - t0)
        line["net_call_ms"] = round(sorted(ts)[len(ts) // 2] * 1e3, 3)
        if how == "labels-host":
            t0 = time.perf_counter()
            line["objects_per_batch"] = host_objects(got)
            line["host_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3, 1)
            t0 = time.perf_counter()
            host_loop(args.host_passes, host_objects)
            line["img_s_host_step_included"] = round(n * args.host_passes / (time.perf_counter() - t0), 1)
        elif how == "objects":
            line["objects_per_batch"] = int(got[1].sum())
    ctx = planer_amd.hip.context()
    if ctx.tune_cache:
        ctx.save_tune_cache()
    print(json.dumps(line), flush=True)


def kernels_child(args):
    sys.path.insert(0, HERE)
    from planer_amd import _lib, hip, util
    from tests import components_ref
    ctx = hip.context()
    rng = np.random.default_rng(4)

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

    def chain(m, max_objects=MAX_OBJECTS):
        """The entry point itself into fixed arrays: no allocation between the events."""
        n, h, w = m.shape
        labels, num = hip.empty((n, h, w), np.int32, ctx=ctx), hip.empty((n,), np.int32, ctx=ctx)
        objects, centroids = hip.empty((n, max_objects, 6), np.int32, ctx=ctx), hip.empty((n, max_objects, 2), np.float32, ctx=ctx)
        scratch = hip.empty((util._cc_scratch_bytes(n, h, w, max_objects) // 8 + 1,), np.int64, ctx=ctx)
        fn = lambda: _lib.call("pl_components_u8_i32", ctx.handle, m.ptr, n, h, w, 8, 0, max_objects, scratch.ptr, labels.ptr,      # noqa: E731
                               num.ptr, objects.ptr, centroids.ptr)
        return fn, num
    floor = timed(chain(hip.asarray(np.ones((1, 4, 4), np.uint8)))[0], args.launches)
    x = hip.asarray(rng.standard_normal((32, 21, 224, 224)).astype(np.float32))
    # argmax of smooth scores: objects of a segmentation net's size rather than salt and pepper
    smooth = np.repeat(np.repeat(rng.standard_normal((32, 21, 14, 14)), 16, 2), 16, 3).astype(np.float32)
    y = hip.empty((32, 224, 224), np.uint8, ctx=ctx)
    label_fn = lambda: _lib.call("pl_labels_f32_u8", ctx.handle, x.ptr, y.ptr, 32, 21, 224, 224, 0.0)      # noqa: E731
    print(json.dumps({"kernel": "pl_labels_f32_u8", "shape": [32, 21, 224, 224], "us": round(timed(label_fn, args.launches) * 1e6, 2)}), flush=True)
    s = args.scan
    blobs = (np.repeat(np.repeat(rng.random((1, s // 32, s // 32)), 32, 1), 32, 2) < 0.45).astype(np.uint8)
    maps = [("batch, argmax of noise", util.label_map(x).get()), ("batch, argmax of smooth scores", smooth.argmax(1).astype(np.uint8)),
            ("scan, random pixels 0.5", components_ref.random_binary(1, s, s, 0.5, 1)), ("scan, random blobs", blobs),
            ("scan, one object", np.ones((1, s, s), np.uint8)), ("scan, serpentine", components_ref.serpentine(1, s, s)),
            ("scan, all background", np.zeros((1, s, s), np.uint8))]
    for name, m in maps:
        fn, num = chain(hip.asarray(m))
        t = timed(fn, (chain_calls(name, args.launches) - 3) // 3)
        print(json.dumps({"kernel": "pl_components_u8_i32", "map": name, "shape": list(m.shape), "us": round(t * 1e6, 2),
                          "objects": int(num.get().sum()), "launch_floor_us": round(floor * 1e6, 2),
                          "ns_per_pixel": round(t * 1e9 / m.size, 4)}), flush=True)


def chain_calls(name, launches):
    """Calls of the chain the kernels step makes for one map: 3 to warm up, then 3 timings."""
    return 3 + 3 * (launches if "batch" in name or "tile" in name else max(launches // 10, 3))


def trace_digest(directory, kernels, launches):
    """Median device time in us of each kernel of the chain, per map, from a rocprofv3 kernel trace of the kernels step: the
    chains in launch order (each begins with tile_kernel), dealt out to the maps by the number of calls the step makes."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if "components::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    chains = []
    for r in rows:
        name = r["Kernel_Name"].split("components::")[1].split("(")[0]
        if name == "tile_kernel":
            chains.append([])
        chains[-1].append((name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    out, at = collections.OrderedDict(), 0
    for name in ["one tile"] + [k["map"] for k in kernels if "map" in k]:
        mine, at = chains[at:at + chain_calls(name, launches)], at + chain_calls(name, launches)
        per = collections.OrderedDict()
        for c in mine:
            for kernel, us in c:
                per.setdefault(kernel, []).append(us)
        out[name] = {k: round(sorted(v)[len(v) // 2], 2) for k, v in per.items()}
        out[name]["sum"] = round(sum(out[name].values()), 2)
    out["chains_in_trace"], out["chains_expected"] = len(chains), at
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=60, help="submits per timed loop")
    ap.add_argument("--host-passes", type=int, default=3, help="submits of the loop that includes the caller's host step")
    ap.add_argument("--calls", type=int, default=7, help="net(x) / net.tiled calls timed")
    ap.add_argument("--launches", type=int, default=50, help="launches between the two events of a kernel timing")
    ap.add_argument("--scan", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=9, help="windows per pass of Net.tiled")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--trace", action="store_true", help="the kernels step once more under rocprofv3 --kernel-trace")
    ap.add_argument("--cache", default=None, help="tuning cache file every process loads and saves")
    ap.add_argument("--timeout", type=int, default=300, help="seconds one child process may take")
    ap.add_argument("--child", choices=["arm", "kernels"])
    ap.add_argument("--arm")
    ap.add_argument("--round", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return arm_child(args) if args.child == "arm" else kernels_child(args)
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
    runs = []
    for rnd in range(args.rounds):
        for arm in arms:
            runs += step(["--child", "arm", "--arm", arm, "--round", str(rnd)])
    kernels = [] if args.no_kernels else step(["--child", "kernels"])
    out = {"dtype": "fp32", "rounds": args.rounds, "passes": args.passes, "arms": {}, "kernels": kernels}
    if args.trace:
        d = os.path.join(tmp.name, "trace")
        step(["--child", "kernels"], wrap=["rocprofv3", "--kernel-trace", "-d", d, "-o", "cc", "--output-format", "csv", "--"])
        out["trace"] = trace_digest(d, kernels, args.launches)
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

"""What a caller who wants POINTS back gets from a heat-map net, fp32 on one GPU.
  pose-keypoints   the pose net of irgen/posenet.py, batch 32, 256 x 192, 17 joints, host uint8 in (Net.image_input),
                   Net.keypoint_output: peaks and num come back                                               (pl_peaks_f32)
  pose-maps-host   the same net handing back its float32 heat maps (32, 17, 64, 48), then per plane maximum_filter(h, 3) == h,
                   threshold, sort, keep the best, quarter-pixel nudge, scale on the host (scipy's filter, or the numpy shifts of
                   tests/peaks_ref.py where scipy is absent: the line says which) -- timed alone and in the loop
  pose-maps        the float32 heat maps alone: what the pass costs with the download and without any of it
Every arm run is a FRESH process under a timeout of its own; the arms alternate --rounds times and share one tuning cache.  Then
the chain alone (one more process): HIP events around --launches launches of pl_peaks_f32 on a batch-sized tensor and on one
large map of several hundred tiles -- random values, a constant plane under ties="all", everything below the threshold -- beside
a one-tile call (the launch floor) and a device-to-device copy of the large map (the copy rate the tile pass is held against).
With --trace that process runs once more under rocprofv3 --kernel-trace and the median device time of each of the two kernels
is reported per input, the tile pass also as bytes read per second and as a fraction of the copy rate.
One JSON line per step as it ends, then one summary line.  The tool stops at the first step that fails.
    python tools/keypoint_bench.py [--rounds 3] [--passes 60] [--arms ...] [--no-kernels] [--trace]
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
ARMS = ["pose-keypoints", "pose-maps-host", "pose-maps"]
SPEC = dict(threshold=0.0, ties="all", max_peaks=32, refine="quarter", stride=4)
BATCH = 32

try:
    from scipy import ndimage
    HOST_STEP = "scipy.ndimage %s maximum_filter + numpy" % __import__("scipy").__version__
except ImportError:
    ndimage = None
    HOST_STEP = "numpy stand-in (tests/peaks_ref.py)"


def host_peaks(maps):
    """The caller's numpy step on float32 (N, K, H, W) heat maps: (peaks (N, K, max_peaks, 3), num (N, K))."""
    if ndimage is None:
        sys.path.insert(0, HERE)
        from tests import peaks_ref
        return peaks_ref.peaks_ref(maps, SPEC["threshold"], SPEC["ties"], SPEC["max_peaks"], SPEC["refine"], SPEC["stride"])
    n, k, h, w = maps.shape
    mp, s = SPEC["max_peaks"], np.float32(SPEC["stride"])
    peaks, num = np.zeros((n, k, mp, 3), np.float32), np.zeros((n, k), np.int32)
    for i in range(n):
        for j in range(k):
            v = maps[i, j]
            idx = np.flatnonzero((ndimage.maximum_filter(v, 3, mode="constant", cval=-np.inf) == v) & (v > SPEC["threshold"]))
            num[i, j] = idx.size
            flat = v.ravel()
            idx = idx[np.argsort(-flat[idx], kind="stable")][:mp]
            py, px = idx // w, idx % w
            dx, dy = np.zeros(idx.size, np.float32), np.zeros(idx.size, np.float32)
            a = (px > 0) & (px < w - 1)
            dx[a] = np.sign(flat[idx[a] + 1] - flat[idx[a] - 1]) * 0.25
            a = (py > 0) & (py < h - 1)
            dy[a] = np.sign(flat[idx[a] + w] - flat[idx[a] - w]) * 0.25
            peaks[i, j, :idx.size] = np.stack([(px + dx) * s, (py + dy) * s, flat[idx]], 1)
    return peaks, num


def arm_child(args):
    sys.path.insert(0, HERE)
    import planer_amd
    from planer_amd.irgen import posenet
    how = args.arm.split("-", 1)[1]
    rng = np.random.default_rng(3)
    g, blob = posenet.build()
    net = planer_amd.from_graph(g, blob)
    net.image_input(*planer_amd.util.image_affine(MEAN, STD))
    if how == "keypoints":
        net.keypoint_output(**SPEC)
    line = {"arm": args.arm, "round": args.round, "host_step": HOST_STEP if how == "maps-host" else None}
    batches = [rng.integers(0, 256, (BATCH,) + posenet.SIZE + (3,), dtype=np.uint8) for _ in range(2)]
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
    line["img_s"] = round(BATCH * args.passes / (time.perf_counter() - t0), 1)
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
    if how == "maps-host":
        t0 = time.perf_counter()
        line["peaks_per_batch"] = int(host_peaks(got)[1].sum())
        line["host_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3, 1)
        t0 = time.perf_counter()
        host_loop(args.host_passes, host_peaks)
        line["img_s_host_step_included"] = round(BATCH * args.host_passes / (time.perf_counter() - t0), 1)
    elif how == "keypoints":
        line["peaks_per_batch"] = int(got[1].sum())
    ctx = planer_amd.hip.context()
    if ctx.tune_cache:
        ctx.save_tune_cache()
    print(json.dumps(line), flush=True)


def inputs(large):
    """[(name, ties, threshold, float32 (N, K, H, W))]: the batch's tensor and the large map's three fillings."""
    rng = np.random.default_rng(4)
    h, w = large
    return [("one tile", "all", 0.0, rng.standard_normal((1, 1, 8, 8)).astype(np.float32)),
            ("batch (32, 17, 64, 48), random", "all", 0.0, rng.standard_normal((32, 17, 64, 48)).astype(np.float32)),
            ("large, random", "all", 0.0, rng.standard_normal((1, 1, h, w)).astype(np.float32)),
            ("large, constant, ties all", "all", 0.0, np.full((1, 1, h, w), 0.5, np.float32)),
            ("large, all below threshold", "all", 0.0, -np.abs(rng.standard_normal((1, 1, h, w))).astype(np.float32) - 1)]


def kernels_child(args):
    sys.path.insert(0, HERE)
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

    def chain(x, ties, threshold):
        """The entry point itself into fixed arrays: no allocation between the events."""
        n, k, h, w = x.shape
        mp = SPEC["max_peaks"]
        peaks, num = hip.empty((n, k, mp, 3), np.float32, ctx=ctx), hip.empty((n, k), np.int32, ctx=ctx)
        scratch = hip.empty((util._peaks_scratch_bytes(n, k, h, w, mp) // 8 + 1,), np.int64, ctx=ctx)
        fn = lambda: _lib.call("pl_peaks_f32", ctx.handle, x.ptr, n, k, h, w, threshold, _lib.PEAKS_TIES[ties], mp,      # noqa: E731
                               _lib.PEAKS_REFINE["quarter"], 4.0, 4.0, scratch.ptr, peaks.ptr, num.ptr)
        return fn, num
    floor = copy_rate = None
    for name, ties, threshold, host in inputs(args.large):
        x = hip.asarray(host)
        fn, num = chain(x, ties, threshold)
        t = timed(fn, calls_per_timing(name, args.launches))
        if name == "one tile":
            floor = t
        line = {"kernel": "pl_peaks_f32", "input": name, "shape": list(host.shape), "us": round(t * 1e6, 2), "peaks": int(num.get().sum()),
                "tiles": int(host.shape[0] * host.shape[1] * -(-host.shape[2] // _lib.PEAKS_TILE_H) * -(-host.shape[3] // _lib.PEAKS_TILE_W)),
                "launch_floor_us": round(floor * 1e6, 2), "input_GB_s_whole_chain": round(host.nbytes / t / 1e9, 1)}
        if name.startswith("large") and copy_rate is None:
            y = hip.empty(host.shape, np.float32, ctx=ctx)
            tc = timed(lambda: y.copy_from(x), calls_per_timing(name, args.launches))
            copy_rate = host.nbytes / tc
            print(json.dumps({"kernel": "device copy", "shape": list(host.shape), "us": round(tc * 1e6, 2),
                              "copied_GB_s": round(copy_rate / 1e9, 1)}), flush=True)
        print(json.dumps(line), flush=True)


def calls_per_timing(name, launches):
    return launches if "large" not in name else max(launches // 5, 3)


def chain_calls(name, launches):
    """Calls of the chain the kernels step makes for one input: 3 to warm up, then 3 timings."""
    return 3 + 3 * calls_per_timing(name, launches)


def trace_digest(directory, large, launches, copy_gb_s):
    """Median device time in us of the two kernels, per input, from a rocprofv3 kernel trace of the kernels step: the chains in
    launch order (each begins with tile_kernel), dealt out to the inputs by the number of calls the step makes."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if "peaks::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    chains = []
    for r in rows:
        name = r["Kernel_Name"].split("peaks::")[1].split("(")[0]
        if name == "tile_kernel":
            chains.append([])
        chains[-1].append((name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    out, at = collections.OrderedDict(), 0
    for name, _, _, host in inputs(large):
        mine, at = chains[at:at + chain_calls(name, launches)], at + chain_calls(name, launches)
        per = collections.OrderedDict()
        for c in mine:
            for kernel, us in c:
                per.setdefault(kernel, []).append(us)
        out[name] = {k: round(sorted(v)[len(v) // 2], 2) for k, v in per.items()}
        out[name]["sum"] = round(sum(out[name].values()), 2)
        if out[name].get("tile_kernel"):
            rate = host.nbytes / out[name]["tile_kernel"] / 1e3
            out[name]["tile_kernel_read_GB_s"] = round(rate, 1)
            if copy_gb_s:
                out[name]["tile_kernel_read_over_copy_rate"] = round(rate / copy_gb_s, 3)
    out["chains_in_trace"], out["chains_expected"] = len(chains), at
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=60, help="submits per timed loop")
    ap.add_argument("--host-passes", type=int, default=3, help="submits of the loop that includes the caller's host step")
    ap.add_argument("--calls", type=int, default=7, help="net(x) calls timed")
    ap.add_argument("--launches", type=int, default=50, help="launches between the two events of a kernel timing")
    ap.add_argument("--large", type=int, nargs=2, default=[1024, 1536], help="H W of the large map (tiles of 32 x 64)")
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
              "--launches", str(args.launches), "--large", str(args.large[0]), str(args.large[1])]

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
    out = {"dtype": "fp32", "rounds": args.rounds, "passes": args.passes, "spec": SPEC, "arms": {}, "kernels": kernels}
    if args.trace:
        d = os.path.join(tmp.name, "trace")
        step(["--child", "kernels"], wrap=["rocprofv3", "--kernel-trace", "-d", d, "-o", "peaks", "--output-format", "csv", "--"])
        copy = [k["copied_GB_s"] for k in kernels if k["kernel"] == "device copy"]
        out["trace"] = trace_digest(d, args.large, args.launches, copy[0] if copy else None)
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

"""What a caller with IMAGES gets from ResNet-18 at batch 32, 224 x 224, fp32 on one GPU: host batches through
net.submit with a window of passes in flight (bench.py's host loop), as
  a  float32 NCHW, prepared by the caller           (what every figure of this project started from)
  b  uint8 NHWC 224 x 224, decoded on the GPU        (Net.image_input: pl_image_u8_nchw_f32 in front of the plan)
  c  uint8 NHWC 256 x 256, resized to 224 x 224 and decoded on the GPU
the three arms ALTERNATING --rounds times in one process on one compiled plan, so that the spread between same-arm rounds is
visible beside the differences; then net(x) on a host array, one call at a time, for the float32 and the uint8 form (d); the
kernel alone, with and without resize (e); and for context the numpy chain the reference's demos write in front of net(x) --
resize, / 255, - mean, / std, transpose -- in ms per batch on one core of this host (f).  One JSON line per arm run, then one
summary line; `b_not_slower_than_a` is the check: the median of b is not below the median of a by more than the largest spread
between same-arm rounds.
    python tools/image_input_bench.py [--batch 32] [--rounds 3] [--passes 100] [--arms abc] [--root DIR]
--arms a with --root DIR times arm a alone on the package found in DIR (another checkout: the parent commit's figure).
The device work runs in a child process under a timeout of its own; the parent never opens the GPU."""
import argparse
import collections
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def numpy_chain(x, size):
    """One batch the way the reference's demos prepare it (planer/util.py resize restated on uint8 -> float32)."""
    mean, std = np.array(MEAN, np.float32), np.array(STD, np.float32)
    out = []
    for img in x:
        if img.shape[:2] != tuple(size):
            h, w = img.shape[:2]
            (ra, rs), (ca, cs) = [_samples(n, s) for n, s in ((h, size[0]), (w, size[1]))]
            rs, cs = rs[:, None, None], cs[None, :, None]
            buf = img[:, ca] * (1 - cs) + img[:, ca + 1] * cs
            img = buf[ra] * (1 - rs) + buf[ra + 1] * rs
        out.append(((img / np.float32(255) - mean) / std).astype(np.float32).transpose(2, 0, 1))
    return np.ascontiguousarray(np.stack(out))      # (stacking transposed views keeps THEIR memory order: the net wants C order)


def _samples(n, size):
    k = size / n
    pos = np.clip(np.linspace(-0.5 + 0.5 / k, n - 0.5 - 0.5 / k, size, dtype=np.float32), 0, n - 1)
    lo = np.floor(np.clip(pos, 0, n - 1.001)).astype(int)
    return lo, pos - lo


def device(args):
    sys.path.insert(0, args.root)
    import planer_amd
    from planer_amd.irgen import resnet18
    n, s = args.batch, args.size
    rng = np.random.default_rng(3)
    u8 = [rng.integers(0, 256, (n, s, s, 3), dtype=np.uint8) for _ in range(2)]
    big = [rng.integers(0, 256, (n, args.big, args.big, 3), dtype=np.uint8) for _ in range(2)]
    g, blob = resnet18.build()
    ctx = planer_amd.hip.context()
    net = planer_amd.from_graph(g, blob)
    arms = {}
    if set(args.arms) - {"a"}:
        k, b = planer_amd.util.image_affine(MEAN, STD)
        net.image_input(k, b, size=(s, s))
        f32 = [planer_amd.util.decode_images(planer_amd.asarray(x), k, b).get() for x in u8]
        arms["b"], arms["c"] = u8, big
    else:
        f32 = [numpy_chain(x, (s, s)) for x in u8]
    arms["a"] = f32
    window, pend = 12, collections.deque()

    def host_loop(count, batches):
        got = None
        for i in range(count):
            pend.append(net.submit(batches[i & 1]))
            if len(pend) > window:
                got = pend.popleft().get()
        while pend:
            got = pend.popleft().get()
        return got
    t0 = time.perf_counter()
    host_loop(20, f32)
    lines = [{"compile_and_warm_s": round(time.perf_counter() - t0, 2), "tune_source": net.tune_source(),
              "streams": [getattr(p, "streams", None) for p in net._plans.values()]}]
    print(json.dumps(lines[0]), flush=True)
    ref = host_loop(2, f32)
    for rnd in range(args.rounds):
        for arm in args.arms:
            host_loop(20, arms[arm])
            t0 = time.perf_counter()
            got = host_loop(args.passes, arms[arm])
            line = {"arm": arm, "round": rnd, "img_s": round(n * args.passes / (time.perf_counter() - t0), 1)}
            if arm == "b":
                line["max_abs_diff_vs_float_route"] = float(np.abs(got - ref).max())
            print(json.dumps(line), flush=True)
    if "d" in args.also:
        for label, batches in (("float32", f32), ("uint8", u8)) if "b" in arms else (("float32", f32),):
            for i in range(5):
                net(batches[i & 1])
            ts = []
            for i in range(args.calls):
                t0 = time.perf_counter()
                net(batches[i & 1])
                ts.append(time.perf_counter() - t0)
            med = sorted(ts)[len(ts) // 2]
            print(json.dumps({"net_call_host": label, "ms": round(med * 1e3, 3), "img_s": round(n / med, 1),
                              "ms_spread": [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]}), flush=True)
    if "e" in args.also and "b" in arms:
        from planer_amd import hip
        from planer_amd.util import ImageFeed, ImageSpec
        y = hip.empty((n, 3, s, s), ctx=ctx)

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
        tiny = ImageFeed(ImageSpec(k, b), planer_amd.asarray(u8[0][:1, :1, :4]))
        floor = timed(lambda: tiny.decode_into(y.ptr))
        for label, x in (("224 no resize", u8[0]), ("%d -> 224 resize" % args.big, big[0])):
            feed = ImageFeed(ImageSpec(k, b, size=(s, s)), planer_amd.asarray(x))
            t = timed(lambda: feed.decode_into(y.ptr))
            nbytes = x.nbytes + y.nbytes
            print(json.dumps({"kernel": label, "us": round(t * 1e6, 1), "bytes": nbytes, "gb_s": round(nbytes / t / 1e9, 1),
                              "launch_floor_us": round(floor * 1e6, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--big", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=100)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--arms", default="abc")
    ap.add_argument("--also", default="def", help="d: net(x) per call, e: the kernel alone, f: the numpy chain on this host")
    ap.add_argument("--root", default=HERE, help="directory that holds the planer_amd package to time")
    ap.add_argument("--timeout", type=int, default=500, help="seconds the device child may take")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return device(args)
    out = {"workload": "resnet18", "batch": args.batch, "size": args.size, "dtype": "fp32", "passes": args.passes,
           "rounds": args.rounds, "root": os.path.relpath(args.root, HERE)}
    if "f" in args.also:
        rng = np.random.default_rng(3)
        for label, side in (("224", args.size), ("%d -> 224" % args.big, args.big)):
            x = rng.integers(0, 256, (args.batch, side, side, 3), dtype=np.uint8)
            numpy_chain(x[:2], (args.size, args.size))
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                numpy_chain(x, (args.size, args.size))
                ts.append(time.perf_counter() - t0)
            out.setdefault("numpy_chain_ms_per_batch_one_core", {})[label] = round(min(ts) * 1e3, 1)
        print(json.dumps({"numpy_chain_ms_per_batch_one_core": out["numpy_chain_ms_per_batch_one_core"]}), flush=True)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("device child failed (exit %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-3000:]))
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    for ln in lines:
        print(json.dumps(ln), flush=True)
    rates = {a: [ln["img_s"] for ln in lines if ln.get("arm") == a] for a in args.arms}
    med = {a: sorted(v)[len(v) // 2] for a, v in rates.items() if v}
    spread = {a: round(max(v) - min(v), 1) for a, v in rates.items() if v}
    out.update(img_s=rates, median_img_s=med, same_arm_spread_img_s=spread,
               net_call_host=[ln for ln in lines if "net_call_host" in ln], kernels=[ln for ln in lines if "kernel" in ln])
    if "a" in med and "b" in med:
        out["b_over_a"] = round(med["b"] / med["a"], 3)
        out["b_not_slower_than_a"] = bool(med["b"] >= med["a"] - max(spread.values()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""What a caller who wants BYTES back gets from two nets, fp32 on one GPU: host batches through net.submit with a
window of passes in flight (bench.py's host loop), and net(x) one call at a time.
  fpn-a   FPN, batch 32, 224 x 224, 21 classes, host uint8 in (Net.image_input): float32 logits out, then
          argmax(1).astype(uint8) on the host -- the host part timed on its own and inside the loop
  fpn-b   the same net with Net.label_output: the label map comes back            (pl_labels_f32_u8 in place of the output copy)
  edsr-a  EDSR x4, batch 8, 128 x 128 in: float32 image out, then clip, rint, transpose to HWC uint8 on the host
  edsr-b  the same net with Net.image_output                                       (pl_image_f32_u8)
Every arm run is a FRESH process under a timeout of its own; the arms alternate --rounds times and share one tuning cache
(--cache, default: a file of this run's own), so that after the first run of a net no process measures a pick again.  Then the
two kernels alone (one more process): HIP events around --launches launches after warm-up, achieved bytes/s from the byte model
(4 C + 1 bytes per pixel for labels, 5 Co per pixel for images) and its share of the 6.29 TB/s a device copy reaches.
One JSON line per step as it ends, then one summary line.  The tool stops at the first step that fails.
    python tools/image_output_bench.py [--rounds 3] [--passes 60] [--arms fpn-a,fpn-b,edsr-a,edsr-b] [--no-kernels]
The parent process never opens the GPU."""
import argparse
import collections
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
COPY_TB_S = 6.29            # a device-to-device copy on this part (bytes read + written per second)
ARMS = ["fpn-a", "fpn-b", "edsr-a", "edsr-b"]
KERNEL_SHAPES = [("labels", (32, 21, 224, 224)), ("labels", (32, 2, 256, 256)), ("image nhwc", (8, 3, 512, 512)),
                 ("image nchw", (8, 3, 512, 512)), ("image nhwc", (32, 3, 224, 224))]


def host_labels(y):
    return y.argmax(1).astype(np.uint8)


def host_image(y):
    return np.ascontiguousarray(np.rint(np.clip(y * np.float32(255), 0, 255)).astype(np.uint8).transpose(0, 2, 3, 1))


def arm_child(args):
    sys.path.insert(0, HERE)
    import planer_amd
    from planer_amd.irgen import edsr, fpn
    name, declared = args.arm.split("-")[0], args.arm.endswith("-b")
    rng = np.random.default_rng(3)
    if name == "fpn":
        n = 32
        g, blob = fpn.build()
        net = planer_amd.from_graph(g, blob)
        net.image_input(*planer_amd.util.image_affine(MEAN, STD))
        batches = [rng.integers(0, 256, (n, 224, 224, 3), dtype=np.uint8) for _ in range(2)]
        post = host_labels
        if declared:
            net.label_output()
    else:
        n = 8
        g, blob = edsr.build(scale=4, size=128)
        net = planer_amd.from_graph(g, blob)
        batches = [edsr.make_input(n, seed=5 + i, size=128) for i in range(2)]
        post = host_image
        if declared:
            net.image_output(*planer_amd.util.image_affine_inverse(0, 1))
    window, pend = 12, collections.deque()

    def host_loop(count, finish=None):
        got = None
        for i in range(count):
            pend.append(net.submit(batches[i & 1]))
            if len(pend) > window:
                got = pend.popleft().get()
                got = finish(got) if finish else got
        while pend:
            got = pend.popleft().get()
            got = finish(got) if finish else got
        return got
    t0 = time.perf_counter()
    host_loop(20)
    line = {"arm": args.arm, "round": args.round, "compile_and_warm_s": round(time.perf_counter() - t0, 2),
            "tune_source": net.tune_source(), "streams": [getattr(p, "streams", None) for p in net._plans.values()]}
    host_loop(20)
    t0 = time.perf_counter()
    got = host_loop(args.passes)
    line["img_s"] = round(n * args.passes / (time.perf_counter() - t0), 1)
    line["output_bytes_per_batch"] = int(got.nbytes)
    line["output"] = [str(got.dtype)] + list(got.shape)
    for i in range(3):
        net(batches[i & 1])
    ts = []
    for i in range(args.calls):
        t0 = time.perf_counter()
        got = net(batches[i & 1])
        ts.append(time.perf_counter() - t0)
    line["net_call_ms"] = round(sorted(ts)[len(ts) // 2] * 1e3, 3)
    if not declared:                                   # the caller's own step: alone, inside the submit loop, behind net(x)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            u8 = post(got)
            ts.append(time.perf_counter() - t0)
        line["host_ms_per_batch"] = round(min(ts) * 1e3, 2)
        line["bytes_wanted_per_batch"] = int(u8.nbytes)
        t0 = time.perf_counter()
        host_loop(args.host_passes, post)
        line["img_s_host_step_included"] = round(n * args.host_passes / (time.perf_counter() - t0), 1)
        line["net_call_ms_host_step_included"] = round(line["net_call_ms"] + line["host_ms_per_batch"], 3)
    else:                                              # the bytes are the host's: checked once against the float route
        net.float_output()
        want = post(net(batches[(args.calls - 1) & 1]))
        line["equals_host_step"] = bool((want == got).all())
        line["bytes_differing_from_host_step"] = int((want != got).sum())
    ctx = planer_amd.hip.context()
    if ctx.tune_cache:
        ctx.save_tune_cache()
    print(json.dumps(line), flush=True)


def kernels_child(args):
    sys.path.insert(0, HERE)
    import planer_amd
    from planer_amd import hip
    from planer_amd.util import ImageOutSpec, LabelSpec
    from planer_amd import _lib
    ctx = hip.context()
    rng = np.random.default_rng(4)

    def launcher(what, x):
        """The entry point itself into one output array: no allocation between the events."""
        n, c, h, w = x.shape
        if what == "labels":
            y = hip.empty((n, h, w), np.uint8, ctx=ctx)
            return y, lambda: _lib.call("pl_labels_f32_u8", ctx.handle, x.ptr, y.ptr, n, c, h, w, 0.0)
        spec = ImageOutSpec(np.ones(c), np.zeros(c), layout=what.split()[1])
        k, b = spec._affine(c)
        y = hip.empty((n, h, w, c) if spec.layout == "nhwc" else (n, c, h, w), np.uint8, ctx=ctx)
        return y, lambda: _lib.call("pl_image_f32_u8", ctx.handle, x.ptr, y.ptr, n, c, h, w, c, None, int(spec.layout == "nhwc"),
                                    k, b, 0)

    def timed(fn):
        for _ in range(10):
            fn()
        best = None
        for _ in range(5):
            e0 = hip.Event(ctx).record()
            for _ in range(args.launches):
                fn()
            e1 = hip.Event(ctx).record()
            t = e0.elapsed_ms(e1) / args.launches * 1e-3
            best = t if best is None else min(best, t)
        return best
    floor = {}
    for what in ("labels", "image nhwc", "image nchw"):                # a one-tile launch: what the host and the launch cost
        tiny = hip.asarray(np.zeros((1, 3, 4, 4), np.float32))
        floor[what] = timed(launcher(what, tiny)[1])
    for what, shape in KERNEL_SHAPES:
        n, c, h, w = shape
        scale, shift = (1, 0) if what == "labels" else (100, 128)
        x = hip.asarray((rng.standard_normal(shape) * scale + shift).astype(np.float32))
        model = (4 * c + 1) * n * h * w if what == "labels" else 5 * c * n * h * w
        y, fn = launcher(what, x)
        best = timed(fn)
        spec = LabelSpec() if what == "labels" else ImageOutSpec(np.ones(c), np.zeros(c), layout=what.split()[1])
        same = bool((spec.encode(x).get() == y.get()).all())          # (the Python surface: the same bytes)
        print(json.dumps({"kernel": what, "shape": list(shape), "us": round(best * 1e6, 2), "model_bytes": model,
                          "tb_s": round(model / best / 1e12, 3), "share_of_copy_rate": round(model / best / 1e12 / COPY_TB_S, 3),
                          "launch_floor_us": round(floor[what] * 1e6, 2), "launches": args.launches, "surface_same_bytes": same}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=60, help="submits per timed loop")
    ap.add_argument("--host-passes", type=int, default=12, help="submits of the loop that includes the caller's host step")
    ap.add_argument("--calls", type=int, default=15, help="net(x) calls timed")
    ap.add_argument("--launches", type=int, default=100, help="launches between the two events of a kernel timing")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--cache", default=None, help="tuning cache file every process loads and saves")
    ap.add_argument("--timeout", type=int, default=240, help="seconds one child process may take")
    ap.add_argument("--child", choices=["arm", "kernels"])
    ap.add_argument("--arm")
    ap.add_argument("--round", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return arm_child(args) if args.child == "arm" else kernels_child(args)
    tmp = None
    if args.cache is None:
        tmp = tempfile.TemporaryDirectory()
        args.cache = os.path.join(tmp.name, "tune.json")
    env = dict(os.environ, PLANER_HIP_TUNE_CACHE=os.path.abspath(args.cache))
    common = ["--passes", str(args.passes), "--host-passes", str(args.host_passes), "--calls", str(args.calls),
              "--launches", str(args.launches)]

    def step(extra):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__)] + extra + common
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
    med = lambda v: sorted(v)[len(v) // 2] if v else None        # noqa: E731
    for arm in arms:
        mine = [r for r in runs if r["arm"] == arm]
        s = {"img_s": [r["img_s"] for r in mine], "median_img_s": med([r["img_s"] for r in mine]),
             "median_net_call_ms": med([r["net_call_ms"] for r in mine]), "output_bytes_per_batch": mine[0]["output_bytes_per_batch"]}
        for key in ("host_ms_per_batch", "img_s_host_step_included", "net_call_ms_host_step_included"):
            if key in mine[0]:
                s["median_" + key] = med([r[key] for r in mine])
        if "equals_host_step" in mine[0]:
            s["equals_host_step"] = all(r["equals_host_step"] for r in mine)
        out["arms"][arm] = s
    for name in ("fpn", "edsr"):
        a, b = out["arms"].get(name + "-a"), out["arms"].get(name + "-b")
        if a and b:
            out[name + "_b_over_a_submit"] = round(b["median_img_s"] / a["median_img_s"], 3)
            out[name + "_b_over_a_submit_host_step_included"] = round(b["median_img_s"] / a["median_img_s_host_step_included"], 3)
            out[name + "_bytes_a_over_b"] = round(a["output_bytes_per_batch"] / b["output_bytes_per_batch"], 1)
    print(json.dumps(out))
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()

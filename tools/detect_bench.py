"""What a caller who wants DETECTIONS back gets from YOLO-v3 at 416 x 416, fp32 on one GPU: host uint8 batches
(Net.image_input) through net.submit with a window of passes in flight (bench.py's host loop), and net(x) one call at a time,
at batch 1 and batch 8.
  a1 / a8   the three float32 heads downloaded, nothing else
  b1 / b8   the same, and the caller's post-processing in numpy on the host: sigmoid and exp over every anchor, threshold,
            sort, a Python-loop NMS -- timed on its own and inside the loop
  c1 / c8   the same net with Net.detection_output: det (N, 100, 6) and num come back      (pl_yolo_decode_f32 x 3, pl_topk_f32,
            pl_nms_f32 behind the pass); also the device time of those five launches alone, by HIP events, and whether det and
            num agree with the host step of b
  p1 / p8   arm a run from ANOTHER source tree (--parent-tree: a built checkout of the parent commit), same session
Then the five launches one by one (one more process): HIP events around --launches launches of each, on seeded heads of the same
shapes, next to the cost of a launch that does nothing.
The generator's random weights give head logits in the hundreds, where every score is 0 or 1, so the heads are built with
head_gain (irgen/yolov3.py), and conf is picked per arm from the scores of its first batch: `sparse`, about --candidates (100)
anchors per image above it, which is what the loops run with, and `dense`, at least max_candidates (1024) per image, which the
post-processing alone is also timed at.  The counts are printed.
Every arm run is a FRESH process under a timeout of its own; the arms alternate --rounds times and share one tuning cache
(--cache, default: a file of this run's own).  One JSON line per arm run as it ends, appended to --lines as well, then one
summary line.  The tool stops at the first step that fails.
    python tools/detect_bench.py [--rounds 3] [--passes 60] [--arms a1,b1,c1,a8,b8,c8] [--parent-tree DIR] [--no-kernels]
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
ANCHORS = [(10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198), (373, 326)]
HEADS = [(ANCHORS[6:], None), (ANCHORS[3:6], None), (ANCHORS[:3], None)]
CLASSES, SIZE, HEAD_GAIN = 80, 416, 1.0 / 512
IOU, MAX_DET, MAX_CANDIDATES = 0.45, 100, 1024
ARMS = ["a1", "b1", "c1", "a8", "b8", "c8"]


# ---- the caller's numpy step --------------------------------------------------------------------------------------------------
def host_decode(heads):
    """(scores, classes, boxes) of every anchor, float32, heads in declared order: what a caller writes in numpy."""
    out = []
    for x, (anchors, _) in zip(heads, HEADS):
        n, _, gh, gw = x.shape
        a = len(anchors)
        t = x.reshape(n, a, 5 + CLASSES, gh, gw)
        sig = lambda v: 1 / (1 + np.exp(-v))                        # noqa: E731
        cls = t[:, :, 5:].argmax(2)
        score = sig(t[:, :, 4]) * sig(np.take_along_axis(t[:, :, 5:], cls[:, :, None], 2)[:, :, 0])
        an = np.asarray(anchors, np.float32)
        cx = (sig(t[:, :, 0]) + np.arange(gw, dtype=np.float32)) * np.float32(SIZE / gw)
        cy = (sig(t[:, :, 1]) + np.arange(gh, dtype=np.float32)[:, None]) * np.float32(SIZE / gh)
        w, h = np.exp(t[:, :, 2]) * an[:, 0, None, None], np.exp(t[:, :, 3]) * an[:, 1, None, None]
        box = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1)
        out.append((score.reshape(n, -1), cls.reshape(n, -1), box.reshape(n, -1, 4)))
    return [np.concatenate(v, 1) for v in zip(*out)]


def host_post(heads, conf):
    """det (N, MAX_DET, 6), num (N,): threshold, sort (score descending, index ascending), class-aware greedy NMS in a loop."""
    with np.errstate(over="ignore"):
        score, cls, box = host_decode(heads)
    n = len(score)
    det, num = np.zeros((n, MAX_DET, 6), np.float32), np.zeros(n, np.int32)
    for i in range(n):
        c = np.flatnonzero(score[i] > np.float32(conf))
        c = c[np.argsort(-score[i, c], kind="stable")][:MAX_CANDIDATES]
        b, k, s = box[i, c], cls[i, c], score[i, c]
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        alive = np.ones(len(c), bool)
        for j in range(len(c)):
            if not alive[j]:
                continue
            det[i, num[i]] = (*b[j], s[j], k[j])
            num[i] += 1
            if num[i] == MAX_DET:
                break
            iw = np.maximum(0, np.minimum(b[j, 2], b[j + 1:, 2]) - np.maximum(b[j, 0], b[j + 1:, 0]))
            ih = np.maximum(0, np.minimum(b[j, 3], b[j + 1:, 3]) - np.maximum(b[j, 1], b[j + 1:, 1]))
            inter = iw * ih
            alive[j + 1:] &= ~((inter > np.float32(IOU) * (area[j] + area[j + 1:] - inter)) & (k[j + 1:] == k[j]))
    return det, num


def pick_conf(scores, per_image):
    """A threshold between two neighbouring scores of the batch with about per_image anchors per image above it."""
    s = np.sort(scores.reshape(-1))[::-1]
    at = min(per_image * len(scores), s.size - 1)
    return float(np.float32((float(s[at - 1]) + float(s[at])) / 2))


# ---- one arm, one process -----------------------------------------------------------------------------------------------------
def arm_child(args):
    sys.path.insert(0, args.root or HERE)
    import planer_amd
    from planer_amd import hip
    from planer_amd.irgen import yolov3
    kind, n = args.arm[0], int(args.arm[1:])
    try:
        g, blob = yolov3.build(head_gain=HEAD_GAIN)
    except TypeError:                                      # a tree from before head_gain: arm p's timing does not hang on the values
        g, blob = yolov3.build()
    net = planer_amd.from_graph(g, blob)
    net.image_input(*planer_amd.util.image_affine(MEAN, STD))
    rng = np.random.default_rng(3)
    batches = [rng.integers(0, 256, (n, SIZE, SIZE, 3), dtype=np.uint8) for _ in range(2)]
    line = {"arm": args.arm, "round": args.round, "batch": n, "tree": "parent" if args.root else "this"}
    t0 = time.perf_counter()
    heads = net(batches[0])
    line["compile_and_first_pass_s"] = round(time.perf_counter() - t0, 2)
    conf = {}
    if kind in "bc":
        with np.errstate(over="ignore"):
            scores = host_decode(heads)[0]
        for name, per_image in (("sparse", args.candidates), ("dense", MAX_CANDIDATES + 200)):
            conf[name] = pick_conf(scores, per_image)
            line["conf_" + name] = conf[name]
            line["candidates_per_image_" + name] = round(float((scores > np.float32(conf[name])).sum(1).mean()), 1)
    if kind == "c":
        net.detection_output(HEADS, CLASSES, conf=conf["sparse"], iou=IOU, max_det=MAX_DET, max_candidates=MAX_CANDIDATES, size=(SIZE, SIZE))
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
    host_loop(20)
    line["tune_source"] = net.tune_source()
    line["streams"] = [getattr(p, "streams", None) for p in net._plans.values()]
    host_loop(20)
    t0 = time.perf_counter()
    got = host_loop(args.passes)
    line["img_s"] = round(n * args.passes / (time.perf_counter() - t0), 1)
    line["output_bytes_per_batch"] = int(sum(v.nbytes for v in got))
    line["output"] = [[str(v.dtype)] + list(v.shape) for v in got]
    for i in range(3):
        net(batches[i & 1])
    ts = []
    for i in range(args.calls):
        t0 = time.perf_counter()
        got = net(batches[i & 1])
        ts.append(time.perf_counter() - t0)
    line["net_call_ms"] = round(sorted(ts)[len(ts) // 2] * 1e3, 3)
    if kind == "b":                                        # the caller's own step: alone at both settings, inside the loop at sparse
        for name in conf:
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                det, num = host_post(got, conf[name])
                ts.append(time.perf_counter() - t0)
            line["host_ms_per_batch_" + name] = round(min(ts) * 1e3, 2)
            line["kept_per_image_" + name] = round(float(num.mean()), 1)
        t0 = time.perf_counter()
        host_loop(args.host_passes, lambda y: host_post(y, conf["sparse"]))
        line["img_s_host_step_included"] = round(n * args.host_passes / (time.perf_counter() - t0), 1)
        line["net_call_ms_host_step_included"] = round(line["net_call_ms"] + line["host_ms_per_batch_sparse"], 3)
    if kind == "c":
        det, num = got
        line["kept_per_image_sparse"] = round(float(num.mean()), 1)
        net.float_output()
        dev_heads = net(hip.asarray(batches[(args.calls - 1) & 1]))          # device tensors of the same batch
        want_det, want_num = host_post([h.get() for h in dev_heads], conf["sparse"])
        line["num_equals_host_step"] = bool((want_num == num).all())
        line["max_abs_diff_from_host_step"] = float(np.abs(want_det - det).max()) if line["num_equals_host_step"] else None
        # the five launches alone: queued behind two 1 GiB copies so that the device, not the host, paces them
        ctx = dev_heads[0].ctx
        big = hip.empty((1 << 28,), np.float32, ctx=ctx), hip.empty((1 << 28,), np.float32, ctx=ctx)
        for name in conf:
            spec = planer_amd.util.DetectionSpec(HEADS, CLASSES, conf=conf[name], iou=IOU, max_det=MAX_DET,
                                                 max_candidates=MAX_CANDIDATES, size=(SIZE, SIZE))
            best, host_best = None, None
            for _ in range(args.post_rounds + 2):
                big[1].copy_from(big[0])
                big[0].copy_from(big[1])
                e0 = hip.Event(ctx).record()
                t0 = time.perf_counter()
                out = spec.encode(list(dev_heads), ctx)
                t1 = time.perf_counter()
                e1 = hip.Event(ctx).record()
                ctx.synchronize()
                t = e0.elapsed_ms(e1) * 1e3
                best = t if best is None else min(best, t)
                host_best = (t1 - t0) * 1e6 if host_best is None else min(host_best, (t1 - t0) * 1e6)
            line["post_device_us_" + name] = round(best, 2)
            line["post_host_enqueue_us_" + name] = round(host_best, 1)
            line["kept_per_image_post_" + name] = round(float(out[1].get().mean()), 1)
        del big
    ctx = hip.context()
    if ctx.tune_cache:
        ctx.save_tune_cache()
    print(json.dumps(line), flush=True)


def kernels_child(args):
    """Each of the five launches alone on heads of YOLO-v3's shapes at 416 (seeded normals, so the scores spread without a net):
    HIP events around --launches launches into the same arrays, best of 5; the floor is pl_nms_f32 with K = 0."""
    sys.path.insert(0, HERE)
    import planer_amd
    from planer_amd import _lib, hip
    ctx = hip.context()
    rng = np.random.default_rng(0)

    def timed(fn):
        for _ in range(5):
            fn()
        best = None
        for _ in range(5):
            e0 = hip.Event(ctx).record()
            for _ in range(args.launches):
                fn()
            e1 = hip.Event(ctx).record()
            t = e0.elapsed_ms(e1) / args.launches * 1e3
            best = t if best is None else min(best, t)
        return round(best, 2)
    for n in (1, 8):
        host = [(rng.standard_normal((n, 255, g, g)) * 1.5 - 1).astype(np.float32) for g in (13, 26, 52)]
        heads = [hip.asarray(h) for h in host]
        host_scores = host_decode(host)[0]
        for name, per_image in (("sparse", args.candidates), ("dense", MAX_CANDIDATES + 200)):
            conf = pick_conf(host_scores, per_image)
            spec = planer_amd.util.DetectionSpec(HEADS, CLASSES, conf=conf, iou=IOU, max_det=MAX_DET, max_candidates=MAX_CANDIDATES,
                                                 size=(SIZE, SIZE))
            _, rows, total, k, md = spec.geometry([h.shape for h in heads])
            scores, boxes, classes = hip.empty((n, total)), hip.empty((n, total, 4)), hip.empty((n, total), np.int32)
            vals, idx = hip.empty((n, k)), hip.empty((n, k), np.int64)
            det, num = hip.empty((n, md, 6)), hip.empty((n,), np.int32)

            def decode(i):
                a, c, gh, gw, sx, sy, off = rows[i]
                return lambda: _lib.call("pl_yolo_decode_f32", ctx.handle, heads[i].ptr, n, a, c, gh, gw, spec._anchors[i], sx, sy,
                                         spec.conf, total, off, scores.ptr, classes.ptr, boxes.ptr)
            line = {"kernels": name, "batch": n, "candidates_per_image": float((host_scores > np.float32(conf)).sum(1).mean()), "k": k,
                    "launches": args.launches}
            for i, grid in enumerate((13, 26, 52)):
                line["decode%d_us" % grid] = timed(decode(i))
            line["topk_us"] = timed(lambda: _lib.call("pl_topk_f32", ctx.handle, scores.ptr, n, total, 1, k, 1, vals.ptr, idx.ptr))
            line["nms_us"] = timed(lambda: _lib.call("pl_nms_f32", ctx.handle, boxes.ptr, classes.ptr, vals.ptr, idx.ptr, n, total, k,
                                                     spec.conf, spec.iou, 1, md, det.ptr, num.ptr))
            line["kept_per_image"] = float(num.get().mean())
            line["launch_floor_us"] = timed(lambda: _lib.call("pl_nms_f32", ctx.handle, boxes.ptr, None, vals.ptr, idx.ptr, n, total, 0,
                                                              0.0, 0.5, 0, 0, det.ptr, num.ptr))
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=60, help="submits per timed loop")
    ap.add_argument("--host-passes", type=int, default=12, help="submits of the loop that includes the caller's host step")
    ap.add_argument("--calls", type=int, default=15, help="net(x) calls timed")
    ap.add_argument("--post-rounds", type=int, default=5, help="timings of the post-processing launches alone (best of)")
    ap.add_argument("--candidates", type=int, default=100, help="anchors per image above conf in the sparse setting")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--parent-tree", default=None, help="a built source tree of the parent commit: adds arms p1 / p8 (arm a from there)")
    ap.add_argument("--cache", default=None, help="tuning cache file every process loads and saves")
    ap.add_argument("--lines", default=os.path.join(HERE, "profiles", "detect_bench_lines.jsonl"), help="JSON lines are appended here")
    ap.add_argument("--timeout", type=int, default=300, help="seconds one child process may take")
    ap.add_argument("--launches", type=int, default=50, help="launches between the two events of a kernel timing")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--child", choices=["arm", "kernels"])
    ap.add_argument("--arm")
    ap.add_argument("--root")
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
              "--post-rounds", str(args.post_rounds), "--candidates", str(args.candidates), "--launches", str(args.launches)]

    def step(extra):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__)] + extra + common
        r = subprocess.run(cmd, capture_output=True, text=True, env=env)
        if r.returncode != 0:                              # the first failing step ends the run: nothing more is started
            sys.exit("step %s failed (exit %d):\n%s\n%s" % (" ".join(extra), r.returncode, r.stdout[-2000:], r.stderr[-3000:]))
        lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        with open(args.lines, "a") as f:
            for ln in lines:
                print(json.dumps(ln), flush=True)
                f.write(json.dumps(ln) + "\n")
        return lines
    arms = [a for a in args.arms.split(",") if a]
    if args.parent_tree:
        arms = [p for a in arms for p in (["p" + a[1:], a] if a[0] == "a" else [a])]
    runs = []
    for rnd in range(args.rounds):
        for arm in arms:
            extra = ["--arm", "a" + arm[1:], "--root", os.path.abspath(args.parent_tree)] if arm[0] == "p" else ["--arm", arm]
            for ln in step(["--child", "arm"] + extra + ["--round", str(rnd)]):
                ln["arm"] = arm
                runs.append(ln)
    kernels = [] if args.no_kernels else step(["--child", "kernels"])
    med = lambda v: sorted(v)[len(v) // 2] if v else None        # noqa: E731
    out = {"dtype": "fp32", "net": "yolov3 at %d" % SIZE, "rounds": args.rounds, "passes": args.passes, "arms": {}, "kernels": kernels}
    for arm in arms:
        mine = [r for r in runs if r["arm"] == arm]
        s = {"img_s": [r["img_s"] for r in mine], "median_img_s": med([r["img_s"] for r in mine]),
             "median_net_call_ms": med([r["net_call_ms"] for r in mine]), "output_bytes_per_batch": mine[0]["output_bytes_per_batch"]}
        for key in mine[0]:
            if key.startswith(("host_ms", "img_s_host", "net_call_ms_host", "post_", "candidates_", "kept_")):
                s["median_" + key] = med([r[key] for r in mine])
        if "num_equals_host_step" in mine[0]:
            s["num_equals_host_step"] = all(r["num_equals_host_step"] for r in mine)
        out["arms"][arm] = s
    print(json.dumps(out))
    with open(args.lines, "a") as f:
        f.write(json.dumps(out) + "\n")
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()

"""What whole-image inference costs through Net.tiled and through today's route, fp32 on one GPU.
  fpn    a --scan x --scan uint8 RGB scan (default 4096), window 512, margin 0.1, FPN with 21 classes -> the uint8 label map
  edsr   a --photo x --photo uint8 RGB image (default 1024), window 512, margin 0.1, EDSR x4 -> the uint8 image (4x the side)
Per workload ONE child process under a timeout of its own; inside it the routes alternate --rounds times, every timing a host
clock around work that ends in a device synchronise or a host copy:
  new        net.tiled(host uint8 image): image_input + label_output / image_output declared, uint8 in, uint8 out
  new-dev    the same from a device image to a device result, synchronised: the GPU-resident part
  old        today's route with the same net and the same batch: normalise on the host, util.tile(batched=True) around
             net(NCHW chunk) with both transposes, .get(), then numpy argmax / clip-rint-uint8; its three parts timed apart
  old-dev    util.tile(batched=True) from a device float32 image to the device float32 result, synchronised
  kernels    the gather and the blend launch alone between HIP events, with the bytes they must move and the time those bytes
             take at 8 TB/s
and once: max |new float32 result - old float32 result| (different batch shapes may pick different conv algorithms, so it is
reported, not asserted) and whether the uint8 results agree.  One JSON line per workload, then one summary line.
    python tools/tile_net_bench.py [--rounds 3] [--workloads fpn,edsr] [--scan 4096] [--photo 1024] [--batch-fpn 9] [--batch-edsr 1]
The parent process never opens the GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
HBM_TB_S = 8.0
WINDOW, MARGIN = 512, 0.1


def child(args):
    sys.path.insert(0, HERE)
    import planer_amd as pa
    from planer_amd import hip, util
    from planer_amd.irgen import edsr, fpn
    ctx = hip.context()
    rng = np.random.default_rng(5)
    if args.child == "fpn":
        side, batch = args.scan, args.batch_fpn
        g, blob = fpn.build()
        k, b = util.image_affine(MEAN, STD)
        post = lambda y: y.argmax(2).astype(np.uint8)                                       # noqa: E731
        declare = lambda net: net.label_output()                                            # noqa: E731
    else:
        side, batch = args.photo, args.batch_edsr
        g, blob = edsr.build(scale=4, size=WINDOW)
        k, b = util.image_affine([0, 0, 0], [1, 1, 1])
        post = lambda y: np.rint(np.clip(y * np.float32(255), 0, 255)).astype(np.uint8)     # noqa: E731
        declare = lambda net: net.image_output(*util.image_affine_inverse(0, 1))            # noqa: E731
    net = pa.from_graph(g, blob)
    net.image_input(k, b)
    img = rng.integers(0, 256, (side, side, 3), dtype=np.uint8)
    tile = dict(window=WINDOW, margin=MARGIN)
    geo = util._Tiling(side, side, 1, 1, WINDOW, MARGIN)
    n = len(geo.windows)
    if n % batch:
        sys.exit("%d windows are no multiple of batch %d: today's route would need a second plan" % (n, batch))

    def f(stack):                                                                           # (n, h, w, c) -> (n, oh, ow, co)
        outs = [pa.Transpose(net(pa.Transpose(stack.rows(lo, lo + batch), [0, 3, 1, 2])), [0, 2, 3, 1]) for lo in range(0, n, batch)]
        if len(outs) == 1:
            return outs[0]
        whole = hip.empty((n,) + outs[0].shape[1:], ctx=ctx)
        for i, o in enumerate(outs):
            whole.rows(i * batch, (i + 1) * batch).copy_from(o)
        return whole
    old_tile = util.tile(progress=lambda i, m: None, batched=True, **tile)(f)
    normalise = lambda u8: u8.astype(np.float32) * k + b                                    # noqa: E731

    def clock(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3, out
    line = {"workload": args.child, "image": [side, side, 3], "window": WINDOW, "margin": geo.margin, "windows": n, "batch": batch}
    # warm up every shape: plans, conv picks, pool
    t0 = time.perf_counter()
    x32 = normalise(img)
    old_float = old_tile(x32)
    net_float = net.tiled(img, batch=batch, **tile)
    line["compile_and_warm_s"] = round(time.perf_counter() - t0, 1)
    line["max_abs_diff_float_results"] = float(np.abs(net_float - old_float).max())
    line["float_result"] = list(net_float.shape)
    declare(net)
    new_u8 = net.tiled(img, batch=batch, **tile)
    old_u8 = post(old_float)
    line["uint8_result"] = list(new_u8.shape)
    line["uint8_results_differ_at"] = int((new_u8.reshape(old_u8.shape) != old_u8).sum())
    line["result_bytes_old_over_new"] = round(old_float.nbytes / new_u8.nbytes, 1)
    dimg, dx32 = hip.asarray(img), hip.asarray(x32)
    rows = {key: [] for key in ("new", "new_dev", "old", "old_pre", "old_tile", "old_post", "old_dev")}
    for _ in range(args.rounds):
        rows["new"].append(clock(lambda: net.tiled(img, batch=batch, **tile))[0])
        net.float_output()
        pre, x = clock(lambda: normalise(img))
        mid, y = clock(lambda: old_tile(x))
        end, _ = clock(lambda: post(y))
        rows["old_pre"].append(pre), rows["old_tile"].append(mid), rows["old_post"].append(end), rows["old"].append(pre + mid + end)
        rows["old_dev"].append(clock(lambda: old_tile(dx32))[0])
        declare(net)
        rows["new_dev"].append(clock(lambda: net.tiled(dimg, batch=batch, **tile))[0])
    for key, v in rows.items():
        line[key + "_ms"] = [round(t, 2) for t in v]
        line["median_" + key + "_ms"] = round(sorted(v)[len(v) // 2], 2)
    # the two kernels alone
    feed = util.WindowFeed(dimg, geo.windows, net._image_spec(0))
    stack = feed.materialise()
    net.float_output()
    outs = f(pa.Transpose(stack, [0, 2, 3, 1]))
    outs = pa.Transpose(outs, [0, 3, 1, 2])
    spec = util.LabelSpec() if args.child == "fpn" else util.ImageOutSpec(*util.image_affine_inverse(0, 1))
    kscale = outs.shape[2] / geo.win_h

    def events(fn, launches=20):
        for _ in range(3):
            fn()
        best = None
        for _ in range(3):
            e0 = hip.Event(ctx).record()
            for _ in range(launches):
                fn()
            e1 = hip.Event(ctx).record()
            t = e0.elapsed_ms(e1) / launches
            best = t if best is None else min(best, t)
        return best
    # the entry points themselves into arrays made once: no upload and no allocation between the events
    from planer_amd import _lib
    bg = util.BlendGeometry(geo.windows, kscale, geo.margin, geo.work, outs.shape[2], outs.shape[3])
    origins = hip.asarray(np.concatenate([bg.R0, bg.C0]), ctx=ctx)
    nn, cc, oh, ow = outs.shape
    bargs = (nn, cc, oh, ow, origins.ptr, origins.ptr + 4 * nn, bg.gr, bg.gc, bg.OH, bg.OW, bg.ramp)
    y32 = hip.empty((bg.OH, bg.OW, cc), ctx=ctx)
    if args.child == "fpn":
        y8 = hip.empty((bg.OH, bg.OW), np.uint8, ctx=ctx)
        blend = lambda: _lib.call("pl_tile_blend_labels_u8", ctx.handle, outs.ptr, y8.ptr, *bargs, 0.0)      # noqa: E731
    else:
        y8 = hip.empty((bg.OH, bg.OW, 3), np.uint8, ctx=ctx)
        kk, bb = spec._affine(3)
        blend = lambda: _lib.call("pl_tile_blend_u8", ctx.handle, outs.ptr, y8.ptr, *bargs, 3, None, 1, kk, bb, 0)  # noqa: E731
    gather_ms = events(lambda: feed.decode_into(stack.ptr))
    blend_ms = events(blend)
    blend_f32_ms = events(lambda: _lib.call("pl_tile_blend_f32", ctx.handle, outs.ptr, y32.ptr, *bargs))
    line["kernels_same_as_surface"] = bool((y8.get() == util.blend_windows(outs, geo.windows, kscale, geo.margin, geo.work, spec).get()).all())
    out_px = bg.OH * bg.OW
    gather_bytes = stack.size * 5                          # a byte read and a float written per element
    blend_bytes = outs.nbytes + out_px * (1 if args.child == "fpn" else 3)
    line["kernels"] = {
        "gather_ms": round(gather_ms, 4), "gather_bytes": gather_bytes, "gather_ms_at_8_tb_s": round(gather_bytes / HBM_TB_S / 1e9, 4),
        "blend_ms": round(blend_ms, 4), "blend_bytes": blend_bytes, "blend_ms_at_8_tb_s": round(blend_bytes / HBM_TB_S / 1e9, 4),
        "blend_to_float32_ms": round(blend_f32_ms, 4),
        "resident_window_results_bytes": outs.nbytes}
    line["streams"] = sorted({str(getattr(p, "streams", None)) for p in net._plans.values()})
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", default="fpn,edsr")
    ap.add_argument("--scan", type=int, default=4096)
    ap.add_argument("--photo", type=int, default=1024)
    ap.add_argument("--batch-fpn", type=int, default=9)
    ap.add_argument("--batch-edsr", type=int, default=1,
                    help="(the tail conv reads 64 planes of 2048 x 2048: two windows would pass the conv kernels' 2 GiB input limit)")
    ap.add_argument("--timeout", type=int, default=420, help="seconds one child process may take")
    ap.add_argument("--child", choices=["fpn", "edsr"])
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = []
    for name in [w for w in args.workloads.split(",") if w]:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", name,
               "--rounds", str(args.rounds), "--scan", str(args.scan), "--photo", str(args.photo),
               "--batch-fpn", str(args.batch_fpn), "--batch-edsr", str(args.batch_edsr)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:                              # the first failing step ends the run: nothing more is started
            sys.exit("workload %s failed (exit %d):\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-3000:]))
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                lines.append(json.loads(ln))
                print(ln, flush=True)
    out = {"dtype": "fp32", "rounds": args.rounds}
    for ln in lines:
        w = ln["workload"]
        out[w + "_new_over_old_host_to_host"] = round(ln["median_old_ms"] / ln["median_new_ms"], 2)
        out[w + "_new_over_old_device_resident"] = round(ln["median_old_dev_ms"] / ln["median_new_dev_ms"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

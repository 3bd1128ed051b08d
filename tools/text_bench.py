"""What a caller who wants TEXT back gets from a line recogniser, fp32 on one GPU.
  crnn-C-text        the CRNN of irgen/crnn.py (two bidirectional LSTMs), batch 32, 32 x 320 in, C classes, host float32 batches
                     through net.submit, Net.text_output: text, length, conf, spans come back               (pl_ctc_greedy_f32)
  crnn-C-float       the same net handing back its float32 (80, 32, C) logits: the pass with the download and nothing else
  crnn-C-float-host  the logits, then the caller's numpy step in the loop: argmax(-1), the max-shifted softmax of the frames,
                     and a Python loop per line that merges repeats and drops blanks
for C = 37 and 6625.  Every arm run is a FRESH process under a timeout of its own; the arms alternate --rounds times and share one
tuning cache.  Then the chain alone (one more process): HIP events around --launches calls of pl_ctc_greedy_f32 on (80, 32, 37)
and (80, 32, 6625) "tnc" and on (32, 6625, 1, 80) "nchw", beside a one-frame call (the launch floor).  With --trace that process
runs once more under rocprofv3 --kernel-trace and the median device time of each launch is reported per input, the frame pass also
as bytes read per second and as a share of 8 TB/s; and one CRNN forward (37 classes) runs under a kernel trace of its own, from
which the share of the LSTM steps -- every lstm_step_fused_kernel, or every lstm_cell_kernel and the h R^T GEMM in
front of it -- in the kernels of one pass is read.  --lstm per-step runs the CRNN arms and the traced forward with
PLANER_HIP_LSTM_FUSED=0 (the per-step program), --lstm both runs every arm in both programs, alternating inside each round; the
per-step lines and summary keys carry "@per-step".
One JSON line per step as it ends, then one summary line.  The tool stops at the first step that fails.
    python tools/text_bench.py [--rounds 2] [--passes 40] [--arms ...] [--no-kernels] [--trace [all|chain|lstm]] [--lstm fused|per-step|both]
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
CLASSES = (37, 6625)
ARMS = ["crnn-%d-%s" % (c, how) for c in CLASSES for how in ("text", "float", "float-host")]
BATCH, SIZE, FRAMES, MAX_LEN = 32, (32, 320), 80, 64
HBM_BYTES_S = 8e12
PER_STEP = "@per-step"          # suffix of an arm run with PLANER_HIP_LSTM_FUSED=0
FUSED_ENV = {"fused": "1", "per-step": "0"}


def host_decode(logits):
    """The caller's numpy step on float32 (T, N, C) logits: (text, length, conf) as lists per line."""
    best = logits.argmax(-1)                                                  # (T, N)
    top = np.take_along_axis(logits, best[..., None], -1)
    conf = 1.0 / np.exp(logits - top).sum(-1)                                 # (T, N)
    texts, confs = [], []
    for n in range(logits.shape[1]):
        line, cs, prev = [], [], -1
        for t in range(logits.shape[0]):
            lab = best[t, n]
            if lab != prev and lab != 0:
                line.append(int(lab))
                cs.append(float(conf[t, n]))
            prev = lab
        texts.append(line[:MAX_LEN])
        confs.append(cs[:MAX_LEN])
    return texts, [len(t) for t in texts], confs


def crnn_net(classes):
    sys.path.insert(0, HERE)
    import planer_amd
    from planer_amd.irgen import crnn
    g, blob = crnn.build(classes=classes, channels=3, batch=BATCH)
    return planer_amd, planer_amd.from_graph(g, blob), crnn


def arm_child(args):
    _, classes, how = args.arm.split("-", 2)
    planer_amd, net, crnn = crnn_net(int(classes))
    if how == "text":
        net.text_output("tnc", max_len=MAX_LEN)
    line = {"arm": args.arm + ("" if planer_amd.layer.lstm_fused_enabled() else PER_STEP), "round": args.round}
    batches = [crnn.make_input(BATCH, seed=s, size=SIZE, channels=3) for s in (1, 2)]
    window, pend = 6, collections.deque()

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
    host_loop(8)
    line["compile_and_warm_s"] = round(time.perf_counter() - t0, 2)
    line["captured"] = bool(net.use_graph)
    host_loop(8)
    finish = host_decode if how == "float-host" else None
    t0 = time.perf_counter()
    got = host_loop(args.passes, finish)
    line["img_s"] = round(BATCH * args.passes / (time.perf_counter() - t0), 1)
    seq = got if isinstance(got, tuple) else (got,)
    line["output_bytes_per_batch"] = int(sum(a.nbytes for a in seq))
    ts = []
    for i in range(3 + args.calls):
        t0 = time.perf_counter()
        got = net(batches[i & 1])
        ts.append(time.perf_counter() - t0)
    line["net_call_ms"] = round(sorted(ts[3:])[args.calls // 2] * 1e3, 3)
    if how == "float-host":
        t0 = time.perf_counter()
        line["symbols_per_batch"] = int(sum(host_decode(got)[1]))
        line["host_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3, 1)
    elif how == "text":
        line["symbols_per_batch"] = int(got[1].sum())
    ctx = planer_amd.hip.context()
    if ctx.tune_cache:
        ctx.save_tune_cache()
    print(json.dumps(line), flush=True)


def inputs():
    """[(name, layout, float32 tensor)]: a one-frame call, then the three tensors of the issue."""
    rng = np.random.default_rng(4)
    return [("one frame", "tnc", rng.standard_normal((1, 1, 37)).astype(np.float32)),
            ("tnc (80, 32, 37)", "tnc", rng.standard_normal((FRAMES, BATCH, 37)).astype(np.float32)),
            ("tnc (80, 32, 6625)", "tnc", rng.standard_normal((FRAMES, BATCH, 6625)).astype(np.float32)),
            ("nchw (32, 6625, 1, 80)", "nchw", rng.standard_normal((BATCH, 6625, 1, FRAMES)).astype(np.float32))]


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
    floor = None
    for name, layout, host in inputs():
        for confidence in ("softmax", "none"):
            spec = util.TextSpec(layout, confidence=confidence, max_len=MAX_LEN)
            lead, n, inner, t, c, st = spec.geometry(host.shape)
            x = hip.asarray(host)
            s = n * inner
            outs = (hip.empty(lead + (MAX_LEN,), np.int32, ctx=ctx), hip.empty(lead, np.int32, ctx=ctx),
                    hip.empty(lead + (MAX_LEN,), np.float32, ctx=ctx), hip.empty(lead + (MAX_LEN, 2), np.int32, ctx=ctx))
            scratch = hip.empty((s * t,), np.int64, ctx=ctx)
            fn = lambda: _lib.call("pl_ctc_greedy_f32", ctx.handle, x.ptr, n, inner, t, c, st[0], st[1], st[2], st[3], None, 0, 1,   # noqa: E731
                                   _lib.TEXT_CONF[confidence], MAX_LEN, scratch.ptr, *[a.ptr for a in outs])
            sec = timed(fn, args.launches)
            if floor is None:
                floor = sec
            print(json.dumps({"kernel": "pl_ctc_greedy_f32", "input": name, "confidence": confidence, "shape": list(host.shape),
                              "us": round(sec * 1e6, 2), "launch_floor_us": round(floor * 1e6, 2), "symbols": int(outs[1].get().sum()),
                              "input_GB_s_whole_chain": round(host.nbytes / sec / 1e9, 1)}), flush=True)


def chain_calls(launches):
    """Calls of the chain the kernels step makes for one input and one confidence: 3 to warm up, then 3 timings."""
    return 3 + 3 * launches


def forward_child(args):
    """A few passes of the 37-class CRNN from a device batch: the last one is what the trace digest reads.  One stream and one
    graph, by name: under the tracer nothing is to be measured or picked, so no multi-stream candidate plan is built there (the
    parent also runs this child once untraced first, which fills the tuning cache with the conv picks)."""
    planer_amd, net, crnn = crnn_net(37)
    net.streams = "1x1"
    x = planer_amd.asarray(crnn.make_input(BATCH, size=SIZE, channels=3))
    for _ in range(5):
        net(x)
    ctx = planer_amd.hip.context()
    ctx.synchronize()
    if ctx.tune_cache:
        ctx.save_tune_cache()
    print(json.dumps({"forward": "crnn-37", "captured": bool(net.use_graph), "tune_source": net.tune_source(),
                      "lstm_fused": planer_amd.layer.lstm_fused_enabled()}), flush=True)


def read_trace(directory):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows]


def chain_digest(directory, launches):
    """Median device time in us of each launch of the chain, per input and confidence: the chains in launch order (each ends
    with collapse_kernel), dealt out by the number of calls the kernels step makes."""
    chains, cur = [], []
    for name, t0, t1 in read_trace(directory):
        if "text::" not in name:
            continue
        short = name.split("text::")[1].split("(")[0].split("<")[0]
        cur.append((short, (t1 - t0) / 1e3))
        if short == "collapse_kernel":
            chains.append(cur)
            cur = []
    out, at = collections.OrderedDict(), 0
    for name, _, host in inputs():
        for confidence in ("softmax", "none"):
            mine, at = chains[at:at + chain_calls(launches)], at + chain_calls(launches)
            per = collections.OrderedDict()
            for c in mine:
                for kernel, us in c:
                    per.setdefault(kernel, []).append(us)
            d = {k: round(sorted(v)[len(v) // 2], 2) for k, v in per.items()}
            frame = [k for k in d if k != "collapse_kernel"]
            if frame:
                rate = host.nbytes / d[frame[0]] / 1e3                        # GB/s
                d["frame_pass_read_GB_s"] = round(rate, 1)
                d["frame_pass_share_of_8_TB_s"] = round(rate * 1e9 / HBM_BYTES_S, 3)
            out["%s, %s" % (name, confidence)] = d
    out["chains_in_trace"], out["chains_expected"] = len(chains), at
    return out


def lstm_fused_digest(rows):
    """The fused program: a step of a whole LSTM op (both directions) is one lstm_step_fused_kernel, 2 x 80 of them a pass."""
    steps = [i for i, r in enumerate(rows) if "lstm_step_fused_kernel" in r[0]]
    per_pass = 2 * FRAMES
    if len(steps) < 2 * per_pass:
        return {"error": "%d fused step kernels in the trace, fewer than two passes" % len(steps)}
    k = steps[-1] - steps[-1 - per_pass]
    last = rows[len(rows) - k:]
    mine = [i for i, r in enumerate(last) if "lstm_step_fused_kernel" in r[0]]
    if len(mine) != per_pass:
        return {"error": "%d fused step kernels in the last %d kernels, expected %d" % (len(mine), k, per_pass)}
    busy = sum(t1 - t0 for _, t0, t1 in last)
    inside = sum(last[i][2] - last[i][1] for i in mine)
    spans = [last[mine[(op + 1) * FRAMES - 1]][2] - last[mine[op * FRAMES]][1] for op in range(2)]
    wall = last[-1][2] - last[0][1]
    return {"kernels_per_pass": k, "fused_step_kernels_per_pass": len(mine), "lstm_step_launches": len(mine),
            "pass_wall_us": round(wall / 1e3, 1), "pass_busy_us": round(busy / 1e3, 1),
            "lstm_steps_busy_us": round(inside / 1e3, 1), "lstm_steps_share_of_busy": round(inside / busy, 3),
            "lstm_step_us": round(inside / len(mine) / 1e3, 2),
            "lstm_ops_wall_us": round(sum(spans) / 1e3, 1), "lstm_ops_share_of_wall": round(sum(spans) / wall, 3)}


def lstm_digest(directory):
    """The last pass of the forward child: its kernels are the last K of the trace, K the distance between two cell kernels
    that are one pass (2 LSTMs x 2 directions x 80 steps) apart.  A step is a cell kernel and the h R^T GEMM in front of it:
    every kernel since the cell of the step before (however many launches the GEMM takes), and for a direction's first step the
    one kernel in front.  `step_gemm_kernels` names what was counted as such a GEMM."""
    rows = read_trace(directory)
    if any("lstm_step_fused_kernel" in r[0] for r in rows):
        return lstm_fused_digest(rows)
    cells = [i for i, r in enumerate(rows) if "lstm_cell_kernel" in r[0]]
    per_pass = 2 * 2 * FRAMES
    if len(cells) < 2 * per_pass:
        return {"error": "%d cell kernels in the trace, fewer than two passes" % len(cells)}
    k = cells[-1] - cells[-1 - per_pass]
    last = rows[len(rows) - k:]
    busy = sum(t1 - t0 for _, t0, t1 in last)
    mine = [i for i, r in enumerate(last) if "lstm_cell_kernel" in r[0]]
    if len(mine) != per_pass:
        return {"error": "%d cell kernels in the last %d kernels, expected %d" % (len(mine), k, per_pass)}
    steps, gemms, launches = 0, collections.Counter(), 0
    for j, i in enumerate(mine):
        inside = j % FRAMES != 0                                              # not the first step of a direction
        front = range(mine[j - 1] + 1, i) if inside else range(max(i - 1, 0), i)
        for f in list(front) + [i]:
            steps += last[f][2] - last[f][1]
            launches += 1
            if f != i:
                gemms[last[f][0].split("(")[0][-60:]] += 1
    spans = []                                                                # wall time of each LSTM op: its first GEMM to its last cell
    for op in range(2):
        part = mine[op * 2 * FRAMES:(op + 1) * 2 * FRAMES]
        spans.append(last[part[-1]][2] - last[max(part[0] - 1, 0)][1])
    wall = last[-1][2] - last[0][1]
    return {"kernels_per_pass": k, "cell_kernels_per_pass": len(mine), "lstm_step_launches": launches, "step_gemm_kernels": dict(gemms),
            "pass_wall_us": round(wall / 1e3, 1), "pass_busy_us": round(busy / 1e3, 1),
            "lstm_steps_busy_us": round(steps / 1e3, 1), "lstm_steps_share_of_busy": round(steps / busy, 3),
            "lstm_ops_wall_us": round(sum(spans) / 1e3, 1), "lstm_ops_share_of_wall": round(sum(spans) / wall, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--passes", type=int, default=40, help="submits per timed loop")
    ap.add_argument("--calls", type=int, default=5, help="net(x) calls timed")
    ap.add_argument("--launches", type=int, default=30, help="calls between the two events of a chain timing")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--trace", nargs="?", const="all", default=None, choices=["all", "chain", "lstm"],
                    help="under rocprofv3 --kernel-trace: the kernels step once more (chain), one CRNN forward (lstm), or both")
    ap.add_argument("--lstm", default="fused", choices=["fused", "per-step", "both"],
                    help="the LSTM program of the CRNN arms and of the traced forward (PLANER_HIP_LSTM_FUSED); both: alternating")
    ap.add_argument("--cache", default=None, help="tuning cache file every process loads and saves")
    ap.add_argument("--timeout", type=int, default=300, help="seconds one child process may take")
    ap.add_argument("--child", choices=["arm", "kernels", "forward"])
    ap.add_argument("--arm")
    ap.add_argument("--round", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return {"arm": arm_child, "kernels": kernels_child, "forward": forward_child}[args.child](args)
    tmp = tempfile.TemporaryDirectory()
    if args.cache is None:
        args.cache = os.path.join(tmp.name, "tune.json")
    env = dict(os.environ, PLANER_HIP_TUNE_CACHE=os.path.abspath(args.cache))
    common = ["--passes", str(args.passes), "--calls", str(args.calls), "--launches", str(args.launches)]

    modes = ["fused", "per-step"] if args.lstm == "both" else [args.lstm]

    def step(extra, wrap=(), mode=None):
        """mode: the LSTM program of a child that runs the CRNN (arm, forward); the chain children run no LSTM and get none"""
        cmd = ["timeout", "-k", "10", str(args.timeout)] + list(wrap) + [sys.executable, os.path.abspath(__file__)] + extra + common
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(env, PLANER_HIP_LSTM_FUSED=FUSED_ENV[mode]) if mode else env)
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
            for mode in modes:
                runs += step(["--child", "arm", "--arm", arm, "--round", str(rnd)], mode=mode)
    kernels = [] if args.no_kernels else step(["--child", "kernels"])
    out = {"dtype": "fp32", "rounds": args.rounds, "passes": args.passes, "batch": BATCH, "size": list(SIZE), "arms": {}, "kernels": kernels}
    if args.trace in ("all", "chain"):
        d = os.path.join(tmp.name, "trace")
        step(["--child", "kernels"], wrap=["rocprofv3", "--kernel-trace", "-d", d, "-o", "text", "--output-format", "csv", "--"])
        out["trace"] = chain_digest(d, args.launches)
        print(json.dumps({"trace": out["trace"]}), flush=True)
    if args.trace in ("all", "lstm"):
        digests = {}
        for rnd in range(args.rounds if len(modes) > 1 else 1):
            for mode in modes:
                d = os.path.join(tmp.name, "forward-%s-%d" % (mode, rnd))
                step(["--child", "forward"], mode=mode)    # untraced first: the conv picks are measured here, not under the tracer
                step(["--child", "forward"], wrap=["rocprofv3", "--kernel-trace", "-d", d, "-o", "crnn", "--output-format", "csv", "--"],
                     mode=mode)
                digest = lstm_digest(d)
                digests.setdefault(mode, []).append(digest)
                print(json.dumps({"lstm": digest, "program": mode, "round": rnd}), flush=True)
        # one program: the digest itself, as before; --lstm both: {program: [a digest per round]}
        out["lstm"] = digests if len(modes) > 1 else digests[modes[0]][0]
    med = lambda v: sorted(v)[len(v) // 2] if v else None        # noqa: E731
    for arm in [a + ("" if m == "fused" else PER_STEP) for a in arms for m in modes]:
        mine = [r for r in runs if r["arm"] == arm]
        keys = [k for k, v in mine[0].items() if isinstance(v, (int, float)) and not isinstance(v, bool) and k != "round"]
        out["arms"][arm] = {"median_" + k: med([r[k] for r in mine]) for k in keys}
    print(json.dumps(out))
    tmp.cleanup()


if __name__ == "__main__":
    main()

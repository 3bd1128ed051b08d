"""pl_topk_select_f32 against pl_topk_f32 (largest = 1) over a grid of shapes: which one layer.topk_select_eligible
should take.  One process; per shape each arm is warmed up, then the two alternate for --rounds rounds, each timing HIP events
around enough calls to fill --fill seconds (from the warm-up's own time; at least one).  An arm whose single call takes more than
--slow seconds is timed once, in the first round only, and pl_topk_f32 is not run at all where its k selection rounds would
read more than --sort-max-work elements per row (one workgroup, many seconds).  Rows are seeded normals with a fifth of the
entries set to -1, the score of a non-candidate in a detection row.  One JSON line per shape, appended to --lines as well.
    python tools/topk_bench.py [--rows 1,8,300] [--n 1000,4096,...] [--k 5,100,1024,4096]"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,8,300")
    ap.add_argument("--n", default="1000,4096,10647,16384,25200,65537,1048576")
    ap.add_argument("--k", default="5,100,1024,4096")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fill", type=float, default=0.2)
    ap.add_argument("--slow", type=float, default=1.0)
    ap.add_argument("--sort-max-work", type=int, default=1 << 28)
    ap.add_argument("--lines", default=os.path.join(HERE, "profiles", "topk_select_lines.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from planer_amd import _lib, hip, util
    ctx = hip.context()
    rng = np.random.default_rng(0)

    def timed(fn, reps):
        e0 = hip.Event(ctx).record()
        for _ in range(reps):
            fn()
        e1 = hip.Event(ctx).record()
        return e0.elapsed_ms(e1) / reps * 1e3

    for n in (int(v) for v in args.n.split(",")):
        for rows in (int(v) for v in args.rows.split(",")):
            host = rng.standard_normal((rows, n)).astype(np.float32)
            host[rng.random((rows, n)) < 0.2] = -1
            x = hip.asarray(host)
            for k in (int(v) for v in args.k.split(",")):
                if k > n:
                    continue
                vals, idx = hip.empty((rows, k)), hip.empty((rows, k), np.int64)
                scratch = hip.empty((util._topk_select_scratch_bytes(rows, n, k) // 8 + 1,), np.int64)
                arms = {"sort": lambda: _lib.call("pl_topk_f32", ctx.handle, x.ptr, rows, n, 1, k, 1, vals.ptr, idx.ptr),
                        "select": lambda: _lib.call("pl_topk_select_f32", ctx.handle, x.ptr, rows, n, 1, k, scratch.ptr, vals.ptr, idx.ptr)}
                if n > 16384 and n * k > args.sort_max_work:
                    del arms["sort"]
                line = {"rows": rows, "n": n, "k": k}
                reps = {}
                for name, fn in arms.items():
                    first = timed(fn, 1)                                # (also the warm-up)
                    reps[name] = 0 if first > args.slow * 1e6 else max(1, min(2000, int(args.fill * 1e6 / first)))
                    line[name + "_us"] = [round(first, 1)] if not reps[name] else []
                    if reps[name]:
                        timed(fn, reps[name])
                for _ in range(args.rounds):
                    for name, fn in arms.items():
                        if reps[name]:
                            line[name + "_us"].append(round(timed(fn, reps[name]), 1))
                line["reps"] = reps
                text = json.dumps(line)
                print(text, flush=True)
                with open(args.lines, "a") as f:
                    f.write(text + "\n")


if __name__ == "__main__":
    main()

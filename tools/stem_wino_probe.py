#!/usr/bin/env python
"""ResNet-18's stem + max-pool at batch 32 (3 -> 64, 7x7 / s2 / p3 on 224x224, scale + shift + ReLU, pool 3x3 / s2 / p1): device time
of the NCHW-reading kernel in its direct form (K = 148) against the polyphase F(4,4) form (7 GEMMs of K = 44), for strips of 7
and of 14 pooled rows.  `--reps N --form direct|wino` runs one form N times (for a rocprofv3 pass)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import planer_amd as pa  # noqa: E402
from planer_amd import hip, q4  # noqa: E402
from tools.wino_chain_bench import timed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=0)
ap.add_argument("--form", default="wino")
args = ap.parse_args()
ctx = hip.context()
rng = np.random.default_rng(0)
x = pa.asarray(rng.standard_normal((args.batch, 3, 224, 224)).astype(np.float32))
K = pa.asarray((rng.standard_normal((64, 3, 7, 7)) * 0.1).astype(np.float32))
Kd, Kw = q4.prepare_stem_nchw_weights(K), q4.prepare_stem_wino_weights(K)
sc = pa.asarray(rng.uniform(0.5, 1.5, (1, 64, 1, 1)).astype(np.float32))
para = dict(strides=[2, 2], pads=[3, 3, 3, 3], dilations=[1, 1], group=1, w_layout=12, act=1)
out = q4.ConvPoolQ4(x, Kd, None, sc, sc, **para)
forms = {"direct": lambda rows: q4.ConvPoolQ4(x, Kd, None, sc, sc, out=out, strip_rows=rows, **para),
         "wino": lambda rows: q4.ConvPoolQ4(x, Kw, None, sc, sc, out=out, strip_rows=rows, wino=44, **para)}
if args.reps:
    for _ in range(args.reps):
        forms[args.form](7)
    ctx.synchronize()
else:
    for rows in (7, 14):
        for name, fn in forms.items():
            t = timed(ctx, lambda: fn(rows))
            print("batch %d strip_rows %2d %-6s %7.1f us  [%s]" % (args.batch, rows, name, t, ctx.last_conv_plan()))

#!/usr/bin/env python
"""Writes tests/golden/tile_net.npz: what the REFERENCE's own util.tile does on the geometries of tests/tile_net_ref.py CASES.
`f` hands back pre-drawn window results in call order (multiples of 0.5 with NaN, +-inf and -0.0 among them; scaled by the
sized by the case's k), so the fixture holds, per case: the image, the windows `f` was given (the resampled cases only), the
results it returned, the blended output and the progress calls.  Arrays only.

    python tools/capture_tile_net_golden.py <directory that holds the reference's `planer` package>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)
CHANNELS, RESULT_CHANNELS = 2, 2


def draw(rng, shape):
    x = (rng.integers(-8, 9, shape) / 2).astype(np.float32)
    where = rng.random(shape) < 0.03
    x[where] = SPECIALS[rng.integers(0, len(SPECIALS), int(where.sum()))]
    x[shape[0] // 2, shape[1] // 2, 0] = -0.0          # a window's centre: where one window covers it, the -0.0 must come through
    return x


def main():
    from tests.tile_net_ref import CASES
    sys.path.insert(0, sys.argv[1])
    from planer import util
    store = {}
    for i, (name, case) in enumerate(CASES.items()):
        rng = np.random.default_rng(9100 + i)
        img = rng.integers(0, 256, case["size"] + (CHANNELS,)).astype(np.float32)
        k, wins, rsts, calls = case["k"], [], [], []

        def f(win):
            wins.append(np.array(win, np.float32))
            rsts.append(draw(rng, (int(win.shape[0] * k), int(win.shape[1] * k), RESULT_CHANNELS)))
            return rsts[-1]
        with np.errstate(all="ignore"):
            out = util.tile(progress=lambda a, b: calls.append((a, b)), **case["tile"])(f)(img)
        assert out.dtype == np.float32, out.dtype
        store[name + "/img"] = img.astype(np.uint8)
        if "sample" in case["tile"] or "glob" in case["tile"]:      # (elsewhere the windows are plain cuts of the image)
            store[name + "/wins"] = np.stack(wins)
        store[name + "/rsts"] = np.stack(rsts)
        store[name + "/out"] = out
        store[name + "/progress"] = np.asarray(calls, np.int32).reshape(-1, 2)
        print(name, img.shape, "->", len(wins), "windows of", wins[0].shape, "->", rsts[0].shape, "->", out.shape)
    path = os.path.join(ROOT, "tests", "golden", "tile_net.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Writes tests/golden/image_input.npz: a handful of seeded uint8 images (none larger than 40 x 56 x 4) and the REFERENCE's
util.resize outputs for them -- down-scale, up-scale, mixed, C = 1, 3 and 4.  Arrays only.

    python tools/capture_image_input_golden.py <directory that holds the reference's `planer` package>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (H, W, C), (OH, OW)
CASES = {
    "down_rgb": ((37, 53, 3), (24, 40)),
    "up_rgb": ((9, 13, 3), (31, 29)),
    "mixed_rgb": ((40, 11, 3), (17, 36)),         # rows down, columns up
    "mixed_rgba": ((12, 56, 4), (33, 20)),        # rows up, columns down
    "down_gray": ((33, 41, 1), (16, 20)),
    "up_rgba": ((5, 7, 4), (8, 12)),
    "two_by_two": ((2, 2, 3), (5, 8)),            # the smallest image the index rule takes
    "same_width": ((21, 16, 3), (13, 16)),
}


def main():
    sys.path.insert(0, sys.argv[1])
    from planer import util
    store = {}
    for i, (name, (shape, size)) in enumerate(CASES.items()):
        rng = np.random.default_rng(7100 + i)
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        img.flat[:4] = (0, 255, 1, 254)[:img.size][:4]
        out = util.resize(img, size)
        assert out.dtype == np.float32 and out.shape == tuple(size) + shape[2:], (out.dtype, out.shape)
        store[name + "/img"] = img
        store[name + "/size"] = np.asarray(size, np.int32)
        store[name + "/out"] = out
    path = os.path.join(ROOT, "tests", "golden", "image_input.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

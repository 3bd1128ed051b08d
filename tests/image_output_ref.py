"""numpy mirrors of the uint8 outputs (pl_image_f32_u8, pl_labels_f32_u8).  Equality with the kernels is bit for
bit: every step of `encode32` is a float32 operation rounded on its own, and `labels` is numpy's argmax itself.

The header of the tile constants is read here, so the GPU tests cut their shapes from what the library was built with."""
import re

import numpy as np

from tests.conftest import ROOT
from tests.image_input_ref import same_bits          # noqa: F401  (reused by the tests of this feature)


def tile_constants():
    """(PL_IMAGE_OUT_TILE_PIXELS, PL_IMAGE_OUT_LANE_PIXELS) as include/planer_hip.h defines them."""
    text = open(ROOT + "/include/planer_hip.h").read()
    got = {k: int(v) for k, v in re.findall(r"#define PL_IMAGE_OUT_(TILE_PIXELS|LANE_PIXELS) (\d+)", text)}
    return got["TILE_PIXELS"], got["LANE_PIXELS"]


def encode32(x, k, b, layout="nhwc", order=None, trunc=False):
    """float32 (N, C, H, W) -> uint8 (N, H, W, Co) or (N, Co, H, W): t = fl(fl(v k[c]) + b[c]) on plane order[c], NaN -> 0,
    clipped to [0, 255], np.rint (ties to even) or truncation.  One value in k and b serves every channel."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4
    k, b = np.atleast_1d(np.asarray(k, np.float32)), np.atleast_1d(np.asarray(b, np.float32))
    v = x if order is None else x[:, list(order)]
    with np.errstate(invalid="ignore", over="ignore"):
        t = v * k[None, :, None, None] + b[None, :, None, None]
        assert t.dtype == np.float32
        t = np.where(np.isnan(t), np.float32(0), np.clip(t, np.float32(0), np.float32(255)))
    y = (t if trunc else np.rint(t)).astype(np.uint8)
    return np.ascontiguousarray(y.transpose(0, 2, 3, 1)) if layout == "nhwc" else y


def labels(x, threshold=0.0):
    """float32 (N, C, H, W) -> uint8 (N, H, W): np.argmax over the planes, x > threshold where there is one plane."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4 and 1 <= x.shape[1] <= 256
    if x.shape[1] == 1:
        with np.errstate(invalid="ignore"):
            return (x[:, 0] > np.float32(threshold)).astype(np.uint8)
    return np.argmax(x, axis=1).astype(np.uint8)

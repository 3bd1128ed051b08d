"""The non-finite contract of tests/nonfinite_ref.py on implementations that exist on the CPU: every case and plant of
tests/test_gpu_conv_nonfinite.py through the float32 oracle conv (oracle/planer_np) with a float32 tail for the direct families and
through `ref64.wino_emulate(dtype=float32)` for the Winograd ones.  A correct float32 implementation meets R1 - R4 on exactly these
inputs, and the mask code runs here without a GPU.  Three emulations with one deliberate bug each show that the rules bite."""
import numpy as np
import pytest

from tests import nonfinite_ref as NF
from tests import ref64 as R
from tests.nonfinite_ref import CASES


def _cpu(case, raw=None, edit=None):
    def run(ops, act, what):
        ops = edit(ops) if edit else ops
        return [np.ascontiguousarray(y, np.float32) for y in NF.compute(case, ops, act, np.float32, case.fam != "direct", raw)]
    return run


def test_masks_on_the_worked_example():
    """(2, 8, 9, 13) -> 12 channels, pad 1, one plant at (1, 3, 4, 6): the 3x3 receptive field in every output channel; under a ReLU
    tail a +inf gives NaN where the filter value is negative; whole tiles for the Winograd families, each holding the field."""
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 8, 9, 13)).astype(np.float32)
    K = rng.standard_normal((12, 8, 3, 3)).astype(np.float32)
    field = np.zeros((2, 12, 9, 13), bool)
    field[1, :, 3:6, 5:8] = True
    for v in NF.VALUES.values():
        xp = x.copy()
        xp[1, 3, 4, 6] = v
        ref = R.ref64(xp, K, pads=[1, 1, 1, 1])
        assert ((~np.isfinite(ref)) == field).all() and field.sum() == 108
        for fam, count in (("f2x2", 192), ("f4x4", 384), ("wino43", 384), ("w1d4", 144)):
            with np.errstate(invalid="ignore"):
                tiles = ~np.isfinite(R.wino_emulate(xp, K, *R.wino_family(fam, 9, 13), dtype=np.float64))
            assert tiles.sum() == count and tiles[field].all(), (fam, tiles.sum())
    xp[1, 3, 4, 6] = np.inf
    with np.errstate(invalid="ignore"):
        cls = NF.classes(R.ref64(xp, K, act=R.ACT_RELU, pads=[1, 1, 1, 1]))
    neg = (K[:, 3, ::-1, ::-1] < 0).sum()
    assert (cls == 1).sum() == neg and (cls == 2).sum() == 108 - neg and (cls == 3).sum() == 0


@pytest.mark.parametrize("name", list(CASES))
def test_float32_implementations_meet_the_contract(name):
    case = CASES[name]
    seen = set()
    count = NF.sweep(case, _cpu(case), seen=seen)
    have = {t for i in range(len(case.tails)) for t, a in zip(NF.TENSORS, case.operands(i)[0]) if a is not None}
    assert {"x", "K"} <= seen and seen == have, (name, seen, have)
    assert count >= 3 * len(NF.input_plants(case)) * len(case.intails)


# ---- negative controls ----------------------------------------------------------------------------------------------------------------
def _masked_border(case, x, K, dtype, wino, conv):
    """Padding taps served by a clamped load times a 0 mask: the padded cells hold 0 x (the nearest pixel), not 0.  Models the direct
    kernels' gathers (implicit GEMM NCHW / tap-major / channel-quad, row-packed, small-Cin, depthwise, the sibling pair, the
    transposed conv's phases) and the Winograd input transforms' loads at the map's edge."""
    from oracle import planer_np as onp
    p = case.conv["pads"]
    x = np.asarray(x, dtype)
    with np.errstate(invalid="ignore"):
        edge = np.pad(x, ((0, 0), (0, 0), (p[0], p[2]), (p[1], p[3])), mode="edge") * dtype(0)
        edge[:, :, p[0]:p[0] + x.shape[2], p[1]:p[1] + x.shape[3]] = x
        return np.ascontiguousarray(onp.conv2d(edge, np.asarray(K, dtype), None, **dict(case.conv, pads=[0, 0, 0, 0])))


def _tiles_across_images(case, x, K, dtype, wino, conv):
    """The tile grid laid over the batch as one tall map: a tile index flattened over (image, tile row) without the per-image
    padding, so the last tile row of an image reads the first rows of the next.  Models every kernel that flattens (image, tile row,
    tile column) or (image, row): the Winograd transforms and fused kernels, the GEMM pixel index of the direct kernels."""
    x = np.asarray(x, dtype)
    n, c, h, w = x.shape
    tall = x.transpose(1, 0, 2, 3).reshape(1, c, n * h, w)
    with np.errstate(invalid="ignore"):
        y = NF.wino_conv(tall, K, case.fam, dtype)
    return np.ascontiguousarray(y.reshape(K.shape[0], n, h, w).transpose(1, 0, 2, 3))


def _next_channels_bias(ops):
    """The bias of channel c + 1 added to channel c: a lane of apply_epilogue4 reading its neighbour's term.  Models every tail
    (apply_epilogue / apply_epilogue4 behind each conv kernel, the split-K reduce, the Winograd output transforms)."""
    ops = list(ops)
    ops[2] = np.roll(ops[2], -1)
    return tuple(ops)


def test_control_zero_mask_multiply_at_the_border_fails_r3():
    case = CASES["d_6to10"]
    NF.sweep(case, _cpu(case), tensors=("x",))
    with pytest.raises(AssertionError, match="R3 .*=\\+?-?inf"):
        NF.sweep(case, _cpu(case, raw=_masked_border), tensors=("x",))


def test_control_tile_grid_shifted_by_an_image_fails_r1():
    case = CASES["f4x4_3x16x9x13"]
    NF.sweep(case, _cpu(case), tensors=("x",))
    with pytest.raises(AssertionError, match="R1 "):
        NF.sweep(case, _cpu(case, raw=_tiles_across_images), tensors=("x",))


def test_control_bias_of_the_next_channel_fails_r1():
    case = CASES["d_6to10"]
    NF.sweep(case, _cpu(case), tensors=("B",))
    with pytest.raises(AssertionError, match="R1 .* B\\["):
        NF.sweep(case, _cpu(case, edit=_next_channels_bias), tensors=("B",))

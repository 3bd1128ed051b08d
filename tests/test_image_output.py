"""uint8 images and label maps as net output, the parts that need no GPU: the numpy mirrors on hand-written tables,
the round trip through image_affine / image_affine_inverse, the tile constants, and what the Python surface refuses before it
touches a device."""
import numpy as np
import pytest

from tests import image_input_ref as RI
from tests import image_output_ref as R

NAN, INF = float("nan"), float("inf")


def _col(values):
    """A row of samples as a (1, 1, 1, n) tensor."""
    return np.array(values, np.float32).reshape(1, 1, 1, -1)


def test_tile_constants_agree_everywhere():
    from planer_amd import _lib
    t, l = R.tile_constants()
    assert (t, l) == (_lib.IMAGE_OUT_TILE_PIXELS, _lib.IMAGE_OUT_LANE_PIXELS)
    assert t == 256 * l                                            # 256-thread workgroups, one lane per LANE pixels
    from tests import test_gpu_image_output as G
    assert (G.T, G.L) == (t, l)


def test_mirror_on_the_table():
    src = [-0.5, 0.5, 1.5, 2.5, 254.5, 255.5, 300, -INF, INF, NAN, -0.0]
    want = [0, 0, 2, 2, 254, 255, 255, 0, 255, 0, 0]
    for layout in ("nhwc", "nchw"):
        y = R.encode32(_col(src), [1], [0], layout)
        assert y.dtype == np.uint8 and y.ravel().tolist() == want
    below = np.nextafter(np.float32(255), np.float32(0))           # 254.99998
    assert R.encode32(_col([1.5, below, 255.0, 0.999]), [1], [0], trunc=True).ravel().tolist() == [1, 254, 255, 0]
    assert R.encode32(_col([1.5, below]), [1], [0]).ravel().tolist() == [2, 255]
    # k and b at work on a large operand: 2^24 (1 + 2^-23) = 2^24 + 2 exactly, minus 2^24
    assert R.encode32(_col([2.0 ** 24]), [1 + 2.0 ** -23], [-(2.0 ** 24)]).ravel().tolist() == [2]
    # layouts and order
    x = np.arange(2 * 3 * 2 * 2, dtype=np.float32).reshape(2, 3, 2, 2)
    assert R.encode32(x, [1] * 3, [0] * 3, "nhwc").shape == (2, 2, 2, 3)
    assert (R.encode32(x, [1] * 3, [0] * 3, "nchw") == x.astype(np.uint8)).all()
    assert (R.encode32(x, [1] * 3, [0] * 3, "nchw", order=(2, 1, 0)) == x[:, ::-1].astype(np.uint8)).all()
    assert (R.encode32(x, [1] * 3, [0] * 3, "nhwc")[1, 0, 1] == x[1, :, 0, 1]).all()
    assert (R.encode32(x, [2, 1], [0, 1], "nchw", order=(1, 1))[:, 0] == 2 * x[:, 1]).all()


def test_round_trip_of_every_byte():
    from planer_amd.util import image_affine, image_affine_inverse
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    r = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :, None], (1, 1, 256, 3)).copy()      # (N, H, W, C)
    x = RI.decode32(r, *image_affine(mean, std))
    k, b = image_affine_inverse(mean, std)
    assert k.dtype == np.float32 and b.dtype == np.float32
    for c in range(3):
        assert k[c] == np.float32(255.0 * std[c]) and b[c] == np.float32(255.0 * mean[c])
    assert (R.encode32(x, k, b) == r).all()
    t = x.astype(np.float64) * k.astype(np.float64)[None, :, None, None] + b.astype(np.float64)[None, :, None, None]
    worst = np.abs(t - r.transpose(0, 3, 1, 2)).max()
    print("worst |t - r| = %.3g" % worst)
    # four roundings (two in the decode, k and b of the inverse) of magnitudes up to 255, and the two in the folded constants
    assert worst <= 8 * RI.U * 255                                  # 1.2e-4: far from the tie at 0.5
    kept = (R.encode32(x, k, b, trunc=True) == r).mean()
    print("truncate keeps %.1f %% of the bytes" % (100 * kept))
    assert kept < 1.0                                               # which is why nearest is the default
    k1, b1 = image_affine_inverse(0, 1)
    assert k1.tolist() == [255.0] and b1.tolist() == [0.0]
    k2, b2 = image_affine_inverse([0.5, 0.25], 2.0, scale=2.0)      # a scalar std broadcasts
    assert k2.tolist() == [4.0, 4.0] and b2.tolist() == [1.0, 0.5]


def test_labels_mirror():
    rows = [[1, NAN, 3], [NAN, NAN, 0], [INF, INF, 1], [-0.0, 0.0, -1], [-INF, -INF, -INF]]
    x = np.array(rows, np.float32).T.reshape(1, 3, 1, 5)            # planes on axis 1, one pixel per row
    y = R.labels(x)
    assert y.dtype == np.uint8 and y.shape == (1, 1, 5) and y.ravel().tolist() == [1, 0, 0, 0, 0]
    above = np.nextafter(np.float32(0.25), np.float32(1))
    one = _col([0.25, above, NAN, -1.0, INF]).reshape(1, 1, 1, 5)
    assert R.labels(one, 0.25).ravel().tolist() == [0, 1, 0, 0, 1]
    assert R.labels(_col([0.0, -0.0, np.float32(1e-45), NAN])).ravel().tolist() == [0, 0, 1, 0]
    last = np.zeros((1, 256, 1, 2), np.float32)
    last[0, 255] = 1
    assert R.labels(last).ravel().tolist() == [255, 255]


def test_python_surface_refuses_without_a_device():
    from planer_amd import Net
    from planer_amd.util import ImageOutSpec, LabelSpec, encode_images, label_map
    one = np.ones(3, np.float32)
    with pytest.raises(ValueError, match="one value per output channel"):
        ImageOutSpec(np.ones(3), np.ones(2))
    with pytest.raises(ValueError, match="one value per output channel"):
        ImageOutSpec(np.ones(0), np.ones(0))
    with pytest.raises(ValueError, match="one value per output channel"):
        ImageOutSpec(np.ones(5), np.ones(5))
    with pytest.raises(ValueError, match="order"):
        ImageOutSpec(one, one, order=(0, -1, 2))
    with pytest.raises(ValueError, match="order"):
        ImageOutSpec(one, one, order=(0, 1))
    with pytest.raises(ValueError, match="order"):
        ImageOutSpec(1.0, 0.0, order=(0, 1, 2, 3, 4))
    with pytest.raises(ValueError, match="rounding"):
        ImageOutSpec(one, one, rounding="floor")
    with pytest.raises(ValueError, match="layout"):
        ImageOutSpec(one, one, layout="hwcn")
    with pytest.raises(ValueError, match="threshold"):
        LabelSpec(NAN)
    spec = ImageOutSpec(one, one, order=(2, 1, 0), layout="nchw", rounding="truncate")
    assert spec.geometry((2, 3, 5, 7)) == (2, 3, 5, 7, 3) and spec.geometry((2, 8, 5, 7)) == (2, 8, 5, 7, 3)
    with pytest.raises(ValueError, match="does not have"):
        spec.geometry((2, 2, 5, 7))
    with pytest.raises(ValueError, match="no order"):
        ImageOutSpec(one, one).geometry((1, 4, 5, 7))
    assert ImageOutSpec(255.0, 0.0).geometry((1, 3, 5, 7)) == (1, 3, 5, 7, 3)          # one value serves every channel
    assert ImageOutSpec(255.0, 0.0, order=(1, 0)).geometry((1, 3, 5, 7))[4] == 2
    with pytest.raises(ValueError, match="1 to 4 output channels"):
        ImageOutSpec(255.0, 0.0).geometry((1, 5, 5, 7))
    assert LabelSpec(0.25).geometry((2, 256, 3, 3)) == (2, 256, 3, 3)
    with pytest.raises(ValueError, match="256"):
        LabelSpec().geometry((2, 257, 3, 3))
    host = np.zeros((1, 3, 4, 4), np.float32)
    with pytest.raises(TypeError, match="got ndarray"):
        encode_images(host, one, one)                                # a host array: upload it first
    with pytest.raises(TypeError, match="got ndarray"):
        label_map(host)
    with pytest.raises(TypeError, match="got ndarray"):
        spec.encode(host)
    net = Net()
    with pytest.raises(ValueError, match="layout"):
        net.image_output(one, one, layout="chw")
    with pytest.raises(ValueError, match="index"):
        net.label_output(index=-1)
    assert net._image_out == {}
    assert net.image_output(one, one, index=1) is net and net._image_out[1].layout == "nhwc"
    assert net.label_output(0.5, index=1) is net and net._image_out[1].threshold == 0.5     # again: replaces
    assert net.float_output(index=1) is net and net._image_out == {}
    net.float_output()                                               # nothing declared: nothing to do

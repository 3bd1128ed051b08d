"""uint8 image input, the parts that need no GPU: the float32 restatement of util.resize on bytes against the
reference's own outputs (tests/golden/image_input.npz, tools/capture_image_input_golden.py) and against float64, image_affine's
values, and the refusals the Python surface makes before it touches a device."""
import re

import numpy as np
import pytest

from tests import image_input_ref as R
from tests.conftest import ROOT, load_golden


def golden_cases():
    z = load_golden("image_input.npz")
    return {n: (z[n + "/img"], tuple(int(v) for v in z[n + "/size"]), z[n + "/out"]) for n in sorted({k.split("/")[0] for k in z.files})}


def test_golden_covers_what_it_should():
    cases = golden_cases()
    assert {img.shape[2] for img, _, _ in cases.values()} == {1, 3, 4}
    kinds = set()
    for img, size, out in cases.values():
        assert img.dtype == np.uint8 and out.dtype == np.float32 and out.shape == size + img.shape[2:]
        assert img.shape[0] <= 40 and img.shape[1] <= 56 and img.shape[2] <= 4
        kinds.add((np.sign(size[0] - img.shape[0]), np.sign(size[1] - img.shape[1])))
    assert {(-1, -1), (1, 1), (-1, 1), (1, -1)} <= kinds              # down, up, mixed both ways


@pytest.mark.parametrize("name", sorted(golden_cases()))
def test_restatement_is_the_reference_bit_for_bit(name):
    img, size, out = golden_cases()[name]
    assert R.same_bits(R.resize32(img, size), out)


@pytest.mark.parametrize("name", sorted(golden_cases()))
def test_restatement_within_the_bound_of_float64(name):
    img, size, out = golden_cases()[name]
    c = img.shape[2]
    for k, b in ((np.ones(c), np.zeros(c)), R_affine(c)):
        y = R.decode32(img[None], k, b, size=size)
        y64, bound = R.decode64(img[None], k, b, size=size)
        q = R.worst(y, y64, bound)
        print(name, "worst err / bound %.3f" % q)
        assert q <= 1.0
    # k = 1, b = 0 is the resize alone: fl(r * 1) + 0 changes no bit
    assert R.same_bits(R.decode32(img[None], np.ones(c), np.zeros(c), size=size)[0].transpose(1, 2, 0), out)


def R_affine(c):
    from planer_amd.util import image_affine
    return image_affine([0.485, 0.456, 0.406, 0.5][:c], [0.229, 0.224, 0.225, 0.25][:c])


def test_table_restatement_matches_the_package():
    from planer_amd.util import _axis_samples
    for n, size in ((37, 24), (9, 31), (2, 5), (224, 224), (256, 224), (5, 5)):
        lo, fr = R.axis_samples(n, size)
        lo2, fr2 = _axis_samples(n, size)
        assert (lo == lo2).all() and R.same_bits(fr, fr2) and lo.min() >= 0 and lo.max() <= n - 2


def test_image_affine_values():
    from planer_amd.util import image_affine
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    k, b = image_affine(mean, std)
    assert k.dtype == np.float32 and b.dtype == np.float32 and k.shape == b.shape == (3,)
    for c in range(3):
        assert k[c] == np.float32(1.0 / (255.0 * std[c])) and b[c] == np.float32(-mean[c] / std[c])
    k, b = image_affine(0.5, 0.25, scale=1.0)                                    # scalars: one channel
    assert k.tolist() == [4.0] and b.tolist() == [-2.0]
    k, b = image_affine([0.0, 1.0], 2.0, scale=0.5)                              # a scalar std broadcasts
    assert k.tolist() == [1.0, 1.0] and b.tolist() == [0.0, -0.5]
    # rounded ONCE from float64: not the float32 quotient of float32 operands where the two differ
    k, _ = image_affine([0.0], [0.229])
    assert k[0] == np.float32(1.0 / (255.0 * 0.229))
    # the chain the reference's demos write, in float64, is what (k, b) folds
    x = np.arange(256, dtype=np.float64)
    k, b = image_affine(mean, std)
    for c in range(3):
        want = (x / 255 - mean[c]) / std[c]
        assert np.abs(x * np.float64(k[c]) + np.float64(b[c]) - want).max() <= 2 * R.U * np.abs(want).max() + 1e-12


def test_python_surface_refuses_without_a_device():
    from planer_amd import Net
    from planer_amd.util import ImageSpec, decode_images
    one = np.ones(3, np.float32)
    with pytest.raises(ValueError, match="layout"):
        ImageSpec(one, one, layout="hwcn")
    with pytest.raises(ValueError, match="one value per output channel"):
        ImageSpec(np.ones(5), np.ones(5))
    with pytest.raises(ValueError, match="one value per output channel"):
        ImageSpec(np.ones(3), np.ones(2))
    with pytest.raises(ValueError, match="order"):
        ImageSpec(one, one, order=(0, 1))
    with pytest.raises(ValueError, match="order"):
        ImageSpec(one, one, order=(0, 1, 4))
    with pytest.raises(ValueError, match="size"):
        ImageSpec(one, one, size=(0, 4))
    with pytest.raises(NotImplementedError, match="nhwc"):
        ImageSpec(one, one, layout="nchw", size=(4, 4))
    spec = ImageSpec(one, one, size=(8, 6), order=(2, 1, 0))
    assert spec.geometry((2, 5, 7, 3)) == ((2, 5, 7, 3), (2, 3, 8, 6))
    assert ImageSpec(one, one, layout="nchw").geometry((2, 3, 5, 7)) == ((2, 5, 7, 3), (2, 3, 5, 7))
    assert ImageSpec(one, one, order=(0, 1, 2)).geometry((1, 4, 4, 4))[1] == (1, 3, 4, 4)      # RGBA -> RGB
    with pytest.raises(ValueError, match="4-d"):
        spec.geometry((5, 7, 3))
    with pytest.raises(NotImplementedError, match="source channels"):
        spec.geometry((1, 5, 7, 5))
    with pytest.raises(ValueError, match="does not have"):
        spec.geometry((1, 5, 7, 2))
    with pytest.raises(ValueError, match="no order"):
        ImageSpec(one, one).geometry((1, 5, 7, 4))
    with pytest.raises(ValueError, match="H, W >= 2"):
        spec.geometry((1, 1, 7, 3))
    with pytest.raises(TypeError, match="uint8 DeviceArray"):
        decode_images(np.zeros((1, 4, 4, 3), np.uint8), one, one)                # a host array: upload it first
    net = Net()
    with pytest.raises(ValueError, match="layout"):
        net.image_input(one, one, layout="chw")
    assert net._image_in == {}
    assert net.image_input(one, one, size=(4, 4)) is net and net._image_in[None].size == (4, 4)
    net.image_input(one, one)                                                    # again: replaces
    assert net._image_in[None].size is None


def test_tile_constants_agree_everywhere():
    from planer_amd import _lib
    text = open(ROOT + "/include/planer_hip.h").read()
    got = {k: int(v) for k, v in re.findall(r"#define PL_IMAGE_U8_(TILE_PIXELS|LANE_PIXELS) (\d+)", text)}
    assert got == {"TILE_PIXELS": _lib.IMAGE_U8_TILE_PIXELS, "LANE_PIXELS": _lib.IMAGE_U8_LANE_PIXELS}

"""Objects as net output, the parts that need no GPU: the header's constants, what `ObjectSpec` and
`connected_components` refuse before they touch a device, the declaration's bookkeeping on a `Net`, and where the four arrays
land in the result tuple."""
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT

F32 = np.float32


def _fake(shape, dtype=np.float32):
    """A DeviceArray that owns nothing and belongs to no device: enough for the checks that look at type, dtype and shape."""
    from planer_amd.hip import DeviceArray
    return DeviceArray(shape, dtype, ctx=object(), ptr=64)


def test_header_constants_agree_with_python():
    from planer_amd import _lib, util
    text = open(os.path.join(ROOT, "include", "planer_hip.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (PL_CC_[A-Z_]+) (\d+)", text)}
    assert consts == dict(PL_CC_TILE_H=_lib.CC_TILE_H, PL_CC_TILE_W=_lib.CC_TILE_W, PL_CC_BLOCK=_lib.CC_BLOCK,
                          PL_CC_SCAN_STEP=_lib.CC_SCAN_STEP, PL_CC_MAX_OBJECTS=_lib.CC_MAX_OBJECTS)
    assert _lib.CC_TILE_W == 64 and _lib.CC_TILE_H * _lib.CC_TILE_W % 256 == 0 and _lib.CC_BLOCK % 256 == 0
    assert "pl_components_u8_i32" in _lib.SIGNATURES and re.search(r"\bint pl_components_u8_i32\(", text)
    assert len(_lib.SIGNATURES["pl_components_u8_i32"]) == 13
    # PL_CC_SCRATCH_BYTES as the header writes it: sums, link, counts
    assert re.search(r"#define PL_CC_SCRATCH_BYTES\(N, H, W, max_objects\)", text)
    assert util._cc_scratch_bytes(3, 5, 7, 10) == 3 * 10 * 16 + 3 * 35 * 4 + 3 * 1 * 4
    assert util._cc_scratch_bytes(1, 2048, 2, 0) == 4096 * 4 + 2 * 4 and util._cc_scratch_bytes(1, 2049, 1, 1) == 16 + 2049 * 4 + 8


def test_spec_argument_errors():
    from planer_amd.util import ObjectSpec
    spec = ObjectSpec()
    assert (spec.threshold, spec.connectivity, spec.background, spec.max_objects) == (0.0, 8, 0, 256)
    assert spec.geometry((2, 21, 64, 48)) == (2, 21, 64, 48)
    assert ObjectSpec(0.5, 4, -1, 0).geometry((1, 1, 3, 3)) == (1, 1, 3, 3)
    assert ObjectSpec(threshold=0.1).threshold == float(F32(0.1))
    for bad in (6, 0, "8", 8.5, True):
        with pytest.raises(ValueError, match="connectivity is 4 or 8"):
            ObjectSpec(connectivity=bad)
    for bad in (-2, 256, 0.5, None):
        with pytest.raises(ValueError, match="background is a class 0 to 255, or -1"):
            ObjectSpec(background=bad)
    for bad in (-1, 65537, 2.5, None):
        with pytest.raises(ValueError, match="max_objects is 0 to 65536"):
            ObjectSpec(max_objects=bad)
    with pytest.raises(ValueError, match="threshold is a number"):
        ObjectSpec(threshold=float("nan"))
    with pytest.raises(ValueError, match="1 to 256 planes fit a byte, got 257"):
        spec.geometry((1, 257, 4, 4))
    with pytest.raises(ValueError, match="planes"):
        spec.geometry((1, 0, 4, 4))
    with pytest.raises(ValueError, match="2\\^31 or more pixels"):
        spec.geometry((1, 3, 1 << 16, 1 << 15))
    with pytest.raises(ValueError, match="2\\^31 or more pixels"):
        spec.geometry((1 << 11, 3, 1 << 10, 1 << 10))
    with pytest.raises(ValueError, match="2\\^31 or more table entries"):
        ObjectSpec(max_objects=65536).geometry((1 << 13, 3, 4, 4))
    with pytest.raises(TypeError, match="got ndarray"):
        spec.check(np.zeros((1, 3, 4, 4), F32))
    with pytest.raises(ValueError, match="float32 tensor"):
        spec.check(_fake((1, 3, 4)))
    with pytest.raises(TypeError, match="got ndarray"):
        spec.encode(np.zeros((1, 3, 4, 4), F32))
    spec.check(_fake((1, 3, 4, 4)))


def test_connected_components_refuses_without_a_device():
    from planer_amd import util
    with pytest.raises(TypeError, match="got ndarray"):
        util.connected_components(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError, match="uint8 map"):
        util.connected_components(_fake((4, 4)))
    with pytest.raises(ValueError, match="uint8 map"):
        util.connected_components(_fake((1, 1, 4, 4), np.uint8))
    m = _fake((2, 4, 4), np.uint8)
    with pytest.raises(ValueError, match="connectivity"):
        util.connected_components(m, connectivity=6)
    with pytest.raises(ValueError, match="background"):
        util.connected_components(m, background=300)
    with pytest.raises(ValueError, match="max_objects"):
        util.connected_components(m, max_objects=-1)
    with pytest.raises(ValueError, match="pixels"):
        util.connected_components(_fake((1 << 16, 1 << 15), np.uint8))


def test_declaration_bookkeeping():
    from planer_amd import Net
    from planer_amd.util import LabelSpec, ObjectSpec
    net = Net()
    assert net.object_output() is net and isinstance(net._image_out[0], ObjectSpec)
    net.object_output(connectivity=4, background=-1, max_objects=9, index=2)
    assert sorted(net._image_out) == [0, 2] and net._image_out[2].max_objects == 9
    with pytest.raises(ValueError, match="connectivity"):
        net.object_output(connectivity=5, index=1)
    with pytest.raises(ValueError, match="position"):
        net.object_output(index=-1)
    assert sorted(net._image_out) == [0, 2]
    # declaring again replaces, whatever was there
    net.label_output(index=2)
    assert isinstance(net._image_out[2], LabelSpec)
    net.object_output(max_objects=3, index=2)
    assert net._image_out[2].max_objects == 3
    # the clash with a detection declaration, from either side
    heads = [([(10, 14)], 8), ([(23, 27)], 16)]
    with pytest.raises(ValueError, match="output 2 is already declared"):
        net.detection_output(heads, 3, indices=(1, 2))
    with pytest.raises(ValueError, match="already declared"):
        net.detection_output(heads, 3)
    net.detection_output(heads, 3, indices=(1, 3))
    with pytest.raises(ValueError, match="output 3 is a head of the declared detection output"):
        net.object_output(index=3)
    # float_output takes it back
    assert net.float_output(2) is net and sorted(net._image_out) == [0] and net._detect is not None
    net.float_output(0)
    assert net._image_out == {}


def test_result_tuple_arithmetic(monkeypatch):
    from planer_amd import Net
    from planer_amd.util import DetectionSpec, LabelSpec, ObjectSpec
    seen = []
    four = ("labels", "num", "objects", "centroids")
    monkeypatch.setattr(ObjectSpec, "encode", lambda self, x, ctx=None: seen.append(x) or four)
    monkeypatch.setattr(LabelSpec, "encode", lambda self, x, ctx=None: "map")
    monkeypatch.setattr(DetectionSpec, "encode", lambda self, xs, ctx=None: ("det", "num"))
    s, a, b = _fake((2, 3, 8, 8)), _fake((2, 5)), _fake((2, 7))
    # a one-output net: labels, num, objects, centroids = net(x)
    assert Net().object_output()._hand_back(s, False) == four and seen[-1] is s
    assert Net().object_output()._hand_back((s,), False) == four
    # spliced in at its position, the others untouched
    assert Net().object_output(index=1)._hand_back((a, s, b), False) == (a,) + four + (b,)
    assert Net().object_output(index=2)._hand_back((a, b, s), False) == (a, b) + four
    # beside a label output and a second object output
    net = Net().object_output(index=0).label_output(index=1).object_output(index=3)
    assert net._hand_back((s, s, a, s), False) == four + ("map", a) + four
    # beside detections: det, num where the lowest head was
    h = [_fake((2, 8, 8, 8)), _fake((2, 8, 4, 4))]
    net = Net().detection_output([([(10, 14)], 8), ([(23, 27)], 16)], 3, indices=(0, 2)).object_output(index=1)
    assert net._hand_back((h[0], s, h[1], a), False) == ("det", "num") + four + (a,)
    # checks come first: a position the net does not have, a tensor the label kernel does not take, a host array
    calls = len(seen)
    with pytest.raises(ValueError, match="output 1 is declared .*, the net returns 1"):
        Net().object_output(index=1)._hand_back(s, False)
    with pytest.raises(ValueError, match="float32 tensor"):
        Net().object_output()._hand_back(a, False)
    with pytest.raises(ValueError, match="planes"):
        Net().object_output()._hand_back(_fake((1, 300, 4, 4)), False)
    with pytest.raises(ValueError, match="no device tensor: ndarray"):
        Net().object_output()._hand_back(np.zeros((2, 3, 8, 8), F32), False)
    assert len(seen) == calls
    # taken back: the float tensor again
    assert Net().object_output().float_output()._hand_back(s, False) is s

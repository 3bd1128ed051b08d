"""Keypoints as net output, the parts that need no GPU: the header's constants, what `KeypointSpec` and
`heatmap_peaks` refuse before they touch a device, the declaration's bookkeeping on a `Net`, the `tiled` refusal, and where the
two arrays land in the result tuple."""
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
    consts = {k: int(v) for k, v in re.findall(r"#define (PL_PEAKS_[A-Z_]+) (\d+)", text)}
    assert consts == dict(PL_PEAKS_TILE_H=_lib.PEAKS_TILE_H, PL_PEAKS_TILE_W=_lib.PEAKS_TILE_W, PL_PEAKS_MAX_PEAKS=_lib.PEAKS_MAX_PEAKS,
                          PL_PEAKS_MERGE_KEYS=_lib.PEAKS_MERGE_KEYS, PL_PEAKS_MAX_EXTENT=_lib.PEAKS_MAX_EXTENT,
                          PL_PEAKS_TIES_ALL=_lib.PEAKS_TIES["all"], PL_PEAKS_TIES_FIRST=_lib.PEAKS_TIES["first"],
                          PL_PEAKS_REFINE_NONE=_lib.PEAKS_REFINE["none"], PL_PEAKS_REFINE_QUARTER=_lib.PEAKS_REFINE["quarter"])
    # px + 0.25 is exact in float32 for every px below the largest extent, and no longer one step above it
    top = _lib.PEAKS_MAX_EXTENT - 1
    assert float(F32(top) + F32(0.25)) == top + 0.25 and float(F32(top) - F32(0.25)) == top - 0.25
    assert float(F32(top + 1) + F32(0.25)) != top + 1.25
    assert _lib.PEAKS_MAX_PEAKS < _lib.PEAKS_MERGE_KEYS and _lib.PEAKS_MERGE_KEYS & (_lib.PEAKS_MERGE_KEYS - 1) == 0
    assert "pl_peaks_f32" in _lib.SIGNATURES and re.search(r"\bint pl_peaks_f32\(", text)
    assert len(_lib.SIGNATURES["pl_peaks_f32"]) == 15
    assert re.search(r"#define PL_PEAKS_SCRATCH_BYTES\(N, K, H, W, max_peaks\)", text)
    th, tw = _lib.PEAKS_TILE_H, _lib.PEAKS_TILE_W
    assert util._peaks_scratch_bytes(2, 3, th, tw, 5) == 6 * 44 and util._peaks_scratch_bytes(1, 1, th + 1, 2 * tw + 1, 1) == 6 * 12
    assert util._peaks_scratch_bytes(4, 1, 0, 9, 7) == 0


def test_spec_argument_errors():
    from planer_amd.util import KeypointSpec
    spec = KeypointSpec()
    assert (spec.threshold, spec.ties, spec.max_peaks, spec.refine, spec.stride) == (0.0, "all", 32, "none", (1.0, 1.0))
    assert spec.places == 2
    assert spec.geometry((2, 17, 64, 48)) == (2, 17, 64, 48)
    s = KeypointSpec(0.1, "first", 1, "quarter", (7.5, 3.3))
    assert s.threshold == float(F32(0.1)) and s.stride == (7.5, float(F32(3.3))) and s.geometry((1, 1, 0, 3)) == (1, 1, 0, 3)
    assert KeypointSpec(threshold=-np.inf, stride=4).stride == (4.0, 4.0)
    for bad in ("last", 0, None, True):
        with pytest.raises(ValueError, match="ties is 'all' or 'first'"):
            KeypointSpec(ties=bad)
    for bad in ("half", 1, None):
        with pytest.raises(ValueError, match="refine is 'none' or 'quarter'"):
            KeypointSpec(refine=bad)
    for bad in (0, -1, 257, 2.5, None, True):
        with pytest.raises(ValueError, match="max_peaks is 1 to 256"):
            KeypointSpec(max_peaks=bad)
    with pytest.raises(ValueError, match="threshold is a number"):
        KeypointSpec(threshold=float("nan"))
    for bad in ((1, 2, 3), "4", None, (1, None)):
        with pytest.raises(ValueError, match="stride is a number or an \\(sy, sx\\) pair"):
            KeypointSpec(stride=bad)
    for bad in (0, -4, float("nan"), float("inf"), (4, 0)):
        with pytest.raises(ValueError, match="stride is positive and finite"):
            KeypointSpec(stride=bad)
    with pytest.raises(ValueError, match="above 4194304 in one extent"):
        spec.geometry((1, 1, 1, (1 << 22) + 1))
    with pytest.raises(ValueError, match="2\\^31 or more pixels"):
        spec.geometry((1, 3, 1 << 16, 1 << 15))
    with pytest.raises(ValueError, match="2\\^31 or more pixels"):
        spec.geometry((1 << 11, 1, 1 << 10, 1 << 10))
    with pytest.raises(ValueError, match="2\\^31 or more output floats"):
        KeypointSpec(max_peaks=256).geometry((1 << 12, 1 << 10, 1, 1))
    with pytest.raises(TypeError, match="got ndarray"):
        spec.check(np.zeros((1, 3, 4, 4), F32))
    with pytest.raises(ValueError, match="float32 tensor"):
        spec.check(_fake((1, 3, 4)))
    with pytest.raises(ValueError, match="float32 tensor"):
        spec.check(_fake((1, 3, 4, 4), np.uint8))
    with pytest.raises(TypeError, match="got ndarray"):
        spec.encode(np.zeros((1, 3, 4, 4), F32))
    spec.check(_fake((1, 3, 4, 4)))


def test_heatmap_peaks_refuses_without_a_device():
    from planer_amd import util
    with pytest.raises(TypeError, match="got ndarray"):
        util.heatmap_peaks(np.zeros((4, 4), F32))
    with pytest.raises(ValueError, match="float32 maps"):
        util.heatmap_peaks(_fake((4, 4), np.uint8))
    with pytest.raises(ValueError, match="float32 maps"):
        util.heatmap_peaks(_fake((4,)))
    with pytest.raises(ValueError, match="float32 maps"):
        util.heatmap_peaks(_fake((1, 1, 1, 4, 4)))
    m = _fake((2, 3, 4, 4))
    with pytest.raises(ValueError, match="ties"):
        util.heatmap_peaks(m, ties="some")
    with pytest.raises(ValueError, match="max_peaks"):
        util.heatmap_peaks(m, max_peaks=0)
    with pytest.raises(ValueError, match="refine"):
        util.heatmap_peaks(m, refine="parabola")
    with pytest.raises(ValueError, match="pixels"):
        util.heatmap_peaks(_fake((1 << 16, 1 << 15)))


def test_declaration_bookkeeping():
    from planer_amd import Net
    from planer_amd.util import KeypointSpec, LabelSpec, ObjectSpec
    net = Net()
    assert net.keypoint_output() is net and isinstance(net._image_out[0], KeypointSpec)
    net.keypoint_output(0.25, "first", 9, "quarter", 4, index=2)
    k = net._image_out[2]
    assert sorted(net._image_out) == [0, 2] and (k.threshold, k.ties, k.max_peaks, k.refine, k.stride) == (0.25, "first", 9, "quarter", (4.0, 4.0))
    with pytest.raises(ValueError, match="ties"):
        net.keypoint_output(ties="both", index=1)
    with pytest.raises(ValueError, match="position"):
        net.keypoint_output(index=-1)
    assert sorted(net._image_out) == [0, 2]
    # declaring again replaces, whatever was there
    net.label_output(index=2)
    assert isinstance(net._image_out[2], LabelSpec)
    net.keypoint_output(max_peaks=3, index=2)
    assert net._image_out[2].max_peaks == 3
    net.object_output(index=2)
    assert isinstance(net._image_out[2], ObjectSpec)
    net.keypoint_output(max_peaks=5, index=2)
    assert isinstance(net._image_out[2], KeypointSpec)
    # the clash with a detection declaration, from either side
    heads = [([(10, 14)], 8), ([(23, 27)], 16)]
    with pytest.raises(ValueError, match="output 2 is already declared"):
        net.detection_output(heads, 3, indices=(1, 2))
    with pytest.raises(ValueError, match="already declared"):
        net.detection_output(heads, 3)
    net.detection_output(heads, 3, indices=(1, 3))
    with pytest.raises(ValueError, match="output 3 is a head of the declared detection output"):
        net.keypoint_output(index=3)
    # float_output takes it back
    assert net.float_output(2) is net and sorted(net._image_out) == [0] and net._detect is not None
    net.float_output(0)
    assert net._image_out == {}


def test_places_are_a_property_of_the_spec():
    from planer_amd.util import ImageOutSpec, KeypointSpec, LabelSpec, ObjectSpec
    assert (ImageOutSpec.places, LabelSpec.places, ObjectSpec.places, KeypointSpec.places) == (1, 1, 4, 2)


def test_tiled_refuses_a_keypoint_declaration():
    from planer_amd import Net
    net = Net()
    net.input = ["x"]
    net.keypoint_output()
    with pytest.raises(ValueError, match="Net.tiled: a keypoint output is declared, and the peaks of a blended scan are not built"):
        net.tiled(np.zeros((64, 64, 3), F32), window=32)
    with pytest.raises(ValueError, match="keypoint output is declared"):
        net.tiled(_fake((64, 64, 3)), window=32)


def test_result_tuple_arithmetic(monkeypatch):
    from planer_amd import Net
    from planer_amd.util import DetectionSpec, KeypointSpec, LabelSpec, ObjectSpec
    seen = []
    two, four = ("peaks", "count"), ("labels", "num", "objects", "centroids")
    monkeypatch.setattr(KeypointSpec, "encode", lambda self, x, ctx=None: seen.append(x) or two)
    monkeypatch.setattr(ObjectSpec, "encode", lambda self, x, ctx=None: four)
    monkeypatch.setattr(LabelSpec, "encode", lambda self, x, ctx=None: "map")
    monkeypatch.setattr(DetectionSpec, "encode", lambda self, xs, ctx=None: ("det", "num"))
    s, a, b = _fake((2, 17, 8, 8)), _fake((2, 5)), _fake((2, 7))
    # a one-output net: peaks, num = net(x)
    assert Net().keypoint_output()._hand_back(s, False) == two and seen[-1] is s
    assert Net().keypoint_output()._hand_back((s,), False) == two
    # spliced in at its position, the others untouched
    assert Net().keypoint_output(index=1)._hand_back((a, s, b), False) == (a,) + two + (b,)
    assert Net().keypoint_output(index=2)._hand_back((a, b, s), False) == (a, b) + two
    # beside a label output, an object output and a second keypoint output
    net = Net().keypoint_output(index=0).label_output(index=1).object_output(index=2).keypoint_output(index=4)
    assert net._hand_back((s, s, s, a, s), False) == two + ("map",) + four + (a,) + two
    # beside detections: det, num where the lowest head was
    h = [_fake((2, 8, 8, 8)), _fake((2, 8, 4, 4))]
    net = Net().detection_output([([(10, 14)], 8), ([(23, 27)], 16)], 3, indices=(0, 2)).keypoint_output(index=1)
    assert net._hand_back((h[0], s, h[1], a), False) == ("det", "num") + two + (a,)
    # checks come first: a position the net does not have, a tensor the kernel does not take, a host array
    calls = len(seen)
    with pytest.raises(ValueError, match="output 1 is declared .*, the net returns 1"):
        Net().keypoint_output(index=1)._hand_back(s, False)
    with pytest.raises(ValueError, match="float32 tensor"):
        Net().keypoint_output()._hand_back(a, False)
    with pytest.raises(ValueError, match="2\\^31 or more output floats"):
        Net().keypoint_output(max_peaks=256)._hand_back(_fake((1 << 12, 1 << 10, 1, 1)), False)
    with pytest.raises(ValueError, match="no device tensor: ndarray"):
        Net().keypoint_output()._hand_back(np.zeros((2, 17, 8, 8), F32), False)
    assert len(seen) == calls
    # taken back: the float tensor again
    assert Net().keypoint_output().float_output()._hand_back(s, False) is s


def test_posenet_is_one_channel_quad_run():
    """irgen/posenet.py at 256 x 192: the ResNet-18 trunk, three transposed convs and the 1 x 1 head between the row-packed stem
    and the only `from_q4`; 64 x 48 heat maps, one plane per joint."""
    from planer_amd.irgen import posenet
    from tests.linear_q4_ref import compile_plan, steps_of
    g, b = posenet.build()
    x = posenet.make_input(2)
    assert x.shape == (2, 3, 256, 192)
    body, flow, _, shapes = compile_plan(g, b, x, force=False)
    names = [s[0] for s in steps_of(body, flow)]
    assert names.count("convt_q4") == 3 and names.count("conv_q4") == 21 and names.count("to_q4") == 0
    assert names.count("from_q4") == 1 and names[-2:] == ["from_q4", "return"]
    assert shapes["heat"] == (2, posenet.JOINTS, 64, 48) and shapes["up0_t"] == (2, 256, 16, 12)
    assert (posenet.SIZE[0] // posenet.STRIDE, posenet.SIZE[1] // posenet.STRIDE) == (64, 48)

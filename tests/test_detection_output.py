"""Detections as net output, the parts that need no GPU: the numpy mirrors on hand-worked cases, planted heads
through the float64 reference, the header's constants, what the Python surface refuses before it touches a device, and where
det and num land in the result tuple."""
import os
import re

import numpy as np
import pytest

from tests import detect_ref as R
from tests.conftest import ROOT

F32 = np.float32
NAN, INF = float("nan"), float("inf")


def _nms(boxes, scores, classes=None, iou=0.45, max_det=None, floor=-INF, class_aware=True):
    v, o = R.topk_order(scores, len(scores))
    return R.nms32(boxes, classes, v, o, floor, iou, class_aware, max_det or len(scores))


def test_header_constants_agree_with_python():
    from planer_amd import _lib
    text = open(os.path.join(ROOT, "include", "planer_hip.h")).read()
    consts = dict(re.findall(r"#define (PL_YOLO_MAX_ANCHORS|PL_NMS_MAX_CANDIDATES) (\d+)", text))
    assert int(consts["PL_YOLO_MAX_ANCHORS"]) == _lib.YOLO_MAX_ANCHORS == 8
    assert int(consts["PL_NMS_MAX_CANDIDATES"]) == _lib.NMS_MAX_CANDIDATES == 4096
    assert 24 * 4096 + 16 * 64 < 100 * 1024                          # the NMS kernel's LDS at its ceiling
    for name in ("pl_yolo_decode_f32", "pl_nms_f32"):
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, text)
    assert len(_lib.SIGNATURES["pl_yolo_decode_f32"]) == 16 and len(_lib.SIGNATURES["pl_nms_f32"]) == 14


def test_mirror_two_overlapping_boxes():
    # A = (0, 0, 10, 10), B = (1, 1, 11, 11): inter = 9 * 9 = 81, union = (100 + 100) - 81 = 119, 0.45 * 119 = 53.55 < 81
    boxes = np.array([[0, 0, 10, 10], [1, 1, 11, 11]], F32)
    det, num = _nms(boxes, [0.9, 0.8], classes=[3, 3])
    assert num == 1 and det.dtype == F32 and det.shape == (2, 6)
    assert det[0].tolist() == [0, 0, 10, 10, F32(0.9), 3] and det[1].tolist() == [0] * 6
    assert not np.signbit(det[1]).any()
    # the better score is kept, whichever comes first in memory
    det, num = _nms(boxes, [0.8, 0.9], classes=[3, 3])
    assert num == 1 and det[0].tolist() == [1, 1, 11, 11, F32(0.9), 3]
    # different classes: both stay when NMS is class-aware, one when it is not; iou at 81 / 119 = 0.6807 decides too
    det, num = _nms(boxes, [0.9, 0.8], classes=[3, 4])
    assert num == 2 and det[:, 5].tolist() == [3, 4] and det[:, 4].tolist() == [F32(0.9), F32(0.8)]
    assert _nms(boxes, [0.9, 0.8], classes=[3, 4], class_aware=False)[1] == 1
    assert _nms(boxes, [0.9, 0.8], classes=None)[1] == 1
    assert _nms(boxes, [0.9, 0.8], classes=[3, 3], iou=0.69)[1] == 2
    assert _nms(boxes, [0.9, 0.8], classes=[3, 3], iou=0.68)[1] == 1
    # max_det stops it; the floor is exclusive; a score at or below it is no candidate
    det, num = _nms(boxes, [0.9, 0.8], classes=[3, 4], max_det=1)
    assert num == 1 and det.shape == (1, 6)
    assert _nms(boxes, [0.9, 0.8], classes=[3, 4], floor=0.8)[1] == 1
    assert _nms(boxes, [0.9, 0.8], classes=[3, 4], floor=0.9)[1] == 0
    # a chain: A suppresses B, and B, had it been kept, would have suppressed C; C stays
    chain = np.array([[0, 0, 10, 10], [3, 0, 13, 10], [6, 0, 16, 10]], F32)         # neighbours 70 / 130, A-C 40 / 160
    det, num = _nms(chain, [0.9, 0.8, 0.7])
    assert num == 2 and det[:2, 0].tolist() == [0, 6]


def test_mirror_exact_tie_is_broken_by_index():
    # pl_topk_f32's own order: descending value, equal values by DESCENDING position, NaN first
    v, o = R.topk_order([0.5, 0.7, 0.7, 0.2, NAN], 5)
    assert o.tolist() == [4, 2, 1, 0, 3] and np.isnan(v[0]) and v[1:].tolist() == [F32(0.7), F32(0.7), F32(0.5), F32(0.2)]
    # the chain stores rows back to front, so in ANCHOR order equal scores go by ascending index
    boxes = np.array([[[0, 0, 1, 1], [10, 0, 11, 1], [20, 0, 21, 1], [30, 0, 31, 1]]], F32)
    scores = np.array([[0.5, 0.7, 0.7, -1]], F32)
    det, num = R.chain32(scores, np.array([[0, 1, 2, 3]]), boxes, 0.25, 0.45, True, 100, 1024)
    assert det.shape == (1, 4, 6) and num.tolist() == [3]
    assert det[0, :, 5].tolist() == [1, 2, 0, 0] and det[0, :, 0].tolist() == [10, 20, 0, 0]
    # ... and when the tie straddles the cut at max_candidates, the lower index is the one that goes on
    det, num = R.chain32(scores, np.array([[0, 1, 2, 3]]), boxes, 0.25, 0.45, True, 100, 1)
    assert det.shape == (1, 1, 6) and num.tolist() == [1] and det[0, 0, 5] == 1
    # two identical boxes with equal scores: the lower index survives
    same = np.array([[[0, 0, 4, 4], [0, 0, 4, 4]]], F32)
    det, num = R.chain32(np.array([[0.6, 0.6]], F32), np.array([[7, 7]]), same, 0.25, 0.45, True, 100, 1024)
    assert num.tolist() == [1]


def test_mirror_zero_area_and_nan_boxes():
    # a point inside A: iw = min(10, 5) - max(0, 5) = 0, inter = 0, union = (100 + 0) - 0 = 100, 0 > 45 is false: it stays
    boxes = np.array([[0, 0, 10, 10], [5, 5, 5, 5]], F32)
    assert _nms(boxes, [0.9, 0.8])[1] == 2
    # two identical points: inter = 0, union = 0, 0 > 0.45 * 0 is false: no division, nothing suppressed
    assert _nms(np.array([[5, 5, 5, 5], [5, 5, 5, 5]], F32), [0.9, 0.8])[1] == 2
    # a zero-height box that crosses A: ih = 0 -> inter = 0
    assert _nms(np.array([[0, 0, 10, 10], [2, 5, 8, 5]], F32), [0.9, 0.8])[1] == 2
    # a NaN coordinate: fmin / fmax skip it, the NaN area makes union NaN, and inter > NaN is false
    det, num = _nms(np.array([[0, 0, 10, 10], [0, 0, NAN, 10]], F32), [0.9, 0.8])
    assert num == 2 and np.isnan(det[1, 2])
    # an inverted box has iw = max(0, negative) = 0
    assert _nms(np.array([[0, 0, 10, 10], [9, 9, 1, 1]], F32), [0.9, 0.8])[1] == 2
    # NaN scores come first out of top-k and are no candidates; an index outside the boxes is dead too
    assert _nms(boxes, [NAN, 0.8])[1] == 1
    det, num = R.nms32(boxes, None, [0.9, 0.8], [5, 1], -INF, 0.45, False, 2)
    assert num == 1 and det[0].tolist() == [5, 5, 5, 5, F32(0.8), 0]


HEADS = [([(10, 14), (23, 27)], None), ([(30, 61), (62, 45)], (16, 16))]
SHAPES = [(2, 2 * 8, 4, 4), (2, 2 * 8, 2, 2)]
ITEMS = [(0, 0, 0, 1, 2, 0.81, 2, (15.0, 9.0, 27.0, 21.0)), (0, 1, 1, 0, 1, 0.64, 0, (2.0, 1.0, 50.0, 29.0)),
         (1, 0, 1, 3, 3, 0.49, 1, (25.0, 24.0, 31.0, 32.0)), (1, 1, 0, 1, 0, 0.3025, 2, (4.0, 20.0, 12.0, 30.0))]


def test_plant_round_trips_through_decode64():
    xs = R.plant(SHAPES, HEADS, 3, ITEMS, size=(32, 32))
    assert [x.shape for x in xs] == SHAPES and all(x.dtype == F32 for x in xs)
    ref = R.decode64(xs, HEADS, 3, 0.25, size=(32, 32))
    rows, total = R.head_geometry(SHAPES, HEADS, 3, (32, 32))
    assert total == 2 * 16 + 2 * 4 and [r[3:6] for r in rows] == [(8.0, 8.0, 0), (16.0, 16.0, 32)]
    assert ref["cand"].sum() == len(ITEMS)
    for n, h, a, gy, gx, score, cls, box in ITEMS:
        _, gh, gw, _, _, off, _ = rows[h]
        i = off + (a * gh + gy) * gw + gx
        assert ref["cand"][n, i] and ref["cls"][n, i] == cls
        assert abs(ref["score"][n, i] - score) < 1e-6
        assert np.abs(ref["box"][n, i] - box).max() < 1e-4, (ref["box"][n, i], box)
        assert 0 < ref["tol_score"][n, i] < 1e-6 and 0 < ref["tol_box"][n, i].max() < 1e-4
    assert R.margins(ref, 0.25, 0.45, 1024) == []
    # the conditions notice what they are there for
    assert any("conf" in m for m in R.margins(ref, 0.49, 0.45, 1024))
    twins = ITEMS[:1] + [(0, 0, 1, 2, 2, 0.81 * (1 + 1e-6), 2, (15.0, 17.0, 27.0, 29.0))]
    assert any("each other" in m for m in R.margins(R.decode64(R.plant(SHAPES, HEADS, 3, twins, size=(32, 32)), HEADS, 3, 0.25, size=(32, 32)),
                                                     0.25, 0.45, 1024))
    # bit-equal logits are an exact tie, which is allowed
    ties = ITEMS[:1] + [(0, 0, 1, 2, 2, 0.81, 2, (15.0, 17.0, 27.0, 29.0))]
    assert R.margins(R.decode64(R.plant(SHAPES, HEADS, 3, ties, size=(32, 32)), HEADS, 3, 0.25, size=(32, 32)), 0.25, 0.45, 1024) == []
    # iou exactly at a pair's overlap: (15, 9, 27, 21) and the same box shifted by 4 have inter 8 * 12 = 96 of union 192
    edge = ITEMS[:1] + [(0, 0, 1, 1, 3, 0.7, 2, (19.0, 9.0, 31.0, 21.0))]
    ref = R.decode64(R.plant(SHAPES, HEADS, 3, edge, size=(32, 32)), HEADS, 3, 0.25, size=(32, 32))
    assert any("inter - iou union" in m for m in R.margins(ref, 0.25, 0.5, 1024))
    assert R.margins(ref, 0.25, 0.45, 1024) == []
    other = ITEMS[:1] + [(0, 0, 1, 1, 3, 0.7, 1, (19.0, 9.0, 31.0, 21.0))]          # another class: the pair is never compared
    ref = R.decode64(R.plant(SHAPES, HEADS, 3, other, size=(32, 32)), HEADS, 3, 0.25, size=(32, 32))
    assert R.margins(ref, 0.25, 0.5, 1024) == [] and R.margins(ref, 0.25, 0.5, 1024, class_aware=False) != []


def test_decode64_special_values():
    x = np.full((1, 7, 1, 3), -2.0, F32)                             # one anchor, two classes, three cells
    x[0, 4] = [3.0, NAN, 3.0]
    x[0, 5] = [1.0, 1.0, NAN]
    x[0, 6] = [1.0, 2.0, 0.0]
    x[0, 2] = [0.0, 0.0, 100.0]
    ref = R.decode64([x], [([(8, 8)], 4)], 2, 0.25)
    assert ref["cls"][0].tolist() == [0, 1, 0]                       # equal logits: the first; a NaN counts as the maximum
    assert ref["cand"][0].tolist() == [True, False, False]           # NaN objectness / NaN class logit: no candidate
    with np.errstate(over="ignore"):
        assert np.isinf(np.asarray(ref["box"][0, 2, 2], F32))        # exp(100) overflows float32
    assert R.close(np.array([np.inf, 1.0, NAN]), np.array([1e300, 1.0, NAN]), np.array([1.0, 0.0, 0.0])).all()
    assert not R.close(np.array([3e38]), np.array([1e300]), np.array([1.0])).any()


def test_spec_and_declaration_argument_errors():
    from planer_amd import Net
    from planer_amd.util import DetectionSpec
    heads = [([(10, 14), (23, 27)], None), ([(30, 61)], 16)]
    spec = DetectionSpec(heads, 3, size=(32, 48))
    n, rows, total, k, md = spec.geometry([(2, 16, 4, 6), (2, 8, 2, 3)])
    assert (n, total, k, md) == (2, 2 * 24 + 6, 54, 54)
    assert rows == [(2, 3, 4, 6, 8.0, 8.0, 0), (1, 3, 2, 3, 16.0, 16.0, 48)]
    assert DetectionSpec(heads, 3, size=(32, 48), max_det=7, max_candidates=20).geometry([(2, 16, 4, 6), (2, 8, 2, 3)])[3:] == (20, 7)
    assert spec.conf == float(F32(0.25)) and spec.iou == float(F32(0.45)) and spec.class_aware is True
    with pytest.raises(ValueError, match=r"head 1 has 9 channels, 1 anchors x \(5 \+ 3 classes\) is 8"):
        spec.geometry([(2, 16, 4, 6), (2, 9, 2, 3)])
    with pytest.raises(ValueError, match="batch size"):
        spec.geometry([(2, 16, 4, 6), (3, 8, 2, 3)])
    with pytest.raises(ValueError, match="2 heads declared, 1 tensors"):
        spec.geometry([(2, 16, 4, 6)])
    with pytest.raises(ValueError, match="no stride"):
        DetectionSpec(heads, 3).geometry([(2, 16, 4, 6), (2, 8, 2, 3)])
    with pytest.raises(ValueError, match="max_candidates is 1 to 4096"):
        DetectionSpec(heads, 3, max_candidates=4097)
    with pytest.raises(ValueError, match="max_candidates"):
        DetectionSpec(heads, 3, max_candidates=0)
    with pytest.raises(ValueError, match="max_det"):
        DetectionSpec(heads, 3, max_det=0)
    with pytest.raises(ValueError, match="classes"):
        DetectionSpec(heads, 0)
    with pytest.raises(ValueError, match="9 anchors"):
        DetectionSpec([([(1, 1)] * 9, 8)], 3)
    with pytest.raises(ValueError, match="no heads"):
        DetectionSpec([], 3)
    with pytest.raises(ValueError, match="size"):
        DetectionSpec(heads, 3, size=(32,))
    net = Net()
    with pytest.raises(ValueError, match="max_candidates"):
        net.detection_output(heads, 3, max_candidates=5000)
    with pytest.raises(ValueError, match="one distinct output position per head"):
        net.detection_output(heads, 3, indices=(0,))
    with pytest.raises(ValueError, match="one distinct output position per head"):
        net.detection_output(heads, 3, indices=(1, 1))
    with pytest.raises(ValueError, match="position"):
        net.detection_output(heads, 3, indices=(0, -1))
    assert net._detect is None
    # a position claimed twice, from either side
    net.label_output(index=1)
    with pytest.raises(ValueError, match="output 1 is already declared"):
        net.detection_output(heads, 3, size=(32, 48), indices=(0, 1))
    with pytest.raises(ValueError, match="already declared"):
        net.detection_output(heads, 3, size=(32, 48))                # every output: 1 among them
    assert net.detection_output(heads, 3, size=(32, 48), indices=(0, 2)) is net
    with pytest.raises(ValueError, match="output 2 is a head of the declared detection output"):
        net.image_output(np.ones(3), np.ones(3), index=2)
    with pytest.raises(ValueError, match="head of the declared detection"):
        net.label_output(index=0)
    net.label_output(index=3)                                        # beside it: fine
    # declaring again replaces; float_output on any of its positions removes it
    net.detection_output(heads, 3, size=(32, 48), indices=(2, 0), max_det=5)
    assert net._detect[1] == (2, 0) and net._detect[0].max_det == 5
    assert net.float_output(1) is net and net._detect is not None and 1 not in net._image_out
    net.float_output(0)
    assert net._detect is None and 3 in net._image_out
    net.float_output(3)
    net.detection_output(heads, 3, size=(32, 48))
    with pytest.raises(ValueError, match="head of the declared"):
        net.label_output(index=5)                                    # every output is a head
    net.float_output(7)
    assert net._detect is None


def _fake(shape):
    """A DeviceArray that owns nothing and belongs to no device: enough for the checks that look at type, dtype and shape."""
    from planer_amd.hip import DeviceArray
    return DeviceArray(shape, np.float32, ctx=object(), ptr=64)


def test_result_tuple_arithmetic(monkeypatch):
    from planer_amd import Net
    from planer_amd.util import DetectionSpec
    heads = [([(10, 14)], 8), ([(23, 27)], 16), ([(30, 61)], 32)]
    seen = []
    monkeypatch.setattr(DetectionSpec, "encode", lambda self, xs, ctx=None: seen.append(list(xs)) or ("det", "num"))
    h = [_fake((2, 8, 8, 8)), _fake((2, 8, 4, 4)), _fake((2, 8, 2, 2))]
    other = _fake((2, 5))
    # heads at (0, 1, 2) of 3: det, num = net(x)
    net = Net().detection_output(heads, 3)
    assert net._hand_back(tuple(h), False) == ("det", "num") and seen[-1] == h
    assert Net().detection_output(heads, 3, indices=(0, 1, 2))._hand_back(tuple(h), False) == ("det", "num")
    # heads at (1, 2) of 4
    net = Net().detection_output(heads[:2], 3, indices=(1, 2))
    a, b = _fake((2, 1)), _fake((2, 2))
    assert net._hand_back((a, h[0], h[1], b), False) == (a, "det", "num", b) and seen[-1] == h[:2]
    # head order is the order of `indices`, det and num go where the LOWEST position was
    net = Net().detection_output(heads[:2], 3, indices=(3, 1))
    assert net._hand_back((a, h[1], b, h[0]), False) == (a, "det", "num", b) and seen[-1] == h[:2]
    net = Net().detection_output(heads[:1], 3, indices=(1,))
    assert net._hand_back((a, h[0]), False) == (a, "det", "num")
    # a single output that is the one head
    assert Net().detection_output(heads[:1], 3)._hand_back(h[0], False) == ("det", "num")
    # checks: indices beyond what the net returns, a head count that does not match, a wrong channel count, a host array
    calls = len(seen)
    with pytest.raises(ValueError, match="output 3 is declared a detection head, the net returns 3"):
        Net().detection_output(heads[:2], 3, indices=(0, 3))._hand_back(tuple(h), False)
    with pytest.raises(ValueError, match="3 heads declared, the net returns 4"):
        Net().detection_output(heads, 3)._hand_back(tuple(h) + (other,), False)
    with pytest.raises(ValueError, match=r"head 1 has 8 channels, 1 anchors x \(5 \+ 4 classes\) is 9"):
        Net().detection_output(heads, 4)._check_outputs((_fake((2, 9, 8, 8)), h[1], h[2]))
    with pytest.raises(ValueError, match="no device tensor: ndarray"):
        Net().detection_output(heads, 3)._hand_back((h[0], np.zeros((2, 8, 4, 4), F32), h[2]), False)
    with pytest.raises(ValueError, match="float32 tensor"):
        Net().detection_output(heads[:1], 3, indices=(1,))._hand_back((h[0], other), False)
    assert len(seen) == calls                                        # refused before anything was encoded
    # nothing declared: the outputs pass through untouched
    assert Net()._hand_back(tuple(h), False) == tuple(h)
    assert Net().detection_output(heads, 3).float_output(1)._hand_back(tuple(h), False) == tuple(h)


def test_python_surface_refuses_without_a_device():
    from planer_amd import util
    heads = [([(10, 14)], 8)]
    host = np.zeros((1, 8, 4, 4), F32)
    with pytest.raises(TypeError, match="got ndarray"):
        util.decode_detections([host], heads, 3)
    with pytest.raises(TypeError, match="got ndarray"):
        util.DetectionSpec(heads, 3).encode([host])
    with pytest.raises(TypeError, match="got ndarray"):
        util.nms(np.zeros((1, 4, 4), F32), np.zeros((1, 4), F32))
    with pytest.raises(ValueError, match="boxes is 3-d float32"):
        util.nms(_fake((1, 4)), _fake((1, 4)))
    with pytest.raises(ValueError, match="do not agree"):
        util.nms(_fake((1, 4, 4)), _fake((1, 5)))
    with pytest.raises(ValueError, match="max_det"):
        util.nms(_fake((1, 4, 4)), _fake((1, 4)), max_det=0)
    with pytest.raises(ValueError, match="max_candidates"):
        util.decode_detections([host], heads, 3, max_candidates=4097)

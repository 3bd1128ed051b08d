"""Instances as net output, the parts that need no GPU: the header's constants and scratch macro, what `FlowSpec`
and `follow_flows` refuse before they touch a device, the declaration's bookkeeping on a `Net`, and where the four arrays land
in the result tuple."""
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


def _macro(text, name):
    """The body of a function-like macro of the header, as a Python expression: casts dropped, / as //."""
    m = re.search(r"#define %s\(([^)]*)\)((?:[^\n]*\\\n)*[^\n]*)" % name, text)
    assert m, name
    body = m.group(2).replace("\\\n", " ").replace("(size_t)", "").replace("/", "//")
    return [a.strip() for a in m.group(1).split(",")], body


def test_header_constants_agree_with_python():
    from planer_amd import _lib, util
    text = open(os.path.join(ROOT, "include", "planer_hip.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (PL_FLOW_[A-Z_]+) (\d+)", text)}
    assert consts == dict(PL_FLOW_SCAN_STEP=_lib.FLOW_SCAN_STEP, PL_FLOW_MAX_ROUNDS=_lib.FLOW_MAX_ROUNDS,
                          PL_FLOW_MAX_INSTANCES=_lib.FLOW_MAX_INSTANCES)
    assert _lib.FLOW_SCAN_STEP % 64 == 0 and _lib.FLOW_SCAN_STEP <= 1024 and 2 ** _lib.FLOW_MAX_ROUNDS < 1 << 31
    assert "pl_flow_instances_f32" in _lib.SIGNATURES and re.search(r"\bint pl_flow_instances_f32\(", text)
    assert len(_lib.SIGNATURES["pl_flow_instances_f32"]) == 20
    # PL_FLOW_SCRATCH_BYTES as the header writes it, evaluated from its text, against the Python twin
    env = {}
    for name in ("PL_FLOW_ALIGN", "PL_FLOW_MAX_RAW", "PL_CC_SCRATCH_BYTES", "PL_FLOW_SCRATCH_BYTES"):
        args, body = _macro(text, name)
        env[name] = eval("lambda %s: %s" % (", ".join(args), body), dict(env, PL_CC_BLOCK=_lib.CC_BLOCK))
        env[name].__globals__.update(env)
    for n, h, w, m in ((1, 1, 1, 0), (3, 5, 7, 10), (1, 2049, 1, 1), (2, 33, 65, 256), (32, 224, 224, 256)):
        assert util._flow_scratch_bytes(n, h, w, m) == env["PL_FLOW_SCRATCH_BYTES"](n, h, w, m), (n, h, w, m)
    assert env["PL_FLOW_MAX_RAW"](5, 7) == 3 * 4 and env["PL_FLOW_ALIGN"](17) == 32
    # by hand: 16 + sums + four int maps + volume table + sink counts + sink map + the components chain's link and counts
    assert util._flow_scratch_bytes(3, 5, 7, 10) == 16 + 480 + 4 * 432 + 144 + 16 + 112 + (420 + 12)


def test_spec_argument_errors():
    from planer_amd.util import FlowSpec
    spec = FlowSpec()
    assert (spec.level, spec.min_flow, spec.rounds, spec.min_size, spec.max_instances, spec.planes) == (0.0, 0.0, 10, 15, 256, (0, 1, 2))
    assert spec.places == 4 and spec.geometry((2, 3, 64, 48)) == (2, 3, 64, 48)
    assert FlowSpec(0.5, 0.1, 0, 0, 0, (4, 0, 2)).geometry((1, 5, 3, 3)) == (1, 5, 3, 3)
    assert FlowSpec(level=0.1).level == float(F32(0.1)) and FlowSpec(min_flow=0.3).min_flow == float(F32(0.3))
    for name in ("level", "min_flow"):
        for bad in (float("nan"), None, "1", True):
            with pytest.raises(ValueError, match="%s is a number" % name):
                FlowSpec(**{name: bad})
    for bad in (-1, 31, 2.0, None, True):
        with pytest.raises(ValueError, match="rounds is 0 to 30"):
            FlowSpec(rounds=bad)
    for bad in (-1, 1 << 31, 1.5, None):
        with pytest.raises(ValueError, match="min_size is 0 to"):
            FlowSpec(min_size=bad)
    for bad in (-1, 65537, 2.5, None):
        with pytest.raises(ValueError, match="max_instances is 0 to 65536"):
            FlowSpec(max_instances=bad)
    for bad in ((0, 1), (0, 1, 1), (0, 0, 2), (0, 1, -1), (0, 1, 2.0), 3, (0, 1, 2, 3)):
        with pytest.raises(ValueError, match="three distinct planes"):
            FlowSpec(planes=bad)
    with pytest.raises(ValueError, match="planes .* of a result with 2 planes"):
        spec.geometry((1, 2, 4, 4))
    with pytest.raises(ValueError, match="planes .* of a result with 3 planes"):
        FlowSpec(planes=(0, 1, 3)).geometry((1, 3, 4, 4))
    with pytest.raises(ValueError, match="2\\^31 or more pixels"):
        spec.geometry((1, 3, 1 << 16, 1 << 15))
    with pytest.raises(ValueError, match="2\\^31 or more pixels"):
        spec.geometry((1 << 11, 3, 1 << 10, 1 << 10))
    with pytest.raises(ValueError, match="2\\^31 or more table entries"):
        FlowSpec(max_instances=65536).geometry((1 << 13, 3, 4, 4))
    with pytest.raises(TypeError, match="got ndarray"):
        spec.check(np.zeros((1, 3, 4, 4), F32))
    with pytest.raises(ValueError, match="float32 tensor"):
        spec.check(_fake((1, 3, 4)))
    with pytest.raises(TypeError, match="got ndarray"):
        spec.encode(np.zeros((1, 3, 4, 4), F32))
    spec.check(_fake((1, 3, 4, 4)))


def test_follow_flows_refuses_without_a_device():
    from planer_amd import util
    with pytest.raises(TypeError, match="got ndarray"):
        util.follow_flows(np.zeros((3, 4, 4), F32))
    with pytest.raises(ValueError, match="float32 planes"):
        util.follow_flows(_fake((4, 4)))
    with pytest.raises(ValueError, match="float32 planes"):
        util.follow_flows(_fake((1, 3, 4, 4), np.uint8))
    x = _fake((2, 3, 4, 4))
    with pytest.raises(ValueError, match="rounds"):
        util.follow_flows(x, rounds=31)
    with pytest.raises(ValueError, match="level"):
        util.follow_flows(x, level=float("nan"))
    with pytest.raises(ValueError, match="planes"):
        util.follow_flows(x, planes=(0, 1, 3))
    with pytest.raises(ValueError, match="planes"):
        util.follow_flows(_fake((2, 4, 4)))
    with pytest.raises(ValueError, match="pixels"):
        util.follow_flows(_fake((3, 1 << 16, 1 << 15)))


def test_declaration_bookkeeping():
    from planer_amd import Net
    from planer_amd.util import FlowSpec, LabelSpec
    net = Net()
    assert net.flow_output() is net and isinstance(net._image_out[0], FlowSpec)
    net.flow_output(level=0.5, rounds=4, max_instances=9, planes=(2, 0, 1), index=2)
    assert sorted(net._image_out) == [0, 2] and net._image_out[2].max_instances == 9 and net._image_out[2].planes == (2, 0, 1)
    with pytest.raises(ValueError, match="rounds"):
        net.flow_output(rounds=-1, index=1)
    with pytest.raises(ValueError, match="position"):
        net.flow_output(index=-1)
    assert sorted(net._image_out) == [0, 2]
    # declaring again replaces, whatever was there
    net.label_output(index=2)
    assert isinstance(net._image_out[2], LabelSpec)
    net.flow_output(max_instances=3, index=2)
    assert net._image_out[2].max_instances == 3
    # the clash with a detection declaration, from either side
    heads = [([(10, 14)], 8), ([(23, 27)], 16)]
    with pytest.raises(ValueError, match="output 2 is already declared"):
        net.detection_output(heads, 3, indices=(1, 2))
    with pytest.raises(ValueError, match="already declared"):
        net.detection_output(heads, 3)
    net.detection_output(heads, 3, indices=(1, 3))
    with pytest.raises(ValueError, match="output 3 is a head of the declared detection output"):
        net.flow_output(index=3)
    # float_output takes it back
    assert net.float_output(2) is net and sorted(net._image_out) == [0] and net._detect is not None
    net.float_output(0)
    assert net._image_out == {}


def test_result_tuple_arithmetic(monkeypatch):
    from planer_amd import Net
    from planer_amd.util import DetectionSpec, FlowSpec, LabelSpec
    seen = []
    four = ("masks", "num", "instances", "centres")
    monkeypatch.setattr(FlowSpec, "encode", lambda self, x, ctx=None: seen.append(x) or four)
    monkeypatch.setattr(LabelSpec, "encode", lambda self, x, ctx=None: "map")
    monkeypatch.setattr(DetectionSpec, "encode", lambda self, xs, ctx=None: ("det", "num"))
    s, a, b = _fake((2, 3, 8, 8)), _fake((2, 5)), _fake((2, 7))
    # a one-output net: masks, num, instances, centres = net(x)
    assert Net().flow_output()._hand_back(s, False) == four and seen[-1] is s
    assert Net().flow_output()._hand_back((s,), False) == four
    # spliced in at its position, the others untouched
    assert Net().flow_output(index=1)._hand_back((a, s, b), False) == (a,) + four + (b,)
    assert Net().flow_output(index=2)._hand_back((a, b, s), False) == (a, b) + four
    # beside a label output and a second flow output
    net = Net().flow_output(index=0).label_output(index=1).flow_output(index=3)
    assert net._hand_back((s, s, a, s), False) == four + ("map", a) + four
    # beside detections: det, num where the lowest head was
    h = [_fake((2, 8, 8, 8)), _fake((2, 8, 4, 4))]
    net = Net().detection_output([([(10, 14)], 8), ([(23, 27)], 16)], 3, indices=(0, 2)).flow_output(index=1)
    assert net._hand_back((h[0], s, h[1], a), False) == ("det", "num") + four + (a,)
    # checks come first: a position the net does not have, a tensor the step kernel does not take, a host array
    calls = len(seen)
    with pytest.raises(ValueError, match="output 1 is declared .*, the net returns 1"):
        Net().flow_output(index=1)._hand_back(s, False)
    with pytest.raises(ValueError, match="float32 tensor"):
        Net().flow_output()._hand_back(a, False)
    with pytest.raises(ValueError, match="planes"):
        Net().flow_output()._hand_back(_fake((1, 2, 4, 4)), False)
    with pytest.raises(ValueError, match="no device tensor: ndarray"):
        Net().flow_output()._hand_back(np.zeros((2, 3, 8, 8), F32), False)
    assert len(seen) == calls
    # taken back: the float tensor again
    assert Net().flow_output().float_output()._hand_back(s, False) is s


def test_cellnet_is_a_three_plane_unet():
    from planer_amd.irgen import cellnet, unet
    assert cellnet.CLASSES == 3 and cellnet.PLANES == (0, 1, 2)
    graph, blob = cellnet.build()
    assert blob.nbytes == 4 * unet.params(3, 3) and graph["input"] == ["x"]
    assert cellnet.make_input(2, size=64).shape == (2, 3, 64, 64)

"""Text as net output, the parts that need no GPU: the header's constants and the three tables that name
pl_ctc_greedy_f32, what `TextSpec` and `ctc_decode` refuse before they touch a device, the stride sets of the layouts, the
declaration's bookkeeping on a `Net`, the `tiled` refusal, `text_strings`, and the CRNN graphs of irgen/crnn.py."""
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


def test_header_ctypes_and_dispatch_agree():
    from planer_amd import _lib, util
    header = open(os.path.join(ROOT, "include", "planer_hip.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (PL_TEXT_[A-Z_]+) (\d+)", header)}
    assert consts == dict(PL_TEXT_MAX_LEN=_lib.TEXT_MAX_LEN, PL_TEXT_MAX_FRAMES=_lib.TEXT_MAX_FRAMES, PL_TEXT_CHUNK=_lib.TEXT_CHUNK,
                          PL_TEXT_ROW_WAVE_MAX=_lib.TEXT_ROW_WAVE_MAX, PL_TEXT_TIME_LANES=_lib.TEXT_TIME_LANES, PL_TEXT_TIME_GROUPS=_lib.TEXT_TIME_GROUPS,
                          PL_TEXT_CONF_NONE=_lib.TEXT_CONF["none"], PL_TEXT_CONF_SOFTMAX=_lib.TEXT_CONF["softmax"],
                          PL_TEXT_CONF_VALUE=_lib.TEXT_CONF["value"])
    assert _lib.TEXT_MAX_LEN == 1024 and _lib.TEXT_TIME_LANES * _lib.TEXT_TIME_GROUPS == 1024
    # the prototype, the ctypes table and the dispatch table: one entry point, twenty arguments of the same kinds
    proto = re.search(r"\bint pl_ctc_greedy_f32\(([^;]*)\);", header).group(1)
    args = [a.strip() for a in proto.replace("\n", " ").split(",")]
    kinds = ["p" if "*" in a else "q" if a.startswith("long long") else "i" for a in args]
    sig = _lib.SIGNATURES["pl_ctc_greedy_f32"]
    assert len(args) == len(sig) == 20
    assert kinds == ["p" if t is _lib.c_void_p else "q" if t is _lib.c_longlong else "i" for t in sig]
    inc = open(os.path.join(ROOT, "planer_amd", "csrc", "plan_dispatch.inc")).read()
    assert '{"pl_ctc_greedy_f32", 20, &thunk_pl_ctc_greedy_f32}' in inc
    thunk = re.search(r"static int thunk_pl_ctc_greedy_f32\(const PlArg \*a\) \{\s*typedef int \(\*fn_t\)\(([^)]*)\);", inc).group(1)
    assert ["p" if "*" in a else "q" if "long long" in a else "i" for a in thunk.split(",")] == kinds
    # the scratch formula: frame labels plus frame confidences
    assert re.search(r"#define PL_TEXT_SCRATCH_BYTES\(S, T\) \(\(size_t\)\(S\) \* \(size_t\)\(T\) \* 8\)", header)
    assert util._text_scratch_bytes(32, 80) == 32 * 80 * 8 and util._text_scratch_bytes(5, 0) == 0 and util._text_scratch_bytes(0, 9) == 0


def test_spec_arguments_and_geometry():
    from planer_amd.util import TextSpec
    spec = TextSpec()
    assert (spec.layout, spec.blank, spec.merge_repeated, spec.confidence, spec.max_len, spec.places) == ("tnc", 0, True, "softmax", 64, 4)
    # the three layouts as stride sets: lead, S_outer, S_inner, T, C, (st_outer, st_inner, st_time, st_class)
    assert spec.geometry((80, 32, 37)) == ((32,), 32, 1, 80, 37, (37, 0, 32 * 37, 1))
    assert TextSpec("ntc").geometry((32, 80, 37)) == ((32,), 32, 1, 80, 37, (80 * 37, 0, 37, 1))
    assert TextSpec("nchw").geometry((2, 11, 3, 16)) == ((2, 3), 2, 3, 16, 11, (11 * 3 * 16, 16, 1, 3 * 16))
    assert TextSpec("nchw", blank=10).geometry((2, 11, 1, 0))[3] == 0
    for bad in ("nct", "NCHW", None, 3):
        with pytest.raises(ValueError, match="layout is 'tnc', 'ntc' or 'nchw'"):
            TextSpec(layout=bad)
    for bad in (-1, 1.0, None, True, "0"):
        with pytest.raises(ValueError, match="blank is a class number"):
            TextSpec(blank=bad)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="merge_repeated is True or False"):
            TextSpec(merge_repeated=bad)
    for bad in ("max", 1, None, True):
        with pytest.raises(ValueError, match="confidence is 'softmax', 'value' or 'none'"):
            TextSpec(confidence=bad)
    for bad in (0, -1, 1025, 2.0, None, True):
        with pytest.raises(ValueError, match="max_len is 1 to 1024"):
            TextSpec(max_len=bad)
    assert TextSpec(max_len=1024).max_len == 1024 and TextSpec(max_len=np.int64(1)).max_len == 1
    with pytest.raises(ValueError, match="layout 'tnc' takes a 3-d tensor"):
        spec.geometry((2, 3, 4, 5))
    with pytest.raises(ValueError, match="layout 'nchw' takes a 4-d tensor"):
        TextSpec("nchw").geometry((2, 3, 4))
    with pytest.raises(ValueError, match="at least one class"):
        spec.geometry((4, 2, 0))
    with pytest.raises(ValueError, match="blank = 5 is no class of the 5"):
        TextSpec(blank=5).geometry((4, 2, 5))
    with pytest.raises(ValueError, match="frames are above 1048576"):
        TextSpec("ntc").geometry((1, (1 << 20) + 1, 2))
    with pytest.raises(ValueError, match="2\\^31 or more"):
        spec.geometry((1 << 10, 1 << 10, 1 << 11))
    with pytest.raises(TypeError, match="got ndarray"):
        spec.check(np.zeros((4, 2, 3), F32))
    with pytest.raises(ValueError, match="float32 tensor"):
        spec.check(_fake((4, 2, 3), np.int32))
    with pytest.raises(TypeError, match="got ndarray"):
        spec.encode(np.zeros((4, 2, 3), F32))
    spec.check(_fake((4, 2, 3)))
    x = _fake((4, 2, 3))
    for bad in ([1.0, 2.0], [1, 2, 3], np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError, match="lengths is an integer array with one entry per sequence \\(2\\)"):
            spec.encode(x, lengths=bad)
    for bad in (_fake((2,), np.int64), _fake((3,), np.int32)):
        with pytest.raises(ValueError, match="lengths is an int32 array with one entry per sequence \\(2\\)"):
            spec.encode(x, lengths=bad)


def test_ctc_decode_refuses_without_a_device():
    from planer_amd import util
    with pytest.raises(TypeError, match="got ndarray"):
        util.ctc_decode(np.zeros((4, 2, 3), F32))
    with pytest.raises(ValueError, match="layout"):
        util.ctc_decode(_fake((4, 2, 3)), layout="cnt")
    with pytest.raises(ValueError, match="max_len"):
        util.ctc_decode(_fake((4, 2, 3)), max_len=0)
    with pytest.raises(ValueError, match="blank = 3"):
        util.ctc_decode(_fake((4, 2, 3)), blank=3)
    with pytest.raises(ValueError, match="4-d"):
        util.ctc_decode(_fake((4, 2, 3)), layout="nchw")


def test_declaration_bookkeeping():
    from planer_amd import Net
    from planer_amd.util import KeypointSpec, LabelSpec, TextSpec
    net = Net()
    assert net.text_output() is net and isinstance(net._image_out[0], TextSpec)
    net.text_output("nchw", 36, False, "value", 9, index=2)
    t = net._image_out[2]
    assert sorted(net._image_out) == [0, 2] and (t.layout, t.blank, t.merge_repeated, t.confidence, t.max_len) == ("nchw", 36, False, "value", 9)
    with pytest.raises(ValueError, match="confidence"):
        net.text_output(confidence="logit", index=1)
    with pytest.raises(ValueError, match="position"):
        net.text_output(index=-1)
    assert sorted(net._image_out) == [0, 2]
    # declaring again replaces, whatever was there
    net.label_output(index=2)
    assert isinstance(net._image_out[2], LabelSpec)
    net.text_output(max_len=3, index=2)
    assert net._image_out[2].max_len == 3
    net.keypoint_output(index=2)
    assert isinstance(net._image_out[2], KeypointSpec)
    net.text_output(max_len=5, index=2)
    assert isinstance(net._image_out[2], TextSpec)
    # the clash with a detection declaration, from either side
    heads = [([(10, 14)], 8), ([(23, 27)], 16)]
    with pytest.raises(ValueError, match="output 2 is already declared"):
        net.detection_output(heads, 3, indices=(1, 2))
    net.detection_output(heads, 3, indices=(1, 3))
    with pytest.raises(ValueError, match="output 3 is a head of the declared detection output"):
        net.text_output(index=3)
    # float_output takes it back
    assert net.float_output(2) is net and sorted(net._image_out) == [0] and net._detect is not None
    net.float_output(0)
    assert net._image_out == {}


def test_result_tuple_arithmetic(monkeypatch):
    from planer_amd import Net
    from planer_amd.util import TextSpec
    four = ("text", "length", "conf", "spans")
    seen = []
    monkeypatch.setattr(TextSpec, "encode", lambda self, x, ctx=None, lengths=None: seen.append(x) or four)
    s, a = _fake((16, 2, 11)), _fake((2, 5))
    assert Net().text_output()._hand_back(s, False) == four and seen[-1] is s
    assert Net().text_output(index=1)._hand_back((a, s, a), False) == (a,) + four + (a,)
    # checks come first: a 4-d tensor under a 3-d layout, a blank the tensor does not have, a host array
    calls = len(seen)
    with pytest.raises(ValueError, match="layout 'tnc' takes a 3-d tensor"):
        Net().text_output()._hand_back(_fake((2, 11, 1, 16)), False)
    with pytest.raises(ValueError, match="blank = 11"):
        Net().text_output(blank=11)._hand_back(s, False)
    with pytest.raises(ValueError, match="no device tensor: ndarray"):
        Net().text_output()._hand_back(np.zeros((16, 2, 11), F32), False)
    assert len(seen) == calls
    assert Net().text_output("nchw")._hand_back(_fake((2, 11, 1, 16)), False) == four
    assert Net().text_output().float_output()._hand_back(s, False) is s


def test_tiled_refuses_a_text_declaration():
    from planer_amd import Net
    net = Net()
    net.input = ["x"]
    net.text_output("nchw")
    with pytest.raises(ValueError, match="Net.tiled: a text output is declared"):
        net.tiled(np.zeros((64, 64, 3), F32), window=32)
    with pytest.raises(ValueError, match="text output is declared"):
        net.tiled(_fake((64, 64, 3)), window=32)


def test_text_strings():
    from planer_amd.util import text_strings
    alphabet = "-abcdefghij"
    text = np.array([[3, 1, 2, -1], [5, 5, 5, 5], [-1, -1, -1, -1]], np.int32)
    length = np.array([3, 9, 0], np.int32)                  # (the second line had more symbols than max_len)
    assert text_strings(text, length, alphabet) == ["cab", "eeee", ""]
    assert text_strings(text.reshape(1, 3, 4), length.reshape(1, 3), alphabet) == [["cab", "eeee", ""]]     # nested for "nchw"
    assert text_strings(text, length, list(alphabet)) == ["cab", "eeee", ""]
    assert text_strings(text[:0], length[:0], alphabet) == []
    with pytest.raises(ValueError, match="text is \\(\\.\\.\\., max_len\\) and length \\(\\.\\.\\.\\)"):
        text_strings(text, length[:2], alphabet)
    with pytest.raises(ValueError, match="outside the alphabet of 3"):
        text_strings(text, length, "-ab")
    with pytest.raises(ValueError, match="outside the alphabet"):
        text_strings(np.array([[2, -1]], np.int32), np.array([2], np.int32), alphabet)     # a length the text does not back


def test_crnn_graphs():
    """irgen/crnn.py in both forms: the trunk is one channel-quad run down to one row, the recurrent form goes on through two
    bidirectional lstm steps to (T, N, classes), the other ends in a 1 x 1 conv at (N, classes, 1, W / 4); and on the numpy
    oracle the recurrent graph computes what its layers say."""
    from planer_amd.irgen import crnn
    from tests.linear_q4_ref import compile_plan, run_on_oracle, steps_of
    x = crnn.make_input(2, size=(32, 64), channels=3)
    g, b = crnn.build(classes=11, hidden=32, channels=3, recurrent=False)
    body, flow, _, shapes = compile_plan(g, b, x, force=False)
    names = [s[0] for s in steps_of(body, flow)]
    assert names.count("conv_q4") == 8 and names.count("maxpool_q4") == 5 and names[-2:] == ["from_q4", "return"]
    assert shapes["p6"] == (2, 512, 1, 16) and shapes["logits"] == (2, 11, 1, 16)
    g, b = crnn.build(classes=11, hidden=32, channels=3, recurrent=True, batch=2)
    body, flow, _, shapes = compile_plan(g, b, x, force=False)
    names = [s[0] for s in steps_of(body, flow)]
    assert names.count("lstm") == 2 and names.count("conv_q4") == 7 and names[-3:] == ["matmul", "add", "return"]
    assert shapes["seq"] == (16, 2, 512) and shapes["lstm0_Y"] == (16, 2, 2, 32) and shapes["lstm0_o"] == (16, 2, 64)
    assert shapes["fc0"] == (16, 2, 32) and shapes["logits"] == (16, 2, 11)
    y = run_on_oracle(g, b, x, body, flow)
    assert y.shape == (16, 2, 11) and np.isfinite(y).all() and len(np.unique(y.argmax(-1))) > 1
    assert [i[0] for i in g["inits"] if i[0].startswith("lstm0_")] == ["lstm0_" + s for s in ("W", "R", "B", "lens", "h0", "c0", "shape")]
    with pytest.raises(ValueError, match="height is a power of two"):
        crnn.build(height=24)

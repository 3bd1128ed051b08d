"""Anchor-free heads and prototype masks, the parts that need no GPU: util.DetectionSpec's geometry and refusals for
("dfl", stride[, reg_max]) heads and `protos`, and the header's constants and entries against _lib's."""
import pytest

from planer_amd import _lib
from planer_amd.util import DetectionSpec
from tests.head_kit import header_constants
from tests.test_abi import header_functions

ENTRIES = {"pl_dfl_decode_f32": 16, "pl_nms_rows_f32": 15, "pl_dfl_coefficients_f32": 14, "pl_proto_masks_f32": 13}


def test_header_constants_and_entries():
    consts = dict(header_constants("PL_DFL_"), **header_constants("PL_MASK_"))
    assert consts == {"PL_DFL_MAX_REG": _lib.DFL_MAX_REG, "PL_MASK_MAX_DET": _lib.MASK_MAX_DET, "PL_MASK_MAX_COEF": _lib.MASK_MAX_COEF}
    assert (_lib.DFL_MAX_REG, _lib.MASK_MAX_DET, _lib.MASK_MAX_COEF) == (32, 128, 64)
    for name, count in ENTRIES.items():
        assert name in header_functions() and len(_lib.SIGNATURES[name]) == count, name


def test_geometry():
    spec = DetectionSpec([("dfl", 8), ("dfl", (16, 15.5), 4), ("dfl", None, 1)], 3, size=(64, 96), max_det=300, max_candidates=50)
    n, rows, total, k, max_det = spec.geometry([(2, 67, 8, 12), (2, 19, 4, 6), (2, 7, 2, 3)])
    assert (n, total, k, max_det) == (2, 96 + 24 + 6, 50, 50)
    assert rows == [(16, 3, 8, 12, 8.0, 8.0, 0), (4, 3, 4, 6, 16.0, 15.5, 96), (1, 3, 2, 3, 32.0, 32.0, 120)]
    masked = DetectionSpec([("dfl", 8, 2), ("dfl", 16, 2)], 3, size=(64, 96), protos=2)
    assert masked.geometry([(2, 19, 8, 12), (2, 19, 4, 6)], (2, 8, 16, 24)) == (
        2, [(2, 3, 8, 12, 8.0, 8.0, 0), (2, 3, 4, 6, 16.0, 16.0, 96)], 120, 120, 100, (8, 16, 24))
    # an anchor declaration is what it was
    plain = DetectionSpec([([(10, 13), (16, 30)], 8)], 2)
    assert not plain.dfl and plain.geometry([(1, 14, 3, 4)]) == (1, [(2, 2, 3, 4, 8.0, 8.0, 0)], 24, 24, 24)


@pytest.mark.parametrize("heads, kw, match", [
    ([("dfl", 8), ([(10, 13)], 8)], {}, "a mix"),
    ([([(10, 13)], 8), ("dfl", 8)], {}, "a mix"),
    ([("dfl", 8, 0)], {}, "reg_max"),
    ([("dfl", 8, 33)], {}, "reg_max"),
    ([("dfl", 8, 2.0)], {}, "reg_max"),
    ([("dfl",)], {}, "stride"),
    ([("dlf", 8)], {}, "stride"),
    ([([(10, 13)], 8)], dict(protos=1, size=(64, 64)), "\"dfl\" heads only"),
    ([("dfl", 8)], dict(protos=1, size=(64, 64), max_det=129), "max_det is 1 to 128"),
    ([("dfl", 8)], dict(protos=1), "need size"),
])
def test_declaration_refusals(heads, kw, match):
    with pytest.raises(ValueError, match=match):
        DetectionSpec(heads, 3, **kw)
    DetectionSpec([("dfl", 8)], 3, protos=1, size=(64, 64), max_det=128)


@pytest.mark.parametrize("shapes, protos, match", [
    ([(2, 4 * 16 + 3 + 8 + 1, 8, 8)], (2, 8, 16, 16), "76 channels, 4 x 16 bins \\+ 3 classes \\+ 8 coefficients is 75"),
    ([(2, 75, 8, 8)], (2, 6, 16, 16), "6 planes"),
    ([(2, 75, 8, 8)], (2, 0, 16, 16), "0 planes"),
    ([(2, 75, 8, 8)], (2, 68, 16, 16), "68 planes"),
    ([(2, 75, 8, 8)], (3, 8, 16, 16), "batch size 3"),
    ([(2, 75, 8, 8)], (2, 8, 16), "protos is a float32 tensor"),
    ([(2, 75, 8, 8)], None, "protos is a float32 tensor"),
    ([(2, 75, 8)], (2, 8, 16, 16), "head 0 is"),
])
def test_geometry_refusals(shapes, protos, match):
    spec = DetectionSpec([("dfl", 8)], 3, protos=1, size=(64, 64))
    with pytest.raises(ValueError, match=match):
        spec.geometry(shapes, protos)
    with pytest.raises(ValueError, match="69 channels"):                    # without protos Md is 0
        DetectionSpec([("dfl", 8)], 3).geometry([(2, 69, 8, 8)])

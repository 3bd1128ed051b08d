"""uint16 image batches and percentile scaling, the parts that need no GPU: what ImageSpec refuses, the numpy
mirror of the contract against np.percentile, and the new entry points in the header and the ctypes table."""
import os
import re

import numpy as np
import pytest

from planer_amd import _lib, util
from tests import image16_ref as R16
from tests.conftest import ROOT


@pytest.mark.parametrize("bad", [("percentile", 99, 1), ("percentile", -1, 50), ("percentile", 0, 100.5), ("percentile", 1),
                                 ("minmax", 0, 100), ("percentile", "1", 99), ("percentile", float("nan"), 99), "percentile"])
def test_a_normalise_that_is_no_percentile_pair_is_a_value_error(bad):
    with pytest.raises(ValueError, match="normalise"):
        util.ImageSpec(np.ones(3), np.zeros(3), normalise=bad)


def test_what_a_spec_takes_and_refuses():
    spec = util.ImageSpec(np.ones(1), np.zeros(1), normalise=("percentile", 1, 99.5))
    assert spec.normalise == ("percentile", 1.0, 99.5)
    assert util.ImageSpec(np.ones(1), np.zeros(1)).normalise is None
    assert spec.geometry((2, 46340, 46340, 1)) == ((2, 46340, 46340, 1), (2, 1, 46340, 46340))      # 46340^2 < 2^31
    with pytest.raises(NotImplementedError, match="32-bit"):
        spec.geometry((1, 1 << 16, 1 << 15, 1))                                                      # 2^31 samples in a plane
    with pytest.raises(TypeError, match="or a uint16 one"):
        util.ImageFeed(spec, np.zeros((1, 4, 4, 1), np.uint16))                                      # a host array is no feed


@pytest.mark.parametrize("pct", [(1, 99), (0, 100), (50, 50), (0.1, 99.9)])
@pytest.mark.parametrize("m", [1, 2, 7, 1000, 4097])
def test_the_mirror_is_numpys_linear_percentile(m, pct):
    """Each side rounds a difference-times-fraction and a sum, relative to a p that lies between the two samples (numpy's
    form for g >= 0.5, s_j1 - (s_j1 - s_j)(1 - g), rounds relative to s_j1 <= 2 p): 4 ulps of p cover both."""
    planes = np.random.default_rng(m).integers(0, 65536, (3, 1, m)).astype(np.uint16)
    got = R16.percentiles(planes, *pct)
    for g, q in zip(got, pct):
        want = np.percentile(planes.astype(np.float64), q, axis=(1, 2))
        assert (np.abs(g - want) <= 4 * np.spacing(np.abs(want))).all(), (g, want)


def test_header_and_ctypes_table_hold_the_new_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "planer_hip.h")).read(), flags=re.S)
    for name in ("pl_image_u16_nchw_f32", "pl_image_norm_nchw_f32", "pl_image_norm_scratch_bytes"):
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name]), name
    assert len(_lib.SIGNATURES["pl_image_u16_nchw_f32"]) == len(_lib.SIGNATURES["pl_image_u8_nchw_f32"])

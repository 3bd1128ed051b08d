"""bench.py --dump-outputs on the host side: the size cap and the fixed sample beyond it.  CPU only."""
import os

import numpy as np

import bench


def test_small_outputs_are_written_whole(tmp_path):
    y = np.random.default_rng(0).standard_normal((32, 1000)).astype(np.float32)
    bench.dump_outputs(str(tmp_path), ["logits", "idx"], [y, np.arange(5)])
    np.testing.assert_array_equal(np.load(tmp_path / "logits.npy"), y)
    i = np.load(tmp_path / "idx.npy")
    assert i.dtype == np.float64 and i.tolist() == [0, 1, 2, 3, 4]


def test_large_outputs_are_sampled_under_the_cap_with_a_fixed_sample(tmp_path):
    y = np.random.default_rng(3).standard_normal((8, 64, 224, 224)).astype(np.float32)     # config 2's output: 102.8 MB
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), ["y"], [y])
    assert os.path.getsize(tmp_path / "a" / "y.npy") <= bench.DUMP_LIMIT_BYTES
    a = np.load(tmp_path / "a" / "y.npy")
    assert a.dtype == np.float32 and a.size > 0.9 * bench.DUMP_LIMIT_BYTES / 4
    np.testing.assert_array_equal(a, np.load(tmp_path / "b" / "y.npy"))
    s = np.sort(y, axis=None)                                     # every value comes from the output
    assert np.array_equal(s[np.minimum(np.searchsorted(s, a), s.size - 1)], a)

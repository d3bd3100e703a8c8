"""bench.py's --dump-outputs plumbing on the CPU: the choice of dumped problems (all of them
when they fit, else a fixed seeded sample under the byte budget) and the files written."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, ROOT)
    import bench as B
    return B


def test_dump_sample_takes_every_problem_that_fits(bench):
    np.testing.assert_array_equal(bench.dump_sample(37, 1000), np.arange(37))
    n = bench.DUMP_BUDGET_BYTES // 1000
    np.testing.assert_array_equal(bench.dump_sample(n, 1000), np.arange(n))


def test_dump_sample_is_fixed_sorted_and_within_budget(bench):
    row = 184320  # one C3 problem: 23040 doubles of trajectories, gains and cost-to-go
    a, b = bench.dump_sample(1024, row), bench.dump_sample(1024, row)
    np.testing.assert_array_equal(a, b)
    assert len(a) == bench.DUMP_BUDGET_BYTES // row < 1024
    assert len(np.unique(a)) == len(a) and (np.diff(a) > 0).all()
    assert 0 <= a[0] and a[-1] < 1024
    assert len(a) * row <= bench.DUMP_BUDGET_BYTES < 64 * 10**6
    assert len(bench.dump_sample(5, 10**9)) == 1  # never empty


def test_write_dump_names_and_dtype(bench, tmp_path):
    arrs = {"J": np.arange(3, dtype=np.float64), "trace": np.arange(6, dtype=np.int32).reshape(3, 2)}
    bench.write_dump(str(tmp_path / "one"), arrs, 0, 1)
    assert sorted(os.listdir(tmp_path / "one")) == ["J.npy", "trace.npy"]
    t = np.load(tmp_path / "one" / "trace.npy")
    assert t.dtype == np.float64 and t.shape == (3, 2)
    np.testing.assert_array_equal(t, arrs["trace"])
    bench.write_dump(str(tmp_path / "two"), arrs, 1, 2)
    assert sorted(os.listdir(tmp_path / "two")) == ["J_rank1.npy", "trace_rank1.npy"]

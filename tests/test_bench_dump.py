"""bench.py --dump-outputs on the CPU: how a field is stored (bench.dump_sample).

A field within the size limit is stored whole, as float64 with one row per column.  A larger one is
stored as a sample of its columns: within the limit, the same columns whenever the shape is the
same (so two builds' files compare row for row), in ascending order."""
import numpy as np

import bench  # the repository root is on sys.path (conftest.py)


def test_small_field_is_stored_whole():
    a = np.arange(7 * 5 * 3, dtype=np.float32).reshape(7, 5, 3)
    s = bench.dump_sample(a)
    assert s.dtype == np.float64 and s.shape == (7, 15) and s.flags["C_CONTIGUOUS"]
    assert np.array_equal(s, a.reshape(7, 15))


def test_large_field_is_a_fixed_sample_of_its_columns():
    rng = np.random.default_rng(1)
    a = rng.standard_normal((1000, 56))
    limit = 100 * 56 * 8 + 17  # room for 100 columns and a bit
    s = bench.dump_sample(a, max_bytes=limit)
    assert s.shape == (100, 56) and s.nbytes <= limit
    # rows of a, each once, in ascending column order
    idx = [int(np.flatnonzero((a == row).all(axis=1))[0]) for row in s]
    assert idx == sorted(set(idx)) and len(idx) == 100
    # the same columns for another field of that shape, and in another call
    b = a + 1.0
    assert np.array_equal(bench.dump_sample(b, max_bytes=limit), b[idx])
    assert np.array_equal(bench.dump_sample(a, max_bytes=limit), s)


def test_default_limit_keeps_five_fields_under_64_mb():
    assert 5 * bench.DUMP_FIELD_BYTES <= 64 * 2 ** 20
    a = np.zeros((163842, 56))
    s = bench.dump_sample(a)
    assert s.nbytes <= bench.DUMP_FIELD_BYTES and s.shape[0] == bench.DUMP_FIELD_BYTES // (56 * 8)

"""bench.py --dump-outputs, host only: dump_outputs writes every result array of a step as <name>.npy in float64, exactly;
whole while they fit the limit, beyond it a seeded sample of rows with the row indices beside it, never more than the limit."""
import os

import numpy as np

import bench


def _result(n_cols, n_mums):
    rng = np.random.default_rng(5)
    return {"n_cols": n_cols, "col_bytes": 1,
            "cols": rng.integers(0, 32, n_cols, dtype=np.uint8),
            "mum_start": rng.integers(-(1 << 31), 1 << 31, (n_mums, 5), dtype=np.int32),
            "left": rng.integers(-(1 << 40), 1 << 40, (100, 5)),
            "reverse": np.zeros((0, 5), np.int8),
            "tree": (np.arange(9, dtype=np.int32), np.arange(9, 0, -1, dtype=np.int32)),
            "dist": np.ones((5, 5), np.int64)}


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_small_result_whole(tmp_path):
    res = _result(1000, 50)
    w = bench.dump_outputs(res, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in ("cols", "mum_start", "left", "reverse", "tree_left", "tree_right", "dist"))
    for k, a in [(k, v) for k, v in res.items() if isinstance(v, np.ndarray)] + [("tree_left", res["tree"][0]), ("tree_right", res["tree"][1])]:
        got = np.load(str(tmp_path / (k + ".npy")))
        assert got.dtype == np.float64 and np.array_equal(got, a.astype(np.float64)) and got.shape == a.shape, k
        assert w[k] == [list(a.shape), a.shape[0]]


def test_dump_large_result_sampled_within_limit(tmp_path):
    res = _result(9_000_000, 800_000)
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    w = bench.dump_outputs(res, d1)
    assert bench.dump_outputs(res, d2) == w
    assert _size(d1) <= bench.DUMP_LIMIT_BYTES
    for k in ("cols", "mum_start"):
        assert 0 < w[k][1] < res[k].shape[0]
        rows = np.load(os.path.join(d1, k + "_sample_rows.npy")).astype(np.int64)
        assert len(rows) == w[k][1] and np.all(np.diff(rows) > 0)
        got = np.load(os.path.join(d1, k + ".npy"))
        assert np.array_equal(got, res[k][rows].astype(np.float64))
        assert np.array_equal(got, np.load(os.path.join(d2, k + ".npy")))          # the same sample on every run
    assert np.array_equal(np.load(os.path.join(d1, "left.npy")), res["left"].astype(np.float64))

"""bench.py --dump-outputs (runs on CPU): finite files that still say exactly what the caller received, within the size limit."""
import os

import numpy as np

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_is_finite_and_keeps_every_value(tmp_path):
    rng = np.random.default_rng(3)
    n, H = 256, 40
    bt = rng.integers(0, H, n).astype(np.int32)
    past = np.arange(H)[None, :] > bt[:, None]
    path_idx = np.where(past, -1, rng.integers(0, 7000, (n, H))).astype(np.int32)
    path_dist = np.where(past, np.nan, rng.random((n, H)) * 50.0)          # NaN past best_t, as the solver returns it
    speed = rng.random(n)
    speed[[3, 7, 11]] = [np.nan, np.inf, -np.inf]
    bench.dump_outputs(str(tmp_path), {"path_idx": path_idx, "best_t": bt, "path_dist": path_dist, "speed": speed})
    got = _load(str(tmp_path))
    assert sorted(got) == ["best_t", "path_dist", "path_dist_nonfinite", "path_idx", "speed", "speed_nonfinite"]
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in got.values())
    assert np.array_equal(got["path_idx"], path_idx) and np.array_equal(got["best_t"], bt)
    assert np.array_equal(got["path_dist_nonfinite"], past.astype(np.float64))
    assert np.array_equal(got["path_dist"][~past], path_dist[~past]) and not got["path_dist"][past].any()
    assert got["speed_nonfinite"][[3, 7, 11]].tolist() == [1.0, 2.0, 3.0] and got["speed_nonfinite"].sum() == 6.0
    keep = np.isfinite(speed)
    assert np.array_equal(got["speed"][keep], speed[keep])


def test_dump_over_the_limit_keeps_a_fixed_sample(tmp_path):
    n, H = 120000, 40                                                       # ~77 MB as float64 with its codes: must be sampled
    cost = np.arange(n, dtype=np.float64)
    arrays = {"path_idx": np.zeros((n, H), np.int32), "path_dist": np.ones((n, H)), "cost": cost}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    size = sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a")))
    assert size <= bench.DUMP_LIMIT_BYTES
    rows = a["sample_rows"]
    assert 0 < len(rows) < n and np.array_equal(a["cost"], rows) and all(v.shape[0] == len(rows) for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)

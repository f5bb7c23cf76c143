"""bench.py --dump-outputs (CPU): the gathered record block written as float
arrays, and the size cap's seeded row sample."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import shard  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_records_round_trips_the_block(tmp_path):
    rng = np.random.default_rng(3)
    recs = [[(int(rng.integers(0, 51866)), 2 * j, 2 * j + 3, float(np.float32(rng.random())))
             for j in range(n)] for n in (5, 0, 9, 1)]
    bench.dump_records(str(tmp_path), shard.pack_records(recs, 12))
    a = _load(str(tmp_path))
    assert sorted(a) == ["token_count", "token_id", "token_p", "token_t0", "token_t1"]
    assert a["token_p"].dtype == np.float32
    assert all(a[k].dtype == np.float64 for k in a if k != "token_p")
    assert a["token_count"].tolist() == [5, 0, 9, 1]
    assert all(a[k].shape == (4, 9) for k in a if k != "token_count")  # longest clip, not capacity
    for c, r in enumerate(recs):
        n = len(r)
        got = list(zip(a["token_id"][c, :n].astype(int), a["token_t0"][c, :n].astype(int),
                       a["token_t1"][c, :n].astype(int), a["token_p"][c, :n].astype(float)))
        assert got == r
        assert all((a[k][c, n:] == -1).all() for k in a if k != "token_count")


def test_dump_over_the_limit_is_a_fixed_row_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    x = np.arange(100 * 16, dtype=np.float64).reshape(100, 16)
    for d in ("a", "b"):
        bench.write_dump(str(tmp_path / d), {"x": x, "y": x[:, 0].astype(np.float32)})
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(v.nbytes for v in a.values()) <= 4096
    rows = a["sample_rows"].astype(int)
    assert 0 < len(rows) < 100 and (np.diff(rows) > 0).all()
    assert (a["x"] == x[rows]).all() and (a["y"] == x[rows, 0]).all()
    assert all((a[k] == b[k]).all() for k in a)  # the same rows in every run

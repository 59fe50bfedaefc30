"""bench.py --dump-outputs: every column of the placement log as <column>.npy in float64,
exact for the engine's dtypes; a log over the size limit is cut to the same seeded rows of
every column, the same from run to run."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402


def _log(n):
    rng = np.random.default_rng(3)
    return {"pl_task": rng.permutation(n).astype(np.int32), "pl_worker": rng.integers(0, 1024, n).astype(np.int32),
            "pl_comm": rng.integers(0, 1 << 50, n), "pl_start": rng.random(n),
            "pl_wsnbytes": rng.integers(0, 1 << 50, n), "pl_route": rng.integers(0, 5, n).astype(np.int8)}


def test_dump_writes_every_column_exactly(tmp_path):
    out = _log(1000)
    bench.dump_outputs(str(tmp_path / "d"), out)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(k + ".npy" for k in out)
    for k, v in out.items():
        got = np.load(tmp_path / "d" / (k + ".npy"))
        assert got.dtype == np.float64 and got.shape == v.shape
        assert np.array_equal(got.astype(v.dtype), v), k


def test_dump_samples_a_large_log(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 100_000)
    out = _log(5000)  # 6 columns x 5000 rows x 8 bytes = 240 kB
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out)
    files = [tmp_path / "a" / f for f in os.listdir(tmp_path / "a")]
    assert sum(os.path.getsize(f) for f in files) <= 100_000
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in out}
    rows = len(a["pl_task"])
    assert 0 < rows < 5000 and all(len(v) == rows for v in a.values())
    # the same rows of every column, in log order: pl_task is a permutation, so it names them
    idx = np.flatnonzero(np.isin(out["pl_task"], a["pl_task"].astype(np.int32)))
    for k, v in out.items():
        assert np.array_equal(a[k], v[idx].astype(np.float64)), k
        assert np.array_equal(a[k], np.load(tmp_path / "b" / (k + ".npy"))), k

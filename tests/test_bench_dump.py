"""CPU: bench.py's --dump-outputs writer -- float32 / float64 arrays only, 64 MB at most (larger outputs are cut to a fixed,
seeded sample), the same files from the same arrays."""
import numpy as np

import bench        # the repository root is on sys.path (tests/conftest.py)


def test_dump_outputs_types_and_names(tmp_path):
    bench.dump_outputs(str(tmp_path), {"loss": [1.5], "w": np.arange(10, dtype=np.float16), "g": np.ones(4, np.float64)})
    got = {f.stem: np.load(f) for f in tmp_path.glob("*.npy")}
    assert set(got) == {"loss", "w", "g"}
    assert got["loss"].dtype == np.float64 and got["loss"].tolist() == [1.5]
    assert got["w"].dtype == np.float32 and got["w"].tolist() == list(range(10))
    assert got["g"].dtype == np.float64


def test_dump_outputs_samples_above_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "MAX_DUMP_BYTES", 4000)
    big = np.arange(5000, dtype=np.float32)
    small = np.arange(100, dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a = {f.stem: np.load(f) for f in (tmp_path / "a").glob("*.npy")}
    b = {f.stem: np.load(f) for f in (tmp_path / "b").glob("*.npy")}
    assert sum(x.nbytes for x in a.values()) <= 4000
    assert np.array_equal(a["small"], small)
    assert a["big"].size > 0 and np.all(np.diff(a["big"]) > 0) and np.isin(a["big"], big).all()
    assert all(np.array_equal(a[k], b[k]) for k in a)

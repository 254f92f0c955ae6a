"""Fixture storage (CPU): conftest.save_golden writes a fixture as one .npz or
as numbered parts under the size cap, and load_golden joins them bit for bit;
no committed fixture file reaches 1 MiB."""
import glob
import os

import numpy as np

import conftest


def test_parts_round_trip_bit_for_bit(tmp_path, monkeypatch):
    monkeypatch.setattr(conftest, "GOLDEN", str(tmp_path))
    monkeypatch.setattr(conftest, "PART_BYTES", 16 * 1024)
    rng = np.random.default_rng(3)
    arrays = {
        "names": np.array(["a.weight", "b.bias"]),
        "big": rng.standard_normal((3, 5, 701)).astype(np.float32),   # several slices
        "scalar": np.float64(2.5),
        "mid": rng.standard_normal(1500),
        "empty": np.zeros((0, 4), dtype=np.float32),
    }
    conftest.save_golden("t", arrays)
    files = sorted(os.listdir(tmp_path))
    assert len(files) > 2 and files[0] == "t.00.npz" and "t.npz" not in files
    assert all(os.path.getsize(tmp_path / f) <= 16 * 1024 for f in files)
    back = conftest.load_golden("t")
    assert list(back) == list(arrays)
    for k, a in arrays.items():
        a = np.asarray(a)
        assert back[k].dtype == a.dtype and back[k].shape == a.shape and back[k].tobytes() == a.tobytes(), k
    # a fixture that fits is one plain file, and replaces the parts
    conftest.save_golden("t", {"scalar": arrays["scalar"]})
    assert os.listdir(tmp_path) == ["t.npz"] and float(conftest.load_golden("t")["scalar"]) == 2.5


def test_committed_fixtures_stay_under_one_mib():
    files = glob.glob(os.path.join(conftest.GOLDEN, "*.npz"))
    assert files and max(os.path.getsize(p) for p in files) < 2**20

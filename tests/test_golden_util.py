"""Golden fixtures larger than a committed file may be are stored as <name>.part<k>.npz: golden_util.save_npz splits,
golden_util.load_npz reads the parts back as one np.load result."""
import os

import numpy as np

import golden_util as gu


def test_save_npz_splits_and_load_npz_joins_bit_identically(tmp_path):
    rng = np.random.RandomState(0)
    arrays = {"g/%d/x" % i: rng.standard_normal(400 + i).astype(np.float32) for i in range(40)}
    arrays["g/ids"] = np.arange(7, dtype=np.int64)
    path = str(tmp_path / "f.npz")
    paths = gu.save_npz(path, arrays, limit=20000)
    assert len(paths) > 1 and not os.path.exists(path) and all(os.path.getsize(p) <= 20000 for p in paths)
    z = gu.load_npz(path)
    assert z.files == list(arrays) and "g/ids" in z and len(z) == len(arrays)
    for k, v in arrays.items():
        assert z[k].dtype == v.dtype and z[k].tobytes() == v.tobytes()
    z.close()
    # small enough: one ordinary file, and the stale parts are gone
    assert gu.save_npz(path, {"a": np.ones(3)}) == [path] and gu.part_paths(path) == []
    assert np.array_equal(gu.load_npz(path)["a"], np.ones(3))


def test_committed_fixtures_are_under_one_mib():
    for f in os.listdir(gu.GOLDEN):
        assert os.path.getsize(os.path.join(gu.GOLDEN, f)) < 1 << 20, f

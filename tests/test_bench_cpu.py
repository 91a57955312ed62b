"""bench.py's --dump-outputs plumbing on the host: the sampled cells are fixed, bounded
and slab-independent, and the files hold float64 (complex as (re, im) pairs)."""
import os

import numpy as np

import bench


class FakeSolver:
    """A slab [z0, z0 + nzl) of a known global field behind the Solver's read-back calls."""

    def __init__(self, full, plane, z0, nzl):
        self.z0, self.nzl, self.n_local = z0, nzl, nzl * plane
        self._u = full[z0 * plane:(z0 + nzl) * plane]

    def get_field(self):
        return self._u.copy()

    def get_sg_velocity(self, dt):
        return self._u.real * dt


def test_dump_sample_index_fixed_and_bounded():
    total = 512 ** 3
    a, b = bench.dump_sample_index(total), bench.dump_sample_index(total)
    assert np.array_equal(a, b) and a.dtype == np.int64
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < total
    assert 0.9 * bench.DUMP_MAX_CELLS < a.size <= bench.DUMP_MAX_CELLS
    # the largest dump: two arrays (u, v) or one complex array, 16 B per sampled cell
    assert bench.DUMP_MAX_CELLS * 16 <= 64e6
    small = bench.dump_sample_index(1000)
    assert np.array_equal(small, np.arange(1000))


def test_as_real_layout():
    z = np.array([1 + 2j, 3 - 4j])
    r = bench.as_real(z)
    assert r.dtype == np.float64 and r.tolist() == [[1.0, 2.0], [3.0, -4.0]]
    x = np.arange(3, dtype=np.float64)
    assert bench.as_real(x).dtype == np.float64 and np.array_equal(bench.as_real(x), x)


def test_dump_outputs_complex_whole_field(tmp_path):
    w = dict(bench.WORKLOADS["nlse3d_512"], n=12)
    full = bench.synthetic_ic(w, 0, 12)
    bench.dump_outputs(str(tmp_path / "d"), FakeSolver(full, 144, 0, 12), w, 1e-3, None, 1, 0)
    assert os.listdir(tmp_path / "d") == ["u.npy"]
    u = np.load(tmp_path / "d" / "u.npy")
    assert u.dtype == np.float64 and u.shape == (12 ** 3, 2)
    assert np.array_equal(u[:, 0] + 1j * u[:, 1], full)


def test_dump_outputs_samples_the_slab(tmp_path, monkeypatch):
    """A sampled real (Gautschi) field: a rank writes the sampled cells that lie in its slab."""
    monkeypatch.setattr(bench, "DUMP_MAX_CELLS", 500)
    w = dict(bench.WORKLOADS["sg2d_8192"], n=64)
    full = bench.synthetic_ic(w, 0, 64)
    idx = bench.dump_sample_index(64 * 64)
    assert 400 < idx.size <= 500
    bench.dump_outputs(str(tmp_path / "a"), FakeSolver(full, 64, 0, 64), w, 0.5, None, 1, 0)
    assert sorted(os.listdir(tmp_path / "a")) == ["u.npy", "v.npy"]
    u, v = np.load(tmp_path / "a" / "u.npy"), np.load(tmp_path / "a" / "v.npy")
    assert u.dtype == v.dtype == np.float64
    assert np.array_equal(u, full[idx]) and np.array_equal(v, 0.5 * full[idx])
    # rows 16..39 only: the same cells, restricted to the slab
    bench.dump_outputs(str(tmp_path / "b"), FakeSolver(full, 64, 16, 24), w, 0.5, None, 1, 0)
    part = idx[(idx >= 16 * 64) & (idx < 40 * 64)]
    assert np.array_equal(np.load(tmp_path / "b" / "u.npy"), full[part])

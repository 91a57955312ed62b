"""bench.py's command-line contract on a tiny grid: a plain run times --steps steps and
prints the headline line only, --full adds the timing-pass and roofline entries, and
--dump-outputs writes the field the last timed step left -- the same field with and
without --full, and the one a caller of the same Solver calls reads back."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu
nls_amd = pytest.importorskip("nls_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M, STEPS, WARMUP = 32, 8, 3, 1
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def run_bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--n", str(N), "--m", str(M), *extra],
                       stdout=subprocess.PIPE, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1  # the contract: one JSON line on stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def direct_field():
    """The bench's timed path through the Solver itself: same field, same calls."""
    w = dict(bench.WORKLOADS["nlse3d_512"], n=N, m=M)
    dx = 2 * w["L"] / (N - 1)
    u = bench.synthetic_ic(w, 0, N)
    u /= np.sqrt(bench.global_mass(u, dx ** 3))
    with nls_amd.Solver(3, N, N, N, dx, dx, equation=w["eq"], m=M, device=0) as s:
        s.set_field(u)
        s.step(w["dt"], WARMUP)
        s.step(w["dt"], STEPS)
        return s.get_field()


def load_u(d):
    a = np.load(os.path.join(d, "u.npy"))
    assert a.dtype == np.float64 and a.shape == (N ** 3, 2)
    return a[:, 0] + 1j * a[:, 1]


def test_plain_run_and_dump(tmp_path, direct_field):
    r = run_bench("--dump-outputs", str(tmp_path / "plain"))
    assert all(k in r for k in HEADLINE_KEYS)
    assert r["steps"] == STEPS and r["warmup"] == WARMUP and r["unit"] == "Mcells*steps/s"
    assert r["higher_is_better"] is True and r["dtype"] == "c128 (fp64 complex)"
    assert r["ms_per_step"] > 0
    assert r["value"] == pytest.approx(N ** 3 / (r["ms_per_step"] * 1e-3) / 1e6, rel=1e-12)
    # what takes runs of its own stays behind --full
    assert not {"roofline", "step_roofline", "cpu_baseline"} & set(r)
    assert os.listdir(tmp_path / "plain") == ["u.npy"]
    # same library, same inputs, same calls: reproducible to the bit (test_gpu_fullsize.py)
    assert np.array_equal(load_u(tmp_path / "plain"), direct_field)


def test_full_run_adds_roofline_and_dumps_the_same_field(tmp_path, direct_field):
    r = run_bench("--full", "--no-cpu-baseline", "--prof-steps", "1", "--dump-outputs", str(tmp_path / "full"))
    assert all(k in r for k in HEADLINE_KEYS) and r["steps"] == STEPS
    assert r["roofline"]["unit"] == "GB/s" and r["roofline"]["avg_launch_ms"] > 0
    assert r["step_roofline"]["gpu_kernel_ms_per_step"]
    # the dump is taken before the timing pass moves the state on
    assert np.array_equal(load_u(tmp_path / "full"), direct_field)

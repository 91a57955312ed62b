"""What observing costs (include/nls.h "Observables"): one process, one handle, the flagship
workload -- 3D cubic NLSE, 512^3, m = 16 -- stepping step(dt, 20)
  1. unmonitored,
  2. with monitor(10, 4)   (2 records per call),
  3. with monitor(1, 32)   (a record after every step),
three interleaved repeats each, host clock around work that ends in a sync; then one run
with per-kernel timing on, where k_observe books under class 3 (pointwise; nothing else of
a steady-state NLSE step does) and k_alpha_l2 -- the pass that streams the same 16 B/cell --
is the only class-0 (alpha) launch of a step, so the two class means compare the kernels
from the same process.
usage: python tools/obs_cost.py [n=512] [m=16] [steps=20] [--plain-only]
--plain-only: variant 1 alone, to time another build of the library (NLS_AMD_LIB = its
libnls_amd.so, NLS_AMD_PKG = the directory holding that build's nls_amd binding)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("NLS_AMD_PKG") or os.path.join(ROOT, "nonlinear-solvers_amd"))
import nls_amd  # noqa: E402

pos = [a for a in sys.argv[1:] if not a.startswith("--")]
n, m, steps = (int(pos[i]) if len(pos) > i else d for i, d in enumerate((512, 16, 20)))
plain_only = "--plain-only" in sys.argv
dt = 1e-3
dx = 20.0 / (n - 1)
rng = np.random.default_rng(0)
x = np.linspace(-10, 10, n)
u0 = (np.exp(-(x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2) / 8)
      + 1e-3 * rng.standard_normal((n, n, n))).astype(np.complex128).ravel()
VARIANTS = [("unmonitored", None)] if plain_only else [("unmonitored", None), ("monitor(10, 4)", (10, 4)),
                                                        ("monitor(1, 32)", (1, 32))]
print(f"obs_cost: {n}^3 cubic NLSE, m = {m}, step(dt, {steps}); library {os.path.relpath(nls_amd.lib_path(), ROOT)}")
print(f"build: {nls_amd.build_info().get('src_sha256', '?')[:16]}")
with nls_amd.Solver(3, n, n, n, dx, dx, m=m) as s:
    s.set_field(u0)
    s.step(dt, 3)  # warm bases, code objects loaded
    if not plain_only:
        s.observe()  # the observation buffers and kernels too
    s.sync()
    ms = {name: [] for name, _ in VARIANTS}
    for rep in range(3):
        for name, mon in VARIANTS:
            if not plain_only:
                s.monitor(*(mon or (0, 0)))
            s.sync()
            t0 = time.perf_counter()
            s.step(dt, steps)
            s.sync()
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
            if mon:
                rec = s.monitor_read()
                assert rec.shape[0] == steps // mon[0], rec.shape
    base = min(ms["unmonitored"])
    for name, mon in VARIANTS:
        v = ms[name]
        line = f"{name:16s} ms/step: " + " ".join(f"{t:.3f}" for t in v) + f"   (min {min(v):.3f})"
        if mon:
            per = (min(v) - base) * steps / (steps // mon[0])
            line += f"   per record over the unmonitored min: {per:.3f} ms"
        print(line)
    if not plain_only:
        s.monitor(1, 32)
        s.step(dt, 1)
        s.monitor_read()
        s.reset_timing()
        s.set_timing(True)
        s.step(dt, steps)
        t = s.timing()
        s.set_timing(False)
        rec = s.monitor_read()
        cm, cc = t["class_ms"], t["class_count"]
        print("timing classes over", steps, "monitored steps (ms total / launches / ms per launch):")
        for k in cm:
            if cc[k]:
                print(f"  {k:10s} {cm[k]:9.3f} / {cc[k]:5d} / {cm[k] / cc[k]:.4f}")
        obs, l2 = cm["pointwise"] / cc["pointwise"], cm["alpha"] / cc["alpha"]
        print(f"k_observe per launch (class 3 mean) {obs:.4f} ms; k_alpha_l2 per launch (class 0 mean) {l2:.4f} ms; "
              f"ratio {obs / l2:.3f} (expected <= 1.25)")
        print(f"bytes: {16 * n ** 3 / 1e9:.3f} GB per observation -> {16 * n ** 3 / obs / 1e9:.2f} TB/s algorithmic")
        # the large-slab reduction path (one tile per workgroup, parallel column sums) by value
        r, u = s.observe(), s.get_field()
        a2 = u.real * u.real + u.imag * u.imag
        em, e4 = abs(r["mass"] - a2.sum()) / a2.sum(), abs(r["p4"] - (a2 * a2).sum()) / (a2 * a2).sum()
        print(f"against numpy at this size: mass rel err {em:.1e}, p4 rel err {e4:.1e}, max_abs2 "
              f"{'equal' if r['max_abs2'] == a2.max() else 'DIFFERS'}, nonfinite {r['nonfinite']:.0f}")
        assert em <= 1e-13 and e4 <= 1e-13 and r["max_abs2"] == a2.max() and r["nonfinite"] == 0
        e = rec[:, nls_amd.OBS_FIELDS.index("energy")]
        print(f"last records: mass {rec[-1, 1]:.12e} energy {e[-1]:.12e} (drift over the run {abs(e[-1] - e[0]) / abs(e[0]):.2e})")

"""bench.py's own contract: the plain line, --full, --dump-outputs."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


class _FakeSolver:
    """What dump_outputs reads of a TinyBatchSolver, with instance b's values all equal to b."""

    def __init__(self, B, nx, nu, N):
        self.B, self.nx, self.nu, self.N = B, nx, nu, N

    def get_status(self):
        b = np.arange(self.B)
        return b.astype(np.int32), (b % 2).astype(np.int32), np.repeat(b[:, None], 4, 1).astype(np.float32)

    def get_x(self):
        return np.broadcast_to(np.arange(self.B, dtype=np.float32)[:, None, None], (self.B, self.N, self.nx)).copy()

    def get_u(self):
        return np.broadcast_to(np.arange(self.B, dtype=np.float32)[:, None, None], (self.B, self.N - 1, self.nu)).copy()


@pytest.mark.parametrize("B,nx,nu,N", [(200, 12, 4, 30), (65536, 12, 4, 30), (16384, 32, 16, 50)])
def test_dump_outputs_is_bounded_seeded_and_float(tmp_path, B, nx, nu, N):
    sys.path.insert(0, str(ROOT))
    import bench
    sol = _FakeSolver(B, nx, nu, N)
    bench.dump_outputs(str(tmp_path / "a"), sol)
    bench.dump_outputs(str(tmp_path / "b"), sol)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(f"{n}.npy" for n in ("x", "u", "iter", "status", "residuals", "sample_index"))
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64e6
    d = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for f in files:
        assert d[f[:-4]].dtype in (np.float32, np.float64)
        assert np.array_equal(d[f[:-4]], np.load(tmp_path / "b" / f))   # the same sample every time
    idx = d["sample_index"].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < B
    if B == 200:
        assert np.array_equal(idx, np.arange(B))   # small batches are written whole
    assert d["x"].shape == (len(idx), N, nx) and d["u"].shape == (len(idx), N - 1, nu)
    assert np.array_equal(d["x"][:, 0, 0], idx) and np.array_equal(d["u"][:, -1, -1], idx) and np.array_equal(d["iter"], idx)
    assert np.array_equal(d["status"], idx % 2) and np.array_equal(d["residuals"][:, 3], idx)


def _bench(*args):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", *args], capture_output=True, text=True, timeout=600,
                       env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_identical_outputs(tmp_path):
    """A plain run prints the headline only; two runs with the same arguments dump the same outputs bit for bit."""
    args = ["--steps", "4", "--warmup", "1", "--batch", "4096"]
    a = _bench(*args, "--dump-outputs", str(tmp_path / "a"))
    b = _bench(*args, "--dump-outputs", str(tmp_path / "b"))
    for d in (a, b):
        assert d["steps"] == 4 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert abs(d["value"] - 4096 * 4 / (d["ms_per_step"] * 1e-3 * 4)) / d["value"] < 1e-6
        assert not {"roofline", "cpu_baseline", "parity", "fixed10", "transfers", "fast_arithmetic", "closed_loop"} & set(d)
    for name in ("x", "u", "iter", "status", "residuals", "sample_index"):
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), name
    u, it, st = np.load(tmp_path / "a" / "u.npy"), np.load(tmp_path / "a" / "iter.npy"), np.load(tmp_path / "a" / "status.npy")
    assert u.shape == (4096, 29, 4) and np.all(np.isfinite(u)) and np.all(np.abs(u) <= 0.5)   # u within the input bounds
    assert it.mean() == pytest.approx(a["config"]["mean_iters"]) and np.mean(st == 1) == pytest.approx(a["config"]["frac_converged"])

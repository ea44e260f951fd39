"""GPU: bench.py on one GPU, as a plain run and with --full, on the smallest mesh (x1.642 x 26).

A plain run times its steps and prints the result line, nothing else: no roofline, CPU baseline or
configs1 line.  --dump-outputs writes the state its last timed step left, which is what the same
number of steps through the Python host gives, bit for bit (also from two ranks on the one GPU, whose
plain run leaves out the profile step and the verification).  --full adds what the plain run leaves
out (here without the CPU baseline and the x1.10242 line, which the options for them switch off)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--ncells", "642", "--levels", "26", "--steps", "2", "--warmup", "1"]
FIELDS = ("u", "theta_m", "rho_zz", "w", "scalars")


def _bench(cache, *extra):
    env = dict(os.environ, MPAS_DYCORE_CACHE=str(cache))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, *extra], capture_output=True,
                       text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(lines[0])


def _one_block(ncells, nsteps):
    """The state after nsteps of the whole mesh as one block through the Python host."""
    from mpas_dycore import Dycore
    from mpas_dycore.cases import jw_case
    case = jw_case(ncells, K=26, ns=1, order=3, cache=False)
    dt = case["dt"]
    dy = Dycore(case, device=0)
    dy.init_diagnostics(dt)
    dy.use_graph(True)
    for i in range(nsteps):
        dy.atm_timestep(dt, i + 1)
        dy.shift_time_levels()
    dy.synchronize()
    want = {n: np.asarray(dy.get("state", n, 1)) for n in FIELDS}
    dy.close()
    return want


def _check_dump(d, want):
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in FIELDS)
    for n in FIELDS:
        got = np.load(d / (n + ".npy"))
        assert got.dtype == np.float64 and np.all(np.isfinite(got))
        assert np.array_equal(got, want[n].reshape(want[n].shape[0], -1)), n


def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = _bench(tmp_path / "cache", "--dump-outputs", str(tmp_path / "dump"))
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1 and not out["full"]
    assert out["unit"] == "cell-updates/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(642 * 26 / (out["ms_per_step"] / 1e3), rel=1e-12)
    assert out["roofline"] is None and out["cpu_baseline"] is None and "configs1" not in out
    assert out["config"]["hip_graph"]
    _check_dump(tmp_path / "dump", _one_block(642, 3))  # the warm-up step and the two timed steps


def test_plain_two_rank_run_dumps_the_whole_mesh(tmp_path):
    """Two ranks on the one GPU (--same-device), plain: no profile step and no verification, and the
    dumped state is the whole mesh in global order -- the one block's after the same steps, bit for
    bit."""
    env = dict(os.environ, MPAS_DYCORE_CACHE=str(tmp_path / "cache"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29551", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--same-device",
           "--ncells", "2562", "--levels", "26", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(tmp_path / "dump")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["ms_per_step"] > 0 and not out["full"]
    assert out["preflight"]["ok"] and out["ranks"] is None and out["verify"] is None and out["roofline"] is None
    _check_dump(tmp_path / "dump", _one_block(2562, 3))


def test_full_run_adds_the_roofline(tmp_path):
    out = _bench(tmp_path / "cache", "--full", "--no-cpu-baseline", "--no-configs1", "--acoustic-reps", "3")
    assert out["full"] and out["steps"] == 2 and out["ms_per_step"] > 0
    roof = out["roofline"]
    assert roof["bound"] == "hbm" and roof["achieved"] > 0 and roof["frac"] == roof["achieved"] / roof["peak"]
    assert set(roof["ms_kernels"]) == {"edges", "cells", "final_divdamp_share"}

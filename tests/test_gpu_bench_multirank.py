"""GPU: bench.py's multi-rank path as the driver runs it (torch.distributed.run, one process per rank,
gloo rendezvous, host-side plan preflight, watchdog, max-over-ranks timing, per-rank exchange profile)
with two ranks on the one GPU of the box (--same-device: no RCCL, the one-sided transfer between the
two processes over IPC), with --full for the profile and the check.  Checks the JSON contract of
the line, not the speed, and the line's own verification: the ranks' owned state after the run equals the whole mesh stepped as one block on
rank 0's GPU, bit for bit -- and with one exchange point's pull switched off (--skip-pull) the check
fails, and the repeated run over the other transport passes."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(port, *extra):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--same-device", "--ncells",
           "10242", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-configs1",
           "--acoustic-reps", "3", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=400, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:] + r.stderr[-3000:]
    return r, json.loads(lines[0])


def test_bench_two_ranks_same_device():
    r, out = _bench(29543)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0
    assert out["preflight"]["ok"] and len(out["ranks"]) == 2
    assert "one-sided" in out["config"]["parallelism"] and out["config"]["hip_graph"]
    # 52 exchange points per dt less the u exchanges after stages 1 and 2 (6 per dt)
    assert all(rk["exchanges"] == 46 for rk in out["ranks"])
    v = out["verify"]
    assert v["bitwise_vs_one_block"] and v["transport"] == "one-sided" and v["steps"] == 5, v
    assert "first_attempt" not in v


def test_bench_verification_catches_a_skipped_exchange():
    """The tend_u exchange (642) pulls nothing: the halo edges keep the previous stage's tend_u, the
    owned state drifts from the one block's, the check says so, and the run is repeated with send /
    receive buffers (which the switch does not touch) and verified bit for bit."""
    r, out = _bench(29547, "--skip-pull", "tend.u.")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    v = out["verify"]
    first = v["first_attempt"]
    assert not first["bitwise_vs_one_block"] and first["transport"] == "one-sided", v
    assert sum(first["differing_columns"].values()) > 0 and first["max_rel_linf"]["u"] > 0, v
    assert v["rerun"] == "p2p buffers" and v["bitwise_vs_one_block"], v
    assert out["config"]["debug_skip_pull"] == "tend.u." and "buffers" in out["config"]["parallelism"]

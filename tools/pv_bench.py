#!/usr/bin/env python3
"""Time mpas_dyc_pv_diagnostics against the host path's downloads, on one GPU.

x1.163842 x 56 (bench.py's case) after a few captured steps: the call through mpas_dyc_set_profile /
mpas_dyc_get_profile out[9] (HIP events around the whole call, the fill's read-backs included), the sweeps
of its fill that changed something (out[10]), and in the same process the eight mpas_dyc_get_field downloads
a host that computes the diagnostics itself needs first (w, theta_m, rho_zz, scalars, uReconstructX/Y/Z,
vorticity).  From the columns the kernels read per cell-level it gives the time a pure stream of those bytes
would take at this code's measured 5.4 TB/s.  Prints one JSON line.

    python tools/pv_bench.py [--ncells 163842] [--levels 56] [--steps 3] [--reps 10]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpas-model_amd"))

HOST_FIELDS = (("state", "w"), ("state", "theta_m"), ("state", "rho_zz"), ("state", "scalars"), ("diag", "uReconstructX"),
               ("diag", "uReconstructY"), ("diag", "uReconstructZ"), ("diag", "vorticity"))
STREAM_TBPS = 5.4


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ncells", type=int, default=163842)
    ap.add_argument("--levels", type=int, default=56)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    from mpas_dycore import Dycore
    from mpas_dycore.cases import jw_case, jw_dt, level_for
    case = jw_case(args.ncells, K=args.levels, ns=1, order=3)
    n, K = case["nCells"], args.levels
    dt = jw_dt(level_for(args.ncells))
    dy = Dycore(case, device=0)
    dy.init_diagnostics(dt)
    dy.use_graph(True)
    for it in range(1, args.steps + 1):
        dy.atm_timestep(dt, it)
        dy.shift_time_levels()
    dy.set_pv(True)
    dy.pv_diagnostics(1)                      # the first call builds the per-cell table
    ms = sorted(dy.pv_ms(1) for _ in range(args.reps))
    sweeps = dy.pv_sweeps()
    ilev = dy.get_raw("diag", "iLev_DT")[:-1]
    epv = dy.get("diag", "ertel_pv")
    # per cell-level: theta_m, qv, rho_zz, zz read and theta, rho written; then about 6 neighbour columns each of
    # theta and w (two levels), 6 vertex columns of vorticity, the cell's own seven columns, ertel_pv written and
    # read again by the fill and the interpolation: about 28 column reads
    nbytes = 8 * n * K * (6 + 28)
    pulls = []
    for _ in range(3):
        dy.synchronize()
        t0 = time.perf_counter()
        got = 0
        for pool, name in HOST_FIELDS:
            got += dy.get_raw(pool, name).nbytes
        pulls.append(1e3 * (time.perf_counter() - t0))
    dy.close()
    med = ms[len(ms) // 2]
    print(json.dumps({"case": f"x1.{n}x{K}", "steps": args.steps, "ms_pv": [round(x, 4) for x in ms], "ms_pv_median": round(med, 4),
                      "fill_sweeps": sweeps, "kernel_bytes": nbytes,
                      "ms_stream_floor_at_5.4TBps": round(nbytes / STREAM_TBPS / 1e9, 3),
                      "ms_eight_get_field": [round(x, 2) for x in pulls], "ms_eight_get_field_min": round(min(pulls), 2),
                      "host_bytes": got, "call_over_downloads": round(med / min(pulls), 4),
                      "iLev_DT_min_max": [int(ilev.min()), int(ilev.max())],
                      "cells_with_tropopause_in_column": int(np.count_nonzero((ilev >= 2) & (ilev <= K))),
                      "ertel_pv_abs_max": float(np.max(np.abs(epv))), "finite": bool(np.all(np.isfinite(epv)))}))


if __name__ == "__main__":
    main()

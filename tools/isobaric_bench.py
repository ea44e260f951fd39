#!/usr/bin/env python3
"""Time mpas_dyc_isobaric_diagnostics against the host path's downloads, on one GPU.

x1.163842 x 56 (bench.py's case), all bits on: the call through mpas_dyc_set_profile / mpas_dyc_get_profile
out[8] (HIP events around its launches), and in the same process the ten mpas_dyc_get_field downloads the
host's interp_diagnostics needs (theta_m, scalars, w, exner, pressure_p, pressure_base, vorticity,
uReconstructZonal, uReconstructMeridional, zgrid).  From the bytes the two kernels must read and write it
gives the fraction of the 8 TB/s HBM roofline.  Prints one JSON line.

    python tools/isobaric_bench.py [--ncells 163842] [--levels 56] [--reps 10]
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

HOST_FIELDS = (("state", "theta_m"), ("state", "scalars"), ("state", "w"), ("diag", "exner"), ("diag", "pressure_p"),
               ("diag", "pressure_base"), ("diag", "vorticity"), ("diag", "uReconstructZonal"),
               ("diag", "uReconstructMeridional"), ("mesh", "zgrid"))
HBM_TBPS = 8.0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ncells", type=int, default=163842)
    ap.add_argument("--levels", type=int, default=56)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    from mpas_dycore import Dycore
    from mpas_dycore.cases import jw_case, jw_dt, level_for
    case = jw_case(args.ncells, K=args.levels, ns=1, order=3)
    n, nv, K = case["nCells"], case["nVertices"], args.levels
    dt = jw_dt(level_for(args.ncells))
    dy = Dycore(case, device=0)
    dy.init_diagnostics(dt)
    dy.atm_timestep(dt, 1)
    dy.shift_time_levels()
    dy.set_isobaric()
    dy.set("diag", "relhum", np.full((n, K), 55.0))
    ms = sorted(dy.isobaric_diagnostics_ms(1) for _ in range(args.reps))
    mslp = dy.get("diag", "mslp")[:, 0]
    # what the two kernels must move: the cell pass reads eight K-level fields and two (K + 1)-level ones per
    # cell and writes 42 + mslp + meanT + 5 + 13 values; the vertex pass reads pressure_p, pressure_base once
    # more and the vorticity, and writes 6 values per vertex
    nbytes = 8 * (n * (8 * K + 2 * (K + 1) + 62) + n * 2 * K + nv * (K + 6))
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
    print(json.dumps({"case": f"x1.{n}x{K}", "ms_isobaric": [round(x, 4) for x in ms], "ms_isobaric_median": round(med, 4),
                      "kernel_bytes": nbytes, "TBps": round(nbytes / med / 1e9, 3),
                      "fraction_of_8TBps": round(nbytes / med / 1e9 / HBM_TBPS, 3),
                      "ms_ten_get_field": [round(x, 2) for x in pulls], "ms_ten_get_field_min": round(min(pulls), 2),
                      "host_bytes": got, "mslp_min_max": [float(mslp.min()), float(mslp.max())],
                      "finite": bool(np.all(np.isfinite(mslp)))}))


if __name__ == "__main__":
    main()

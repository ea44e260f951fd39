#!/usr/bin/env python3
"""Time mpas_dyc_pv_budget_diagnostics against the host path, on one GPU.

    python tools/pvbudget_bench.py [--ncells 163842] [--levels 56] [--steps 3] [--reps 10]
    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python tools/pvbudget_bench.py --kernels-only 20

x1.163842 x 56 (bench.py's mesh) after a few captured steps with physics_get_tend on the device (bl_ysu +
cu_ntiedtke + lw + sw, smooth raw tendencies: cases.raw_physics_forcing at scale 0.02), all four sources on:
  * the call through mpas_dyc_set_profile / mpas_dyc_get_profile out[13] (HIP events around the whole call, the
    PV diagnostics and their fill's read-backs included), and in the same process mpas_dyc_pv_diagnostics alone
    (out[9]): the difference is the budget's share;
  * the host alternative: the mpas_dyc_get_field downloads of the 3-D fields a host that computes the budget
    itself needs first (the PV diagnostics' eight, the four raw theta tendencies, dtheta_dt_mp, tend_u_phys,
    tend.u_euler / w_euler / theta_euler, rho_edge), and the numpy restatement's time per column on a
    ``--host-ncells`` mesh of the same levels, scaled to the mesh's columns (numpy's vector loops, one thread: a
    floor for the reference's scalar loops, which repeat the geometry at every level);
  * the bytes k_pvb_budget and k_pv_epv move at least -- every column they read or write counted once -- for the
    kernel trace's times: the share of 8 TB/s each reaches.
Prints one JSON line.  --kernels-only N: one context, N calls and nothing else, for a kernel trace.
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

SET = dict(pbl="bl_ysu", convection="cu_ntiedtke", lw=True, sw=True)
RAW = ("rthratenlw", "rthratensw", "rthblten", "rthcuten")
HOST_FIELDS = (("state", "w"), ("state", "theta_m"), ("state", "rho_zz"), ("state", "scalars"), ("diag", "uReconstructX"),
               ("diag", "uReconstructY"), ("diag", "uReconstructZ"), ("diag", "vorticity")) + \
    tuple(("tend_physics", n) for n in RAW) + (("diag", "dtheta_dt_mp"), ("diag", "tend_u_phys"), ("tend", "u_euler"),
                                               ("tend", "w_euler"), ("tend", "theta_euler"), ("diag", "rho_edge"))
HBM_BPS = 8.0e12
# columns per cell, each counted once (an icosahedral mesh has 2 vertices per cell).  k_pvb_budget reads zgrid, w,
# theta, rho, vorticity (2), uReconstructX/Y/Z, the six sources, the uncoupled tend_w, the curl (2), tenduX/Y/Z and
# writes its eight outputs; k_pv_epv reads the first nine and writes ertel_pv
BUDGET_COLUMNS, EPV_COLUMNS = 21 + 8, 10 + 1


def img(a):
    out = np.zeros((a.shape[0] + 1,) + a.shape[1:], dtype=np.float64)
    out[:-1] = a
    return out


def context(ncells, levels, steps):
    from mpas_dycore import Dycore, todynamics as T
    from mpas_dycore.cases import jw_case, jw_dt, level_for, raw_physics_forcing
    case = T.with_vectors(jw_case(ncells, K=levels, ns=1, order=3))
    dt = jw_dt(level_for(ncells))
    dy = Dycore(case, device=0)
    dy.init_diagnostics(dt)
    dy.use_graph(True)
    dy.set_todynamics(**SET)
    for n, a in raw_physics_forcing(case, 0.02).items():
        if n != "rniblten":
            dy.set_raw("tend_physics", n, img(a))
    for it in range(1, steps + 1):
        dy.atm_timestep(dt, it)
        dy.shift_time_levels()
    dy.set_pv(True)
    dy.set_pv_budget()
    dy.pv_budget_diagnostics(1)               # the first call builds the per-cell table and the exchange-free plans
    return case, dy


def host_loop_ms_per_column(ncells, levels):
    """The restatement on a small mesh of the same levels, synthetic inputs: milliseconds per column."""
    from mpas_dycore import pvbudget as B, reconstruct
    from mpas_dycore.cases import jw_case
    case = jw_case(ncells, K=levels, ns=1, order=3, cache=False)
    m = dict(case)
    m.update(reconstruct.initialize_vectors(case))
    n, ne, nv, K = case["nCells"], case["nEdges"], case["nVertices"], levels
    rng = np.random.default_rng(1)
    f = {"qv": np.zeros((n, K)), "theta_m": np.asarray(case["theta"], dtype=np.float64),
         "rho_zz": np.asarray(case["rho"]) / np.asarray(case["zz"]), "w": rng.random((n, K + 1)) - 0.5,
         "vorticity": 1e-5 * (rng.random((nv, K)) - 0.5), "tend_w_euler": rng.random((n, K + 1)) - 0.5,
         "tend_u_euler": rng.random((ne, K)) - 0.5, "tend_u_phys": rng.random((ne, K)) - 0.5,
         "rho_edge": 0.5 + rng.random((ne, K))}
    for name in ("uReconstructX", "uReconstructY", "uReconstructZ", "uReconstructZonal", "uReconstructMeridional",
                 "tend_theta_euler", "dtheta_dt_mp") + RAW:
        f[name] = rng.random((n, K)) - 0.5
    B.driver(m, f, B.ALL)
    t0 = time.perf_counter()
    B.driver(m, f, B.ALL)
    return 1e3 * (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ncells", type=int, default=163842)
    ap.add_argument("--levels", type=int, default=56)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-ncells", type=int, default=2562)
    ap.add_argument("--kernels-only", type=int, default=0)
    args = ap.parse_args()
    case, dy = context(args.ncells, args.levels, args.steps)
    n, K = case["nCells"], args.levels
    bytes_budget, bytes_epv = 8 * n * K * BUDGET_COLUMNS, 8 * n * K * EPV_COLUMNS
    floors = {"k_pvb_budget_bytes": bytes_budget, "k_pv_epv_bytes": bytes_epv,
              "ms_at_8TBps": {"k_pvb_budget": round(bytes_budget / HBM_BPS * 1e3, 4),
                              "k_pv_epv": round(bytes_epv / HBM_BPS * 1e3, 4)}}
    if args.kernels_only:
        for _ in range(args.kernels_only):
            dy.pv_budget_diagnostics(1)
        dy.synchronize()
        dy.close()
        print(json.dumps({"case": f"x1.{n}x{K}", "calls": args.kernels_only + 1, **floors}))
        return
    ms = sorted(dy.pv_budget_ms(1) for _ in range(args.reps))
    ms_pv = sorted(dy.pv_ms(1) for _ in range(args.reps))
    fric = dy.get("diag", "depv_dt_fric")
    diab = dy.get("diag", "depv_dt_diab")
    pulls = []
    for _ in range(3):
        dy.synchronize()
        t0 = time.perf_counter()
        got = 0
        for pool, name in HOST_FIELDS:
            got += dy.get_raw(pool, name).nbytes
        pulls.append(1e3 * (time.perf_counter() - t0))
    dy.close()
    per_column = host_loop_ms_per_column(args.host_ncells, K)
    med, med_pv = ms[len(ms) // 2], ms_pv[len(ms_pv) // 2]
    host_ms = min(pulls) + per_column * n
    print(json.dumps({"case": f"x1.{n}x{K}", "steps": args.steps, "ms_call": [round(x, 4) for x in ms],
                      "ms_call_median": round(med, 4), "ms_pv_diagnostics_median": round(med_pv, 4),
                      "ms_budget_share": round(med - med_pv, 4), **floors,
                      "ms_host_downloads": [round(x, 2) for x in pulls], "ms_host_downloads_min": round(min(pulls), 2),
                      "host_bytes": got, "host_loop_ms_per_column": round(per_column, 5),
                      "host_loop_mesh": args.host_ncells, "ms_host_loop_scaled": round(per_column * n, 1),
                      "ms_host_total": round(host_ms, 1), "host_over_call": round(host_ms / med, 1),
                      "depv_dt_diab_abs_max": float(np.max(np.abs(diab))), "depv_dt_fric_abs_max": float(np.max(np.abs(fric))),
                      "finite": bool(np.all(np.isfinite(diab)) and np.all(np.isfinite(fric)))}))


if __name__ == "__main__":
    main()

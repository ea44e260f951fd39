#!/usr/bin/env python3
"""What the convective running maxima cost on the device, against what the host path would cost.

    python tools/diag_update_bench.py [--ncells 163842] [--levels 56] [--steps 10]

Runs ``--steps`` captured steps of the dry JW case.  After the shift of every step from the third on
it times
  * mpas_dyc_diag_update with all three maxima on: HIP events around its launch on the compute
    stream (mpas_dyc_set_profile, mpas_dyc_get_profile out[6]);
  * the four downloads the host's convective_diagnostics_update would need that step -- state.w,
    diag.vorticity, diag.uReconstructZonal, diag.uReconstructMeridional -- with get_field into
    numpy buffers (wall clock around the four synchronous calls).
Prints one JSON line: the per-step numbers, their medians, the ratio, the bytes the update reads
and its fraction of an 8 TB/s HBM.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpas-model_amd"))

INPUTS = (("state", "w"), ("diag", "vorticity"), ("diag", "uReconstructZonal"), ("diag", "uReconstructMeridional"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncells", type=int, default=163842)
    ap.add_argument("--levels", type=int, default=56)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    import numpy as np
    from mpas_dycore import Dycore
    from mpas_dycore.cases import jw_case
    case = jw_case(a.ncells, K=a.levels, ns=1, order=3)
    dt = case["dt"]
    dy = Dycore(case, device=0)
    dy.init_diagnostics(dt)
    dy.use_graph(True)
    dy.set_diag_update()
    out = (C.c_double * 7)()
    ms_update, ms_download, ms_step = [], [], []
    for it in range(1, a.steps + 1):
        dy.synchronize()
        t0 = time.perf_counter()
        dy.atm_timestep(dt, it)
        dy.shift_time_levels()
        dy.synchronize()
        ms_step.append((time.perf_counter() - t0) * 1e3)
        if it < 3:
            dy.diag_update()
            continue
        dy._check(dy.lib.mpas_dyc_set_profile(dy.h, 1), "set_profile")
        dy.diag_update()
        dy._check(dy.lib.mpas_dyc_set_profile(dy.h, 0), "set_profile")
        dy._check(dy.lib.mpas_dyc_get_profile(dy.h, out, 7), "get_profile")
        ms_update.append(out[6])
        t0 = time.perf_counter()
        nbytes = 0
        for pool, name in INPUTS:
            nbytes += dy.get_raw(pool, name).nbytes
        ms_download.append((time.perf_counter() - t0) * 1e3)
    uh = dy.get_raw("diag", "updraft_helicity_max")[:-1]
    wm = dy.get_raw("diag", "w_velocity_max")[:-1]
    dy.close()
    # what one update reads: w and zgrid (K + 1), the level-1 winds, and the vorticity columns of the
    # in-band levels (6 or 7 vertices per cell) -- counted as whole K-columns of w and zgrid only
    z = case["zgrid"] - case["zgrid"][:, :1]
    band = np.sum((np.minimum(z[:, 1:], 5000.0) - np.maximum(z[:, :-1], 2000.0)) > 0)
    read = 8 * (2 * case["nCells"] * (a.levels + 1) + int(band) * 6)
    med_u, med_d = statistics.median(ms_update), statistics.median(ms_download)
    print(json.dumps({
        "case": f"x1.{a.ncells}x{a.levels}", "steps_timed": len(ms_update),
        "ms_diag_update": [round(x, 4) for x in ms_update], "ms_diag_update_median": round(med_u, 4),
        "ms_four_downloads": [round(x, 2) for x in ms_download], "ms_four_downloads_median": round(med_d, 2),
        "download_bytes": nbytes, "download_over_update": round(med_d / med_u, 1),
        "ms_step_median": round(statistics.median(ms_step[2:]), 2),
        "update_bytes_read_estimate": read, "fraction_of_8TBps": round(read / (med_u * 1e-3) / 8e12, 3),
        "in_band_levels_per_cell": round(float(band) / case["nCells"], 2),
        "updraft_helicity_max_nonzero_cells": int(np.count_nonzero(uh)), "w_velocity_max_max": float(wm.max()),
    }))


if __name__ == "__main__":
    main()

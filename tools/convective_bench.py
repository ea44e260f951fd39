#!/usr/bin/env python3
"""Time mpas_dyc_convective_diagnostics against the host path's downloads, on one GPU.

x1.163842 x 56 (bench.py's mesh) holding mpas_dycore.convcompute.synthetic_fields (unstable soundings, one per
cell of an x1.642 draw, broadcast over the mesh): the call through mpas_dyc_set_profile / mpas_dyc_get_profile
out[11] (HIP events around the call) for the mask CAPE | CIN and for all bits, and in the same process the
seven mpas_dyc_get_field downloads a host that computes the diagnostics itself needs first (theta_m, scalars,
exner, pressure_p, pressure_base, uReconstructZonal, uReconstructMeridional).  The sub-steps and iterations per
column come from the host restatement of the distinct soundings.  Prints one JSON line.

    python tools/convective_bench.py [--ncells 163842] [--levels 56] [--reps 5] [--host-s-per-column 3.8e-4]
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

HOST_FIELDS = (("state", "theta_m"), ("state", "scalars"), ("diag", "exner"), ("diag", "pressure_p"), ("diag", "pressure_base"),
               ("diag", "uReconstructZonal"), ("diag", "uReconstructMeridional"))
NDRAW = 642


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ncells", type=int, default=163842)
    ap.add_argument("--levels", type=int, default=56)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-s-per-column", type=float, default=0.0,
                    help="tools/make_convective_golden.py --time, to scale to the mesh (0: leave out)")
    args = ap.parse_args()
    from mpas_dycore import Dycore, _lib, convcompute as cc
    from mpas_dycore.cases import jw_case
    case = jw_case(args.ncells, K=args.levels, ns=1, order=3)
    n, K = case["nCells"], args.levels
    # NDRAW distinct soundings on the first cells' interfaces, repeated over the mesh (a permutation, so that
    # neighbouring lanes do not hold the same column)
    zg = np.asarray(case["zgrid"], dtype=np.float64)
    draw = cc.synthetic_fields({"zgrid": zg[:NDRAW]}, K)
    host = cc.compute(draw)
    pick = np.random.default_rng(5).integers(0, NDRAW, size=n)
    dy = Dycore(case, device=0)
    img = lambda a: np.concatenate([a, np.zeros((1,) + a.shape[1:])])  # noqa: E731
    dy.set("mesh", "zgrid", draw["zgrid"][pick])
    dy.set_raw("state", "scalars", img(draw["qv"][pick][:, :, None]), 1)
    dy.set_raw("state", "theta_m", img(draw["theta_m"][pick]), 1)
    for name, fld in (("exner", "exner"), ("pressure_p", "pressure_p"), ("pressure_base", "pressure_base"),
                      ("uReconstructZonal", "uzonal"), ("uReconstructMeridional", "umeridional")):
        dy.set_raw("diag", name, img(draw[fld][pick]))
    out = {"case": f"x1.{n}x{K}", "distinct_soundings": NDRAW}
    for label, mask in (("cape_cin", _lib.CONV_CAPE | _lib.CONV_CIN), ("all", _lib.CONV_ALL)):
        dy.set_convective(mask)
        dy.convective_diagnostics(1)
        ms = sorted(dy.convective_diagnostics_ms(1) for _ in range(args.reps))
        out[f"ms_{label}"] = [round(x, 3) for x in ms]
        out[f"ms_{label}_median"] = round(ms[len(ms) // 2], 3)
    cape = dy.get_raw("diag", "cape")[:-1]
    want = host["cape"][pick]
    pulls = []
    for _ in range(3):
        dy.synchronize()
        t0 = time.perf_counter()
        got = 0
        for pool, name in HOST_FIELDS:
            got += dy.get_raw(pool, name).nbytes
        pulls.append(1e3 * (time.perf_counter() - t0))
    dy.close()
    info = host["info"]
    its = info["iters"].sum(axis=1)
    out.update({"ms_seven_get_field": [round(x, 2) for x in pulls], "ms_seven_get_field_min": round(min(pulls), 2),
                "host_bytes": got, "substeps_max": int(info["nsub"].max()), "substeps_mean": round(float(info["nsub"].mean()), 1),
                "iterations_max": int(its.max()), "iterations_mean": round(float(its.mean()), 1),
                "cape_max": float(cape.max()), "cape_rel_linf_vs_restatement": float(np.max(np.abs(cape - want)) / np.max(np.abs(want))),
                "finite": bool(np.all(np.isfinite(cape)))})
    if args.host_s_per_column > 0.0:
        out["host_seconds_one_core_scaled"] = round(args.host_s_per_column * n, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

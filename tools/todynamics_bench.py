#!/usr/bin/env python3
"""What coupling the physics tendencies costs per step: on the device (mpas_dyc_set_todynamics) and the host's way.

    python tools/todynamics_bench.py [--ncells 163842] [--levels 56] [--ns 6] [--steps 10]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/todynamics_bench.py --kernels-only 20

Moist JW, scheme set bl_mynn + cu_ntiedtke + lw + sw without ni (num_scalars = 6: qv qc qr qi qs qg), smooth raw
tendencies (cases.raw_physics_forcing at scale 0.02, so ten steps stay in the model's range).  Four contexts one
after the other, each ``--steps`` steps with graph replay, timed from the third on (wall clock around what the
host does for the step + step + shift + synchronize):
  (a) no physics;
  (b) the host couples: before every step it downloads rho_zz, rho_edge, theta_m and scalars and uploads
      tend_ru_physics, tend_rtheta_physics, tend_rho_physics and scalars_tend (arrays formed once, outside
      the timing: only the transfers and the library's own layout conversion of the scalars count);
  (c) the hook, the raw tendencies resident;
  (d) the hook, the PBL's six raw fields uploaded before every step.
In (c), after every timed step, one mpas_dyc_physics_get_tend between HIP events times the two kernels alone.
Prints one JSON line with the per-step numbers, their medians, the orderings (c) - (a) and (c) < (b), and the
bytes the kernels move at least: the edge kernel 4 cell fields read once + rho_edge read + 4 edge fields written,
the cell kernel 13 streams read + 2 + the touched planes written + the untouched planes zeroed.
--kernels-only N: one context, N mpas_dyc_physics_get_tend calls and nothing else, for a kernel trace.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpas-model_amd"))

SET = dict(pbl="bl_mynn", convection="cu_ntiedtke", lw=True, sw=True)
IDX = dict(index_qc=2, index_qr=3, index_qi=4, index_qs=5, index_ni=0)
PBL_RAW = ("rublten", "rvblten", "rthblten", "rqvblten", "rqcblten", "rqiblten")
COUPLED = (("tend_physics", "tend_ru_physics"), ("tend_physics", "tend_rtheta_physics"),
           ("tend_physics", "tend_rho_physics"), ("tend", "scalars_tend"))
STATE_BACK = (("state", "rho_zz"), ("diag", "rho_edge"), ("state", "theta_m"), ("state", "scalars"))
HBM_BPS = 8.0e12


def img(a):
    import numpy as np
    out = np.zeros((a.shape[0] + 1,) + a.shape[1:], dtype=np.float64)
    out[:-1] = a
    return out


def context(case, raw, ns, mode):
    from mpas_dycore import Dycore
    dy = Dycore(case, device=0, moist_end=ns)
    dy.init_diagnostics(case["dt"])
    dy.use_graph(True)
    if mode in ("c", "d"):
        dy.set_todynamics(**SET, **IDX)
        for n, a in raw.items():
            dy.set_raw("tend_physics", n, img(a))
    elif mode == "b":
        dy.set_physics(tendencies=True)
    return dy


def run(case, raw, ns, steps, mode, coupled=None):
    import numpy as np
    dy = context(case, raw, ns, mode)
    dt = case["dt"]
    pbl = {n: img(raw[n]) for n in PBL_RAW}
    ms_step, ms_kernels = [], []
    for it in range(1, steps + 1):
        dy.synchronize()
        t0 = time.perf_counter()
        if mode == "b":
            for p, n in STATE_BACK:
                dy.get_raw(p, n, 1)
            for p, n in COUPLED:
                dy.set_raw(p, n, coupled[n])
        elif mode == "d":
            for n, a in pbl.items():
                dy.set_raw("tend_physics", n, a)
        dy.atm_timestep(dt, it)
        dy.shift_time_levels()
        dy.synchronize()
        if it >= 3:
            ms_step.append((time.perf_counter() - t0) * 1e3)
            if mode == "c":
                ms_kernels.append(dy.physics_get_tend_ms())
    out = {"finite": bool(np.isfinite(dy.get("state", "theta_m", 1)).all()), "captures": dy.graph_captures()}
    if mode == "c":
        out["coupled"] = {n: dy.get_raw(p, n) for p, n in COUPLED}
    dy.close()
    return ms_step, ms_kernels, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncells", type=int, default=163842)
    ap.add_argument("--levels", type=int, default=56)
    ap.add_argument("--ns", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernels-only", type=int, default=0)
    a = ap.parse_args()
    from mpas_dycore.cases import jw_case, raw_physics_forcing
    from mpas_dycore import todynamics as T
    case = T.with_vectors(jw_case(a.ncells, K=a.levels, ns=a.ns, moist=True, order=3))
    raw = {n: v for n, v in raw_physics_forcing(case, 0.02).items() if n != "rniblten"}
    nC, nE, K = case["nCells"], case["nEdges"], a.levels
    edge_bytes = 8 * K * (4 * (nC + 1) + 5 * (nE + 1))
    cell_bytes = 8 * K * (nC + 1) * (13 + 2 + a.ns)
    if a.kernels_only:
        dy = context(case, raw, a.ns, "c")
        for _ in range(a.kernels_only):
            dy.physics_get_tend()
        dy.synchronize()
        dy.close()
        print(json.dumps({"case": f"x1.{a.ncells}x{K} ns={a.ns}", "calls": a.kernels_only, "k_todyn_edges_bytes": edge_bytes,
                          "k_todyn_cells_bytes": cell_bytes, "ms_at_8TBps": {
                              "k_todyn_edges": round(edge_bytes / HBM_BPS * 1e3, 4),
                              "k_todyn_cells": round(cell_bytes / HBM_BPS * 1e3, 4)}}))
        return
    res = {}
    ms_c, ms_k, out_c = run(case, raw, a.ns, a.steps, "c")
    res["c"] = (ms_c, out_c)
    res["a"] = run(case, raw, a.ns, a.steps, "a")[::2]
    res["b"] = run(case, raw, a.ns, a.steps, "b", out_c["coupled"])[::2]
    res["d"] = run(case, raw, a.ns, a.steps, "d")[::2]
    med = {m: statistics.median(v[0]) for m, v in res.items()}
    med_k = statistics.median(ms_k)
    flags = T.scheme_flags(**SET)
    print(json.dumps({
        "case": f"x1.{a.ncells}x{K} moist ns={a.ns}", "flags": flags, "dt": case["dt"], "steps_timed": len(ms_c),
        **{f"ms_step_{m}": [round(x, 2) for x in res[m][0]] for m in "abcd"},
        **{f"ms_step_{m}_median": round(med[m], 3) for m in "abcd"},
        "finite": {m: res[m][1]["finite"] for m in "abcd"}, "captures": {m: res[m][1]["captures"] for m in "abcd"},
        "c_minus_a_ms": round(med["c"] - med["a"], 3), "c_less_than_b": bool(med["c"] < med["b"]),
        "ms_kernels": [round(x, 4) for x in ms_k], "ms_kernels_median": round(med_k, 4),
        "kernel_bytes": {"k_todyn_edges": edge_bytes, "k_todyn_cells": cell_bytes},
        "kernels_TBps": round((edge_bytes + cell_bytes) / (med_k * 1e-3) / 1e12, 3),
        "kernels_share_of_8TBps": round((edge_bytes + cell_bytes) / HBM_BPS / (med_k * 1e-3), 3),
        "upload_bytes_b": sum(len(out_c["coupled"][n]) * 8 for _, n in COUPLED),
        "upload_bytes_d": len(PBL_RAW) * 8 * K * (nC + 1),
    }))


if __name__ == "__main__":
    main()

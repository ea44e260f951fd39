#!/usr/bin/env python3
"""Per-kernel micro-benchmark of the acoustic sub-step (and optionally one dt) for
the library named by $MPAS_DYCORE_LIB (default: the in-tree build).

    MPAS_DYCORE_LIB=exp/lib_x.so python tools/kbench.py [--ncells 163842] [--steps 2]

--iau WINDOW_S: after the plain timing, the incremental analysis update is switched on with
synthetic increments and the step timed inside the window (k_iau_edges / k_iau_cells run) and after it
(they do not); ms_dt_iau_in / ms_dt_iau_after, next to ms_dt (IAU off) and ms_dt_physics (IAU off, physics coupling on with zero tendencies: the
step that IAU implies).  iau_bytes = the two kernels'
algorithmic bytes per call, for their fraction of the HBM peak under a kernel trace.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpas-model_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncells", type=int, default=163842)
    ap.add_argument("--levels", type=int, default=56)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--moist", action="store_true", help="BASELINE configs[3]: ns=6 moist species")
    ap.add_argument("--iau", type=float, default=0.0, metavar="WINDOW_S",
                    help="also time the step with the incremental analysis update on (window in seconds)")
    a = ap.parse_args()
    from mpas_dycore import Dycore
    from mpas_dycore.cases import jw_case
    ns = 6 if a.moist else 1
    case = jw_case(a.ncells, K=a.levels, ns=ns, moist=a.moist)
    dt = case["dt"]
    dy = Dycore(case, device=0, moist_end=ns)
    dy.init_diagnostics(dt)
    dy.use_graph(not a.no_graph)
    for i in range(2):
        dy.atm_timestep(dt, i + 1)
        dy.shift_time_levels()
    dy.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        dy.atm_timestep(dt, i + 3)
        dy.shift_time_levels()
    dy.synchronize()
    ms_dt = (time.perf_counter() - t0) / a.steps * 1e3
    # the prognostic state after the timed steps: equal digests = the two libraries' steps agree bit for bit
    import hashlib
    hsh = hashlib.sha256()
    for name in ("u", "w", "theta_m", "rho_zz", "scalars"):
        hsh.update(dy.get("state", name).tobytes())
    digest = hsh.hexdigest()[:16]
    dts = dt / case["config"]["config_dynamics_split_steps"] / case["config"]["config_number_of_sub_steps"]
    ms, ks = dy.time_acoustic_step(dts, 2, a.reps)
    b = dy.acoustic_bytes()
    out = {}
    if a.iau > 0.0:
        import numpy as np
        # synthetic increments, small enough that the forced steps stay in the model's range
        nC, nE, K = case["nCells"], case["nEdges"], a.levels
        kk = ((np.arange(K) + 0.5) / K)[None, :]
        lc, le = case["lonCell"][:, None], case["lonEdge"][:, None]
        dy.set("tend_iau", "u", 1e-2 * np.sin(2 * le) * np.cos(np.pi * kk))
        dy.set("tend_iau", "theta", 1e-2 * np.cos(3 * lc) * (1 - kk))
        dy.set("tend_iau", "rho", 1e-5 * np.sin(lc) * (1 - kk) ** 2)
        dy.set("tend_iau", "scalars", np.repeat((1e-7 * np.cos(lc) * (1 - kk) ** 3)[:, :, None], ns, axis=2))
        n_in = int(np.floor(a.iau / dt + 0.5))  # nint: the last forced step
        # ms_dt_physics: IAU off, physics coupling on with zero tendencies -- the step IAU implies, and
        # what the steps after the window are to be compared with
        for key, it in (("ms_dt_physics", 1), ("ms_dt_iau_in", 1), ("ms_dt_iau_after", n_in + 1)):
            if key == "ms_dt_physics":
                dy.set_physics(tendencies=True)
            elif key == "ms_dt_iau_in":
                dy.set_physics(tendencies=False)
                dy.set_iau(True, a.iau)
            assert (dy.iau_weight(dt, it) > 0.0) == (key == "ms_dt_iau_in"), (key, it, dt, a.iau)
            for i in range(2):  # the captured step of either time-level parity
                dy.atm_timestep(dt, it)
                dy.shift_time_levels()
            dy.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                dy.atm_timestep(dt, it)
                dy.shift_time_levels()
            dy.synchronize()
            out[key] = (time.perf_counter() - t0) / a.steps * 1e3
        # algorithmic bytes per call: the edge kernel reads rho_edge, u_amb and writes the sum over the
        # owned edges (no host physics here); the cell kernel reads zz, rho_zz, theta_m, rho_amb,
        # theta_amb, 2 arrays per moist scalar (scalars, scalars_amb; scalars_tend counts as 0.0
        # without host physics) and writes rtheta, rho and one scalars_tend plane per scalar
        out["iau_bytes"] = dict(k_iau_edges=8.0 * 3 * nE * K, k_iau_cells=8.0 * (5 + 2 * ns + 2 + ns) * nC * K)
    print(json.dumps(dict(**out, lib=os.environ.get("MPAS_DYCORE_LIB", "in-tree"), state=digest, ms_dt=ms_dt, ms_sub=sum(ks),
                          edges=ks[0], cells=ks[1], divdamp=ks[2], frac=b / (sum(ks) / 1e3) / 8e12)))


if __name__ == "__main__":
    main()

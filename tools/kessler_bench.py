#!/usr/bin/env python3
"""What the Kessler microphysics costs on the device: the kernel alone, and the step with it off and on.

    python tools/kessler_bench.py [--ncells 163842] [--levels 56] [--ns 6] [--steps 4]

Moist JW with cloud and rain seeded in the lower troposphere of every fourth cell, so that the
sedimentation's split loop runs (nfall > 1) on a quarter of the columns.  Two contexts, one after the
other, each ``--steps`` captured steps timed from the third on (wall clock around step + shift +
synchronize): the scheme off, then on.  Four steps by default: the JW state's top levels (p < 250 Pa at
about 262 K) have es > p, where the scheme's qvs is negative and it condenses cloud out of nothing, 25 K of
heating per call at the top level (the reference's scheme does the same: mpas_dycore.kessler, which
equals it bit for bit, shows it on the initial state); a JW run with Kessler leaves the model's range
at its fifth step, so the timed steps are the third and fourth, and ``state_finite`` says whether they
were taken on a finite state.  In the second context, after every timed step, one
mpas_dyc_microphysics on time level 1 between HIP events (mpas_dyc_set_profile, mpas_dyc_get_profile
out[7]) times the kernel alone on the state the step left.
Prints one JSON line: the per-step numbers and medians, the kernel against its streaming floor -- 19
fp64 streams per owned cell-level (11 read: theta_m, qv, qc, qr, rho_zz, zz, exner, zgrid, rtheta_base,
exner_base and theta_m again; 8 written: theta_m, qv, qc, qr, rt_diabatic_tend, rtheta_p, exner,
pressure_p) at the 5.4 TB/s this code's streaming kernels reach -- and the transcendentals it evaluates
(7 pow, 1 exp, 1 sqrt per cell-level plus one pow per level and further split step).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpas-model_amd"))

STREAMS = 19
FLOOR_BPS = 5.4e12


def seeded(case, ns):
    import numpy as np
    n, K = case["nCells"], case["nVertLevels"]
    sc = np.array(case["scalars"], dtype=np.float64).reshape(n, K, ns)
    kk = np.arange(K)[None, :]
    patch = (np.arange(n) % 4 == 0)[:, None]
    sc[:, :, 1] = np.where(patch & (kk >= K // 10) & (kk < K // 3), 1.0e-3, 0.0)
    sc[:, :, 2] = np.where(patch & (kk >= K // 20) & (kk < K // 4), 2.0e-3 * (1.0 + np.sin(np.arange(n)))[:, None], 0.0)
    out = dict(case)
    out["scalars"] = sc.reshape(np.asarray(case["scalars"]).shape)
    return out


def run(case, dt, ns, steps, on):
    from mpas_dycore import Dycore
    dy = Dycore(case, device=0, moist_end=ns)
    dy.init_diagnostics(dt)
    dy.use_graph(True)
    if on:
        dy.set_microphysics("kessler", 2, 3)
    ms_step, ms_kernel = [], []
    for it in range(1, steps + 1):
        dy.synchronize()
        t0 = time.perf_counter()
        dy.atm_timestep(dt, it)
        dy.shift_time_levels()
        dy.synchronize()
        if it >= 3:
            ms_step.append((time.perf_counter() - t0) * 1e3)
            if on:
                ms_kernel.append(dy.microphysics_ms(dt, 1))
    extra = {}
    if on:
        rain = dy.get("diag_physics", "rainnc")
        import numpy as np
        extra = {"rainnc_max_mm": float(rain.max()), "cells_with_rain": int((rain > 0).sum()),
                 "state_finite": bool(np.isfinite(dy.get("state", "theta_m", 1)).all())}
    dy.close()
    return ms_step, ms_kernel, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncells", type=int, default=163842)
    ap.add_argument("--levels", type=int, default=56)
    ap.add_argument("--ns", type=int, default=6)
    ap.add_argument("--steps", type=int, default=4)
    a = ap.parse_args()
    from mpas_dycore.cases import jw_case
    case = seeded(jw_case(a.ncells, K=a.levels, ns=a.ns, moist=True, order=3), a.ns)
    dt = case["dt"]
    off, _, _ = run(case, dt, a.ns, a.steps, False)
    on, kern, extra = run(case, dt, a.ns, a.steps, True)
    cell_levels = case["nCells"] * a.levels
    floor_ms = STREAMS * 8 * cell_levels / FLOOR_BPS * 1e3
    med_k, med_on, med_off = statistics.median(kern), statistics.median(on), statistics.median(off)
    print(json.dumps({
        "case": f"x1.{a.ncells}x{a.levels} moist ns={a.ns}", "dt": dt, "steps_timed": len(on),
        "ms_kernel": [round(x, 4) for x in kern], "ms_kernel_median": round(med_k, 4),
        "ms_streaming_floor": round(floor_ms, 4), "kernel_over_floor": round(med_k / floor_ms, 2),
        "kernel_bytes": STREAMS * 8 * cell_levels, "kernel_TBps_if_streams_only": round(
            STREAMS * 8 * cell_levels / (med_k * 1e-3) / 1e12, 3),
        "ns_per_cell_level": round(med_k * 1e6 / cell_levels, 4),
        "ms_step_off": [round(x, 2) for x in off], "ms_step_off_median": round(med_off, 3),
        "ms_step_on": [round(x, 2) for x in on], "ms_step_on_median": round(med_on, 3),
        "step_on_minus_off_ms": round(med_on - med_off, 3), **extra,
    }))


if __name__ == "__main__":
    main()

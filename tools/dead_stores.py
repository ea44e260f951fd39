#!/usr/bin/env python3
"""Dead-store candidates of the step: walk the kernel sequence of two dt from a rocprofv3 kernel
trace of bench.py (tools/gpu.sh prof) and flag every array a kernel writes that the next write
overwrites before any kernel reads it.  Reads and writes per kernel come from tools/kernel_access.py
(text scan of the kernels' Ptrs accesses) with the template-variant rules of kernel_roofline.py.

It is a candidate list, not a proof: the scan does not see element ranges (a kernel over the halo
cells only overwrites nothing of the owned ones), most runtime store flags, or the pool the host
reads after the step.  Each candidate was checked by hand.

The stores that a launch skips by its place in the dt, which its name does not show, are modelled
(stage_drops): the recoveries of stages 1 and 2 store no ruAvg / wwAvg (SA_SKIP; --all-stage-stores
for a trace taken with MPAS_DYCORE_SKIP_STAGE_AVG=0), and with the deriving cell phases in the trace
only the dt's last k_vert_imp_coefs_p stores cofwr, a_tri and gamma_tri (store_drv); the diagnostics'
cell kernel stores divergence and vorticity only after stage 3 (store_dv).

    python tools/dead_stores.py gpurun_out/prof/run_kernel_trace.csv
"""
import csv
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import kernel_roofline as kr  # noqa: E402
from kernel_access import access_map  # noqa: E402


FIN_CELLS = re.compile(r"k_acoustic_cells_r<\d, true|k_dyn_cells3_acoustic_r<\d, (true|false), true")
DIAG_CELLS = re.compile(r"k_recover3_diag_cells_b<|k_diag_cells_b<|k_diag_cells_vtx_b<")
DRV_CELLS = re.compile(r"k_acoustic_cells_r<\d, (true|false), [1-7]>|k_dyn_cells3_acoustic_r<\d, (true|false), (true|false), [1-7]>")


def stage_drops(seq, ndt, skip_stage_avg=True):
    """Per launch of seq (ndt whole dt): the Ptrs members it does not store because of where it
    stands in the dt.  Every third recovering damping / cell phase is a stage 3, which stores ruAvg /
    wwAvg; the others do not.  With deriving cell phases, every k_vert_imp_coefs_p but the last of a
    dt leaves cofwr, a_tri and gamma_tri to them."""
    drops = [set() for _ in seq]
    if skip_stage_avg:
        for pick, member in ((lambda k: k.startswith("k_divdamp_p<true"), "ruAvg"),
                             (lambda k: FIN_CELLS.match(k) is not None, "wwAvg")):
            for j, i in enumerate([i for i, k in enumerate(seq) if pick(k)]):
                if j % 3 != 2:
                    drops[i].add(member)
    # the diagnostics' cell kernel stores divergence (and, where it forms the vertices, vorticity) only
    # after stage 3 (store_dv): every third launch
    for j, i in enumerate([i for i, k in enumerate(seq) if DIAG_CELLS.match(k)]):
        if j % 3 != 2:
            drops[i] |= {"divergence", "vorticity"}
    if any(DRV_CELLS.match(k) for k in seq):
        vic = [i for i, k in enumerate(seq) if k.startswith("k_vert_imp_coefs_p")]
        per = len(vic) // ndt
        for j, i in enumerate(vic):
            if per and j % per != per - 1:
                drops[i] |= {"cofwr", "a_tri", "gamma_tri"}
    return drops


def main():
    skip_stage_avg = "--all-stage-stores" not in sys.argv
    sys.argv = [a for a in sys.argv if a != "--all-stage-stores"]
    amap = access_map()
    reg = kr.registry(163842, 56)
    rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
    ends = [i for i, r in enumerate(rows) if "k_summary_final" in r["Kernel_Name"] and
            (i + 1 == len(rows) or "k_summary" not in rows[i + 1]["Kernel_Name"])]
    seq = [r["Kernel_Name"].split("(")[0].replace("void ", "").replace("mpas::", "").strip()
           for r in rows[ends[-3] + 1:ends[-1] + 1]]

    drops = stage_drops(seq, 2, skip_stage_avg)

    def acc(full, skipped=frozenset()):
        base = full.split("<")[0]
        if base not in amap:
            return set(), set()
        R, W = (set(x) for x in amap[base])
        R -= kr.NOT_DEFAULT
        W -= kr.NOT_DEFAULT | skipped
        for pre, rule in kr.VARIANT.items():
            if full.startswith(pre):
                R -= rule.get("drop", set())
                W -= rule.get("drop_w", set())

        def key(m):
            k = kr.field_key(m, reg)
            if k is None:
                return None
            return k + ":" + m.rstrip("_rd")[-1] if k.startswith("state.") else k
        R = {key(m) for m in R} | {k + ":x" for k in kr.EXTRA_READS.get(base, set())}
        W = {key(m) for m in W}
        return {r for r in R if r}, {w for w in W if w}

    n = len(seq)
    pending, dead = {}, {}
    both = seq + seq
    for i, k in enumerate(both):
        R, W = acc(k, drops[i % n])
        for a in R:
            pending.pop(a, None)
        for a in W:
            if a in pending and i >= n:
                dead.setdefault((both[pending[a]], a), []).append(k)
            pending[a] = i
    for (w, a), by in sorted(dead.items()):
        print(f"{w[:40]:40s} writes {a:28s} overwritten by {by[0][:40]} (x{len(by) // 2 or 1} per dt)")


if __name__ == "__main__":
    main()

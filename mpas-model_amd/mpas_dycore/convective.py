"""The convective running maxima in numpy: what ``Dycore.diag_update()`` computes on the device.

A restatement of the arithmetic of convective_diagnostics_update
(core_atmosphere/diagnostics/convective_diagnostics.F:99-198, integral_zstaggered :548-565) on one
block's own local numbering: every binary operation in the Fortran's order, and the two sums whose
order decides the bits in the reference's order --

* the cell vorticity: the reference loops over the vertices ``v = 1..nVertices`` and their three
  cells ``j = 1..3`` and adds ``kiteAreasOnVertex(j, v) * vorticity(k, v)`` into cell
  ``cellsOnVertex(j, v)``, from 0.0.  A cell's terms arrive in ascending local vertex index, which
  is not verticesOnCell order;
* the 2-5 km integral: the levels are added in ascending k, from 0.0.

This is the yardstick of tests/test_gpu_convective.py: the oracle's harness driver does not call
mpas_atm_diag_update, so there is no compiled-reference parity for this routine (as for the
incremental analysis update).  Arrays are element-major as everywhere in this package: ``w``
(nCells, K + 1), ``vorticity`` (nVertices, K), the reconstructed winds (nCells, K).  Results are
meant for finite inputs; Fortran's ``max`` with a NaN is unspecified.
"""
from __future__ import annotations

import numpy as np

W_VELOCITY_MAX, WIND_SPEED_LEVEL1_MAX, UPDRAFT_HELICITY_MAX = 1, 2, 4   # MPAS_DYC_DIAG_*
ALL = W_VELOCITY_MAX | WIND_SPEED_LEVEL1_MAX | UPDRAFT_HELICITY_MAX
FIELDS = {W_VELOCITY_MAX: "w_velocity_max", WIND_SPEED_LEVEL1_MAX: "wind_speed_level1_max",
          UPDRAFT_HELICITY_MAX: "updraft_helicity_max"}
Z_BOT, Z_TOP = 2000.0, 5000.0   # :188


def zeros(case: dict) -> dict:
    """The three fields as a reset (convective_diagnostics_reset, :501-525) leaves them."""
    return {n: np.zeros(case["nCells"]) for n in FIELDS.values()}


def vertex_table(case: dict, n_solve: int | None = None):
    """The (cell, vertex, j) triples of the reference's scatter, in its loop order (vertex ascending,
    then j), restricted to the owned cells, and each triple's rank among its cell's triples."""
    n_solve = case["nCells"] if n_solve is None else int(n_solve)
    cov = np.asarray(case["cellsOnVertex"])
    cell = cov.ravel()                                   # C order of (nVertices, 3): vertex, then j
    vert = np.repeat(np.arange(cov.shape[0]), cov.shape[1])
    j = np.tile(np.arange(cov.shape[1]), cov.shape[0])
    keep = (cell >= 0) & (cell < n_solve)
    cell, vert, j = cell[keep], vert[keep], j[keep]
    order = np.argsort(cell, kind="stable")              # per cell, the loop order survives
    first = np.searchsorted(cell[order], cell[order], side="left")
    rank = np.empty(cell.size, dtype=np.int64)
    rank[order] = np.arange(cell.size) - first
    return cell, vert, j, rank


def updraft_helicity(case: dict, w: np.ndarray, vorticity: np.ndarray, n_solve: int | None = None) -> np.ndarray:
    """uph of the cells [0, n_solve): the 2-5 km AGL integral of max(0, w) max(0, zeta) (:166-188)."""
    n_solve = case["nCells"] if n_solve is None else int(n_solve)
    K = int(case["nVertLevels"])
    kite = np.asarray(case["kiteAreasOnVertex"], dtype=np.float64)
    cell, vert, j, rank = vertex_table(case, n_solve)
    zeta = np.zeros((n_solve, K))                                                    # :168
    for r in range(int(rank.max()) + 1 if rank.size else 0):   # a cell's r-th term, all cells at once
        s = rank == r
        zeta[cell[s]] = zeta[cell[s]] + (kite[vert[s], j[s]][:, None] * vorticity[vert[s]])   # :172
    w = np.asarray(w, dtype=np.float64)[:n_solve]
    area = np.asarray(case["areaCell"], dtype=np.float64)[:n_solve, None]
    uh = np.maximum(0.0, 0.5 * (w[:, :K] + w[:, 1:K + 1])) * np.maximum(0.0, zeta / area)    # :177-178
    zgrid = np.asarray(case["zgrid"], dtype=np.float64)[:n_solve]
    z_agl = zgrid - zgrid[:, :1]                                                     # :187
    uph = np.zeros(n_solve)                                                          # :559
    for k in range(K):                                                               # :560-564
        zb = np.maximum(z_agl[:, k], Z_BOT)
        zt = np.minimum(z_agl[:, k + 1], Z_TOP)
        uph = uph + (uh[:, k] * np.maximum(0.0, zt - zb))
    return uph


def update(case: dict, w, vorticity, uzonal, umeridional, running: dict, flags: int = ALL,
           n_solve: int | None = None) -> dict:
    """One convective_diagnostics_update: ``running`` (w_velocity_max, wind_speed_level1_max,
    updraft_helicity_max, each (nCells,)) advanced on the cells [0, n_solve) (default: every cell of
    the case; a block passes its nCellsSolve) for the fields named by ``flags``.  Returns new arrays;
    halo cells and unnamed fields keep their values."""
    if flags & ~ALL:
        raise ValueError(f"unknown flag bits in {flags}")
    n_solve = case["nCells"] if n_solve is None else int(n_solve)
    K = int(case["nVertLevels"])
    out = {n: np.array(running[n], dtype=np.float64, copy=True) for n in FIELDS.values()}
    if flags & W_VELOCITY_MAX:                                                       # :156
        f = out["w_velocity_max"]
        f[:n_solve] = np.maximum(f[:n_solve], np.max(np.asarray(w)[:n_solve, :K], axis=1))
    if flags & WIND_SPEED_LEVEL1_MAX:                                                # :162
        uz, um = np.asarray(uzonal)[:n_solve, 0], np.asarray(umeridional)[:n_solve, 0]
        f = out["wind_speed_level1_max"]
        f[:n_solve] = np.maximum(f[:n_solve], np.sqrt((uz * uz) + (um * um)))
    if flags & UPDRAFT_HELICITY_MAX:                                                 # :189
        f = out["updraft_helicity_max"]
        f[:n_solve] = np.maximum(f[:n_solve], updraft_helicity(case, w, vorticity, n_solve))
    return out

"""Numpy restatement of the Ertel PV budget.

atm_compute_pvBudget_diagnostics (core_atmosphere/diagnostics/pv_diagnostics.F:1291-1613) on a block's own
numbering, after the PV diagnostics of the same time level (mpas_dycore.pv, whose geometry, theta, rho, ertel_pv
and iLev_DT it reads): dtheta_dt_mix (:1578-1584), the six diabatic terms and their sum (:1386-1473), the
frictional term (:1475-1529) and the two on the 2-PVU surface (:786-824).  The device kernels
(csrc/pvbudget.hip) follow the same sequence; this module is what they are compared with bit for bit, and
tests/golden/pvbudget.npz (tools/make_pvbudget_golden.py) pins it to the compiled reference.

Every + - * / is in the Fortran's order, as in mpas_dycore.pv.  What is particular to the budget:
  * calc_vertical_curl (:1113-1137) is a scatter over the edges in ascending edge index, so a vertex sums its
    valid edges in ascending local edge index -- not in edgesOnVertex order -- from 0.0, with - dcEdge u where it
    is verticesOnEdge(1, .) and + where it is (2, .);
  * depv_dt_diab = ((((lw + sw) + bl) + cu) + mp) + mix;
  * depv_dt_mix is guarded by dtheta_dt_mp's association (:1460), which always holds here;
  * without tend_u_phys (no physics_get_tend) the edge field is 0.0 + tend_u_euler / rho_edge.

Defined deviations, as on the device: tend_u_phys and tend_w_euler are not overwritten (the reference works in
place, :1479, :1496-1501); the outputs exist on the owned cells only; at level nVertLevels dv_dz takes velCellm
(mpas_dycore.pv).

Arrays are element-major, 0-based, as in mpas_dycore.pv.
"""
from __future__ import annotations

import numpy as np

from . import pv

ON, LW, SW, BL, CU = 1, 2, 4, 8, 16     # MPAS_DYC_PVB_*
ALL = ON | LW | SW | BL | CU
# the raw tendency of tend_physics behind each source bit, in the order of the reference's sum
RAW = ((LW, "rthratenlw", "depv_dt_lw"), (SW, "rthratensw", "depv_dt_sw"), (BL, "rthblten", "depv_dt_bl"),
       (CU, "rthcuten", "depv_dt_cu"))
OUT_3D = ("depv_dt_lw", "depv_dt_sw", "depv_dt_bl", "depv_dt_cu", "depv_dt_mp", "depv_dt_mix", "depv_dt_diab",
          "depv_dt_fric")
OUT_2D = ("depv_dt_diab_pv", "depv_dt_fric_pv")


def flags_from_todynamics(todyn_flags: int) -> int:
    """The source bits that a MPAS_DYC_TODYN_* mask implies: LW, SW, PBL -> BL, CU."""
    from . import todynamics as T
    f = 0
    for bit, src in ((T.LW, LW), (T.SW, SW), (T.PBL, BL), (T.CU, CU)):
        if todyn_flags & bit:
            f |= src
    return f


def check_flags(flags: int):
    """mpas_dyc_set_pv_budget's argument errors."""
    if flags & ~ALL:
        raise ValueError("unknown flag bits")
    if flags and not flags & ON:
        raise ValueError("a source bit without ON")


def dtheta_dt_mix(tend_theta_euler, qv):
    """:1578-1584."""
    return np.asarray(tend_theta_euler, dtype=np.float64) / (1.0 + pv.RVORD * np.asarray(qv, dtype=np.float64))


def uncouple_w(tend_w_euler, rho):
    """:1492-1501: interfaces 2..K over the mean of the two levels' rho, interface 1 over rho(1), K+1 over rho(K)."""
    tw, rho = np.asarray(tend_w_euler, dtype=np.float64), np.asarray(rho, dtype=np.float64)
    out = np.empty_like(tw)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[:, 1:-1] = tw[:, 1:-1] / (.5 * (rho[:, :-1] + rho[:, 1:]))
        out[:, 0] = tw[:, 0] / rho[:, 0]
        out[:, -1] = tw[:, -1] / rho[:, -1]
    return out


def edge_tendency(tend_u_phys, tend_u_euler, rho_edge):
    """:1477-1481; tend_u_phys None: the literal 0.0."""
    phys = 0.0 if tend_u_phys is None else np.asarray(tend_u_phys, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return phys + np.asarray(tend_u_euler, dtype=np.float64) / np.asarray(rho_edge, dtype=np.float64)


def vertical_curl(m: dict, u, order: str = "edge") -> np.ndarray:
    """calc_vertical_curl of every level (:1483-1485, :1113-1137) on the vertices of the block.  order "edge":
    the reference's, ascending local edge index; "edgesOnVertex": the slots as they stand (the variant
    tests/test_pvbudget_host.py shows to differ)."""
    nV, nE = int(m["nVertices"]), int(m["nEdges"])
    eov = np.asarray(m["edgesOnVertex"]).astype(np.int64)
    eov = np.where((eov >= 0) & (eov < nE), eov, nE)                 # the garbage slot sorts last
    if order == "edge":
        eov = np.sort(eov, axis=1)
    voe = np.asarray(m["verticesOnEdge"])
    dc = np.asarray(m["dcEdge"], dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    v = np.arange(nV)
    r = np.zeros((nV, u.shape[1]))
    for i in range(3):
        valid = eov[:, i] < nE
        e = np.where(valid, eov[:, i], 0)
        first = valid & (voe[e, 0] == v)
        second = valid & ~first & (voe[e, 1] == v)
        term = dc[e][:, None] * u[e]
        r = np.where(first[:, None], r - term, np.where(second[:, None], r + term, r))
    with np.errstate(divide="ignore", invalid="ignore"):
        return r / np.asarray(m["areaTriangle"], dtype=np.float64)[:nV, None]


def reconstruct(m: dict, u, n_solve: int) -> tuple:
    """mpas_reconstruct (mpas_vector_reconstruction.F:245-294) of an edge field on the owned cells: the sums of
    coeffs_reconstruct times u over the cell's edges, from 0.0, in edgesOnCell order."""
    n = int(n_solve)
    ne = np.asarray(m["nEdgesOnCell"])[:n]
    eoc = np.asarray(m["edgesOnCell"])[:n]
    cf = np.asarray(m["coeffs_reconstruct"], dtype=np.float64)[:n]
    u = pv._pad(u)
    out = [np.zeros((n, u.shape[1])) for _ in range(3)]
    for i in range(int(ne.max())):
        on = (i < ne)[:, None]
        ue = u[eoc[:, i]]
        out = [np.where(on, o + cf[:, i, j, None] * ue, o) for j, o in enumerate(out)]
    return tuple(out)


def _height(m: dict, n: int):
    zgrid = np.asarray(m["zgrid"], dtype=np.float64)[:n]
    return 0.5 * (zgrid[:, :-1] + zgrid[:, 1:])                      # calc_heightCellCenter


def _gradxu(m: dict, g: dict, zc, w, vel, vort) -> list:
    """calc_gradxu_cell (:901-1022) before local2FullVorticity on the cells of g: the curl of (vel, w) with the
    vertex field vort as its vertical component.  vel: (n, K, 3)."""
    n, me = g["g1"].shape
    ne = g["nEdgesOnCell"]
    coc = np.asarray(m["cellsOnCell"])[:n]
    w = pv._pad(w)
    wc = .5 * (w[:, 1:] + w[:, :-1])
    w_edges = [0.5 * (wc[coc[:, i]] + wc[:n]) for i in range(me)]
    dw_dx, dw_dy = pv._horiz(w_edges, g["g1"], ne, g["vol"]), pv._horiz(w_edges, g["g2"], ne, g["vol"])
    du_dz = pv._vert((pv._dot(vel, g["x1"][:, None, :]), zc))
    dv_dz = pv._vert((pv._dot(vel, g["x2"][:, None, :]), zc))         # level K: velCellm (the defined deviation)
    return [dw_dy - dv_dz, du_dz - dw_dx, pv.vertical_vorticity(m, g, vort)]


def _grad(m: dict, g: dict, zc, field) -> list:
    """calc_grad_cell (:1024-1111) on the cells of g."""
    n, me = g["g1"].shape
    ne = g["nEdgesOnCell"]
    coc = np.asarray(m["cellsOnCell"])[:n]
    f = pv._pad(field)
    edges = [0.5 * (f[coc[:, i]] + f[:n]) for i in range(me)]
    return [pv._horiz(edges, g["g1"], ne, g["vol"]), pv._horiz(edges, g["g2"], ne, g["vol"]), pv._vert((f[:n], zc))]


def _dot3(a, b):
    return ((0.0 + a[0] * b[0]) + a[1] * b[1]) + a[2] * b[2]


def _cells(a, n):
    return np.asarray(a, dtype=np.float64)[:n]


def budget(m: dict, g: dict, f: dict, flags: int, curl_order: str = "edge", reverse_sum: bool = False) -> dict:
    """calc_pvBudget (:1291-1538) on the cells of g.  f: theta, rho, w, uReconstructX/Y/Z, vorticity as for
    pv.epv; the raw tendencies whose bits are set, dtheta_dt_mp, dtheta_dt_mix; tend_u_euler, rho_edge, tend_w_euler
    and tend_u_phys (or None).  m carries coeffs_reconstruct, dcEdge, areaTriangle, verticesOnEdge, edgesOnVertex.
    curl_order / reverse_sum: the two summation-order variants of the tests."""
    n = g["g1"].shape[0]
    zc = _height(m, n)
    rho = _cells(f["rho"], n)
    vel = np.stack([_cells(f[k], n) for k in ("uReconstructX", "uReconstructY", "uReconstructZ")], axis=-1)
    gxu = _gradxu(m, g, zc, f["w"], vel, f["vorticity"])
    gxu = [(a + g["ev"][:, j, None]) / rho for j, a in enumerate(gxu)]
    out = {}
    srcs = [(name, dep, bool(flags & bit)) for bit, name, dep in RAW]
    srcs += [("dtheta_dt_mp", "depv_dt_mp", True), ("dtheta_dt_mix", "depv_dt_mix", True)]   # :1448, :1460
    for name, dep, on in srcs:
        out[dep] = _dot3(gxu, _grad(m, g, zc, f[name])) * 1.0e6 if on else np.zeros_like(rho)
    terms = [out[dep] for _, dep, _ in srcs]
    if reverse_sum:
        terms = terms[::-1]
    diab = terms[0]
    for t in terms[1:]:
        diab = diab + t
    out["depv_dt_diab"] = diab
    tend_u = edge_tendency(f.get("tend_u_phys"), f["tend_u_euler"], f["rho_edge"])
    curl = vertical_curl(m, tend_u, order=curl_order)
    tendu = np.stack(reconstruct(m, tend_u, n), axis=-1)
    tend_w = uncouple_w(f["tend_w_euler"], f["rho"])
    gth = [a / rho for a in _grad(m, g, zc, f["theta"])]
    out["depv_dt_fric"] = _dot3(_gradxu(m, g, zc, tend_w, tendu, curl), gth) * 1.0e6
    out["tend_u"], out["curl"], out["tend_w"] = tend_u, curl, tend_w
    out["tenduX"], out["tenduY"], out["tenduZ"] = (tendu[..., j] for j in range(3))
    return out


def interp(ertel_pv, field1, ilev, lat) -> np.ndarray:
    """interp_pv (:826-899) as pv.interp_pv, but for iLev_DT = 1 -- which floodFill_tropo never gives, and the
    fixture hands in -- with the reference's own reads: level 0 of the column is the element before it in
    memory, the top level of the cell before (the block's first cell must not have it)."""
    f0, f1 = np.asarray(ertel_pv, dtype=np.float64), np.asarray(field1, dtype=np.float64)
    n, K = f0.shape
    ilev = np.asarray(ilev)[:n].astype(np.int64)
    inside = (ilev >= 1) & (ilev <= K)
    assert not (inside[0] and ilev[0] == 1), "iLev_DT = 1 in the first cell reads before the array"
    ih = np.arange(n) * K + np.clip(ilev - 1, 0, K - 1)
    il = np.where(inside, ih - 1, ih)
    a0, a1 = np.ascontiguousarray(f0).ravel(), np.ascontiguousarray(f1).ravel()
    val = pv.PVU_VAL * pv._sgn_hemi(lat)[:n]
    dv_dl = a0[ih] - a0[il]
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(np.abs(dv_dl) < 1.e-6, 0.5, (val - a0[il]) / dv_dl)
    return np.where(inside, a1[il] + (a1[ih] - a1[il]) * frac, np.where(ilev < 1, f1[:, 0], f1[:, K - 1]))


def driver(m: dict, f: dict, flags: int, n_solve: int | None = None, ertel_pv_held=None, ilev=None,
           curl_order: str = "edge", reverse_sum: bool = False, mix_held=None, theta_held=None) -> dict:
    """mpas_dyc_pv_budget_diagnostics on one block without its halo exchanges: pv.driver, then the budget on the
    same fields.  m: what pv.driver needs, and coeffs_reconstruct, dcEdge, areaTriangle, verticesOnEdge,
    edgesOnVertex.  f: what pv.driver needs, and tend_theta_euler, tend_u_euler, tend_w_euler, rho_edge, the raw
    tendencies whose bits are set, and optionally dtheta_dt_mp (default 0.0) and tend_u_phys (default: absent).
    ilev: an iLev_DT handed in for the two interpolations instead of the fill's (the fixture).  mix_held: what
    diag.dtheta_dt_mix holds on the cells past n_solve after its halo exchange (default: what the block computes
    there itself), as ertel_pv_held; theta_held: the same for diag.theta (pv.driver).  Returns pv.driver's
    outputs, dtheta_dt_mix (nCells, K), the eight depv_dt_* (n_solve, K), the two *_pv (n_solve) and the
    intermediates tend_u, curl, tend_w, tenduX/Y/Z."""
    check_flags(flags)
    n = int(m["nCells"])
    ns = n if n_solve is None else int(n_solve)
    out = pv.driver(m, f, ns, ertel_pv_held, theta_held)
    if not flags:
        return out
    g = pv.geom(m, ns)
    mix = dtheta_dt_mix(f["tend_theta_euler"], f["qv"])
    if mix_held is not None:
        mix[ns:] = np.asarray(mix_held, dtype=np.float64)[ns:]
    mp = f.get("dtheta_dt_mp")
    fb = dict(f, theta=out["theta"], rho=out["rho"], dtheta_dt_mix=mix,
              dtheta_dt_mp=np.zeros_like(mix) if mp is None else np.asarray(mp, dtype=np.float64))
    out["dtheta_dt_mix"] = mix
    out.update(budget(m, g, fb, flags, curl_order, reverse_sum))
    lev = out["iLev_DT"] if ilev is None else np.asarray(ilev)
    lat = np.asarray(m["latCell"])
    for name in ("depv_dt_diab", "depv_dt_fric"):
        out[name + "_pv"] = interp(out["ertel_pv"][:ns], out[name], lev, lat)
    return out


# ---- the fixture tests/golden/pvbudget.npz (tools/make_pvbudget_golden.py) ----
FIXTURE_MESH_LEVEL = 1
FIXTURE_KS = (4, 65)
FIXTURE_SETS = {"all": ALL, "none": ON, "lwcu": ON | LW | CU}
FIXTURE_CELL_FIELDS = ("rthratenlw", "rthratensw", "rthblten", "rthcuten", "dtheta_dt_mp", "tend_theta_euler",
                       "tend_w_euler")
FIXTURE_EDGE_FIELDS = ("tend_u_phys", "tend_u_euler", "rho_edge")
FIXTURE_FIELDS = pv.FIXTURE_FIELDS + FIXTURE_CELL_FIELDS + FIXTURE_EDGE_FIELDS
# what the file stores of a source set other than "all": the rest has the bits of "all" (the tool asserts it)
FIXTURE_SET_FIELDS = ("depv_dt_lw", "depv_dt_sw", "depv_dt_bl", "depv_dt_cu", "depv_dt_diab", "depv_dt_diab_pv")


def fixture_mesh() -> dict:
    """The fixture's mesh: the level-1 icosahedral mesh (42 cells, 12 of them pentagons) with the vector arrays of
    mpas_initialize_vectors and the reconstruction coefficients of mpas_init_reconstruct."""
    from . import mesh, reconstruct as rec
    m = mesh.build_mesh(FIXTURE_MESH_LEVEL)
    vec = rec.initialize_vectors(m)
    m.update(vec)
    m["coeffs_reconstruct"] = rec.init_reconstruct(m, vec)
    return m


def fixture_state(z, K: int, name: str = "all") -> tuple:
    """(inputs as float64, the handed-in iLev_DT, the compiled reference's outputs of source set `name`): the 3-D
    outputs hold the levels 1..K-1 (the reference's level K is undefined)."""
    f = {n: np.asarray(z[f"{n}_K{K}"], dtype=np.float64) for n in FIXTURE_FIELDS}
    ref = {}
    for n in OUT_3D + OUT_2D + ("dtheta_dt_mix",):
        key = f"ref_{name}_{n}_K{K}"
        ref[n] = np.asarray(z[key if key in z else f"ref_all_{n}_K{K}"])
    return f, np.asarray(z[f"iLev_DT_K{K}"]), ref


def fixture_driver(m: dict, f: dict, flags: int, ilev=None, **kw) -> dict:
    """driver() on a fixture state: zz = 1, zgrid the state's."""
    return driver(dict(m, zgrid=f["zgrid"], zz=np.ones_like(f["rho_zz"])), f, flags, ilev=ilev, **kw)

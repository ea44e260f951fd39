"""Numpy restatement of the Ertel PV and dynamic-tropopause diagnostics.

atm_compute_pv_diagnostics (core_atmosphere/diagnostics/pv_diagnostics.F:1218-1289) on a block's own
numbering: the theta / rho preamble, calc_epv (:1139-1216) with calc_gradxu_cell / calc_grad_cell and their
helpers (:147-422, :901-1111), floodFill_tropo (:581-716) and interp_pv_diagnostics / interp_pv (:718-784,
:826-899).  The device kernels (csrc/pv.hip) follow the same sequence; this module is what they are compared
with bit for bit, and tests/golden/pv_x1.162.npz (tools/make_pv_golden.py) pins it to the compiled reference.

Every + - * / sqrt is in the Fortran's order:
  * dotProduct and normalizeVector sum from 0.0, left to right: ((0 + a1 b1) + a2 b2) + a3 b3;
  * calc_horizDeriv_fv normalises again the edge normal that calc_gradxu_cell already normalised and signed;
  * the average face height is a running sum of 100.0 divided by nEdgesOnCell.
What does not depend on the level (``geom``) is formed once per cell, with the operations the Fortran
repeats at every level, so no bit of ertel_pv changes (tests/test_pv_host.py).

One defined deviation: at level nVertLevels the reference forms dv_dz from velCellp, a local it never
set there (:997).  Here, as on the device, that line takes velCellm, like the u line two above it.

Arrays are element-major, 0-based: a field is (nCells, K); an index of -1 (no neighbour in the block)
reads the garbage slot, which is never in the troposphere.  The PV budget (calc_pvBudget) is restated in
mpas_dycore.pvbudget, on top of this module; floodFill_strato is not restated: the reference never calls it.
"""
from __future__ import annotations

import numpy as np

OMEGA = 7.29212e-5          # mpas_constants: omega
RVORD = 461.6 / 287.0       # mpas_constants: rvord = rv / rgas
PVU_VAL = 2.0               # pvuVal (:1282)
SEED_LEVELS = 3             # floodFill_tropo seeds levels 1..min(K, 3) (:643)


def _dot(a, b):
    """dotProduct (:147-164): from 0.0, left to right."""
    return ((0.0 + a[..., 0] * b[..., 0]) + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize(v):
    """normalizeVector (:329-345)."""
    mag = np.sqrt(((0.0 + v[..., 0] * v[..., 0]) + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    return v / mag[..., None]


def _sgn_hemi(lat):
    """sign(1.0, latCell), with the `.EQ. 0.0 -> 1.0` line that never fires (:632-633)."""
    return np.copysign(1.0, np.asarray(lat, dtype=np.float64))


def theta_rho(theta_m, qv, rho_zz, zz):
    """The preamble (:1253-1258)."""
    return theta_m / (1.0 + RVORD * qv), rho_zz * zz


def kite_slot(m: dict, n_solve: int):
    """elementIndexInArray(c0, cellsOnVertex(:, verticesOnCell(i, c0)), 3) per (cell, slot): the first match."""
    voc = np.asarray(m["verticesOnCell"])[:n_solve]
    cov = np.asarray(m["cellsOnVertex"])[voc]                       # (n, ME, 3)
    hit = cov == np.arange(n_solve)[:, None, None]
    return voc, np.argmax(hit, axis=2)


def geom(m: dict, n_solve: int | None = None) -> dict:
    """What calc_gradxu_cell / calc_grad_cell form per cell whatever the level (the device's k_pv_geom):
    x1, x2 the normalised tangent vectors; g1, g2 per edge slot (dvEdge * 100.0) times the dot product of
    the twice-normalised, sign-flipped edge normal with x1 / x2; vol = volumeCell; ev the three
    Earth-vorticity components; kite the cell's kite area at each of its vertices; area = areaCell."""
    n = int(m["nCells"] if n_solve is None else n_solve)
    ne = np.asarray(m["nEdgesOnCell"])[:n]
    me = int(ne.max())
    ctp = np.asarray(m["cellTangentPlane"], dtype=np.float64)[:n]
    x1, x2 = _normalize(ctp[:, 0]), _normalize(ctp[:, 1])
    x3 = np.asarray(m["localVerticalUnitVectors"], dtype=np.float64)[:n]
    eoc = np.asarray(m["edgesOnCell"])[:n]
    coe = np.asarray(m["cellsOnEdge"])
    env = np.asarray(m["edgeNormalVectors"], dtype=np.float64)
    dv = np.asarray(m["dvEdge"], dtype=np.float64)
    area = np.asarray(m["areaCell"], dtype=np.float64)[:n]
    g1, g2 = np.zeros((n, me)), np.zeros((n, me))
    avg = np.zeros(n)
    for i in range(me):
        on = i < ne
        e = np.where(on, eoc[:, i], 0)
        sign = np.where(coe[e, 0] == np.arange(n), 1.0, -1.0)      # fluxSign
        normal = _normalize(env[e]) * sign[:, None]
        unit = _normalize(normal)                                    # calc_horizDeriv_fv, again
        face = dv[e] * 100.0
        g1[:, i] = np.where(on, face * _dot(unit, x1), 0.0)
        g2[:, i] = np.where(on, face * _dot(unit, x2), 0.0)
        avg = np.where(on, avg + 100.0, avg)
    avg = avg / ne.astype(np.float64)
    e_vort = 2.0 * OMEGA
    ev = np.stack([(0.0 + 0.0 * x[:, 0]) + 0.0 * x[:, 1] + e_vort * x[:, 2] for x in (x1, x2, x3)], axis=1)
    voc, j = kite_slot(m, n)
    kite = np.asarray(m["kiteAreasOnVertex"], dtype=np.float64)[voc, j]
    kite = np.where(np.arange(kite.shape[1])[None, :] < ne[:, None], kite, 0.0)[:, :me]
    return dict(x1=x1, x2=x2, g1=g1, g2=g2, vol=area * avg, ev=ev, kite=kite, area=area, nEdgesOnCell=ne)


def _pad(a):
    """A field with its garbage row (zero), so that index -1 reads it."""
    a = np.asarray(a, dtype=np.float64)
    return np.concatenate([a, np.zeros((1,) + a.shape[1:])], axis=0)


def _horiz(val_edges, g, ne, vol):
    """calc_horizDeriv_fv (:368-395) with the level-independent factor g; val_edges a list per slot."""
    rsum = np.zeros_like(val_edges[0])
    for i, vale in enumerate(val_edges):
        rsum = np.where((i < ne)[:, None], rsum + vale * g[:, i, None], rsum)
    return rsum / vol[:, None]


def _vert(val):
    """calc_vertDeriv_one at the ends, calc_vertDeriv_center inside (:398-422): val = (value, height)."""
    v, z = val
    dp = (v[:, 1:] - v[:, :-1]) / (z[:, 1:] - z[:, :-1])            # between k and k + 1
    out = np.empty_like(v)
    out[:, 0] = dp[:, 0]
    out[:, -1] = dp[:, -1]
    out[:, 1:-1] = 0.5 * (dp[:, 1:] + dp[:, :-1])
    return out


def vertical_vorticity(m: dict, g: dict, vorticity) -> np.ndarray:
    """calc_verticalVorticity_cell (:245-267) on the cells of g: kite * vort / areaCell in verticesOnCell order."""
    n, me = g["kite"].shape
    voc = np.asarray(m["verticesOnCell"])[:n]
    vort = _pad(vorticity)
    out = np.zeros((n, vort.shape[1]))
    for i in range(me):
        term = g["kite"][:, i, None] * vort[voc[:, i]] / g["area"][:, None]
        out = np.where((i < g["nEdgesOnCell"])[:, None], out + term, out)
    return out


def epv(m: dict, g: dict, f: dict) -> np.ndarray:
    """calc_epv (:1194-1215) on the cells of g.  f: theta, rho, w, uReconstructX/Y/Z (nCells, ...),
    vorticity (nVertices, K)."""
    n, me = g["g1"].shape
    ne = g["nEdgesOnCell"]
    coc = np.asarray(m["cellsOnCell"])[:n]
    zgrid = np.asarray(m["zgrid"], dtype=np.float64)[:n]
    theta, w = _pad(f["theta"]), _pad(f["w"])
    rho = np.asarray(f["rho"], dtype=np.float64)[:n]
    zc = 0.5 * (zgrid[:, :-1] + zgrid[:, 1:])                        # calc_heightCellCenter
    wc = .5 * (w[:, 1:] + w[:, :-1])
    w0, t0 = wc[:n], theta[:n]
    w_edges = [0.5 * (wc[coc[:, i]] + w0) for i in range(me)]
    t_edges = [0.5 * (theta[coc[:, i]] + t0) for i in range(me)]
    dw_dx, dw_dy = _horiz(w_edges, g["g1"], ne, g["vol"]), _horiz(w_edges, g["g2"], ne, g["vol"])
    vel = np.stack([np.asarray(f[k], dtype=np.float64)[:n] for k in ("uReconstructX", "uReconstructY", "uReconstructZ")],
                   axis=-1)
    du_dz = _vert((_dot(vel, g["x1"][:, None, :]), zc))
    dv_dz = _vert((_dot(vel, g["x2"][:, None, :]), zc))              # level K: velCellm (the defined deviation)
    gxu = [dw_dy - dv_dz, du_dz - dw_dx, vertical_vorticity(m, g, f["vorticity"])]
    gxu = [(a + g["ev"][:, j, None]) / rho for j, a in enumerate(gxu)]
    gth = [_horiz(t_edges, g["g1"], ne, g["vol"]), _horiz(t_edges, g["g2"], ne, g["vol"]), _vert((t0, zc))]
    return (((0.0 + gxu[0] * gth[0]) + gxu[1] * gth[1]) + gxu[2] * gth[2]) * 1.0e6


def candidates(ertel_pv, lat) -> np.ndarray:
    """candInTropo before the seeding (:631-638), with the garbage row (never a candidate)."""
    c = (np.asarray(ertel_pv) * _sgn_hemi(lat)[:, None] - PVU_VAL) < 0
    return np.concatenate([c, np.zeros((1, c.shape[1]), dtype=bool)], axis=0)


def flood_fill_tropo(m: dict, ertel_pv, count_sweeps: bool = False):
    """floodFill_tropo (:581-716) over all cells of the block: inTropo as its unique fixed point -- the
    candidate cell-levels connected to a seed (levels 1..min(K, 3)) through vertical neighbours and
    same-level horizontal neighbours -- reached as the device reaches it: a sweep ORs in the neighbours'
    members of the sweep before, masks with the candidates and closes each column vertically.
    Returns (inTropo (nCells, K), iLev_DT (nCells) int32[, sweeps that changed something])."""
    n = int(m["nCells"])
    K = np.asarray(ertel_pv).shape[1]
    cand = candidates(np.asarray(ertel_pv)[:n], np.asarray(m["latCell"])[:n])
    ne = np.asarray(m["nEdgesOnCell"])[:n]
    coc = np.asarray(m["cellsOnCell"])[:n]
    coc = np.where((np.arange(coc.shape[1])[None, :] < ne[:, None]) & (coc >= 0), coc, n)
    mem = np.zeros_like(cand)
    mem[:, :min(K, SEED_LEVELS)] = cand[:, :min(K, SEED_LEVELS)]
    sweeps = 0
    for _ in range(n + 1):
        new = mem.copy()
        for i in range(coc.shape[1]):
            new[:n] |= mem[coc[:, i]]
        new &= cand
        for k in range(1, K):
            new[:, k] |= new[:, k - 1] & cand[:, k]
        for k in range(K - 2, -1, -1):
            new[:, k] |= new[:, k + 1] & cand[:, k]
        if np.array_equal(new, mem):
            break
        mem = new
        sweeps += 1
    top = K - np.argmax(mem[:n, ::-1], axis=1)                       # highest member level, 1-based
    ilev = np.where(mem[:n].any(axis=1), top + 1, 0).astype(np.int32)
    return (mem[:n], ilev, sweeps) if count_sweeps else (mem[:n], ilev)


def interp_pv(ertel_pv, field1, ilev, lat, info: bool = False):
    """interp_pv (:826-899): field1 where ertel_pv is 2 sign(lat) PVU, between levels iLev_DT - 1 and iLev_DT."""
    f0, f1 = np.asarray(ertel_pv, dtype=np.float64), np.asarray(field1, dtype=np.float64)
    n, K = f0.shape
    ilev = np.asarray(ilev)[:n].astype(np.int64)
    val = PVU_VAL * _sgn_hemi(lat)[:n]
    inside = (ilev >= 1) & (ilev <= K)
    hi = np.clip(ilev - 1, 1, K - 1)                                 # 0-based level iLev; iLev - 1 below it
    r = np.arange(n)
    valh, vall = f0[r, hi], f0[r, hi - 1]
    dv_dl = valh - vall
    small = np.abs(dv_dl) < 1.e-6
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(small, 0.5, (val - vall) / dv_dl)
    fh, fl = f1[r, hi], f1[r, hi - 1]
    out = np.where(inside, fl + (fh - fl) * frac, np.where(ilev < 1, f1[:, 0], f1[:, K - 1]))
    return (out, inside & small) if info else out


def driver(m: dict, f: dict, n_solve: int | None = None, ertel_pv_held=None, theta_held=None) -> dict:
    """atm_compute_pv_diagnostics on one block without its halo exchanges.  m: the block's mesh arrays
    with cellTangentPlane, localVerticalUnitVectors, edgeNormalVectors, zgrid, zz.  f: theta_m, qv, rho_zz,
    w, uReconstructX/Y/Z, uReconstructZonal/Meridional (nCells, ...) and vorticity (nVertices, K) of the
    time level.  ertel_pv_held: what diag.ertel_pv holds on the cells past n_solve (default 0.0) -- the
    fill reads it, as the reference's does after its exchange.  theta_held: what diag.theta holds there after
    its exchange (default: what the block computes from its own halo of theta_m and qv).  Returns theta, rho (nCells, K), ertel_pv
    (nCells, K), iLev_DT (nCells) and u_pv, v_pv, theta_pv, vort_pv (n_solve)."""
    n = int(m["nCells"])
    ns = n if n_solve is None else int(n_solve)
    theta, rho = theta_rho(np.asarray(f["theta_m"], dtype=np.float64), np.asarray(f["qv"], dtype=np.float64),
                           np.asarray(f["rho_zz"], dtype=np.float64), np.asarray(m["zz"], dtype=np.float64))
    if theta_held is not None:
        theta[ns:] = np.asarray(theta_held, dtype=np.float64)[ns:]
    g = geom(m, ns)
    K = theta.shape[1]
    pv = np.zeros((n, K)) if ertel_pv_held is None else np.array(ertel_pv_held, dtype=np.float64)
    pv[:ns] = epv(m, g, {**f, "theta": theta, "rho": rho})
    mem, ilev = flood_fill_tropo(m, pv)
    lat = np.asarray(m["latCell"])
    vvort = vertical_vorticity(m, g, f["vorticity"])
    out = dict(theta=theta, rho=rho, ertel_pv=pv, iLev_DT=ilev, inTropo=mem)
    for name, src in (("u_pv", f["uReconstructZonal"]), ("v_pv", f["uReconstructMeridional"]), ("theta_pv", theta),
                      ("vort_pv", vvort)):
        out[name] = interp_pv(pv[:ns], np.asarray(src)[:ns], ilev, lat)
    return out


# ---- the fixture tests/golden/pv_x1.162.npz (tools/make_pv_golden.py) ----
FIXTURE_MESH_LEVEL = 2
FIXTURE_FIELDS = ("zgrid", "theta_m", "qv", "rho_zz", "w", "uReconstructX", "uReconstructY", "uReconstructZ",
                  "uReconstructZonal", "uReconstructMeridional", "vorticity")
FIELDS_2D = ("u_pv", "v_pv", "theta_pv", "vort_pv")


def fixture_mesh() -> dict:
    """The fixture's mesh: the level-2 icosahedral mesh (162 cells) with the three vector arrays of
    mpas_initialize_vectors."""
    from . import mesh, reconstruct
    m = mesh.build_mesh(FIXTURE_MESH_LEVEL)
    m.update(reconstruct.initialize_vectors(m))
    return m


def fixture_state(z, K: int) -> tuple:
    """(inputs as float64, the compiled reference's outputs) of the fixture's K-level state: ertel_pv holds the
    levels 1..K-1 (the reference's level K is undefined), inTropo is unpacked."""
    f = {n: np.asarray(z[f"{n}_K{K}"], dtype=np.float64) for n in FIXTURE_FIELDS}
    ref = {n: np.asarray(z[f"ref_{n}_K{K}"]) for n in ("ertel_pv", "iLev_DT") + FIELDS_2D}
    ref["inTropo"] = np.unpackbits(np.asarray(z[f"ref_inTropo_K{K}"]), axis=1)[:, :K].astype(bool)
    return f, ref


def fixture_driver(m: dict, f: dict) -> dict:
    """driver() on a fixture state: zz = 1, zgrid the state's."""
    return driver(dict(m, zgrid=f["zgrid"], zz=np.ones_like(f["rho_zz"])), f)


def column_only_members(cand: np.ndarray) -> np.ndarray:
    """The members a column would have on its own: the candidates connected to a seed level vertically."""
    mem = np.zeros_like(cand)
    mem[:, :min(cand.shape[1], SEED_LEVELS)] = cand[:, :min(cand.shape[1], SEED_LEVELS)]
    for k in range(1, cand.shape[1]):
        mem[:, k] |= mem[:, k - 1] & cand[:, k]
    for k in range(cand.shape[1] - 2, -1, -1):
        mem[:, k] |= mem[:, k + 1] & cand[:, k]
    return mem


def conditions(m: dict, ertel_pv: np.ndarray) -> dict:
    """What a fixture state must exercise (tools/make_pv_golden.py asserts it, tests/test_pv_host.py again):
    cells with iLev_DT = 0, = K + 1 and inside the column (by hemisphere), cells on interp_pv's
    abs(dv_dl) < 1e-6 branch, columns with a candidate level above a non-candidate one that the fill never
    reaches (where a plain top-down search gives another iLev_DT), columns with a level reached only
    sideways, the fill's sweeps that change something, the pentagons."""
    nC, K = ertel_pv.shape
    lat = np.asarray(m["latCell"])
    mem, ilev, sweeps = flood_fill_tropo(m, ertel_pv, count_sweeps=True)
    cand = candidates(ertel_pv, lat)[:nC]
    interior = (ilev >= 2) & (ilev <= K)
    _, small = interp_pv(ertel_pv, ertel_pv, ilev, lat, info=True)
    below_noncand = np.concatenate([np.zeros((nC, 1), dtype=bool), ~cand[:, :-1]], axis=1)
    plain_top_down = np.where(cand.any(axis=1), K - np.argmax(cand[:, ::-1], axis=1) + 1, 0)
    detached = np.any(cand & ~mem & below_noncand, axis=1) & (plain_top_down != ilev)
    return dict(none=int(np.sum(ilev == 0)), above=int(np.sum(ilev == K + 1)), interior=float(np.mean(interior)),
                north=int(np.sum(interior & (lat > 0))), south=int(np.sum(interior & (lat < 0))),
                small_dv_dl=int(np.sum(small)), detached=int(np.sum(detached)),
                sideways=int(np.sum(np.any(mem & ~column_only_members(cand), axis=1))), sweeps=int(sweeps),
                pentagons=int(np.sum(np.asarray(m["nEdgesOnCell"]) == 5)))

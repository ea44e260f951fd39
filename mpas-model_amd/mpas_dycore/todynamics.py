"""physics_get_tend (physics/mpas_atmphys_todynamics.F:59-434) restated in numpy, one Fortran statement
per line in its operand order: the yardstick of the device's kernels (csrc/todynamics.hip) and of a host
that still couples the physics tendencies by itself.

Arrays are element-major without the garbage slot: cell fields (nCells, K), edge fields (nEdges, K),
scalars (nCells, K, num_scalars); ``east`` / ``north`` (nCells, 3), ``edgeNormalVectors`` (nEdges, 3),
``cellsOnEdge`` (nEdges, 2) 0-based with -1 for a missing cell, which reads as the garbage cell: zero
tendencies and zero vectors.  Every + * / is a separate fp64 numpy operation, so the bits are the
compiled reference's (tests/golden/todynamics.npz)."""
from __future__ import annotations

import numpy as np

R_D, R_V = 287.0, 461.6
RVORD = R_V / R_D

# MPAS_DYC_TODYN_* of include/mpas_dycore.h
PBL, PBL_MYNN, CU, CU_KF, CU_WINDS, LW, SW, RQVDYNTEN = 1, 2, 4, 8, 16, 32, 64, 128
ALL = 255

RAW_CELL = ("rublten", "rvblten", "rthblten", "rqvblten", "rqcblten", "rqiblten", "rniblten", "rucuten", "rvcuten",
            "rthcuten", "rqvcuten", "rqccuten", "rqrcuten", "rqicuten", "rqscuten", "rthratenlw", "rthratensw")
EDGE_FIELDS = ("rublten_Edge", "rucuten_Edge")

# config_pbl_scheme / config_convection_scheme (Registry.xml possible_values) -> flags
PBL_SCHEMES = {None: 0, "off": 0, "bl_ysu": PBL, "bl_mynn": PBL | PBL_MYNN}
CONVECTION_SCHEMES = {None: 0, "off": 0, "cu_kain_fritsch": CU | CU_KF, "cu_tiedtke": CU | CU_WINDS,
                      "cu_ntiedtke": CU | CU_WINDS, "cu_grell_freitas": CU}


def scheme_flags(pbl=None, convection=None, lw: bool = False, sw: bool = False, rqvdynten: bool = False) -> int:
    """The reference's scheme names -> the MPAS_DYC_TODYN_* mask.  ``lw`` / ``sw``: a radiation scheme's
    name, or a bool (config_radt_*_scheme /= 'off')."""
    if pbl not in PBL_SCHEMES:
        raise ValueError(f"unknown config_pbl_scheme {pbl!r}: one of {sorted(k for k in PBL_SCHEMES if k)}")
    if convection not in CONVECTION_SCHEMES:
        raise ValueError(f"unknown config_convection_scheme {convection!r}: one of "
                         f"{sorted(k for k in CONVECTION_SCHEMES if k)}")
    on = lambda s: bool(s) and s != "off"
    return (PBL_SCHEMES[pbl] | CONVECTION_SCHEMES[convection] | (LW if on(lw) else 0) | (SW if on(sw) else 0)
            | (RQVDYNTEN if rqvdynten else 0))


def init_dirs(latCell, lonCell):
    """init_dirs_forphys (mpas_atmphys_init.F:427-439): the unit vectors to the east and to the north at
    every cell centre, (nCells, 3) each.  sin / cos are the host C library's."""
    lat, lon = np.asarray(latCell, dtype=np.float64), np.asarray(lonCell, dtype=np.float64)

    def normalize(ax, ay, az):  # r3_normalize, :453-456
        mi = 1.0 / np.sqrt(ax ** 2 + ay ** 2 + az ** 2)
        return np.stack([ax * mi, ay * mi, az * mi], axis=1)

    east = normalize(-np.sin(lon), np.cos(lon), np.zeros_like(lon))
    north = normalize(-np.cos(lon) * np.sin(lat), -np.sin(lon) * np.sin(lat), np.cos(lat))
    return east, north


def with_vectors(case: dict) -> dict:
    """The case with the vectors the projection reads: east / north (init_dirs of its cell centres) and
    edgeNormalVectors (reconstruct.initialize_vectors; a case that has them keeps its own)."""
    from .reconstruct import initialize_vectors
    out = dict(case)
    if "east" not in case or "north" not in case:
        out["east"], out["north"] = init_dirs(case["latCell"], case["lonCell"])
    if "edgeNormalVectors" not in case:
        with np.errstate(invalid="ignore"):
            out["edgeNormalVectors"] = initialize_vectors(case)["edgeNormalVectors"]
    return out


def _slot(a):
    """The array with its garbage slot: a zero row at the end."""
    a = np.asarray(a, dtype=np.float64)
    return np.concatenate([a, np.zeros((1,) + a.shape[1:])], axis=0)


def tend_to_edges(ux, uy, cellsOnEdge, east, north, edgeNormalVectors, dot_right: bool = False):
    """tend_toEdges (:494-510) on every edge: (nEdges, K)."""
    coe = np.asarray(cellsOnEdge)
    nC = np.asarray(ux).shape[0]
    coe = np.where((coe < 0) | (coe > nC), nC, coe)
    ux, uy, east, north = _slot(ux), _slot(uy), _slot(east), _slot(north)
    nv = np.asarray(edgeNormalVectors, dtype=np.float64)
    c1, c2 = coe[:, 0], coe[:, 1]

    def dot(v, c):
        if dot_right:  # a changed association, for the fixture's sensitivity check only
            return (nv[:, 0] * v[c, 0] + (nv[:, 1] * v[c, 1] + nv[:, 2] * v[c, 2]))[:, None]
        return (nv[:, 0] * v[c, 0] + nv[:, 1] * v[c, 1] + nv[:, 2] * v[c, 2])[:, None]

    return (ux[c1] * 0.5 * dot(east, c1)
            + uy[c1] * 0.5 * dot(north, c1)
            + ux[c2] * 0.5 * dot(east, c2)
            + uy[c2] * 0.5 * dot(north, c2))


def physics_get_tend(flags: int, indices: dict, raw: dict, rho_zz, rho_edge, theta_m, scalars, mesh: dict,
                     tend_u_phys_in=None, nCellsSolve: int | None = None, nEdgesSolve: int | None = None) -> dict:
    """physics_get_tend_work (:265-434) after the zeroing of physics_get_tend (:176-182).

    ``indices``: 0-based ``index_qv`` and, where present, ``index_qc`` / ``index_qr`` / ``index_qi`` /
    ``index_qs`` / ``index_ni`` (absent or negative: the scalar's terms are skipped).  ``raw``: the raw
    tendencies by name (those the flags do not select are not read).  ``mesh``: cellsOnEdge, east, north,
    edgeNormalVectors.  ``tend_u_phys_in``: diag.tend_u_phys before the call (zeros by default).
    Returns tend_ru_physics, tend_rtheta_physics, tend_rho_physics, scalars_tend, rublten_Edge,
    rucuten_Edge (None when not computed) and tend_u_phys; elements outside the owned range are 0.0."""
    mass = np.asarray(rho_zz, dtype=np.float64)
    mass_edge = np.asarray(rho_edge, dtype=np.float64)
    theta_m = np.asarray(theta_m, dtype=np.float64)
    scalars = np.asarray(scalars, dtype=np.float64)
    nC, K = mass.shape
    nE = mass_edge.shape[0]
    ncs = nC if nCellsSolve is None else nCellsSolve
    nes = nE if nEdgesSolve is None else nEdgesSolve
    ix = lambda n: indices.get(n, -1) if indices.get(n) is not None else -1
    iqv = indices["index_qv"]
    tend_th = np.zeros((nC, K))                                                       # :176
    tend_scalars = np.zeros(scalars.shape)                                            # :178
    tend_u = np.zeros((nE, K))                                                        # :180
    tend_theta = np.zeros((nC, K))                                                    # :181
    tend_rho = np.zeros((nC, K))                                                      # :182
    tend_u_phys = np.zeros((nE, K)) if tend_u_phys_in is None else np.array(tend_u_phys_in, dtype=np.float64)
    rublten_Edge = rucuten_Edge = None
    c, e = slice(0, ncs), slice(0, nes)
    r = lambda n: np.asarray(raw[n], dtype=np.float64)

    def add(index, name):
        if index >= 0:
            tend_scalars[c, :, index] = tend_scalars[c, :, index] + r(name)[c] * mass[c]

    def project(ux, uy):
        return tend_to_edges(r(ux), r(uy), mesh["cellsOnEdge"], mesh["east"], mesh["north"], mesh["edgeNormalVectors"],
                             bool(mesh.get("_dot_right")))

    if flags & PBL:                                                                   # :329
        rublten_Edge = project("rublten", "rvblten")                                  # :331
        tend_u_phys[:] = rublten_Edge                                                 # :334
        tend_u[e] = tend_u[e] + rublten_Edge[e] * mass_edge[e]                        # :339
        tend_th[c] = tend_th[c] + r("rthblten")[c] * mass[c]                          # :345
        add(iqv, "rqvblten")                                                          # :346
        add(ix("index_qc"), "rqcblten")                                               # :347
        add(ix("index_qi"), "rqiblten")                                               # :348
        if flags & PBL_MYNN:
            add(ix("index_ni"), "rniblten")                                           # :358
    if flags & CU:                                                                    # :368
        tend_th[c] = tend_th[c] + r("rthcuten")[c] * mass[c]                          # :372
        add(iqv, "rqvcuten")                                                          # :373
        add(ix("index_qc"), "rqccuten")                                               # :374
        add(ix("index_qi"), "rqicuten")                                               # :375
        if flags & CU_KF:
            add(ix("index_qr"), "rqrcuten")                                           # :384
            add(ix("index_qs"), "rqscuten")                                           # :385
        if flags & CU_WINDS:
            rucuten_Edge = project("rucuten", "rvcuten")                              # :391
            tend_u_phys[:] = tend_u_phys + rucuten_Edge                               # :393-394
            tend_u[e] = tend_u[e] + rucuten_Edge[e] * mass_edge[e]                    # :398
    if flags & LW:
        tend_th[c] = tend_th[c] + r("rthratenlw")[c] * mass[c]                        # :410
    if flags & SW:
        tend_th[c] = tend_th[c] + r("rthratensw")[c] * mass[c]                        # :419
    coeff = (1. + RVORD * scalars[c, :, iqv])                                         # :428
    tend_th[c] = coeff * tend_th[c] + RVORD * theta_m[c] * tend_scalars[c, :, iqv] / coeff   # :429
    tend_theta[c] = tend_theta[c] + tend_th[c]                                        # :430
    return {"tend_ru_physics": tend_u, "tend_rtheta_physics": tend_theta, "tend_rho_physics": tend_rho,
            "scalars_tend": tend_scalars, "rublten_Edge": rublten_Edge, "rucuten_Edge": rucuten_Edge,
            "tend_u_phys": tend_u_phys}


# ---- the fixture tests/golden/todynamics.npz (tools/make_todynamics_golden.py) ----
FIXTURE_MESH_LEVEL = 1                    # mesh.build_mesh(1): 42 cells (12 pentagons), 120 edges, one block
FIXTURE_KS = (4, 5)                       # (nCells + 1) K is even at 4 and odd at 5
FIXTURE_NUM_SCALARS = 7                   # qv qc qr qi qs qg ni
FIXTURE_INDICES = dict(index_qv=0, index_qc=1, index_qr=2, index_qi=3, index_qs=4, index_qg=5, index_ni=6)  # 0-based
# name -> (pbl, convection, lw, sw, calls, index_qi absent).  cu_tiedtke_twice: the PBL is off, so tend_u_phys
# accumulates over its two calls.  bl_ysu_no_qi: the reference side runs with rqiblten = 0 and a valid index.
FIXTURE_SETS = {
    "off": (None, None, False, False, 1, False),
    "bl_ysu": ("bl_ysu", None, False, False, 1, False),
    "bl_mynn_cu_ntiedtke_lw_sw": ("bl_mynn", "cu_ntiedtke", True, True, 1, False),
    "cu_kain_fritsch": (None, "cu_kain_fritsch", False, False, 1, False),
    "cu_tiedtke_twice": (None, "cu_tiedtke", False, False, 2, False),
    "cu_grell_freitas_lw": (None, "cu_grell_freitas", True, False, 1, False),
    "lw": (None, None, True, False, 1, False),
    "sw": (None, None, False, True, 1, False),
    "bl_ysu_no_qi": ("bl_ysu", None, False, False, 1, True),
}
FIXTURE_OUTPUTS = ("tend_ru_physics", "tend_rtheta_physics", "tend_rho_physics", "scalars_tend", "rublten_Edge",
                   "rucuten_Edge", "tend_u_phys")
FIXTURE_STATE = ("rho_zz", "rho_edge", "theta_m", "scalars")
FIXTURE_MESH = ("cellsOnEdge", "east", "north", "edgeNormalVectors", "latCell", "lonCell")


def same_bits(a, b) -> bool:
    """Equal as 64-bit patterns (so -0.0 is not 0.0, and a NaN equals itself)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


def fixture_mesh() -> dict:
    """The fixture's mesh with the vectors the projection reads."""
    from .mesh import build_mesh
    from .reconstruct import initialize_vectors
    m = build_mesh(FIXTURE_MESH_LEVEL, lloyd_iters=20)
    m["east"], m["north"] = init_dirs(m["latCell"], m["lonCell"])
    m["edgeNormalVectors"] = initialize_vectors(m)["edgeNormalVectors"]
    return m


def fixture_set(name: str) -> tuple:
    """(flags, 0-based indices, calls) of a scheme set of the fixture."""
    pbl, cu, lw, sw, calls, no_qi = FIXTURE_SETS[name]
    idx = dict(FIXTURE_INDICES)
    if no_qi:
        idx["index_qi"] = -1
    return scheme_flags(pbl, cu, lw, sw), idx, calls


def fixture_run(name: str, raw: dict, state: dict, mesh: dict, get_tend=None) -> dict:
    """A scheme set's call(s) through ``get_tend`` (default: physics_get_tend), tend_u_phys carried from
    call to call from zero."""
    flags, idx, calls = fixture_set(name)
    out, tup = None, None
    for _ in range(calls):
        out = (get_tend or physics_get_tend)(flags, idx, raw, state["rho_zz"], state["rho_edge"], state["theta_m"],
                                             state["scalars"], mesh, tup)
        tup = out["tend_u_phys"]
    return out


# Restatements with one association changed: what the fixture must tell apart (the generator asserts the share
# of elements that differ from the reference, tests/test_todynamics_host.py re-checks it).
MIN_SENSITIVE_SHARE = 0.10


def variant_theta_m_right(flags, idx, raw, rho_zz, rho_edge, theta_m, scalars, mesh, tup=None) -> dict:
    """:429 with the second term associated from the right: R_v/R_d * (theta_m * (tend_qv / coeff))."""
    o = physics_get_tend(flags, idx, raw, rho_zz, rho_edge, theta_m, scalars, mesh, tup)
    iqv = idx["index_qv"]
    th = _tend_th(flags, raw, rho_zz)
    coeff = (1. + RVORD * np.asarray(scalars)[:, :, iqv])
    o["tend_rtheta_physics"] = 0.0 + (coeff * th + RVORD * (np.asarray(theta_m) * (o["scalars_tend"][:, :, iqv] / coeff)))
    return o


def variant_theta_sum_first(flags, idx, raw, rho_zz, rho_edge, theta_m, scalars, mesh, tup=None) -> dict:
    """The theta tendencies summed before the mass weighting: (rthblten + rthcuten + ...) * mass."""
    o = physics_get_tend(flags, idx, raw, rho_zz, rho_edge, theta_m, scalars, mesh, tup)
    iqv = idx["index_qv"]
    th = _tend_th(flags, raw, rho_zz, sum_first=True)
    coeff = (1. + RVORD * np.asarray(scalars)[:, :, iqv])
    o["tend_rtheta_physics"] = 0.0 + (coeff * th + RVORD * np.asarray(theta_m) * o["scalars_tend"][:, :, iqv] / coeff)
    return o


def variant_dot_right(flags, idx, raw, rho_zz, rho_edge, theta_m, scalars, mesh, tup=None) -> dict:
    """tend_toEdges with each dot product associated from the right: n1 e1 + (n2 e2 + n3 e3)."""
    m = dict(mesh)
    m["_dot_right"] = True
    return physics_get_tend(flags, idx, raw, rho_zz, rho_edge, theta_m, scalars, m, tup)


def _tend_th(flags, raw, rho_zz, sum_first=False):
    names = [n for f, n in ((PBL, "rthblten"), (CU, "rthcuten"), (LW, "rthratenlw"), (SW, "rthratensw")) if flags & f]
    mass = np.asarray(rho_zz, dtype=np.float64)
    th = np.zeros(mass.shape)
    if sum_first:
        for n in names:
            th = th + np.asarray(raw[n])
        return th * mass
    for n in names:
        th = th + np.asarray(raw[n]) * mass
    return th

"""Synthetic benchmark / test cases of BASELINE.json (SURVEY.md §8d "Synthetic inputs").

x1.N quasi-uniform icosahedral meshes with the JW baroclinic-wave state; dt and
config_len_disp scale with resolution as SURVEY.md §8d lists them:
2562 -> 2880 s / 480 km, 10242 -> 1440 s / 240 km, 163842 -> 360 s / 60 km.
Cases are cached as pickle files (they take tens of seconds to build at 163842) under
$MPAS_DYCORE_CACHE, by default the user's cache directory ($XDG_CACHE_HOME or ~/.cache, mpas_dycore):
what the build puts there (the benchmark's case) is still there when the benchmark runs.
"""
from __future__ import annotations

import os
import pickle
import sys

import numpy as np

from .init_atm import build_case
from .mesh import build_mesh, build_varres_mesh

CACHE = os.environ.get("MPAS_DYCORE_CACHE") or os.path.join(
    os.environ.get("XDG_CACHE_HOME") or os.path.join(os.path.expanduser("~"), ".cache"), "mpas_dycore")

LEVEL_OF = {162: 2, 642: 3, 2562: 4, 10242: 5, 40962: 6, 163842: 7, 655362: 8}

# the last mesh built in this process: the dry and moist cases of one resolution share it
_MESH_MEMO: dict = {}


def _mesh(level: int, lloyd_iters: int) -> dict:
    key = (level, lloyd_iters)
    if key not in _MESH_MEMO:
        _MESH_MEMO.clear()
        _MESH_MEMO[key] = build_mesh(level, lloyd_iters=lloyd_iters)
    return _MESH_MEMO[key]


def level_for(ncells: int) -> int:
    return LEVEL_OF[ncells]


def jw_dt(level: int) -> float:
    return 360.0 * 2 ** (7 - level)


def jw_len_disp(level: int) -> float:
    return 60000.0 * 2 ** (7 - level)


def jw_case(ncells: int, K: int = 56, ns: int = 1, moist: bool = False, order: int = 2,
            lloyd_iters: int = 20, cache: bool = True) -> dict:
    level = level_for(ncells)
    key = f"jw_l{level}_K{K}_ns{ns}_m{int(moist)}_o{order}_ll{lloyd_iters}_v6"
    path = os.path.join(CACHE, key + ".pkl")
    if cache and os.path.isfile(path):
        with open(path, "rb") as f:  # our own cache file, written below
            return pickle.load(f)
    m = _mesh(level, lloyd_iters)
    cfg = dict(config_len_disp=jw_len_disp(level), config_dt=jw_dt(level), config_time_integration_order=order)
    case = build_case(m, K=K, ns=ns, moist=moist, config=cfg)
    case["dt"] = jw_dt(level)
    if cache:
        os.makedirs(CACHE, exist_ok=True)
        tmp = path + f".{os.getpid()}.tmp"
        with open(tmp, "wb") as f:
            pickle.dump(case, f, protocol=pickle.HIGHEST_PROTOCOL)
        os.replace(tmp, path)
    return case


def varres_case(ncells: int, ratio: float = 20.0, K: int = 56, ns: int = 1, moist: bool = False,
                lloyd_iters: int | None = None, cache: bool = True, order: int = 2) -> dict:
    """JW state on a variable-resolution SCVT (BASELINE.json configs[4]).

    ncells = 835586 with ratio 20: the 60-3 km mesh of configs[4] from its stored generators
    (mesh.varres_from_generators, Lloyd-relaxed offline by tools/make_varres_mesh.py); other sizes
    are generated here (mesh.build_varres_mesh).  dt and config_len_disp follow the finest spacing,
    as MPAS variable-resolution runs do (dt ~ 5 s per km of the finest cells, len_disp = finest
    spacing); ``order`` = config_time_integration_order (3 for the BASELINE runs)."""
    from .mesh import X20_835586, varres_from_generators
    stored = ncells == 835586 and ratio == 20.0 and os.path.isfile(X20_835586)
    if lloyd_iters is None:
        lloyd_iters = 40 if ncells <= 200000 else 6
    key = (f"vr_x20.835586_K{K}_ns{ns}_m{int(moist)}_o{order}_v7" if stored else
           f"vr_n{ncells}_r{ratio:g}_K{K}_ns{ns}_m{int(moist)}_ll{lloyd_iters}_o{order}_v6")
    path = os.path.join(CACHE, key + ".pkl")
    if cache and os.path.isfile(path):
        with open(path, "rb") as f:  # our own cache file, written below
            return pickle.load(f)
    m = varres_from_generators(X20_835586) if stored else build_varres_mesh(ncells, ratio=ratio,
                                                                               lloyd_iters=lloyd_iters)
    dx_min = float(m["dcEdge"].min())
    dt = float(max(1.0, round(5.0 * dx_min / 1000.0)))
    cfg = dict(config_len_disp=dx_min, config_dt=dt, config_time_integration_order=order)
    if ncells > 200000:
        print(f"varres case: mesh done ({m['nCells']} cells), building the JW state", file=sys.__stderr__, flush=True)
    case = build_case(m, K=K, ns=ns, moist=moist, config=cfg)
    case["dt"] = dt
    if cache and ncells <= 400000:  # larger cases are rebuilt rather than pickled to /tmp
        os.makedirs(CACHE, exist_ok=True)
        tmp = path + f".{os.getpid()}.tmp"
        with open(tmp, "wb") as f:
            pickle.dump(case, f, protocol=pickle.HIGHEST_PROTOCOL)
        os.replace(tmp, path)
    return case


STRESS_DT = 2880.0


def stress_case(K: int, ns: int = 3, **config) -> dict:
    """The moist JW state on x1.642 with tracers and a mixing coefficient that load the paths the
    smooth case barely takes.  config_smagorinsky_coef = 1 puts most of kdiff at its cap
    (0.01 len_disp^2 / dt); the tracer species are discontinuous, so the monotone limiter rescales
    fluxes by factors well below 1 and the unlimited scheme undershoots zero:
      species 1 (and 3, ns = 6): a top-hat, 1e-3 (5e-4) within 0.6 rad of (1, 0, 0) ((0, 1, 0)) on
        the levels (3K)//20 .. (11K)//20, exactly 0 elsewhere;
      species 2 (and 4): 1e-3 r1 (r2 > 0.5), r1 and r2 uniform noise (seed 7, 8): half the entries 0;
      species 5: identically 0.
    qv (species 0) stays the JW moisture.  ``config`` overrides namelist options; it goes through
    build_case, since model_init folds config_coef_3rd_order into adv_coefs_3rd and zb3_cell.
    Meant to run with moist_end = ns and dt = case["dt"] = 2880 s, the step the x1.642 parity tests
    take (half of jw_dt(3); the step is an argument of atm_timestep, config_dt is not read)."""
    if ns not in (3, 6):
        raise ValueError(f"stress_case: ns = {ns}, the species are defined for 3 and 6")
    level = 3
    m = _mesh(level, 20)
    cfg = dict(config_len_disp=jw_len_disp(level), config_dt=jw_dt(level), config_time_integration_order=2,
               config_smagorinsky_coef=1.0)
    cfg.update(config)
    case = build_case(m, K=K, ns=ns, moist=True, config=cfg)
    case["dt"] = STRESS_DT
    nC = case["nCells"]
    shape = np.asarray(case["scalars"]).shape
    sc = np.array(case["scalars"], dtype=np.float64).reshape(nC, K, ns)
    xyz = np.stack([np.asarray(case["xCell"]), np.asarray(case["yCell"]), np.asarray(case["zCell"])], 1)
    xyz = xyz / np.sqrt((xyz ** 2).sum(1))[:, None]
    kk = np.arange(K)
    levels = (kk >= (3 * K) // 20) & (kk <= (11 * K) // 20)

    def top_hat(centre, amplitude):
        ang = np.arccos(np.clip(xyz @ np.asarray(centre, dtype=np.float64), -1.0, 1.0))
        return np.where((ang < 0.6)[:, None] & levels[None, :], amplitude, 0.0)

    def noise(seed):
        rng = np.random.default_rng(seed)
        r1 = rng.random((nC, K))
        r2 = rng.random((nC, K))
        return 1e-3 * r1 * (r2 > 0.5)

    sc[:, :, 1] = top_hat((1.0, 0.0, 0.0), 1e-3)
    sc[:, :, 2] = noise(7)
    if ns == 6:
        sc[:, :, 3] = top_hat((0.0, 1.0, 0.0), 5e-4)
        sc[:, :, 4] = noise(8)
        sc[:, :, 5] = 0.0
    case["scalars"] = sc.reshape(shape)
    return case


def regional_lbc(case: dict,interior_deg: float = 40.0, interval_end: float = 10800.0) -> tuple[dict, dict]:
    """A limited-area configuration on a global case (config_apply_lbcs): the cells farther than
    ``interior_deg`` from (0N, 0E) form the boundary zones, ring by ring outward -- bdyMaskCell 1..5
    relaxation, 6 and 7 (and everything beyond) specified -- as a regional mesh's masks count them
    (mpas_atm_boundaries.F:10-12).  Edges take the smaller mask of their two cells.  Also sets
    specZoneMask* and nearestRelaxationCell as mpas_atm_setup_bdy_masks does (:426-495; here every
    specified cell gets its nearest relaxation cell of mask 5, so no read falls outside the mesh)
    and meshScalingRegional* as atm_compute_mesh_scaling (mpas_atm_core.F:967-981).  Returns the
    case with these fields and the driving data of the lbc pool: lbc_<f>_s (interval-end state) and
    lbc_<f>_t (tendency) for u, ru, rho_zz, rtheta_m and scalars, element-major, plus
    ``interval_end`` = seconds from the first step's start to the LBC interval end."""
    import numpy as np
    from .init_atm import _pow
    c = dict(case)
    nC, nE = c["nCells"], c["nEdges"]
    lat, lon = np.asarray(c["latCell"]), np.asarray(c["lonCell"])
    ang = np.degrees(np.arccos(np.clip(np.cos(lat) * np.cos(lon), -1.0, 1.0)))
    mask = np.full(nC, 99, dtype=np.int64)
    mask[ang < interior_deg] = 0
    coc, noc = np.asarray(c["cellsOnCell"]), np.asarray(c["nEdgesOnCell"])
    ring = np.flatnonzero(mask == 0)
    for r in range(1, 8):
        nb = coc[ring]
        nb = nb[np.arange(coc.shape[1])[None, :] < noc[ring][:, None]]
        nb = np.unique(nb[nb >= 0])
        ring = nb[mask[nb] == 99]
        mask[ring] = r
    mask[mask == 99] = 7
    coe = np.asarray(c["cellsOnEdge"])
    emask = np.minimum(mask[coe[:, 0]], mask[coe[:, 1]])
    c["bdyMaskCell"] = mask.astype(np.int32)
    c["bdyMaskEdge"] = emask.astype(np.int32)
    c["specZoneMaskCell"] = (mask > 5).astype(np.float64)
    c["specZoneMaskEdge"] = (emask > 5).astype(np.float64)
    xyz = np.stack([np.asarray(c["xCell"]), np.asarray(c["yCell"]), np.asarray(c["zCell"])], 1)
    relax = np.flatnonzero(mask == 5)
    near = np.full(nC, -1, dtype=np.int64)
    for i in np.flatnonzero(mask > 5):
        d2 = ((xyz[relax] - xyz[i]) ** 2).sum(1)
        near[i] = relax[np.argmin(d2)]
    c["nearestRelaxationCell"] = near
    md = np.asarray(c.get("meshDensity", np.ones(nC)), dtype=np.float64)
    c["meshScalingRegionalCell"] = 1.0 / _pow(md, 0.25)
    c["meshScalingRegionalEdge"] = 1.0 / _pow((md[coe[:, 0]] + md[coe[:, 1]]) / 2.0, 0.25)
    # driving data: the initial state with a smooth perturbation at the interval end, and the
    # tendency that leads there
    K, ns = c["nVertLevels"], c["num_scalars"]
    zz = np.asarray(c["zz"])
    rho_zz = np.asarray(c["rho"]) / zz
    sc = np.asarray(c["scalars"]).reshape(nC, K, ns)
    theta_m = np.asarray(c["theta"]) * (1.0 + 461.6 / 287.0 * sc[:, :, 0])
    u = np.asarray(c["u"])
    ru = u * 0.5 * (rho_zz[coe[:, 0]] + rho_zz[coe[:, 1]])
    lonE, latE = np.asarray(c["lonEdge"]), np.asarray(c["latEdge"])
    pc, pe = 0.003 * np.cos(lon)[:, None], 0.003 * np.cos(lonE)[:, None]
    tc, te = 1e-7 * np.sin(lat)[:, None], 1e-7 * np.sin(latE)[:, None]
    lbc = {"interval_end": float(interval_end)}
    for name, base, p_, t_ in (("u", u, pe, te), ("ru", ru, pe, te), ("rho_zz", rho_zz, pc, tc),
                               ("rtheta_m", rho_zz * theta_m, pc, tc)):
        lbc[f"lbc_{name}_s"] = base * (1.0 + p_)
        lbc[f"lbc_{name}_t"] = base * t_
    lbc["lbc_scalars_s"] = sc * (1.0 + 3.0 * pc[:, :, None])
    lbc["lbc_scalars_t"] = sc * tc[:, :, None]
    return c, lbc


def seed_cloud_and_rain(case: dict) -> dict:
    """A copy of a moist case of ns >= 3 (qv, qc, qr) with cloud and rain seeded in the lower
    troposphere of every tenth cell: what makes the Kessler scheme's data-dependent sedimentation loop
    run in a few steps of the JW state."""
    case = dict(case)
    n, K, ns = case["nCells"], case["nVertLevels"], case["num_scalars"]
    sc = np.array(case["scalars"], dtype=np.float64).reshape(n, K, ns)
    kk = np.arange(K)[None, :]
    patch = (np.arange(n) % 10 == 0)[:, None]
    sc[:, :, 1] = np.where(patch & (kk >= 2) & (kk < 10), 1.0e-3, 0.0)
    sc[:, :, 2] = np.where(patch & (kk >= 1) & (kk < 8), 2.0e-3 * (1.0 + np.sin(np.arange(n)))[:, None], 0.0)
    case["scalars"] = sc.reshape(np.asarray(case["scalars"]).shape)
    return case


def reference_nearest(case: dict) -> np.ndarray:
    """nearestRelaxationCell as mpas_atm_setup_bdy_masks computes it (:466-518; 0-based, -1 = none):
    the nearest mask-5 cell among the neighbours, for row 7 through a row-6 neighbour, so every index
    lies within two cells of its cell and therefore inside the halo of a block that owns the cell."""
    mask = np.asarray(case["bdyMaskCell"])
    coc, noc = np.asarray(case["cellsOnCell"]), np.asarray(case["nEdgesOnCell"])
    xyz = np.stack([np.asarray(case["xCell"]), np.asarray(case["yCell"]), np.asarray(case["zCell"])], 1)
    near = np.full(case["nCells"], -1, dtype=np.int64)
    for c in np.flatnonzero(mask == 6):
        best = 1.0e36
        for i in coc[c, :noc[c]]:
            if mask[i] == 5:
                d = ((xyz[i] - xyz[c]) ** 2).sum()
                if d < best:
                    best, near[c] = d, i
    for c in np.flatnonzero(mask == 7):
        best = 1.0e36
        for i in coc[c, :noc[c]]:
            if mask[i] != 6:
                continue
            for ii in coc[i, :noc[i]]:
                if mask[ii] == 5:
                    d = ((xyz[ii] - xyz[c]) ** 2).sum()
                    if d < best:
                        best, near[c] = d, ii
    return near


def iau_increments(case: dict) -> dict:
    """Smooth analysis increments of both signs over every element and level: u_amb ~ 1 m/s,
    theta_amb ~ 1 K, rho_amb ~ 1e-2, q*_amb ~ 1e-4.  rho_amb has that size where the air is densest and
    falls off with the base-state density above, as an analysis increment of density does: 1e-2 at the
    model top, where rho is a few 1e-2, would halve or double the density within the window, and the
    run (with IAU on the device or with the host's sums alike) leaves the range of the model."""
    K, ns = case["nVertLevels"], case["num_scalars"]
    kk = ((np.arange(K) + 0.5) / K)[None, :]
    latc, lonc = case["latCell"][:, None], case["lonCell"][:, None]
    late, lone = case["latEdge"][:, None], case["lonEdge"][:, None]
    sc = np.zeros((case["nCells"], K, ns))
    for i in range(ns):
        sc[:, :, i] = 1e-4 * np.sin((i + 2) * lonc + i) * np.cos(latc) * np.cos(np.pi * (i + 1) * kk)
    rb = case["rho_base"] / np.max(case["rho_base"])
    return dict(u_amb=np.cos(late) * np.sin(2 * lone + 0.3) * np.cos(np.pi * kk) + 0.25 * np.sin(3 * late),
                theta_amb=np.sin(2 * latc) * np.cos(lonc) * (1.0 - 2.0 * kk) + 0.3 * np.sin(3 * lonc),
                rho_amb=1e-2 * rb * np.cos(latc) * np.sin(lonc - 0.7) * np.cos(2 * np.pi * kk), scalars_amb=sc)


def physics_forcing(case: dict, scale: float = 1.0) -> dict:
    """Smooth prescribed physics tendencies (what physics_get_tend hands the dycore,
    mpas_atm_time_integration.F:424-449): coupled momentum / theta / density tendencies and scalar
    tendencies of typical magnitude, element-major; the water-vapour tendency is negative aloft so that
    the clip of negative mixing ratios (1642-1644) is exercised.  The suite's forcing:
    tests/test_forecast_case.py holds this to the test helper of the same name bit for bit."""
    K, ns = case["nVertLevels"], case["num_scalars"]
    kk = (np.arange(K) + 0.5) / K
    latc, lonc = case["latCell"][:, None], case["lonCell"][:, None]
    late, lone = case["latEdge"][:, None], case["lonEdge"][:, None]
    f = dict(
        tend_ru_physics=scale * 2e-4 * np.cos(late) * np.sin(2 * lone) * (1 - kk),
        tend_rtheta_physics=scale * 3e-4 * np.cos(latc) ** 2 * np.exp(-3 * kk) * (1 + 0.5 * np.sin(lonc)),
        tend_rho_physics=scale * 1e-7 * np.sin(latc) * np.cos(lonc) * (1 - kk),
    )
    st = np.zeros((case["nCells"], K, ns))
    for i in range(ns):
        st[:, :, i] = scale * 1e-7 * np.cos((i + 1) * latc) * np.sin(lonc + i) * (1 - kk) ** (i + 1)
    st[:, :, 0] -= scale * 5e-7 * kk ** 2
    f["scalars_tend"] = st
    return f


def raw_physics_forcing(case: dict, scale: float = 1.0) -> dict:
    """Smooth raw tendencies of the PBL, convection and radiation schemes (the tend_physics pool that
    physics_get_tend couples: rublten ... rthratensw, fields.TODYN_RAW), element-major (nCells, K).  They are
    physics_forcing's coupled tendencies split between the schemes and divided by the case's rho_zz, so
    what physics_get_tend makes of them on the initial state has physics_forcing's size -- its drying aloft
    included -- and both signs; every field has its own pattern, so a swapped pair shows."""
    K = case["nVertLevels"]
    kk = (np.arange(K) + 0.5) / K
    latc, lonc = case["latCell"][:, None], case["lonCell"][:, None]
    rho = np.asarray(case["rho"], dtype=np.float64) / np.asarray(case["zz"], dtype=np.float64)
    wave = lambda i: np.cos((i + 1) * latc) * np.sin(lonc + i) * (1 - kk) ** (i % 3 + 1)  # noqa: E731
    th = 3e-4 * np.cos(latc) ** 2 * np.exp(-3 * kk)
    f = dict(
        rublten=2e-4 * np.cos(latc) * np.sin(2 * lonc) * (1 - kk), rvblten=1.5e-4 * np.sin(2 * latc) * np.cos(lonc) * (1 - kk),
        rucuten=1e-4 * np.cos(latc) * np.cos(3 * lonc + 0.4) * kk * (1 - kk), rvcuten=8e-5 * np.sin(latc) * np.sin(lonc - 0.3) * kk,
        rthblten=0.4 * th * (1 + 0.5 * np.sin(lonc)), rthcuten=0.3 * th * (1 + 0.5 * np.cos(2 * lonc)) * 4 * kk * (1 - kk),
        rthratenlw=-0.2 * th * (1 + 0.3 * np.sin(latc)), rthratensw=0.3 * th * np.maximum(np.cos(lonc), 0.0),
        rqvblten=0.6e-7 * wave(0) - 5e-7 * kk ** 2, rqvcuten=0.4e-7 * wave(1),
        rqcblten=1e-8 * wave(2), rqccuten=2e-8 * wave(3), rqiblten=0.5e-8 * wave(4), rqicuten=1e-8 * wave(5),
        rqrcuten=1.5e-8 * wave(6), rqscuten=1e-8 * wave(7), rniblten=1e2 * wave(8),
    )
    return {n: scale * a / rho for n, a in f.items()}


FORECAST_DT = 600.0
FORECAST_NS = 3


def forecast_case(K: int) -> tuple[dict, dict, dict, dict]:
    """A regional forecast with every optional part of the step in play, on x1.642 with qv, qc, qr
    (moist_end = 3) and a step of case["dt"] = 600 s: (case, lbc, increments, physics).
      case: the moist JW state with cloud and rain seeded (seed_cloud_and_rain), made limited-area by
        regional_lbc(interior_deg = 120) -- applied after the seeding, so the driving scalars hold qc
        and qr -- with nearestRelaxationCell as the reference computes it (reference_nearest), so the
        case can be decomposed.  Every zone is populated: bdyMaskCell 1..7 holds 40 / 34 / 30 / 26 / 18 /
        12 / 3 cells around 479 interior ones;
      lbc: regional_lbc's driving data;
      increments: iau_increments, and "window" = 2.5 dt: three forced steps, then free ones;
      physics: physics_forcing(case, 0.1), which keeps a run with IAU inside the model's range.
    Meant to run with the physics forcing and IAU together when the Kessler scheme is on: the JW column
    reaches 45 km, and on its top levels (the top three of 26) the saturation vapour pressure of the initial
    state exceeds the pressure, where the scheme's qvs = ep_2 es / (p - es) turns negative and its
    saturation adjustment heats without bound.  The forcing's drying aloft times Rv/Rd theta in IAU's
    theta_m tendency cools those levels enough to keep es at or below p; with either left out the top
    level's theta_m passes 8000 K within four steps (tests/test_gpu_forecast.py::test_each_hook_acts)."""
    case = seed_cloud_and_rain(jw_case(642, K, ns=FORECAST_NS, moist=True, cache=False))
    case, lbc = regional_lbc(case, interior_deg=120.0)
    case["nearestRelaxationCell"] = reference_nearest(case)
    case["dt"] = FORECAST_DT
    inc = iau_increments(case)
    inc["window"] = 2.5 * FORECAST_DT
    return case, lbc, inc, physics_forcing(case, 0.1)

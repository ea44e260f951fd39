"""Host restatement of the isobaric output diagnostics (csrc/isobaric.hip, mpas_dyc_isobaric_diagnostics).

interp_diagnostics of the reference (core_atmosphere/diagnostics/isobaric_diagnostics.F:265-895) with its
array routines interp_tofixed_pressure (:899-985), compute_slp (:988-1121) and compute_layer_mean
(:1139-1245), in numpy, fp64, every + - * / in the Fortran's order.  ``log`` / ``exp`` / ``pow`` are the C
library's (csrc/host_libm.c, as mpas_dycore.kessler and init_atm call it), so the restatement has the
compiled reference's bits when the helper is built (tests/test_isobaric_host.py checks it against
tests/golden/isobaric_columns.npz).  It is the yardstick of the device kernel on states the fixture does
not cover, and it reports per column and output which branch was taken and the margins of every
comparison whose operand passed through a transcendental function.

Arrays are element-major in model order: ``(n, K)`` mass levels and ``(n, K + 1)`` interfaces, level 1
(the ground) first, so pressure decreases with the index; the Fortran reverses its copies so that
pressure increases with the index, and "the level above" here is its ``kk``, the level itself its
``kk + 1``.

interp_tofixed_pressure is restated per column (``interp``), which is what it does for strictly monotone
columns; ``interp_reference_loops`` is the loop transcription with its kupper / kount bookkeeping.
"""
from __future__ import annotations

import math

import numpy as np

from . import init_atm as _ia

# MPAS_DYC_ISO_*
TEMPERATURE, RELHUM, DEWPOINT, UZONAL, UMERIDIONAL, HEIGHT, W, VORTICITY = 1, 2, 4, 8, 16, 32, 64, 128
MSLP, T_ISOBARIC, Z_ISOBARIC, MEANT_500_300 = 256, 512, 1024, 2048
ALL = 4095
GROUPS = ("temperature", "relhum", "dewpoint", "uzonal", "umeridional", "height", "w", "vorticity")
HPA = (200, 250, 500, 700, 850, 925)
T_ISO_LEVELS = tuple(30000.0 + 5000.0 * i for i in range(5))
Z_ISO_LEVELS = tuple(30000.0 + 5000.0 * i for i in range(13))
RVORD = 461.6 / 287.0
# compute_slp's parameters (:1011-1015)
SLP_GAMMA, SLP_RR, SLP_GRAV, SLP_TC, SLP_PCONST = 0.0065, 287.0, 9.80616, 273.16 + 17.5, 100.0
# branches of interp(): a bracket inside the column, the target above the column's top, below the
# ground, equal to the top level's pressure
INTERIOR, ABOVE_TOP, BELOW_GROUND, EQUAL_TOP = 0, 1, 2, 3
# branches of layer_mean(): the layer meets the column's top or bottom; inside one model layer; general
LM_BOUNDARY, LM_SINGLE, LM_GENERAL = 0, 1, 2
# outcomes of compute_slp's mm5_test: t_msl = tc; the else branch because t_msl < tc; because t_surf > tc
MM5_TC, MM5_ELSE_COLD, MM5_ELSE_HOT = 0, 1, 2


def field_name(group: int, level: int) -> str:
    return f"{GROUPS[group]}_{HPA[level]}hPa"


CELL_FIELDS = tuple(field_name(g, l) for g in range(7) for l in range(6)) + ("mslp", "meanT_500_300", "t_isobaric",
                                                                            "z_isobaric")
VERTEX_FIELDS = tuple(field_name(7, l) for l in range(6))


def group_fields(flag: int) -> tuple:
    """The diag fields one MPAS_DYC_ISO_* bit writes."""
    if flag <= VORTICITY:
        g = flag.bit_length() - 1
        return tuple(field_name(g, l) for l in range(6))
    return {MSLP: ("mslp",), T_ISOBARIC: ("t_isobaric",), Z_ISOBARIC: ("z_isobaric",),
            MEANT_500_300: ("meanT_500_300",)}[flag]


_LIBM_LOG = np.frompyfunc(math.log, 1, 1)
_HOST_LOG = None
if _ia._HOST is not None:
    try:
        import ctypes as _C
        _ia._HOST.hl_log.argtypes = [_C.c_void_p, _C.c_void_p, _C.c_int64]
        _HOST_LOG = _ia._HOST.hl_log
    except AttributeError:  # a stale build of the helper: math.log, the same C library one call at a time
        _HOST_LOG = None


def host_libm_loaded() -> bool:
    return _ia.host_libm_loaded()


def _log(x):
    if _HOST_LOG is not None:
        return _ia._host1(_HOST_LOG, x)
    return np.asarray(_LIBM_LOG(np.asarray(x, dtype=np.float64)), dtype=np.float64)


def _exp(x):
    return _ia._exp(x)


def _pow(x, y: float):
    x = np.ascontiguousarray(x, dtype=np.float64)
    if _ia._HOST is not None:
        out = np.empty_like(x)
        _ia._HOST.hl_pow_s(x.ctypes.data, float(y), out.ctypes.data, x.size)
        return out
    return np.asarray(_ia._LIBM_POW(x, float(y)), dtype=np.float64)


# ------------------------------------------------------------------------------------------ pressures
def pressure(pressure_p, pressure_base):
    """pressure(k) in hPa (:506)."""
    return (np.asarray(pressure_p, dtype=np.float64) + np.asarray(pressure_base, dtype=np.float64)) / 100.0


def pressure2(p, zgrid):
    """Pressure at the K + 1 interfaces (:517-542); only the top one goes through exp / log."""
    z = np.asarray(zgrid, dtype=np.float64)
    n, K = p.shape
    out = np.empty((n, K + 1))
    k = K
    z0, z1, z2 = z[:, k], 0.5 * (z[:, k] + z[:, k - 1]), 0.5 * (z[:, k - 1] + z[:, k - 2])
    w1 = (z0 - z2) / (z1 - z2)
    w2 = 1. - w1
    out[:, k] = _exp(w1 * _log(p[:, k - 1]) + w2 * _log(p[:, k - 2]))
    w1 = (z[:, 1:K] - z[:, 0:K - 1]) / (z[:, 2:K + 1] - z[:, 0:K - 1])
    w2 = (z[:, 2:K + 1] - z[:, 1:K]) / (z[:, 2:K + 1] - z[:, 0:K - 1])
    out[:, 1:K] = w1 * p[:, 1:K] + w2 * p[:, 0:K - 1]
    z0, z1, z2 = z[:, 0], 0.5 * (z[:, 0] + z[:, 1]), 0.5 * (z[:, 1] + z[:, 2])
    w1 = (z0 - z2) / (z1 - z2)
    w2 = 1. - w1
    out[:, 0] = w1 * p[:, 0] + w2 * p[:, 1]
    return out


def pressure_v(p_img, cellsOnVertex, kiteAreasOnVertex, areaTriangle):
    """Pressure at the vertices (:545-555).  p_img: pressure of every cell and of the garbage slot,
    (nCells + 1, K); cellsOnVertex 0-based, the garbage cell = nCells."""
    cov = np.asarray(cellsOnVertex)
    kite = np.asarray(kiteAreasOnVertex, dtype=np.float64)
    pv = np.zeros((cov.shape[0], p_img.shape[1]))
    for j in range(3):
        pv = pv + kite[:, j:j + 1] * p_img[cov[:, j]]
    return pv / np.asarray(areaTriangle, dtype=np.float64)[:, None]


def thermo(p, theta_m, qv, exner):
    """temperature, dewpoint and whether the evp clamp was active (:561-569)."""
    temperature = (theta_m / (1.0 + RVORD * qv)) * exner
    evp0 = p * qv / (qv + 0.622)
    evp = np.maximum(evp0, 1.0e-8)
    lg = _log(evp / 6.112)
    dewpoint = (243.5 * lg) / (17.67 - lg)
    dewpoint = dewpoint + 273.15
    return temperature, dewpoint, evp0 < 1.0e-8


# ---------------------------------------------------------------------------- interp_tofixed_pressure
def interp(p, f, targets):
    """interp_tofixed_pressure per column.  p, f: (n, L) in model order; targets: the output pressures.
    Returns (out (n, nt), info): info["branch"] (n, nt) one of INTERIOR .. EQUAL_TOP, info["k"] the
    bracket's lower level (0-based; L - 2 for EQUAL_TOP, -1 otherwise), info["equal_lower"] p_out equals
    the bracket's lower level's pressure exactly, info["uses_top"] the result reads the top level's
    pressure."""
    p = np.asarray(p, dtype=np.float64)
    f = np.asarray(f, dtype=np.float64)
    n, L = p.shape
    rows = np.arange(n)
    out = np.empty((n, len(targets)))
    branch = np.empty((n, len(targets)), dtype=np.int8)
    kk = np.empty((n, len(targets)), dtype=np.int64)
    eq = np.zeros((n, len(targets)), dtype=bool)
    for t, po in enumerate(targets):
        hit = (p[:, 1:] < po) & (po <= p[:, :-1])
        has = hit.any(axis=1)
        k = np.where(has, hit.argmax(axis=1), L - 2)
        pk, pu, fk, fu = p[rows, k], p[rows, k + 1], f[rows, k], f[rows, k + 1]
        dpu = po - pu
        dpl = pk - po
        with np.errstate(all="ignore"):
            br = (fu * dpl + fk * dpu) / (dpl + dpu)
            top = f[:, -1] * po / p[:, -1]
        b = np.where(has, INTERIOR, np.where(po < p[:, -1], ABOVE_TOP, np.where(po > p[:, 0], BELOW_GROUND, EQUAL_TOP)))
        out[:, t] = np.select([b == INTERIOR, b == ABOVE_TOP, b == BELOW_GROUND], [br, top, f[:, 0]], br)
        branch[:, t] = b
        kk[:, t] = np.where((b == INTERIOR) | (b == EQUAL_TOP), k, -1)
        eq[:, t] = has & (po == pk)
    uses_top = (branch == ABOVE_TOP) | (branch == EQUAL_TOP) | ((branch == INTERIOR) & (kk == L - 2))
    return out, {"branch": branch, "k": kk, "equal_lower": eq, "uses_top": uses_top}


def interp_reference_loops(pres_in, field_in, pres_out):
    """interp_tofixed_pressure as the Fortran writes it (:932-983), loop for loop, with its kupper / kount
    bookkeeping over the whole batch.  pres_in, field_in: (ncol, nlev_in) with pressure increasing with
    the index (the routine's own order); pres_out: (ncol, nlev_out)."""
    ncol, nlev_in = pres_in.shape
    nlev_out = pres_out.shape[1]
    field_out = np.zeros((ncol, nlev_out))
    kupper = [1] * ncol
    for k in range(1, nlev_out + 1):
        kkstart = nlev_in
        for icol in range(ncol):
            kkstart = min(kkstart, kupper[icol])
        kount = 0
        done = False
        for kk in range(kkstart, nlev_in):
            for icol in range(ncol):
                if pres_out[icol, k - 1] > pres_in[icol, kk - 1] and pres_out[icol, k - 1] <= pres_in[icol, kk]:
                    kupper[icol] = kk
                    kount = kount + 1
            if kount == ncol:
                for icol in range(ncol):
                    ku = kupper[icol]
                    dpu = pres_out[icol, k - 1] - pres_in[icol, ku - 1]
                    dpl = pres_in[icol, ku] - pres_out[icol, k - 1]
                    field_out[icol, k - 1] = (field_in[icol, ku - 1] * dpl + field_in[icol, ku] * dpu) / (dpl + dpu)
                done = True
                break
        if done:
            continue
        for icol in range(ncol):
            po = pres_out[icol, k - 1]
            if po < pres_in[icol, 0]:
                field_out[icol, k - 1] = field_in[icol, 0] * po / pres_in[icol, 0]
            elif po > pres_in[icol, nlev_in - 1]:
                field_out[icol, k - 1] = field_in[icol, nlev_in - 1]
            else:
                ku = kupper[icol]
                dpu = po - pres_in[icol, ku - 1]
                dpl = pres_in[icol, ku] - po
                field_out[icol, k - 1] = (field_in[icol, ku - 1] * dpl + field_in[icol, ku] * dpu) / (dpl + dpu)
    return field_out


# --------------------------------------------------------------------------------- compute_layer_mean
def layer_mean(P, T, p1=50000.0, p2=30000.0):
    """compute_layer_mean (:1139-1245).  P (Pa), T: (n, K) in model order.  Returns (mean (n,), info):
    info["branch"] one of LM_BOUNDARY / LM_SINGLE / LM_GENERAL, info["middle"] the number of middle layers."""
    P = np.asarray(P, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    n, K = P.shape
    p_top, p_bot = (p1, p2) if p1 < p2 else (p2, p1)
    out = np.zeros(n)
    branch = np.zeros(n, dtype=np.int8)
    middle = np.zeros(n, dtype=np.int64)
    for i in range(n):
        # the Fortran's arrays: index kk = 1..K, pressure increasing
        pin, fin = P[i, ::-1], T[i, ::-1]
        k_bot = k_top = -1
        for k in range(K - 1):
            if pin[k] <= p_top and pin[k + 1] > p_top:
                k_top = k
                wtop_p = (p_top - pin[k]) / (pin[k + 1] - pin[k])
                wtop_m = (pin[k + 1] - p_top) / (pin[k + 1] - pin[k])
            if pin[k] <= p_bot and pin[k + 1] > p_bot:
                k_bot = k
                wbot_m = (p_bot - pin[k]) / (pin[k + 1] - pin[k])
                wbot_p = (pin[k + 1] - p_bot) / (pin[k + 1] - pin[k])
        if k_top == -1 or k_bot == -1:
            out[i] = 0.0
            branch[i] = LM_BOUNDARY
        elif k_top == k_bot:
            m = wtop_m * fin[k_top] + wtop_p * fin[k_top + 1]
            m = m + wbot_m * fin[k_bot] + wbot_p * fin[k_bot + 1]
            out[i] = 0.5 * m
            branch[i] = LM_SINGLE
        else:
            wtotal = pin[k_top + 1] - p_top
            temp = wtop_m * fin[k_top] + wtop_p * fin[k_top + 1]
            m = wtotal * 0.5 * (fin[k_top + 1] + temp)
            for k in range(k_top + 1, k_bot):
                w = pin[k + 1] - pin[k]
                wtotal = wtotal + w
                m = m + w * 0.5 * (fin[k] + fin[k + 1])
                middle[i] += 1
            w = p_bot - pin[k_bot]
            wtotal = wtotal + w
            temp = wbot_m * fin[k_bot] + wbot_p * fin[k_bot + 1]
            m = m + w * 0.5 * (fin[k_bot] + temp)
            out[i] = m / wtotal
            branch[i] = LM_GENERAL
    return out, {"branch": branch, "middle": middle}


# ---------------------------------------------------------------------------------------- compute_slp
def slp(p, t, zgrid, qv):
    """compute_slp (:988-1121) in hPa.  Returns (slp (n,), info): info["fail"] per column (no level
    100 hPa above the ground, or klo == khi) -- if any column fails, slp is 0.0 everywhere, as the
    reference returns it; info["mm5"] the outcome of the mm5_test; info["margin"] the least relative
    distance of t_msl and t_surf from tc."""
    p = np.asarray(p, dtype=np.float64)
    n, K = p.shape
    z = np.asarray(zgrid, dtype=np.float64)
    rows = np.arange(n)
    above = p < (p[:, 0] - SLP_PCONST)[:, None]
    found = above.any(axis=1)
    level = np.where(found, above.argmax(axis=1) + 1, -1)       # 1-based
    klo = np.maximum(level - 1, 1)
    khi = np.minimum(klo + 1, K - 1)
    fail = ~found | (klo == khi)
    klo0, khi0 = np.where(fail, 0, klo - 1), np.where(fail, 1, khi - 1)
    plo, phi = p[rows, klo0], p[rows, khi0]
    tlo = t[rows, klo0] * (1. + 0.608 * qv[rows, klo0])
    thi = t[rows, khi0] * (1. + 0.608 * qv[rows, khi0])
    zlo = 0.5 * (z[rows, klo0] + z[rows, klo0 + 1])
    zhi = 0.5 * (z[rows, khi0] + z[rows, khi0 + 1])
    with np.errstate(all="ignore"):
        p_at_pconst = p[:, 0] - SLP_PCONST
        arg1 = np.where(fail, 1.0, p_at_pconst / phi)
        arg2 = np.where(fail, 1.0, plo / phi)
        l1, l2 = _log(arg1), _log(arg2)
        t_at_pconst = thi - (thi - tlo) * l1 * l2
        z_at_pconst = zhi - (zhi - zlo) * l1 * l2
        t_surf = t_at_pconst * _pow(np.where(fail, 1.0, p[:, 0] / p_at_pconst), SLP_GAMMA * SLP_RR / SLP_GRAV)
        t_msl = t_at_pconst + SLP_GAMMA * z_at_pconst
        cold, cool_surface = t_msl < SLP_TC, t_surf <= SLP_TC
        mm5 = np.where(cool_surface & ~cold, MM5_TC, np.where(cold, MM5_ELSE_COLD, MM5_ELSE_HOT)).astype(np.int8)
        margin = np.minimum(np.abs(t_msl - SLP_TC), np.abs(t_surf - SLP_TC)) / SLP_TC
        t_msl = np.where(mm5 == MM5_TC, SLP_TC, SLP_TC - 0.005 * ((t_surf - SLP_TC) * (t_surf - SLP_TC)))
        z_half_lowest = 0.5 * (z[:, 0] + z[:, 1])
        out = p[:, 0] * _exp(np.where(fail, 0.0, (2. * SLP_GRAV * z_half_lowest) / (SLP_RR * (t_msl + t_surf))))
    if fail.any():
        out = np.zeros(n)
    return out, {"fail": fail, "mm5": mm5, "margin": np.where(fail, np.inf, margin), "level": level}


# ------------------------------------------------------------------------------------------ the whole
def cells(f: dict, flags: int = ALL) -> dict:
    """interp_diagnostics on cell columns.  f: pressure_p, pressure_base, theta_m, qv, exner, relhum,
    uzonal, umeridional (n, K) and zgrid, w (n, K + 1).  Returns the enabled diag fields by name
    ((n,), t_isobaric (n, 5), z_isobaric (n, 13)) and "info": per output group the interp() info
    ("mass", "iface", "t_isobaric", "z_isobaric"), "layer_mean", "slp", "evp_clamp" (n, K), and
    "top_margin": the least relative distance of pressure2(K + 1) from a target it is compared with."""
    g = {k: np.asarray(v, dtype=np.float64) for k, v in f.items()}
    p = pressure(g["pressure_p"], g["pressure_base"])
    out, info = {}, {}
    temperature, dewpoint, clamp = thermo(p, g["theta_m"], g["qv"], g["exner"])
    info["evp_clamp"] = clamp
    mass = ((TEMPERATURE, temperature), (RELHUM, g["relhum"]), (DEWPOINT, dewpoint), (UZONAL, g["uzonal"]),
            (UMERIDIONAL, g["umeridional"]))
    hpa = [float(x) for x in HPA]
    for gi, (bit, field) in enumerate(mass):
        if flags & bit:
            v, info["mass"] = interp(p, field, hpa)
            for l in range(6):
                out[field_name(gi, l)] = v[:, l]
    if flags & (HEIGHT | W | Z_ISOBARIC):
        p2 = pressure2(p, g["zgrid"])
        margins = []
        for gi, bit, field in ((5, HEIGHT, g["zgrid"]), (6, W, g["w"])):
            if flags & bit:
                v, info["iface"] = interp(p2, field, hpa)
                margins.append(np.min(np.abs(p2[:, -1:] - np.array(hpa)[None, :]) / np.array(hpa)[None, :], axis=1))
                for l in range(6):
                    out[field_name(gi, l)] = v[:, l]
        if flags & Z_ISOBARIC:
            lev = np.array(Z_ISO_LEVELS)
            out["z_isobaric"], info["z_isobaric"] = interp(p2 * 100.0, g["zgrid"], list(Z_ISO_LEVELS))
            margins.append(np.min(np.abs((p2[:, -1:] * 100.0) - lev[None, :]) / lev[None, :], axis=1))
        info["top_margin"] = np.min(np.stack(margins), axis=0)
    if flags & MSLP:
        s, info["slp"] = slp(p, temperature, g["zgrid"], g["qv"])
        out["mslp"] = s * 100.0
    if flags & T_ISOBARIC:
        out["t_isobaric"], info["t_isobaric"] = interp(p * 100.0, temperature, list(T_ISO_LEVELS))
    if flags & MEANT_500_300:
        out["meanT_500_300"], info["layer_mean"] = layer_mean(p * 100.0, temperature)
    out["info"] = info
    return out


def vertices(pressure_p_img, pressure_base_img, vorticity, cellsOnVertex, kiteAreasOnVertex, areaTriangle) -> dict:
    """vorticity_*hPa of the given vertices: pressure images with the garbage slot (nCells + 1, K),
    vorticity (nv, K), cellsOnVertex (nv, 3) 0-based with nCells for the garbage cell."""
    pv = pressure_v(pressure(pressure_p_img, pressure_base_img), cellsOnVertex, kiteAreasOnVertex, areaTriangle)
    v, info = interp(pv, vorticity, [float(x) for x in HPA])
    out = {field_name(7, l): v[:, l] for l in range(6)}
    out["info"] = {"vertex": info, "pressure_v": pv}
    return out


# --------------------------------------------------------------------------------------- the fixture
FIXTURE_CELL_IN = ("theta_m", "qv", "exner", "relhum", "uzonal", "umeridional", "zgrid", "w")


def fixture_columns(golden: dict, tag: str):
    """tests/golden/isobaric_columns.npz, one set ("K4" .. "K150", "fail"): (columns, reference outputs).
    columns: the cell inputs of cells() plus pressure_p_img / pressure_base_img (with the garbage slot),
    vorticity, cellsOnVertex (0-based, nCells = the garbage cell), kiteAreasOnVertex, areaTriangle."""
    c = {n: golden[f"{n}_{tag}"].astype(np.float64) for n in FIXTURE_CELL_IN + (
        "pressure_p_img", "pressure_base_img", "vorticity", "kiteAreasOnVertex", "areaTriangle")}
    c["pressure_p"], c["pressure_base"] = c["pressure_p_img"][:-1], c["pressure_base_img"][:-1]
    c["cellsOnVertex"] = golden[f"cellsOnVertex_{tag}"].astype(np.int64)
    ref = {n: golden[f"ref_{n}_{tag}"] for n in CELL_FIELDS + VERTEX_FIELDS}
    return c, ref


def fixture_cells(c: dict) -> dict:
    """The arguments of cells() out of fixture_columns()'s columns."""
    return {n: c[n] for n in FIXTURE_CELL_IN + ("pressure_p", "pressure_base")}

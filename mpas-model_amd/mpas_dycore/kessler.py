"""The Kessler microphysics of the time step in numpy: what ``Dycore.microphysics()`` computes on the device.

A restatement of driver_microphysics for config_microp_scheme = 'mp_kessler'
(physics/mpas_atmphys_driver_microphysics.F:237-425):

* ``from_mpas``        microphysics_from_MPAS (mpas_atmphys_interface.F:541-559)
* ``kessler``          physics_wrf/module_mp_kessler.F, with 8-byte REAL as the reference builds it
* ``precip_to_mpas``   precip_from_MPAS / precip_to_MPAS (mpas_atmphys_driver_microphysics.F:429-583)
* ``to_mpas``          microphysics_to_MPAS (mpas_atmphys_interface.F:694-737)
* ``driver``           the chain, on a dict of MPAS fields

Every binary operation is in the Fortran's order; ``x**2`` is ``x * x``; ``x**r`` with a real ``r`` and
``exp`` are the C library's (csrc/host_libm.c, as mpas_dycore.init_atm calls it), so ``kessler`` has the
compiled reference's bits where the reference calls the same library (tests/test_kessler_host.py).
Arrays are element-major as everywhere in this package: a column is a row, (ncol, K); ``zgrid`` is
(ncol, K + 1), ``scalars`` (ncol, K, num_scalars).  The sedimentation's time-split loop runs per column
in plain Python: test shapes are small.

The scheme's one discontinuity is ``nfall = max(1, nint(0.5 + crmax / 0.75))``; ``kessler`` also returns,
per column and split decision, the distance of ``crmax / 0.75`` from the nearest integer >= 1 (nfall is 1
on all of [0, 1), so 0 is no threshold) -- the margin by which a last-bit difference in ``pow`` could
change a column's ``nfall``.
"""
from __future__ import annotations

import math

import numpy as np

from . import init_atm as _ia

# mpas_constants.F / mpas_atmphys_constants.F
GRAVITY = 9.80616
R_D = 287.0
R_V = 461.6
CP = 7.0 * R_D / 2.0
P0 = 100000.0
RCV = R_D / (CP - R_D)
EP_2 = R_D / R_V
XLV = 2.50e6
SVP1, SVP2, SVP3, SVPT0 = 0.6112, 17.67, 29.65, 273.15
RHO_W = 1000.0
# module_mp_kessler.F:23-26, 76
C1, C2, C3, C4 = .001, .001, 2.2, .875
MAX_CR_SEDIMENTATION = 0.75


def _pow(x, y: float) -> np.ndarray:
    """The C library's pow(x, y), element by element (no compiler shortcut applies to these exponents)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if _ia._HOST is not None:
        out = np.empty_like(x)
        _ia._HOST.hl_pow_s(x.ctypes.data, float(y), out.ctypes.data, x.size)
        return out
    return np.asarray(_ia._LIBM_POW(x, float(y)), dtype=np.float64).reshape(x.shape)


def _exp(x) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float64)
    return np.asarray(_ia._exp(x), dtype=np.float64).reshape(x.shape)


def _nint(x: float) -> int:
    """Fortran nint: halves round away from zero."""
    return int(math.floor(x + 0.5)) if x >= 0.0 else -int(math.floor(-x + 0.5))


def _nfall(crmax: float):
    x = crmax / MAX_CR_SEDIMENTATION
    return max(1, _nint(0.5 + x)), abs(x - max(1.0, round(x)))


def fixture_columns(npz, K: int):
    """The columns of tests/golden/kessler_columns.npz (tools/make_kessler_golden.py) for one K: (inputs of
    kessler() as float64 plus ``zgrid``, the compiled reference's outputs, dt).  z and dz8w are zgrid's
    levels and differences, as microphysics_from_MPAS forms them."""
    cols = {n: np.asarray(npz[f"{n}_K{K}"], dtype=np.float64) for n in ("t", "qv", "qc", "qr", "rho", "pii", "zgrid")}
    cols["z"] = cols["zgrid"][:, :K].copy()
    cols["dz8w"] = cols["zgrid"][:, 1:] - cols["zgrid"][:, :K]
    ref = {n: np.asarray(npz[f"ref_{n}_K{K}"]) for n in ("t", "qv", "qc", "qr", "rainnc", "rainncv")}
    return cols, ref, float(npz[f"dt_K{K}"])


def from_mpas(theta_m, scalars, rho_zz, zz, exner, zgrid, index_qv=0, index_qc=1, index_qr=2) -> dict:
    """microphysics_from_MPAS (:541-559) for Kessler; scalar indices 0-based."""
    theta_m, zz, rho_zz = (np.asarray(a, dtype=np.float64) for a in (theta_m, zz, rho_zz))
    scalars, zgrid = np.asarray(scalars, dtype=np.float64), np.asarray(zgrid, dtype=np.float64)
    K = theta_m.shape[1]
    qv = scalars[:, :, index_qv].copy()
    return {"qv": qv, "qc": scalars[:, :, index_qc].copy(), "qr": scalars[:, :, index_qr].copy(),
            "rho": zz * rho_zz,
            "t": theta_m / (1.0 + R_V / R_D * np.maximum(0.0, qv)),
            "pii": np.array(exner, dtype=np.float64, copy=True),
            "z": zgrid[:, :K].copy(), "dz8w": zgrid[:, 1:K + 1] - zgrid[:, :K]}


def kessler(t, qv, qc, qr, rho, pii, z, dz8w, dt: float, rainnc=None, rainncv=None) -> dict:
    """SUBROUTINE kessler.  Returns the new t, qv, qc, qr, rainnc, rainncv (inputs are not changed) and
    ``info``: ``margin`` (per column, the nint margins of its split decisions), ``nfall0`` (the first
    nfall), ``resplit`` (per column: nfall_new /= nfall occurred), and per cell-level the branches of the
    sweep: ``cond`` (prod > 0), ``ern1`` / ``ern2`` / ``ern3`` (ern > 0 and equal to that amin1 argument),
    ``exhaust`` (product = -qc with cloud to exhaust, qc > 0)."""
    t, qv, qc, qr, rho, pii, z, dz8w = (np.array(a, dtype=np.float64, copy=True)
                                        for a in (t, qv, qc, qr, rho, pii, z, dz8w))
    n, K = t.shape
    dt = float(dt)
    rainnc = np.zeros(n) if rainnc is None else np.array(rainnc, dtype=np.float64, copy=True)
    rainncv = np.zeros(n) if rainncv is None else np.array(rainncv, dtype=np.float64, copy=True)
    f5 = SVP2 * (SVPT0 - SVP3) * XLV / CP
    prod = np.empty((n, K))
    margins, nfall0, resplit = [], np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)

    for i in range(n):                                                               # :95-195
        prodk = qr[i].copy()
        rhok = rho[i].copy()
        qrr = np.maximum(0.0, qr[i] * 0.001 * rhok)
        vtden = np.sqrt(rhok[0] / rhok)
        vt = 36.34 * _pow(qrr, 0.1364) * vtden
        rdzw = 1.0 / dz8w[i]
        crmax = 0.0
        for k in range(K):
            crmax = max(vt[k] * dt * rdzw[k], crmax)
        rdzk = np.empty(K)
        rdzk[:K - 1] = 1.0 / (z[i, 1:] - z[i, :K - 1])
        rdzk[K - 1] = 1.0 / (z[i, K - 1] - z[i, K - 2])
        nfall, m = _nfall(float(crmax))
        col_margin = [m]
        nfall0[i] = nfall
        dtfall = dt / float(nfall)
        time_sediment = dt
        while nfall > 0:
            time_sediment = time_sediment - dtfall
            factor = np.empty(K)
            factor[:K - 1] = dtfall * rdzk[:K - 1] / rhok[:K - 1]
            factor[K - 1] = dtfall * rdzk[K - 1]
            ppt = rhok[0] * prodk[0] * vt[0] * dtfall / RHO_W
            rainncv[i] = ppt * 1000.0
            rainnc[i] = rainnc[i] + ppt * 1000.0
            flux = rhok * prodk * vt                      # old values: level k reads k + 1 before its update
            new = prodk.copy()
            new[:K - 1] = prodk[:K - 1] - factor[:K - 1] * (flux[:K - 1] - flux[1:])
            new[K - 1] = prodk[K - 1] - factor[K - 1] * prodk[K - 1] * vt[K - 1]
            prodk = new
            if nfall > 1:
                nfall = nfall - 1
                qrr = np.maximum(0.0, prodk * 0.001 * rhok)
                vt = 36.34 * _pow(qrr, 0.1364) * vtden
                crmax = 0.0
                for k in range(K):
                    crmax = max(vt[k] * time_sediment * rdzw[k], crmax)
                nfall_new, m = _nfall(float(crmax))
                col_margin.append(m)
                if nfall_new != nfall:
                    resplit[i] = True
                    nfall = nfall_new
                    dtfall = time_sediment / float(nfall)
            else:
                prod[i] = prodk
                nfall = 0
        margins.append(np.array(col_margin))

    # production, saturation adjustment, evaporation (:203-236): per level, all columns at once
    factorn = 1.0 / (1.0 + C3 * dt * _pow(np.maximum(0.0, qr), C4))
    qrprod = qc * (1.0 - factorn) + factorn * C1 * dt * np.maximum(qc - C2, 0.0)
    rcgs = 0.001 * rho
    qc = np.maximum(qc - qrprod, 0.0)
    qr = (qr + prod - qr)
    qr = np.maximum(qr + qrprod, 0.0)
    temp = pii * t
    pressure = 1.000e+05 * _pow(pii, 1004. / 287.)
    gam = 2.5e+06 / (1004. * pii)
    es = 1000. * SVP1 * _exp(SVP2 * (temp - SVPT0) / (temp - SVP3))
    qvs = EP_2 * es / (pressure - es)
    t3 = temp - SVP3
    prod = (qv - qvs) / (1. + pressure / (pressure - es) * qvs * f5 / (t3 * t3))
    rq = rcgs * qr
    dim = np.where(qvs > qv, qvs - qv, 0.0)
    e1 = dt * (((1.6 + 124.9 * _pow(rq, .2046)) * _pow(rq, .525)) / (2.55e8 / (pressure * qvs) + 5.4e5)) * (
        dim / (rcgs * qvs))
    e2 = np.maximum(-prod - qc, 0.0)
    e3 = qr
    ern = np.minimum(np.minimum(e1, e2), e3)
    product = np.maximum(prod, -qc)
    info = {"margin": margins, "nfall0": nfall0, "resplit": resplit, "cond": prod > 0.0,
            "ern1": (ern > 0.0) & (ern == e1), "ern2": (ern > 0.0) & (ern == e2), "ern3": (ern > 0.0) & (ern == e3),
            "exhaust": (product == -qc) & (qc > 0.0)}
    t = t + gam * (product - ern)
    qv = np.maximum(qv - product + ern, 0.0)
    qc = qc + product
    qr = qr - ern
    return {"t": t, "qv": qv, "qc": qc, "qr": qr, "rainnc": rainnc, "rainncv": rainncv, "info": info}


def precip_to_mpas(rho, qv, dz8w, rainnc_p, rainnc, i_rainnc, bucket_rainnc: float = 0.0) -> dict:
    """precip_to_MPAS (:533-559) after a scheme that started from precip_from_MPAS's rainnc_p = 0:
    precipw summed over k ascending from 0.0, rainncv = rainnc_p, rainnc += rainncv, the bucket."""
    rho, qv, dz8w = (np.asarray(a, dtype=np.float64) for a in (rho, qv, dz8w))
    precipw = np.zeros(rho.shape[0])
    for k in range(rho.shape[1]):
        rho_a = rho[:, k] / (1.0 + qv[:, k])
        precipw = precipw + qv[:, k] * rho_a * dz8w[:, k]
    rainncv = np.array(rainnc_p, dtype=np.float64, copy=True)
    rainnc = np.asarray(rainnc, dtype=np.float64) + rainncv
    i_rainnc = np.array(i_rainnc, dtype=np.int32, copy=True)
    if bucket_rainnc > 0.0:                                # l_acrain
        over = rainnc > bucket_rainnc
        i_rainnc[over] = i_rainnc[over] + 1
        rainnc = np.where(over, rainnc - bucket_rainnc, rainnc)
    return {"precipw": precipw, "rainncv": rainncv, "rainnc": rainnc, "i_rainnc": i_rainnc}


def to_mpas(t, qv, theta_m, rho_zz, zz, zgrid, rtheta_base, exner_base, pressure_base, surface_pressure,
            dt: float) -> dict:
    """microphysics_to_MPAS (:694-737): from the scheme's th and qv and the state's old theta_m, the new
    theta_m, rt_diabatic_tend, rtheta_p, exner, pressure_p, surface_pressure and tend_sfc_pressure."""
    t, qv, theta_m, rho_zz, zz, zgrid, rtb, exb, pb = (np.asarray(a, dtype=np.float64) for a in (
        t, qv, theta_m, rho_zz, zz, zgrid, rtheta_base, exner_base, pressure_base))
    tm = t * (1. + R_V / R_D * qv)
    rt_diabatic_tend = (tm - theta_m) / dt
    rtheta_p = rho_zz * tm - rtb
    exner = _pow(zz * (R_D / P0) * (rtheta_p + rtb), RCV)
    pressure_p = zz * R_D * (exner * rtheta_p + (exner - exb) * rtb)
    tem1 = zgrid[:, 1] - zgrid[:, 0]
    tem2 = zgrid[:, 2] - zgrid[:, 1]
    rho1 = rho_zz[:, 0] * zz[:, 0] * (1. + qv[:, 0])
    rho2 = rho_zz[:, 1] * zz[:, 1] * (1. + qv[:, 1])
    sp = 0.5 * GRAVITY * (zgrid[:, 1] - zgrid[:, 0]) * (rho1 - 0.5 * (rho2 - rho1) * tem1 / (tem1 + tem2))
    sp = sp + pressure_p[:, 0] + pb[:, 0]
    tend_sfc_pressure = (sp - np.asarray(surface_pressure, dtype=np.float64)) / dt
    return {"theta_m": tm, "rt_diabatic_tend": rt_diabatic_tend, "rtheta_p": rtheta_p, "exner": exner,
            "pressure_p": pressure_p, "surface_pressure": sp, "tend_sfc_pressure": tend_sfc_pressure}


DRIVER_IN = ("theta_m", "scalars", "rho_zz", "zz", "exner", "zgrid", "rtheta_base", "exner_base", "pressure_base")


def driver(f: dict, dt: float, index_qv: int = 0, index_qc: int = 1, index_qr: int = 2,
           bucket_rainnc: float = 0.0, scheme_out: dict | None = None) -> dict:
    """driver_microphysics for mp_kessler on the rows of ``f``: DRIVER_IN plus, optionally, ``rainnc``,
    ``i_rainnc`` and ``surface_pressure`` (default 0).  Returns the fields the call changes: theta_m,
    scalars, rt_diabatic_tend, rtheta_p, exner, pressure_p, rainnc, rainncv, i_rainnc, precipw,
    surface_pressure, tend_sfc_pressure, and ``info`` of the scheme.  ``scheme_out``: the scheme's own
    t, qv, qc, qr, rainnc in place of kessler()'s (a test substitutes the compiled reference's)."""
    n = np.asarray(f["theta_m"]).shape[0]
    a = from_mpas(f["theta_m"], f["scalars"], f["rho_zz"], f["zz"], f["exner"], f["zgrid"], index_qv, index_qc,
                  index_qr)
    k = scheme_out if scheme_out is not None else kessler(a["t"], a["qv"], a["qc"], a["qr"], a["rho"], a["pii"],
                                                         a["z"], a["dz8w"], dt)
    p = precip_to_mpas(a["rho"], k["qv"], a["dz8w"], k["rainnc"], f.get("rainnc", np.zeros(n)),
                       f.get("i_rainnc", np.zeros(n, dtype=np.int32)), bucket_rainnc)
    m = to_mpas(k["t"], k["qv"], f["theta_m"], f["rho_zz"], f["zz"], f["zgrid"], f["rtheta_base"], f["exner_base"],
                f["pressure_base"], f.get("surface_pressure", np.zeros(n)), dt)
    scalars = np.array(f["scalars"], dtype=np.float64, copy=True)
    scalars[:, :, index_qv], scalars[:, :, index_qc], scalars[:, :, index_qr] = k["qv"], k["qc"], k["qr"]
    return {**m, **p, "scalars": scalars, "info": k.get("info")}

"""Host restatement of the output-time convective diagnostics (csrc/convcompute.hip,
mpas_dyc_convective_diagnostics).

convective_diagnostics_compute of the reference (core_atmosphere/diagnostics/convective_diagnostics.F:227-487)
with column_height_value, integral_zstaggered, integral_zpoint (:528-589) and getcape (:595-1037; source = 2,
adiabat = 1, pinc = 100), in numpy, fp64, vectorised over columns, every + - * / in the Fortran's order.
``exp`` / ``log`` / ``pow`` are the C library's (csrc/host_libm.c), ``x**2`` is ``x * x`` and ``x**(-1)`` is
``1 / x``, as the compiled reference evaluates them, so the restatement has the compiled reference's bits
(tests/test_convcompute_host.py checks all twelve written outputs against tests/golden/convective_columns.npz).

Arrays are element-major in model order: ``(n, K)`` mass levels and ``(n, K + 1)`` interfaces, the ground
first.  ``compute`` returns the twelve written outputs (lcl and lfc have none: the reference never computes
them) and ``info``, the discrete decisions of every column's parcel ascent:
  kmax      the source level (0-based);
  iters     the iterations of every sub-step, (n, most sub-steps), 0 beyond a column's last;
  nsub      the sub-steps taken;
  branch    per level the branch of the area bookkeeping (0: not reached);
  end       how the ascent ended (END_*).
The optional ``ulp`` moves every exp / log / pow result by that many ``nextafter`` steps: a column whose
``info`` is the same for ulp in (0, +4, -4) is *stable* -- a library whose functions are within that envelope
takes the same decisions and differs in cape / cin by rounding only -- and *borderline* otherwise
(``classify``).  The classification depends on this module alone.

One defined deviation from the reference, shared with the device kernel: BOUNDED WORK.  A column's ascent
ends, with cape and cin as accumulated so far, before the sub-step that would be its
(SUBSTEP_CAP + K + 1)th, and int(dp / pinc) counts as at most 2**30.  A column monotone below 8192 hPa never
gets there.
"""
from __future__ import annotations

import numpy as np

from . import init_atm as _ia
from . import isobaric as _iso
from .fields import CONV_OUTPUTS

# MPAS_DYC_CONV_*, in the order of the reference's list (:285-312)
OUTPUTS = CONV_OUTPUTS
(CAPE, CIN, LCL, LFC, SRH_0_1KM, SRH_0_3KM, UZONAL_SURFACE, UZONAL_1KM, UZONAL_6KM, UMERIDIONAL_SURFACE,
 UMERIDIONAL_1KM, UMERIDIONAL_6KM, TEMPERATURE_SURFACE, DEWPOINT_SURFACE) = (1 << i for i in range(14))
ALL = 16383
WRITTEN = tuple(n for n in OUTPUTS if n not in ("lcl", "lfc"))
# through the device's exp / log / pow: held to a bound; the other nine written outputs bit for bit
SOFT = ("cape", "cin", "dewpoint_surface")
INPUTS = ("theta_m", "qv", "exner", "pressure_p", "pressure_base", "uzonal", "umeridional", "zgrid")
RVORD = 461.6 / 287.0
SUBSTEP_CAP = 8192
# info["branch"]: first trip into positive area, first trip into negative area, still negative, still positive
NOT_REACHED, FIRST_POSITIVE, FIRST_NEGATIVE, NEGATIVE, POSITIVE = 0, 1, 2, 3, 4
# info["end"]: the top level, the 100 hPa stop, no convergence in 100 iterations, the sub-step cap
END_TOP, END_100HPA, END_NOCONV, END_CAP = 0, 1, 2, 3

# getcape's parameters (:637, :677-700)
PINC, G, P00, CP, RD, RV, XLV = 100.0, 9.81, 100000.0, 1005.7, 287.04, 461.5, 2501000.0
T0, CPV, CPL = 273.15, 1875.0, 4190.0
LV1, LV2 = XLV + (CPL - CPV) * T0, CPL - CPV
RP00, EPS, REPS, RDDCP, CPDG = 1.0 / P00, RD / RV, RV / RD, RD / CP, CP / G
CONVERGE = 0.0002


if _ia._HOST is not None:
    import ctypes as _C
    _ia._HOST.hl_pow_v.argtypes = [_C.c_void_p, _C.c_void_p, _C.c_void_p, _C.c_int64]


def written_by(flags: int) -> tuple:
    """The diag fields a MPAS_DYC_CONV_* mask writes: the reference's quirks."""
    if not flags:
        return ()
    out = ["uzonal_surface", "umeridional_surface", "temperature_surface", "dewpoint_surface"]
    if flags & (CAPE | CIN):
        out += ["cape", "cin"]
    for bit in (SRH_0_1KM, SRH_0_3KM, UZONAL_1KM, UZONAL_6KM, UMERIDIONAL_1KM, UMERIDIONAL_6KM):
        if flags & bit:
            out.append(OUTPUTS[bit.bit_length() - 1])
    return tuple(out)


class _Libm:
    """exp / log / pow of the C library, each result moved by ``ulp`` nextafter steps."""

    def __init__(self, ulp: int = 0):
        self.ulp = int(ulp)

    def _shift(self, x):
        to = np.inf if self.ulp > 0 else -np.inf
        for _ in range(abs(self.ulp)):
            x = np.nextafter(x, to)
        return x

    def exp(self, x):
        return self._shift(_ia._exp(x))

    def log(self, x):
        return self._shift(_iso._log(x))

    def pow(self, x, y):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if np.ndim(y) == 0:
            return self._shift(_iso._pow(x, float(y)))
        y = np.ascontiguousarray(y, dtype=np.float64)
        if _ia._HOST is not None:
            out = np.empty_like(x)
            _ia._HOST.hl_pow_v(x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size)
        else:
            out = np.asarray(_ia._LIBM_POW(x, y), dtype=np.float64)
        return self._shift(out)


def host_libm_loaded() -> bool:
    return _ia.host_libm_loaded()


# ------------------------------------------------------------------------------------ :361-374
def temperature(f):
    return (f["theta_m"] / (1.0 + RVORD * f["qv"])) * f["exner"]


def dewpoint(f, m: _Libm):
    evp = 0.01 * (f["pressure_base"] + f["pressure_p"]) * f["qv"] / (f["qv"] + 0.622)
    evp = np.maximum(evp, 1.0e-8)
    lg = m.log(evp / 6.112)
    return (243.5 * lg) / (17.67 - lg) + 273.15


# ------------------------------------------------------------------------------------ :528-589
def column_height_value(v, zp, z):
    n, K = zp.shape
    below = zp <= z
    kz = np.where(below.any(axis=1), K - 1 - np.argmax(below[:, ::-1], axis=1), 0)
    kz = np.minimum(kz, K - 2)
    r = np.arange(n)
    wz = (zp[r, kz + 1] - z) / (zp[r, kz + 1] - zp[r, kz])
    wzp1 = 1. - wz
    return wz * v[r, kz] + wzp1 * v[r, kz + 1]


def integral_zstaggered(v, z, zbot, ztop):
    s = np.zeros(v.shape[0])
    for k in range(v.shape[1]):
        zb = np.maximum(z[:, k], zbot)
        zt = np.minimum(z[:, k + 1], ztop)
        s = s + v[:, k] * np.maximum(0., zt - zb)
    return s


def integral_zpoint(v, z, zbot, ztop):
    s = np.zeros(v.shape[0])
    for k in range(v.shape[1] - 1):
        zb = np.maximum(z[:, k], zbot)
        zt = np.minimum(z[:, k + 1], ztop)
        dz = np.maximum(0., zt - zb)
        zr_midpoint = (0.5 * (zt + zb) - z[:, k]) / (z[:, k + 1] - z[:, k])
        midpoint_value = v[:, k] + (v[:, k + 1] - v[:, k]) * zr_midpoint
        s = s + dz * midpoint_value
    return s


def shear(f, m: _Libm | None = None) -> dict:
    """:377-451: the surface, 1 km and 6 km fields and the two helicities; ``shear_magnitude`` and ``srh``
    (before the max) ride along for the coverage checks."""
    m = m or _Libm()
    u, v, h = f["uzonal"], f["umeridional"], f["zgrid"]
    n, K = u.shape
    zp = 0.5 * (h[:, :K] + h[:, 1:]) - h[:, :1]
    zrel = h - h[:, :1]
    out = {"uzonal_surface": u[:, 0].copy(), "umeridional_surface": v[:, 0].copy(),
           "temperature_surface": temperature({k: f[k][:, :1] for k in ("theta_m", "qv", "exner")})[:, 0],
           "dewpoint_surface": dewpoint({k: f[k][:, :1] for k in ("pressure_base", "pressure_p", "qv")}, m)[:, 0]}
    out["uzonal_1km"] = column_height_value(u, zp, 1000.0)
    out["umeridional_1km"] = column_height_value(v, zp, 1000.0)
    out["uzonal_6km"] = column_height_value(u, zp, 6000.0)
    out["umeridional_6km"] = column_height_value(v, zp, 6000.0)
    dev_motion, z_bunker_bot, z_bunker_top = 7.5, 0., 6000.
    low = z_bunker_bot > zp[:, 0]
    u_srh_bot = np.where(low, column_height_value(u, zp, z_bunker_bot), u[:, 0])
    v_srh_bot = np.where(low, column_height_value(v, zp, z_bunker_bot), v[:, 0])
    u_shear = out["uzonal_6km"] - u_srh_bot
    v_shear = out["umeridional_6km"] - v_srh_bot
    u_mean = integral_zstaggered(u, zrel, z_bunker_bot, z_bunker_top) / (z_bunker_top - z_bunker_bot)
    v_mean = integral_zstaggered(v, zrel, z_bunker_bot, z_bunker_top) / (z_bunker_top - z_bunker_bot)
    shear_raw = np.sqrt(u_shear * u_shear + v_shear * v_shear)
    shear_magnitude = np.maximum(0.0001, shear_raw)
    u_storm = u_mean + dev_motion * v_shear / shear_magnitude
    v_storm = v_mean - dev_motion * u_shear / shear_magnitude
    dudz, dvdz = np.empty((n, K)), np.empty((n, K))
    for d, w in ((dudz, u), (dvdz, v)):
        d[:, 1:K - 1] = (w[:, 1:K - 1] - w[:, 0:K - 2]) / (0.5 * (h[:, 2:K] - h[:, 0:K - 2]))
        d[:, 0] = d[:, 1]
        d[:, K - 1] = d[:, K - 2]
    srh = np.empty((n, K + 1))
    us, vs = u_storm[:, None], v_storm[:, None]
    srh[:, 1:K] = -(0.5 * (u[:, 1:] + u[:, :-1]) - us) * dvdz[:, 1:] + (0.5 * (v[:, 1:] + v[:, :-1]) - vs) * dudz[:, 1:]
    srh[:, 0] = -(u[:, 0] - u_storm) * dvdz[:, 0] + (v[:, 0] - v_storm) * dudz[:, 0]
    srh[:, K] = srh[:, K - 1]
    pos = np.maximum(0., srh)
    out["srh_0_1km"] = integral_zpoint(pos, zrel, 0.0, 1000.0)
    out["srh_0_3km"] = integral_zpoint(pos, zrel, 0.0, 3000.0)
    out["info_shear"] = {"shear_raw": shear_raw, "srh_raw": srh, "zp": zp}
    return out


# ------------------------------------------------------------------------------------ getcape
def getqvs(p, t, m: _Libm):
    es = 611.2 * m.exp(17.67 * (t - 273.15) / (t - 29.65))
    return (287.04 / 461.5) * es / (p - es)


def getthe(p, t, td, q, m: _Libm):
    with np.errstate(all="ignore"):
        tlcl = np.where((td - t) >= -0.1, t, 56.0 + 1.0 / (1.0 / (td - 56.0) + 0.00125 * m.log(t / td)))
        return t * m.pow(100000.0 / p, 0.2854 * (1.0 - 0.28 * q)) * m.exp(((3376.0 / tlcl) - 2.54) * q * (1.0 + 0.81 * q))


def levels(f, m: _Libm) -> dict:
    """p, t, td, pi, q, th, thv of every level (:456-458, :708-716)."""
    p_in = (f["pressure_p"] + f["pressure_base"]) / 100.0
    t_in = temperature(f) - 273.15
    td_in = dewpoint(f, m) - 273.15
    L = {"p": 100.0 * p_in, "t": 273.15 + t_in, "td": 273.15 + td_in}
    L["pi"] = m.pow(L["p"] * RP00, RDDCP)
    L["q"] = getqvs(L["p"], L["td"], m)
    L["th"] = L["t"] / L["pi"]
    L["thv"] = L["th"] * (1.0 + REPS * L["q"]) / (1.0 + L["q"])
    return L


def getcape(f, m: _Libm | None = None):
    """cape, cin and info of every column."""
    m = m or _Libm()
    with np.errstate(all="ignore"):
        return _getcape(f, m)


def _getcape(f, m):
    L = levels(f, m)
    n, K = L["p"].shape
    r = np.arange(n)
    # the source parcel (:732-751): the first maximum of theta-e over the levels with p >= 500 hPa
    the = getthe(L["p"], L["t"], L["td"], L["q"], m)
    kmax = np.zeros(n, dtype=np.int64)
    maxthe = np.zeros(n)
    for k in range(K):
        better = (L["p"][:, k] >= 50000.0) & (the[:, k] > maxthe)
        maxthe = np.where(better, the[:, k], maxthe)
        kmax = np.where(better, k, kmax)
    kmax = np.where(L["p"][:, 0] < 50000.0, 0, kmax)

    k = kmax.copy()
    st = {q: L[q][r, kmax].copy() for q in ("th", "pi", "p", "t", "thv")}
    th2, pi2, p2, t2, thv2 = st["th"], st["pi"], st["p"], st["t"], st["thv"]
    qv2 = L["q"][r, kmax].copy()
    b2, narea, cape, cin = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    qt = qv2.copy()
    left = np.full(n, SUBSTEP_CAP + K, dtype=np.int64)
    end = np.full(n, END_TOP, dtype=np.int8)
    branch = np.zeros((n, K), dtype=np.int8)
    iters = np.zeros((n, 1024), dtype=np.int16)
    nsub = np.zeros(n, dtype=np.int64)
    active = k < K - 1

    while active.any():
        idx = np.flatnonzero(active)
        k[idx] += 1
        ki = k[idx]
        b1 = b2[idx].copy()
        e_p, e_pi, e_thv = L["p"][idx, ki], L["pi"][idx, ki], L["thv"][idx, ki]
        dp = L["p"][idx, ki - 1] - e_p
        ratio = dp / PINC
        big = np.where(ratio < 1073741824.0, np.trunc(np.where(ratio < 1073741824.0, ratio, 0.0)), 1073741824.0)
        nloop = np.where(dp < PINC, 1, 1 + big.astype(np.int64))
        dp = np.where(dp < PINC, dp, dp / nloop.astype(np.float64))
        alive = np.ones(idx.size, dtype=bool)      # still inside this level's sub-steps
        for s in range(int(nloop.max())):
            run = alive & (s < nloop)
            if not run.any():
                break
            capped = run & (left[idx] <= 0)        # the bounded-work deviation
            if capped.any():
                end[idx[capped]] = END_CAP
                active[idx[capped]] = False
                alive &= ~capped
                run &= ~capped
                if not run.any():
                    break
            sub = idx[run]
            left[sub] -= 1
            p1, t1, th1, qv1, qts, dps = p2[sub], t2[sub], th2[sub], qv2[sub], qt[sub], dp[run]
            p2s = p1 - dps
            pi2s = m.pow(p2s * RP00, RDDCP)
            logp = m.log(p2s / p1)
            thlast = th1.copy()
            t2s, qv2s, th2s = t1.copy(), qv1.copy(), th1.copy()
            it = np.zeros(sub.size, dtype=np.int64)
            nc = np.ones(sub.size, dtype=bool)
            failed = np.zeros(sub.size, dtype=bool)
            while nc.any():
                it = np.where(nc, it + 1, it)
                t2n = thlast * pi2s
                qv2n = np.minimum(qts, getqvs(p2s, t2n, m))
                ql2n = np.maximum(qts - qv2n, 0.0)
                tbar = 0.5 * (t1 + t2n)
                qvbar = 0.5 * (qv1 + qv2n)
                qlbar = 0.5 * ql2n
                lhv = LV1 - LV2 * tbar
                rm = RD + RV * qvbar
                cpm = CP + CPV * qvbar + CPL * qlbar
                th2n = th1 * m.exp(lhv * ql2n / (cpm * tbar) + (rm / cpm - RD / CP) * logp)
                t2s, qv2s, th2s = np.where(nc, t2n, t2s), np.where(nc, qv2n, qv2s), np.where(nc, th2n, th2s)
                fail = nc & (it > 100)
                failed |= fail
                nc &= ~fail
                more = nc & (np.abs(th2s - thlast) > CONVERGE)
                thlast = np.where(more, thlast + 0.3 * (th2s - thlast), thlast)
                nc = more
            col = nsub[sub]
            if col.max() >= iters.shape[1]:
                iters = np.concatenate([iters, np.zeros_like(iters)], axis=1)
            iters[sub, col] = it
            nsub[sub] += 1
            p2[sub], pi2[sub], t2[sub], qv2[sub], th2[sub] = p2s, pi2s, t2s, qv2s, th2s
            qt[sub] = np.where(failed, qts, qv2s)
            if failed.any():                       # :935-945: return with cape and cin as they are
                bad = sub[failed]
                end[bad] = END_NOCONV
                active[bad] = False
                alive[np.flatnonzero(run)[failed]] = False
        a = idx[alive]
        if a.size == 0:
            continue
        ka, b1, e_p, e_pi, e_thv = k[a], b1[alive], e_p[alive], e_pi[alive], e_thv[alive]
        thv2[a] = th2[a] * (1.0 + REPS * qv2[a]) / (1.0 + qv2[a])
        b2a = G * (thv2[a] - e_thv) / e_thv
        dz = -CPDG * 0.5 * (e_thv + L["thv"][a, ka - 1]) * (e_pi - L["pi"][a, ka - 1])
        first_pos = (b2a >= 0.0) & (b1 < 0.0)
        first_neg = ~first_pos & (b2a < 0.0) & (b1 > 0.0)
        neg = ~first_pos & ~first_neg & (b2a < 0.0)
        pos = ~first_pos & ~first_neg & ~neg
        na = narea[a]
        frac_p = b2a / (b2a - b1)
        frac_n = b1 / (b1 - b2a)
        parea = np.where(first_pos, 0.5 * b2a * dz * frac_p,
                         np.where(first_neg, 0.5 * b1 * dz * frac_n, np.where(neg, 0.0, 0.5 * dz * (b1 + b2a))))
        na_fp = na - 0.5 * b1 * dz * (1.0 - frac_p)
        cin[a] = np.where(first_pos, cin[a] + na_fp, cin[a])
        narea[a] = np.where(first_pos | pos, 0.0,
                            np.where(first_neg, -0.5 * b2a * dz * (1.0 - frac_n), na - 0.5 * dz * (b1 + b2a)))
        cape[a] = cape[a] + np.maximum(0.0, parea)
        b2[a] = b2a
        branch[a, ka] = np.where(first_pos, FIRST_POSITIVE, np.where(first_neg, FIRST_NEGATIVE, np.where(neg, NEGATIVE, POSITIVE)))
        stop = (e_p <= 10000.0) & (b2a < 0.0)
        end[a[stop]] = END_100HPA
        active[a] = ~stop & (ka < K - 1)
    width = max(1, int(nsub.max()))
    info = {"kmax": kmax, "iters": iters[:, :width].copy(), "nsub": nsub, "branch": branch, "end": end,
            "p1": L["p"][:, 0].copy()}
    return cape, cin, info


def compute(f, ulp: int = 0) -> dict:
    """The twelve written outputs of convective_diagnostics_compute over the columns of ``f`` (INPUTS), and
    ``info``."""
    f = {k: np.asarray(f[k], dtype=np.float64) for k in INPUTS}
    m = _Libm(ulp)
    with np.errstate(all="ignore"):
        out = shear(f, m)
    cape, cin, info = getcape(f, m)
    out["cape"], out["cin"] = cape, cin
    info.update(out.pop("info_shear"))
    out["info"] = info
    return out


DECISIONS = ("kmax", "iters", "nsub", "branch", "end")


def same_decisions(a: dict, b: dict) -> np.ndarray:
    """Per column: the two runs' info agree."""
    ok = np.ones(a["kmax"].shape[0], dtype=bool)
    for name in DECISIONS:
        x, y = a[name], b[name]
        if x.ndim == 2 and x.shape[1] != y.shape[1]:
            w = max(x.shape[1], y.shape[1])
            x = np.pad(x, ((0, 0), (0, w - x.shape[1])))
            y = np.pad(y, ((0, 0), (0, w - y.shape[1])))
        ok &= (x == y) if x.ndim == 1 else np.all(x == y, axis=1)
    return ok


def classify(f, ulps=(4, -4)):
    """(the ulp = 0 run, per column stable?, the shifted runs)."""
    base = compute(f)
    others = [compute(f, u) for u in ulps]
    stable = np.ones(base["cape"].shape[0], dtype=bool)
    for o in others:
        stable &= same_decisions(base["info"], o["info"])
    return base, stable, others


# ------------------------------------------------------------------------------------ synthetic inputs
def sounding(zgrid, prm: dict, rng) -> dict:
    """MPAS-level inputs of columns on the interfaces ``zgrid`` (n, K + 1): a moist boundary layer under a
    conditionally unstable troposphere and an isothermal stratosphere, hydrostatic, with seeded winds.
    ``prm`` (each (n,) or a scalar): psfc (Pa at the lowest interface), tsfc (K), bl_depth (m), bl_lapse,
    lapse (K / m), trop (m above the ground), rh_bl, rh_free, and optionally dry_sfc (m: a dry layer under
    the moist one) and calm (bool: a uniform wind).  Every array holds numbers float32 holds exactly."""
    z = np.asarray(zgrid, dtype=np.float64)
    n, K1 = z.shape
    K = K1 - 1
    col = lambda name, default=None: np.broadcast_to(np.asarray(prm.get(name, default), dtype=np.float64), (n,))[:, None]  # noqa: E731
    zm = 0.5 * (z[:, :K] + z[:, 1:]) - z[:, :1]
    bl, trop = col("bl_depth"), col("trop")
    t_bl_top = col("tsfc") - col("bl_lapse") * bl
    temp = np.where(zm <= bl, col("tsfc") - col("bl_lapse") * zm,
                    np.where(zm <= trop, t_bl_top - col("lapse") * (zm - bl), t_bl_top - col("lapse") * (trop - bl)))
    temp = np.maximum(temp, 190.0)
    p = np.empty((n, K))
    p[:, 0] = col("psfc")[:, 0] * _ia._exp(-9.80616 * zm[:, 0] / (287.0 * temp[:, 0]))
    for k in range(1, K):
        p[:, k] = p[:, k - 1] * _ia._exp(-9.80616 * (zm[:, k] - zm[:, k - 1]) / (287.0 * 0.5 * (temp[:, k] + temp[:, k - 1])))
    dry = col("dry_sfc", 0.0)
    rh = np.where(zm < dry, 0.15, np.where(zm <= dry + bl, col("rh_bl"), col("rh_free")))
    rh = rh * (0.9 + 0.1 * rng.random((n, K)))
    es = 611.2 * _ia._exp(17.67 * (temp - 273.15) / (temp - 29.65))
    qv = np.maximum(rh * 0.622 * es / np.maximum(p - es, 1.0), 1.0e-7)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)  # noqa: E731
    f = {"zgrid": f32(z), "qv": f32(qv), "exner": f32(_iso._pow(p / 1.0e5, 287.0 / 1004.5))}
    f["theta_m"] = f32(temp / f["exner"] * (1.0 + RVORD * f["qv"]))
    f["pressure_base"] = f32(0.97 * p)
    f["pressure_p"] = f32(p - f["pressure_base"])
    turn = zm / 6000.0
    f["uzonal"] = f32(8.0 + 22.0 * np.minimum(turn, 2.0) + 3.0 * (rng.random((n, K)) - 0.5))
    f["umeridional"] = f32(10.0 * np.cos(1.6 * np.minimum(turn, 2.0)) + 3.0 * (rng.random((n, K)) - 0.5))
    calm = np.broadcast_to(np.asarray(prm.get("calm", False), dtype=bool), (n,))
    f["uzonal"][calm] = 5.0
    f["umeridional"][calm] = -3.0
    return f


def synthetic_fields(case: dict, K: int, seed: int = 0) -> dict:
    """MPAS-level inputs (INPUTS) of every cell of ``case`` (its zgrid, nVertLevels = K): unstable soundings,
    so that cape is not zero everywhere as it is for the JW states; deterministic on the CPU."""
    zgrid = np.asarray(case["zgrid"], dtype=np.float64)
    n = zgrid.shape[0]
    assert zgrid.shape[1] == K + 1, (zgrid.shape, K)
    rng = np.random.default_rng(1000 * K + seed)
    prm = {"psfc": 98000.0 + 3000.0 * rng.random(n), "tsfc": 296.0 + 8.0 * rng.random(n),
           "bl_depth": 800.0 + 900.0 * rng.random(n), "bl_lapse": 0.004 + 0.004 * rng.random(n),
           "lapse": 0.0066 + 0.0012 * rng.random(n), "trop": 10500.0 + 2500.0 * rng.random(n),
           "rh_bl": 0.6 + 0.3 * rng.random(n), "rh_free": 0.25 + 0.3 * rng.random(n),
           "dry_sfc": np.where(rng.random(n) < 0.2, 400.0, 0.0), "calm": rng.random(n) < 0.05}
    return sounding(zgrid, prm, rng)


def alternating_column(K: int = 26) -> dict:
    """One column (INPUTS, (1, K)) whose pressure alternates between 1000 and 10 hPa: every second level
    transition is 991 sub-steps, so the ascent meets the sub-step cap.  The 10 hPa levels are cold enough for
    the parcel to stay buoyant there, which keeps the 100 hPa stop out of the way."""
    low = np.arange(K) % 2 == 0
    p = np.where(low, 100000.0, 1000.0)[None, :]
    temp = np.where(low, 300.0, 80.0)[None, :]
    f = {"qv": np.where(low, 0.015625, 1.0e-7)[None, :].astype(np.float32).astype(np.float64)}
    f["exner"] = np.asarray(_iso._pow(p / 1.0e5, 287.0 / 1004.5), dtype=np.float32).astype(np.float64)
    f["theta_m"] = np.asarray(temp / f["exner"] * (1.0 + RVORD * f["qv"]), dtype=np.float32).astype(np.float64)
    f["pressure_base"], f["pressure_p"] = p.copy(), np.zeros((1, K))
    f["zgrid"] = (400.0 * np.arange(K + 1, dtype=np.float64))[None, :]
    f["uzonal"] = (10.0 + 0.5 * np.arange(K, dtype=np.float64))[None, :]
    f["umeridional"] = (5.0 - 0.25 * np.arange(K, dtype=np.float64))[None, :]
    return f


def fixture_columns(golden: dict, tag: str):
    """(inputs, reference outputs) of one set of tests/golden/convective_columns.npz."""
    cols = {name: np.asarray(golden[f"{name}_{tag}"], dtype=np.float64) for name in INPUTS}
    ref = {name: np.asarray(golden[f"ref_{name}_{tag}"], dtype=np.float64) for name in WRITTEN}
    return cols, ref

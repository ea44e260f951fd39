#!/usr/bin/env python3
"""Generate tests/golden/isobaric_columns.npz: synthetic columns through the reference's compiled isobaric diagnostics.

Build machine only (it needs the reference tree and amdflang).  In a temporary directory the script cuts
two line ranges out of the reference's unmodified diagnostics/isobaric_diagnostics.F at run time -- the three
array routines interp_tofixed_pressure, compute_slp, compute_layer_mean (:899-1245) and interp_diagnostics'
glue loops (:503-572: pressure, pressure2, pressure_v, temperature, dewpoint) -- and wraps them into a
generated module: the routines as they are, the glue inside a driver subroutine that declares pressure,
pressure_p, pressure_b, height, ... as plain arrays.  A small stand-in module of our own supplies RKIND,
MPAS_LOG_ERR, rvord and a no-op mpas_log_write.  The driver's calling sequence (reverse the levels, call
interp_tofixed_pressure; compute_slp times 100; pressure * 100 against the levels in Pa) restates
interp_diagnostics :574-888.  Compiled with the oracle's flags (amdflang -O2 -fdefault-real-8
-fdefault-double-8) and run on synthetic MPAS-level columns; inputs and outputs are stored.  Only data is
written: neither the reference's source nor the binary leaves the temporary directory.

For each K in KS: NCOL columns and NVERT vertices over them.  Inputs are numbers that float32 holds
exactly, stored as float32.  With the host restatement (mpas_dycore.isobaric) the script asserts what the
inputs must exercise (check_coverage; tests/test_isobaric_host.py re-checks it on the committed file), and
that every comparison whose operand passed through log / exp / pow keeps its sides apart by a relative
1e-9 (columns that miss it are redrawn).  One extra K = 4 set ("fail") makes compute_slp fail (no level
100 hPa above the ground on three columns): it zeroes the whole mslp array, so it is stored apart.

    python tools/make_isobaric_golden.py [--ref /path/to/reference] [--out tests/golden/isobaric_columns.npz]
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpas-model_amd"))

from mpas_dycore import isobaric as iso  # noqa: E402

KS = (4, 26, 63, 64, 150)
NCOL, NVERT = 40, 32
MIN_MARGIN = 1.0e-9
MIN_COLUMNS = 3
CELL_IN = ("pressure_p", "pressure_base", "theta_m", "qv", "exner", "relhum", "uzonal", "umeridional", "zgrid", "w")
VERT_IN = ("vorticity", "kiteAreasOnVertex", "areaTriangle")
ROUTINES = (899, 1245)   # interp_tofixed_pressure, compute_slp, compute_layer_mean
GLUE = (503, 572)        # pressure, pressure2, pressure_v, temperature, dewpoint

STANDIN = """
module iso_standin
   implicit none
   integer, parameter :: RKIND = selected_real_kind(12)
   integer, parameter :: MPAS_LOG_ERR = 2
   real (kind=RKIND), parameter :: rgas = 287.0, rv = 461.6
   real (kind=RKIND), parameter :: rvord = rv/rgas
contains
   subroutine mpas_log_write(message, messageType, intArgs, realArgs, logicArgs)
      character (len=*), intent(in) :: message
      integer, intent(in), optional :: messageType
      integer, dimension(:), intent(in), optional :: intArgs
      real (kind=RKIND), dimension(:), intent(in), optional :: realArgs
      logical, dimension(:), intent(in), optional :: logicArgs
   end subroutine mpas_log_write
end module iso_standin
"""

MODULE_HEAD = """
module iso_cut
   use iso_standin
   implicit none
contains
"""

GLUE_HEAD = """
   subroutine iso_glue(nCells, nVertLevels, nVertices, vertexDegree, index_qv, num_scalars, pressure_p, pressure_b, &
                       height, theta_m, scalars, exner, kiteAreasOnVertex, areaTriangle, cellsOnVertex, &
                       pressure, pressureCp1, pressure2, pressure_v, temperature, dewpoint)
      integer, intent(in) :: nCells, nVertLevels, nVertices, vertexDegree, index_qv, num_scalars
      real (kind=RKIND), intent(in) :: pressure_p(nVertLevels,nCells+1), pressure_b(nVertLevels,nCells+1)
      real (kind=RKIND), intent(in) :: height(nVertLevels+1,nCells), theta_m(nVertLevels,nCells), exner(nVertLevels,nCells)
      real (kind=RKIND), intent(in) :: scalars(num_scalars,nVertLevels,nCells)
      real (kind=RKIND), intent(in) :: kiteAreasOnVertex(vertexDegree,nVertices), areaTriangle(nVertices)
      integer, intent(in) :: cellsOnVertex(vertexDegree,nVertices)
      real (kind=RKIND), intent(out) :: pressure(nVertLevels,nCells), pressureCp1(nVertLevels,nCells+1)
      real (kind=RKIND), intent(out) :: pressure2(nVertLevels+1,nCells), pressure_v(nVertLevels,nVertices)
      real (kind=RKIND), intent(out) :: temperature(nVertLevels,nCells), dewpoint(nVertLevels,nCells)
      integer :: iCell, iVert, iVertD, k, nVertLevelsP1
      real (kind=RKIND) :: evp, w1, w2, z0, z1, z2
      logical, parameter :: NEED_TEMP = .true., NEED_RELHUM = .true., NEED_DEWPOINT = .true., need_mslp = .true.
      nVertLevelsP1 = nVertLevels + 1
"""

DRIVER = """
   end subroutine iso_glue

   ! field(L, n) on pres(L, n) to targets: the reversal loops and the call of interp_diagnostics (:587-605)
   subroutine rev_interp(n, L, nout, pres, field, targets, scale, field_interp)
      integer, intent(in) :: n, L, nout
      real (kind=RKIND), intent(in) :: pres(L,n), field(L,n), targets(nout), scale
      real (kind=RKIND), intent(out) :: field_interp(n,nout)
      real (kind=RKIND), allocatable :: press_in(:,:), field_in(:,:), press_interp(:,:)
      integer :: i, k, kk
      allocate(press_in(n,L), field_in(n,L), press_interp(n,nout))
      do k = 1, nout
         press_interp(:,k) = targets(k)
      end do
      do i = 1, n
      do k = 1, L
         kk = L+1-k
         if (scale > 0.0) then
            press_in(i,kk) = pres(k,i) * 100.0
         else
            press_in(i,kk) = pres(k,i)
         end if
         field_in(i,kk) = field(k,i)
      end do
      end do
      call interp_tofixed_pressure(n, L, nout, press_in, field_in, press_interp, field_interp)
   end subroutine rev_interp
end module iso_cut

program isobaric_columns
   use iso_cut
   implicit none
   integer(4) :: n, K, nv, i, kk, a
   real(8), allocatable :: pp(:,:), pb(:,:), f(:,:,:), height(:,:), w(:,:), vort(:,:), kite(:,:), area(:), scalars(:,:,:)
   integer(4), allocatable :: cov(:,:)
   real(8), allocatable :: pressure(:,:), pressureCp1(:,:), pressure2(:,:), pressure_v(:,:), temperature(:,:), dewpoint(:,:)
   real(8), allocatable :: o6(:,:), ov(:,:), mslp(:), ot(:,:), oz(:,:), meanT(:), press_in(:,:), field_in(:,:)
   real(8) :: hpa(6), tl(5), zl(13)
   hpa = (/ 200.0, 250.0, 500.0, 700.0, 850.0, 925.0 /)
   do i = 1, 5
      tl(i) = 30000.0 + 5000.0*(i-1)
   end do
   do i = 1, 13
      zl(i) = 30000.0 + 5000.0*(i-1)
   end do
   open(10, file='in.bin', access='stream', form='unformatted', status='old')
   read(10) n, K, nv
   allocate(pp(K,n+1), pb(K,n+1), f(K,n,6), height(K+1,n), w(K+1,n), vort(K,nv), kite(3,nv), area(nv), cov(3,nv))
   allocate(scalars(1,K,n))
   read(10) pp, pb
   do a = 1, 6
      read(10) f(:,:,a)      ! theta_m, qv, exner, relhum, uzonal, umeridional
   end do
   read(10) height, w, vort, kite, area, cov
   close(10)
   scalars(1,:,:) = f(:,:,2)
   allocate(pressure(K,n), pressureCp1(K,n+1), pressure2(K+1,n), pressure_v(K,nv), temperature(K,n), dewpoint(K,n))
   call iso_glue(n, K, nv, 3, 1, 1, pp, pb, height, f(:,:,1), scalars, f(:,:,3), kite, area, cov, &
                 pressure, pressureCp1, pressure2, pressure_v, temperature, dewpoint)
   allocate(o6(n,6), ov(nv,6), mslp(n), ot(n,5), oz(n,13), meanT(n))
   open(11, file='out.bin', access='stream', form='unformatted', status='replace')
   call rev_interp(n, K, 6, pressure, temperature, hpa, -1.0_8, o6)
   write(11) o6
   call rev_interp(n, K, 6, pressure, f(:,:,4), hpa, -1.0_8, o6)
   write(11) o6
   call rev_interp(n, K, 6, pressure, dewpoint, hpa, -1.0_8, o6)
   write(11) o6
   call rev_interp(n, K, 6, pressure, f(:,:,5), hpa, -1.0_8, o6)
   write(11) o6
   call rev_interp(n, K, 6, pressure, f(:,:,6), hpa, -1.0_8, o6)
   write(11) o6
   call rev_interp(n, K+1, 6, pressure2, height, hpa, -1.0_8, o6)
   write(11) o6
   call rev_interp(n, K+1, 6, pressure2, w, hpa, -1.0_8, o6)
   write(11) o6
   call rev_interp(nv, K, 6, pressure_v, vort, hpa, -1.0_8, ov)
   write(11) ov
   call compute_slp(n, K, 1, temperature, height, pressure, 1, scalars, mslp)
   mslp(:) = mslp(:) * 100.0
   write(11) mslp
   call rev_interp(n, K, 5, pressure, temperature, tl, 1.0_8, ot)
   write(11) ot
   allocate(press_in(n,K), field_in(n,K))
   do i = 1, n
   do kk = 1, K
      field_in(i,K+1-kk) = temperature(kk,i)
      press_in(i,K+1-kk) = pressure(kk,i) * 100.0
   end do
   end do
   call compute_layer_mean(meanT, 50000.0_8, 30000.0_8, field_in, press_in)
   write(11) meanT
   call rev_interp(n, K+1, 13, pressure2, height, zl, 1.0_8, oz)
   write(11) oz
   close(11)
end program isobaric_columns
"""


def build_reference(ref: str, tmp: str) -> str:
    src = os.path.join(ref, "src", "core_atmosphere", "diagnostics", "isobaric_diagnostics.F")
    lines = open(src).read().split("\n")
    cut = lambda r: "\n".join(lines[r[0] - 1:r[1]]) + "\n"  # noqa: E731
    open(os.path.join(tmp, "standin.f90"), "w").write(STANDIN)
    open(os.path.join(tmp, "iso_cut.f90"), "w").write(MODULE_HEAD + cut(ROUTINES) + GLUE_HEAD + cut(GLUE) + DRIVER)
    exe = os.path.join(tmp, "isobaric_columns")
    flags = ["-O2", "-fdefault-real-8", "-fdefault-double-8", "-ffree-form"]
    subprocess.run(["amdflang", *flags, "-c", "standin.f90"], check=True, cwd=tmp)
    subprocess.run(["amdflang", *flags, "iso_cut.f90", "standin.o", "-o", exe], check=True, cwd=tmp)
    return exe


def run_reference(exe: str, tmp: str, c: dict) -> dict:
    n, K = c["theta_m"].shape
    nv = c["vorticity"].shape[0]
    with open(os.path.join(tmp, "in.bin"), "wb") as fh:
        fh.write(np.array([n, K, nv], dtype=np.int32).tobytes())
        for name in ("pressure_p_img", "pressure_base_img", "theta_m", "qv", "exner", "relhum", "uzonal", "umeridional",
                     "zgrid", "w", "vorticity", "kiteAreasOnVertex", "areaTriangle"):
            fh.write(np.ascontiguousarray(c[name], dtype=np.float64).tobytes())
        fh.write(np.ascontiguousarray(c["cellsOnVertex"] + 1, dtype=np.int32).tobytes())
    subprocess.run([exe], check=True, cwd=tmp)
    raw = np.fromfile(os.path.join(tmp, "out.bin"), dtype=np.float64)
    out, pos = {}, 0

    def take(rows, cols):
        nonlocal pos
        a = raw[pos:pos + rows * cols].reshape(cols, rows).T.copy()
        pos += rows * cols
        return a
    for g in range(7):
        a = take(n, 6)
        for l in range(6):
            out[iso.field_name(g, l)] = a[:, l].copy()
    a = take(nv, 6)
    for l in range(6):
        out[iso.field_name(7, l)] = a[:, l].copy()
    out["mslp"] = take(n, 1)[:, 0]
    out["t_isobaric"] = take(n, 5)
    out["meanT_500_300"] = take(n, 1)[:, 0]
    out["z_isobaric"] = take(n, 13)
    assert pos == raw.size, (pos, raw.size)
    return out


def _quantize(a, bits: int) -> np.ndarray:
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return (u & np.uint32((0xFFFFFFFF << (23 - bits)) & 0xFFFFFFFF)).view(np.float32).astype(np.float64)


K4 = {  # K = 4 level pressures in hPa by column kind (two variants of the general kind)
    0: (990.0, 450.0, 350.0, 100.0), 1: (990.0, 920.0, 350.0, 100.0), 2: (620.0, 450.0, 350.0, 100.0),
    3: (980.0, 760.0, 540.0, 330.0), 4: (980.0, 700.0, 500.0, 120.0), 5: (980.0, 600.0, 400.0, 200.0),
    6: (980.0, 600.0, 330.0, 205.0), 7: (990.0, 520.0, 280.0, 100.0)}


def level_pressures(rng, K: int, kind: int, i: int, warm_high: bool, shallow: bool = False) -> tuple:
    """Mass-level pressures (hPa, ground first) of one column, and whether they are exact in hPa.
    Kinds: 0, 1 general; 2 mountain (targets below the ground); 3 shallow top (targets above the top);
    4 exact, one level on a target; 5 exact, the top level on a target; 6 a target between the two top
    interfaces; 7 one model layer holds 300 .. 500 hPa."""
    if shallow:  # compute_slp's failure: no level 100 hPa above the ground
        return 1000.0 - 90.0 * (np.arange(K) / (K - 1)) * (1.0 + 0.05 * rng.random()), False
    if K == 4:
        p = np.array(K4[kind])
        if kind in (4, 5):
            return p, True
        if kind == 6:
            return p * np.array([1.0, 1.0, 1.0, (1.0, 1.25, 1.0)[i % 3]]) * (1.0 + 0.002 * rng.random()), False
        p = p * (1.0 + 0.01 * rng.random())
        if warm_high:
            p[0] = min(p[0], 940.0)
        return p, False
    s = (np.arange(K) / (K - 1)) ** 1.3
    pbot = {2: 740.0 + 90.0 * rng.random()}.get(kind, 900.0 + 100.0 * rng.random())
    if warm_high:
        pbot = min(pbot, 940.0)
    ptop = 40.0 + 110.0 * rng.random()
    if kind == 3:
        ptop = 310.0 + 140.0 * rng.random()
    if kind in (4, 5):
        ptop = (200.0, 250.0)[i % 2] if kind == 5 else 100.0
        p = np.round(pbot * (ptop / pbot) ** s)
        if kind == 4:
            t = (500.0, 700.0, 850.0)[i % 3]
            p[np.argmin(np.abs(p - t))] = t
        assert np.all(np.diff(p) < 0), p
        return p, True
    if kind == 6:
        t = (200.0, 250.0, 500.0)[i % 3]
        r = (t / pbot) ** (s[-1] - s[-2])
        ptop = t * (1.0 + 0.25 * (1.0 - r))
    if kind == 7:
        h = K // 2
        lo = pbot * (520.0 / pbot) ** (np.arange(h) / (h - 1))
        hi = 280.0 * (ptop / 280.0) ** (np.arange(K - h) / (K - h - 1))
        return np.concatenate([lo, hi]), False
    return pbot * (ptop / pbot) ** s, False


def draw_column(rng, K: int, i: int, shallow: bool = False) -> dict:
    kind, mm5 = i % 8, i % 3                      # mm5: 0 cold, 1 hot, 2 a cool surface well above sea level
    p, exact = level_pressures(rng, K, kind, i, mm5 == 2, shallow)
    ps = p[0] * (1.0 + 0.5 * (1.0 - p[1] / p[0]))
    zs = -8000.0 * np.log(ps / 1013.0)
    pif = np.concatenate([[ps], np.sqrt(p[1:] * p[:-1]), [p[-1] * np.sqrt(p[-1] / p[-2])]])
    zgrid = _quantize(zs + 7500.0 * np.log(ps / pif) + 30.0 * np.arange(K + 1), 16)
    zm = 0.5 * (zgrid[1:] + zgrid[:-1])
    if mm5 == 0:
        temp = np.maximum(265.0 - 6.5e-3 * (zm - zs), 205.0)
    else:
        temp = np.full(K, 300.0 if mm5 == 1 else iso.SLP_TC - 9.0) + 0.5 * rng.random()
    dry = (kind == 7) & (np.arange(K) >= K // 3)
    qv = np.where(dry, 1.0e-12, 0.018 * np.exp(-(zm - zs) / 2500.0) * (0.2 + 0.8 * rng.random(K)))
    exner = (p / 1000.0) ** (287.0 / 1004.5)
    c = {"zgrid": zgrid, "qv": _quantize(qv, 12), "exner": _quantize(exner, 14)}
    c["theta_m"] = _quantize(temp / c["exner"] * (1.0 + iso.RVORD * c["qv"]), 14)
    if exact:
        c["pressure_base"], c["pressure_p"] = p * 100.0, np.zeros(K)
    else:
        c["pressure_base"] = _quantize(0.97 * p * 100.0, 16)
        c["pressure_p"] = _quantize(p * 100.0 - c["pressure_base"], 12)
    c["relhum"] = _quantize(rng.random(K), 12)
    c["uzonal"] = _quantize(40.0 * (rng.random(K) - 0.3), 12)
    c["umeridional"] = _quantize(20.0 * (rng.random(K) - 0.5), 12)
    c["w"] = _quantize(2.0 * (rng.random(K + 1) - 0.5), 12)
    tot = (c["pressure_p"] + c["pressure_base"]) / 100.0
    assert np.all(np.diff(tot) < 0) and np.all(np.diff(zgrid) > 0), (K, i)
    return c


def draw(rng, K: int, fail: bool = False) -> dict:
    cols = [draw_column(rng, K, i, shallow=fail and i in (5, 17, 29)) for i in range(NCOL)]
    c = {n: np.stack([col[n] for col in cols]) for n in CELL_IN}
    # the garbage cell's pressures: a level set of their own, read through cellsOnVertex
    g = draw_column(rng, K, 0)
    for n in ("pressure_p", "pressure_base"):
        c[n + "_img"] = np.concatenate([c[n], g[n][None, :]])
    cov = np.stack([rng.choice(NCOL, size=3, replace=False) for _ in range(NVERT)]).astype(np.int32)
    cov[::8, 2] = NCOL                                  # every eighth vertex touches the garbage cell
    c["cellsOnVertex"] = cov
    kite = _quantize(1.0e8 * (0.5 + rng.random((NVERT, 3))), 12)
    c["kiteAreasOnVertex"] = kite
    c["areaTriangle"] = _quantize(kite.sum(axis=1), 12)
    c["vorticity"] = _quantize(1.0e-4 * (rng.random((NVERT, K)) - 0.5), 12)
    return c


def margins(host: dict) -> np.ndarray:
    """Per column: the least relative distance of a transcendental operand from what it is compared with."""
    info = host["info"]
    return np.minimum(info["top_margin"], info["slp"]["margin"])


def coverage(host: dict, vert: dict) -> dict:
    """Columns per branch (the fixture needs MIN_COLUMNS of each, for every K)."""
    info = host["info"]
    m, t, ifc, zi = info["mass"], info["t_isobaric"], info["iface"], info["z_isobaric"]
    col = lambda a: int(np.count_nonzero(np.any(a, axis=1)))  # noqa: E731
    cov = {"interior": col(m["branch"] == iso.INTERIOR), "above_top": col(m["branch"] == iso.ABOVE_TOP),
           "below_ground": col(m["branch"] == iso.BELOW_GROUND), "equal_lower": col(m["equal_lower"]),
           "equal_top": col(m["branch"] == iso.EQUAL_TOP),
           "iface_interior": col(ifc["branch"] == iso.INTERIOR), "iface_above_top": col(ifc["branch"] == iso.ABOVE_TOP),
           "iface_below_ground": col(ifc["branch"] == iso.BELOW_GROUND),
           "top_interface_bracket": col((ifc["branch"] == iso.INTERIOR) & ifc["uses_top"]),
           "t_iso_equal_lower": col(t["equal_lower"]), "z_iso_interior": col(zi["branch"] == iso.INTERIOR),
           "evp_clamp": col(info["evp_clamp"]),
           "vertex_interior": col(vert["info"]["vertex"]["branch"] == iso.INTERIOR)}
    lm = info["layer_mean"]
    cov["layer_boundary"] = int(np.count_nonzero(lm["branch"] == iso.LM_BOUNDARY))
    cov["layer_single"] = int(np.count_nonzero(lm["branch"] == iso.LM_SINGLE))
    cov["layer_general_with_middle"] = int(np.count_nonzero((lm["branch"] == iso.LM_GENERAL) & (lm["middle"] >= 1)))
    for name, code in (("mm5_tc", iso.MM5_TC), ("mm5_else_cold", iso.MM5_ELSE_COLD), ("mm5_else_hot", iso.MM5_ELSE_HOT)):
        cov[name] = int(np.count_nonzero(info["slp"]["mm5"] == code))
    return cov


def check_coverage(cov: dict, K: int):
    short = {name: count for name, count in cov.items() if count < MIN_COLUMNS}
    assert not short, f"K={K}: branches on fewer than {MIN_COLUMNS} columns: {short}"


def host_run(c: dict):
    host = iso.cells({n: c[n] for n in CELL_IN})
    vert = iso.vertices(c["pressure_p_img"], c["pressure_base_img"], c["vorticity"], c["cellsOnVertex"],
                        c["kiteAreasOnVertex"], c["areaTriangle"])
    return host, vert


def make(K: int, rng, fail: bool = False) -> dict:
    for _ in range(20):
        c = draw(rng, K, fail)
        host, _ = host_run(c)
        m = margins(host)
        if fail or np.all(m >= MIN_MARGIN):
            return c
    raise RuntimeError(f"K={K}: a margin below {MIN_MARGIN} after 20 redraws")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ref", default=os.environ.get("MPAS_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "isobaric_columns.npz"))
    args = ap.parse_args()
    rng = np.random.default_rng(20240917)
    data = {"K": np.array(KS, dtype=np.int32)}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(args.ref, tmp)
        for K, tag in [(K, f"K{K}") for K in KS] + [(4, "fail")]:
            fail = tag == "fail"
            c = make(K, rng, fail)
            host, vert = host_run(c)
            if fail:
                assert host["info"]["slp"]["fail"].sum() == 3 and not host["mslp"].any()
            else:
                cov = coverage(host, vert)
                check_coverage(cov, K)
                print(f"{tag}: {cov} min margin {margins(host).min():.3e}")
            ref = run_reference(exe, tmp, c)
            worst, exact = 0.0, 0
            for name, r in ref.items():
                h = vert[name] if name in vert else host[name]
                d = float(np.max(np.abs(h - r)) / max(np.max(np.abs(r)), 1e-300))
                worst = max(worst, d)
                exact += int(np.array_equal(h, r))
                data[f"ref_{name}_{tag}"] = r
            print(f"{tag}: restatement vs reference rel_linf {worst:.3e}, {exact} of {len(ref)} outputs bit for bit")
            for name in CELL_IN + VERT_IN + ("pressure_p_img", "pressure_base_img"):
                a32 = c[name].astype(np.float32)
                assert np.array_equal(a32.astype(np.float64), c[name]), name
                if name in ("pressure_p", "pressure_base"):
                    continue  # the images hold them
                data[f"{name}_{tag}"] = a32
            data[f"cellsOnVertex_{tag}"] = c["cellsOnVertex"].astype(np.int32)
    np.savez_compressed(args.out, **data)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()

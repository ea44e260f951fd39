#!/usr/bin/env python3
"""Generate tests/golden/pvbudget.npz: synthetic states through the reference's compiled PV budget.

Build machine only (it needs the reference tree and amdflang).  In a temporary directory the script cuts line
ranges out of the reference's unmodified diagnostics/pv_diagnostics.F at run time -- the helper and array
routines (:147-422, :826-1111) and calc_vertical_curl (:1113-1137) as they are, and the dtheta_dt_mix loop
(:1578-1584) and the two halves of calc_pvBudget's body (:1386-1485 and :1491-1529) inside driver subroutines
of our own, which declare the pool arrays as plain arrays and the raw tendencies as pointers, associated by
the source set, so that the body's `associated` tests work -- and compiles them with the oracle's flags
(amdflang -O2 -fdefault-real-8 -fdefault-double-8) next to a stand-in module of our own for RKIND, omega and
rvord.  Only data is written: neither the reference's source nor the binary leaves the directory.

Between the two halves the reference calls mpas_reconstruct (:1488-1490); here tenduX/Y/Z are handed in from
mpas_dycore.pvbudget.reconstruct with the coefficients of mpas_dycore.reconstruct, which
tests/golden/reconstruct_x1.642.npz pins to the reference bit for bit.  The two interp_pv calls of
interp_pvBudget_diagnostics run on a depv_dt_diab / depv_dt_fric handed in from the restatement -- equal to
the reference's below level K (asserted bit for bit), with the defined value at level K, where the reference
reads a local it never set (:997) -- on the restatement's ertel_pv and on an iLev_DT handed in: 0, 1, 2, K,
K + 1 and levels spread between (every value 0..K+1 where the mesh has cells enough), never 1 in the first
cell, where the reference's field0(iLev-1, iCell) would lie before the array.

Mesh: the level-1 icosahedral mesh of mesh.build_mesh (42 cells, 12 pentagons; the level-2 mesh's file would
pass 1 MiB), one block that owns every cell.  K in pvbudget.FIXTURE_KS: 4, and 65, one past the 64-level chunk.
Inputs are zero-mean perturbations of both signs (the tendencies), numbers float32 holds exactly, stored as
float32.  Three source sets (pvbudget.FIXTURE_SETS): all four raw tendencies, none, LW + CU.  Of a set other
than "all" only the fields that can differ are stored (pvbudget.FIXTURE_SET_FIELDS); the rest is asserted to
have the bits of "all".

The tool asserts that a curl summed in edgesOnVertex order, and a depv_dt_diab summed from mix down to lw,
each differ from the reference in at least one element (else it draws again with the next seed) and stores
the two shares.

    python tools/make_pvbudget_golden.py [--ref /path/to/reference] [--out tests/golden/pvbudget.npz]
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

from mpas_dycore import pv, pvbudget as pb  # noqa: E402

HELPERS, ARRAYS, CURL = (147, 422), (826, 1111), (1113, 1137)
MIX_BODY, HALF_1, HALF_2 = (1578, 1584), (1386, 1485), (1491, 1529)

STANDIN = """
module mpas_constants
   implicit none
   integer, parameter :: RKIND = selected_real_kind(12)
   real (kind=RKIND), parameter :: omega = 7.29212e-5
   real (kind=RKIND), parameter :: rgas = 287.0, rv = 461.6
   real (kind=RKIND), parameter :: rvord = rv/rgas
end module mpas_constants
"""

MODULE_HEAD = """
module pvb_cut
   use mpas_constants
   implicit none
contains
"""

MIX_HEAD = """
   subroutine pvb_mix_driver(nCells, nVertLevels, tend_theta_euler, scalars, dtheta_dt_mix)
      integer, intent(in) :: nCells, nVertLevels
      real (kind=RKIND), intent(in) :: tend_theta_euler(nVertLevels,nCells+1), scalars(1,nVertLevels,nCells+1)
      real (kind=RKIND), intent(out) :: dtheta_dt_mix(nVertLevels,nCells+1)
      integer :: iCell, k
      integer, parameter :: index_qv = 1
      dtheta_dt_mix(:,:) = 0.0
"""

BUDGET_HEAD = """
   end subroutine pvb_mix_driver

   subroutine pvb_budget_driver(nCellsSolve, nVertLevels, nCells, nEdges, nVertices, maxEdges, flags, nEdgesOnCell, &
                                cellsOnCell, cellsOnEdge, edgesOnCell, verticesOnCell, cellsOnVertex, verticesOnEdge, &
                                kiteAreasOnVertex, dvEdge, dcEdge, areaCell, areaTriangle, cellTangentPlane, &
                                localVerticalUnitVectors, edgeNormalVectors, zgrid, w, rho, vorticity, theta, &
                                uReconstructX, uReconstructY, uReconstructZ, lw_t, sw_t, bl_t, cu_t, mp_t, mix_t, &
                                tend_u_phys, tend_u_euler, rho_edge, tend_w_euler, tenduX, tenduY, tenduZ, &
                                depv_dt_lw, depv_dt_sw, depv_dt_bl, depv_dt_cu, depv_dt_mp, depv_dt_mix, depv_dt_diab, &
                                depv_dt_fric)
      integer, intent(in) :: nCellsSolve, nVertLevels, nCells, nEdges, nVertices, maxEdges, flags
      integer, intent(in) :: nEdgesOnCell(nCells+1), cellsOnCell(maxEdges,nCells+1), cellsOnEdge(2,nEdges+1)
      integer, intent(in) :: edgesOnCell(maxEdges,nCells+1), verticesOnCell(maxEdges,nCells+1), cellsOnVertex(3,nVertices+1)
      integer, intent(in) :: verticesOnEdge(2,nEdges+1)
      real (kind=RKIND), intent(in) :: kiteAreasOnVertex(3,nVertices+1), dvEdge(nEdges+1), dcEdge(nEdges+1)
      real (kind=RKIND), intent(in) :: areaCell(nCells+1), areaTriangle(nVertices+1)
      real (kind=RKIND), intent(in) :: cellTangentPlane(3,2,nCells+1), localVerticalUnitVectors(3,nCells+1)
      real (kind=RKIND), intent(in) :: edgeNormalVectors(3,nEdges+1), zgrid(nVertLevels+1,nCells+1), w(nVertLevels+1,nCells+1)
      real (kind=RKIND), intent(in) :: rho(nVertLevels,nCells+1), vorticity(nVertLevels,nVertices+1), theta(nVertLevels,nCells+1)
      real (kind=RKIND), intent(in) :: uReconstructX(nVertLevels,nCells+1), uReconstructY(nVertLevels,nCells+1)
      real (kind=RKIND), intent(in) :: uReconstructZ(nVertLevels,nCells+1)
      real (kind=RKIND), intent(in), target :: lw_t(nVertLevels,nCells+1), sw_t(nVertLevels,nCells+1)
      real (kind=RKIND), intent(in), target :: bl_t(nVertLevels,nCells+1), cu_t(nVertLevels,nCells+1)
      real (kind=RKIND), intent(in), target :: mp_t(nVertLevels,nCells+1), mix_t(nVertLevels,nCells+1)
      real (kind=RKIND), intent(inout) :: tend_u_phys(nVertLevels,nEdges+1), tend_w_euler(nVertLevels+1,nCells+1)
      real (kind=RKIND), intent(in) :: tend_u_euler(nVertLevels,nEdges+1), rho_edge(nVertLevels,nEdges+1)
      real (kind=RKIND), intent(in) :: tenduX(nVertLevels,nCells+1), tenduY(nVertLevels,nCells+1), tenduZ(nVertLevels,nCells+1)
      real (kind=RKIND), intent(out) :: depv_dt_lw(nVertLevels,nCells+1), depv_dt_sw(nVertLevels,nCells+1)
      real (kind=RKIND), intent(out) :: depv_dt_bl(nVertLevels,nCells+1), depv_dt_cu(nVertLevels,nCells+1)
      real (kind=RKIND), intent(out) :: depv_dt_mp(nVertLevels,nCells+1), depv_dt_mix(nVertLevels,nCells+1)
      real (kind=RKIND), intent(out) :: depv_dt_diab(nVertLevels,nCells+1), depv_dt_fric(nVertLevels,nCells+1)
      real (kind=RKIND), dimension(:,:), pointer :: rthblten, rthcuten, rthratenlw, rthratensw, dtheta_dt_mp, dtheta_dt_mix
      real (kind=RKIND), dimension(:,:), allocatable :: varVerts
      real (kind=RKIND), dimension(3) :: gradxu, gradtheta, gradxf
      integer :: iCell, k, iEdge
      nullify(rthblten, rthcuten, rthratenlw, rthratensw)
      if (iand(flags, 2) /= 0) rthratenlw => lw_t
      if (iand(flags, 4) /= 0) rthratensw => sw_t
      if (iand(flags, 8) /= 0) rthblten => bl_t
      if (iand(flags, 16) /= 0) rthcuten => cu_t
      dtheta_dt_mp => mp_t
      dtheta_dt_mix => mix_t
      allocate(varVerts(nVertLevels,nVertices+1))
      depv_dt_lw(:,:) = 0.0
      depv_dt_sw(:,:) = 0.0
      depv_dt_bl(:,:) = 0.0
      depv_dt_cu(:,:) = 0.0
      depv_dt_mp(:,:) = 0.0
      depv_dt_mix(:,:) = 0.0
      depv_dt_fric(:,:) = 0.0
"""

DRIVER = """
      deallocate(varVerts)
   end subroutine pvb_budget_driver
end module pvb_cut

program pvb_columns
   use pvb_cut
   implicit none
   integer(4) :: nC, nE, nV, K, me, flags
   integer(4), allocatable :: noc(:), coc(:,:), coe(:,:), eoc(:,:), voc(:,:), cov(:,:), voe(:,:), ilev(:)
   real(8), allocatable :: kite(:,:), dv(:), dc(:), area(:), areat(:), ctp(:,:,:), lv(:,:), env(:,:), lat(:)
   real(8), allocatable :: zgrid(:,:), w(:,:), rho(:,:), vort(:,:), theta(:,:), ux(:,:), uy(:,:), uz(:,:), qv(:,:,:)
   real(8), allocatable :: lw(:,:), sw(:,:), bl(:,:), cu(:,:), mp(:,:), tte(:,:), mix(:,:)
   real(8), allocatable :: tup(:,:), tue(:,:), rhoe(:,:), twe(:,:), tx(:,:), ty(:,:), tz(:,:)
   real(8), allocatable :: d(:,:,:), epv_in(:,:), diab_in(:,:), fric_in(:,:), o(:)
   integer :: j
   open(10, file='in.bin', access='stream', form='unformatted', status='old')
   read(10) nC, nE, nV, K, me, flags
   allocate(noc(nC+1), coc(me,nC+1), coe(2,nE+1), eoc(me,nC+1), voc(me,nC+1), cov(3,nV+1), voe(2,nE+1), ilev(nC+1))
   allocate(kite(3,nV+1), dv(nE+1), dc(nE+1), area(nC+1), areat(nV+1), ctp(3,2,nC+1), lv(3,nC+1), env(3,nE+1), lat(nC+1))
   allocate(zgrid(K+1,nC+1), w(K+1,nC+1), rho(K,nC+1), vort(K,nV+1), theta(K,nC+1), ux(K,nC+1), uy(K,nC+1), uz(K,nC+1))
   allocate(qv(1,K,nC+1), lw(K,nC+1), sw(K,nC+1), bl(K,nC+1), cu(K,nC+1), mp(K,nC+1), tte(K,nC+1), mix(K,nC+1))
   allocate(tup(K,nE+1), tue(K,nE+1), rhoe(K,nE+1), twe(K+1,nC+1), tx(K,nC+1), ty(K,nC+1), tz(K,nC+1))
   allocate(d(K,nC+1,8), epv_in(K,nC+1), diab_in(K,nC+1), fric_in(K,nC+1), o(nC))
   read(10) noc, coc, coe, eoc, voc, cov, voe, ilev
   read(10) kite, dv, dc, area, areat, ctp, lv, env, lat
   read(10) zgrid, w, rho, vort, theta, ux, uy, uz, qv
   read(10) lw, sw, bl, cu, mp, tte, tup, tue, rhoe, twe, tx, ty, tz
   read(10) epv_in, diab_in, fric_in
   close(10)
   call pvb_mix_driver(nC, K, tte, qv, mix)
   call pvb_budget_driver(nC, K, nC, nE, nV, me, flags, noc, coc, coe, eoc, voc, cov, voe, kite, dv, dc, area, areat, ctp, &
                          lv, env, zgrid, w, rho, vort, theta, ux, uy, uz, lw, sw, bl, cu, mp, mix, tup, tue, rhoe, twe, &
                          tx, ty, tz, d(:,:,1), d(:,:,2), d(:,:,3), d(:,:,4), d(:,:,5), d(:,:,6), d(:,:,7), d(:,:,8))
   open(11, file='out.bin', access='stream', form='unformatted', status='replace')
   write(11) mix(:,1:nC)
   do j = 1, 8
      write(11) d(:,1:nC,j)
   end do
   call interp_pv(nC, K, 2.0_8, lat, epv_in, diab_in, o, -99999.0_8, ilev)
   write(11) o
   call interp_pv(nC, K, 2.0_8, lat, epv_in, fric_in, o, -99999.0_8, ilev)
   write(11) o
   close(11)
end program pvb_columns
"""


def build_reference(ref: str, tmp: str) -> str:
    src = os.path.join(ref, "src", "core_atmosphere", "diagnostics", "pv_diagnostics.F")
    lines = open(src).read().split("\n")
    cut = lambda r: "\n".join(lines[r[0] - 1:r[1]]) + "\n"  # noqa: E731
    open(os.path.join(tmp, "standin.f90"), "w").write(STANDIN)
    open(os.path.join(tmp, "pvb_cut.f90"), "w").write(MODULE_HEAD + cut(HELPERS) + cut(ARRAYS) + cut(CURL) + MIX_HEAD +
                                                       cut(MIX_BODY) + BUDGET_HEAD + cut(HALF_1) + cut(HALF_2) + DRIVER)
    exe = os.path.join(tmp, "pvb_columns")
    flags = ["-O2", "-fdefault-real-8", "-fdefault-double-8", "-ffree-form"]
    subprocess.run(["amdflang", *flags, "-c", "standin.f90"], check=True, cwd=tmp)
    subprocess.run(["amdflang", *flags, "pvb_cut.f90", "standin.o", "-o", exe], check=True, cwd=tmp)
    return exe


def _img(a, garbage=0):
    """Element-major (n, ...) -> the Fortran image with its garbage slot."""
    a = np.asarray(a)
    pad = np.full((1,) + a.shape[1:], garbage, dtype=a.dtype)
    return np.ascontiguousarray(np.concatenate([a, pad], axis=0))


def run_reference(exe: str, tmp: str, m: dict, f: dict, flags: int, host: dict, ilev) -> dict:
    nC, nE, nV, me = m["nCells"], m["nEdges"], m["nVertices"], m["maxEdges"]
    K = host["theta"].shape[1]
    one = lambda name, n: _img(np.where(np.asarray(m[name]) >= 0, np.asarray(m[name]) + 1, n + 1).astype(np.int32), n + 1)  # noqa: E731
    r8 = lambda a: _img(np.asarray(a, dtype=np.float64)).tobytes()  # noqa: E731
    with open(os.path.join(tmp, "in.bin"), "wb") as fh:
        fh.write(np.array([nC, nE, nV, K, me, flags], dtype=np.int32).tobytes())
        fh.write(_img(np.asarray(m["nEdgesOnCell"], dtype=np.int32)).tobytes())
        for name, n in (("cellsOnCell", nC), ("cellsOnEdge", nC), ("edgesOnCell", nE), ("verticesOnCell", nV),
                        ("cellsOnVertex", nC), ("verticesOnEdge", nV)):
            fh.write(one(name, n).tobytes())
        fh.write(_img(np.asarray(ilev, dtype=np.int32)).tobytes())
        for name in ("kiteAreasOnVertex", "dvEdge", "dcEdge", "areaCell", "areaTriangle", "cellTangentPlane",
                     "localVerticalUnitVectors", "edgeNormalVectors", "latCell"):
            fh.write(r8(m[name]))
        for a in (f["zgrid"], f["w"], host["rho"], f["vorticity"], host["theta"], f["uReconstructX"], f["uReconstructY"],
                  f["uReconstructZ"], f["qv"]):
            fh.write(r8(a))
        for a in (f["rthratenlw"], f["rthratensw"], f["rthblten"], f["rthcuten"], f["dtheta_dt_mp"], f["tend_theta_euler"],
                  f["tend_u_phys"], f["tend_u_euler"], f["rho_edge"], f["tend_w_euler"], host["tenduX"], host["tenduY"],
                  host["tenduZ"]):
            fh.write(r8(a))
        for a in (host["ertel_pv"], host["depv_dt_diab"], host["depv_dt_fric"]):
            fh.write(r8(a))
    subprocess.run([exe], check=True, cwd=tmp)
    raw = np.fromfile(os.path.join(tmp, "out.bin"), dtype=np.float64)
    out, pos = {}, 0
    for name in ("dtheta_dt_mix",) + pb.OUT_3D:
        out[name] = raw[pos:pos + nC * K].reshape(nC, K).copy()
        pos += nC * K
    for name in pb.OUT_2D:
        out[name] = raw[pos:pos + nC].copy()
        pos += nC
    assert pos == raw.size, (pos, raw.size)
    return out


def _q(a, step):
    """Multiples of `step` (a power of two), exact in float32."""
    q = np.round(np.asarray(a, dtype=np.float64) / step) * step
    assert np.array_equal(q.astype(np.float32).astype(np.float64), q)
    return q


def _zero_mean(rng, shape, amp, step):
    """Both signs, the mean taken out before the rounding to float32's grid."""
    a = amp * (2.0 * rng.random(shape) - 1.0)
    a = _q(a - a.mean(), step)
    assert (a > 0).any() and (a < 0).any()
    return a


def draw(m: dict, K: int, rng) -> dict:
    """One state: a stable stratification with perturbed winds, and tendencies of both signs."""
    nC, nE, nV = m["nCells"], m["nEdges"], m["nVertices"]
    dz = _q(15000.0 / K, 0.125) * rng.choice([0.75, 1.0, 1.25], size=nC)
    zgrid = _q(50.0 * rng.integers(0, 40, size=nC)[:, None] + dz[:, None] * np.arange(K + 1)[None, :], 1.0 / 32)
    rho_col = 2.0 ** (-4.0 * np.arange(K) / K)
    rho = _q(rho_col[None, :] * (1.0 + 0.05 * (2.0 * rng.random((nC, K)) - 1.0)), 2.0 ** -12)
    qv = _q(0.012 * np.exp(-np.arange(K) * (15000.0 / K) / 2500.0)[None, :] * rng.random((nC, K)), 2.0 ** -16)
    theta = 290.0 + 4.0e-3 * 0.5 * (zgrid[:, 1:] + zgrid[:, :-1]) + 2.0 * (2.0 * rng.random((nC, K)) - 1.0)
    wind = lambda amp, step: _q(amp * (2.0 * rng.random(nC) - 1.0)[:, None] + 0.25 * (2.0 * rng.random((nC, K)) - 1.0), step)  # noqa: E731
    f = dict(zgrid=zgrid, theta_m=_q(theta * (1.0 + pv.RVORD * qv), 2.0 ** -10), qv=qv, rho_zz=rho,
             w=_q(0.25 * (2.0 * rng.random((nC, K + 1)) - 1.0), 2.0 ** -6),
             uReconstructX=wind(8.0, 0.125), uReconstructY=wind(8.0, 0.125), uReconstructZ=wind(4.0, 0.125),
             uReconstructZonal=wind(10.0, 0.25), uReconstructMeridional=wind(6.0, 0.25),
             vorticity=_q(1.0e-5 * (2.0 * rng.random((nV, K)) - 1.0), 2.0 ** -20))
    for name in pb.FIXTURE_CELL_FIELDS[:6]:                          # K / s
        f[name] = _zero_mean(rng, (nC, K), 1.0e-3, 2.0 ** -24)
    f["tend_w_euler"] = _zero_mean(rng, (nC, K + 1), 1.0e-2, 2.0 ** -20)
    f["tend_u_phys"] = _zero_mean(rng, (nE, K), 1.0e-3, 2.0 ** -24)
    f["tend_u_euler"] = _zero_mean(rng, (nE, K), 1.0e-2, 2.0 ** -20)
    f["rho_edge"] = _q(rho_col[None, :] * (1.0 + 0.05 * (2.0 * rng.random((nE, K)) - 1.0)), 2.0 ** -12)
    return f


def handed_ilev(nC: int, K: int) -> np.ndarray:
    """0, 1, 2, K, K + 1 and levels spread over 2..K; every value of 0..K+1 where there are cells enough.  The
    first cell gets 0."""
    if nC >= K + 2:
        v = np.arange(nC) % (K + 2)
    else:
        v = np.concatenate([[0, 1, 2, K, K + 1], np.round(np.linspace(2, K, nC - 5))])
    v = v.astype(np.int32)
    assert v[0] != 1 and {0, 1, 2, K, K + 1} <= set(v.tolist())
    return v


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ref", default=os.environ.get("MPAS_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pvbudget.npz"))
    args = ap.parse_args()
    m = pb.fixture_mesh()
    nC = m["nCells"]
    data = {"K": np.array(pb.FIXTURE_KS, dtype=np.int32), "mesh_level": np.array(pb.FIXTURE_MESH_LEVEL, dtype=np.int32)}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(args.ref, tmp)
        for K in pb.FIXTURE_KS:
            ilev = handed_ilev(nC, K)
            for seed in range(20261021, 20261041):
                f = draw(m, K, np.random.default_rng(seed + K))
                refs = {}
                for name, flags in pb.FIXTURE_SETS.items():
                    host = pb.fixture_driver(m, f, flags, ilev=ilev)
                    ref = refs[name] = run_reference(exe, tmp, m, f, flags, host, ilev)
                    for n in pb.OUT_3D:
                        assert np.array_equal(ref[n][:, :K - 1], host[n][:, :K - 1]), \
                            f"K={K} {name}: the restatement's {n} differs from the reference's below level K"
                    for n in pb.OUT_2D + ("dtheta_dt_mix",):
                        assert np.array_equal(ref[n], host[n]), f"K={K} {name}: the restatement's {n} differs"
                    print(f"K{K} {name}: restatement vs reference bit for bit below level K, both _pv fields and "
                          f"dtheta_dt_mix: True")
                below = lambda a: a[:, :K - 1]  # noqa: E731
                by_slot = pb.fixture_driver(m, f, pb.ALL, ilev=ilev, curl_order="edgesOnVertex")
                reverse = pb.fixture_driver(m, f, pb.ALL, ilev=ilev, reverse_sum=True)
                share_curl = float(np.mean(below(by_slot["depv_dt_fric"]) != below(refs["all"]["depv_dt_fric"])))
                share_sum = float(np.mean(below(reverse["depv_dt_diab"]) != below(refs["all"]["depv_dt_diab"])))
                if share_curl > 0 and share_sum > 0:
                    break
            else:
                raise RuntimeError(f"K={K}: the order variants never differed")
            print(f"K{K}: share of depv_dt_fric that a curl in edgesOnVertex order changes {share_curl:.3f}, of "
                  f"depv_dt_diab that a reversed sum changes {share_sum:.3f}")
            for name in pb.FIXTURE_FIELDS:
                a32 = f[name].astype(np.float32)
                assert np.array_equal(a32.astype(np.float64), f[name]), name
                data[f"{name}_K{K}"] = a32
            data[f"iLev_DT_K{K}"] = ilev
            data[f"share_curl_K{K}"], data[f"share_sum_K{K}"] = np.array(share_curl), np.array(share_sum)
            for name, ref in refs.items():
                for n in pb.OUT_3D + pb.OUT_2D + ("dtheta_dt_mix",):
                    a = below(ref[n]).copy() if n in pb.OUT_3D else ref[n]
                    if name == "all" or n in pb.FIXTURE_SET_FIELDS:
                        data[f"ref_{name}_{n}_K{K}"] = a
                    else:
                        assert np.array_equal(a, data[f"ref_all_{n}_K{K}"]), (name, n)
    np.savez_compressed(args.out, **data)
    size = os.path.getsize(args.out)
    assert size < 1 << 20, size
    print(f"wrote {args.out} ({size} bytes)")


if __name__ == "__main__":
    main()

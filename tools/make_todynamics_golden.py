#!/usr/bin/env python3
"""Generate tests/golden/todynamics.npz: random tendencies through the reference's compiled physics_get_tend.

Build machine only (it needs the reference tree and amdflang).  In a temporary directory the script cuts
physics_get_tend_work (physics/mpas_atmphys_todynamics.F:265-434) and the loop of tend_toEdges (:494-510) out
of the unmodified reference at run time and compiles them with the oracle's flags (amdflang -O2
-fdefault-real-8 -fdefault-double-8) next to a stand-in of our own: RKIND, StrKIND, R_d, R_v, nVertLevels,
num_scalars, empty block_type / mpas_pool_type, and a tend_toEdges head written here (explicit-shape arguments,
the mesh arrays from the stand-in module, no halo exchange).  The driver zeroes the outputs as physics_get_tend does (:176-182).
Only data is written: neither the reference's source nor the binary leaves the directory.

Mesh: mesh.build_mesh(1) (42 cells, 12 of them pentagons, 120 edges) as one block that owns every element,
east / north from todynamics.init_dirs, edgeNormalVectors from reconstruct.initialize_vectors.  num_scalars = 7
(qv qc qr qi qs qg ni), K = 4 and 5.  Inputs are random, of realistic magnitude and of both signs.  The scheme
sets are todynamics.FIXTURE_SETS.  check_sensitivity asserts what makes the fixture tell a changed association
apart; tests/test_todynamics_host.py re-checks it on the committed file.

    python tools/make_todynamics_golden.py [--ref /path/to/reference] [--out tests/golden/todynamics.npz]
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

from mpas_dycore import todynamics as T  # noqa: E402

WORK, EDGE_LOOP = (265, 434), (494, 510)

STANDIN = """
module mpas_atm_dimensions
   implicit none
   integer :: nVertLevels, num_scalars
end module mpas_atm_dimensions

module todyn_standin
   implicit none
   integer, parameter :: RKIND = selected_real_kind(12)
   integer, parameter :: StrKIND = 512
   real (kind=RKIND), parameter :: R_d = 287.0, R_v = 461.6
   type block_type
   end type block_type
   type mpas_pool_type
   end type mpas_pool_type
   ! the mesh arrays the projection loop reads, under the names it uses; filled by the driver
   integer :: nCellsAll, nEdgesAll
   integer, allocatable :: cellsOnEdge(:,:)
   real (kind=RKIND), allocatable :: east(:,:), north(:,:), edgeNormalVectors(:,:)
end module todyn_standin
"""

MODULE_HEAD = """
module todyn_cut
   use todyn_standin
   implicit none
contains
"""

# our own head for the cut loop: explicit-shape arguments under the names the loop reads, the mesh arrays
# from the stand-in module, no halo exchange; the first two arguments are the empty stand-in types
EDGES_HEAD = """
   subroutine tend_toEdges(unused_block, unused_pool, Ux_tend_halo, Uy_tend_halo, U_tend)
      use mpas_atm_dimensions, only : nVertLevels
      type (block_type), intent(in) :: unused_block
      type (mpas_pool_type), intent(in) :: unused_pool
      real (kind=RKIND), intent(in) :: Ux_tend_halo(nVertLevels, nCellsAll + 1)
      real (kind=RKIND), intent(in) :: Uy_tend_halo(nVertLevels, nCellsAll + 1)
      real (kind=RKIND), intent(inout) :: U_tend(nVertLevels, nEdgesAll + 1)
      integer :: nEdges, iEdge, cell1, cell2
      nEdges = nEdgesAll
"""

DRIVER = """
   end subroutine
end module todyn_cut

program todyn_driver
   use mpas_atm_dimensions
   use todyn_cut
   implicit none
   integer(4) :: nC, nE, K, ns, idx(6)
   character(len=StrKIND) :: pbl, cu, lw, sw
   type(block_type) :: block
   type(mpas_pool_type) :: mesh
   real(8), allocatable :: rublten(:,:), rvblten(:,:), rthblten(:,:), rqvblten(:,:), rqcblten(:,:), rqiblten(:,:)
   real(8), allocatable :: rniblten(:,:), rucuten(:,:), rvcuten(:,:), rthcuten(:,:), rqvcuten(:,:), rqccuten(:,:)
   real(8), allocatable :: rqrcuten(:,:), rqicuten(:,:), rqscuten(:,:), rthratenlw(:,:), rthratensw(:,:)
   real(8), allocatable :: mass(:,:), mass_edge(:,:), theta_m(:,:), scalars(:,:,:), tend_u_phys(:,:)
   real(8), allocatable :: rublten_Edge(:,:), rucuten_Edge(:,:), tend_u(:,:), tend_th(:,:), tend_scalars(:,:,:)
   real(8), allocatable :: tend_theta(:,:), tend_rho(:,:), dummy(:,:)
   open(12, file='schemes.txt', status='old')
   read(12,'(A)') pbl
   read(12,'(A)') cu
   read(12,'(A)') lw
   read(12,'(A)') sw
   close(12)
   open(10, file='in.bin', access='stream', form='unformatted', status='old')
   read(10) nC, nE, K, ns, idx
   nVertLevels = K
   num_scalars = ns
   nCellsAll = nC
   nEdgesAll = nE
   allocate(cellsOnEdge(2,nE+1), east(3,nC+1), north(3,nC+1), edgeNormalVectors(3,nE+1))
   allocate(rublten(K,nC+1), rvblten(K,nC+1), rthblten(K,nC+1), rqvblten(K,nC+1), rqcblten(K,nC+1), rqiblten(K,nC+1))
   allocate(rniblten(K,nC+1), rucuten(K,nC+1), rvcuten(K,nC+1), rthcuten(K,nC+1), rqvcuten(K,nC+1), rqccuten(K,nC+1))
   allocate(rqrcuten(K,nC+1), rqicuten(K,nC+1), rqscuten(K,nC+1), rthratenlw(K,nC+1), rthratensw(K,nC+1))
   allocate(mass(K,nC+1), mass_edge(K,nE+1), theta_m(K,nC+1), scalars(ns,K,nC+1), tend_u_phys(K,nE+1))
   allocate(rublten_Edge(K,nE+1), rucuten_Edge(K,nE+1), tend_u(K,nE+1), tend_th(K,nC+1), tend_scalars(ns,K,nC+1))
   allocate(tend_theta(K,nC+1), tend_rho(K,nC+1), dummy(K,nC+1))
   read(10) cellsOnEdge, east, north, edgeNormalVectors
   read(10) rublten, rvblten, rthblten, rqvblten, rqcblten, rqiblten, rniblten, rucuten, rvcuten, rthcuten, rqvcuten
   read(10) rqccuten, rqrcuten, rqicuten, rqscuten, rthratenlw, rthratensw
   read(10) mass, mass_edge, theta_m, scalars, tend_u_phys
   close(10)
   rublten_Edge = 0.0
   rucuten_Edge = 0.0
   dummy = 0.0
   tend_th = 0.0                  ! physics_get_tend :176-182
   tend_scalars(:,:,:) = 0.0
   tend_u(:,:) = 0.0
   tend_theta(:,:) = 0.0
   tend_rho(:,:) = 0.0
   call physics_get_tend_work(block, mesh, nC, nE, nC, nE, 1, 1, pbl, cu, lw, sw, &
                              idx(1), idx(2), idx(3), idx(4), idx(5), idx(6), &
                              rublten, rvblten, mass_edge, rublten_Edge, tend_u, rucuten, rvcuten, rucuten_Edge, &
                              tend_th, tend_scalars, mass, rthblten, rqvblten, rqcblten, rqiblten, rniblten, &
                              rthcuten, rqvcuten, rqccuten, rqrcuten, rqicuten, rqscuten, rthratenlw, rthratensw, dummy, &
                              tend_u_phys, dummy, dummy, theta_m, scalars, tend_theta, dummy)
   open(11, file='out.bin', access='stream', form='unformatted', status='replace')
   write(11) tend_u, tend_theta, tend_rho, tend_scalars, rublten_Edge, rucuten_Edge, tend_u_phys
   close(11)
end program todyn_driver
"""


def build_reference(ref: str, tmp: str) -> str:
    src = os.path.join(ref, "src", "core_atmosphere", "physics", "mpas_atmphys_todynamics.F")
    lines = open(src).read().split("\n")
    cut = lambda r: "\n".join(lines[r[0] - 1:r[1]]) + "\n"  # noqa: E731
    open(os.path.join(tmp, "standin.f90"), "w").write(STANDIN)
    open(os.path.join(tmp, "todyn_cut.f90"), "w").write(MODULE_HEAD + cut(WORK) + EDGES_HEAD + cut(EDGE_LOOP) + DRIVER)
    exe = os.path.join(tmp, "todyn_driver")
    flags = ["-O2", "-fdefault-real-8", "-fdefault-double-8", "-ffree-form"]
    subprocess.run(["amdflang", *flags, "-c", "standin.f90"], check=True, cwd=tmp)
    subprocess.run(["amdflang", *flags, "todyn_cut.f90", "standin.o", "-o", exe], check=True, cwd=tmp)
    return exe


def _img(a, garbage=0):
    """Element-major (n, ...) -> the Fortran image with its garbage slot."""
    a = np.asarray(a)
    pad = np.full((1,) + a.shape[1:], garbage, dtype=a.dtype)
    return np.ascontiguousarray(np.concatenate([a, pad], axis=0))


def run_reference(exe: str, tmp: str, m: dict, name: str, raw: dict, state: dict) -> dict:
    """One scheme set through the compiled reference: its call(s), tend_u_phys carried from call to call."""
    pbl, cu, lw, sw, calls, no_qi = T.FIXTURE_SETS[name]
    nC, nE = m["nCells"], m["nEdges"]
    K, ns = state["scalars"].shape[1:]
    raw = dict(raw)
    if no_qi:  # the reference indexes with index_qi whatever it is: a zero tendency at a valid index
        raw["rqiblten"] = np.zeros_like(raw["rqiblten"])
    with open(os.path.join(tmp, "schemes.txt"), "w") as fh:
        fh.write("\n".join([pbl or "off", cu or "off", "rrtmg_lw" if lw else "off", "rrtmg_sw" if sw else "off"]) + "\n")
    idx = T.FIXTURE_INDICES
    tup = np.zeros((nE, K))
    out = {}
    for _ in range(calls):
        with open(os.path.join(tmp, "in.bin"), "wb") as fh:
            fh.write(np.array([nC, nE, K, ns] + [idx[n] + 1 for n in ("index_qv", "index_qc", "index_qr", "index_qi",
                                                                     "index_qs", "index_ni")], dtype=np.int32).tobytes())
            coe = np.asarray(m["cellsOnEdge"])
            fh.write(_img(np.where(coe >= 0, coe + 1, nC + 1).astype(np.int32), nC + 1).tobytes())
            for n in ("east", "north", "edgeNormalVectors"):
                fh.write(_img(np.asarray(m[n], dtype=np.float64)).tobytes())
            for n in T.RAW_CELL:
                fh.write(_img(raw[n]).tobytes())
            for n in T.FIXTURE_STATE:
                fh.write(_img(state[n]).tobytes())
            fh.write(_img(tup).tobytes())
        subprocess.run([exe], check=True, cwd=tmp)
        buf = np.fromfile(os.path.join(tmp, "out.bin"), dtype=np.float64)
        pos = 0
        for n, shape in (("tend_ru_physics", (nE + 1, K)), ("tend_rtheta_physics", (nC + 1, K)),
                         ("tend_rho_physics", (nC + 1, K)), ("scalars_tend", (nC + 1, K, ns)), ("rublten_Edge", (nE + 1, K)),
                         ("rucuten_Edge", (nE + 1, K)), ("tend_u_phys", (nE + 1, K))):
            cnt = int(np.prod(shape))
            a = buf[pos:pos + cnt].reshape(shape)
            assert not np.any(a[-1]), (name, n, "garbage slot written")
            out[n] = a[:-1].copy()
            pos += cnt
        assert pos == buf.size
        tup = out["tend_u_phys"]
    return out


def draw(m: dict, K: int, rng) -> tuple:
    """Random inputs of realistic magnitude and both signs: (raw, state)."""
    nC, nE, ns = m["nCells"], m["nEdges"], T.FIXTURE_NUM_SCALARS
    sym = lambda shape, amp: amp * (2.0 * rng.random(shape) - 1.0)  # noqa: E731
    amp = dict(rublten=2e-3, rvblten=2e-3, rucuten=1e-3, rvcuten=1e-3, rthblten=5e-4, rthcuten=8e-4, rthratenlw=3e-5,
               rthratensw=4e-5, rqvblten=2e-7, rqcblten=3e-8, rqiblten=1e-8, rniblten=50.0, rqvcuten=4e-7, rqccuten=5e-8,
               rqrcuten=4e-8, rqicuten=2e-8, rqscuten=2e-8)
    raw = {n: sym((nC, K), amp[n]) for n in T.RAW_CELL}
    rho = (1.1 * np.exp(-np.arange(K) / K * 2.0))[None, :] * (1.0 + sym((nC, K), 0.05))
    coe = np.asarray(m["cellsOnEdge"])
    scalars = np.abs(sym((nC, K, ns), 1.0)) * np.array([1.5e-2, 1e-4, 1e-4, 5e-5, 5e-5, 5e-5, 1e5])[None, None, :]
    state = dict(rho_zz=rho, rho_edge=0.5 * (rho[coe[:, 0]] + rho[coe[:, 1]]),
                 theta_m=(290.0 + 60.0 * np.arange(K) / K)[None, :] + sym((nC, K), 8.0), scalars=scalars)
    return raw, state


def sensitivity(m: dict, raw: dict, state: dict, ref: dict) -> dict:
    """Shares of the elements on which a restatement with one association changed differs from the reference,
    on the scheme set with every theta term and both projections."""
    name = "bl_mynn_cu_ntiedtke_lw_sw"
    share = lambda a, b: float(np.mean(a.view(np.int64) != b.view(np.int64)))  # noqa: E731
    r = ref[name]
    a = T.fixture_run(name, raw, state, m, T.variant_theta_m_right)["tend_rtheta_physics"]
    b = T.fixture_run(name, raw, state, m, T.variant_theta_sum_first)["tend_rtheta_physics"]
    c = T.fixture_run(name, raw, state, m, T.variant_dot_right)
    return dict(theta_m_right=share(a, r["tend_rtheta_physics"]), theta_sum_first=share(b, r["tend_rtheta_physics"]),
                dot_right=share(np.stack([c["rublten_Edge"], c["rucuten_Edge"]]),
                                np.stack([r["rublten_Edge"], r["rucuten_Edge"]])))


def check_sensitivity(s: dict, K: int):
    for n, v in s.items():
        assert v >= T.MIN_SENSITIVE_SHARE, (K, n, v)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ref", default=os.environ.get("MPAS_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "todynamics.npz"))
    args = ap.parse_args()
    rng = np.random.default_rng(20261021)
    m = T.fixture_mesh()
    data = {"K": np.array(T.FIXTURE_KS, dtype=np.int32), "mesh_level": np.array(T.FIXTURE_MESH_LEVEL, dtype=np.int32)}
    for n in T.FIXTURE_MESH:
        data[f"mesh_{n}"] = np.asarray(m[n])
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(args.ref, tmp)
        for K in T.FIXTURE_KS:
            raw, state = draw(m, K, rng)
            ref = {name: run_reference(exe, tmp, m, name, raw, state) for name in T.FIXTURE_SETS}
            for name in T.FIXTURE_SETS:
                host = T.fixture_run(name, raw, state, m)
                same = {n: T.same_bits(np.zeros_like(ref[name][n]) if host[n] is None else host[n], ref[name][n])
                        for n in T.FIXTURE_OUTPUTS}
                print(f"K{K} {name}: restatement vs reference bit for bit: {same}")
                assert all(same.values()), (K, name, same)
            s = sensitivity(m, raw, state, ref)
            print(f"K{K}: shares that differ with one association changed: {s}")
            check_sensitivity(s, K)
            for n, a in {**raw, **state}.items():
                data[f"{n}_K{K}"] = a
            for name in T.FIXTURE_SETS:
                for n in T.FIXTURE_OUTPUTS:
                    data[f"ref_{name}_{n}_K{K}"] = ref[name][n]
    np.savez_compressed(args.out, **data)
    size = os.path.getsize(args.out)
    print(f"wrote {args.out} ({size} bytes)")
    assert size < 1 << 20, size


if __name__ == "__main__":
    main()

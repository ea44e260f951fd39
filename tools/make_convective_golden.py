#!/usr/bin/env python3
"""Generate tests/golden/convective_columns.npz: synthetic columns through the reference's compiled
convective_diagnostics_compute and getcape.

Build machine only (it needs the reference tree and amdflang).  In a temporary directory the script cuts two
line ranges out of the reference's unmodified diagnostics/convective_diagnostics.F at run time -- the loops of
convective_diagnostics_compute (:361-472: temperature, dewpoint, the shear / helicity loop, the cape loop) and
column_height_value ... getthe (:528-1093) -- and wraps them into a generated module: the functions as they
are, the loops inside a driver subroutine that declares the reference's locals and takes theta_m, scalars,
exner, ... as plain arrays.  A small stand-in module of our own supplies RKIND, rvord, MPAS_LOG_ERR and a no-op
mpas_log_write.  Compiled with the oracle's flags (amdflang -O2 -fdefault-real-8 -fdefault-double-8) and run
on synthetic MPAS-level columns; inputs and outputs are stored.  Only data is written: neither the
reference's source nor the binary leaves the temporary directory.

For each K in KS: NCOL columns.  Inputs are numbers that float32 holds exactly, stored as float32.  With the
host restatement (mpas_dycore.convcompute) the script asserts what the inputs must exercise (check_coverage;
tests/test_convcompute_host.py re-checks it on the committed file) and that every column is stable: its
discrete decisions are the same when every exp / log / pow result is moved by +4 or -4 ulp (the others are
redrawn).  Within a small budget of draws it also looks for a column that trips getcape's `i > 100` exit; one
that does goes into a set "noconv".

    python tools/make_convective_golden.py [--ref /path/to/reference] [--out tests/golden/convective_columns.npz]
    python tools/make_convective_golden.py --time      # seconds per column of the compiled cut-out, no file
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpas-model_amd"))

from mpas_dycore import convcompute as cc  # noqa: E402

KS = (4, 26, 64, 150)
NCOL = 40
LOOPS = (361, 472)       # the loops of convective_diagnostics_compute
FUNCTIONS = (528, 1093)  # column_height_value, integral_zstaggered, integral_zpoint, getcape, getqvs, getqvi, getthe
NOCONV_BUDGET = 400

STANDIN = """
module conv_standin
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
end module conv_standin
"""

MODULE_HEAD = """
module conv_cut
   use conv_standin
   implicit none
contains
   subroutine conv_loops(nCells, nCellsSolve, nVertLevels, theta_m, scalars, exner, pressure_p, pressure_base, height, &
                         uzonal, umeridional, cape, cin, srh_0_1km, srh_0_3km, uzonal_surface, uzonal_1km, uzonal_6km, &
                         umeridional_surface, umeridional_1km, umeridional_6km, temperature_surface, dewpoint_surface)
      integer, intent(in) :: nCells, nCellsSolve, nVertLevels
      real (kind=RKIND), intent(in) :: theta_m(nVertLevels,nCells), scalars(1,nVertLevels,nCells), exner(nVertLevels,nCells)
      real (kind=RKIND), intent(in) :: pressure_p(nVertLevels,nCells), pressure_base(nVertLevels,nCells)
      real (kind=RKIND), intent(in) :: height(nVertLevels+1,nCells), uzonal(nVertLevels,nCells), umeridional(nVertLevels,nCells)
      real (kind=RKIND), dimension(nCells), intent(out) :: cape, cin, srh_0_1km, srh_0_3km, uzonal_surface, uzonal_1km, &
         uzonal_6km, umeridional_surface, umeridional_1km, umeridional_6km, temperature_surface, dewpoint_surface
      integer, parameter :: index_qv = 1
      logical, parameter :: need_cape = .true., need_cin = .true., need_srh_01km = .true., need_srh_03km = .true., &
         need_uzonal_1km = .true., need_uzonal_6km = .true., need_umerid_1km = .true., need_umerid_6km = .true.
      integer :: iCell, k, nVertLevelsP1
      real (kind=RKIND), parameter :: dev_motion = 7.5, z_bunker_bot = 0., z_bunker_top = 6000.
      real (kind=RKIND) :: u_storm, v_storm, u_srh_bot, v_srh_bot, u_srh_top, v_srh_top
      real (kind=RKIND) :: u_mean, v_mean, u_shear, v_shear, shear_magnitude
      real (kind=RKIND) :: b_term, cape_out, cin_out, evp
      real (kind=RKIND), dimension(:), allocatable :: dudz, dvdz, zp, zrel, srh, p_in, t_in, td_in
      real (kind=RKIND), dimension(:,:), allocatable :: temperature, dewpoint
      nVertLevelsP1 = nVertLevels + 1
      allocate(temperature(nVertLevels,nCells), dewpoint(nVertLevels,nCells))
      allocate(dudz(nVertLevels), dvdz(nVertLevels), zp(nVertLevels), zrel(nVertLevels+1), srh(nVertLevels+1))
      allocate(p_in(nVertLevels), t_in(nVertLevels), td_in(nVertLevels))
"""

DRIVER = """
   end subroutine conv_loops
"""

PROGRAM = """
end module conv_cut

program convective_columns
   use conv_cut
   implicit none
   integer(4) :: n, K, nrep, a, irep
   integer(8) :: c0, c1, rate
   real(8), allocatable :: f(:,:,:), height(:,:), scalars(:,:,:), o(:,:)
   open(10, file='in.bin', access='stream', form='unformatted', status='old')
   read(10) n, K, nrep
   allocate(f(K,n,7), height(K+1,n), scalars(1,K,n), o(n,12))
   do a = 1, 7
      read(10) f(:,:,a)      ! theta_m, qv, exner, pressure_p, pressure_base, uzonal, umeridional
   end do
   read(10) height
   close(10)
   scalars(1,:,:) = f(:,:,2)
   call system_clock(c0, rate)
   do irep = 1, nrep
      call conv_loops(n, n, K, f(:,:,1), scalars, f(:,:,3), f(:,:,4), f(:,:,5), height, f(:,:,6), f(:,:,7), &
                      o(:,1), o(:,2), o(:,3), o(:,4), o(:,5), o(:,6), o(:,7), o(:,8), o(:,9), o(:,10), o(:,11), o(:,12))
   end do
   call system_clock(c1)
   open(11, file='out.bin', access='stream', form='unformatted', status='replace')
   write(11) o
   write(11) real(c1 - c0, 8) / real(rate, 8)
   close(11)
end program convective_columns
"""


def build_reference(ref: str, tmp: str) -> str:
    src = os.path.join(ref, "src", "core_atmosphere", "diagnostics", "convective_diagnostics.F")
    lines = open(src).read().split("\n")
    cut = lambda r: "\n".join(lines[r[0] - 1:r[1]]) + "\n"  # noqa: E731
    open(os.path.join(tmp, "standin.f90"), "w").write(STANDIN)
    open(os.path.join(tmp, "conv_cut.f90"), "w").write(MODULE_HEAD + cut(LOOPS) + DRIVER + cut(FUNCTIONS) + PROGRAM)
    exe = os.path.join(tmp, "convective_columns")
    flags = ["-O2", "-fdefault-real-8", "-fdefault-double-8", "-ffree-form"]
    subprocess.run(["amdflang", *flags, "-c", "standin.f90"], check=True, cwd=tmp)
    subprocess.run(["amdflang", *flags, "conv_cut.f90", "standin.o", "-o", exe], check=True, cwd=tmp)
    return exe


def run_reference(exe: str, tmp: str, c: dict, nrep: int = 1):
    n, K = c["theta_m"].shape
    with open(os.path.join(tmp, "in.bin"), "wb") as fh:
        fh.write(np.array([n, K, nrep], dtype=np.int32).tobytes())
        for name in cc.INPUTS:
            fh.write(np.ascontiguousarray(c[name], dtype=np.float64).tobytes())
    subprocess.run([exe], check=True, cwd=tmp)
    raw = np.fromfile(os.path.join(tmp, "out.bin"), dtype=np.float64)
    assert raw.size == 12 * n + 1, raw.size
    o = raw[:-1].reshape(12, n)
    return {name: o[i].copy() for i, name in enumerate(cc.WRITTEN)}, float(raw[-1])


def interfaces(rng, K: int, kind: int, i: int) -> np.ndarray:
    """Interface heights of one column (m, the ground first).  The column's top: about 21 km (the top level
    above 100 hPa: the 100 hPa stop) or about 13 km (the ascent reaches the top level), 5 km on the shallow
    kind (zp(K) < 6000).  K = 150 has thin layers (5 m: less than 100 Pa, nloop = 1) under thick ones; kind 6
    has a first layer thicker than 2 km (zp(1) > 1000)."""
    zs = 5800.0 if kind == 3 else 50.0 + 700.0 * rng.random()
    ztop = 5000.0 if kind == 5 else (21000.0, 13000.0)[i % 2] - (zs if kind == 3 else 0.0) + 600.0 * rng.random()
    s = np.arange(K + 1) / K
    if K == 150:
        thin = 5.0 * np.arange(41)
        z = np.concatenate([thin, thin[-1] + (ztop - thin[-1]) * (np.arange(1, K - 39) / (K - 40)) ** 1.2])
    else:
        z = ztop * s ** (1.0 if K == 4 else 1.4)
    if kind == 6 and K > 4:
        z[1:] = 2200.0 + (ztop - 2200.0) * (np.arange(K) / (K - 1)) ** 1.2
    return zs + z


def draw(rng, K: int) -> dict:
    """NCOL columns by kind (i % 8): 0, 4 unstable under a stable boundary layer (cape and cin); 1 stable and
    dry (cape = 0); 2 a dry surface layer under the moist one (kmax > 1); 3 a mountain column, p(1) < 500 hPa;
    5 shallow (the top below 6000 m); 6 a thick first layer; 7 calm (the shear floor)."""
    z = np.stack([interfaces(rng, K, i % 8, i) for i in range(NCOL)])
    kind = np.arange(NCOL) % 8
    u = rng.random
    prm = {"psfc": np.where(kind == 3, 47500.0 + 1500.0 * u(NCOL), 97000.0 + 4000.0 * u(NCOL)),
           "tsfc": np.where(kind == 3, 268.0 + 4.0 * u(NCOL), 297.0 + 7.0 * u(NCOL)),
           "bl_depth": 900.0 + 800.0 * u(NCOL), "bl_lapse": 0.004 + 0.003 * u(NCOL),
           "lapse": np.where(kind == 1, 0.003, 0.0068 + 0.001 * u(NCOL)),
           "trop": np.where(kind == 3, 5500.0, 11000.0 + 1500.0 * u(NCOL)),
           "rh_bl": np.where(kind == 1, 0.2, 0.7 + 0.25 * u(NCOL)), "rh_free": np.where(kind == 1, 0.1, 0.3 + 0.3 * u(NCOL)),
           "dry_sfc": np.where(kind == 2, 350.0 + 300.0 * u(NCOL), 0.0), "calm": kind == 7}
    return cc.sounding(z, prm, rng)


def coverage(host: dict, c: dict) -> dict:
    info = host["info"]
    K = c["theta_m"].shape[1]
    nloop1 = thick = 0
    if K == 150:
        p = c["pressure_p"] + c["pressure_base"]
        nloop1 = int(np.count_nonzero(np.any(p[:, :-1] - p[:, 1:] < 100.0, axis=1)))
        thick = int(np.count_nonzero(np.any(p[:, :-1] - p[:, 1:] > 1000.0, axis=1)))
    zp, ztop = info["zp"], info["zp"][:, -1]
    return {"cape_and_cin": int(np.count_nonzero((host["cape"] > 100.0) & (host["cin"] > 0.0))),
            "cape_zero": int(np.count_nonzero(host["cape"] == 0.0)),
            "kmax_elevated": int(np.count_nonzero(info["kmax"] > 0)),
            "first_above_500hPa": int(np.count_nonzero(info["p1"] < 50000.0)),
            "end_100hPa": int(np.count_nonzero(info["end"] == cc.END_100HPA)),
            "end_top": int(np.count_nonzero(info["end"] == cc.END_TOP)),
            "first_positive": int(np.count_nonzero(np.any(info["branch"] == cc.FIRST_POSITIVE, axis=1))),
            "first_negative": int(np.count_nonzero(np.any(info["branch"] == cc.FIRST_NEGATIVE, axis=1))),
            "zp1_above_1000": int(np.count_nonzero(zp[:, 0] > 1000.0)), "zp1_below_1000": int(np.count_nonzero(zp[:, 0] <= 1000.0)),
            "ztop_below_6000": int(np.count_nonzero(ztop < 6000.0)) if K == 4 else 1,
            "ztop_above_6000": int(np.count_nonzero(ztop >= 6000.0)),
            "shear_floor": int(np.count_nonzero(info["shear_raw"] < 1.0e-4)),
            "negative_srh": int(np.count_nonzero(np.any(info["srh_raw"] < 0.0, axis=1))),
            "thin_layers": nloop1 if K == 150 else 1, "thick_layers": thick if K == 150 else 1}


def check_coverage(cov: dict, K: int):
    short = {name: count for name, count in cov.items() if count < 1}
    assert not short, f"K={K}: not exercised: {short}"


def make(K: int, rng) -> dict:
    """A set whose columns are all stable: the borderline ones are replaced from further draws."""
    c = draw(rng, K)
    for _ in range(20):
        _, stable, _ = cc.classify(c)
        if stable.all():
            return c
        d = draw(rng, K)
        for name in cc.INPUTS:
            c[name][~stable] = d[name][~stable]
    raise RuntimeError(f"K={K}: borderline columns after 20 redraws")


def find_noconv(rng):
    """A K = 26 column whose fixed-point iteration does not converge in 100 iterations, or None: draws with
    extreme moisture and temperature, NOCONV_BUDGET columns in all."""
    for _ in range(NOCONV_BUDGET // NCOL):
        c = draw(rng, 26)
        c["qv"] = np.asarray(c["qv"] * (1.0 + 40.0 * rng.random(c["qv"].shape)), dtype=np.float32).astype(np.float64)
        c["theta_m"] = np.asarray(c["theta_m"] * (0.6 + 1.2 * rng.random(c["qv"].shape)), dtype=np.float32).astype(np.float64)
        host = cc.compute(c)
        bad = np.flatnonzero(host["info"]["end"] == cc.END_NOCONV)
        if bad.size:
            return {name: c[name][bad[:4]] for name in cc.INPUTS}
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ref", default=os.environ.get("MPAS_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "convective_columns.npz"))
    ap.add_argument("--time", action="store_true", help="print the compiled cut-out's seconds per column and write no file")
    args = ap.parse_args()
    rng = np.random.default_rng(20241020)
    data = {"K": np.array(KS, dtype=np.int32)}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(args.ref, tmp)
        sets = [(K, f"K{K}", make(K, rng)) for K in KS]
        if args.time:
            for K, tag, c in sets:
                _, sec = run_reference(exe, tmp, c, nrep=20)
                print(f"{tag}: {sec / 20 / NCOL:.3e} s per column (compiled reference, one core, all outputs)")
            return
        nc = find_noconv(rng)
        print("noconv:", "none found in %d columns" % NOCONV_BUDGET if nc is None else f"{nc['qv'].shape[0]} columns")
        if nc is not None:
            sets.append((26, "noconv", nc))
        for K, tag, c in sets:
            t0 = time.time()
            host = cc.compute(c)
            if tag != "noconv":
                cov = coverage(host, c)
                check_coverage(cov, K)
                print(f"{tag}: {cov}")
            ref, _ = run_reference(exe, tmp, c)
            exact = [name for name in cc.WRITTEN if np.array_equal(host[name], ref[name])]
            worst = max(float(np.max(np.abs(host[n] - ref[n])) / max(np.max(np.abs(ref[n])), 1e-300)) for n in cc.WRITTEN)
            print(f"{tag}: restatement vs reference rel_linf {worst:.3e}, {len(exact)} of 12 outputs bit for bit; sub-steps "
                  f"{host['info']['nsub'].max()} max, {time.time() - t0:.1f} s")
            for name in cc.INPUTS:
                a32 = c[name].astype(np.float32)
                assert np.array_equal(a32.astype(np.float64), c[name]), name
                data[f"{name}_{tag}"] = a32
            for name in cc.WRITTEN:
                data[f"ref_{name}_{tag}"] = ref[name]
    np.savez_compressed(args.out, **data)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()

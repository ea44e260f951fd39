#!/usr/bin/env python3
"""Generate tests/golden/kessler_columns.npz: synthetic columns through the reference's compiled Kessler.

Build machine only (it needs the reference tree and amdflang).  The script compiles
physics_wrf/module_mp_kessler.F from the reference tree, unchanged, into a temporary directory with the
oracle's Fortran flags (amdflang -O2 -fdefault-real-8 -fdefault-double-8) and the small driver below,
which reads and writes raw arrays; runs it on 64 synthetic columns for each K in KS; and writes the
inputs (t, qv, qc, qr, rho, pii, dt, and zgrid, whose levels and differences are z and dz8w; numbers
that float32 holds exactly, stored as float32) and the reference's outputs (t, qv, qc, qr, rainnc, rainncv) as ``<name>_K<K>`` / ``ref_<name>_K<K>``.  Only data is written: neither the reference's
source nor the binary leaves the temporary directory.

The columns are a warm moist sounding with seeded cloud and rain; dt is large enough that nfall ranges
from 1 to more than 8.  With the host restatement (mpas_dycore.kessler) the script asserts what the
inputs must exercise -- tests/test_kessler_host.py re-checks the same on the committed file:
  * on at least 5 % of the cell-levels each: prod > 0 (condensation); ern > 0 limited by each of the
    three amin1 arguments; product = -qc (cloud exhausted);
  * on at least 10 % of the columns nfall_new /= nfall occurs at least once;
  * every nint margin (distance of crmax / 0.75 from the nearest integer >= 1, where nfall changes) is
    >= 1e-6, so a last-bit difference in pow can never change a column's nfall.  Columns that miss it
    are redrawn.

    python tools/make_kessler_golden.py [--ref /path/to/reference] [--out tests/golden/kessler_columns.npz]
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

from mpas_dycore import kessler as ks  # noqa: E402

KS = (4, 26, 63, 64, 150)
DT = {4: 400.0, 26: 300.0, 63: 200.0, 64: 200.0, 150: 120.0}
NCOL = 64
MIN_MARGIN = 1.0e-6
INPUTS = ("t", "qv", "qc", "qr", "rho", "pii", "z", "dz8w")
STORED = ("t", "qv", "qc", "qr", "rho", "pii", "zgrid")   # float32 in the file, exactly
OUTPUTS = ("t", "qv", "qc", "qr", "rainnc", "rainncv")

DRIVER = """
program kessler_columns
   use module_mp_kessler
   implicit none
   integer(4) :: n, K, i, kk, a
   real(8) :: dt
   real(8), allocatable :: buf(:,:), f(:,:,:,:), z(:,:,:), rainnc(:,:), rainncv(:,:)
   open(10, file='in.bin', access='stream', form='unformatted', status='old')
   read(10) n, K
   read(10) dt
   allocate(buf(K, n), f(n, K, 1, 8), rainnc(n, 1), rainncv(n, 1))
   do a = 1, 8
      read(10) buf
      do kk = 1, K
         do i = 1, n
            f(i, kk, 1, a) = buf(kk, i)
         end do
      end do
   end do
   close(10)
   rainnc = 0.0
   rainncv = 0.0
   call kessler(f(:,:,:,1), f(:,:,:,2), f(:,:,:,3), f(:,:,:,4), f(:,:,:,5), f(:,:,:,6), dt, f(:,:,:,7), &
                2.50e6, 7.0*287.0/2.0, 287.0/461.6, 0.6112, 17.67, 29.65, 273.15, 1000.0, f(:,:,:,8), &
                rainnc, rainncv, 1, n, 1, 1, 1, K, 1, n, 1, 1, 1, K, 1, n, 1, 1, 1, K)
   open(11, file='out.bin', access='stream', form='unformatted', status='replace')
   do a = 1, 4
      do kk = 1, K
         do i = 1, n
            buf(kk, i) = f(i, kk, 1, a)
         end do
      end do
      write(11) buf
   end do
   write(11) rainnc, rainncv
   close(11)
end program kessler_columns
"""


def build_reference(ref: str, tmp: str) -> str:
    src = os.path.join(ref, "src", "core_atmosphere", "physics", "physics_wrf", "module_mp_kessler.F")
    open(os.path.join(tmp, "driver.f90"), "w").write(DRIVER)
    exe = os.path.join(tmp, "kessler_columns")
    flags = ["-O2", "-fdefault-real-8", "-fdefault-double-8"]
    subprocess.run(["amdflang", *flags, "-ffree-form", "-c", src, "-o", os.path.join(tmp, "module_mp_kessler.o")],
                   check=True, cwd=tmp)
    subprocess.run(["amdflang", *flags, "driver.f90", "module_mp_kessler.o", "-o", exe], check=True, cwd=tmp)
    return exe


def run_reference(exe: str, tmp: str, cols: dict, dt: float) -> dict:
    n, K = cols["t"].shape
    with open(os.path.join(tmp, "in.bin"), "wb") as fh:
        fh.write(np.array([n, K], dtype=np.int32).tobytes())
        fh.write(np.array([dt], dtype=np.float64).tobytes())
        for name in INPUTS:
            fh.write(np.ascontiguousarray(cols[name], dtype=np.float64).tobytes())
    subprocess.run([exe], check=True, cwd=tmp)
    raw = np.fromfile(os.path.join(tmp, "out.bin"), dtype=np.float64)
    assert raw.size == 4 * n * K + 2 * n, raw.size
    out = {name: raw[i * n * K:(i + 1) * n * K].reshape(n, K).copy() for i, name in enumerate(OUTPUTS[:4])}
    out["rainnc"] = raw[4 * n * K:4 * n * K + n].copy()
    out["rainncv"] = raw[4 * n * K + n:].copy()
    return out


def _quantize(a: np.ndarray, bits: int) -> np.ndarray:
    """a rounded to float32 with only the leading `bits` mantissa bits kept: the inputs are synthetic, so
    they may as well be numbers that store in 4 bytes and compress (the file stays under 1 MB)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return (u & np.uint32((0xFFFFFFFF << (23 - bits)) & 0xFFFFFFFF)).view(np.float32).astype(np.float64)


def draw_columns(rng, n: int, K: int) -> dict:
    """n columns: a warm sounding (6.5 K/km, hydrostatic pressure) on stretched levels, each level drawn
    into one of the sweep's regimes -- 0 supersaturated with cloud; 1 dry with a trace of rain (it all
    evaporates); 2 sub-saturated with light rain (the rate limits the evaporation); 3 sub-saturated with
    rain and cloud that, after autoconversion, covers most of the deficit (the rest of the deficit limits
    it); 4 sub-saturated with a little cloud (exhausted); 5 around saturation with cloud -- under a
    per-column rain amount between none and heavy."""
    ztop = min(8000.0, 400.0 * K)
    zgrid = ztop * (np.arange(K + 1) / K) ** (1.2 if K < 100 else 1.0)
    zgrid = np.tile(zgrid, (n, 1)) * (1.0 + 0.05 * rng.random((n, 1)))
    zgrid = _quantize(zgrid, 16)
    z = zgrid[:, :K].copy()
    dz8w = zgrid[:, 1:] - zgrid[:, :K]
    zm = 0.5 * (zgrid[:, 1:] + zgrid[:, :K])
    t0 = 295.0 + 10.0 * rng.random((n, 1))
    temp = t0 - 6.5e-3 * zm
    p = 1.0e5 * (temp / t0) ** (ks.GRAVITY / (ks.R_D * 6.5e-3))
    pii = (p / ks.P0) ** (ks.R_D / ks.CP)
    rho = p / (ks.R_D * temp)
    es = 1000.0 * ks.SVP1 * np.exp(ks.SVP2 * (temp - ks.SVPT0) / (temp - ks.SVP3))
    qvs = ks.EP_2 * es / (p - es)
    f5 = ks.SVP2 * (ks.SVPT0 - ks.SVP3) * ks.XLV / ks.CP
    regime = rng.choice(6, size=(n, K), p=np.array([1.0, 1.5, 1.5, 1.5, 1.0, 0.5]) / 7.0)
    u, v = rng.random((n, K)), rng.random((n, K))
    amount = np.where(rng.random((n, 1)) < 0.1, 0.0, rng.random((n, 1)) ** 2)      # per column: none .. heavy
    rh = np.select([regime == r for r in range(6)],
                   [1.0 + 0.05 * u, 0.2 + 0.4 * u, 0.9 + 0.09 * u, 0.6 + 0.35 * u, 0.5 + 0.4 * u, 0.9 + 0.2 * u])
    qv = rh * qvs
    qr = np.select([regime == 1, regime == 2], [1.0e-5 * v, 1.0e-3 * v], 6.0e-3 * v) * amount
    qr = np.where(rng.random((n, K)) < 0.1, 0.0, qr)
    # the deficit the saturation adjustment sees (-prod), and the part of qc that survives autoconversion
    deficit = np.maximum(qvs - qv, 0.0) / (1.0 + p / (p - es) * qvs * f5 / (temp - ks.SVP3) ** 2)
    factorn = 1.0 / (1.0 + ks.C3 * DT[K] * qr ** ks.C4)
    w = rng.random((n, K))
    qc = np.select([regime == 0, regime == 3, regime == 4, regime == 5],
                   [2.0e-3 * w, deficit * (0.5 + 0.49 * w) / factorn, deficit * 0.5 * w / factorn, 3.0e-3 * w], 0.0)
    q = {n: _quantize(a, 12) for n, a in (("t", temp / pii), ("qv", qv), ("qc", qc), ("qr", qr), ("rho", rho),
                                          ("pii", pii))}
    return {"zgrid": zgrid, **q, "z": z, "dz8w": dz8w}


def coverage(info: dict) -> dict:
    """The fractions the fixture must reach, from kessler()'s info."""
    out = {n: float(np.mean(info[n])) for n in ("cond", "ern1", "ern2", "ern3", "exhaust")}
    out["resplit"] = float(np.mean(info["resplit"]))
    out["min_margin"] = float(min(m.min() for m in info["margin"]))
    out["nfall_min"], out["nfall_max"] = int(info["nfall0"].min()), int(info["nfall0"].max())
    return out


def check_coverage(cov: dict, K: int):
    for n in ("cond", "ern1", "ern2", "ern3", "exhaust"):
        assert cov[n] >= 0.05, f"K={K}: {n} on {cov[n]:.3f} of the cell-levels (< 5 %)"
    assert cov["resplit"] >= 0.10, f"K={K}: nfall_new /= nfall on {cov['resplit']:.3f} of the columns (< 10 %)"
    assert cov["min_margin"] >= MIN_MARGIN, f"K={K}: nint margin {cov['min_margin']:.3e}"
    assert cov["nfall_min"] == 1 and cov["nfall_max"] > 8, f"K={K}: nfall {cov['nfall_min']}..{cov['nfall_max']}"


def make(K: int, rng) -> dict:
    dt = DT[K]
    cols = draw_columns(rng, NCOL, K)
    for _ in range(20):
        info = ks.kessler(dt=dt, **{n: cols[n] for n in INPUTS})["info"]
        bad = np.array([m.min() < MIN_MARGIN for m in info["margin"]])
        if not bad.any():
            break
        new = draw_columns(rng, int(bad.sum()), K)
        for name in new:
            cols[name][bad] = new[name]
    else:
        raise RuntimeError(f"K={K}: columns with a nint margin below {MIN_MARGIN} after 20 redraws")
    return cols


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ref", default=os.environ.get("MPAS_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "kessler_columns.npz"))
    args = ap.parse_args()
    rng = np.random.default_rng(20240613)
    data = {"K": np.array(KS, dtype=np.int32)}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(args.ref, tmp)
        for K in KS:
            cols = make(K, rng)
            host = ks.kessler(dt=DT[K], **{n: cols[n] for n in INPUTS})
            cov = coverage(host["info"])
            check_coverage(cov, K)
            ref = run_reference(exe, tmp, cols, DT[K])
            worst = 0.0
            for name in OUTPUTS:
                d = float(np.max(np.abs(host[name] - ref[name])) / max(np.max(np.abs(ref[name])), 1e-300))
                worst = max(worst, d)
                data[f"ref_{name}_K{K}"] = ref[name]
            # z and dz8w are zgrid's levels and differences (the MPAS form; mpas_dycore.kessler.fixture_columns)
            for name in STORED:
                a32 = cols[name].astype(np.float32)
                assert np.array_equal(a32.astype(np.float64), cols[name]), name
                data[f"{name}_K{K}"] = a32
            data[f"dt_K{K}"] = np.array(DT[K])
            print(f"K={K}: {cov}  restatement vs reference rel_linf {worst:.3e}")
    np.savez_compressed(args.out, **data)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()

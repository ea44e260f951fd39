// The Kessler warm-rain microphysics of the time step: everything driver_microphysics
// (physics/mpas_atmphys_driver_microphysics.F:237-425) does for config_microp_scheme = 'mp_kessler' on
// the owned cells of a block, on one time level of the state:
//   precip_from_MPAS          (:429-500)  rainncv = 0; the scheme's own rainnc_p / rainncv_p start at 0
//   microphysics_from_MPAS    (mpas_atmphys_interface.F:541-559)
//       rho = zz rho_zz, th = theta_m / (1 + R_v/R_d max(0, qv)), pii = exner, z = zgrid(k),
//       dz = zgrid(k+1) - zgrid(k)
//   kessler                   (physics_wrf/module_mp_kessler.F), dt_in = dt (n_microp = 1)
//   precip_to_MPAS            (:533-559)  precipw, rainncv, rainnc, the config_bucket_rainnc bucket
//   microphysics_to_MPAS      (mpas_atmphys_interface.F:694-737)  qv, qc, qr, rt_diabatic_tend, theta_m,
//       rtheta_p, exner, pressure_p, then surface_pressure / tend_sfc_pressure from levels 1-3
// The l_diags branch (compute_relhum) and w_p / pres_p, which Kessler does not read, are not part of it.
//
// fp64 throughout (the reference builds the WRF physics with 8-byte REAL), every + - * / in the
// Fortran's order, left to right; the build's -ffp-contract=off keeps them apart.  x**2 is x * x, every
// x**r with a real r is pow.  pow / exp / sqrt are the device library's: they agree with the C
// library's to the last bits, not bit for bit (tests/test_gpu_kessler.py states the bounds).
//
// One wavefront per owned cell, the cell index a scalar; lanes stride over the levels, level
// k = lane + 64 j of chunk j < NCH: one source for nVertLevels 4..511 in every build of the library.
// The kernel is a template on the chunk count; a build of the library instantiates the one its columns
// need (KESSLER_CHUNKS: 1 in the one-wavefront build, lanes / 64 in the wide ones, i.e. ceil(K / 64)
// for the levels that build serves, at most 8), chunks past the column's top are masked.  Every field is K-contiguous (scalars scalar-major), so loads and stores
// coalesce.  Halo cells and the garbage slot are never written.
//
// Sedimentation (:99-195).  The column's prodk, vt, rhok, vtden, rdzw stay in registers for the whole
// time-split loop.  rdzk needs no registers: with z = zgrid(k) and dz8w = zgrid(k+1) - zgrid(k), as
// microphysics_from_MPAS sets them, rdzk(k) = 1 / (z(k+1) - z(k)) is rdzw(k) for k < K and
// rdzk(K) = 1 / (z(K) - z(K-1)) is rdzw(K-1), the same operations on the same operands.  nfall, dtfall
// and time_sediment are wave-uniform: crmax is a wave max-reduction (the order of a max does not
// matter for finite values).  The flux-upstream update reads the old prodk(k+1), vt(k+1) -- the
// Fortran loop ascends, so level k+1 is not yet updated when level k reads it: a lane shift, lane 63
// taking lane 0 of the next chunk.  nfall is re-evaluated after every split step as :167-182 do.
// RAINNCV / RAINNC are level 1's, once per split step, in split-step order.
// nfall is capped at KESSLER_MAX_NFALL (a Courant number of 7500 per step) and the loop at
// KESSLER_MAX_SPLITS split steps: finite, sane input never gets near either; they keep a column of Inf or
// garbage from spinning the wave for ever.
//
// precip_to_MPAS's precipw is summed over k ascending from 0.0, the terms added one after the other
// in level order as k_convdiag adds uph (a tree sum would change the bits).  No term is negative
// (qv >= 0 after the scheme), so skipping the exact zeros leaves the sum as it is.
#pragma once

namespace mpas {

constexpr int KESSLER_THREADS = 256;
constexpr int KESSLER_WAVES = KESSLER_THREADS / 64;
#ifdef MPAS_WIDE
constexpr int KESSLER_CHUNKS = WIDE_THREADS / 64;
#else
constexpr int KESSLER_CHUNKS = 1;
#endif
constexpr double KESSLER_MAX_NFALL = 10000.0;
constexpr int KESSLER_MAX_SPLITS = 40000;

// mpas_atmphys_constants.F:40-65 (cp, R_d, gravity are mpas_constants': CP, RGAS, GRAVITY)
constexpr double KS_XLV = 2.50e6, KS_EP_2 = RGAS / RV, KS_SVP1 = 0.6112, KS_SVP2 = 17.67, KS_SVP3 = 29.65;
constexpr double KS_SVPT0 = 273.15, KS_RHO_W = 1000.0;
// module_mp_kessler.F:23-26, 76
constexpr double KS_C1 = .001, KS_C2 = .001, KS_C3 = 2.2, KS_C4 = .875, KS_MAX_CR = 0.75;

struct Kessler {
  int nCellsSolve, nCells, K;
  int iqv, iqc, iqr;                 // 0-based scalar indices
  double dt, bucket;                 // dt_microp = dt_dyn; config_bucket_rainnc (<= 0: no bucket)
  const double *zz, *zgrid, *rho_zz, *rtheta_base, *exner_base, *pressure_base;
  double *theta_m, *scalars, *exner, *rtheta_p, *pressure_p, *rt_diabatic_tend;
  double *rainnc, *rainncv, *precipw, *surface_pressure, *tend_sfc_pressure;
  int* i_rainnc;
};

// The hook's host state (mpas_dyc_ctx::microp): the MPAS_DYC_MICROP_* scheme of the step, the 0-based
// scalar indices of cloud and rain water, config_bucket_rainnc, and the last mpas_dyc_microphysics
// under mpas_dyc_set_profile (mpas_dyc_get_profile out[7])
struct MicropState {
  int scheme = 0, iqc = -1, iqr = -1;
  double bucket = 0.0, ms = 0.0;
};

__device__ __forceinline__ double kessler_wave_max(double x) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) x = fmax(x, __shfl_xor(x, s, 64));
  return x;
}

// nint(0.5 + crmax / max_cr_sedimentation), at least 1 (:118, :177); nint rounds halves away from zero
__device__ __forceinline__ int kessler_nfall(double crmax) {
  const double r = round(0.5 + crmax / KS_MAX_CR);
  return r >= 1.0 ? (int)fmin(r, KESSLER_MAX_NFALL) : 1;
}

// x**r: inlined where a lane holds one or two levels; with more chunks the unrolled sweep would hold
// 7 NCH copies of the library's pow, so those builds call one out-of-line copy (the same function,
// the same bits)
__device__ __attribute__((noinline)) double kessler_pow_call(double x, double y) { return pow(x, y); }
template <int NCH>
__device__ __forceinline__ double kessler_pow(double x, double y) {
  if constexpr (NCH <= 2) return pow(x, y);
  else return kessler_pow_call(x, y);
}

template <int NCH>
__global__ __launch_bounds__(KESSLER_THREADS) void k_kessler(Kessler a) {
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * KESSLER_WAVES + (threadIdx.x >> 6)));
  if (c >= a.nCellsSolve) return;
  const int K = a.K;
  const double dt = a.dt;
  const int64_t o = (int64_t)c * K, oz = (int64_t)c * (K + 1), sn = (int64_t)(a.nCells + 1) * K;
  double* __restrict__ qvp = a.scalars + a.iqv * sn + o;
  double* __restrict__ qcp = a.scalars + a.iqc * sn + o;
  double* __restrict__ qrp = a.scalars + a.iqr * sn + o;
  const double* __restrict__ zg = a.zgrid + oz;

  // microphysics_from_MPAS
  double th[NCH], qv[NCH], qc[NCH], qr[NCH], rho[NCH], pii[NCH], dz[NCH], zz[NCH], rz[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int k = lane + 64 * j;
    const bool in = k < K;
    qv[j] = in ? qvp[k] : 0.0;
    qc[j] = in ? qcp[k] : 0.0;
    qr[j] = in ? qrp[k] : 0.0;
    zz[j] = in ? a.zz[o + k] : 1.0;
    rz[j] = in ? a.rho_zz[o + k] : 1.0;
    pii[j] = in ? a.exner[o + k] : 1.0;
    const double tm = in ? a.theta_m[o + k] : 300.0;
    dz[j] = in ? zg[k + 1] - zg[k] : 1.0;
    rho[j] = zz[j] * rz[j];
    th[j] = tm / (1.0 + RV / RGAS * fmax(0.0, qv[j]));
  }

  // ---- sedimentation (:99-195)
  double prodk[NCH], vt[NCH], vtden[NCH], rdzw[NCH];
  const double rho1 = __shfl(rho[0], 0, 64);                         // rhok(1)
  double crmax = 0.0;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    prodk[j] = qr[j];
    const double qrr = fmax(0.0, qr[j] * 0.001 * rho[j]);
    vtden[j] = sqrt(rho1 / rho[j]);
    vt[j] = 36.34 * kessler_pow<NCH>(qrr, 0.1364) * vtden[j];
    rdzw[j] = 1.0 / dz[j];
    if (lane + 64 * j < K) crmax = fmax(vt[j] * dt * rdzw[j], crmax);
  }
  crmax = kessler_wave_max(crmax);
  // rdzk(K) = rdzw(K-1)
  double rdz_top = 0.0;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const double v = __shfl(rdzw[j], (K - 2) & 63, 64);
    if (((K - 2) >> 6) == j) rdz_top = v;
  }
  int nfall = kessler_nfall(crmax);
  double dtfall = dt / (double)nfall;
  double time_sediment = dt;
  double rainnc_p = 0.0;                                             // precip_from_MPAS (rainncv_p is never read)
  const int nxt = (lane + 1) & 63;
  for (int split = 0; nfall > 0 && split < KESSLER_MAX_SPLITS; ++split) {
    time_sediment = time_sediment - dtfall;
    // the upstream flux of every level, then each level's neighbour above (old values)
    double fl[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) fl[j] = rho[j] * prodk[j] * vt[j];
    const double ppt = __shfl(fl[0], 0, 64) * dtfall / KS_RHO_W;      // k = 1
    rainnc_p = rainnc_p + ppt * 1000.0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const int k = lane + 64 * j;
      const double same = __shfl(fl[j], nxt, 64);
      const double next = __shfl(fl[j + 1 < NCH ? j + 1 : j], nxt, 64);
      const double up = lane == 63 ? next : same;
      if (k < K - 1) {
        const double factor = dtfall * rdzw[j] / rho[j];
        prodk[j] = prodk[j] - factor * (fl[j] - up);
      } else if (k == K - 1) {
        const double factor = dtfall * rdz_top;
        prodk[j] = prodk[j] - factor * prodk[j] * vt[j];
      }
    }
    if (nfall > 1) {  // not the last split step: new fall speeds, and the split re-evaluated
      nfall = nfall - 1;
      crmax = 0.0;
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const double qrr = fmax(0.0, prodk[j] * 0.001 * rho[j]);
        vt[j] = 36.34 * kessler_pow<NCH>(qrr, 0.1364) * vtden[j];
        if (lane + 64 * j < K) crmax = fmax(vt[j] * time_sediment * rdzw[j], crmax);
      }
      crmax = kessler_wave_max(crmax);
      const int nfall_new = kessler_nfall(crmax);
      if (nfall_new != nfall) {
        nfall = nfall_new;
        dtfall = time_sediment / (double)nfall;
      }
    } else {
      nfall = 0;
    }
  }

  // ---- production, saturation adjustment, evaporation (:203-236), then microphysics_to_MPAS per level
  const double f5 = KS_SVP2 * (KS_SVPT0 - KS_SVP3) * KS_XLV / CP;
  const double rcv = RGAS / (CP - RGAS);
  double pw[NCH], pp[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int k = lane + 64 * j;
    const bool in = k < K;
    const double factorn = 1.0 / (1.0 + KS_C3 * dt * kessler_pow<NCH>(fmax(0.0, qr[j]), KS_C4));
    const double qrprod = qc[j] * (1.0 - factorn) + factorn * KS_C1 * dt * fmax(qc[j] - KS_C2, 0.0);
    const double rcgs = 0.001 * rho[j];
    double qcn = fmax(qc[j] - qrprod, 0.0);
    double qrn = (qr[j] + prodk[j] - qr[j]);
    qrn = fmax(qrn + qrprod, 0.0);
    const double temp = pii[j] * th[j];
    const double pressure = 1.000e+05 * kessler_pow<NCH>(pii[j], 1004. / 287.);
    const double gam = 2.5e+06 / (1004. * pii[j]);
    const double es = 1000. * KS_SVP1 * exp(KS_SVP2 * (temp - KS_SVPT0) / (temp - KS_SVP3));
    const double qvs = KS_EP_2 * es / (pressure - es);
    const double t3 = temp - KS_SVP3;
    const double prod = (qv[j] - qvs) / (1. + pressure / (pressure - es) * qvs * f5 / (t3 * t3));
    const double rq = rcgs * qrn;
    const double dim = qvs > qv[j] ? qvs - qv[j] : 0.0;
    const double e1 = dt * (((1.6 + 124.9 * kessler_pow<NCH>(rq, .2046)) * kessler_pow<NCH>(rq, .525)) / (2.55e8 / (pressure * qvs) + 5.4e5)) *
                      (dim / (rcgs * qvs));
    const double ern = fmin(fmin(e1, fmax(-prod - qcn, 0.0)), qrn);
    const double product = fmax(prod, -qcn);
    const double thn = th[j] + gam * (product - ern);
    const double qvn = fmax(qv[j] - product + ern, 0.0);
    qcn = qcn + product;
    qrn = qrn - ern;
    // precip_to_MPAS: this level's term of precipw
    const double rho_a = rho[j] / (1.0 + qvn);
    pw[j] = in ? qvn * rho_a * dz[j] : 0.0;
    qv[j] = qvn;
    // microphysics_to_MPAS (:694-719)
    pp[j] = 0.0;
    if (in) {
      qvp[k] = qvn;
      qcp[k] = qcn;
      qrp[k] = qrn;
      const double tm_old = a.theta_m[o + k];
      const double tm = thn * (1. + RV / RGAS * qvn);
      a.rt_diabatic_tend[o + k] = (tm - tm_old) / dt;
      a.theta_m[o + k] = tm;
      const double rtb = a.rtheta_base[o + k];
      const double rtp = rz[j] * tm - rtb;
      a.rtheta_p[o + k] = rtp;
      const double ex = kessler_pow<NCH>(zz[j] * (RGAS / P0) * (rtp + rtb), rcv);
      a.exner[o + k] = ex;
      pp[j] = zz[j] * RGAS * (ex * rtp + (ex - a.exner_base[o + k]) * rtb);
      a.pressure_p[o + k] = pp[j];
    }
  }

  // precipw: the terms in level order
  double precipw = 0.0;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    unsigned long long todo = __ballot(pw[j] != 0.0);
    while (todo) {
      const int l = __builtin_ctzll(todo);
      precipw = precipw + __shfl(pw[j], l, 64);
      todo &= todo - 1;
    }
  }
  // surface pressure and its tendency (:722-737), from levels 1-3 (lanes 0-2 of chunk 0)
  const double qv1 = __shfl(qv[0], 0, 64), qv2 = __shfl(qv[0], 1, 64);
  const double rz1 = __shfl(rz[0], 0, 64), rz2 = __shfl(rz[0], 1, 64);
  const double zz1 = __shfl(zz[0], 0, 64), zz2 = __shfl(zz[0], 1, 64);
  const double tem1 = __shfl(dz[0], 0, 64), tem2 = __shfl(dz[0], 1, 64);
  const double pp1 = __shfl(pp[0], 0, 64);
  if (lane == 0) {
    a.precipw[c] = precipw;
    a.rainncv[c] = rainnc_p;
    double rn = a.rainnc[c] + rainnc_p;
    if (a.bucket > 0.0 && rn > a.bucket) {  // l_acrain (config_bucket_rainnc > 0)
      a.i_rainnc[c] = a.i_rainnc[c] + 1;
      rn = rn - a.bucket;
    }
    a.rainnc[c] = rn;
    const double r1 = rz1 * zz1 * (1. + qv1);
    const double r2 = rz2 * zz2 * (1. + qv2);
    const double old = a.surface_pressure[c];
    double sp = 0.5 * GRAVITY * tem1 * (r1 - 0.5 * (r2 - r1) * tem1 / (tem1 + tem2));
    sp = sp + pp1 + a.pressure_base[o];
    a.surface_pressure[c] = sp;
    a.tend_sfc_pressure[c] = (sp - old) / dt;
  }
}

}  // namespace mpas

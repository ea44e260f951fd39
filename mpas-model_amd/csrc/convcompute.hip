// The output-time half of the reference's convective diagnostics: convective_diagnostics_compute
// (core_atmosphere/diagnostics/convective_diagnostics.F:227-487) with column_height_value,
// integral_zstaggered, integral_zpoint (:528-589) and getcape (:595-1037, getqvs :1043, getthe :1077),
// on the owned cells of a block.  Two kernels, one bit per output (MPAS_DYC_CONV_* of
// include/mpas_dycore.h), the reference's quirks kept:
//   * with any bit set the four *_surface fields are written (:383-386 have no test);
//   * uzonal / umeridional _1km / _6km and srh_0_1km / srh_0_3km each under their own bit (:387-398, :443-448);
//   * cape and cin are both written if either bit is set (:454-469);
//   * lcl and lfc are never written: the reference fetches them and never computes them (getcape's lfc
//     is a dead local); their bits only count towards "any".
// Halo cells and the garbage slot are never written.  relhum, which the reference fetches, is not read.
//
// fp64, every + - * / as in the Fortran, left to right, under the build's -ffp-contract=off; default-real
// literals are doubles (the oracle's -fdefault-real-8).  x**2 is x * x and x**(-1) is 1 / x, as the
// compiled reference evaluates them.
//
// k_conv_shear (:361-451): one wavefront per owned cell, lanes striding over the levels, as k_convdiag.
//   temperature(1), dewpoint(1) (Bolton, through log); column_height_value, whose kz is the last level
//   with zp(k) <= z (a ballot per 64 levels; the last chunk that has one wins), clamped to n - 1;
//   integral_zstaggered and integral_zpoint, each lane forming the term of its level and the wave adding
//   the non-zero terms one after the other in ascending k from +0.0 (a sum that starts at +0.0 never
//   becomes -0.0, and adding a zero term leaves it as it is: skipping them cannot change a bit for finite
//   inputs); dudz / dvdz with their copied end levels; srh with its max(0., .).  Except dewpoint_surface
//   everything is + - * / and sqrt: it has the reference's bits.
//
// k_conv_cape (getcape with source = 2, adiabat = 1, pinc = 100): one lane per owned column in 64-thread
//   blocks, so a block retires when its own columns are done.  The lane walks its own K-contiguous
//   columns; p, pi, q, th, thv of a level cost one pow, one exp and one log and are recomputed where
//   used (the kmax scan, then the ascent, which carries level k - 1 in registers); z(k), which only the
//   source = 3 branch reads, is not formed.  What the device's exp / log / pow return is not the C
//   library's to the last bit: cape, cin (and dewpoint_surface) are held to a relative bound, not to bits.
//   Left out because it cannot change a bit (for finite operands):
//     - the ice terms: adiabat = 1 has fliq = 1, fice = 0, so fice * getqvi(..) is an exact zero added to
//       getqvs(..) > 0, qi2 = max(0 * (..), 0) = 0, qibar = 0, and lhs * (qi2 - qi1) / (cpm * tbar) is +0;
//       ql1 is 0 at the start of every sub-step (the pseudoadiabat resets ql2), so ql2 - ql1 = ql2 and
//       qlbar = 0.5 * ql2; the denominators 1 + qv2 + ql2 + qi2 add exact zeros;
//     - getthe inside the loop and before it: `the` is not read after the source parcel is found;
//     - ps, cloud and lfc, which nothing reads; the source = 1 / 3 and adiabat = 2..4 branches.
//   log(p2 / p1) and pi2 are formed once per sub-step, not once per iteration: the same operands.
//   The `i > 100` exit (no convergence) returns with cape and cin as accumulated so far, as the reference.
//   BOUNDED WORK, a defined deviation: a column's ascent ends, with cape and cin as accumulated so far,
//   before the sub-step that would be its (8192 + K + 1)th.  A column that is monotone below 8192 hPa
//   never gets there (real columns take under a thousand sub-steps), but pressures that go up and down,
//   or garbage, could otherwise keep a lane running: 1 + int(dp / pinc) is unbounded.  With it, with
//   int(dp / pinc) read as at most 2^30 (also for a NaN), and with the reference's own 100-iteration cap,
//   every lane's trip count is bounded whatever the inputs.  mpas_dycore/convcompute.py does the same.
#pragma once

namespace mpas {

constexpr int CONV_THREADS = 256;
constexpr int CONV_WAVES = CONV_THREADS / 64;
constexpr int CONV_CAPE_THREADS = 64;
// = MPAS_DYC_CONV_* of include/mpas_dycore.h, in the order of the reference's list (:285-312)
constexpr int CONV_CAPE = 1, CONV_CIN = 2, CONV_LCL = 4, CONV_LFC = 8, CONV_SRH_0_1KM = 16, CONV_SRH_0_3KM = 32;
constexpr int CONV_UZONAL_SURFACE = 64, CONV_UZONAL_1KM = 128, CONV_UZONAL_6KM = 256, CONV_UMERIDIONAL_SURFACE = 512;
constexpr int CONV_UMERIDIONAL_1KM = 1024, CONV_UMERIDIONAL_6KM = 2048, CONV_TEMPERATURE_SURFACE = 4096;
constexpr int CONV_DEWPOINT_SURFACE = 8192, CONV_ALL = 16383;
constexpr int CONV_NFIELDS = 14;
// the diag fields (Registry_convective.xml), in the bit order of the flags
constexpr const char* CONV_FIELDS[CONV_NFIELDS] = {
    "cape", "cin", "lcl", "lfc", "srh_0_1km", "srh_0_3km", "uzonal_surface", "uzonal_1km", "uzonal_6km",
    "umeridional_surface", "umeridional_1km", "umeridional_6km", "temperature_surface", "dewpoint_surface"};
constexpr int CONV_SUBSTEP_CAP = 8192;  // + K: the sub-steps of one column's ascent

// The hook's host state (mpas_dyc_ctx::conv): the MPAS_DYC_CONV_* mask, and the last
// mpas_dyc_convective_diagnostics under mpas_dyc_set_profile (mpas_dyc_get_profile out[11])
struct ConvState {
  int flags = 0;
  double ms = 0.0;
};

struct ConvCompute {
  int nCellsSolve, K, flags;
  const double *theta_m, *qv;                    // state, time level tl: K per cell
  const double *exner, *pressure_p, *pressure_base, *uzonal, *umeridional;  // diag: K per cell
  const double *zgrid;                           // K + 1 per cell
  double *out[CONV_NFIELDS];                     // in the bit order; lcl and lfc are never written
};

// temperature(k, iCell) (:363) and dewpoint(k, iCell) (:366-372)
__device__ __forceinline__ double conv_temperature(double theta_m, double qv, double exner) {
  return (theta_m / (1.0 + (RV / RGAS) * qv)) * exner;
}
__device__ __forceinline__ double conv_dewpoint(double pb, double pp, double qv) {
  double evp = 0.01 * (pb + pp) * qv / (qv + 0.622);
  evp = fmax(evp, 1.0e-8);
  const double l = log(evp / 6.112);
  return (243.5 * l) / (17.67 - l) + 273.15;
}

// column_height_value (:528-544) of the wave's column: zp(k) = 0.5 (zg(k) + zg(k+1)) - zg(1); every lane
// returns the same kz (0-based)
__device__ __forceinline__ int conv_kz(const double* __restrict__ zg, int K, int lane, double z) {
  int kz = 0;
  for (int kb = 0; kb < K; kb += 64) {
    const int k = kb + lane;
    const bool below = k < K && 0.5 * (zg[k] + zg[k + 1]) - zg[0] <= z;
    const unsigned long long m = __ballot(below);
    if (m) kz = kb + 63 - __builtin_clzll(m);
  }
  return min(kz, K - 2);
}
__device__ __forceinline__ double conv_height_value(const double* __restrict__ v, const double* __restrict__ zg, int kz,
                                                    double z) {
  const double z0 = 0.5 * (zg[kz] + zg[kz + 1]) - zg[0], z1 = 0.5 * (zg[kz + 1] + zg[kz + 2]) - zg[0];
  const double wz = (z1 - z) / (z1 - z0);
  const double wzp1 = 1. - wz;
  return wz * v[kz] + wzp1 * v[kz + 1];
}

// the wave's terms (one per level of each 64-level chunk, `term(k)` for 0-based k < n) added in level order
template <class F>
__device__ __forceinline__ double conv_ordered_sum(int n, int lane, F term) {
  double s = 0.0;
  for (int kb = 0; kb < n; kb += 64) {
    const int k = kb + lane;
    const double t = k < n ? term(k) : 0.0;
    unsigned long long todo = __ballot(t != 0.0);  // wave-uniform
    while (todo) {
      const int l = __builtin_ctzll(todo);
      s = s + __shfl(t, l, 64);
      todo &= todo - 1;
    }
  }
  return s;
}

// integral_zstaggered (:548-565) over 0 .. ztop of the relative heights
__device__ __forceinline__ double conv_integral_zstaggered(const double* __restrict__ v, const double* __restrict__ zg, int K,
                                                           int lane, double zbot, double ztop) {
  return conv_ordered_sum(K, lane, [&](int k) {
    const double zb = fmax(zg[k] - zg[0], zbot);
    const double zt = fmin(zg[k + 1] - zg[0], ztop);
    return v[k] * fmax(0., zt - zb);
  });
}

// dudz(k) (:422-429) of a 1-based level k1 in 1 .. K; v is uzonal or umeridional
__device__ __forceinline__ double conv_ddz(const double* __restrict__ v, const double* __restrict__ zg, int K, int k1) {
  const int k = min(max(k1, 2), K - 1);  // the copied end levels
  return (v[k - 1] - v[k - 2]) / (0.5 * (zg[k] - zg[k - 2]));
}
// srh(k) (:431-441) of a 1-based point k1 in 1 .. K + 1, after max(0., .)
__device__ __forceinline__ double conv_srh(const double* __restrict__ u, const double* __restrict__ v,
                                           const double* __restrict__ zg, int K, int k1, double u_storm, double v_storm) {
  const int k = min(k1, K);  // srh(K + 1) = srh(K)
  const double dudz = conv_ddz(u, zg, K, k), dvdz = conv_ddz(v, zg, K, k);
  double s;
  if (k == 1) s = -(u[0] - u_storm) * dvdz + (v[0] - v_storm) * dudz;
  else s = -(0.5 * (u[k - 1] + u[k - 2]) - u_storm) * dvdz + (0.5 * (v[k - 1] + v[k - 2]) - v_storm) * dudz;
  return fmax(0., s);
}

__global__ __launch_bounds__(CONV_THREADS) void k_conv_shear(ConvCompute a) {
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * CONV_WAVES + (threadIdx.x >> 6)));
  if (c >= a.nCellsSolve) return;
  const int K = a.K, flags = a.flags;
  const double* __restrict__ u = a.uzonal + (int64_t)c * K;
  const double* __restrict__ v = a.umeridional + (int64_t)c * K;
  const double* __restrict__ zg = a.zgrid + (int64_t)c * (K + 1);

  if (lane == 0) {  // :383-386, written whatever the bits
    const int64_t o = (int64_t)c * K;
    a.out[6][c] = u[0];
    a.out[9][c] = v[0];
    a.out[12][c] = conv_temperature(a.theta_m[o], a.qv[o], a.exner[o]);
    a.out[13][c] = conv_dewpoint(a.pressure_base[o], a.pressure_p[o], a.qv[o]);
  }
  if (flags & (CONV_UZONAL_1KM | CONV_UMERIDIONAL_1KM)) {
    const int kz = conv_kz(zg, K, lane, 1000.0);
    if (lane == 0 && (flags & CONV_UZONAL_1KM)) a.out[7][c] = conv_height_value(u, zg, kz, 1000.0);
    if (lane == 0 && (flags & CONV_UMERIDIONAL_1KM)) a.out[10][c] = conv_height_value(v, zg, kz, 1000.0);
  }
  const bool srh = (flags & (CONV_SRH_0_1KM | CONV_SRH_0_3KM)) != 0;
  int kz6 = 0;
  if (srh || (flags & (CONV_UZONAL_6KM | CONV_UMERIDIONAL_6KM))) kz6 = conv_kz(zg, K, lane, 6000.0);
  if (lane == 0 && (flags & CONV_UZONAL_6KM)) a.out[8][c] = conv_height_value(u, zg, kz6, 6000.0);
  if (lane == 0 && (flags & CONV_UMERIDIONAL_6KM)) a.out[11][c] = conv_height_value(v, zg, kz6, 6000.0);
  if (!srh) return;

  // storm motion, Bunkers' formula for right movers (:403-418); every lane forms the same scalars
  const double dev_motion = 7.5, z_bunker_bot = 0., z_bunker_top = 6000.;
  double u_srh_bot = u[0], v_srh_bot = v[0];
  const double zp1 = 0.5 * (zg[0] + zg[1]) - zg[0];
  if (z_bunker_bot > zp1) {  // wave-uniform
    const int kz0 = conv_kz(zg, K, lane, z_bunker_bot);
    u_srh_bot = conv_height_value(u, zg, kz0, z_bunker_bot);
    v_srh_bot = conv_height_value(v, zg, kz0, z_bunker_bot);
  }
  const double u_srh_top = conv_height_value(u, zg, kz6, z_bunker_top);
  const double v_srh_top = conv_height_value(v, zg, kz6, z_bunker_top);
  const double u_shear = u_srh_top - u_srh_bot;
  const double v_shear = v_srh_top - v_srh_bot;
  const double u_mean = conv_integral_zstaggered(u, zg, K, lane, z_bunker_bot, z_bunker_top) / (z_bunker_top - z_bunker_bot);
  const double v_mean = conv_integral_zstaggered(v, zg, K, lane, z_bunker_bot, z_bunker_top) / (z_bunker_top - z_bunker_bot);
  const double shear_magnitude = fmax(0.0001, sqrt(u_shear * u_shear + v_shear * v_shear));
  const double u_storm = u_mean + dev_motion * v_shear / shear_magnitude;
  const double v_storm = v_mean - dev_motion * u_shear / shear_magnitude;

  // integral_zpoint (:569-589) of srh over the K + 1 relative interface heights
  for (int which = 0; which < 2; ++which) {
    if (!(flags & (which ? CONV_SRH_0_3KM : CONV_SRH_0_1KM))) continue;
    const double ztop = which ? 3000.0 : 1000.0;
    const double s = conv_ordered_sum(K, lane, [&](int k) {
      const double zk = zg[k] - zg[0], zk1 = zg[k + 1] - zg[0];
      const double zb = fmax(zk, 0.0);
      const double zt = fmin(zk1, ztop);
      const double dz = fmax(0., zt - zb);
      if (!(dz != 0.0)) return 0.0;  // the layers above ztop: the term is an exact zero
      const double zr_midpoint = (0.5 * (zt + zb) - zk) / (zk1 - zk);
      const double s0 = conv_srh(u, v, zg, K, k + 1, u_storm, v_storm), s1 = conv_srh(u, v, zg, K, k + 2, u_storm, v_storm);
      const double midpoint_value = s0 + (s1 - s0) * zr_midpoint;
      return dz * midpoint_value;
    });
    if (lane == 0) a.out[which ? 5 : 4][c] = s;
  }
}

// ---- getcape ----
namespace capec {
constexpr double pinc = 100.0, g = 9.81, p00 = 100000.0, cp = 1005.7, rd = 287.04, rv = 461.5, xlv = 2501000.0;
constexpr double t0 = 273.15, cpv = 1875.0, cpl = 4190.0;
constexpr double lv1 = xlv + (cpl - cpv) * t0, lv2 = cpl - cpv;
constexpr double rp00 = 1.0 / p00, eps = rd / rv, reps = rv / rd, rddcp = rd / cp, cpdg = cp / g;
constexpr double converge = 0.0002;
}  // namespace capec

__device__ __forceinline__ double conv_getqvs(double p, double t) {
  const double es = 611.2 * exp(17.67 * (t - 273.15) / (t - 29.65));
  return (287.04 / 461.5) * es / (p - es);
}

__device__ __forceinline__ double conv_getthe(double p, double t, double td, double q) {
  double tlcl;
  if ((td - t) >= -0.1) tlcl = t;
  else tlcl = 56.0 + 1.0 / (1.0 / (td - 56.0) + 0.00125 * log(t / td));
  return t * pow(100000.0 / p, 0.2854 * (1.0 - 0.28 * q)) * exp(((3376.0 / tlcl) - 2.54) * q * (1.0 + 0.81 * q));
}

// p, t, td, pi, q, th, thv of a level (:708-716), through p_in, t_in, td_in (:456-458)
struct ConvLevel {
  double p, t, td, pi, q, th, thv;
};
__device__ __forceinline__ ConvLevel conv_level(const ConvCompute& a, int64_t i) {
  using namespace capec;
  const double qv = a.qv[i], pb = a.pressure_base[i], pp = a.pressure_p[i];
  const double p_in = (pp + pb) / 100.0;
  const double t_in = conv_temperature(a.theta_m[i], qv, a.exner[i]) - 273.15;
  const double td_in = conv_dewpoint(pb, pp, qv) - 273.15;
  ConvLevel l;
  l.p = 100.0 * p_in;
  l.t = 273.15 + t_in;
  l.td = 273.15 + td_in;
  l.pi = pow(l.p * rp00, rddcp);
  l.q = conv_getqvs(l.p, l.td);
  l.th = l.t / l.pi;
  l.thv = l.th * (1.0 + reps * l.q) / (1.0 + l.q);
  return l;
}

__global__ __launch_bounds__(CONV_CAPE_THREADS) void k_conv_cape(ConvCompute a) {
  using namespace capec;
  const int c = blockIdx.x * CONV_CAPE_THREADS + threadIdx.x;
  if (c >= a.nCellsSolve) return;
  const int nk = a.K;
  const int64_t o = (int64_t)c * nk;

  // the source parcel: the most unstable level below 500 hPa, the first maximum (:732-751)
  ConvLevel l = conv_level(a, o);
  int kmax = 0;
  if (!(l.p < 50000.0)) {
    double maxthe = 0.0;
    for (int k = 0; k < nk; ++k) {
      const ConvLevel lk = k ? conv_level(a, o + k) : l;
      if (lk.p >= 50000.0) {
        const double the = conv_getthe(lk.p, lk.t, lk.td, lk.q);
        if (the > maxthe) maxthe = the, kmax = k;
      }
    }
    if (kmax) l = conv_level(a, o + kmax);
  }

  double narea = 0.0;
  int k = kmax;
  double th2 = l.th, pi2 = l.pi, p2 = l.p, t2 = l.t, thv2 = l.thv, qv2 = l.q, b2 = 0.0;
  double qt = qv2, cape = 0.0, cin = 0.0;
  double p_km1 = l.p, pi_km1 = l.pi, thv_km1 = l.thv;  // level k - 1 of the environment
  bool doit = true;
  int left = CONV_SUBSTEP_CAP + nk;                    // sub-steps this column may still take

  while (doit && k < nk - 1) {
    k = k + 1;
    const double b1 = b2;
    const ConvLevel e = conv_level(a, o + k);
    double dp = p_km1 - e.p;
    int nloop = 1;
    if (!(dp < pinc)) {
      const double r = dp / pinc;
      nloop = 1 + (r < 1073741824.0 ? (int)r : 1073741824);
      dp = dp / (double)nloop;
    }
    for (int n = 0; n < nloop; ++n) {
      if (left-- <= 0) goto done;  // the bounded-work deviation
      const double p1 = p2, t1 = t2, th1 = th2, qv1 = qv2;
      p2 = p2 - dp;
      pi2 = pow(p2 * rp00, rddcp);
      const double logp = log(p2 / p1);
      double thlast = th1, ql2 = 0.0;
      int i = 0;
      for (;;) {
        i = i + 1;
        t2 = thlast * pi2;
        qv2 = fmin(qt, conv_getqvs(p2, t2));
        ql2 = fmax(qt - qv2, 0.0);
        const double tbar = 0.5 * (t1 + t2);
        const double qvbar = 0.5 * (qv1 + qv2);
        const double qlbar = 0.5 * ql2;
        const double lhv = lv1 - lv2 * tbar;
        const double rm = rd + rv * qvbar;
        const double cpm = cp + cpv * qvbar + cpl * qlbar;
        th2 = th1 * exp(lhv * ql2 / (cpm * tbar) + (rm / cpm - rd / cp) * logp);
        if (i > 100) goto done;  // no convergence: cape and cin as accumulated so far
        if (fabs(th2 - thlast) > converge) thlast = thlast + 0.3 * (th2 - thlast);
        else break;
      }
      qt = qv2;  // pseudoadiabat: the condensate falls out
    }
    {
      thv2 = th2 * (1.0 + reps * qv2) / (1.0 + qv2);
      b2 = g * (thv2 - e.thv) / e.thv;
      const double dz = -cpdg * 0.5 * (e.thv + thv_km1) * (e.pi - pi_km1);
      double parea;
      if (b2 >= 0.0 && b1 < 0.0) {  // first trip into positive area
        const double frac = b2 / (b2 - b1);
        parea = 0.5 * b2 * dz * frac;
        narea = narea - 0.5 * b1 * dz * (1.0 - frac);
        cin = cin + narea;
        narea = 0.0;
      } else if (b2 < 0.0 && b1 > 0.0) {  // first trip into negative area
        const double frac = b1 / (b1 - b2);
        parea = 0.5 * b1 * dz * frac;
        narea = -0.5 * b2 * dz * (1.0 - frac);
      } else if (b2 < 0.0) {  // still collecting negative buoyancy
        parea = 0.0;
        narea = narea - 0.5 * dz * (b1 + b2);
      } else {  // still collecting positive buoyancy
        parea = 0.5 * dz * (b1 + b2);
        narea = 0.0;
      }
      cape = cape + fmax(0.0, parea);
      if (e.p <= 10000.0 && b2 < 0.0) doit = false;  // stop if b < 0 and p < 100 mb
      p_km1 = e.p, pi_km1 = e.pi, thv_km1 = e.thv;
    }
  }
done:
  a.out[0][c] = cape;
  a.out[1][c] = cin;
}

}  // namespace mpas

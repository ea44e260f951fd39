// The isobaric output diagnostics and mslp: interp_diagnostics
// (core_atmosphere/diagnostics/isobaric_diagnostics.F:265-895) with its three array routines
// interp_tofixed_pressure (:899-985), compute_slp (:988-1121) and compute_layer_mean (:1139-1245), on the
// owned cells and owned vertices of a block:
//   pressure(k)   = (pressure_p + pressure_base) / 100                                  hPa   (:506)
//   pressure2(k)  the same at the K + 1 interfaces, height-weighted; the top one through exp / log (:517-542)
//   pressure_v(k) = (sum over iVertD = 1..3 of kiteAreasOnVertex * pressure(cellsOnVertex)) / areaTriangle (:545-555)
//   temperature   = (theta_m / (1 + rvord qv)) exner,  dewpoint after Bolton (1980)           (:561-569)
//   <field>_{200,250,500,700,850,925}hPa: temperature, relhum, dewpoint, uzonal, umeridional on
//       pressure; height (zgrid), w on pressure2; vorticity on pressure_v
//   mslp = 100 compute_slp;  t_isobaric on 100 pressure, z_isobaric on 100 pressure2 (levels in Pa);
//   meanT_500_300 = compute_layer_mean(temperature, 100 pressure)
//
// interp_tofixed_pressure per column.  The routine works on arrays reversed so that pressure increases
// with the index; its kupper / kount bookkeeping couples columns only where some column's pressure is
// not strictly monotone.  For strictly monotone columns it is, with f, p a level and fu, pu the level
// above it (the routine's kk + 1 and kk):
//   pu < p_out <= p for some level:   (fu dpl + f dpu) / (dpl + dpu),  dpu = p_out - pu, dpl = p - p_out
//   else p_out < p(top):              f(top) p_out / p(top)
//   else p_out > p(bottom):           f(bottom)
//   else (p_out == p(top)):           the bracket formula on the two topmost levels
// Results are guaranteed for strictly monotone columns only.
//
// One wavefront per owned column, lane = level, looping over chunks of 64 levels (k = lane + 64 j): one
// source for every nVertLevels the library accepts, whatever the build's column shape.  A column's
// inputs are read once, K-contiguous, and every enabled output is formed in the same pass.  Each lane
// tests its own bracket (level k and level k + 1) against a target: the level above comes from the next
// lane by a cross-lane move, for lane 63 from lane 0 of the next chunk, which is loaded one iteration
// ahead.  The lane that holds the bracket stores the result; a ballot records that the target is done.
// The K + 1 interfaces of height / w / pressure2 spill into one more chunk exactly when K is a multiple
// of 64.  What no bracket holds is finished after the loop from the column's two topmost levels and its
// lowest one.  compute_slp's level search is the first set bit of a ballot in ascending chunks;
// compute_layer_mean's middle-layer sum adds its terms one after the other in the Fortran's order
// (descending level = ascending reversed index), every lane the same sum.
//
// compute_slp's two failure paths (no level 100 hPa above the ground; klo == khi) set the whole
// block's mslp to 0 in the reference.  Here such a column raises the block's word (IsoCells::fail, a
// plain store of 1) and k_iso_mslp_fail, launched after the cell kernel, zeroes mslp over the owned cells
// when the word is set: no host synchronisation.  The test runs over the owned cells only.
//
// fp64, every + - * / in the Fortran's order, left to right; the build's -ffp-contract=off keeps them
// apart.  x**2 is x * x.  log / exp / pow are the device library's: dewpoint_*, mslp and a bracket that
// contains pressure2(K + 1) agree with the C library's to the last bits, everything else bit for bit.
// Halo elements and the garbage slot are never written.
#pragma once

namespace mpas {

constexpr int ISO_THREADS = 256;
constexpr int ISO_WAVES = ISO_THREADS / 64;
// = MPAS_DYC_ISO_* of include/mpas_dycore.h; the first eight are the groups of six pressure levels
constexpr int ISO_TEMPERATURE = 1, ISO_RELHUM = 2, ISO_DEWPOINT = 4, ISO_UZONAL = 8, ISO_UMERIDIONAL = 16;
constexpr int ISO_HEIGHT = 32, ISO_W = 64, ISO_VORTICITY = 128, ISO_MSLP = 256, ISO_T_ISOBARIC = 512;
constexpr int ISO_Z_ISOBARIC = 1024, ISO_MEANT_500_300 = 2048, ISO_ALL = 4095;
constexpr int ISO_NGROUPS = 8, ISO_NP = 6, ISO_NT = 5, ISO_NZ = 13;
constexpr const char* ISO_GROUPS[ISO_NGROUPS] = {"temperature", "relhum", "dewpoint", "uzonal", "umeridional",
                                                 "height", "w", "vorticity"};
constexpr int ISO_HPA[ISO_NP] = {200, 250, 500, 700, 850, 925};
constexpr double ISO_RVORD = RV / RGAS;  // mpas_constants: rvord
// compute_slp's parameters (:1011-1015)
constexpr double SLP_GAMMA = 0.0065, SLP_RR = 287.0, SLP_GRAV = 9.80616, SLP_TC = 273.16 + 17.5, SLP_PCONST = 100.;

// The hook's host state (mpas_dyc_ctx::iso): the MPAS_DYC_ISO_* mask of mpas_dyc_isobaric_diagnostics and
// the last call under mpas_dyc_set_profile (mpas_dyc_get_profile out[8])
struct IsoState {
  int flags = 0;
  double ms = 0.0;
};

struct IsoCells {
  int nCellsSolve, K, flags;
  const double *pressure_p, *pressure_base, *theta_m, *qv, *exner, *relhum, *uzonal, *umeridional;  // K per cell
  const double *zgrid, *w;                                                                      // K + 1 per cell
  double hpa[ISO_NP], t_lev[ISO_NT], z_lev[ISO_NZ];
  double* out[ISO_NGROUPS - 1][ISO_NP];  // the cell groups in bit order
  double *mslp, *t_isobaric, *z_isobaric, *meanT_500_300;
  int* fail;
};

struct IsoVerts {
  int nVerticesSolve, K;
  const double *pressure_p, *pressure_base, *vorticity, *kiteAreasOnVertex, *areaTriangle;
  const int* cellsOnVertex;
  double hpa[ISO_NP];
  double* out[ISO_NP];
};

struct IsoLev { double p, t, td, rh, uz, um; };  // a mass level: pressure (hPa) and the fields on it
struct IsoIf { double p2, z, w; };               // an interface
struct IsoVtx { double p, f; };                  // a vertex level

// the value of level k + 1: the next lane's, for lane 63 lane 0's of the next chunk
__device__ __forceinline__ double iso_up(double cur, double nxt, int lane) {
  const double a = __shfl(cur, (lane + 1) & 63, 64), b = __shfl(nxt, 0, 64);
  return lane == 63 ? b : a;
}
__device__ __forceinline__ bool iso_bracket(double p, double pu, double po) { return po > pu && po <= p; }
__device__ __forceinline__ double iso_interp(double f, double fu, double p, double pu, double po) {
  const double dpu = po - pu, dpl = p - po;
  return (fu * dpl + f * dpu) / (dpl + dpu);
}
// a target no bracket holds: t the topmost level, t1 the one below it, b the lowest
__device__ __forceinline__ double iso_outside(double po, double pt, double pt1, double pb, double ft, double ft1,
                                              double fb) {
  if (po < pt) return ft * po / pt;
  if (po > pb) return fb;
  return iso_interp(ft1, ft, pt1, pt, po);
}

__device__ __forceinline__ double iso_pressure(const IsoCells& a, int64_t o, int k) {
  return (a.pressure_p[o + k] + a.pressure_base[o + k]) / 100.0;
}
__device__ __forceinline__ double iso_temperature(const IsoCells& a, int64_t o, int k) {
  return (a.theta_m[o + k] / (1.0 + ISO_RVORD * a.qv[o + k])) * a.exner[o + k];
}

// what the enabled outputs read of a mass level
__device__ __forceinline__ IsoLev iso_level(const IsoCells& a, int64_t o, int k, bool needT) {
  IsoLev v{};
  if (k >= a.K) return v;
  v.p = iso_pressure(a, o, k);
  if (needT) v.t = iso_temperature(a, o, k);
  if (a.flags & ISO_DEWPOINT) {
    const double qv = a.qv[o + k];
    double evp = v.p * qv / (qv + 0.622);
    evp = fmax(evp, 1.0e-8);
    v.td = (243.5 * log(evp / 6.112)) / (17.67 - log(evp / 6.112));
    v.td = v.td + 273.15;
  }
  if (a.flags & ISO_RELHUM) v.rh = a.relhum[o + k];
  if (a.flags & ISO_UZONAL) v.uz = a.uzonal[o + k];
  if (a.flags & ISO_UMERIDIONAL) v.um = a.umeridional[o + k];
  return v;
}

// interface i (0-based, 0..K): pressure2 (:517-542), zgrid and w
__device__ __forceinline__ IsoIf iso_iface(const IsoCells& a, int64_t o, int64_t oz, int i) {
  IsoIf v{};
  const int K = a.K;
  if (i > K) return v;
  const double* __restrict__ z = a.zgrid + oz;
  v.z = z[i];
  if (a.flags & ISO_W) v.w = a.w[oz + i];
  if (i == K) {
    const double z0 = z[i], z1 = 0.5 * (z[i] + z[i - 1]), z2 = 0.5 * (z[i - 1] + z[i - 2]);
    const double w1 = (z0 - z2) / (z1 - z2), w2 = 1. - w1;
    v.p2 = exp(w1 * log(iso_pressure(a, o, i - 1)) + w2 * log(iso_pressure(a, o, i - 2)));
  } else if (i == 0) {
    const double z0 = z[0], z1 = 0.5 * (z[0] + z[1]), z2 = 0.5 * (z[1] + z[2]);
    const double w1 = (z0 - z2) / (z1 - z2), w2 = 1. - w1;
    v.p2 = w1 * iso_pressure(a, o, 0) + w2 * iso_pressure(a, o, 1);
  } else {
    const double w1 = (z[i] - z[i - 1]) / (z[i + 1] - z[i - 1]), w2 = (z[i + 1] - z[i]) / (z[i + 1] - z[i - 1]);
    v.p2 = w1 * iso_pressure(a, o, i) + w2 * iso_pressure(a, o, i - 1);
  }
  return v;
}

// compute_slp of one column whose level search found 0-based level `lev`: the column's slp in hPa, or
// fail = true (klo == khi).  Every lane the same values.
__device__ __forceinline__ double iso_slp(const IsoCells& a, int64_t o, int64_t oz, int lev, bool& fail) {
  const int K = a.K;
  const int klo = max(lev + 1 - 1, 1), khi = min(klo + 1, K - 1);  // 1-based, as the Fortran's
  fail = klo == khi;
  if (fail) return 0.0;
  const double* __restrict__ z = a.zgrid + oz;
  const double p1 = iso_pressure(a, o, 0);
  const double plo = iso_pressure(a, o, klo - 1), phi = iso_pressure(a, o, khi - 1);
  const double tlo = iso_temperature(a, o, klo - 1) * (1. + 0.608 * a.qv[o + klo - 1]);
  const double thi = iso_temperature(a, o, khi - 1) * (1. + 0.608 * a.qv[o + khi - 1]);
  const double zlo = 0.5 * (z[klo - 1] + z[klo]), zhi = 0.5 * (z[khi - 1] + z[khi]);
  const double p_at_pconst = p1 - SLP_PCONST;
  const double t_at_pconst = thi - (thi - tlo) * log(p_at_pconst / phi) * log(plo / phi);
  const double z_at_pconst = zhi - (zhi - zlo) * log(p_at_pconst / phi) * log(plo / phi);
  const double t_surf = t_at_pconst * pow(p1 / p_at_pconst, SLP_GAMMA * SLP_RR / SLP_GRAV);
  double t_msl = t_at_pconst + SLP_GAMMA * z_at_pconst;
  const bool l1 = t_msl < SLP_TC, l2 = t_surf <= SLP_TC;  // mm5_test
  if (l2 && !l1) t_msl = SLP_TC;
  else t_msl = SLP_TC - 0.005 * ((t_surf - SLP_TC) * (t_surf - SLP_TC));
  const double z_half_lowest = 0.5 * (z[0] + z[1]);
  return p1 * exp((2. * SLP_GRAV * z_half_lowest) / (SLP_RR * (t_msl + t_surf)));
}

// compute_layer_mean(temperature, 100 pressure) between p_bot = 50000 and p_top = 30000 of one column:
// kt / kb the 0-based level k whose (k + 1, k] holds p_top / p_bot (-1: none).  Every lane the same value.
__device__ __forceinline__ double iso_layer_mean(const IsoCells& a, int64_t o, int kt, int kb, int lane) {
  const double p_top = 30000.0, p_bot = 50000.0;
  if (kt < 0 || kb < 0) return 0.0;
  // in the Fortran's (reversed) index kk a level's upper neighbour comes first: field_in(kk) = fu, (kk + 1) = f
  const double pt = iso_pressure(a, o, kt) * 100.0, ptu = iso_pressure(a, o, kt + 1) * 100.0;
  const double pb = iso_pressure(a, o, kb) * 100.0, pbu = iso_pressure(a, o, kb + 1) * 100.0;
  const double ft = iso_temperature(a, o, kt), ftu = iso_temperature(a, o, kt + 1);
  const double fb = iso_temperature(a, o, kb), fbu = iso_temperature(a, o, kb + 1);
  const double wtop_p = (p_top - ptu) / (pt - ptu), wtop_m = (pt - p_top) / (pt - ptu);
  const double wbot_m = (p_bot - pbu) / (pb - pbu), wbot_p = (pb - p_bot) / (pb - pbu);
  if (kt == kb) {
    double m = wtop_m * ftu + wtop_p * ft;
    m = m + wbot_m * fbu + wbot_p * fb;
    return 0.5 * m;
  }
  double wtotal = pt - p_top;
  double temp = wtop_m * ftu + wtop_p * ft;
  double m = wtotal * 0.5 * (ft + temp);
  // the middle layers kt - 1 .. kb + 1, descending (the Fortran's k ascending)
  const int hi = kt - 1, lo = kb + 1;
  for (int base = hi & ~63; base >= (lo & ~63) && hi >= lo; base -= 64) {
    const int k = base + lane;
    const bool in = k >= lo && k <= hi;
    double w = 0.0, term = 0.0;
    if (in) {
      w = iso_pressure(a, o, k) * 100.0 - iso_pressure(a, o, k + 1) * 100.0;
      term = w * 0.5 * (iso_temperature(a, o, k + 1) + iso_temperature(a, o, k));
    }
    unsigned long long todo = __ballot(in);
    while (todo) {
      const int l = 63 - __builtin_clzll(todo);
      wtotal = wtotal + __shfl(w, l, 64);
      m = m + __shfl(term, l, 64);
      todo &= ~(1ull << l);
    }
  }
  const double w = p_bot - pbu;
  wtotal = wtotal + w;
  temp = wbot_m * fbu + wbot_p * fb;
  m = m + w * 0.5 * (fbu + temp);
  return m / wtotal;
}

__global__ __launch_bounds__(ISO_THREADS) void k_iso_cells(IsoCells a) {
  const int lane = threadIdx.x & 63;
  // the wave's cell, as a scalar
  const int c = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * ISO_WAVES + (threadIdx.x >> 6)));
  if (c >= a.nCellsSolve) return;
  const int K = a.K, flags = a.flags;
  const int64_t o = (int64_t)c * K, oz = (int64_t)c * (K + 1);
  const bool needT = (flags & (ISO_TEMPERATURE | ISO_T_ISOBARIC)) != 0;
  const bool mass = (flags & (ISO_TEMPERATURE | ISO_RELHUM | ISO_DEWPOINT | ISO_UZONAL | ISO_UMERIDIONAL)) != 0;
  const bool iface = (flags & (ISO_HEIGHT | ISO_W | ISO_Z_ISOBARIC)) != 0;
  const double p1 = iso_pressure(a, o, 0);

  // targets done: bits 0-5 the mass levels' hPa targets, 6-11 the interfaces', 12-16 t_isobaric, 17-29 z_isobaric
  unsigned done = 0;
  int slp_level = -1, kt = -1, kb = -1;
  IsoLev cur = iso_level(a, o, lane, needT), nxt{};
  IsoIf icur{}, inxt{};
  if (iface) icur = iso_iface(a, o, oz, lane);
  const int nchunk = (K + 1 + 63) >> 6;
  for (int j = 0; j < nchunk; ++j) {
    const int k = lane + 64 * j;
    nxt = iso_level(a, o, k + 64, needT);
    IsoLev up;
    up.p = iso_up(cur.p, nxt.p, lane);
    const bool mv = k <= K - 2;  // levels k and k + 1 exist
    if (mass) {
      if (flags & ISO_TEMPERATURE) up.t = iso_up(cur.t, nxt.t, lane);
      if (flags & ISO_DEWPOINT) up.td = iso_up(cur.td, nxt.td, lane);
      if (flags & ISO_RELHUM) up.rh = iso_up(cur.rh, nxt.rh, lane);
      if (flags & ISO_UZONAL) up.uz = iso_up(cur.uz, nxt.uz, lane);
      if (flags & ISO_UMERIDIONAL) up.um = iso_up(cur.um, nxt.um, lane);
#pragma unroll
      for (int t = 0; t < ISO_NP; ++t) {
        const double po = a.hpa[t];
        const bool hit = mv && iso_bracket(cur.p, up.p, po);
        if (hit) {
          if (flags & ISO_TEMPERATURE) a.out[0][t][c] = iso_interp(cur.t, up.t, cur.p, up.p, po);
          if (flags & ISO_RELHUM) a.out[1][t][c] = iso_interp(cur.rh, up.rh, cur.p, up.p, po);
          if (flags & ISO_DEWPOINT) a.out[2][t][c] = iso_interp(cur.td, up.td, cur.p, up.p, po);
          if (flags & ISO_UZONAL) a.out[3][t][c] = iso_interp(cur.uz, up.uz, cur.p, up.p, po);
          if (flags & ISO_UMERIDIONAL) a.out[4][t][c] = iso_interp(cur.um, up.um, cur.p, up.p, po);
        }
        if (__ballot(hit)) done |= 1u << t;
      }
    }
    if (flags & (ISO_T_ISOBARIC | ISO_MEANT_500_300)) {
      const double pp = cur.p * 100.0, ppu = up.p * 100.0;
      if (flags & ISO_T_ISOBARIC) {
        if (!(flags & ISO_TEMPERATURE)) up.t = iso_up(cur.t, nxt.t, lane);
#pragma unroll
        for (int t = 0; t < ISO_NT; ++t) {
          const double po = a.t_lev[t];
          const bool hit = mv && iso_bracket(pp, ppu, po);
          if (hit) a.t_isobaric[(int64_t)c * ISO_NT + t] = iso_interp(cur.t, up.t, pp, ppu, po);
          if (__ballot(hit)) done |= 1u << (12 + t);
        }
      }
      if (flags & ISO_MEANT_500_300) {  // the trapping levels (:1197-1208)
        const unsigned long long mt = __ballot(mv && ppu <= 30000.0 && pp > 30000.0);
        const unsigned long long mb = __ballot(mv && ppu <= 50000.0 && pp > 50000.0);
        if (mt) kt = 64 * j + __builtin_ctzll(mt);
        if (mb) kb = 64 * j + __builtin_ctzll(mb);
      }
    }
    if (flags & ISO_MSLP) {  // the least level pconst hPa above the surface (:1035-1046)
      const unsigned long long m = __ballot(k < K && cur.p < p1 - SLP_PCONST);
      if (m && slp_level < 0) slp_level = 64 * j + __builtin_ctzll(m);
    }
    if (iface) {
      inxt = iso_iface(a, o, oz, k + 64);
      IsoIf iup;
      iup.p2 = iso_up(icur.p2, inxt.p2, lane);
      iup.z = iso_up(icur.z, inxt.z, lane);
      iup.w = (flags & ISO_W) ? iso_up(icur.w, inxt.w, lane) : 0.0;
      const bool iv = k <= K - 1;  // interfaces k and k + 1 exist
      if (flags & (ISO_HEIGHT | ISO_W)) {
#pragma unroll
        for (int t = 0; t < ISO_NP; ++t) {
          const double po = a.hpa[t];
          const bool hit = iv && iso_bracket(icur.p2, iup.p2, po);
          if (hit) {
            if (flags & ISO_HEIGHT) a.out[5][t][c] = iso_interp(icur.z, iup.z, icur.p2, iup.p2, po);
            if (flags & ISO_W) a.out[6][t][c] = iso_interp(icur.w, iup.w, icur.p2, iup.p2, po);
          }
          if (__ballot(hit)) done |= 1u << (6 + t);
        }
      }
      if (flags & ISO_Z_ISOBARIC) {
        const double pp = icur.p2 * 100.0, ppu = iup.p2 * 100.0;
#pragma unroll
        for (int t = 0; t < ISO_NZ; ++t) {
          const double po = a.z_lev[t];
          const bool hit = iv && iso_bracket(pp, ppu, po);
          if (hit) a.z_isobaric[(int64_t)c * ISO_NZ + t] = iso_interp(icur.z, iup.z, pp, ppu, po);
          if (__ballot(hit)) done |= 1u << (17 + t);
        }
      }
      icur = inxt;
    }
    cur = nxt;
  }

  // the targets no bracket holds, from the two topmost levels and the lowest one (every lane the same)
  const unsigned mass_want = (mass ? 0x3fu : 0u) | ((flags & ISO_T_ISOBARIC) ? 0x1fu << 12 : 0u);
  if (mass_want & ~done) {
    const IsoLev t0 = iso_level(a, o, K - 1, needT), t1 = iso_level(a, o, K - 2, needT), b0 = iso_level(a, o, 0, needT);
    if (lane == 0) {
      for (int t = 0; t < ISO_NP; ++t) {
        if (!mass || (done >> t & 1)) continue;
        const double po = a.hpa[t];
        if (flags & ISO_TEMPERATURE) a.out[0][t][c] = iso_outside(po, t0.p, t1.p, b0.p, t0.t, t1.t, b0.t);
        if (flags & ISO_RELHUM) a.out[1][t][c] = iso_outside(po, t0.p, t1.p, b0.p, t0.rh, t1.rh, b0.rh);
        if (flags & ISO_DEWPOINT) a.out[2][t][c] = iso_outside(po, t0.p, t1.p, b0.p, t0.td, t1.td, b0.td);
        if (flags & ISO_UZONAL) a.out[3][t][c] = iso_outside(po, t0.p, t1.p, b0.p, t0.uz, t1.uz, b0.uz);
        if (flags & ISO_UMERIDIONAL) a.out[4][t][c] = iso_outside(po, t0.p, t1.p, b0.p, t0.um, t1.um, b0.um);
      }
      if (flags & ISO_T_ISOBARIC)
        for (int t = 0; t < ISO_NT; ++t)
          if (!(done >> (12 + t) & 1))
            a.t_isobaric[(int64_t)c * ISO_NT + t] =
                iso_outside(a.t_lev[t], t0.p * 100.0, t1.p * 100.0, b0.p * 100.0, t0.t, t1.t, b0.t);
    }
  }
  const unsigned if_want = ((flags & (ISO_HEIGHT | ISO_W)) ? 0x3fu << 6 : 0u) | ((flags & ISO_Z_ISOBARIC) ? 0x1fffu << 17 : 0u);
  if (if_want & ~done) {
    const IsoIf t0 = iso_iface(a, o, oz, K), t1 = iso_iface(a, o, oz, K - 1), b0 = iso_iface(a, o, oz, 0);
    if (lane == 0) {
      if (flags & (ISO_HEIGHT | ISO_W))
        for (int t = 0; t < ISO_NP; ++t) {
          if (done >> (6 + t) & 1) continue;
          const double po = a.hpa[t];
          if (flags & ISO_HEIGHT) a.out[5][t][c] = iso_outside(po, t0.p2, t1.p2, b0.p2, t0.z, t1.z, b0.z);
          if (flags & ISO_W) a.out[6][t][c] = iso_outside(po, t0.p2, t1.p2, b0.p2, t0.w, t1.w, b0.w);
        }
      if (flags & ISO_Z_ISOBARIC)
        for (int t = 0; t < ISO_NZ; ++t)
          if (!(done >> (17 + t) & 1))
            a.z_isobaric[(int64_t)c * ISO_NZ + t] =
                iso_outside(a.z_lev[t], t0.p2 * 100.0, t1.p2 * 100.0, b0.p2 * 100.0, t0.z, t1.z, b0.z);
    }
  }

  if (flags & ISO_MEANT_500_300) {
    const double m = iso_layer_mean(a, o, kt, kb, lane);
    if (lane == 0) a.meanT_500_300[c] = m;
  }

  if (flags & ISO_MSLP) {
    bool fail = slp_level < 0;
    double slp = 0.0;
    if (!fail) slp = iso_slp(a, o, oz, slp_level, fail);
    if (lane == 0) {
      a.mslp[c] = slp * 100.0;  // hPa -> Pa (:794)
      if (fail) *a.fail = 1;
    }
  }
}

// compute_slp's failure paths: the whole block's mslp is 0 when any owned column failed
__global__ void k_iso_mslp_fail(int n, const int* __restrict__ fail, double* __restrict__ mslp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && *fail) mslp[i] = 0.0;
}

// pressure_v of level k of vertex v (:545-555), and the vorticity on it
__device__ __forceinline__ IsoVtx iso_vertex_level(const IsoVerts& a, int v, int c0, int c1, int c2, double k0, double k1,
                                                   double k2, double area, int k) {
  IsoVtx r{};
  const int K = a.K;
  if (k >= K) return r;
  double p = 0.0;
  p = p + k0 * ((a.pressure_p[(int64_t)c0 * K + k] + a.pressure_base[(int64_t)c0 * K + k]) / 100.0);
  p = p + k1 * ((a.pressure_p[(int64_t)c1 * K + k] + a.pressure_base[(int64_t)c1 * K + k]) / 100.0);
  p = p + k2 * ((a.pressure_p[(int64_t)c2 * K + k] + a.pressure_base[(int64_t)c2 * K + k]) / 100.0);
  r.p = p / area;
  r.f = a.vorticity[(int64_t)v * K + k];
  return r;
}

__global__ __launch_bounds__(ISO_THREADS) void k_iso_vertices(IsoVerts a) {
  const int lane = threadIdx.x & 63;
  const int v = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * ISO_WAVES + (threadIdx.x >> 6)));
  if (v >= a.nVerticesSolve) return;
  const int K = a.K;
  const int c0 = a.cellsOnVertex[3 * (int64_t)v], c1 = a.cellsOnVertex[3 * (int64_t)v + 1], c2 = a.cellsOnVertex[3 * (int64_t)v + 2];
  const double k0 = a.kiteAreasOnVertex[3 * (int64_t)v], k1 = a.kiteAreasOnVertex[3 * (int64_t)v + 1];
  const double k2 = a.kiteAreasOnVertex[3 * (int64_t)v + 2], area = a.areaTriangle[v];
  unsigned done = 0;
  IsoVtx cur = iso_vertex_level(a, v, c0, c1, c2, k0, k1, k2, area, lane), nxt{};
  const int nchunk = (K + 63) >> 6;
  for (int j = 0; j < nchunk; ++j) {
    const int k = lane + 64 * j;
    nxt = iso_vertex_level(a, v, c0, c1, c2, k0, k1, k2, area, k + 64);
    const double pu = iso_up(cur.p, nxt.p, lane), fu = iso_up(cur.f, nxt.f, lane);
    const bool mv = k <= K - 2;
#pragma unroll
    for (int t = 0; t < ISO_NP; ++t) {
      const double po = a.hpa[t];
      const bool hit = mv && iso_bracket(cur.p, pu, po);
      if (hit) a.out[t][v] = iso_interp(cur.f, fu, cur.p, pu, po);
      if (__ballot(hit)) done |= 1u << t;
    }
    cur = nxt;
  }
  if (done != 0x3fu) {
    const IsoVtx t0 = iso_vertex_level(a, v, c0, c1, c2, k0, k1, k2, area, K - 1);
    const IsoVtx t1 = iso_vertex_level(a, v, c0, c1, c2, k0, k1, k2, area, K - 2);
    const IsoVtx b0 = iso_vertex_level(a, v, c0, c1, c2, k0, k1, k2, area, 0);
    if (lane == 0)
      for (int t = 0; t < ISO_NP; ++t)
        if (!(done >> t & 1)) a.out[t][v] = iso_outside(a.hpa[t], t0.p, t1.p, b0.p, t0.f, t1.f, b0.f);
  }
}

}  // namespace mpas

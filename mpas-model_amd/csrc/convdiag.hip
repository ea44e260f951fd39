// The convective running maxima between history writes: convective_diagnostics_update
// (core_atmosphere/diagnostics/convective_diagnostics.F:99-198), the only worker of
// mpas_atm_diag_update (mpas_atm_core.F:700), on the owned cells of a block:
//   w_velocity_max(i)        = max(w_velocity_max(i), maxval(w(1:K,i)))                       (:156)
//   wind_speed_level1_max(i) = max(wind_speed_level1_max(i), sqrt(uz(1,i)**2 + um(1,i)**2))   (:162)
//   updraft_helicity_max(i)  = max(updraft_helicity_max(i), uph(i))                           (:189)
// with uph the 2-5 km AGL integral (integral_zstaggered, :548-565) of
//   uh(k,i) = max(0, 0.5 (w(k,i) + w(k+1,i))) * max(0, zeta(k,i) / areaCell(i))               (:177-178)
// and zeta the kite-area-weighted vorticity of the cell's vertices (:169-174).
//
// The two sums that decide the bits keep the Fortran's order:
//  * zeta(k,i).  The reference scatters kiteAreasOnVertex(j,v) * vorticity(k,v) into cellsOnVertex(j,v)
//    for v = 1..nVertices, j = 1..3, from 0.0.  A cell's terms therefore arrive in ascending block-local
//    vertex index (then j), not in verticesOnCell order.  The host builds that list per owned cell
//    from cellsOnVertex (ConvDiag::cv_start / cv_kite, physics_host.hip convdiag_table); an entry is the
//    index 3 v + j into kiteAreasOnVertex, v = entry / 3.  Entries of the garbage cell are dropped.
//  * uph(i) = sum over k = 1..K of uh(k,i) * max(0, min(z_agl(k+1), 5000) - max(z_agl(k), 2000)),
//    z_agl(k) = zgrid(k,i) - zgrid(1,i), added in ascending k from 0.0.  Each lane forms the term of
//    its level; the wave then adds the terms one after the other in level order, every lane the same
//    sum (a tree reduction would change the bits).
// Levels outside the 2-5 km band have a thickness of exactly 0 and their term is an exact +0 for
// finite inputs: they are skipped, and with them their vorticity gathers, and so is every in-band
// term that is itself zero.  Adding such a term would leave the sum as it is (the sum starts at +0.0
// and no term is negative).  Consequence: an Inf in w or vorticity outside the band does not turn the
// sum into NaN here, as 0 * Inf would in the reference.  Results are guaranteed for finite inputs
// only; Fortran's max with a NaN operand is unspecified anyway.
//
// One wavefront per owned cell, lanes striding over the levels (k = lane, lane + 64, ...): one source
// for nVertLevels 4..511 in every build of the library, every field K-contiguous, so the loads
// coalesce.  The maxval is a wave max-reduction (order does not matter for finite values).  One
// launch per block does all enabled maxima.  Halo cells and the garbage slot are never written.
// Every + - * / as in the Fortran, left to right; the build's -ffp-contract=off keeps them apart;
// the division is by areaCell, not a multiplication by invAreaCell.
#pragma once

namespace mpas {

constexpr int CONVDIAG_THREADS = 256;
constexpr int CONVDIAG_WAVES = CONVDIAG_THREADS / 64;
// = MPAS_DYC_DIAG_* of include/mpas_dycore.h
constexpr int CONVDIAG_W = 1, CONVDIAG_WSP = 2, CONVDIAG_UH = 4;
// the diag fields of mpas_dyc_diag_update, in the bit order of the flags
constexpr const char* CONVDIAG_FIELDS[3] = {"w_velocity_max", "wind_speed_level1_max", "updraft_helicity_max"};

// The hook's host state (mpas_dyc_ctx::convdiag): the MPAS_DYC_DIAG_* mask mpas_dyc_diag_update applies,
// and the last mpas_dyc_diag_update under mpas_dyc_set_profile (mpas_dyc_get_profile out[6])
struct ConvDiagState {
  int flags = 0;
  double ms = 0.0;
};
// A block's table (Block::cv; physics_host.hip convdiag_table), on the device: per owned cell its
// (vertex, j) pairs in ascending vertex index, as 3 v + j
struct ConvDiagTable {
  int *start = nullptr, *kite = nullptr;
  bool ready = false;
};

struct ConvDiag {
  int nCellsSolve, K, flags;
  const double *w;                               // state, time level 1: (K + 1) per cell
  const double *vorticity;                       // K per vertex
  const double *uzonal, *umeridional;            // diag.uReconstructZonal / Meridional: K per cell
  const double *zgrid, *areaCell, *kiteAreasOnVertex;
  const int *cv_start, *cv_kite;                 // nCellsSolve + 1 offsets; entries 3 v + j
  double *w_velocity_max, *wind_speed_level1_max, *updraft_helicity_max;
};

__device__ __forceinline__ double convdiag_wave_max(double x) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) x = fmax(x, __shfl_xor(x, s, 64));
  return x;
}

__global__ __launch_bounds__(CONVDIAG_THREADS) void k_convdiag(ConvDiag a) {
  const int lane = threadIdx.x & 63;
  // the wave's cell, as a scalar: the per-cell loads below are scalar loads
  const int c = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * CONVDIAG_WAVES + (threadIdx.x >> 6)));
  if (c >= a.nCellsSolve) return;
  const int K = a.K;
  const double* __restrict__ w = a.w + (int64_t)c * (K + 1);

  if (a.flags & CONVDIAG_W) {  // interface K + 1 is not part of the maxval
    double m = -INFINITY;
    for (int k = lane; k < K; k += 64) m = fmax(m, w[k]);
    m = convdiag_wave_max(m);
    if (lane == 0) a.w_velocity_max[c] = fmax(a.w_velocity_max[c], m);
  }

  if ((a.flags & CONVDIAG_WSP) && lane == 0) {
    const double uz = a.uzonal[(int64_t)c * K], um = a.umeridional[(int64_t)c * K];
    a.wind_speed_level1_max[c] = fmax(a.wind_speed_level1_max[c], sqrt(uz * uz + um * um));
  }

  if (a.flags & CONVDIAG_UH) {
    const double* __restrict__ zg = a.zgrid + (int64_t)c * (K + 1);
    const double z0 = zg[0], area = a.areaCell[c];
    const int e0 = a.cv_start[c], e1 = a.cv_start[c + 1];
    double uph = 0.0;
    for (int kb = 0; kb < K; kb += 64) {
      const int k = kb + lane;
      double term = 0.0;
      if (k < K) {
        const double zb = fmax(zg[k] - z0, 2000.0);
        const double zt = fmin(zg[k + 1] - z0, 5000.0);
        const double dz = fmax(0.0, zt - zb);
        if (dz > 0.0) {
          double zeta = 0.0;
          for (int e = e0; e < e1; ++e) {
            const int i = a.cv_kite[e];
            zeta = zeta + a.kiteAreasOnVertex[i] * a.vorticity[(int64_t)(i / 3) * K + k];
          }
          const double uh = fmax(0.0, 0.5 * (w[k] + w[k + 1])) * fmax(0.0, zeta / area);
          term = uh * dz;
        }
      }
      // the non-zero terms of these 64 levels, added in level order (the mask is wave-uniform)
      unsigned long long todo = __ballot(term != 0.0);
      while (todo) {
        const int l = __builtin_ctzll(todo);
        uph = uph + __shfl(term, l, 64);
        todo &= todo - 1;
      }
    }
    if (lane == 0) a.updraft_helicity_max[c] = fmax(a.updraft_helicity_max[c], uph);
  }
}

}  // namespace mpas

// Incremental analysis update (config_IAU_option = 'on'): atm_add_tend_anal_incr
// (core_atmosphere/dynamics/mpas_atm_iau.F:81-217), called from atm_srk3 after physics_get_tend
// (mpas_atm_time_integration.F:459-469).  The analysis-minus-background increments of the tend_iau
// pool (u, theta, rho, scalars), weighted by wgt = 1 / config_IAU_window_length_s, are added to the
// physics tendencies of the step on the owned edges and cells.
//
// The reference adds into tend_ru_physics / tend_rtheta_physics / tend_rho_physics, module scratch
// it refills every step.  Here the host may set tend_physics.* once and keep it, so the sums go
// into arrays of their own (scratch.iau_ru / iau_rtheta / iau_rho), which the step's consumers read
// in place of the host's (make_ptrs): physics + IAU on the owned elements, the physics value (0.0
// when the host supplies none: phys == nullptr) on every other element, the garbage slot included,
// because the consumers read the arrays wherever they run.  tend.scalars_tend is updated in place,
// as in the reference.
//
// Both kernels are pure streams: no stencil, no cross-level move.  They run flat over the
// (element, level) image [n+1][K] instead of one column per wavefront, so no lane idles at any K
// and one source serves every build (K = 4..511).  V2: two consecutive values per lane as one
// 16-byte access.  The flat image is 16-byte aligned from its base whatever K is, so the edge
// kernel always takes this form (a last single value when (nEdges + 1) K is odd); the cell kernel
// takes it when the scalar-major planes are aligned too, (nCells + 1) K even -- every even K --
// and one value per lane otherwise.  Every + - * / in the Fortran's left-to-right order; the
// build's -ffp-contract=off keeps them apart.
#pragma once

namespace mpas {

constexpr int IAU_THREADS = 256;
constexpr int IAU_MAX_BLOCKS = 2048;  // 8 workgroups per CU; the rest of the image by grid stride

// The hook's host state (mpas_dyc_ctx::iau): config_IAU_option / _window_length_s, and atm_iau_coef of
// the step being enqueued (> 1e-12: the step applies the forcing).  stale: the library's own
// tendencies (scratch.iau_*, tend.scalars_tend of a host that supplies none) hold a forced step's
// sums and are zeroed before the next unforced one reads them
struct IauState {
  int on = 0;
  double window = 0.0, wgt = 0.0;
  bool stale = false;
};

// tend_ru(k,i) = tend_ru(k,i) + wgt_iau * rho_edge(k,i) * u_amb(k,i)                      (170)
__device__ __forceinline__ double iau_edge_term(double t, double wgt, double rho_edge, double u_amb) {
  return t + wgt * rho_edge * u_amb;
}

// n = (nEdges + 1) K values, the first n_solve = nEdgesSolve K of them owned
__global__ __launch_bounds__(IAU_THREADS) void k_iau_edges(int64_t n, int64_t n_solve, double wgt,
                                                           const double* __restrict__ rho_edge,
                                                           const double* __restrict__ u_amb,
                                                           const double* __restrict__ phys, double* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * IAU_THREADS;
  const int64_t npair = n >> 1;
  for (int64_t i = (int64_t)blockIdx.x * IAU_THREADS + threadIdx.x; i < npair; i += stride) {
    const int64_t o = 2 * i;
    d2 t = phys ? ld2(phys + o) : d2{0.0, 0.0};
    if (o < n_solve) {  // uniform but for the one pair across the owned range's end
      const d2 re = ld2(rho_edge + o), ua = ld2(u_amb + o);
      t.x = iau_edge_term(t.x, wgt, re.x, ua.x);
      if (o + 1 < n_solve) t.y = iau_edge_term(t.y, wgt, re.y, ua.y);
    }
    st2(out + o, t);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[n - 1] = phys ? phys[n - 1] : 0.0;  // never owned
}

// What one (cell, level) point needs besides the scalars, and what it produces.
struct IauPoint {
  double zz, rho_zz, theta_m, qv, rho_amb, theta_amb;
};

// rho_t and the part of tend_th before the scalars (177, 190, 197); returns theta
__device__ __forceinline__ double iau_cell_head(const IauPoint& q, double wgt, double& rho_t, double& tend_th) {
  rho_t = rho_t + wgt * q.rho_amb / q.zz;                                            // 177
  const double theta = q.theta_m / (1.0 + RVORD * q.qv);                             // 190
  tend_th = 0.0 + wgt * (q.theta_amb * q.rho_zz + theta * q.rho_amb / q.zz);         // 163, 197
  return theta;
}
// tend_scalars += wgt * (scalars_amb * rho_zz + scalars * rho_amb / zz)                    (198-199)
__device__ __forceinline__ double iau_scalar_term(const IauPoint& q, double wgt, double st, double s_amb, double s) {
  return st + wgt * (s_amb * q.rho_zz + s * q.rho_amb / q.zz);
}
// the conversion to a theta_m tendency and the sum into rtheta_t (207-209)
__device__ __forceinline__ double iau_cell_tail(const IauPoint& q, double theta, double tend_th, double st_qv,
                                                double rtheta_t) {
  tend_th = (1. + RVORD * q.qv) * tend_th + RVORD * theta * st_qv;
  return rtheta_t + tend_th;
}

struct IauCells {
  int64_t n, n_solve, plane;        // (nCells + 1) K, nCellsSolve K, the scalars' plane stride = n
  int ns, moist_start, moist_end;   // 0-based inclusive; moist_end < moist_start: no scalar term
  int index_qv;                     // 0-based
  int st_zero;                      // the host supplies no scalars_tend: it counts as 0.0 before the IAU term
  double wgt;
  const double *zz, *rho_zz, *theta_m, *scalars;  // time level 1 (rho_zz_2 = rho_zz_1 at this point)
  const double *rho_amb, *theta_amb, *scalars_amb;
  const double *phys_rtheta, *phys_rho;           // the host's, or nullptr for 0.0
  double *out_rtheta, *out_rho, *scalars_tend;
};

// All of a point's work in one thread, in the reference's order: rho_t, theta, tend_th, the moist
// scalars' tendencies (a runtime loop over the scalar-major planes; qv and every moist scalar read
// once), the theta_m conversion with the scalars_tend(qv) just updated, rtheta_t.
template <bool V2>
__global__ __launch_bounds__(IAU_THREADS) void k_iau_cells(IauCells a) {
  constexpr int W = V2 ? 2 : 1;
  const int64_t stride = (int64_t)gridDim.x * IAU_THREADS;
  const int64_t nw = a.n / W;  // V2: n is even
  const bool qv_moist = a.index_qv >= a.moist_start && a.index_qv <= a.moist_end;
  for (int64_t i = (int64_t)blockIdx.x * IAU_THREADS + threadIdx.x; i < nw; i += stride) {
    const int64_t o = W * i;
    double rt[W], rr[W];
    if constexpr (V2) {
      const d2 t = a.phys_rtheta ? ld2(a.phys_rtheta + o) : d2{0.0, 0.0};
      const d2 r = a.phys_rho ? ld2(a.phys_rho + o) : d2{0.0, 0.0};
      rt[0] = t.x, rt[1] = t.y, rr[0] = r.x, rr[1] = r.y;
    } else {
      rt[0] = a.phys_rtheta ? a.phys_rtheta[o] : 0.0;
      rr[0] = a.phys_rho ? a.phys_rho[o] : 0.0;
    }
    const bool own0 = o < a.n_solve, own1 = V2 && o + 1 < a.n_solve;  // own1 implies own0
    if (own0) {
      IauPoint q[W];
      double v[6][W];
      const double* src[6] = {a.zz, a.rho_zz, a.theta_m, a.scalars + (int64_t)a.index_qv * a.plane, a.rho_amb,
                              a.theta_amb};
#pragma unroll
      for (int f = 0; f < 6; ++f) {
        if constexpr (V2) {
          const d2 x = ld2(src[f] + o);
          v[f][0] = x.x, v[f][1] = x.y;
        } else {
          v[f][0] = src[f][o];
        }
      }
      double theta[W], tend_th[W], st_qv[W];
#pragma unroll
      for (int j = 0; j < W; ++j) {
        q[j] = IauPoint{v[0][j], v[1][j], v[2][j], v[3][j], v[4][j], v[5][j]};
        const bool own = j == 0 || own1;
        tend_th[j] = 0.0;
        theta[j] = 0.0;
        if (own) theta[j] = iau_cell_head(q[j], a.wgt, rr[j], tend_th[j]);
      }
      // scalars_tend(index_qv) as 207-208 read it: updated by the loop below when qv is a moist
      // scalar, the host's value (0.0 without one) otherwise
      if (!qv_moist) {
        const int64_t so = (int64_t)a.index_qv * a.plane + o;
#pragma unroll
        for (int j = 0; j < W; ++j) st_qv[j] = a.st_zero ? 0.0 : a.scalars_tend[so + j];
      }
      for (int is = a.moist_start; is <= a.moist_end; ++is) {
        const int64_t so = (int64_t)is * a.plane + o;
        double st[W], sa[W], s[W];
        if constexpr (V2) {
          const d2 x = a.st_zero ? d2{0.0, 0.0} : ld2(a.scalars_tend + so);
          const d2 y = ld2(a.scalars_amb + so);
          d2 z;
          if (is == a.index_qv) z = d2{q[0].qv, q[1].qv};
          else z = ld2(a.scalars + so);
          st[0] = x.x, st[1] = x.y, sa[0] = y.x, sa[1] = y.y, s[0] = z.x, s[1] = z.y;
        } else {
          st[0] = a.st_zero ? 0.0 : a.scalars_tend[so];
          sa[0] = a.scalars_amb[so];
          s[0] = is == a.index_qv ? q[0].qv : a.scalars[so];
        }
#pragma unroll
        for (int j = 0; j < W; ++j)
          if (j == 0 || own1) st[j] = iau_scalar_term(q[j], a.wgt, st[j], sa[j], s[j]);
        if (is == a.index_qv) {
#pragma unroll
          for (int j = 0; j < W; ++j) st_qv[j] = st[j];
        }
        if constexpr (V2) st2(a.scalars_tend + so, d2{st[0], st[1]});
        else a.scalars_tend[so] = st[0];
      }
#pragma unroll
      for (int j = 0; j < W; ++j)
        if (j == 0 || own1) rt[j] = iau_cell_tail(q[j], theta[j], tend_th[j], st_qv[j], rt[j]);
    }
    if (a.st_zero) {
      // what the host would have supplied: 0.0 on every plane and element the loop above left alone
      for (int is = 0; is < a.ns; ++is) {
        const bool moist = is >= a.moist_start && is <= a.moist_end;
        const int64_t so = (int64_t)is * a.plane + o;
        if constexpr (V2) {
          if (!(moist && own0)) st2(a.scalars_tend + so, d2{0.0, 0.0});
        } else {
          if (!(moist && own0)) a.scalars_tend[so] = 0.0;
        }
      }
    }
    if constexpr (V2) {
      st2(a.out_rtheta + o, d2{rt[0], rt[1]});
      st2(a.out_rho + o, d2{rr[0], rr[1]});
    } else {
      a.out_rtheta[o] = rt[0];
      a.out_rho[o] = rr[0];
    }
  }
}

}  // namespace mpas

// The Ertel PV budget: atm_compute_pvBudget_diagnostics (core_atmosphere/diagnostics/pv_diagnostics.F:
// 1291-1613) of a block, after the PV diagnostics of the same time level (pv.hip, whose geometry table,
// theta, rho, ertel_pv and iLev_DT it reads) --
//   dtheta_dt_mix = tend_theta_euler / (1 + rvord qv) on all cells                              (:1578-1584)
//   depv_dt_{lw,sw,bl,cu,mp,mix} = ((curl u + 2 Omega) / rho) . grad(dtheta/dt) 1e6 on the owned cells, one
//       per source of heating; depv_dt_diab their sum                                           (:1386-1473)
//   depv_dt_fric = (curl F) . (grad theta / rho) 1e6, F = tend_u_phys + tend_u_euler / rho_edge on the
//       edges (its curl at the vertices, its reconstruction at the cell centres) and tend_w_euler over the
//       density at the interfaces                                                               (:1475-1529)
//   depv_dt_diab_pv, depv_dt_fric_pv: interp_pv of the two on the 2-PVU surface                 (:786-824)
// The halo exchanges between them are the host's (physics_host.hip pvb_run).
//
// Two defined deviations.  The reference overwrites tend_u_phys and tend_w_euler in place (:1479, :1496-1501);
// here both keep their bits and the uncoupled fields go to scratch (k_pvb_cells, k_pvb_edges), so a second
// call gives the same bits and the next step's physics_get_tend does not accumulate onto a polluted array.
// And the outputs are written on the owned cells only: the reference's whole-array depv_dt_diab sum (:1473)
// also covers halo columns that nothing computed.  pv.hip's deviation carries over: at level nVertLevels
// dv_dz takes velCellm (:997).
//
// k_pvb_curl: calc_vertical_curl (:1113-1137) gathered per vertex.  The reference's edge loop adds an edge's
// term to its two vertices in ascending edge index, so a vertex sums its valid edges in ascending local edge
// index -- not in edgesOnVertex order -- with - dcEdge u where it is verticesOnEdge(1, .), + where it is (2, .).
//
// k_pvb_budget: one wavefront per owned column, lane = level, chunks of 64 levels, the cell index
// wave-uniform (table and neighbour indices are scalar loads), no LDS -- k_pv_epv's layout.  The six
// gradients share the neighbour indices and the table's factors; a source that is off is not read and
// writes 0.0.  Levels k - 1 and k + 1 of the column are loaded directly (the neighbouring lanes' cache
// lines) rather than shuffled with a chunk carry as in k_pv_epv: thirteen column fields take part, and the
// direct loads keep the kernel one plain loop over the chunks (the shuffled form was not built or measured).
//
// k_pvb_interp: for iLev_DT = 1, which the fill never gives, the reference reads level 0 (the element before
// the column); the kernel clamps the lower level into the column instead.
//
// fp64, every + - * / in the Fortran's order; the build's -ffp-contract=off keeps them apart.
#pragma once

namespace mpas {

// MPAS_DYC_PVB_* (include/mpas_dycore.h)
constexpr int PVB_ON = 1, PVB_LW = 2, PVB_SW = 4, PVB_BL = 8, PVB_CU = 16, PVB_ALL = 31;
constexpr int PVB_NSRC = 6;  // rthratenlw, rthratensw, rthblten, rthcuten, dtheta_dt_mp, dtheta_dt_mix
// the group's diag fields of one column per cell: the outputs in the order of PvBudget::out, diab, fric, the
// host's dtheta_dt_mp and the call's dtheta_dt_mix
constexpr const char* PVB_CELL_FIELDS[] = {"depv_dt_lw",   "depv_dt_sw",   "depv_dt_bl",   "depv_dt_cu",  "depv_dt_mp",
                                           "depv_dt_mix",  "depv_dt_diab", "depv_dt_fric", "dtheta_dt_mp", "dtheta_dt_mix"};
// the raw tendency of tend_physics behind each source bit, in the order of PvBudget::src
constexpr struct { int bit; const char* name; } PVB_RAW[] = {
    {PVB_LW, "rthratenlw"}, {PVB_SW, "rthratensw"}, {PVB_BL, "rthblten"}, {PVB_CU, "rthcuten"}};

// The hook's host state (mpas_dyc_ctx::pvb): the mask of mpas_dyc_set_pv_budget and the last call under
// mpas_dyc_set_profile (mpas_dyc_get_profile out[13])
struct PvbState {
  int flags = 0;
  double ms = 0.0;
};

struct PvbCurl {
  int nVertices, nEdges, K;
  const int *edgesOnVertex, *verticesOnEdge;
  const double *dcEdge, *areaTriangle, *u;
  double* curl;
};

struct PvBudget {
  int nCellsSolve, K, ME;
  const int *nEdgesOnCell, *cellsOnCell, *verticesOnCell;
  const double *geom, *zgrid, *w, *theta, *rho, *vorticity, *ux, *uy, *uz;
  const double* src[PVB_NSRC];  // nullptr: not associated
  const double *tend_w, *curl, *tx, *ty, *tz;  // the uncoupled tend_w_euler, the vertex curl, tenduX/Y/Z
  double* out[PVB_NSRC];        // depv_dt_lw, sw, bl, cu, mp, mix
  double *diab, *fric;
};

struct PvbInterp {
  int nCellsSolve, K;
  const int* iLev_DT;
  const double *latCell, *ertel_pv, *diab, *fric;
  double *diab_pv, *fric_pv;
};

// dtheta_dt_mix (:1578-1584) and the uncoupled tend_w_euler (:1492-1501) of the cells 1..nCells: one lane
// per (cell, interface)
__global__ void k_pvb_cells(int64_t nCells, int K, const double* __restrict__ tend_theta_euler,
                            const double* __restrict__ qv, const double* __restrict__ rho,
                            const double* __restrict__ tend_w_euler, double* __restrict__ dtheta_dt_mix,
                            double* __restrict__ tend_w) {
  const int64_t n = nCells * (K + 1);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = i / (K + 1);
    const int k = (int)(i - c * (K + 1));
    const int64_t o = c * K;
    if (k < K) dtheta_dt_mix[o + k] = tend_theta_euler[o + k] / (1.0 + PV_RVORD * qv[o + k]);
    const double tw = tend_w_euler[i];
    if (k == 0) tend_w[i] = tw / rho[o];
    else if (k == K) tend_w[i] = tw / rho[o + K - 1];
    else tend_w[i] = tw / (.5 * (rho[o + k - 1] + rho[o + k]));
  }
}

// tend_u_phys + tend_u_euler / rho_edge (:1477-1481) of the edges 1..nEdges; tend_u_phys == nullptr (no
// physics_get_tend on the device): the literal 0.0, still added as the reference adds its zero array
__global__ void k_pvb_edges(int64_t n, const double* __restrict__ tend_u_phys, const double* __restrict__ tend_u_euler,
                            const double* __restrict__ rho_edge, double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double phys = tend_u_phys ? tend_u_phys[i] : 0.0;
    out[i] = phys + tend_u_euler[i] / rho_edge[i];
  }
}

// calc_vertical_curl of every level (:1483-1485) on the vertices 1..nVertices: one wavefront per vertex
__global__ __launch_bounds__(PV_THREADS) void k_pvb_curl(PvbCurl a) {
  const int lane = threadIdx.x & 63;
  const int v = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * PV_WAVES + (threadIdx.x >> 6)));
  if (v >= a.nVertices) return;
  const int K = a.K;
  int e0 = a.edgesOnVertex[3 * (int64_t)v], e1 = a.edgesOnVertex[3 * (int64_t)v + 1], e2 = a.edgesOnVertex[3 * (int64_t)v + 2];
  int t;  // ascending local edge index; the garbage edge (nEdges) sorts last
  if (e0 > e1) t = e0, e0 = e1, e1 = t;
  if (e1 > e2) t = e1, e1 = e2, e2 = t;
  if (e0 > e1) t = e0, e0 = e1, e1 = t;
  const int e[3] = {e0, e1, e2};
  int sgn[3];
  double dc[3];
  for (int i = 0; i < 3; ++i) {
    sgn[i] = 0, dc[i] = 0.0;
    if (e[i] < 0 || e[i] >= a.nEdges) continue;  // the garbage slot
    if (a.verticesOnEdge[2 * (int64_t)e[i]] == v) sgn[i] = -1;
    else if (a.verticesOnEdge[2 * (int64_t)e[i] + 1] == v) sgn[i] = 1;
    dc[i] = a.dcEdge[e[i]];
  }
  const double area = a.areaTriangle[v];
  for (int k = lane; k < K; k += 64) {
    double r = 0.0;
    for (int i = 0; i < 3; ++i) {
      if (sgn[i] < 0) r = r - dc[i] * a.u[(int64_t)e[i] * K + k];
      else if (sgn[i] > 0) r = r + dc[i] * a.u[(int64_t)e[i] * K + k];
    }
    a.curl[(int64_t)v * K + k] = r / area;
  }
}

// level k of a column field and its vertical neighbours (0.0 past the column's ends, where pv_vert reads none)
struct PvbCol { double m, c, p; };
__device__ __forceinline__ PvbCol pvb_col(const double* __restrict__ f, int64_t o, int k, int K) {
  PvbCol v;
  v.c = f[o + k];
  v.m = k > 0 ? f[o + k - 1] : 0.0;
  v.p = k + 1 < K ? f[o + k + 1] : 0.0;
  return v;
}

// calc_gradxu_cell (:901-1022) without local2FullVorticity at 0-based level k of owned cell c: the curl of
// (ux, uy, uz, w) with the vertex field `vort` as its vertical component
__device__ __forceinline__ void pvb_gradxu(const PvBudget& a, const double* __restrict__ t, const int* __restrict__ coc,
                                           const int* __restrict__ voc, int ne, int64_t o, int64_t oz, int k,
                                           const PvbCol& zc, const double* __restrict__ ux, const double* __restrict__ uy,
                                           const double* __restrict__ uz, const double* __restrict__ w,
                                           const double* __restrict__ vort, double& g0, double& g1, double& g2) {
  const int K = a.K, ME = a.ME;
  const double vol = t[6], area = t[10];
  const double w0 = .5 * (w[oz + k + 1] + w[oz + k]);
  double wx = 0.0, wy = 0.0, vv = 0.0;
  for (int i = 0; i < ne; ++i) {
    const int64_t nb = coc[i];
    const double wn = .5 * (w[nb * (K + 1) + k + 1] + w[nb * (K + 1) + k]);
    const double we = 0.5 * (wn + w0);
    wx = wx + we * t[PV_HDR + i];
    wy = wy + we * t[PV_HDR + ME + i];
    vv = vv + t[PV_HDR + 2 * ME + i] * vort[(int64_t)voc[i] * K + k] / area;
  }
  const double dw_dx = wx / vol, dw_dy = wy / vol;
  const PvbCol x = pvb_col(ux, o, k, K), y = pvb_col(uy, o, k, K), z = pvb_col(uz, o, k, K);
  const double ud0 = pv_dot(x.c, y.c, z.c, t[0], t[1], t[2]), vd0 = pv_dot(x.c, y.c, z.c, t[3], t[4], t[5]);
  const double udp = pv_dot(x.p, y.p, z.p, t[0], t[1], t[2]), vdp = pv_dot(x.p, y.p, z.p, t[3], t[4], t[5]);
  const double udm = pv_dot(x.m, y.m, z.m, t[0], t[1], t[2]), vdm = pv_dot(x.m, y.m, z.m, t[3], t[4], t[5]);
  const double du_dz = pv_vert(ud0, udp, udm, zc.c, zc.p, zc.m, k, K);
  const double dv_dz = pv_vert(vd0, vdp, vdm, zc.c, zc.p, zc.m, k, K);  // level K: velCellm
  g0 = dw_dy - dv_dz;
  g1 = du_dz - dw_dx;
  g2 = vv;
}

__global__ __launch_bounds__(PV_THREADS) void k_pvb_budget(PvBudget a) {
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * PV_WAVES + (threadIdx.x >> 6)));
  if (c >= a.nCellsSolve) return;
  const int K = a.K, ME = a.ME;
  const int ne = a.nEdgesOnCell[c];
  const int64_t o = (int64_t)c * K, oz = (int64_t)c * (K + 1);
  const double* __restrict__ t = a.geom + (int64_t)c * (PV_HDR + 3 * ME);
  const int* __restrict__ coc = a.cellsOnCell + (int64_t)c * ME;
  const int* __restrict__ voc = a.verticesOnCell + (int64_t)c * ME;
  const double vol = t[6];
  for (int k = lane; k < K; k += 64) {
    PvbCol zc;  // calc_heightCellCenter of the three levels
    zc.c = 0.5 * (a.zgrid[oz + k] + a.zgrid[oz + k + 1]);
    zc.m = k > 0 ? 0.5 * (a.zgrid[oz + k - 1] + a.zgrid[oz + k]) : 0.0;
    zc.p = k + 1 < K ? 0.5 * (a.zgrid[oz + k + 1] + a.zgrid[oz + k + 2]) : 0.0;
    const double rho = a.rho[o + k];
    // the diabatic terms (:1386-1473): gradxu / rho is ertel_pv's, Earth vorticity included
    double g0, g1, g2;
    pvb_gradxu(a, t, coc, voc, ne, o, oz, k, zc, a.ux, a.uy, a.uz, a.w, a.vorticity, g0, g1, g2);
    g0 = (g0 + t[7]) / rho, g1 = (g1 + t[8]) / rho, g2 = (g2 + t[9]) / rho;
    PvbCol f[PVB_NSRC];
    double sx[PVB_NSRC], sy[PVB_NSRC];
#pragma unroll
    for (int j = 0; j < PVB_NSRC; ++j) {
      sx[j] = sy[j] = 0.0;
      if (a.src[j]) f[j] = pvb_col(a.src[j], o, k, K);
    }
    const PvbCol th = pvb_col(a.theta, o, k, K);
    double tx = 0.0, ty = 0.0;
    for (int i = 0; i < ne; ++i) {
      const int64_t nb = coc[i];
      const double c1 = t[PV_HDR + i], c2 = t[PV_HDR + ME + i];
#pragma unroll
      for (int j = 0; j < PVB_NSRC; ++j) {
        if (!a.src[j]) continue;
        const double fe = 0.5 * (a.src[j][nb * K + k] + f[j].c);
        sx[j] = sx[j] + fe * c1;
        sy[j] = sy[j] + fe * c2;
      }
      const double te = 0.5 * (a.theta[nb * K + k] + th.c);
      tx = tx + te * c1;
      ty = ty + te * c2;
    }
    double d[PVB_NSRC];
#pragma unroll
    for (int j = 0; j < PVB_NSRC; ++j) {
      d[j] = 0.0;
      if (a.src[j]) {
        const double h0 = sx[j] / vol, h1 = sy[j] / vol;
        const double h2 = pv_vert(f[j].c, f[j].p, f[j].m, zc.c, zc.p, zc.m, k, K);
        d[j] = pv_dot(g0, g1, g2, h0, h1, h2) * 1.0e6;
      }
      a.out[j][o + k] = d[j];
    }
    a.diab[o + k] = ((((d[0] + d[1]) + d[2]) + d[3]) + d[4]) + d[5];
    // the frictional term (:1503-1529): grad theta / rho, and the curl of the tendencies without the Earth's
    const double th0 = (tx / vol) / rho, th1 = (ty / vol) / rho;
    const double th2 = pv_vert(th.c, th.p, th.m, zc.c, zc.p, zc.m, k, K) / rho;
    double x0, x1, x2;
    pvb_gradxu(a, t, coc, voc, ne, o, oz, k, zc, a.tx, a.ty, a.tz, a.tend_w, a.curl, x0, x1, x2);
    a.fric[o + k] = pv_dot(x0, x1, x2, th0, th1, th2) * 1.0e6;
  }
}

// interp_pvBudget_diagnostics (:786-824) on the owned cells, one lane per cell, with the iLev_DT and
// ertel_pv the PV diagnostics just produced
__global__ void k_pvb_interp(PvbInterp a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nCellsSolve) return;
  const int K = a.K, iLev = a.iLev_DT[c];
  const int64_t o = (int64_t)c * K;
  const bool inside = iLev >= 1 && iLev <= K;
  // 0-based levels iLev and iLev - 1; the fill gives no iLev_DT of 1 (0, or 2 and up), where the reference
  // would read level 0: kl stays inside the column
  const int kh = inside ? iLev - 1 : 0, kl = inside && iLev >= 2 ? iLev - 2 : 0;
  double frac = 0.0;
  if (inside) {
    const double valInterpCell = PV_PVU * copysign(1.0, a.latCell[c]);
    const double valh = a.ertel_pv[o + kh], vall = a.ertel_pv[o + kl];
    const double dv_dl = valh - vall;
    frac = fabs(dv_dl) < 1.e-6 ? 0.5 : (valInterpCell - vall) / dv_dl;
  }
  a.diab_pv[c] = pv_interp(iLev, K, frac, a.diab[o + K - 1], a.diab[o], a.diab[o + kl], a.diab[o + kh]);
  a.fric_pv[c] = pv_interp(iLev, K, frac, a.fric[o + K - 1], a.fric[o], a.fric[o + kl], a.fric[o + kh]);
}

}  // namespace mpas

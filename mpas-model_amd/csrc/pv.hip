// The Ertel PV and dynamic-tropopause diagnostics: atm_compute_pv_diagnostics
// (core_atmosphere/diagnostics/pv_diagnostics.F:1218-1289) of a block --
//   theta = theta_m / (1 + rvord qv), rho = rho_zz zz on all cells                          (:1253-1258)
//   ertel_pv = ((curl u + 2 Omega) / rho) . grad theta  1e6 on the owned cells: calc_epv (:1139-1216) with
//       calc_gradxu_cell / calc_grad_cell and their helpers (:147-422, :901-1111)
//   iLev_DT on all cells: floodFill_tropo (:581-716), the level above the highest cell-level below 2 PVU
//       that is connected to the near-surface seeds
//   u_pv, v_pv, theta_pv, vort_pv on the owned cells: interp_pv_diagnostics / interp_pv (:718-784, :826-899)
// The halo exchanges between them are the host's (physics_host.hip pv_run).  The PV budget (calc_pvBudget,
// interp_pvBudget_diagnostics) is pvbudget.hip, which reads this file's table, pv_dot, pv_vert and pv_interp;
// floodFill_strato is never called by the reference.
//
// k_pv_geom: everything of calc_gradxu_cell / calc_grad_cell that does not depend on the level, once per
// owned cell, with the operations the Fortran repeats at every level: the two normalised tangent vectors;
// per edge slot (dvEdge * 100.0) times the dot product of the twice-normalised (calc_horizDeriv_fv
// normalises the already normalised, signed vector again), sign-flipped edge normal with each tangent
// vector; volumeCell = areaCell * (running sum of 100.0 / nEdgesOnCell); the Earth-vorticity components;
// the cell's kite area at each of its vertices (elementIndexInArray: the first match).  Dot products and
// squared norms are ((0.0 + a1 b1) + a2 b2) + a3 b3.  A derived table (Block::pv.geom), rebuilt after a
// set_field of a mesh array.
//
// k_pv_epv: one wavefront per owned column, lane = level, looping over chunks of 64 levels: one source for
// every nVertLevels.  The cell index is wave-uniform, so the table and the neighbour indices are scalar
// loads; the neighbour columns of theta and w and the vertex columns of vorticity are coalesced gathers;
// level k - 1 and k + 1 of the column come from the neighbouring lanes, across chunks from the chunk
// before (carried) and the chunk after (loaded one iteration ahead).  calc_verticalVorticity_cell adds
// kite * vort / areaCell in verticesOnCell order.  Any nEdgesOnCell, by a run-time loop.  No LDS.
//
// One defined deviation: at level nVertLevels the reference forms dv_dz from velCellp, a local it never
// set there (:997), so its value is undefined; here that line takes velCellm, as the u line two above it.
//
// The fill: floodFill_tropo's result is the unique fixed point of its sweeps -- the candidate cell-levels
// (ertel_pv sgnHemi - 2 < 0) connected to a seed (levels 1..min(K, 3)) through vertical neighbours and
// same-level horizontal neighbours -- so the order of the sweeps does not matter.  Candidates and members
// are bit masks, ceil(K / 64) 64-bit words per cell, word-major.  k_pv_sweep, one lane per cell: a word's
// members are its own and its neighbours' of the sweep before, masked by the candidates; then every run of
// candidates that holds a member is filled, upwards by the carry chain of (candidates + members), downwards
// by the same on the bit-reversed words, carrying across words.  It writes a second buffer (reads never race
// with writes) and, where a word changed, a plain store of 1 to the block's flag.  A neighbour outside the
// block is the garbage slot, whose words stay 0.
//
// fp64, every + - * / sqrt in the Fortran's order; the build's -ffp-contract=off keeps them apart.
// Halo cells and garbage slots of the 2-D outputs are never written (iLev_DT: the garbage slot).
#pragma once

namespace mpas {

constexpr int PV_THREADS = 256;
constexpr int PV_WAVES = PV_THREADS / 64;
constexpr double PV_OMEGA = 7.29212e-5;   // mpas_constants: omega
constexpr double PV_RVORD = RV / RGAS;    // mpas_constants: rvord
constexpr double PV_PVU = 2.0;            // pvuVal (:1282)
constexpr int PV_SEED_LEVELS = 3;         // :643
constexpr int PV_HDR = 12;                // x1[3], x2[3], vol, ev[3], areaCell, pad; then g1, g2, kite per edge slot
constexpr int PV_BATCH = 4;               // sweeps between two read-backs of the flags
// the mesh inputs of the group that the host has set (Block::pv.set)
constexpr int PV_SET_TANGENT = 1, PV_SET_VERTICAL = 2, PV_SET_NORMALS = 4;

// The hook's host state (mpas_dyc_ctx::pv): the switch of mpas_dyc_set_pv, the last call under
// mpas_dyc_set_profile (mpas_dyc_get_profile out[9]) and the sweeps of its fill that changed something,
// the most over the blocks (out[10])
struct PvState {
  int on = 0;
  double ms = 0.0;
  int sweeps = 0;
};

// A block's derived table and fill buffers, on the device
struct PvBlock {
  double* geom = nullptr;                 // nCellsSolve x (PV_HDR + 3 maxEdges)
  unsigned long long *cand = nullptr, *mem[2] = {nullptr, nullptr};  // words x (nCells + 1)
  int* flags = nullptr;                   // PV_BATCH words
  int64_t geom_n = 0, words_n = 0;        // what the buffers were allocated for
  bool ready = false;                     // geom describes the mesh arrays as they are
  int set = 0;                            // PV_SET_*
};

struct PvGeomArgs {
  int nCellsSolve, ME;
  const int *nEdgesOnCell, *edgesOnCell, *verticesOnCell, *cellsOnEdge, *cellsOnVertex;
  const double *cellTangentPlane, *localVerticalUnitVectors, *edgeNormalVectors, *dvEdge, *areaCell, *kiteAreasOnVertex;
  double* geom;
};

struct PvEpv {
  int nCellsSolve, K, ME;
  const int *nEdgesOnCell, *cellsOnCell, *verticesOnCell;
  const double *geom, *zgrid, *w, *theta, *rho, *vorticity, *ux, *uy, *uz;
  double* ertel_pv;
};

struct PvInterp {
  int nCells, nCellsSolve, K, ME, words;
  const int *nEdgesOnCell, *verticesOnCell;
  const unsigned long long* mem;
  const double *geom, *latCell, *ertel_pv, *uzonal, *umeridional, *theta, *vorticity;
  int* iLev_DT;
  double *u_pv, *v_pv, *theta_pv, *vort_pv;
};

__device__ __forceinline__ double pv_dot(double a1, double a2, double a3, double b1, double b2, double b3) {
  return ((0.0 + a1 * b1) + a2 * b2) + a3 * b3;
}
__device__ __forceinline__ void pv_normalize(double& a, double& b, double& c) {
  const double mag = sqrt(((0.0 + a * a) + b * b) + c * c);
  a = a / mag, b = b / mag, c = c / mag;
}

// the preamble (:1253-1258) on the cells 1..nCells
__global__ void k_pv_theta_rho(int64_t n, const double* __restrict__ theta_m, const double* __restrict__ qv,
                               const double* __restrict__ rho_zz, const double* __restrict__ zz, double* __restrict__ theta,
                               double* __restrict__ rho) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    theta[i] = theta_m[i] / (1.0 + PV_RVORD * qv[i]);
    rho[i] = rho_zz[i] * zz[i];
  }
}

__global__ void k_pv_geom(PvGeomArgs a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nCellsSolve) return;
  const int ME = a.ME, ne = a.nEdgesOnCell[c];
  double* __restrict__ t = a.geom + (int64_t)c * (PV_HDR + 3 * ME);
  const double* __restrict__ tp = a.cellTangentPlane + 6 * (int64_t)c;
  double x1[3] = {tp[0], tp[1], tp[2]}, x2[3] = {tp[3], tp[4], tp[5]};
  pv_normalize(x1[0], x1[1], x1[2]);
  pv_normalize(x2[0], x2[1], x2[2]);
  const double* __restrict__ x3 = a.localVerticalUnitVectors + 3 * (int64_t)c;
  const double area = a.areaCell[c];
  double avg = 0.0;
  for (int i = 0; i < ME; ++i) {
    double g1 = 0.0, g2 = 0.0, kite = 0.0;
    if (i < ne) {
      const int e = a.edgesOnCell[(int64_t)c * ME + i];
      const double sign = a.cellsOnEdge[2 * (int64_t)e] == c ? 1.0 : -1.0;  // fluxSign
      double n1 = a.edgeNormalVectors[3 * (int64_t)e], n2 = a.edgeNormalVectors[3 * (int64_t)e + 1],
             n3 = a.edgeNormalVectors[3 * (int64_t)e + 2];
      pv_normalize(n1, n2, n3);
      n1 = n1 * sign, n2 = n2 * sign, n3 = n3 * sign;
      pv_normalize(n1, n2, n3);  // calc_horizDeriv_fv, again
      const double face = a.dvEdge[e] * 100.0;
      g1 = face * pv_dot(n1, n2, n3, x1[0], x1[1], x1[2]);
      g2 = face * pv_dot(n1, n2, n3, x2[0], x2[1], x2[2]);
      avg = avg + 100.0;
      const int v = a.verticesOnCell[(int64_t)c * ME + i];
      int j = 0;  // elementIndexInArray: the first match (a vertex of an owned cell holds the cell)
      if (a.cellsOnVertex[3 * (int64_t)v] != c) j = a.cellsOnVertex[3 * (int64_t)v + 1] == c ? 1 : 2;
      kite = a.kiteAreasOnVertex[3 * (int64_t)v + j];
    }
    t[PV_HDR + i] = g1, t[PV_HDR + ME + i] = g2, t[PV_HDR + 2 * ME + i] = kite;
  }
  avg = avg / (double)ne;
  const double e_vort = 2.0 * PV_OMEGA;
  for (int j = 0; j < 3; ++j) t[j] = x1[j], t[3 + j] = x2[j];
  t[6] = area * avg;
  t[7] = pv_dot(0.0, 0.0, e_vort, x1[0], x1[1], x1[2]);
  t[8] = pv_dot(0.0, 0.0, e_vort, x2[0], x2[1], x2[2]);
  t[9] = pv_dot(0.0, 0.0, e_vort, x3[0], x3[1], x3[2]);
  t[10] = area;
  t[11] = 0.0;
}

// what the vertical differences read of level k of the column: the wind along the two tangent vectors,
// theta, and the height of the cell centre
struct PvLev { double ud, vd, th, zc; };

__device__ __forceinline__ PvLev pv_level(const PvEpv& a, const double* __restrict__ t, int64_t o, int64_t oz, int k) {
  PvLev v{};
  if (k >= a.K) return v;
  const double ux = a.ux[o + k], uy = a.uy[o + k], uz = a.uz[o + k];
  v.ud = pv_dot(ux, uy, uz, t[0], t[1], t[2]);
  v.vd = pv_dot(ux, uy, uz, t[3], t[4], t[5]);
  v.th = a.theta[o + k];
  v.zc = 0.5 * (a.zgrid[oz + k] + a.zgrid[oz + k + 1]);
  return v;
}
// level k + 1: the next lane's, for lane 63 lane 0's of the next chunk
__device__ __forceinline__ double pv_up(double cur, double nxt, int lane) {
  const double x = __shfl(cur, (lane + 1) & 63, 64), y = __shfl(nxt, 0, 64);
  return lane == 63 ? y : x;
}
// level k - 1: the lane before, for lane 0 lane 63's of the chunk before
__device__ __forceinline__ double pv_down(double cur, double carry, int lane) {
  const double x = __shfl(cur, (lane + 63) & 63, 64);
  return lane == 0 ? carry : x;
}
// calc_vertDeriv_one at the column's ends, calc_vertDeriv_center inside (:398-422)
__device__ __forceinline__ double pv_vert(double v0, double vp, double vm, double z0, double zp, double zm, int k, int K) {
  if (k == 0) return (vp - v0) / (zp - z0);
  if (k == K - 1) return (v0 - vm) / (z0 - zm);
  const double dzp = (vp - v0) / (zp - z0), dzm = (v0 - vm) / (z0 - zm);
  return 0.5 * (dzp + dzm);
}

__global__ __launch_bounds__(PV_THREADS) void k_pv_epv(PvEpv a) {
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * PV_WAVES + (threadIdx.x >> 6)));
  if (c >= a.nCellsSolve) return;
  const int K = a.K, ME = a.ME;
  const int ne = a.nEdgesOnCell[c];
  const int64_t o = (int64_t)c * K, oz = (int64_t)c * (K + 1);
  const double* __restrict__ t = a.geom + (int64_t)c * (PV_HDR + 3 * ME);
  const int* __restrict__ coc = a.cellsOnCell + (int64_t)c * ME;
  const int* __restrict__ voc = a.verticesOnCell + (int64_t)c * ME;
  const double vol = t[6], area = t[10];
  const int nchunk = (K + 63) / 64;
  PvLev cur = pv_level(a, t, o, oz, lane), nxt, carry{};
  for (int j = 0; j < nchunk; ++j) {
    const int k = lane + 64 * j;
    nxt = pv_level(a, t, o, oz, k + 64);
    PvLev up, dn;
    up.ud = pv_up(cur.ud, nxt.ud, lane), up.vd = pv_up(cur.vd, nxt.vd, lane);
    up.th = pv_up(cur.th, nxt.th, lane), up.zc = pv_up(cur.zc, nxt.zc, lane);
    dn.ud = pv_down(cur.ud, carry.ud, lane), dn.vd = pv_down(cur.vd, carry.vd, lane);
    dn.th = pv_down(cur.th, carry.th, lane), dn.zc = pv_down(cur.zc, carry.zc, lane);
    carry.ud = __shfl(cur.ud, 63, 64), carry.vd = __shfl(cur.vd, 63, 64);
    carry.th = __shfl(cur.th, 63, 64), carry.zc = __shfl(cur.zc, 63, 64);
    if (k < K) {
      const double w0 = .5 * (a.w[oz + k + 1] + a.w[oz + k]);
      const double t0 = cur.th;
      double wx = 0.0, wy = 0.0, tx = 0.0, ty = 0.0, vv = 0.0;
      for (int i = 0; i < ne; ++i) {
        const int64_t nb = coc[i];
        const double g1 = t[PV_HDR + i], g2 = t[PV_HDR + ME + i], kite = t[PV_HDR + 2 * ME + i];
        const double wn = .5 * (a.w[nb * (K + 1) + k + 1] + a.w[nb * (K + 1) + k]);
        const double we = 0.5 * (wn + w0);
        wx = wx + we * g1;
        wy = wy + we * g2;
        const double te = 0.5 * (a.theta[nb * K + k] + t0);
        tx = tx + te * g1;
        ty = ty + te * g2;
        vv = vv + kite * a.vorticity[(int64_t)voc[i] * K + k] / area;
      }
      const double dw_dx = wx / vol, dw_dy = wy / vol;
      const double du_dz = pv_vert(cur.ud, up.ud, dn.ud, cur.zc, up.zc, dn.zc, k, K);
      const double dv_dz = pv_vert(cur.vd, up.vd, dn.vd, cur.zc, up.zc, dn.zc, k, K);  // level K: velCellm
      const double rho = a.rho[o + k];
      const double g0 = ((dw_dy - dv_dz) + t[7]) / rho;
      const double g1 = ((du_dz - dw_dx) + t[8]) / rho;
      const double g2 = (vv + t[9]) / rho;
      const double th0 = tx / vol, th1 = ty / vol;
      const double th2 = pv_vert(cur.th, up.th, dn.th, cur.zc, up.zc, dn.zc, k, K);
      a.ertel_pv[o + k] = pv_dot(g0, g1, g2, th0, th1, th2) * 1.0e6;
    }
    cur = nxt;
  }
}

// candInTropo (:631-638) and the seeds (:643-652) of every cell of the block: one wavefront per cell,
// a word of 64 levels is one ballot
__global__ __launch_bounds__(PV_THREADS) void k_pv_cand(int nCells, int K, int words, const double* __restrict__ latCell,
                                                        const double* __restrict__ ertel_pv,
                                                        unsigned long long* __restrict__ cand,
                                                        unsigned long long* __restrict__ mem) {
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * PV_WAVES + (threadIdx.x >> 6)));
  if (c >= nCells) return;
  const double sgnHemi = copysign(1.0, latCell[c]);  // sign(1.0, lat) is never 0.0
  const int seeds = K < PV_SEED_LEVELS ? K : PV_SEED_LEVELS;
  for (int j = 0; j < words; ++j) {
    const int k = lane + 64 * j;
    bool in = false;
    if (k < K) in = ertel_pv[(int64_t)c * K + k] * sgnHemi - PV_PVU < 0.0;
    const unsigned long long word = __ballot(in);
    if (lane == 0) {
      cand[(int64_t)j * (nCells + 1) + c] = word;
      mem[(int64_t)j * (nCells + 1) + c] = j == 0 ? word & ((1ull << seeds) - 1ull) : 0ull;
    }
  }
}

// the runs of candidates `c` that hold a member of `m` (a subset of c), filled from each member towards
// the higher bits: the carry of c + m ripples through a run; `carry` enters at bit 0 and leaves at bit 63
__device__ __forceinline__ unsigned long long pv_smear(unsigned long long c, unsigned long long m, unsigned& carry) {
  const unsigned long long s = c + m, s2 = s + carry;
  carry = (s < c) | (s2 < s);
  return m | ((s2 ^ c) & c);
}

// One sweep of the fill, one lane per cell
__global__ void k_pv_sweep(int nCells, int words, int ME, const int* __restrict__ nEdgesOnCell,
                           const int* __restrict__ cellsOnCell, const unsigned long long* __restrict__ cand,
                           const unsigned long long* __restrict__ prev, unsigned long long* out, int* __restrict__ flag) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nCells) return;
  const int64_t n1 = (int64_t)nCells + 1;
  const int ne = nEdgesOnCell[c];
  unsigned carry = 0;
  for (int w = 0; w < words; ++w) {
    const int64_t idx = w * n1 + c;
    unsigned long long m = prev[idx];
    for (int i = 0; i < ne; ++i) m |= prev[w * n1 + cellsOnCell[(int64_t)c * ME + i]];
    const unsigned long long cw = cand[idx];
    out[idx] = pv_smear(cw, m & cw, carry);
  }
  carry = 0;
  bool changed = false;
  for (int w = words - 1; w >= 0; --w) {
    const int64_t idx = w * n1 + c;
    const unsigned long long m = __brevll(pv_smear(__brevll(cand[idx]), __brevll(out[idx]), carry));
    changed = changed || m != prev[idx];
    out[idx] = m;
  }
  if (changed) *flag = 1;
}

// interp_pv (:826-899) of one column once its level fraction is known
__device__ __forceinline__ double pv_interp(int iLev, int K, double frac, double f_top, double f_bottom, double fl,
                                            double fh) {
  if (iLev > K) return f_top;
  if (iLev < 1) return f_bottom;
  const double dv_dl = fh - fl;
  return fl + dv_dl * frac;
}
// calc_verticalVorticity_cell (:245-267) at 0-based level k
__device__ __forceinline__ double pv_vvort(const PvInterp& a, const double* __restrict__ t, int c, int ne, int k) {
  double vv = 0.0;
  for (int i = 0; i < ne; ++i)
    vv = vv + t[PV_HDR + 2 * a.ME + i] * a.vorticity[(int64_t)a.verticesOnCell[(int64_t)c * a.ME + i] * a.K + k] / t[10];
  return vv;
}

// iLev_DT (:699-714) on the cells 1..nCells and the four interpolated fields on the owned cells, one lane per cell
__global__ void k_pv_interp(PvInterp a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nCells) return;
  const int K = a.K;
  int top = -1;  // the highest member level, 0-based
  for (int w = a.words - 1; w >= 0 && top < 0; --w) {
    const unsigned long long m = a.mem[(int64_t)w * (a.nCells + 1) + c];
    if (m) top = 64 * w + 63 - __clzll((long long)m);
  }
  const int iLev = top >= 0 ? top + 2 : 0;
  a.iLev_DT[c] = iLev;
  if (c >= a.nCellsSolve) return;
  const int64_t o = (int64_t)c * K;
  const bool inside = iLev >= 1 && iLev <= K;
  const int kh = inside ? iLev - 1 : 0, kl = inside ? iLev - 2 : 0;  // 0-based levels iLev and iLev - 1
  double frac = 0.0;
  if (inside) {
    const double valInterpCell = PV_PVU * copysign(1.0, a.latCell[c]);
    const double valh = a.ertel_pv[o + kh], vall = a.ertel_pv[o + kl];
    const double dv_dl = valh - vall;
    frac = fabs(dv_dl) < 1.e-6 ? 0.5 : (valInterpCell - vall) / dv_dl;
  }
  a.u_pv[c] = pv_interp(iLev, K, frac, a.uzonal[o + K - 1], a.uzonal[o], a.uzonal[o + kl], a.uzonal[o + kh]);
  a.v_pv[c] = pv_interp(iLev, K, frac, a.umeridional[o + K - 1], a.umeridional[o], a.umeridional[o + kl],
                        a.umeridional[o + kh]);
  a.theta_pv[c] = pv_interp(iLev, K, frac, a.theta[o + K - 1], a.theta[o], a.theta[o + kl], a.theta[o + kh]);
  // vVort only at the two levels it is read at
  const double* __restrict__ t = a.geom + (int64_t)c * (PV_HDR + 3 * a.ME);
  const int ne = a.nEdgesOnCell[c];
  const double v1 = pv_vvort(a, t, c, ne, inside ? kl : iLev > K ? K - 1 : 0);
  const double v2 = inside ? pv_vvort(a, t, c, ne, kh) : v1;
  a.vort_pv[c] = pv_interp(iLev, K, frac, v1, v1, v1, v2);
}

}  // namespace mpas

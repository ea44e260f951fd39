// The coupling of the physics tendencies to the dynamics: physics_get_tend
// (core_atmosphere/physics/mpas_atmphys_todynamics.F:59-434), called from atm_srk3 after the moist
// coefficients and before the IAU add (mpas_atm_time_integration.F:424-449).  The raw tendencies of the
// PBL, convection and radiation schemes (the tend_physics pool: rublten ... rthratensw, cell-centred,
// independent of the dycore's state) become tend_ru_physics, tend_rtheta_physics, tend_rho_physics and
// tend.scalars_tend, the arrays a host that couples by itself uploads (mpas_dyc_set_physics).
//
// Edge kernel: tend_toEdges (:494-510) for the PBL's and a Tiedtke scheme's wind tendencies on every edge
// of the block, tend_u_phys (:334, :393-394) and tend_ru_physics on the owned edges (:337-341, :396-400).
// One group of 16, 32 or 64 lanes per edge, a lane per level (and a stride of the group above 64 levels):
// the two cells' columns are gathered as contiguous rows, the edge's own values are uniform over the group.
// The four projection coefficients are formed per lane from the mesh vectors, each dot product as
// (n1 e1 + n2 e2) + n3 e3; the twelve doubles they read are the same for every lane of the group.
//
// Cell kernel (:343-432): a pure stream, flat over the (cell, level) image like iau.hip's, two values per
// lane when (nCells + 1) K is even.  Every element outside the owned range, the garbage slot included,
// gets 0.0 in every output, and so does every plane of scalars_tend that no scheme touches (:178).
// Every + * / in the Fortran's left-to-right order; the build's -ffp-contract=off keeps them apart.
#pragma once

namespace mpas {

constexpr int TODYN_THREADS = 256;
constexpr int TODYN_MAX_BLOCKS = 2048;  // 8 workgroups per CU; the rest of the image by grid stride
constexpr int TODYN_MAX_TERMS = 9;      // rq{v,c,i}blten, rniblten, rq{v,c,i}cuten, rqrcuten, rqscuten

// MPAS_DYC_TODYN_* of include/mpas_dycore.h
enum : int {
  TODYN_PBL = 1, TODYN_PBL_MYNN = 2, TODYN_CU = 4, TODYN_CU_KF = 8, TODYN_CU_WINDS = 16, TODYN_LW = 32, TODYN_SW = 64,
  TODYN_RQVDYNTEN = 128, TODYN_ALL = 255
};
// mesh.east / north have been set on a block (Block::todyn_set)
enum : int { TODYN_SET_EAST = 1, TODYN_SET_NORTH = 2 };
// the raw tendencies (tend_physics pool, (K, nCells + 1) each)
constexpr const char* TODYN_CELL_FIELDS[] = {
    "rublten",  "rvblten",  "rthblten", "rqvblten", "rqcblten", "rqiblten", "rniblten",   "rucuten",   "rvcuten",
    "rthcuten", "rqvcuten", "rqccuten", "rqrcuten", "rqicuten", "rqscuten", "rthratenlw", "rthratensw"};

// The hook's host state (mpas_dyc_ctx::todyn): the flags, and the 0-based scalar indices (-1: absent, its
// terms are skipped)
struct TodynState {
  int flags = 0;
  int iqc = -1, iqr = -1, iqi = -1, iqs = -1, ini = -1;
  double ms = 0.0;  // mpas_dyc_get_profile out[12]
};

struct TodynEdges {
  int nEdges, nEdgesSolve, nCells, K;
  int group;      // lanes per edge: 16, 32 or 64
  int pbl, cu;    // project rublten / rvblten; rucuten / rvcuten
  const int* cellsOnEdge;
  const double *east, *north, *edgeNormalVectors;  // (3, nCells + 1), (3, nCells + 1), (3, nEdges + 1)
  const double *rublten, *rvblten, *rucuten, *rvcuten, *rho_edge;
  double *rublten_Edge, *rucuten_Edge, *tend_u_phys, *tend_ru_physics;
};

// edgeNormalVectors(:,iEdge) . v(:,cell), :498-500
__device__ __forceinline__ double todyn_dot(const double* __restrict__ n, const double* __restrict__ v) {
  return n[0] * v[0] + n[1] * v[1] + n[2] * v[2];
}
// Ux(cell1) 0.5 dot + Uy(cell1) 0.5 dot + Ux(cell2) 0.5 dot + Uy(cell2) 0.5 dot, :498-509
__device__ __forceinline__ double todyn_project(double ux1, double uy1, double ux2, double uy2, double e1, double n1,
                                                double e2, double n2) {
  return ux1 * 0.5 * e1 + uy1 * 0.5 * n1 + ux2 * 0.5 * e2 + uy2 * 0.5 * n2;
}

__global__ __launch_bounds__(TODYN_THREADS) void k_todyn_edges(TodynEdges a) {
  const int per_block = TODYN_THREADS / a.group;
  const int lane = threadIdx.x % a.group;
  const int K = a.K;
  // edges 0 .. nEdges - 1, and the garbage slot nEdges (tend_ru_physics alone: 0.0)
  for (int64_t e = (int64_t)blockIdx.x * per_block + threadIdx.x / a.group; e <= a.nEdges;
       e += (int64_t)gridDim.x * per_block) {
    const int64_t row = e * K;
    if (e == a.nEdges || !(a.pbl || a.cu)) {
      for (int k = lane; k < K; k += a.group) a.tend_ru_physics[row + k] = 0.0;
      continue;
    }
    int c1 = a.cellsOnEdge[2 * e], c2 = a.cellsOnEdge[2 * e + 1];
    c1 = min(max(c1, 0), a.nCells), c2 = min(max(c2, 0), a.nCells);  // the garbage cell at most
    const double* nv = a.edgeNormalVectors + 3 * e;
    const double e1 = todyn_dot(nv, a.east + 3 * (int64_t)c1), n1 = todyn_dot(nv, a.north + 3 * (int64_t)c1);
    const double e2 = todyn_dot(nv, a.east + 3 * (int64_t)c2), n2 = todyn_dot(nv, a.north + 3 * (int64_t)c2);
    const int64_t r1 = (int64_t)c1 * K, r2 = (int64_t)c2 * K;
    const bool own = e < a.nEdgesSolve;
    for (int k = lane; k < K; k += a.group) {
      double tu = 0.0, up = 0.0;
      const double re = own ? a.rho_edge[row + k] : 0.0;
      if (a.pbl) {
        const double bl = todyn_project(a.rublten[r1 + k], a.rvblten[r1 + k], a.rublten[r2 + k], a.rvblten[r2 + k], e1,
                                        n1, e2, n2);
        a.rublten_Edge[row + k] = bl;
        up = bl;                                   // :334
        tu = tu + bl * re;                         // :339
      } else {
        up = a.tend_u_phys[row + k];               // assigned only under the PBL branch: it accumulates
      }
      if (a.cu) {
        const double cu = todyn_project(a.rucuten[r1 + k], a.rvcuten[r1 + k], a.rucuten[r2 + k], a.rvcuten[r2 + k], e1,
                                        n1, e2, n2);
        a.rucuten_Edge[row + k] = cu;
        up = up + cu;                              // :393-394
        tu = tu + cu * re;                         // :398
      }
      a.tend_u_phys[row + k] = up;
      a.tend_ru_physics[row + k] = own ? tu : 0.0;
    }
  }
}

struct TodynCells {
  int64_t n, n_solve, plane;  // (nCells + 1) K, nCellsSolve K, the scalars' plane stride = n
  int ns, index_qv;           // 0-based
  // t = t + x mass, in the reference's statement order: the theta terms (rthblten, rthcuten, rthratenlw,
  // rthratensw) and the scalar terms with the plane each adds to
  int nth, nterm;
  const double* th[4];
  const double* term[TODYN_MAX_TERMS];
  int term_plane[TODYN_MAX_TERMS];
  const double *mass, *theta_m, *qv;  // rho_zz, theta_m and scalars(index_qv) of time level 1
  double *tend_rtheta, *tend_rho, *scalars_tend;
};

template <bool V2>
__global__ __launch_bounds__(TODYN_THREADS) void k_todyn_cells(TodynCells a) {
  constexpr int W = V2 ? 2 : 1;
  const int64_t stride = (int64_t)gridDim.x * TODYN_THREADS;
  const int64_t nw = a.n / W;  // V2: n is even
  auto load = [](const double* __restrict__ p, int64_t o, double (&v)[W]) {
    if constexpr (V2) {
      const d2 x = ld2(p + o);
      v[0] = x.x, v[1] = x.y;
    } else {
      v[0] = p[o];
    }
  };
  auto store = [](double* p, int64_t o, const double (&v)[W]) {
    if constexpr (V2) st2(p + o, d2{v[0], v[1]});
    else p[o] = v[0];
  };
  for (int64_t i = (int64_t)blockIdx.x * TODYN_THREADS + threadIdx.x; i < nw; i += stride) {
    const int64_t o = W * i;
    const bool own0 = o < a.n_solve, own1 = V2 && o + 1 < a.n_solve;  // own1 implies own0
    double rt[W] = {}, zero[W] = {}, st_qv[W] = {};
    if (!own0) {
      for (int is = 0; is < a.ns; ++is) store(a.scalars_tend, (int64_t)is * a.plane + o, zero);
    } else {
      double mass[W], x[W];
      load(a.mass, o, mass);
      double th[W] = {};
      for (int j = 0; j < a.nth; ++j) {
        load(a.th[j], o, x);
#pragma unroll
        for (int w = 0; w < W; ++w) th[w] = th[w] + x[w] * mass[w];                  // :345, 372, 410, 419
      }
      for (int is = 0; is < a.ns; ++is) {
        double t[W] = {};
        for (int j = 0; j < a.nterm; ++j) {
          if (a.term_plane[j] != is) continue;
          load(a.term[j], o, x);
#pragma unroll
          for (int w = 0; w < W; ++w) t[w] = t[w] + x[w] * mass[w];                  // :346-348, 358, 373-375, 384-385
        }
        if (V2 && !own1) t[W - 1] = 0.0;
        if (is == a.index_qv) {
#pragma unroll
          for (int w = 0; w < W; ++w) st_qv[w] = t[w];
        }
        store(a.scalars_tend, (int64_t)is * a.plane + o, t);
      }
      double qv[W], tm[W];
      load(a.qv, o, qv);
      load(a.theta_m, o, tm);
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const double coeff = (1. + RVORD * qv[w]);                                   // :428
        const double t = coeff * th[w] + RVORD * tm[w] * st_qv[w] / coeff;           // :429
        rt[w] = (w == 0 || own1) ? 0.0 + t : 0.0;                                    // :181, 430
      }
    }
    store(a.tend_rtheta, o, rt);
    store(a.tend_rho, o, zero);                                                      // :182
  }
}

}  // namespace mpas

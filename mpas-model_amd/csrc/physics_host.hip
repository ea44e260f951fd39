// Host side of the step's physics hooks: the incremental analysis update (kernels: iau.hip), the coupling
// of the physics tendencies (physics_get_tend: todynamics.hip), the
// convective running maxima (convdiag.hip), the device microphysics (kessler.hip), the isobaric output
// diagnostics (isobaric.hip), the PV diagnostics (pv.hip) with their budget (pvbudget.hip) and the output-time
// convective diagnostics (convcompute.hip; the last four are not part of the step, but hooks of the same shape).  Per hook: what
// enqueues its kernels, and its entry points of include/mpas_dycore.h.  A hook's state struct
// (mpas_dyc_ctx::iau / todyn / convdiag / microp / iso / pv / conv, Block::cv / pv) stands next to its kernels' argument struct; its
// fields are a Group of the registry (dycore.hip build_registry), allocated by alloc_group.
//
// Included by dycore.hip inside its namespace, before srk3: after the structs (Field, Block,
// mpas_dyc_ctx), HIPCHK / CHK, find, P, field_bytes, physics_tendencies, drop_graphs, require_device,
// alloc_group, group_ready, timed_on_stream, iso_field_name, compute_bnd, exchange and block_ptrs.  The file closes that namespace for its
// extern "C" entry points and opens it again at its end.

// ---- incremental analysis update ----
// atm_add_tend_anal_incr (mpas_atm_iau.F:81-217) of every block: physics + IAU into scratch.iau_*,
// which P's tend_*_physics point at (make_ptrs), and into tend.scalars_tend in place.  Reads the
// host's tend_physics arrays themselves (nullptr, read as 0.0, when the host supplies none).
int iau_add_tend(mpas_dyc_ctx* ctx, const std::vector<Ptrs>& P) {
  if (ctx->planning) return MPAS_DYC_OK;
  const bool host_phys = coupled_tendencies(ctx);  // the host's, or the device's physics_get_tend's
  for (size_t ib = 0; ib < ctx->blk.size(); ++ib) {
    Block& b = ctx->blk[ib];
    const Dims& d = b.d;
    const Ptrs& p = P[ib];
    const double* u_amb = (const double*)find(b, "tend_iau", "u")->buf[0];
    const int64_t ne = (int64_t)(d.nEdges + 1) * d.K, nc = (int64_t)(d.nCells + 1) * d.K;
    auto grid = [](int64_t n) {
      return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + IAU_THREADS - 1) / IAU_THREADS, IAU_MAX_BLOCKS)));
    };
    hipLaunchKernelGGL(k_iau_edges, grid(ne / 2), dim3(IAU_THREADS), 0, ctx->stream, ne, (int64_t)d.nEdgesSolve * d.K,
                       ctx->iau.wgt, (const double*)p.rho_edge, u_amb,
                       host_phys ? ::P<const double>(ctx, b, "tend_physics", "tend_ru_physics") : nullptr, p.tend_ru_physics);
    IauCells a{};
    a.n = a.plane = nc;
    a.n_solve = (int64_t)d.nCellsSolve * d.K;
    a.ns = d.ns, a.moist_start = d.moist_start, a.moist_end = d.moist_end, a.index_qv = ctx->index_qv;
    a.st_zero = host_phys ? 0 : 1;
    a.wgt = ctx->iau.wgt;
    a.zz = p.zz, a.rho_zz = p.rho_zz1, a.theta_m = p.theta_m1, a.scalars = p.scalars1;
    a.rho_amb = (const double*)find(b, "tend_iau", "rho")->buf[0];
    a.theta_amb = (const double*)find(b, "tend_iau", "theta")->buf[0];
    a.scalars_amb = (const double*)find(b, "tend_iau", "scalars")->buf[0];
    a.phys_rtheta = host_phys ? ::P<const double>(ctx, b, "tend_physics", "tend_rtheta_physics") : nullptr;
    a.phys_rho = host_phys ? ::P<const double>(ctx, b, "tend_physics", "tend_rho_physics") : nullptr;
    a.out_rtheta = p.tend_rtheta_physics, a.out_rho = p.tend_rho_physics, a.scalars_tend = p.scalars_tend;
    if (nc & 1) hipLaunchKernelGGL(k_iau_cells<false>, grid(nc), dim3(IAU_THREADS), 0, ctx->stream, a);
    else hipLaunchKernelGGL(k_iau_cells<true>, grid(nc / 2), dim3(IAU_THREADS), 0, ctx->stream, a);
  }
  return MPAS_DYC_OK;
}

// ---- convective running maxima ----
int convdiag_check_flags(mpas_dyc_ctx* ctx, int32_t flags, const char* entry) {
  if (!(flags & ~(CONVDIAG_W | CONVDIAG_WSP | CONVDIAG_UH))) return MPAS_DYC_OK;
  ctx->err = std::string(entry) + ": unknown flag bits";
  return MPAS_DYC_EINVAL;
}

// The running maxima's derived table of one block: for each owned cell the (vertex, j) pairs with
// cellsOnVertex(j, vertex) = cell, in ascending vertex index and then j -- the order in which the
// reference's scatter over the vertices (convective_diagnostics.F:169-174) adds a cell's terms --
// stored as 3 vertex + j.  Pairs of halo cells and of the garbage cell are dropped.  Rebuilt like
// the other derived tables: setting cellsOnVertex clears cv.ready (and bnd_ready).
int convdiag_table(mpas_dyc_ctx* ctx, Block& b) {
  const Dims& d = b.d;
  if ((int64_t)b.h_cov.size() < 3LL * d.nVertices) {
    ctx->err = "mesh.cellsOnVertex not set";
    return MPAS_DYC_ESTATE;
  }
  if (3LL * ((int64_t)d.nVertices + 1) > INT32_MAX) {
    ctx->err = "too many vertices for the convective diagnostics' table";
    return MPAS_DYC_EINVAL;
  }
  std::vector<int32_t> start((size_t)d.nCellsSolve + 1, 0);
  for (int64_t i = 0; i < 3LL * d.nVertices; ++i)
    if (b.h_cov[i] < d.nCellsSolve) ++start[b.h_cov[i] + 1];
  for (int c = 0; c < d.nCellsSolve; ++c) start[c + 1] += start[c];
  std::vector<int32_t> fill(start.begin(), start.end() - 1), kite((size_t)std::max(1, start[d.nCellsSolve]));
  for (int64_t i = 0; i < 3LL * d.nVertices; ++i)  // ascending (vertex, j)
    if (b.h_cov[i] < d.nCellsSolve) kite[fill[b.h_cov[i]]++] = (int32_t)i;
  HIPCHK(hipStreamSynchronize(ctx->stream));  // a running update still reads the old table
  if (b.cv.start) (void)hipFree(b.cv.start);
  if (b.cv.kite) (void)hipFree(b.cv.kite);
  b.cv.start = b.cv.kite = nullptr;
  HIPCHK(hipMalloc(&b.cv.start, start.size() * 4));
  HIPCHK(hipMalloc(&b.cv.kite, kite.size() * 4));
  HIPCHK(hipMemcpy(b.cv.start, start.data(), start.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b.cv.kite, kite.data(), kite.size() * 4, hipMemcpyHostToDevice));
  b.cv.ready = true;
  return MPAS_DYC_OK;
}

// convective_diagnostics_update with the context's mask on every block: one launch per block
int convdiag_enqueue(mpas_dyc_ctx* ctx) {
  for (auto& b : ctx->blk) {
    const Dims& d = b.d;
    if (d.nCellsSolve <= 0) continue;
    ConvDiag a{};
    a.nCellsSolve = d.nCellsSolve, a.K = d.K, a.flags = ctx->convdiag.flags;
    a.w = P<const double>(ctx, b, "state", "w", 1);
    a.vorticity = P<const double>(ctx, b, "diag", "vorticity");
    a.uzonal = P<const double>(ctx, b, "diag", "uReconstructZonal");
    a.umeridional = P<const double>(ctx, b, "diag", "uReconstructMeridional");
    a.zgrid = P<const double>(ctx, b, "mesh", "zgrid");
    a.areaCell = P<const double>(ctx, b, "mesh", "areaCell");
    a.kiteAreasOnVertex = P<const double>(ctx, b, "mesh", "kiteAreasOnVertex");
    a.cv_start = b.cv.start, a.cv_kite = b.cv.kite;
    a.w_velocity_max = P<double>(ctx, b, "diag", CONVDIAG_FIELDS[0]);
    a.wind_speed_level1_max = P<double>(ctx, b, "diag", CONVDIAG_FIELDS[1]);
    a.updraft_helicity_max = P<double>(ctx, b, "diag", CONVDIAG_FIELDS[2]);
    hipLaunchKernelGGL(k_convdiag, dim3((unsigned)((d.nCellsSolve + CONVDIAG_WAVES - 1) / CONVDIAG_WAVES)),
                       dim3(CONVDIAG_THREADS), 0, ctx->stream, a);
  }
  HIPCHK(hipGetLastError());
  return MPAS_DYC_OK;
}

// ---- device microphysics ----
// k_kessler<KESSLER_CHUNKS> holds a column of at most 64 levels per chunk
int kessler_check_levels(mpas_dyc_ctx* ctx, int K) {
  if (K <= 64 * KESSLER_CHUNKS) return MPAS_DYC_OK;
  ctx->err = "the Kessler kernel of this build holds at most " + std::to_string(64 * KESSLER_CHUNKS) + " levels";
  return MPAS_DYC_EINVAL;
}

// driver_microphysics for mp_kessler on time level tl of every block: one launch per block
int kessler_enqueue(mpas_dyc_ctx* ctx, double dt, int tl) {
  if (ctx->planning) return MPAS_DYC_OK;
  for (auto& b : ctx->blk) {
    const Dims& d = b.d;
    if (d.nCellsSolve <= 0) continue;
    Kessler a{};
    a.nCellsSolve = d.nCellsSolve, a.nCells = d.nCells, a.K = d.K;
    a.iqv = ctx->index_qv, a.iqc = ctx->microp.iqc, a.iqr = ctx->microp.iqr;
    a.dt = dt, a.bucket = ctx->microp.bucket;
    a.zz = P<const double>(ctx, b, "mesh", "zz");
    a.zgrid = P<const double>(ctx, b, "mesh", "zgrid");
    a.rho_zz = P<const double>(ctx, b, "state", "rho_zz", tl);
    a.rtheta_base = P<const double>(ctx, b, "diag", "rtheta_base");
    a.exner_base = P<const double>(ctx, b, "diag", "exner_base");
    a.pressure_base = P<const double>(ctx, b, "diag", "pressure_base");
    a.theta_m = P<double>(ctx, b, "state", "theta_m", tl);
    a.scalars = P<double>(ctx, b, "state", "scalars", tl);
    a.exner = P<double>(ctx, b, "diag", "exner");
    a.rtheta_p = P<double>(ctx, b, "diag", "rtheta_p");
    a.pressure_p = P<double>(ctx, b, "diag", "pressure_p");
    a.rt_diabatic_tend = P<double>(ctx, b, "tend", "rt_diabatic_tend");
    a.rainnc = P<double>(ctx, b, "diag_physics", "rainnc");
    a.rainncv = P<double>(ctx, b, "diag_physics", "rainncv");
    a.precipw = P<double>(ctx, b, "diag_physics", "precipw");
    a.i_rainnc = P<int>(ctx, b, "diag_physics", "i_rainnc");
    a.surface_pressure = P<double>(ctx, b, "diag", "surface_pressure");
    a.tend_sfc_pressure = P<double>(ctx, b, "tend", "tend_sfc_pressure");
    CHK(kessler_check_levels(ctx, d.K));
    hipLaunchKernelGGL(k_kessler<KESSLER_CHUNKS>, dim3((unsigned)((d.nCellsSolve + KESSLER_WAVES - 1) / KESSLER_WAVES)),
                       dim3(KESSLER_THREADS), 0, ctx->stream, a);
  }
  return MPAS_DYC_OK;
}

// ---- isobaric diagnostics ----
// interp_diagnostics with the context's mask on time level tl of every block: the failure word's reset,
// the cell kernel and mslp's failure pass, then the vertex kernel
int iso_enqueue(mpas_dyc_ctx* ctx, int tl) {
  const int flags = ctx->iso.flags;
  for (auto& b : ctx->blk) {
    const Dims& d = b.d;
    const int K = d.K;
    if ((flags & ~ISO_VORTICITY) && d.nCellsSolve > 0) {
      IsoCells a{};
      a.nCellsSolve = d.nCellsSolve, a.K = K, a.flags = flags;
      a.pressure_p = P<const double>(ctx, b, "diag", "pressure_p");
      a.pressure_base = P<const double>(ctx, b, "diag", "pressure_base");
      a.theta_m = P<const double>(ctx, b, "state", "theta_m", tl);
      a.qv = P<const double>(ctx, b, "state", "scalars", tl) + (int64_t)ctx->index_qv * (d.nCells + 1) * K;
      a.exner = P<const double>(ctx, b, "diag", "exner");
      a.relhum = P<const double>(ctx, b, "diag", "relhum");
      a.uzonal = P<const double>(ctx, b, "diag", "uReconstructZonal");
      a.umeridional = P<const double>(ctx, b, "diag", "uReconstructMeridional");
      a.zgrid = P<const double>(ctx, b, "mesh", "zgrid");
      a.w = P<const double>(ctx, b, "state", "w", tl);
      for (int l = 0; l < ISO_NP; ++l) a.hpa[l] = (double)ISO_HPA[l];
      for (int l = 0; l < ISO_NT; ++l) a.t_lev[l] = 30000.0 + 5000.0 * l;  // :479-501
      for (int l = 0; l < ISO_NZ; ++l) a.z_lev[l] = 30000.0 + 5000.0 * l;
      for (int g = 0; g < ISO_NGROUPS - 1; ++g)
        for (int l = 0; l < ISO_NP; ++l) a.out[g][l] = P<double>(ctx, b, "diag", iso_field_name(g, l).c_str());
      a.mslp = P<double>(ctx, b, "diag", "mslp");
      a.t_isobaric = P<double>(ctx, b, "diag", "t_isobaric");
      a.z_isobaric = P<double>(ctx, b, "diag", "z_isobaric");
      a.meanT_500_300 = P<double>(ctx, b, "diag", "meanT_500_300");
      if (flags & ISO_MSLP) {
        if (!b.iso_fail) HIPCHK(hipMalloc(&b.iso_fail, 256));
        HIPCHK(hipMemsetAsync(b.iso_fail, 0, 4, ctx->stream));
      }
      a.fail = b.iso_fail;
      hipLaunchKernelGGL(k_iso_cells, dim3((unsigned)((d.nCellsSolve + ISO_WAVES - 1) / ISO_WAVES)), dim3(ISO_THREADS), 0,
                         ctx->stream, a);
      if (flags & ISO_MSLP)
        hipLaunchKernelGGL(k_iso_mslp_fail, dim3((unsigned)((d.nCellsSolve + 255) / 256)), dim3(256), 0, ctx->stream,
                           d.nCellsSolve, (const int*)b.iso_fail, a.mslp);
    }
    if ((flags & ISO_VORTICITY) && d.nVerticesSolve > 0) {
      IsoVerts a{};
      a.nVerticesSolve = d.nVerticesSolve, a.K = K;
      a.pressure_p = P<const double>(ctx, b, "diag", "pressure_p");
      a.pressure_base = P<const double>(ctx, b, "diag", "pressure_base");
      a.vorticity = P<const double>(ctx, b, "diag", "vorticity");
      a.kiteAreasOnVertex = P<const double>(ctx, b, "mesh", "kiteAreasOnVertex");
      a.areaTriangle = P<const double>(ctx, b, "mesh", "areaTriangle");
      a.cellsOnVertex = P<const int>(ctx, b, "mesh", "cellsOnVertex");
      for (int l = 0; l < ISO_NP; ++l) {
        a.hpa[l] = (double)ISO_HPA[l];
        a.out[l] = P<double>(ctx, b, "diag", iso_field_name(ISO_NGROUPS - 1, l).c_str());
      }
      hipLaunchKernelGGL(k_iso_vertices, dim3((unsigned)((d.nVerticesSolve + ISO_WAVES - 1) / ISO_WAVES)), dim3(ISO_THREADS), 0,
                         ctx->stream, a);
    }
  }
  HIPCHK(hipGetLastError());
  return MPAS_DYC_OK;
}

// ---- Ertel PV and dynamic-tropopause diagnostics ----
// a needed mesh input of block b that was never set, or nullptr
const char* pv_missing_input(Block& b) {
  if (!(b.pv.set & PV_SET_TANGENT)) return "mesh.cellTangentPlane";
  if (!(b.pv.set & PV_SET_VERTICAL)) return "mesh.localVerticalUnitVectors";
  if (!(b.pv.set & PV_SET_NORMALS)) return "mesh.edgeNormalVectors";
  if (!find(b, "mesh", "areaCell")->buf[0]) return "mesh.areaCell";
  if (!b.kite_set) return "mesh.kiteAreasOnVertex";
  if ((int64_t)b.h_cov.size() < 3LL * b.d.nVertices) return "mesh.cellsOnVertex";
  return nullptr;
}

// The block's derived table (k_pv_geom) and its fill buffers, for the mesh arrays and strides as they are
int pv_prepare(mpas_dyc_ctx* ctx, Block& b) {
  const Dims& d = b.d;
  const int64_t geom_n = (int64_t)std::max(1, d.nCellsSolve) * (PV_HDR + 3 * d.maxEdges);
  const int64_t words_n = (int64_t)((d.K + 63) / 64) * (d.nCells + 1);
  if (b.pv.geom_n != geom_n || b.pv.words_n != words_n) {
    HIPCHK(hipStreamSynchronize(ctx->stream));  // a running call still reads the old buffers
    for (void** q : {(void**)&b.pv.geom, (void**)&b.pv.cand, (void**)&b.pv.mem[0], (void**)&b.pv.mem[1]}) {
      if (*q) (void)hipFree(*q);
      *q = nullptr;
    }
    b.pv.geom_n = b.pv.words_n = 0;
    HIPCHK(hipMalloc(&b.pv.geom, geom_n * 8));
    HIPCHK(hipMalloc(&b.pv.cand, words_n * 8));
    HIPCHK(hipMalloc(&b.pv.mem[0], words_n * 8));
    HIPCHK(hipMalloc(&b.pv.mem[1], words_n * 8));
    b.pv.geom_n = geom_n, b.pv.words_n = words_n;
    b.pv.ready = false;
  }
  if (!b.pv.flags) HIPCHK(hipMalloc(&b.pv.flags, PV_BATCH * sizeof(int)));
  if (b.pv.ready) return MPAS_DYC_OK;
  // the garbage slot's words stay 0: no kernel writes them
  for (unsigned long long* q : {b.pv.cand, b.pv.mem[0], b.pv.mem[1]}) HIPCHK(hipMemsetAsync(q, 0, words_n * 8, ctx->stream));
  if (d.nCellsSolve > 0) {
    PvGeomArgs a{};
    a.nCellsSolve = d.nCellsSolve, a.ME = d.maxEdges;
    a.nEdgesOnCell = P<const int>(ctx, b, "mesh", "nEdgesOnCell");
    a.edgesOnCell = P<const int>(ctx, b, "mesh", "edgesOnCell");
    a.verticesOnCell = P<const int>(ctx, b, "mesh", "verticesOnCell");
    a.cellsOnEdge = P<const int>(ctx, b, "mesh", "cellsOnEdge");
    a.cellsOnVertex = P<const int>(ctx, b, "mesh", "cellsOnVertex");
    a.cellTangentPlane = P<const double>(ctx, b, "mesh", "cellTangentPlane");
    a.localVerticalUnitVectors = P<const double>(ctx, b, "mesh", "localVerticalUnitVectors");
    a.edgeNormalVectors = P<const double>(ctx, b, "mesh", "edgeNormalVectors");
    a.dvEdge = P<const double>(ctx, b, "mesh", "dvEdge");
    a.areaCell = P<const double>(ctx, b, "mesh", "areaCell");
    a.kiteAreasOnVertex = P<const double>(ctx, b, "mesh", "kiteAreasOnVertex");
    a.geom = b.pv.geom;
    hipLaunchKernelGGL(k_pv_geom, dim3((unsigned)((d.nCellsSolve + 255) / 256)), dim3(256), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
  }
  b.pv.ready = true;
  return MPAS_DYC_OK;
}

// floodFill_tropo of one block: the candidates and seeds, then sweeps in batches of PV_BATCH until one
// changes nothing (the host reads the batch's flags back: synchronous), at most nCells + 1 of them.
// Returns in `members` the buffer that holds the fixed point.
int pv_fill(mpas_dyc_ctx* ctx, Block& b, const unsigned long long** members, int* sweeps) {
  const Dims& d = b.d;
  const int words = (d.K + 63) / 64;
  hipLaunchKernelGGL(k_pv_cand, dim3((unsigned)((d.nCells + PV_WAVES - 1) / PV_WAVES)), dim3(PV_THREADS), 0, ctx->stream,
                     d.nCells, d.K, words, P<const double>(ctx, b, "mesh", "latCell"),
                     P<const double>(ctx, b, "diag", "ertel_pv"), b.pv.cand, b.pv.mem[0]);
  int src = 0;
  *sweeps = 0;
  for (int64_t done = 0; done <= d.nCells;) {
    HIPCHK(hipMemsetAsync(b.pv.flags, 0, PV_BATCH * sizeof(int), ctx->stream));
    const int n = (int)std::min<int64_t>(PV_BATCH, (int64_t)d.nCells + 1 - done);
    for (int i = 0; i < n; ++i, src ^= 1)
      hipLaunchKernelGGL(k_pv_sweep, dim3((unsigned)((d.nCells + 255) / 256)), dim3(256), 0, ctx->stream, d.nCells, words,
                         d.maxEdges, P<const int>(ctx, b, "mesh", "nEdgesOnCell"), P<const int>(ctx, b, "mesh", "cellsOnCell"),
                         (const unsigned long long*)b.pv.cand, (const unsigned long long*)b.pv.mem[src], b.pv.mem[src ^ 1],
                         b.pv.flags + i);
    HIPCHK(hipGetLastError());
    int h[PV_BATCH] = {};
    HIPCHK(hipMemcpyAsync(h, b.pv.flags, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    done += n;
    bool fixed = false;
    for (int i = 0; i < n && !fixed; ++i) {
      if (h[i]) ++*sweeps;
      else fixed = true;  // the later sweeps of the batch copied the fixed point
    }
    if (fixed) break;
  }
  *members = b.pv.mem[src];
  return MPAS_DYC_OK;
}

// atm_compute_pv_diagnostics on time level tl of every block (pv.hip), `lists`: with its halo exchanges
int pv_run(mpas_dyc_ctx* ctx, int tl, bool lists) {
  const int layers = 7;
  for (auto& b : ctx->blk) {
    const Dims& d = b.d;
    const int64_t n = (int64_t)d.nCells * d.K;
    if (n <= 0) continue;
    hipLaunchKernelGGL(k_pv_theta_rho, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65536)), dim3(256), 0, ctx->stream, n,
                       P<const double>(ctx, b, "state", "theta_m", tl),
                       P<const double>(ctx, b, "state", "scalars", tl) + (int64_t)ctx->index_qv * (d.nCells + 1) * d.K,
                       P<const double>(ctx, b, "state", "rho_zz", tl), P<const double>(ctx, b, "mesh", "zz"),
                       P<double>(ctx, b, "diag", "theta"), P<double>(ctx, b, "diag", "rho"));
  }
  HIPCHK(hipGetLastError());
  if (lists) {  // :1270-1274
    for (const char* n : {"theta", "uReconstructX", "uReconstructY", "uReconstructZ"})
      CHK(mpas_dyc_halo_exchange(ctx, "diag", n, 1, layers));
    CHK(mpas_dyc_halo_exchange(ctx, "state", "w", tl, layers));
  }
  for (auto& b : ctx->blk) {
    const Dims& d = b.d;
    if (d.nCellsSolve <= 0) continue;
    PvEpv a{};
    a.nCellsSolve = d.nCellsSolve, a.K = d.K, a.ME = d.maxEdges;
    a.nEdgesOnCell = P<const int>(ctx, b, "mesh", "nEdgesOnCell");
    a.cellsOnCell = P<const int>(ctx, b, "mesh", "cellsOnCell");
    a.verticesOnCell = P<const int>(ctx, b, "mesh", "verticesOnCell");
    a.geom = b.pv.geom;
    a.zgrid = P<const double>(ctx, b, "mesh", "zgrid");
    a.w = P<const double>(ctx, b, "state", "w", tl);
    a.theta = P<const double>(ctx, b, "diag", "theta");
    a.rho = P<const double>(ctx, b, "diag", "rho");
    a.vorticity = P<const double>(ctx, b, "diag", "vorticity");
    a.ux = P<const double>(ctx, b, "diag", "uReconstructX");
    a.uy = P<const double>(ctx, b, "diag", "uReconstructY");
    a.uz = P<const double>(ctx, b, "diag", "uReconstructZ");
    a.ertel_pv = P<double>(ctx, b, "diag", "ertel_pv");
    hipLaunchKernelGGL(k_pv_epv, dim3((unsigned)((d.nCellsSolve + PV_WAVES - 1) / PV_WAVES)), dim3(PV_THREADS), 0, ctx->stream,
                       a);
  }
  HIPCHK(hipGetLastError());
  if (lists) CHK(mpas_dyc_halo_exchange(ctx, "diag", "ertel_pv", 1, layers));  // :1279-1280
  ctx->pv.sweeps = 0;
  for (auto& b : ctx->blk) {
    const Dims& d = b.d;
    if (d.nCells <= 0) continue;
    const unsigned long long* members = nullptr;
    int sweeps = 0;
    CHK(pv_fill(ctx, b, &members, &sweeps));
    ctx->pv.sweeps = std::max(ctx->pv.sweeps, sweeps);
    PvInterp a{};
    a.nCells = d.nCells, a.nCellsSolve = d.nCellsSolve, a.K = d.K, a.ME = d.maxEdges, a.words = (d.K + 63) / 64;
    a.nEdgesOnCell = P<const int>(ctx, b, "mesh", "nEdgesOnCell");
    a.verticesOnCell = P<const int>(ctx, b, "mesh", "verticesOnCell");
    a.mem = members;
    a.geom = b.pv.geom;
    a.latCell = P<const double>(ctx, b, "mesh", "latCell");
    a.ertel_pv = P<const double>(ctx, b, "diag", "ertel_pv");
    a.uzonal = P<const double>(ctx, b, "diag", "uReconstructZonal");
    a.umeridional = P<const double>(ctx, b, "diag", "uReconstructMeridional");
    a.theta = P<const double>(ctx, b, "diag", "theta");
    a.vorticity = P<const double>(ctx, b, "diag", "vorticity");
    a.iLev_DT = P<int>(ctx, b, "diag", "iLev_DT");
    a.u_pv = P<double>(ctx, b, "diag", "u_pv");
    a.v_pv = P<double>(ctx, b, "diag", "v_pv");
    a.theta_pv = P<double>(ctx, b, "diag", "theta_pv");
    a.vort_pv = P<double>(ctx, b, "diag", "vort_pv");
    hipLaunchKernelGGL(k_pv_interp, dim3((unsigned)((d.nCells + 255) / 256)), dim3(256), 0, ctx->stream, a);
  }
  HIPCHK(hipGetLastError());
  return MPAS_DYC_OK;
}

// What mpas_dyc_pv_diagnostics and mpas_dyc_pv_budget_diagnostics do before they enqueue: the group, the mesh
// inputs of every block, the packed strides and the derived table.  `lists`: a block has exchange lists
int pv_check_prepare(mpas_dyc_ctx* ctx, const char* entry, bool* lists) {
  if (!group_ready(ctx, G_PV)) CHK(alloc_group(ctx, G_PV));
  *lists = false;
  for (auto& b : ctx->blk) {
    if (const char* missing = pv_missing_input(b)) {
      ctx->err = std::string(entry) + ": " + missing + " not set";
      return MPAS_DYC_ESTATE;
    }
    *lists = *lists || !b.xl.empty();
  }
  if (!ctx->bnd_ready) CHK(compute_bnd(ctx));  // the packed strides the table is indexed with
  for (auto& b : ctx->blk) CHK(pv_prepare(ctx, b));
  return MPAS_DYC_OK;
}

// ---- Ertel PV budget ----
// an input of block b that the budget with mask `flags` needs and that was never set or allocated, or nullptr
const char* pvb_missing_input(Block& b, int flags) {
  if (!b.rec_set) return "mesh.coeffs_reconstruct";
  if (!find(b, "mesh", "areaTriangle")->buf[0]) return "mesh.areaTriangle";
  for (const auto& r : PVB_RAW)
    if ((flags & r.bit) && !find(b, "tend_physics", r.name)->buf[0]) return r.name;
  return nullptr;
}

// atm_compute_pvBudget_diagnostics on time level tl of every block (pvbudget.hip) after pv_run of the same
// level, `lists`: with its halo exchanges (:1592-1605; dtheta_dt_mix's after the kernel that forms it)
int pvb_run(mpas_dyc_ctx* ctx, int tl, bool lists) {
  const int fl = ctx->pvb.flags, layers = 7;
  const bool phys = find(ctx->blk[0], "diag", "tend_u_phys")->buf[0] != nullptr;  // a group: the same on every block
  if (lists) {
    for (const auto& r : PVB_RAW)
      if (fl & r.bit) CHK(mpas_dyc_halo_exchange(ctx, "tend_physics", r.name, 1, layers));
    CHK(mpas_dyc_halo_exchange(ctx, "diag", "dtheta_dt_mp", 1, layers));
    if (phys) CHK(mpas_dyc_halo_exchange(ctx, "diag", "tend_u_phys", 1, layers));
    CHK(mpas_dyc_halo_exchange(ctx, "tend", "u_euler", 1, layers));
    CHK(mpas_dyc_halo_exchange(ctx, "tend", "w_euler", 1, layers));
  }
  auto grid = [](int64_t n) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 65536))); };
  for (auto& b : ctx->blk) {
    const Dims& d = b.d;
    if (d.nCells <= 0) continue;
    hipLaunchKernelGGL(k_pvb_cells, grid((int64_t)d.nCells * (d.K + 1)), dim3(256), 0, ctx->stream, (int64_t)d.nCells, d.K,
                       P<const double>(ctx, b, "tend", "theta_euler"),
                       P<const double>(ctx, b, "state", "scalars", tl) + (int64_t)ctx->index_qv * (d.nCells + 1) * d.K,
                       P<const double>(ctx, b, "diag", "rho"), P<const double>(ctx, b, "tend", "w_euler"),
                       P<double>(ctx, b, "diag", "dtheta_dt_mix"), P<double>(ctx, b, "scratch", "pvb_tend_w"));
  }
  HIPCHK(hipGetLastError());
  if (lists) CHK(mpas_dyc_halo_exchange(ctx, "diag", "dtheta_dt_mix", 1, layers));
  const std::vector<Ptrs> ptrs = block_ptrs(ctx);
  for (size_t ib = 0; ib < ctx->blk.size(); ++ib) {
    Block& b = ctx->blk[ib];
    const Dims& d = b.d;
    double* tend_u = P<double>(ctx, b, "scratch", "pvb_tend_u");
    if (d.nEdges > 0)
      hipLaunchKernelGGL(k_pvb_edges, grid((int64_t)d.nEdges * d.K), dim3(256), 0, ctx->stream, (int64_t)d.nEdges * d.K,
                         phys ? P<const double>(ctx, b, "diag", "tend_u_phys") : nullptr,
                         P<const double>(ctx, b, "tend", "u_euler"), P<const double>(ctx, b, "diag", "rho_edge"), tend_u);
    if (d.nVertices > 0) {
      PvbCurl a{};
      a.nVertices = d.nVertices, a.nEdges = d.nEdges, a.K = d.K;
      a.edgesOnVertex = P<const int>(ctx, b, "mesh", "edgesOnVertex");
      a.verticesOnEdge = P<const int>(ctx, b, "mesh", "verticesOnEdge");
      a.dcEdge = P<const double>(ctx, b, "mesh", "dcEdge");
      a.areaTriangle = P<const double>(ctx, b, "mesh", "areaTriangle");
      a.u = tend_u;
      a.curl = P<double>(ctx, b, "scratch", "pvb_curl");
      hipLaunchKernelGGL(k_pvb_curl, dim3((unsigned)((d.nVertices + PV_WAVES - 1) / PV_WAVES)), dim3(PV_THREADS), 0,
                         ctx->stream, a);
    }
    if (d.nCellsSolve <= 0) continue;
    reconstruct_to(ctx, d, ptrs[ib], tend_u, P<double>(ctx, b, "scratch", "pvb_tenduX"),
                   P<double>(ctx, b, "scratch", "pvb_tenduY"), P<double>(ctx, b, "scratch", "pvb_tenduZ"),
                   P<double>(ctx, b, "scratch", "pvb_tenduZonal"), P<double>(ctx, b, "scratch", "pvb_tenduMerid"));
    PvBudget a{};
    a.nCellsSolve = d.nCellsSolve, a.K = d.K, a.ME = d.maxEdges;
    a.nEdgesOnCell = P<const int>(ctx, b, "mesh", "nEdgesOnCell");
    a.cellsOnCell = P<const int>(ctx, b, "mesh", "cellsOnCell");
    a.verticesOnCell = P<const int>(ctx, b, "mesh", "verticesOnCell");
    a.geom = b.pv.geom;
    a.zgrid = P<const double>(ctx, b, "mesh", "zgrid");
    a.w = P<const double>(ctx, b, "state", "w", tl);
    a.theta = P<const double>(ctx, b, "diag", "theta");
    a.rho = P<const double>(ctx, b, "diag", "rho");
    a.vorticity = P<const double>(ctx, b, "diag", "vorticity");
    a.ux = P<const double>(ctx, b, "diag", "uReconstructX");
    a.uy = P<const double>(ctx, b, "diag", "uReconstructY");
    a.uz = P<const double>(ctx, b, "diag", "uReconstructZ");
    for (int j = 0; j < 4; ++j) a.src[j] = (fl & PVB_RAW[j].bit) ? P<const double>(ctx, b, "tend_physics", PVB_RAW[j].name) : nullptr;
    a.src[4] = P<const double>(ctx, b, "diag", "dtheta_dt_mp");
    a.src[5] = P<const double>(ctx, b, "diag", "dtheta_dt_mix");  // guarded by dtheta_dt_mp's association (:1460)
    a.tend_w = P<const double>(ctx, b, "scratch", "pvb_tend_w");
    a.curl = P<const double>(ctx, b, "scratch", "pvb_curl");
    a.tx = P<const double>(ctx, b, "scratch", "pvb_tenduX");
    a.ty = P<const double>(ctx, b, "scratch", "pvb_tenduY");
    a.tz = P<const double>(ctx, b, "scratch", "pvb_tenduZ");
    for (int j = 0; j < PVB_NSRC; ++j) a.out[j] = P<double>(ctx, b, "diag", PVB_CELL_FIELDS[j]);
    a.diab = P<double>(ctx, b, "diag", "depv_dt_diab");
    a.fric = P<double>(ctx, b, "diag", "depv_dt_fric");
    hipLaunchKernelGGL(k_pvb_budget, dim3((unsigned)((d.nCellsSolve + PV_WAVES - 1) / PV_WAVES)), dim3(PV_THREADS), 0,
                       ctx->stream, a);
    PvbInterp q{};
    q.nCellsSolve = d.nCellsSolve, q.K = d.K;
    q.iLev_DT = P<const int>(ctx, b, "diag", "iLev_DT");
    q.latCell = P<const double>(ctx, b, "mesh", "latCell");
    q.ertel_pv = P<const double>(ctx, b, "diag", "ertel_pv");
    q.diab = a.diab, q.fric = a.fric;
    q.diab_pv = P<double>(ctx, b, "diag", "depv_dt_diab_pv");
    q.fric_pv = P<double>(ctx, b, "diag", "depv_dt_fric_pv");
    hipLaunchKernelGGL(k_pvb_interp, dim3((unsigned)((d.nCellsSolve + 255) / 256)), dim3(256), 0, ctx->stream, q);
  }
  HIPCHK(hipGetLastError());
  return MPAS_DYC_OK;
}

// ---- cape, cin, storm-relative helicity and the surface / 1 km / 6 km fields ----
// convective_diagnostics_compute with the context's mask on time level tl of every block: the shear and
// helicity kernel, then the parcel ascent if cape or cin is asked for
int conv_enqueue(mpas_dyc_ctx* ctx, int tl) {
  const int flags = ctx->conv.flags;
  for (auto& b : ctx->blk) {
    const Dims& d = b.d;
    if (d.nCellsSolve <= 0) continue;
    ConvCompute a{};
    a.nCellsSolve = d.nCellsSolve, a.K = d.K, a.flags = flags;
    a.theta_m = P<const double>(ctx, b, "state", "theta_m", tl);
    a.qv = P<const double>(ctx, b, "state", "scalars", tl) + (int64_t)ctx->index_qv * (d.nCells + 1) * d.K;
    a.exner = P<const double>(ctx, b, "diag", "exner");
    a.pressure_p = P<const double>(ctx, b, "diag", "pressure_p");
    a.pressure_base = P<const double>(ctx, b, "diag", "pressure_base");
    a.uzonal = P<const double>(ctx, b, "diag", "uReconstructZonal");
    a.umeridional = P<const double>(ctx, b, "diag", "uReconstructMeridional");
    a.zgrid = P<const double>(ctx, b, "mesh", "zgrid");
    for (int i = 0; i < CONV_NFIELDS; ++i) a.out[i] = P<double>(ctx, b, "diag", CONV_FIELDS[i]);
    hipLaunchKernelGGL(k_conv_shear, dim3((unsigned)((d.nCellsSolve + CONV_WAVES - 1) / CONV_WAVES)), dim3(CONV_THREADS), 0,
                       ctx->stream, a);
    if (flags & (CONV_CAPE | CONV_CIN))
      hipLaunchKernelGGL(k_conv_cape, dim3((unsigned)((d.nCellsSolve + CONV_CAPE_THREADS - 1) / CONV_CAPE_THREADS)),
                         dim3(CONV_CAPE_THREADS), 0, ctx->stream, a);
  }
  HIPCHK(hipGetLastError());
  return MPAS_DYC_OK;
}

// ---- physics_get_tend ----
// the wind tendencies are projected to the edges: the PBL's, a Tiedtke scheme's
bool todyn_winds(int flags) { return (flags & (TODYN_PBL | TODYN_CU_WINDS)) != 0; }

// a needed mesh input of block b that was never set, or nullptr
const char* todyn_missing_input(const mpas_dyc_ctx* ctx, const Block& b) {
  if (!todyn_winds(ctx->todyn.flags)) return nullptr;
  if (!(b.todyn_set & TODYN_SET_EAST)) return "mesh.east";
  if (!(b.todyn_set & TODYN_SET_NORTH)) return "mesh.north";
  if (!(b.pv.set & PV_SET_NORMALS)) return "mesh.edgeNormalVectors";
  return nullptr;
}
int todyn_check_inputs(mpas_dyc_ctx* ctx, const char* entry) {
  for (const auto& b : ctx->blk)
    if (const char* missing = todyn_missing_input(ctx, b)) {
      ctx->err = std::string(entry) + ": physics_get_tend needs " + missing + ", which was never set";
      return MPAS_DYC_ESTATE;
    }
  return MPAS_DYC_OK;
}

// physics_get_tend of every block from the fields of time level 1 that P names (rho_zz of time level 2 has
// the same bits after atm_rk_integration_setup, :369): the halo of the raw wind tendencies (:474-492, only
// when a wind flag is on), then the edge and the cell kernel.  The results go to tend_physics.tend_*_physics
// and tend.scalars_tend themselves, whatever P's tend_*_physics point at (the IAU sums read them).
int todyn_step(mpas_dyc_ctx* ctx, const std::vector<Ptrs>& P) {
  const TodynState& t = ctx->todyn;
  const int fl = t.flags;
  if (todyn_winds(fl)) {
    std::vector<XField> fs;
    if (fl & TODYN_PBL) fs.insert(fs.end(), {{"tend_physics", "rublten", 0, ALL_LAYERS}, {"tend_physics", "rvblten", 0, ALL_LAYERS}});
    if (fl & TODYN_CU_WINDS) fs.insert(fs.end(), {{"tend_physics", "rucuten", 0, ALL_LAYERS}, {"tend_physics", "rvcuten", 0, ALL_LAYERS}});
    CHK((exchange)(ctx, fs));
  }
  if (ctx->planning) return MPAS_DYC_OK;
  for (size_t ib = 0; ib < ctx->blk.size(); ++ib) {
    Block& b = ctx->blk[ib];
    const Dims& d = b.d;
    const Ptrs& p = P[ib];
    auto raw = [&](const char* n) { return ::P<const double>(ctx, b, "tend_physics", n); };
    TodynEdges e{};
    e.nEdges = d.nEdges, e.nEdgesSolve = d.nEdgesSolve, e.nCells = d.nCells, e.K = d.K;
    e.group = d.K > 32 ? 64 : d.K > 16 ? 32 : 16;
    e.pbl = (fl & TODYN_PBL) != 0, e.cu = (fl & TODYN_CU_WINDS) != 0;
    e.cellsOnEdge = p.cellsOnEdge;
    e.east = ::P<const double>(ctx, b, "mesh", "east"), e.north = ::P<const double>(ctx, b, "mesh", "north");
    e.edgeNormalVectors = ::P<const double>(ctx, b, "mesh", "edgeNormalVectors");
    e.rublten = raw("rublten"), e.rvblten = raw("rvblten"), e.rucuten = raw("rucuten"), e.rvcuten = raw("rvcuten");
    e.rho_edge = p.rho_edge;
    e.rublten_Edge = ::P<double>(ctx, b, "tend_physics", "rublten_Edge");
    e.rucuten_Edge = ::P<double>(ctx, b, "tend_physics", "rucuten_Edge");
    e.tend_u_phys = ::P<double>(ctx, b, "diag", "tend_u_phys");
    e.tend_ru_physics = ::P<double>(ctx, b, "tend_physics", "tend_ru_physics");
    const int64_t per_block = TODYN_THREADS / e.group;
    auto grid = [](int64_t n) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(n, TODYN_MAX_BLOCKS))); };
    hipLaunchKernelGGL(k_todyn_edges, grid(((int64_t)d.nEdges + 1 + per_block - 1) / per_block), dim3(TODYN_THREADS), 0,
                       ctx->stream, e);

    TodynCells a{};
    a.n = a.plane = (int64_t)(d.nCells + 1) * d.K;
    a.n_solve = (int64_t)d.nCellsSolve * d.K;
    a.ns = d.ns, a.index_qv = ctx->index_qv;
    auto th = [&](const char* n) { a.th[a.nth++] = raw(n); };
    auto term = [&](const char* n, int plane) {  // an absent scalar's term is skipped
      if (plane < 0) return;
      a.term[a.nterm] = raw(n);
      a.term_plane[a.nterm++] = plane;
    };
    if (fl & TODYN_PBL) {                          // :343-364
      th("rthblten");
      term("rqvblten", ctx->index_qv), term("rqcblten", t.iqc), term("rqiblten", t.iqi);
      if (fl & TODYN_PBL_MYNN) term("rniblten", t.ini);
    }
    if (fl & TODYN_CU) {                           // :368-387
      th("rthcuten");
      term("rqvcuten", ctx->index_qv), term("rqccuten", t.iqc), term("rqicuten", t.iqi);
      if (fl & TODYN_CU_KF) term("rqrcuten", t.iqr), term("rqscuten", t.iqs);
    }
    if (fl & TODYN_LW) th("rthratenlw");           // :407-413
    if (fl & TODYN_SW) th("rthratensw");           // :416-422
    a.mass = p.rho_zz1, a.theta_m = p.theta_m1;
    a.qv = p.scalars1 + (int64_t)ctx->index_qv * a.plane;
    a.tend_rtheta = ::P<double>(ctx, b, "tend_physics", "tend_rtheta_physics");
    a.tend_rho = ::P<double>(ctx, b, "tend_physics", "tend_rho_physics");
    a.scalars_tend = ::P<double>(ctx, b, "tend", "scalars_tend");
    auto cgrid = [](int64_t n) {
      return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + TODYN_THREADS - 1) / TODYN_THREADS, TODYN_MAX_BLOCKS)));
    };
    if (a.n & 1) hipLaunchKernelGGL(k_todyn_cells<false>, cgrid(a.n), dim3(TODYN_THREADS), 0, ctx->stream, a);
    else hipLaunchKernelGGL(k_todyn_cells<true>, cgrid(a.n / 2), dim3(TODYN_THREADS), 0, ctx->stream, a);
  }
  return MPAS_DYC_OK;
}

}  // namespace

extern "C" {

int mpas_dyc_set_todynamics(mpas_dyc_ctx* ctx, int32_t flags, int32_t index_qc, int32_t index_qr, int32_t index_qi,
                            int32_t index_qs, int32_t index_ni) {
  if (!ctx) return MPAS_DYC_EINVAL;
  const char* bad = nullptr;
  if (flags & ~TODYN_ALL) bad = "unknown flag bits";
  else if ((flags & TODYN_PBL_MYNN) && !(flags & TODYN_PBL)) bad = "MPAS_DYC_TODYN_PBL_MYNN without MPAS_DYC_TODYN_PBL";
  else if ((flags & (TODYN_CU_KF | TODYN_CU_WINDS)) && !(flags & TODYN_CU))
    bad = "MPAS_DYC_TODYN_CU_KF / _CU_WINDS without MPAS_DYC_TODYN_CU";
  else if ((flags & TODYN_CU_KF) && (flags & TODYN_CU_WINDS)) bad = "MPAS_DYC_TODYN_CU_KF together with MPAS_DYC_TODYN_CU_WINDS";
  const int ns = ctx->blk.empty() ? 0 : ctx->blk[0].d.ns;
  if (!bad && flags)
    for (int32_t i : {index_qc, index_qr, index_qi, index_qs, index_ni})
      if (i > ns || (i > 0 && i - 1 == ctx->index_qv)) bad = "an index is above num_scalars or equal to index_qv";
  if (bad) {
    ctx->err = std::string("mpas_dyc_set_todynamics: ") + bad;
    return MPAS_DYC_EINVAL;
  }
  if (flags && (ctx->physics & MPAS_DYC_PHYSICS_TENDENCIES)) {
    ctx->err = "mpas_dyc_set_todynamics with MPAS_DYC_PHYSICS_TENDENCIES (the host's coupled tendencies) set";
    return MPAS_DYC_ESTATE;
  }
  if (!ctx->host_only) {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (flags && !group_ready(ctx, G_TODYN)) CHK(alloc_group(ctx, G_TODYN));
  }
  const bool replan = (flags & (TODYN_PBL | TODYN_CU_WINDS)) != (ctx->todyn.flags & (TODYN_PBL | TODYN_CU_WINDS));
  if (!flags && ctx->todyn.flags && !ctx->host_only)
    // off: the coupled arrays go back to the zeros of a context that never coupled, so a step that keeps the
    // physics form (IAU, the device microphysics) does not go on applying the last coupling's values
    for (auto& b : ctx->blk)
      for (const char* n : {"tend_physics.tend_ru_physics", "tend_physics.tend_rtheta_physics",
                            "tend_physics.tend_rho_physics", "tend.scalars_tend"}) {
        Field& f = b.fields[b.by_name[n]];
        HIPCHK(hipMemsetAsync(f.buf[0], 0, field_bytes(b, f), ctx->stream));
      }
  ctx->todyn.flags = flags;
  if (flags) {
    ctx->todyn.iqc = index_qc - 1, ctx->todyn.iqr = index_qr - 1, ctx->todyn.iqi = index_qi - 1;
    ctx->todyn.iqs = index_qs - 1, ctx->todyn.ini = index_ni - 1;
    for (int* i : {&ctx->todyn.iqc, &ctx->todyn.iqr, &ctx->todyn.iqi, &ctx->todyn.iqs, &ctx->todyn.ini})
      if (*i < 0) *i = -1;
  }
  for (auto& b : ctx->blk) b.d.physics = physics_tendencies(ctx) ? 1 : 0;
  ctx->iau.stale = ctx->iau.on != 0;
  // captured steps bake the flags and the indices in; the wind flags decide an exchange point of the step
  if (replan) invalidate_plans(ctx);
  else if (!ctx->host_only) drop_graphs(ctx);
  return MPAS_DYC_OK;
}

int mpas_dyc_physics_get_tend(mpas_dyc_ctx* ctx) {
  if (!ctx) return MPAS_DYC_EINVAL;
  CHK(require_device(ctx));
  if (ctx->tail_pending) {
    ctx->err = "mpas_dyc_physics_get_tend between mpas_dyc_timestep and mpas_dyc_finish_step";
    return MPAS_DYC_ESTATE;
  }
  if (!ctx->todyn.flags) {
    ctx->err = "mpas_dyc_physics_get_tend: no scheme set (mpas_dyc_set_todynamics)";
    return MPAS_DYC_ESTATE;
  }
  HIPCHK(hipSetDevice(ctx->device));
  CHK(todyn_check_inputs(ctx, "mpas_dyc_physics_get_tend"));
  return timed_on_stream(ctx, ctx->todyn.ms, [&]() -> int {
    CHK(todyn_step(ctx, block_ptrs(ctx)));
    HIPCHK(hipGetLastError());
    return MPAS_DYC_OK;
  });
}

int mpas_dyc_set_convective(mpas_dyc_ctx* ctx, int32_t flags) {
  if (!ctx) return MPAS_DYC_EINVAL;
  if (flags & ~CONV_ALL) {
    ctx->err = "mpas_dyc_set_convective: unknown flag bits";
    return MPAS_DYC_EINVAL;
  }
  ctx->conv.flags = flags;
  if (ctx->host_only || !flags) return MPAS_DYC_OK;
  HIPCHK(hipSetDevice(ctx->device));
  if (!group_ready(ctx, G_CONVCOMPUTE)) CHK(alloc_group(ctx, G_CONVCOMPUTE));
  return MPAS_DYC_OK;
}

int mpas_dyc_convective_diagnostics(mpas_dyc_ctx* ctx, int32_t time_level) {
  if (!ctx || (time_level != 1 && time_level != 2)) return MPAS_DYC_EINVAL;
  CHK(require_device(ctx));
  if (ctx->tail_pending) {
    ctx->err = "mpas_dyc_convective_diagnostics between mpas_dyc_timestep and mpas_dyc_finish_step";
    return MPAS_DYC_ESTATE;
  }
  if (!ctx->conv.flags) return MPAS_DYC_OK;
  HIPCHK(hipSetDevice(ctx->device));
  if (!group_ready(ctx, G_CONVCOMPUTE)) CHK(alloc_group(ctx, G_CONVCOMPUTE));
  return timed_on_stream(ctx, ctx->conv.ms, [&]() -> int { return conv_enqueue(ctx, time_level); });
}

int mpas_dyc_set_pv(mpas_dyc_ctx* ctx, int32_t on) {
  if (!ctx) return MPAS_DYC_EINVAL;
  ctx->pv.on = on ? 1 : 0;
  if (ctx->host_only || !on) return MPAS_DYC_OK;
  HIPCHK(hipSetDevice(ctx->device));
  if (!group_ready(ctx, G_PV)) CHK(alloc_group(ctx, G_PV));
  return MPAS_DYC_OK;
}

int mpas_dyc_pv_diagnostics(mpas_dyc_ctx* ctx, int32_t time_level) {
  if (!ctx || (time_level != 1 && time_level != 2)) return MPAS_DYC_EINVAL;
  CHK(require_device(ctx));
  if (ctx->tail_pending) {
    ctx->err = "mpas_dyc_pv_diagnostics between mpas_dyc_timestep and mpas_dyc_finish_step";
    return MPAS_DYC_ESTATE;
  }
  if (!ctx->pv.on) return MPAS_DYC_OK;
  HIPCHK(hipSetDevice(ctx->device));
  bool lists = false;
  CHK(pv_check_prepare(ctx, "mpas_dyc_pv_diagnostics", &lists));
  return timed_on_stream(ctx, ctx->pv.ms, [&]() -> int { return pv_run(ctx, time_level, lists); });
}

int mpas_dyc_set_pv_budget(mpas_dyc_ctx* ctx, int32_t flags) {
  if (!ctx) return MPAS_DYC_EINVAL;
  if (flags & ~PVB_ALL) {
    ctx->err = "mpas_dyc_set_pv_budget: unknown flag bits";
    return MPAS_DYC_EINVAL;
  }
  if (flags && !(flags & PVB_ON)) {
    ctx->err = "mpas_dyc_set_pv_budget: a source bit without MPAS_DYC_PVB_ON";
    return MPAS_DYC_EINVAL;
  }
  if (flags && !ctx->pv.on) {
    ctx->err = "mpas_dyc_set_pv_budget: MPAS_DYC_PVB_ON while mpas_dyc_set_pv is off (the budget reads its outputs)";
    return MPAS_DYC_ESTATE;
  }
  ctx->pvb.flags = flags;
  if (ctx->host_only || !flags) return MPAS_DYC_OK;
  HIPCHK(hipSetDevice(ctx->device));
  if (!group_ready(ctx, G_PVB)) CHK(alloc_group(ctx, G_PVB));
  return MPAS_DYC_OK;
}

int mpas_dyc_pv_budget_diagnostics(mpas_dyc_ctx* ctx, int32_t time_level) {
  if (!ctx || (time_level != 1 && time_level != 2)) return MPAS_DYC_EINVAL;
  CHK(require_device(ctx));
  if (ctx->tail_pending) {
    ctx->err = "mpas_dyc_pv_budget_diagnostics between mpas_dyc_timestep and mpas_dyc_finish_step";
    return MPAS_DYC_ESTATE;
  }
  if (!ctx->pvb.flags) return MPAS_DYC_OK;
  if (!ctx->pv.on) {
    ctx->err = "mpas_dyc_pv_budget_diagnostics: mpas_dyc_set_pv is off (the budget reads its outputs)";
    return MPAS_DYC_ESTATE;
  }
  HIPCHK(hipSetDevice(ctx->device));
  for (auto& b : ctx->blk)
    if (const char* missing = pvb_missing_input(b, ctx->pvb.flags)) {
      ctx->err = std::string("mpas_dyc_pv_budget_diagnostics: ") + missing +
                 (std::string(missing) == "mesh.coeffs_reconstruct" ? " not set (mpas_dyc_init_reconstruct)"
                  : std::string(missing).rfind("mesh.", 0) == 0    ? " not set"
                                                                    : " never allocated (tend_physics)");
      return MPAS_DYC_ESTATE;
    }
  bool lists = false;
  CHK(pv_check_prepare(ctx, "mpas_dyc_pv_budget_diagnostics", &lists));
  if (!group_ready(ctx, G_PVB)) CHK(alloc_group(ctx, G_PVB));
  return timed_on_stream(ctx, ctx->pvb.ms, [&]() -> int {
    CHK(pv_run(ctx, time_level, lists));
    return pvb_run(ctx, time_level, lists);
  });
}

int mpas_dyc_set_isobaric(mpas_dyc_ctx* ctx, int32_t flags) {
  if (!ctx) return MPAS_DYC_EINVAL;
  if (flags & ~ISO_ALL) {
    ctx->err = "mpas_dyc_set_isobaric: unknown flag bits";
    return MPAS_DYC_EINVAL;
  }
  ctx->iso.flags = flags;
  if (ctx->host_only || !flags) return MPAS_DYC_OK;
  HIPCHK(hipSetDevice(ctx->device));
  if (!group_ready(ctx, G_ISOBARIC)) CHK(alloc_group(ctx, G_ISOBARIC));
  return MPAS_DYC_OK;
}

int mpas_dyc_isobaric_diagnostics(mpas_dyc_ctx* ctx, int32_t time_level) {
  if (!ctx || (time_level != 1 && time_level != 2)) return MPAS_DYC_EINVAL;
  CHK(require_device(ctx));
  if (ctx->tail_pending) {
    ctx->err = "mpas_dyc_isobaric_diagnostics between mpas_dyc_timestep and mpas_dyc_finish_step";
    return MPAS_DYC_ESTATE;
  }
  const int flags = ctx->iso.flags;
  if (!flags) return MPAS_DYC_OK;
  HIPCHK(hipSetDevice(ctx->device));
  if (!group_ready(ctx, G_ISOBARIC)) CHK(alloc_group(ctx, G_ISOBARIC));
  if (flags & ISO_VORTICITY) {
    bool lists = false;
    for (auto& b : ctx->blk) {
      if (!find(b, "mesh", "areaTriangle")->buf[0] || !b.kite_set || (int64_t)b.h_cov.size() < 3LL * b.d.nVertices) {
        ctx->err = "mpas_dyc_isobaric_diagnostics: MPAS_DYC_ISO_VORTICITY needs mesh.areaTriangle, kiteAreasOnVertex and "
                   "cellsOnVertex set";
        return MPAS_DYC_ESTATE;
      }
      lists = lists || !b.xl.empty();
    }
    // the vertex pressure of an owned vertex reads halo cells (isobaric_diagnostics.F:397-398)
    if (lists) CHK(mpas_dyc_halo_exchange(ctx, "diag", "pressure_p", 1, 7));
  }
  return timed_on_stream(ctx, ctx->iso.ms, [&]() -> int { return iso_enqueue(ctx, time_level); });
}

int mpas_dyc_set_physics(mpas_dyc_ctx* ctx, int32_t flags) {
  if (!ctx || (flags & ~(MPAS_DYC_PHYSICS_TENDENCIES | MPAS_DYC_PHYSICS_RQVDYNTEN | MPAS_DYC_PHYSICS_MICROPHYSICS)))
    return MPAS_DYC_EINVAL;
  if ((flags & MPAS_DYC_PHYSICS_RQVDYNTEN) && !(flags & MPAS_DYC_PHYSICS_TENDENCIES)) return MPAS_DYC_EINVAL;
  if ((flags & MPAS_DYC_PHYSICS_MICROPHYSICS) && ctx->microp.scheme) {
    ctx->err = "MPAS_DYC_PHYSICS_MICROPHYSICS (the host's microphysics) with mpas_dyc_set_microphysics on";
    return MPAS_DYC_ESTATE;
  }
  if ((flags & MPAS_DYC_PHYSICS_TENDENCIES) && ctx->todyn.flags) {
    ctx->err = "MPAS_DYC_PHYSICS_TENDENCIES (the host's coupled tendencies) with mpas_dyc_set_todynamics on";
    return MPAS_DYC_ESTATE;
  }
  if (!ctx->host_only) {  // a planner's context keeps the flags alone
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  ctx->physics = flags;
  for (auto& b : ctx->blk) b.d.physics = physics_tendencies(ctx) ? 1 : 0;
  ctx->iau.stale = ctx->iau.on != 0;
  if (!ctx->host_only) drop_graphs(ctx);  // captured steps bake the flags in
  return MPAS_DYC_OK;
}

int mpas_dyc_set_iau(mpas_dyc_ctx* ctx, int32_t on, double window_length_s) {
  if (!ctx) return MPAS_DYC_EINVAL;
  if (on && !(window_length_s > 0.0)) {
    ctx->err = "mpas_dyc_set_iau: config_IAU_window_length_s must be positive";
    return MPAS_DYC_EINVAL;
  }
  ctx->iau.on = on ? 1 : 0;
  ctx->iau.window = on ? window_length_s : 0.0;
  ctx->iau.wgt = 0.0;
  if (ctx->host_only) return MPAS_DYC_OK;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (on)  // the increments a host has not set are zero; and the step's physics + IAU arrays
    for (Group g : {G_IAU_INCR, G_IAU_SUMS}) CHK(alloc_group(ctx, g));
  for (auto& b : ctx->blk) b.d.physics = physics_tendencies(ctx) ? 1 : 0;
  ctx->iau.stale = on != 0;
  drop_graphs(ctx);  // captured steps bake the flag, the weight and the tendencies' pointers in
  return MPAS_DYC_OK;
}

int mpas_dyc_iau_weight(const mpas_dyc_ctx* ctx, double dt, int32_t itimestep, double* wgt) {
  if (!ctx || !wgt || !(dt > 0.0)) return MPAS_DYC_EINVAL;
  *wgt = 0.0;
  if (!ctx->iau.on) return MPAS_DYC_OK;
  const long nsteps_iau = std::lround(ctx->iau.window / dt);  // nint: halves away from zero
  if (itimestep <= nsteps_iau) *wgt = 1.0 / ctx->iau.window;
  return MPAS_DYC_OK;
}

int mpas_dyc_set_diag_update(mpas_dyc_ctx* ctx, int32_t flags) {
  if (!ctx) return MPAS_DYC_EINVAL;
  CHK(convdiag_check_flags(ctx, flags, "mpas_dyc_set_diag_update"));
  ctx->convdiag.flags = flags;
  if (ctx->host_only || !flags) return MPAS_DYC_OK;
  HIPCHK(hipSetDevice(ctx->device));
  if (!group_ready(ctx, G_CONVDIAG)) CHK(alloc_group(ctx, G_CONVDIAG));
  return MPAS_DYC_OK;
}

int mpas_dyc_diag_update(mpas_dyc_ctx* ctx) {
  if (!ctx) return MPAS_DYC_EINVAL;
  CHK(require_device(ctx));
  if (ctx->tail_pending) {
    ctx->err = "mpas_dyc_diag_update between mpas_dyc_timestep and mpas_dyc_finish_step";
    return MPAS_DYC_ESTATE;
  }
  if (!ctx->convdiag.flags) return MPAS_DYC_OK;
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->convdiag.flags & CONVDIAG_UH) {
    if (!ctx->bnd_ready) CHK(compute_bnd(ctx));  // rebuilds the table after a new cellsOnVertex
    for (auto& b : ctx->blk) {
      if (!b.cv.ready) CHK(convdiag_table(ctx, b));
      if (!find(b, "mesh", "areaCell")->buf[0]) {
        ctx->err = "mpas_dyc_diag_update: mesh.areaCell not set (MPAS_DYC_DIAG_UPDRAFT_HELICITY_MAX divides by it)";
        return MPAS_DYC_ESTATE;
      }
    }
  }
  return timed_on_stream(ctx, ctx->convdiag.ms, [&]() -> int { return convdiag_enqueue(ctx); });
}

int mpas_dyc_diag_reset(mpas_dyc_ctx* ctx, int32_t flags) {
  if (!ctx) return MPAS_DYC_EINVAL;
  CHK(convdiag_check_flags(ctx, flags, "mpas_dyc_diag_reset"));
  CHK(require_device(ctx));
  if (!group_ready(ctx, G_CONVDIAG)) return MPAS_DYC_OK;  // never allocated: zero when they are
  HIPCHK(hipSetDevice(ctx->device));
  for (auto& b : ctx->blk)
    for (int i = 0; i < 3; ++i) {
      if (!(flags & (1 << i))) continue;
      Field* f = find(b, "diag", CONVDIAG_FIELDS[i]);
      HIPCHK(hipMemsetAsync(f->buf[0], 0, field_bytes(b, *f), ctx->stream));
    }
  return MPAS_DYC_OK;
}

int mpas_dyc_set_microphysics(mpas_dyc_ctx* ctx, int32_t scheme, int32_t index_qc, int32_t index_qr,
                              double bucket_rainnc) {
  if (!ctx) return MPAS_DYC_EINVAL;
  if (scheme != MPAS_DYC_MICROP_OFF && scheme != MPAS_DYC_MICROP_KESSLER) {
    ctx->err = "mpas_dyc_set_microphysics: unknown scheme";
    return MPAS_DYC_EINVAL;
  }
  if (scheme != MPAS_DYC_MICROP_OFF) {
    const int ns = ctx->blk.empty() ? 0 : ctx->blk[0].d.ns;
    if (index_qc < 1 || index_qc > ns || index_qr < 1 || index_qr > ns || index_qc == index_qr ||
        index_qc - 1 == ctx->index_qv || index_qr - 1 == ctx->index_qv) {
      ctx->err = "mpas_dyc_set_microphysics: index_qc / index_qr must be distinct scalars in 1..num_scalars, not index_qv";
      return MPAS_DYC_EINVAL;
    }
    if (ctx->physics & MPAS_DYC_PHYSICS_MICROPHYSICS) {
      ctx->err = "mpas_dyc_set_microphysics with MPAS_DYC_PHYSICS_MICROPHYSICS (the host's microphysics) set";
      return MPAS_DYC_ESTATE;
    }
    for (auto& b : ctx->blk) CHK(kessler_check_levels(ctx, b.d.K));
  }
  if (!ctx->host_only) {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (scheme != MPAS_DYC_MICROP_OFF && !group_ready(ctx, G_MICROP)) CHK(alloc_group(ctx, G_MICROP));
  }
  ctx->microp.scheme = scheme;
  if (scheme != MPAS_DYC_MICROP_OFF) {
    ctx->microp.iqc = index_qc - 1;
    ctx->microp.iqr = index_qr - 1;
    ctx->microp.bucket = bucket_rainnc;
  }
  for (auto& b : ctx->blk) {
    b.d.physics = physics_tendencies(ctx) ? 1 : 0;
    if (scheme != MPAS_DYC_MICROP_OFF) b.d.diabatic = 1;  // the step reads the scheme's rt_diabatic_tend
  }
  if (!ctx->host_only) drop_graphs(ctx);  // captured steps bake the switch, the indices and the bucket in
  return MPAS_DYC_OK;
}

int mpas_dyc_microphysics(mpas_dyc_ctx* ctx, double dt, int32_t time_level) {
  if (!ctx || !(dt > 0.0) || (time_level != 1 && time_level != 2)) return MPAS_DYC_EINVAL;
  CHK(require_device(ctx));
  if (ctx->microp.scheme == MPAS_DYC_MICROP_OFF) {
    ctx->err = "mpas_dyc_microphysics: no scheme set (mpas_dyc_set_microphysics)";
    return MPAS_DYC_ESTATE;
  }
  HIPCHK(hipSetDevice(ctx->device));
  return timed_on_stream(ctx, ctx->microp.ms, [&]() -> int {
    CHK(kessler_enqueue(ctx, dt, time_level));
    HIPCHK(hipGetLastError());
    return MPAS_DYC_OK;
  });
}

}  // extern "C"

namespace {

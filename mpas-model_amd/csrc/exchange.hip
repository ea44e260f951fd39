// Halo exchange (mpas_dmpar_exch_halo_field, framework/mpas_dmpar.F): the planner that compiles an
// exchange point into an XPlan, and the code that runs one.  Included by dycore.hip inside its
// namespace, after the structs (Field, XList, Block, XPlan, mpas_dyc_ctx), drop_graphs and the
// kernel-family predicates (batched, pair_layout).
//
// The planner works in stages (build_plan): classify names the exchange point, plan_layout does the
// host bookkeeping (segments as indices, messages, totals -- all a dry run needs), plan_bind picks
// the transport, allocates the buffers and forms the XSeg records, and fuse_substep / fuse_rec build
// the device maps of the exchanges whose pack and unpack their producers and consumers do.
bool needs_exchange(const mpas_dyc_ctx* ctx) { return ctx->blk.size() > 1 || ctx->nranks > 1 || ctx->loopback; }

// An exchange plan holds the fields' buffers, so its key names them: the time level and, per field,
// which of the buffers that the step's rotations move it is (buffer index of block 0)
std::string plan_key(mpas_dyc_ctx* ctx, const std::vector<XField>& fs) {
  std::string k = std::to_string(ctx->cur) + (ctx->plain_exchange ? "plain" : "");
  for (const auto& f : fs) {
    k += "|" + std::string(f.pool) + "." + f.name + "." + std::to_string(f.tl) + "." + std::to_string(f.layers);
    Field* F = ctx->blk.empty() ? nullptr : find(ctx->blk[0], f.pool, f.name);
    if (F && F->rot >= 0) k += "@" + std::to_string(F->rot_pos);
    else if (F && swaps_levels(*F)) k += "@" + std::to_string(slot_of(ctx, *F, f.tl) ^ F->flip);
  }
  return k;
}

const XList* find_list(const Block& b, int loc, int layer, int dir, int peer_rank, int peer_block) {
  for (const auto& x : b.xl)
    if (x.loc == loc && x.layer == layer && x.dir == dir && x.peer_rank == peer_rank && x.peer_block == peer_block)
      return &x;
  return nullptr;
}

// true if `key` contains one of the comma-separated substrings of `list` (a debugging switch's value)
bool key_in_list(const char* list, const std::string& key) {
  const std::string s = list ? list : "";
  for (size_t a = 0; a < s.size();) {
    size_t b = s.find(',', a);
    if (b == std::string::npos) b = s.size();
    if (b > a && key.find(s.substr(a, b - a)) != std::string::npos) return true;
    a = b + 1;
  }
  return false;
}

// The one way a plan gets device memory: the allocation (at least 8 bytes) is recorded in pl.owned
// the moment it exists, so free_plan frees it whatever fails later; `d` is a view.
template <class T>
int plan_alloc(mpas_dyc_ctx* ctx, XPlan& pl, T*& d, size_t bytes) {
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, std::max<size_t>(bytes, 8)));
  pl.owned.push_back(p);
  d = (T*)p;
  return MPAS_DYC_OK;
}
template <class T>
int plan_upload(mpas_dyc_ctx* ctx, XPlan& pl, T*& d, const void* host, size_t bytes) {
  CHK(plan_alloc(ctx, pl, d, bytes));
  if (bytes) HIPCHK(hipMemcpy((void*)d, host, bytes, hipMemcpyHostToDevice));
  return MPAS_DYC_OK;
}
template <class T, class V>
int plan_upload(mpas_dyc_ctx* ctx, XPlan& pl, T*& d, const std::vector<V>& host) {
  return plan_upload(ctx, pl, d, host.data(), host.size() * sizeof(V));
}

void free_plan(XPlan& pl) {
  for (void* p : pl.mapped) (void)hipIpcCloseMemHandle(p);
  for (void* p : pl.owned) (void)hipFree(p);
  pl = XPlan{};
}

// loopback: per emulated peer rank, its (send, receive) messages (either may be missing)
std::map<int, std::pair<const XMsg*, const XMsg*>> loopback_pairs(const XPlan& pl) {
  std::map<int, std::pair<const XMsg*, const XMsg*>> peers;
  for (const XMsg& m : pl.rsend) peers[m.peer_rank].first = &m;
  for (const XMsg& m : pl.rrecv) peers[m.peer_rank].second = &m;
  return peers;
}

void invalidate_plans(mpas_dyc_ctx* ctx) {
  if (!ctx->host_only) (void)hipStreamSynchronize(ctx->stream);
  for (auto& kv : ctx->plans) free_plan(kv.second);
  ctx->plans.clear();
  ctx->planned.clear();
  drop_graphs(ctx);
}

bool is_local(const mpas_dyc_ctx* ctx, int peer_rank) { return peer_rank == ctx->rank && !ctx->rccl_local; }

std::vector<std::pair<int, int>> peers_of(const Block& b, int dir) {
  std::vector<std::pair<int, int>> peers;
  for (const auto& x : b.xl)
    if (x.dir == dir && x.n > 0 && x.peer_block >= 0) peers.emplace_back(x.peer_rank, x.peer_block);
  std::sort(peers.begin(), peers.end());
  peers.erase(std::unique(peers.begin(), peers.end()), peers.end());
  return peers;
}

// Auto mode splits only when halo traffic goes through RCCL: block-to-block copies inside
// one GPU are a single short kernel, and splitting them only adds launches.
bool split_phase(const mpas_dyc_ctx* ctx) {
  if (!needs_exchange(ctx)) return false;
  if (ctx->overlap >= 0) return ctx->overlap != 0;
  if (ctx->p2p) return false;  // the transfer is the receiver's kernel: nothing to overlap it with
  return ctx->nranks > 1 || ctx->rccl_local || ctx->loopback;
}

// ---- the planner, stage 1: classify ----
// The exchange points whose pack and unpack kernels their producers and consumers can replace:
//   X_SUBSTEP  the per-sub-step exchange (diag rtheta_pp [+ rho_pp], halo layer 1): the acoustic cell
//              phase packs, the next edge phase or the stage's last damping unpacks (PackMap / UnpackMap)
//   X_RECOVERY the 876-887 exchange (rw_p, ru_p, rho_pp all layers, rtheta_pp layer 2): the stage's last
//              cell phase and damping pack, the halo recovery unpacks (XPack / XUnpack, dycore.h)
//   X_TEND_U   the tend_u exchange (642), packed by the stage's final tend_u kernel (k_dyn_edges_p with
//              finalize, k_dyn_edges_rk1b_b) and unpacked by k_smlstep_pert_b
//   X_U        the u exchange after the recovery (988); regional runs overwrite u after the recovery
enum XKind { X_NONE, X_SUBSTEP, X_RECOVERY, X_TEND_U, X_U };
struct XClass {
  XKind kind = X_NONE;
  std::vector<int> fid;  // per field of the call, its index in the kind's maps (X_SUBSTEP: 1 = rho_pp)
};

// The only place that tells exchange points apart by their fields' names.
XClass classify(const mpas_dyc_ctx* ctx, const std::vector<XField>& fs) {
  auto is = [](const XField& f, const char* pool, const char* name) {
    return std::string(f.pool) == pool && std::string(f.name) == name;
  };
  // a field's index in the maps of kind k, or -1: no field of such an exchange
  auto fid_of = [&](XKind k, const XField& f) -> int {
    const unsigned l = f.layers;
    switch (k) {
      case X_SUBSTEP: return l != 0x1u ? -1 : is(f, "diag", "rtheta_pp") ? 0 : is(f, "diag", "rho_pp") ? 1 : -1;
      case X_RECOVERY:
        if (is(f, "diag", "rw_p") && (l == ALL_LAYERS || l == 0x1u)) return 0;  // 0x1: MPAS_DYCORE_HALO_TRIM
        if (is(f, "diag", "rho_pp") && l == ALL_LAYERS) return 1;
        if (is(f, "diag", "rtheta_pp") && l == 0x2u) return 2;
        return is(f, "diag", "ru_p") && l == ALL_LAYERS ? 0 : -1;  // the edge field
      case X_TEND_U: return is(f, "tend", "u") && l == 0x1u ? 0 : -1;
      case X_U: return !ctx->lbc && is(f, "state", "u") && f.tl == 2 && l == ALL_LAYERS ? 0 : -1;
      default: return -1;
    }
  };
  XClass c;
  if (ctx->plain_exchange) return c;
  const size_t n = fs.size();
  for (XKind k : {X_SUBSTEP, X_RECOVERY, X_TEND_U, X_U}) {
    if (k == X_SUBSTEP ? n < 1 || n > 2 : k == X_RECOVERY ? n != 4 : n != 1) continue;
    c.fid.clear();
    for (const auto& f : fs) c.fid.push_back(fid_of(k, f));
    if (std::count(c.fid.begin(), c.fid.end(), -1) == 0) {
      c.kind = k;
      break;
    }
  }
  return c;
}

// ---- the planner, stage 2: layout (host bookkeeping only: no Field::buf, no device pointer) ----
// A pack or unpack segment before any buffer exists: sub-field `sub` of fs[field] in block `block`,
// the elements of `list` (the block's send list of a pack segment, its receive list of an unpack one)
struct LSeg {
  int block, field, sub;
  Loc loc;
  int inner;          // doubles per element of the sub-field
  const XList* list;  // positional when list->peer_block < 0
  int64_t off;        // doubles into the send or the receive buffer; -1: a direct copy (pack segments)
  // a direct copy fills the halo of block to_block of this process, at the elements of its list to_list
  int to_block = -1;
  const XList* to_list = nullptr;
};
struct XLayout {
  XClass cls;                        // kind X_NONE once a direct copy or a positional list rules fusion out
  std::vector<LSeg> pre, post;       // pack and unpack segments, in launch order
  std::vector<XMsg> rsend, rrecv;    // one message per peer rank, in matching order
  int64_t stotal = 0, rtotal = 0;    // doubles in the send and the receive buffer
  int maxn_pre = 0, maxn_post = 0;   // the longest list among pre / post
  bool positional = false;
};

Field* exchange_field(mpas_dyc_ctx* ctx, Block& b, const XField& f) {
  Field* F = find(b, f.pool, f.name);
  // (a field allocated at its first set_field has no buffer yet: a null test, and not in a dry run)
  if (!F || F->is_int || F->loc == L_NONE || (!ctx->host_only && !F->buf[0])) {
    ctx->err = std::string("halo exchange of unsupported field ") + f.pool + "." + f.name;
    return nullptr;
  }
  return F;
}

// The order both sides of a message agree on: the fields in call order, per field the exchanged halo
// layers in ascending order, per layer the sub-fields (a scalar-major field moves as nsub fields of
// inner/nsub doubles).  fn(field index, the field in block b, layer, sub-field) returns an error code.
template <class Fn>
int for_each_subfield(mpas_dyc_ctx* ctx, Block& b, const std::vector<XField>& fs, Fn fn) {
  for (size_t fi = 0; fi < fs.size(); ++fi) {
    Field* F = exchange_field(ctx, b, fs[fi]);
    if (!F) return MPAS_DYC_EINVAL;
    for (int layer = 1; layer <= 3; ++layer) {
      if (!((fs[fi].layers >> (layer - 1)) & 1u)) continue;
      for (int is = 0; is < F->nsub; ++is) CHK(fn((int)fi, *F, layer, is));
    }
  }
  return MPAS_DYC_OK;
}

int lists_disagree(mpas_dyc_ctx* ctx, int from, int to) {
  ctx->err = "send/recv lists of blocks " + std::to_string(from) + "->" + std::to_string(to) + " disagree";
  return MPAS_DYC_EINVAL;
}

// Block-pair lists.  Message layout: per block, peers in (rank, block) order; per peer the order of
// for_each_subfield.  A peer block of this process is filled by a direct copy (no message).
int layout_block_pairs(mpas_dyc_ctx* ctx, const std::vector<XField>& fs, XLayout& lay) {
  const int nb = (int)ctx->blk.size();
  for (int bi = 0; bi < nb; ++bi) {
    Block& b = ctx->blk[bi];
    for (const auto& pr : peers_of(b, MPAS_DYC_SEND)) {
      const bool local = is_local(ctx, pr.first);
      if (local && (pr.second < 0 || pr.second >= nb)) {
        ctx->err = "exchange list names block " + std::to_string(pr.second) + " not in this process";
        return MPAS_DYC_EINVAL;
      }
      const int64_t start = lay.stotal;
      CHK(for_each_subfield(ctx, b, fs, [&](int fi, const Field& F, int layer, int is) -> int {
        const XList* sx = find_list(b, (int)F.loc, layer, MPAS_DYC_SEND, pr.first, pr.second);
        if (!sx || sx->n == 0) return MPAS_DYC_OK;
        LSeg sg{bi, fi, is, F.loc, (int)(F.inner / F.nsub), sx, -1};
        if (local) {
          sg.to_block = pr.second;
          sg.to_list = find_list(ctx->blk[pr.second], (int)F.loc, layer, MPAS_DYC_RECV, ctx->rank, bi);
          if (!sg.to_list || sg.to_list->n != sx->n) return lists_disagree(ctx, bi, pr.second);
          // a direct copy would reach the peer's halo before its cell phase reads it
          lay.cls.kind = X_NONE;
        } else {
          sg.off = lay.stotal;
          lay.stotal += (int64_t)sx->n * sg.inner;
        }
        lay.pre.push_back(sg);
        lay.maxn_pre = std::max(lay.maxn_pre, sx->n);
        return MPAS_DYC_OK;
      }));
      if (!local && lay.stotal > start) lay.rsend.push_back(XMsg{bi, pr.first, pr.second, start, lay.stotal - start});
    }
    for (const auto& pr : peers_of(b, MPAS_DYC_RECV)) {
      const bool local = is_local(ctx, pr.first);
      const int64_t start = lay.rtotal;
      CHK(for_each_subfield(ctx, b, fs, [&](int fi, const Field& F, int layer, int is) -> int {
        const XList* rx = find_list(b, (int)F.loc, layer, MPAS_DYC_RECV, pr.first, pr.second);
        if (!rx || rx->n == 0) return MPAS_DYC_OK;
        if (local) {  // filled by the sender's direct copy; check that one exists
          const XList* sx = (pr.second >= 0 && pr.second < nb)
                                ? find_list(ctx->blk[pr.second], (int)F.loc, layer, MPAS_DYC_SEND, ctx->rank, bi)
                                : nullptr;
          return (!sx || sx->n != rx->n) ? lists_disagree(ctx, pr.second, bi) : MPAS_DYC_OK;
        }
        lay.post.push_back(LSeg{bi, fi, is, F.loc, (int)(F.inner / F.nsub), rx, lay.rtotal});
        lay.rtotal += (int64_t)rx->n * (F.inner / F.nsub);
        lay.maxn_post = std::max(lay.maxn_post, rx->n);
        return MPAS_DYC_OK;
      }));
      if (!local && lay.rtotal > start) lay.rrecv.push_back(XMsg{bi, pr.first, pr.second, start, lay.rtotal - start});
    }
  }
  return MPAS_DYC_OK;
}

// Positional lists (mpas_dyc_set_exchange_positions): per peer rank one message, laid out as
// mpas_dmpar lays out its buffer (mpas_dmpar.F:5448-5535): per field, per halo layer a region whose
// slots the blocks of this process fill at their positions; the receiver reads its blocks' slots
// at theirs.  Region sizes are the largest position over the blocks (both sides agree: it is one
// buffer).  No fused pack / unpack for them.
int layout_positional(mpas_dyc_ctx* ctx, const std::vector<XField>& fs, XLayout& lay) {
  const int nb = (int)ctx->blk.size();
  std::set<int> pos_ranks;
  for (const auto& b : ctx->blk)
    for (const auto& x : b.xl)
      if (x.peer_block < 0 && x.n > 0) pos_ranks.insert(x.peer_rank);
  if (pos_ranks.empty()) return MPAS_DYC_OK;
  for (int dir = MPAS_DYC_SEND; dir <= MPAS_DYC_RECV; ++dir)
    for (int pr : pos_ranks) {
      const bool send = dir == MPAS_DYC_SEND;
      int64_t& total = send ? lay.stotal : lay.rtotal;
      const int64_t start = total;
      CHK(for_each_subfield(ctx, ctx->blk[0], fs, [&](int fi, const Field& F0, int layer, int is) -> int {
        std::vector<const XList*> lx(nb, nullptr);
        int64_t npos = 0;
        for (int bi = 0; bi < nb; ++bi)
          for (const auto& x : ctx->blk[bi].xl)
            if (x.peer_block < 0 && x.n > 0 && x.peer_rank == pr && x.dir == dir && x.loc == (int)F0.loc &&
                x.layer == layer) {
              lx[bi] = &x;
              for (int32_t q : x.h_pos) npos = std::max<int64_t>(npos, (int64_t)q + 1);
            }
        const int sub_inner = (int)(F0.inner / F0.nsub);
        for (int bi = 0; bi < nb; ++bi) {
          if (!lx[bi]) continue;
          if (!exchange_field(ctx, ctx->blk[bi], fs[fi])) return MPAS_DYC_EINVAL;
          (send ? lay.pre : lay.post).push_back(LSeg{bi, fi, is, F0.loc, sub_inner, lx[bi], total});
          int& maxn = send ? lay.maxn_pre : lay.maxn_post;
          maxn = std::max(maxn, lx[bi]->n);
        }
        total += npos * sub_inner;
        return MPAS_DYC_OK;
      }));
      if (total > start) (send ? lay.rsend : lay.rrecv).push_back(XMsg{-1, pr, -1, start, total - start});
    }
  lay.positional = true;
  lay.cls.kind = X_NONE;
  for (const auto& m : lay.rsend)
    for (const auto& m2 : lay.rsend)
      if (m.peer_rank == m2.peer_rank && (m.block < 0) != (m2.block < 0)) {
        ctx->err = "rank " + std::to_string(m.peer_rank) + " has both positional and block-pair exchange lists";
        return MPAS_DYC_EINVAL;
      }
  return MPAS_DYC_OK;
}

// One RCCL message per peer rank, as mpas_dmpar packs one buffer per processor for all its
// blocks (mpas_dmpar.F:5386-5552): the block-pair messages to one rank (sorted by the caller) are
// laid out back to back and go as one send / one receive; the segments' offsets follow.  (With one
// block per rank nothing changes; with several, e.g. bench.py --blocks B or --rccl-local, the group
// holds one message per peer rank instead of one per block pair.)
void merge_by_rank(std::vector<XMsg>& msgs, std::vector<LSeg>& segs) {
  std::map<int64_t, int64_t> base;  // message start, old layout -> new layout
  int64_t cur = 0;
  for (const XMsg& m : msgs) {
    base[m.off] = cur;
    cur += m.count;
  }
  for (LSeg& s : segs) {
    if (s.off < 0) continue;  // a direct in-process copy
    auto it = std::prev(base.upper_bound(s.off));
    s.off = it->second + (s.off - it->first);
  }
  std::vector<XMsg> merged;
  for (XMsg m : msgs) {
    m.off = base[m.off];
    if (!merged.empty() && merged.back().peer_rank == m.peer_rank) {
      merged.back().count += m.count;
      merged.back().block = merged.back().peer_block = -1;  // several block pairs
    } else {
      merged.push_back(m);
    }
  }
  msgs.swap(merged);
}

int plan_layout(mpas_dyc_ctx* ctx, const std::vector<XField>& fs, XLayout& lay) {
  lay.cls = classify(ctx, fs);
  CHK(layout_block_pairs(ctx, fs, lay));
  CHK(layout_positional(ctx, fs, lay));
  if ((!lay.rsend.empty() || !lay.rrecv.empty()) && !ctx->comm && !(ctx->host_allgather && ctx->p2p) &&
      !ctx->host_only) {
    ctx->err = "exchange lists name other processes but no communicator was set (mpas_dyc_comm_init)";
    return MPAS_DYC_ECOMM;
  }
  // point-to-point messages between two ranks match in issue order: order both sides by
  // (source block, destination block)
  std::sort(lay.rsend.begin(), lay.rsend.end(), [](const XMsg& a, const XMsg& b) {
    return std::make_tuple(a.peer_rank, a.block, a.peer_block) < std::make_tuple(b.peer_rank, b.block, b.peer_block);
  });
  std::sort(lay.rrecv.begin(), lay.rrecv.end(), [](const XMsg& a, const XMsg& b) {
    return std::make_tuple(a.peer_rank, a.peer_block, a.block) < std::make_tuple(b.peer_rank, b.peer_block, b.block);
  });
  merge_by_rank(lay.rsend, lay.pre);
  merge_by_rank(lay.rrecv, lay.post);
  return MPAS_DYC_OK;
}

// ---- the planner, stage 3: bind (transport, buffers, XSeg records) ----
double* subfield_ptr(mpas_dyc_ctx* ctx, const XField& f, int block, int sub, int inner) {
  Block& b = ctx->blk[block];
  Field* F = find(b, f.pool, f.name);
  return (double*)F->buf[slot_of(ctx, *F, f.tl)] + (size_t)sub * nloc(b, F->loc) * inner;
}

// Chooses the transport (pl.p2p, pl.pull), allocates the buffers and forms the pack and unpack
// segments `pre` / `post`.  A pull plan is complete after it (pl.h_pre .. pl.d_local; no buffers).
int plan_bind(mpas_dyc_ctx* ctx, const std::vector<XField>& fs, const XLayout& lay, XPlan& pl, std::vector<XSeg>& pre,
              std::vector<XSeg>& post) {
  for (const LSeg& s : lay.pre) {
    XSeg sg{};
    sg.src = subfield_ptr(ctx, fs[s.field], s.block, s.sub, s.inner);
    sg.sidx = s.list->d_idx;
    sg.n = s.list->n;
    sg.inner = s.inner;
    if (s.to_list) {
      sg.dst = subfield_ptr(ctx, fs[s.field], s.to_block, s.sub, s.inner);
      sg.didx = s.to_list->d_idx;
    } else {
      sg.didx = s.list->d_pos;  // null unless positional
    }
    pre.push_back(sg);
  }
  for (const LSeg& s : lay.post) {
    XSeg sg{};
    sg.sidx = s.list->d_pos;  // null unless positional
    sg.dst = subfield_ptr(ctx, fs[s.field], s.block, s.sub, s.inner);
    sg.didx = s.list->d_idx;
    sg.n = s.list->n;
    sg.inner = s.inner;
    post.push_back(sg);
  }
  int64_t stotal = lay.stotal, rtotal = lay.rtotal;
  if (ctx->loopback) stotal = rtotal = stotal + rtotal;  // rccl_group's loopback pairs stay inside
  // with other ranks, every exchange point is a one-sided one on every rank, messages or not: the
  // set-up numbers the exchange points in the same order on every rank (flag indices, records)
  pl.p2p = ctx->p2p && (!pl.rsend.empty() || !pl.rrecv.empty() || ctx->nranks > 1);
  pl.pull = pl.p2p && ctx->p2p_pull && !lay.positional && !split_phase(ctx);
  // debugging: MPAS_DYCORE_P2P_BUFFERS names exchange points (key substrings) to run in buffers mode
  if (pl.pull && key_in_list(getenv("MPAS_DYCORE_P2P_BUFFERS"), plan_key(ctx, fs))) pl.pull = false;
  if (pl.pull) {
    // the receiver copies from the fields: no buffers, and the kernels store and read the fields
    // themselves (no fused pack / unpack)
    pl.h_pre = pre;
    pl.h_post = post;
    std::vector<XSeg> loc;
    for (size_t i = 0; i < pre.size(); ++i) {
      pl.h_pre_off.push_back(lay.pre[i].off);
      pl.h_pre_idx.push_back(&lay.pre[i].list->h_idx);
      if (lay.pre[i].off < 0) {
        loc.push_back(pre[i]);
        pl.maxn_local = std::max(pl.maxn_local, pre[i].n);
      }
    }
    for (const LSeg& s : lay.post) pl.h_post_off.push_back(s.off);
    pl.nlocal = (int)loc.size();
    if (pl.nlocal) CHK(plan_upload(ctx, pl, pl.d_local, loc));
    return MPAS_DYC_OK;
  }
  if (pl.p2p) {
    // read by the peers (IPC): ordinary device memory, as the fields a pull reads -- the producer's
    // stores reach memory when its kernel ends (the L2 write-back that makes them visible to the
    // other XCDs), and the peers load it with system-scope loads (an uncached allocation here was
    // read stale by a peer process now and then: halo.hip)
    CHK(plan_alloc(ctx, pl, pl.sendbuf, std::max<int64_t>(stotal, 1) * sizeof(double) + 256));
  } else if (stotal) {
    CHK(plan_alloc(ctx, pl, pl.sendbuf, stotal * sizeof(double)));
  }
  // 256 B of slack: a fused unpack (ld_pp) reads the two levels of its lane's pair, one past the
  // last column at an odd K
  if (rtotal) CHK(plan_alloc(ctx, pl, pl.recvbuf, rtotal * sizeof(double) + 256));
  for (size_t i = 0; i < pre.size(); ++i)
    if (lay.pre[i].off >= 0) pre[i].dst = pl.sendbuf + lay.pre[i].off;
  for (size_t i = 0; i < post.size(); ++i) post[i].src = pl.recvbuf + lay.post[i].off;
  pl.npre = (int)pre.size();
  pl.npost = (int)post.size();
  return MPAS_DYC_OK;
}

// ---- the planner, stage 4: fused maps ----
// (never with a direct copy, a positional list or a pull: every segment lies in a buffer)
// The CSR maps' one builder: per[i] holds element i's slots (bucket); uploaded are start[n + 1]
// (prefix) and the slots' two halves in element order (`b` only if asked for).  Nothing if no
// element has a slot.
template <class A, class B>
int csr_upload(mpas_dyc_ctx* ctx, XPlan& pl, const std::vector<std::vector<std::pair<A, B>>>& per, const int*& start,
               const A*& a, const B** b) {
  std::vector<int> h_start(per.size() + 1, 0);
  std::vector<A> h_a;
  std::vector<B> h_b;
  for (size_t i = 0; i < per.size(); ++i) {
    h_start[i] = (int)h_a.size();
    for (const auto& sl : per[i]) {
      h_a.push_back(sl.first);
      h_b.push_back(sl.second);
    }
  }
  h_start[per.size()] = (int)h_a.size();
  if (h_a.empty()) return MPAS_DYC_OK;
  CHK(plan_upload(ctx, pl, start, h_start));
  CHK(plan_upload(ctx, pl, a, h_a));
  if (b) CHK(plan_upload(ctx, pl, *b, h_b));
  return MPAS_DYC_OK;
}

bool all_blocks(const mpas_dyc_ctx* ctx, bool (*pred)(const Dims&)) {
  for (const auto& b : ctx->blk)
    if (!pred(b.d)) return false;
  return true;
}

// X_SUBSTEP pack, per block: CSR over owned cells of (rtheta_pp slot, rho_pp slot) pairs; a cell has
// one slot per RCCL peer that needs it (element i of a peer's list in both fields' segments)
int substep_pack_maps(mpas_dyc_ctx* ctx, const XLayout& lay, bool with_rho, XPlan& pl) {
  const int nb = (int)ctx->blk.size();
  pl.pack.assign(nb, PackMap{});
  for (int bi = 0; bi < nb; ++bi) {
    std::map<std::pair<const XList*, int>, std::pair<double*, double*>> slot;  // (list, i) -> (rt, rho)
    for (const LSeg& s : lay.pre) {
      if (s.block != bi) continue;
      for (int i = 0; i < s.list->n; ++i) {
        auto& e = slot[{s.list, i}];
        (lay.cls.fid[s.field] ? e.second : e.first) = pl.sendbuf + s.off + (size_t)i * s.inner;
      }
    }
    std::vector<std::vector<std::pair<double*, double*>>> per_cell(ctx->blk[bi].d.nCellsSolve);
    for (const auto& kv : slot) per_cell[kv.first.first->h_idx[kv.first.second]].push_back(kv.second);
    PackMap& pm = pl.pack[bi];
    CHK(csr_upload(ctx, pl, per_cell, pm.start, pm.rt, with_rho ? &pm.rho : nullptr));
  }
  return MPAS_DYC_OK;
}

// X_SUBSTEP unpack, per block: halo cell -> its columns in the receive buffer
int substep_unpack_maps(mpas_dyc_ctx* ctx, const XLayout& lay, bool with_rho, XPlan& pl) {
  const int nb = (int)ctx->blk.size();
  pl.unpack.assign(nb, UnpackMap{});
  for (int bi = 0; bi < nb; ++bi) {
    const Dims& d = ctx->blk[bi].d;
    const int nh = d.nCells - d.nCellsSolve;
    std::vector<int> rt(nh, -1), rho(nh, -1);
    bool any = false;
    for (const LSeg& s : lay.post) {
      if (s.block != bi) continue;
      for (int i = 0; i < s.list->n; ++i) {
        (lay.cls.fid[s.field] ? rho : rt)[s.list->h_idx[i] - d.nCellsSolve] = (int)(s.off + (int64_t)i * s.inner);
        any = true;
      }
    }
    if (!any) continue;
    UnpackMap& um = pl.unpack[bi];
    um.recv = pl.recvbuf;
    CHK(plan_upload(ctx, pl, um.rt, rt));
    if (with_rho) CHK(plan_upload(ctx, pl, um.rho, rho));
  }
  return MPAS_DYC_OK;
}

int fuse_substep(mpas_dyc_ctx* ctx, const XLayout& lay, bool with_rho, XPlan& pl) {
  if (lay.pre.empty() || !all_blocks(ctx, batched)) return MPAS_DYC_OK;
  CHK(substep_pack_maps(ctx, lay, with_rho, pl));
  pl.fused_pack = ctx->fused_pack_enabled;
  // the unpack maps' consumers are pair kernels only
  if (!all_blocks(ctx, pair_layout) || lay.post.empty() || !ctx->fused_pack_enabled) return MPAS_DYC_OK;
  CHK(substep_unpack_maps(ctx, lay, with_rho, pl));
  pl.fused_unpack = true;
  return MPAS_DYC_OK;
}

// X_RECOVERY / X_TEND_U / X_U pack of block bi's cells or edges: per owned element, (field,
// send-buffer column) slots in element order
int rec_pack_map(mpas_dyc_ctx* ctx, const XLayout& lay, int bi, Loc loc, int nsolve, XPlan& pl, XPack& xp) {
  std::vector<std::vector<std::pair<int, double*>>> per(nsolve);
  for (const LSeg& s : lay.pre) {
    if (s.block != bi || s.loc != loc) continue;
    for (int i = 0; i < s.list->n; ++i)
      per[s.list->h_idx[i]].emplace_back(lay.cls.fid[s.field], pl.sendbuf + s.off + (size_t)i * s.inner);
  }
  return csr_upload(ctx, pl, per, xp.start, xp.fid, &xp.dst);
}

// ... and their unpack: per field and halo element, its column in the receive buffer (empty: none)
std::vector<int> rec_unpack_offsets(const XLayout& lay, int bi, Loc loc, int nsolve, int nh) {
  std::vector<int> off((size_t)(loc == L_CELL ? 3 : 1) * std::max(nh, 0), -1);
  bool any = false;
  for (const LSeg& s : lay.post) {
    if (s.block != bi || s.loc != loc) continue;
    for (int i = 0; i < s.list->n; ++i) {
      off[(size_t)lay.cls.fid[s.field] * nh + (s.list->h_idx[i] - nsolve)] = (int)(s.off + (int64_t)i * s.inner);
      any = true;
    }
  }
  if (!any) off.clear();
  return off;
}

// X_U: each received halo edge (off[i] >= 0) is written back by one vertex of the block that has it
// among its edgesOnVertex (the vertex kernel is its first reader).  False: an edge without one.
bool writeback_vertices(const Block& b, const std::vector<int>& off, std::vector<int>& wb) {
  const Dims& d = b.d;
  const int nsolve = d.nEdgesSolve, nh = d.nEdges - nsolve;
  wb.assign(std::max(nh, 0), -1);
  if ((int64_t)b.h_voe.size() < 2LL * d.nEdges || (int64_t)b.h_eov.size() < 3LL * d.nVertices) return false;
  for (int i = 0; i < nh; ++i) {
    if (off[i] < 0) continue;
    const int e = nsolve + i;
    for (int j = 0; j < 2 && wb[i] < 0; ++j) {
      const int v = b.h_voe[2 * (size_t)e + j];
      if (v < 0 || v >= d.nVertices) continue;
      for (int m = 0; m < 3; ++m)
        if (b.h_eov[3 * (size_t)v + m] == e) wb[i] = v;
    }
    if (wb[i] < 0) return false;
  }
  return true;
}

int fuse_rec(mpas_dyc_ctx* ctx, const XLayout& lay, XPlan& pl) {
  const int nb = (int)ctx->blk.size();
  if ((lay.pre.empty() && lay.post.empty()) || !ctx->fused_pack_enabled || !all_blocks(ctx, pair_layout))
    return MPAS_DYC_OK;
  auto nsolve_of = [](const Dims& d, Loc loc) { return loc == L_CELL ? d.nCellsSolve : d.nEdgesSolve; };
  auto nh_of = [&](const Dims& d, Loc loc) { return (loc == L_CELL ? d.nCells : d.nEdges) - nsolve_of(d, loc); };
  // before anything is uploaded: without a write-back vertex for every halo edge the pack and unpack
  // kernels run, and no map is built
  std::vector<std::vector<int>> wb(nb);
  if (lay.cls.kind == X_U)
    for (int bi = 0; bi < nb; ++bi) {
      const Dims& d = ctx->blk[bi].d;
      const std::vector<int> off = rec_unpack_offsets(lay, bi, L_EDGE, nsolve_of(d, L_EDGE), nh_of(d, L_EDGE));
      if (!off.empty() && !writeback_vertices(ctx->blk[bi], off, wb[bi])) return MPAS_DYC_OK;
    }
  pl.rpk_cell.assign(nb, XPack{});
  pl.rpk_edge.assign(nb, XPack{});
  pl.rup_cell.assign(nb, XUnpack{});
  pl.rup_edge.assign(nb, XUnpack{});
  for (int bi = 0; bi < nb; ++bi)
    for (const Loc loc : {L_CELL, L_EDGE}) {
      const Dims& d = ctx->blk[bi].d;
      const int nsolve = nsolve_of(d, loc), nh = nh_of(d, loc);
      CHK(rec_pack_map(ctx, lay, bi, loc, nsolve, pl, (loc == L_CELL ? pl.rpk_cell : pl.rpk_edge)[bi]));
      const std::vector<int> off = rec_unpack_offsets(lay, bi, loc, nsolve, nh);
      if (off.empty()) continue;
      const int *d_wb = nullptr, *d_off = nullptr;
      if (loc == L_EDGE && !wb[bi].empty()) CHK(plan_upload(ctx, pl, d_wb, wb[bi]));
      CHK(plan_upload(ctx, pl, d_off, off));
      (loc == L_CELL ? pl.rup_cell : pl.rup_edge)[bi] = XUnpack{pl.recvbuf, d_off, nh, d_wb};
    }
  pl.fused_rec = lay.cls.kind == X_RECOVERY ? 1 : lay.cls.kind == X_TEND_U ? 2 : 3;
  pl.fused_pack = pl.fused_unpack = true;
  return MPAS_DYC_OK;
}

// An exchange point, compiled.  The dry run (a host-only context) stops after the layout: it keeps
// the message lists only, and no pointer is formed from its fields' null buffers.
int build_plan(mpas_dyc_ctx* ctx, const std::vector<XField>& fs, XPlan& pl) {
  XLayout lay;
  CHK(plan_layout(ctx, fs, lay));
  pl.rsend = lay.rsend;
  pl.rrecv = lay.rrecv;
  pl.maxn_pre = lay.maxn_pre;
  pl.maxn_post = lay.maxn_post;
  if (ctx->host_only) return MPAS_DYC_OK;
  std::vector<XSeg> pre, post;
  CHK(plan_bind(ctx, fs, lay, pl, pre, post));
  if (pl.pull) return MPAS_DYC_OK;
  if (lay.cls.kind == X_SUBSTEP) CHK(fuse_substep(ctx, lay, fs.size() == 2, pl));
  else if (lay.cls.kind != X_NONE) CHK(fuse_rec(ctx, lay, pl));
  if (pl.npre) CHK(plan_upload(ctx, pl, pl.d_pre, pre));
  if (pl.npost) CHK(plan_upload(ctx, pl, pl.d_post, post));
  return MPAS_DYC_OK;
}

// ---- running an exchange ----
// a profile event pair's first half on `s` (the second is prof_mark_end); nothing unless profiling
int prof_mark(mpas_dyc_ctx* ctx, std::vector<hipEvent_t>& v, hipStream_t s) {
  if (!ctx->profile || ctx->planning) return MPAS_DYC_OK;
  hipEvent_t e = nullptr;
  HIPCHK(hipEventCreate(&e));
  HIPCHK(hipEventRecord(e, s));
  v.push_back(e);
  return MPAS_DYC_OK;
}

void set_last_key(mpas_dyc_ctx* ctx, const std::string& k) {
  const size_t n = std::min(k.size(), sizeof(ctx->last_key) - 1);
  memcpy(ctx->last_key, k.data(), n);
  ctx->last_key[n] = 0;
}

// The RCCL group of an exchange: one send and one receive per peer rank.  Loopback (timing
// emulation): each peer's pair goes to this rank itself; a send to self and the receive that
// matches it must have one size, so both move min(send, receive) doubles.
int rccl_group(mpas_dyc_ctx* ctx, const XPlan& pl) {
  NCCLCHK(ncclGroupStart());
  if (ctx->loopback) {
    // one self pair per peer rank of max(send, receive) doubles (a peer this rank only sends to or
    // only receives from gets one too); plan_bind sizes both buffers for it
    for (const auto& kv : loopback_pairs(pl)) {
      const XMsg *sm = kv.second.first, *rm = kv.second.second;
      const size_t n = (size_t)std::max(sm ? sm->count : 0, rm ? rm->count : 0);
      if (ctx->loopback == 2) {
        HIPCHK(hipMemcpyAsync(pl.recvbuf + (rm ? rm->off : 0), pl.sendbuf + (sm ? sm->off : 0), n * sizeof(double),
                              hipMemcpyDeviceToDevice, ctx->stream));
        continue;
      }
      NCCLCHK(ncclSend(pl.sendbuf + (sm ? sm->off : 0), n, ncclFloat64, ctx->rank, ctx->comm, ctx->stream));
      NCCLCHK(ncclRecv(pl.recvbuf + (rm ? rm->off : 0), n, ncclFloat64, ctx->rank, ctx->comm, ctx->stream));
    }
  } else {
    for (const XMsg& m : pl.rsend)
      NCCLCHK(ncclSend(pl.sendbuf + m.off, (size_t)m.count, ncclFloat64, m.peer_rank, ctx->comm, ctx->stream));
    for (const XMsg& m : pl.rrecv)
      NCCLCHK(ncclRecv(pl.recvbuf + m.off, (size_t)m.count, ncclFloat64, m.peer_rank, ctx->comm, ctx->stream));
  }
  NCCLCHK(ncclGroupEnd());
  return MPAS_DYC_OK;
}

// one-sided transfer (MPAS_DYCORE_P2P, halo.hip): p2p_setup, p2p_fallback, p2p_teardown, p2p_check
#include "p2p_setup.hip"

// the pack, unpack or in-process copy launch: one workgroup per 4 elements of each segment
void launch_copy(mpas_dyc_ctx* ctx, const XSeg* segs, int nseg, int maxn) {
  if (nseg) hipLaunchKernelGGL(k_halo_copy, dim3((maxn + 3) / 4, nseg), dim3(256), 0, ctx->stream, segs);
}
void launch_pack(mpas_dyc_ctx* ctx, const XPlan& pl) {
  if (!pl.fused_pack) launch_copy(ctx, pl.d_pre, pl.npre, pl.maxn_pre);
}
void launch_unpack(mpas_dyc_ctx* ctx, const XPlan& pl) {
  if (!pl.fused_unpack) launch_copy(ctx, pl.d_post, pl.npost, pl.maxn_post);
}

// The one-sided paths of exchange() (pl.p2p, set up).  part: 0 the whole exchange, 1 pack and post
// (exchange_async), 2 get and unpack (exchange_wait), all on the compute stream.
int exchange_p2p(mpas_dyc_ctx* ctx, const XPlan& pl, const std::string& key, int part) {
  if (pl.pull) {  // blocking only (plan_bind): the whole exchange at the first call
    if (part == 2) return MPAS_DYC_OK;
    CHK(prof_mark(ctx, ctx->prof_exposed, ctx->stream));
    launch_copy(ctx, pl.d_local, pl.nlocal, pl.maxn_local);
    set_last_key(ctx, key);
    CHK(prof_mark(ctx, ctx->prof_rccl, ctx->stream));
    hipLaunchKernelGGL(k_p2p_pull, dim3(pl.nchunk + 1), dim3(256), 0, ctx->stream, (const P2PSeg*)pl.d_pseg,
                       (const int2*)pl.d_chunk, pl.nchunk, (const P2PPeer*)pl.d_peer, pl.npeer_work,
                       (unsigned long long* const*)pl.d_ready, pl.nready, (const unsigned long long* const*)pl.d_cons,
                       pl.ncons, pl.p2p_cnt, ctx->p2p_status, ctx->p2p_release);
    CHK(prof_mark(ctx, ctx->prof_rccl, ctx->stream));
    CHK(prof_mark(ctx, ctx->prof_exposed, ctx->stream));
    return MPAS_DYC_OK;
  }
  if (part == 0 && !ctx->p2p_merge) {  // the two launches (A/B of the merged one)
    CHK(exchange_p2p(ctx, pl, key, 1));
    return exchange_p2p(ctx, pl, key, 2);
  }
  if (part == 0) {  // blocking: post and get as one launch (k_p2p_exchange)
    CHK(prof_mark(ctx, ctx->prof_exposed, ctx->stream));
    launch_pack(ctx, pl);
    set_last_key(ctx, key);
    CHK(prof_mark(ctx, ctx->prof_rccl, ctx->stream));
    hipLaunchKernelGGL(k_p2p_exchange, dim3(std::max(pl.get_chunks, 1), pl.nget + 1), dim3(256), 0, ctx->stream,
                       (const P2PGet*)pl.d_get, pl.nget, (unsigned long long* const*)pl.d_ready, pl.nready,
                       (const unsigned long long* const*)pl.d_cons, pl.ncons, pl.p2p_cnt, ctx->p2p_status,
                       ctx->p2p_release);
    CHK(prof_mark(ctx, ctx->prof_rccl, ctx->stream));
    launch_unpack(ctx, pl);
    CHK(prof_mark(ctx, ctx->prof_exposed, ctx->stream));
    return MPAS_DYC_OK;
  }
  if (part == 1) {
    launch_pack(ctx, pl);
    set_last_key(ctx, key);
    hipLaunchKernelGGL(k_p2p_post, dim3(1), dim3(64), 0, ctx->stream, pl.p2p_cnt, pl.d_ready, pl.nready,
                       ctx->p2p_release);
    return MPAS_DYC_OK;
  }
  // part 2
  CHK(prof_mark(ctx, ctx->prof_rccl, ctx->stream));
  hipLaunchKernelGGL(k_p2p_get, dim3(std::max(pl.get_chunks, 1), pl.nget + 1), dim3(256), 0, ctx->stream,
                     (const P2PGet*)pl.d_get, pl.nget, (const unsigned long long* const*)pl.d_cons, pl.ncons,
                     (const unsigned long long*)pl.p2p_cnt, ctx->p2p_status);
  CHK(prof_mark(ctx, ctx->prof_rccl, ctx->stream));
  launch_unpack(ctx, pl);
  return MPAS_DYC_OK;
}

// part: 0 the whole exchange; with one-sided transfer a split-phase exchange runs as 1 (pack and
// post, at exchange_async) and 2 (get and unpack, at exchange_wait), all on the compute stream
int exchange(mpas_dyc_ctx* ctx, const std::vector<XField>& fs, int part = 0) {
  if (!needs_exchange(ctx)) return MPAS_DYC_OK;
  const std::string key = plan_key(ctx, fs);
  if (ctx->record) ctx->record->push_back(key);
  auto it = ctx->plans.find(key);
  if (it == ctx->plans.end()) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (!ctx->host_only) (void)hipStreamIsCapturing(ctx->stream, &cs);
    if (cs != hipStreamCaptureStatusNone) {
      ctx->err = "internal: exchange plan missing during graph capture";
      return MPAS_DYC_ESTATE;
    }
    XPlan pl;
    int r = build_plan(ctx, fs, pl);
    if (r) {
      free_plan(pl);
      return r;
    }
    it = ctx->plans.emplace(key, std::move(pl)).first;
  }
  if (ctx->planning) return MPAS_DYC_OK;
  XPlan& pl = it->second;
  if (pl.p2p) {
    if (pl.p2p_id < 0) {  // built outside plan_all (mpas_dyc_halo_exchange): every rank is here too
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      (void)hipStreamIsCapturing(ctx->stream, &cs);
      if (cs != hipStreamCaptureStatusNone) {
        ctx->err = "internal: one-sided exchange set up during graph capture";
        return MPAS_DYC_ESTATE;
      }
      const int r = p2p_setup(ctx);
      if (r == P2P_UNAVAILABLE) {  // every rank is here: this exchange, and the rest, through RCCL
        if (!ctx->comm) return MPAS_DYC_ECOMM;
        p2p_fallback(ctx);
        return exchange(ctx, fs, part);
      }
      CHK(r);
    }
    return exchange_p2p(ctx, pl, key, part);
  }
  if (part == 2) return MPAS_DYC_OK;  // in-process copies only: done at part 1
  const bool whole = !ctx->in_async;  // a blocking exchange: all of it is exposed
  if (whole) CHK(prof_mark(ctx, ctx->prof_exposed, ctx->stream));
  launch_pack(ctx, pl);
  if (!pl.rsend.empty() || !pl.rrecv.empty()) {
    set_last_key(ctx, key);
    CHK(prof_mark(ctx, ctx->prof_rccl, ctx->stream));
    CHK(rccl_group(ctx, pl));
    CHK(prof_mark(ctx, ctx->prof_rccl, ctx->stream));
  }
  launch_unpack(ctx, pl);
  if (whole) CHK(prof_mark(ctx, ctx->prof_exposed, ctx->stream));
  return MPAS_DYC_OK;
}

// The plan of an exchange whose pack the producing kernel does (XPlan::fused_pack), or nullptr
const XPlan* fused_pack_plan(mpas_dyc_ctx* ctx, const std::vector<XField>& fs) {
  if (ctx->planning || !needs_exchange(ctx)) return nullptr;
  auto it = ctx->plans.find(plan_key(ctx, fs));
  if (it == ctx->plans.end() || !it->second.fused_pack || it->second.pack.size() != ctx->blk.size()) return nullptr;
  return &it->second;
}

// The plan of the 876-887 or 642 exchange when its pack and unpack are fused (XPlan::fused_rec), or
// nullptr
const XPlan* fused_rec_plan(mpas_dyc_ctx* ctx, const std::vector<XField>& fs) {
  if (ctx->planning || !needs_exchange(ctx)) return nullptr;
  auto it = ctx->plans.find(plan_key(ctx, fs));
  if (it == ctx->plans.end() || !it->second.fused_rec || it->second.rpk_cell.size() != ctx->blk.size()) return nullptr;
  return &it->second;
}

// First half of a split-phase exchange: after everything queued on the compute stream,
// the exchange stream packs, talks RCCL and unpacks; exchange_wait joins it back.
int issue_async(mpas_dyc_ctx* ctx, const std::vector<XField>& fs) {
  HIPCHK(hipStreamWaitEvent(ctx->xstream, ctx->xfork, 0));
  hipStream_t s = ctx->stream;
  ctx->stream = ctx->xstream;  // exchange() issues on ctx->stream
  ctx->in_async = true;
  const int r = exchange(ctx, fs);
  ctx->in_async = false;
  ctx->stream = s;
  if (r) return r;
  HIPCHK(hipEventRecord(ctx->xjoin, ctx->xstream));
  return MPAS_DYC_OK;
}

int exchange_async(mpas_dyc_ctx* ctx, const std::vector<XField>& fs) {
  if (ctx->planning) return exchange(ctx, fs);
  if (ctx->p2p) {  // no second stream: pack and post now, the get at exchange_wait
    ctx->p2p_open = fs;
    ctx->p2p_pending = true;
    return exchange(ctx, fs, 1);
  }
  HIPCHK(hipEventRecord(ctx->xfork, ctx->stream));
  if (ctx->late_issue) {
    ctx->late_fs = fs;
    ctx->late_pending = true;
    return MPAS_DYC_OK;
  }
  return issue_async(ctx, fs);
}

int exchange_wait(mpas_dyc_ctx* ctx) {
  if (ctx->planning) return MPAS_DYC_OK;
  if (ctx->p2p_pending) {
    ctx->p2p_pending = false;
    CHK(prof_mark(ctx, ctx->prof_exposed, ctx->stream));
    CHK(exchange(ctx, ctx->p2p_open, 2));
    CHK(prof_mark(ctx, ctx->prof_exposed, ctx->stream));
    return MPAS_DYC_OK;
  }
  if (ctx->late_pending) {
    ctx->late_pending = false;
    CHK(issue_async(ctx, ctx->late_fs));
  }
  CHK(prof_mark(ctx, ctx->prof_exposed, ctx->stream));  // the compute stream's work before the join
  HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->xjoin, 0));
  CHK(prof_mark(ctx, ctx->prof_exposed, ctx->stream));  // ... completes once the join has
  return MPAS_DYC_OK;
}

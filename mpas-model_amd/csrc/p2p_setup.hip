// One-sided halo transfer (MPAS_DYCORE_P2P, kernels in halo.hip): its set-up and its teardown.
// Collective, outside graph capture.  Included by dycore.hip inside its namespace (it needs
// mpas_dyc_ctx and XPlan).  The records the ranks all-gather are p2p_wire.h's; what the context
// owns for the transfer is the "one-sided transfer: owned" section of mpas_dyc_ctx, released by
// p2p_teardown; what an exchange point owns is XPlan::owned / XPlan::mapped, released by free_plan.
constexpr int P2P_MAX_POINTS = 4096;  // exchange points per context (a run builds ~60)

// nbytes from every rank, in rank order, over the library's communicator
int allgather_bytes(mpas_dyc_ctx* ctx, const void* mine, size_t nbytes, std::vector<char>& all) {
  all.assign(nbytes * ctx->nranks, 0);
  if (ctx->nranks == 1) {
    memcpy(all.data(), mine, nbytes);
    return MPAS_DYC_OK;
  }
  if (ctx->host_allgather) {  // the host's collective, even beside an RCCL communicator (kept for fallback)
    if (ctx->host_allgather(mine, all.data(), (int64_t)nbytes, ctx->host_user) != 0) {
      ctx->err = "the host's all-gather (mpas_dyc_comm_init_host) failed";
      return MPAS_DYC_ECOMM;
    }
    return MPAS_DYC_OK;
  }
  char* d = nullptr;
  HIPCHK(hipMalloc(&d, nbytes * (ctx->nranks + 1)));
  const int r = [&]() -> int {
    HIPCHK(hipMemcpy(d, mine, nbytes, hipMemcpyHostToDevice));
    NCCLCHK(ncclAllGather(d, d + nbytes, nbytes, ncclUint8, ctx->comm, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(all.data(), d + nbytes, nbytes * ctx->nranks, hipMemcpyDeviceToHost));
    return MPAS_DYC_OK;
  }();
  (void)hipFree(d);
  return r;
}

// variable-size all-gather: every rank's bytes, in rank order
int allgatherv_bytes(mpas_dyc_ctx* ctx, const std::vector<char>& mine, std::vector<std::vector<char>>& out) {
  int64_t n = (int64_t)mine.size();
  std::vector<char> sizes;
  CHK(allgather_bytes(ctx, &n, sizeof(n), sizes));
  int64_t mx = 0;
  for (int r = 0; r < ctx->nranks; ++r) mx = std::max(mx, ((const int64_t*)sizes.data())[r]);
  std::vector<char> pad(mine);
  pad.resize(std::max<int64_t>(mx, 1), 0);
  std::vector<char> all;
  CHK(allgather_bytes(ctx, pad.data(), pad.size(), all));
  out.assign(ctx->nranks, {});
  for (int r = 0; r < ctx->nranks; ++r) {
    const char* b = all.data() + (size_t)r * pad.size();
    out[r].assign(b, b + ((const int64_t*)sizes.data())[r]);
  }
  return MPAS_DYC_OK;
}

// the node a rank runs on: IPC mappings exist only between processes of one node
uint64_t node_id() {
  char buf[512] = {0};
  (void)gethostname(buf, 255);
  if (FILE* f = fopen("/proc/sys/kernel/random/boot_id", "r")) {
    const size_t n = strlen(buf);
    if (!fgets(buf + n, (int)(sizeof(buf) - n - 1), f)) buf[n] = 0;
    fclose(f);
  }
  uint64_t h = 1469598103934665603ull;
  for (const char* c = buf; *c; ++c) h = (h ^ (unsigned char)*c) * 1099511628211ull;
  return h;
}

// p2p_init / p2p_setup return this when the one-sided transfer cannot run on some rank (IPC
// unsupported, ranks on several nodes, a mapping refused): every rank learns it from the same
// all-gathers, drops the transfer and plans again with RCCL (plan_all, p2p_fallback)
constexpr int P2P_UNAVAILABLE = 1;

// every rank's verdict on a local step of the set-up (collective): P2P_UNAVAILABLE on all ranks if
// any rank failed, with the first failing rank's reason in ctx->err.  One rank: its own verdict.
int p2p_vote(mpas_dyc_ctx* ctx, int local, const std::string& what) {
  if (ctx->nranks == 1) return local;
  int32_t mine = local == MPAS_DYC_OK ? 0 : 1;
  std::vector<char> all;
  CHK(allgather_bytes(ctx, &mine, sizeof(mine), all));
  for (int r = 0; r < ctx->nranks; ++r)
    if (((const int32_t*)all.data())[r]) {
      ctx->err = "one-sided transfer unavailable (" + what + " failed on rank " + std::to_string(r) +
                 (r == ctx->rank ? ": " + ctx->err : std::string()) + ")";
      return P2P_UNAVAILABLE;
    }
  return MPAS_DYC_OK;
}

// device memory of this rank as the handle its peers open (zeros with one rank: nobody opens it),
// and a peer's handle mapped here; whoever keeps the mapping closes it (free_plan, p2p_teardown)
static_assert(sizeof(hipIpcMemHandle_t) == sizeof(p2p_wire::Handle), "p2p_wire::Handle carries a hipIpcMemHandle_t");
int p2p_export(mpas_dyc_ctx* ctx, const void* dptr, p2p_wire::Handle& out) {
  hipIpcMemHandle_t h{};
  if (ctx->nranks > 1) HIPCHK(hipIpcGetMemHandle(&h, (void*)dptr));
  memcpy(&out, &h, sizeof(h));
  return MPAS_DYC_OK;
}
template <class T>
int p2p_open(mpas_dyc_ctx* ctx, const p2p_wire::Handle& in, T*& mapped) {  // mapped: set on success only
  hipIpcMemHandle_t h;
  void* p = nullptr;
  memcpy(&h, &in, sizeof(h));
  HIPCHK(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
  mapped = (T*)p;
  return MPAS_DYC_OK;
}

// the flag arenas: this rank's, and every peer's mapped here
int p2p_init(mpas_dyc_ctx* ctx) {
  if (ctx->p2p_flags) return MPAS_DYC_OK;
  if (!ctx->comm && !ctx->host_allgather) {
    ctx->err = "MPAS_DYCORE_P2P: no communicator for the set-up (mpas_dyc_comm_init / _comm_init_host)";
    return MPAS_DYC_ECOMM;
  }
  int nr = ctx->nranks;
  if (ctx->loopback)  // the emulated peers are ranks the lists name, beyond this one-rank communicator
    for (const auto& b : ctx->blk)
      for (const auto& x : b.xl) nr = std::max(nr, x.peer_rank + 1);
  ctx->p2p_nr = nr;
  struct Rec {
    p2p_wire::Handle h;
    uint64_t node;
  } rec{};
  const int local = [&]() -> int {
    const size_t bytes = (size_t)P2P_MAX_POINTS * nr * 2 * sizeof(unsigned long long);
    HIPCHK(hipExtMallocWithFlags((void**)&ctx->p2p_flags, bytes, hipDeviceMallocUncached));
    HIPCHK(hipMemset(ctx->p2p_flags, 0, bytes));
    HIPCHK(hipMalloc(&ctx->p2p_status, sizeof(int)));
    HIPCHK(hipMemset(ctx->p2p_status, 0, sizeof(int)));
    HIPCHK(hipHostMalloc((void**)&ctx->p2p_status_host, sizeof(int), hipHostMallocDefault));
    *ctx->p2p_status_host = 0;
    HIPCHK(hipDeviceSynchronize());
    return p2p_export(ctx, ctx->p2p_flags, rec.h);
  }();
  ctx->p2p_peer_flags.assign(ctx->nranks, nullptr);
  ctx->p2p_peer_flags[ctx->rank] = ctx->p2p_flags;
  if (ctx->nranks == 1) return local;
  CHK(p2p_vote(ctx, local, "flag arena allocation"));
  rec.node = node_id();
  std::vector<char> all;
  CHK(allgather_bytes(ctx, &rec, sizeof(rec), all));
  for (int r = 0; r < ctx->nranks; ++r)
    if (((const Rec*)all.data())[r].node != rec.node) {
      ctx->err = "one-sided transfer unavailable (rank " + std::to_string(r) + " runs on another node)";
      return P2P_UNAVAILABLE;
    }
  const int opened = [&]() -> int {
    for (int r = 0; r < ctx->nranks; ++r)  // closed by p2p_teardown
      if (r != ctx->rank) CHK(p2p_open(ctx, ((const Rec*)all.data())[r].h, ctx->p2p_peer_flags[r]));
    return MPAS_DYC_OK;
  }();
  return p2p_vote(ctx, opened, "mapping the peers' flag arenas");
}

// Releases what the context owns for the transfer (mpas_dyc_ctx, "one-sided transfer: owned"); the
// one place where the peers' arenas and fields mapped here are closed.  Callers free the plans first
// (invalidate_plans: each plan closes its own mappings of the peers' send buffers), and
// mpas_dyc_destroy frees this rank's field buffers between the two.  So the order of release is:
// plans, field buffers, then here the peers' mappings, the arena, the status word.  Nothing here
// waits for the peers: whether a peer may still map or read what is freed is not decided here.
void p2p_teardown(mpas_dyc_ctx* ctx) {
  for (int r = 0; r < (int)ctx->p2p_peer_flags.size(); ++r)
    if (r != ctx->rank && ctx->p2p_peer_flags[r]) (void)hipIpcCloseMemHandle(ctx->p2p_peer_flags[r]);
  for (auto& kv : ctx->p2p_fields) (void)hipIpcCloseMemHandle(kv.second);
  if (ctx->p2p_flags) (void)hipFree(ctx->p2p_flags);
  if (ctx->p2p_status) (void)hipFree(ctx->p2p_status);
  if (ctx->p2p_status_host) (void)hipHostFree(ctx->p2p_status_host);
  ctx->p2p_peer_flags.clear();
  ctx->p2p_fields.clear();
  ctx->p2p_flags = nullptr;
  ctx->p2p_status = ctx->p2p_status_host = nullptr;
}

// ---- what both kinds of exchange point (buffers, pull) do ----

// the next flag slot of the context, for exchange point `pl`
int p2p_take_slot(mpas_dyc_ctx* ctx, XPlan& pl) {
  if (ctx->p2p_next >= P2P_MAX_POINTS) {
    ctx->err = "MPAS_DYCORE_P2P: more than " + std::to_string(P2P_MAX_POINTS) + " exchange points";
    return MPAS_DYC_ESTATE;
  }
  pl.p2p_id = ctx->p2p_next++;
  return MPAS_DYC_OK;
}

// the flag rank `r` raises at exchange point `pl` in `arena` (this rank's or a peer's mapped here):
// k = 0 ready, 1 consumed
unsigned long long* p2p_flag(const mpas_dyc_ctx* ctx, const XPlan& pl, unsigned long long* arena, int r, int k) {
  return arena + ((size_t)pl.p2p_id * ctx->p2p_nr + r) * 2 + k;
}

// the segments (indices into `off`, the segments' offsets in the send or receive buffer) that lie in
// message m, in buffer order: sender and receiver pair their segments of a message in this order
std::vector<size_t> segs_of(const std::vector<int64_t>& off, const XMsg& m) {
  std::vector<size_t> segs;
  for (size_t i = 0; i < off.size(); ++i)
    if (off[i] >= m.off && off[i] < m.off + m.count) segs.push_back(i);
  std::sort(segs.begin(), segs.end(), [&](size_t a, size_t b) { return off[a] < off[b]; });
  return segs;
}

// An exchange point's counters (ncnt, zeroed: [0] uses, the rest its kernel's) and flag lists: the
// ready flags this rank raises, in the arena of every rank it sends to, and the consumed flags it
// waits for in its own.  Loopback: both in its own arena, for the emulated peers given.
int p2p_flags_and_counters(mpas_dyc_ctx* ctx, XPlan& pl, size_t ncnt, const std::vector<int>& loop_ready,
                           const std::vector<int>& loop_cons) {
  std::vector<unsigned long long*> ready;
  std::vector<const unsigned long long*> cons;
  if (ctx->loopback) {
    for (int q : loop_ready) ready.push_back(p2p_flag(ctx, pl, ctx->p2p_flags, q, 0));
    for (int q : loop_cons) cons.push_back(p2p_flag(ctx, pl, ctx->p2p_flags, q, 1));
  } else
    for (const XMsg& m : pl.rsend) {
      ready.push_back(p2p_flag(ctx, pl, ctx->p2p_peer_flags[m.peer_rank], ctx->rank, 0));
      cons.push_back(p2p_flag(ctx, pl, ctx->p2p_flags, m.peer_rank, 1));
    }
  if (cons.size() > 256 || ready.size() > 256) {
    ctx->err = "MPAS_DYCORE_P2P: more than 256 peers";
    return MPAS_DYC_EINVAL;
  }
  CHK(plan_alloc(ctx, pl, pl.p2p_cnt, ncnt * sizeof(unsigned long long)));
  HIPCHK(hipMemset(pl.p2p_cnt, 0, ncnt * sizeof(unsigned long long)));
  pl.nready = (int)ready.size();
  pl.ncons = (int)cons.size();
  CHK(plan_upload(ctx, pl, pl.d_ready, ready.data(), ready.size() * sizeof(void*)));
  return plan_upload(ctx, pl, pl.d_cons, cons.data(), cons.size() * sizeof(void*));
}

// All-gathers one record per rank and decodes them all before anything is built from them: every
// rank decodes every rank's record, so a malformed one fails on all ranks alike.  `bytes` backs the
// decoded records (the send lists point into it).
template <class Rec>
int p2p_gather_records(mpas_dyc_ctx* ctx, const Rec& mine, size_t npoints, const char* kind,
                       std::vector<std::vector<char>>& bytes, std::vector<Rec>& recs) {
  CHK(allgatherv_bytes(ctx, mine.encode(), bytes));
  recs.resize(ctx->nranks);
  for (int r = 0; r < ctx->nranks; ++r)
    if (!Rec::decode(bytes[r].data(), bytes[r].size(), recs[r]) || !recs[r].fits(npoints, ctx->nranks)) {
      ctx->err = "MPAS_DYCORE_P2P: rank " + std::to_string(r) + "'s " + kind + " record ends early (its exchange "
                 "points or messages differ from rank " + std::to_string(ctx->rank) + "'s)";
      return MPAS_DYC_ECOMM;
    }
  return MPAS_DYC_OK;
}

// ---- buffer plans: the receiver's kernel copies each message out of the sender's send buffer ----
int p2p_setup_buffers(mpas_dyc_ctx* ctx, const std::vector<XPlan*>& todo) {
  const int nr = ctx->nranks, me = ctx->rank;
  if (todo.empty()) return MPAS_DYC_OK;
  p2p_wire::BufRecord mine;
  const int exported = [&]() -> int {
    for (const XPlan* pl : todo) {
      p2p_wire::BufPoint pt;
      CHK(p2p_export(ctx, pl->sendbuf, pt.h));
      pt.to.assign(nr, {-1, -1});
      for (const XMsg& m : pl->rsend)
        if (m.peer_rank < nr) pt.to[m.peer_rank] = {m.off, m.count};  // loopback: emulated ranks lie beyond
      mine.points.push_back(std::move(pt));
    }
    return MPAS_DYC_OK;
  }();
  CHK(p2p_vote(ctx, exported, "exporting the send buffers"));
  std::vector<std::vector<char>> bytes;
  std::vector<p2p_wire::BufRecord> recs;
  CHK(p2p_gather_records(ctx, mine, todo.size(), "buffer", bytes, recs));
  const int built = [&]() -> int {
    for (size_t i = 0; i < todo.size(); ++i) {
      XPlan& pl = *todo[i];
      CHK(p2p_take_slot(ctx, pl));
      auto nchunk = [](int64_t n) { return (int)std::max<int64_t>(1, (n + P2P_CHUNK - 1) / P2P_CHUNK); };
      std::vector<P2PGet> gets;
      std::vector<int> loop_peers;
      if (ctx->loopback) {
        // as rccl_group: one pair per emulated peer of max(send, receive) doubles, all in this rank
        for (const auto& kv : loopback_pairs(pl)) {
          const XMsg *sm = kv.second.first, *rm = kv.second.second;
          const int64_t n = std::max(sm ? sm->count : 0, rm ? rm->count : 0);
          gets.push_back(P2PGet{pl.sendbuf + (sm ? sm->off : 0), pl.recvbuf + (rm ? rm->off : 0), n,
                                p2p_flag(ctx, pl, ctx->p2p_flags, kv.first, 0),
                                p2p_flag(ctx, pl, ctx->p2p_flags, kv.first, 1), nullptr, nchunk(n)});
          loop_peers.push_back(kv.first);
        }
      } else {
        for (const XMsg& m : pl.rrecv) {
          const p2p_wire::BufPoint& pt = recs[m.peer_rank].points[i];
          const int64_t off = pt.to[me].first, count = pt.to[me].second;
          if (count != m.count) {
            ctx->err = "MPAS_DYCORE_P2P: rank " + std::to_string(m.peer_rank) + " sends " + std::to_string(count) +
                       " doubles where this rank receives " + std::to_string(m.count);
            return MPAS_DYC_ECOMM;
          }
          const double* base = pl.sendbuf;
          if (m.peer_rank != me) {
            CHK(p2p_open(ctx, pt.h, base));
            pl.mapped.push_back((void*)base);
          }
          gets.push_back(P2PGet{base + off, pl.recvbuf + m.off, m.count, p2p_flag(ctx, pl, ctx->p2p_flags, m.peer_rank, 0),
                                p2p_flag(ctx, pl, ctx->p2p_peer_flags[m.peer_rank], me, 1), nullptr, nchunk(m.count)});
        }
      }
      // [0] uses, [1 + i] chunks pulled from get peer i, [1 + nget] finished workgroups of k_p2p_exchange
      CHK(p2p_flags_and_counters(ctx, pl, 2 + gets.size(), loop_peers, loop_peers));
      for (size_t j = 0; j < gets.size(); ++j) {
        gets[j].done = pl.p2p_cnt + 1 + j;
        pl.get_chunks = std::max(pl.get_chunks, gets[j].nchunk);
      }
      pl.nget = (int)gets.size();
      CHK(plan_upload(ctx, pl, pl.d_get, gets.data(), gets.size() * sizeof(P2PGet)));
    }
    return MPAS_DYC_OK;
  }();
  return p2p_vote(ctx, built, "mapping the peers' send buffers");
}

// ---- pull plans: the receiver's kernel copies the peers' owned columns out of their fields ----

// the field buffer (with its 256 B of slack) that p lies in
const double* field_buffer_of(const mpas_dyc_ctx* ctx, const double* p) {
  for (const auto& b : ctx->blk)
    for (const auto& f : b.fields)
      for (int t = 0; t < f.ntl; ++t) {
        const char* q = (const char*)f.buf[t];
        if (!q || f.is_int) continue;
        if ((const char*)p >= q && (const char*)p < q + (size_t)field_bytes(b, f) + 256) return (const double*)q;
      }
  return nullptr;
}

// rank r's field buffer `b` mapped here: each buffer is opened once per context and stays open
// until p2p_teardown
int p2p_map_field(mpas_dyc_ctx* ctx, int r, const p2p_wire::PullBuf& b, const double*& out) {
  if (r == ctx->rank) {
    out = (const double*)(uintptr_t)b.addr;
    return MPAS_DYC_OK;
  }
  auto it = ctx->p2p_fields.find({r, b.addr});
  if (it == ctx->p2p_fields.end()) {
    void* p = nullptr;
    CHK(p2p_open(ctx, b.h, p));
    it = ctx->p2p_fields.emplace(std::make_pair(r, b.addr), p).first;
  }
  out = (const double*)it->second;
  return MPAS_DYC_OK;
}

// Every rank exports, per exchange point and message, its pack segments (the field buffer -- IPC
// handle, mapped once per peer and buffer -- the sub-field offset, the send list); the receiver
// pairs them in buffer order with its unpack segments into k_p2p_pull's segments.
int p2p_setup_pull(mpas_dyc_ctx* ctx, const std::vector<XPlan*>& todo) {
  const int me = ctx->rank;
  if (todo.empty()) return MPAS_DYC_OK;
  p2p_wire::PullRecord mine;
  const int exported = [&]() -> int {
    std::map<const double*, int32_t> buf_id;
    for (const XPlan* pl : todo) {
      mine.points.emplace_back();
      for (const XMsg& m : pl->rsend) {
        p2p_wire::PullMsg msg{m.peer_rank, {}};
        for (size_t i : segs_of(pl->h_pre_off, m)) {
          const XSeg& sg = pl->h_pre[i];
          const double* b = field_buffer_of(ctx, sg.src);
          if (!b) {
            ctx->err = "internal: pack segment outside every field";
            return MPAS_DYC_ESTATE;
          }
          auto it = buf_id.find(b);
          if (it == buf_id.end()) {
            p2p_wire::PullBuf pb{(uint64_t)(uintptr_t)b, {}};
            CHK(p2p_export(ctx, b, pb.h));
            it = buf_id.emplace(b, (int32_t)mine.bufs.size()).first;
            mine.bufs.push_back(pb);
          }
          msg.segs.push_back(p2p_wire::PullSeg{it->second, (int64_t)((const char*)sg.src - (const char*)b), sg.n,
                                               sg.inner, pl->h_pre_idx[i]->data()});
        }
        mine.points.back().push_back(std::move(msg));
      }
    }
    return MPAS_DYC_OK;
  }();
  CHK(p2p_vote(ctx, exported, "exporting the field buffers"));
  std::vector<std::vector<char>> bytes;
  std::vector<p2p_wire::PullRecord> recs;
  CHK(p2p_gather_records(ctx, mine, todo.size(), "pull", bytes, recs));
  const int built = [&]() -> int {
    for (size_t ip = 0; ip < todo.size(); ++ip) {
      XPlan& pl = *todo[ip];
      CHK(p2p_take_slot(ctx, pl));
      std::vector<P2PSeg> segs;
      std::vector<P2PPeer> peers;  // the ranks this one reads from (loopback: every emulated peer)
      std::vector<int> peer_rank;
      auto peer_of = [&](int src) -> int {
        const auto it = std::find(peer_rank.begin(), peer_rank.end(), src);
        if (it != peer_rank.end()) return (int)(it - peer_rank.begin());
        const bool here = ctx->loopback || src == me;
        peers.push_back(P2PPeer{p2p_flag(ctx, pl, ctx->p2p_flags, src, 0),
                                p2p_flag(ctx, pl, here ? ctx->p2p_flags : ctx->p2p_peer_flags[src], here ? src : me, 1),
                                nullptr, 0});
        peer_rank.push_back(src);
        return (int)peers.size() - 1;
      };
      for (const XMsg& m : pl.rrecv) {
        const std::vector<size_t> mine_post = segs_of(pl.h_post_off, m);
        const int src = m.peer_rank;
        const int ix = peer_of(src);
        if (ctx->loopback) {
          // timing only: the peer's segments are this rank's own pack segments to that peer
          std::vector<size_t> theirs;
          for (const XMsg& sm : pl.rsend)
            if (sm.peer_rank == src) theirs = segs_of(pl.h_pre_off, sm);  // one message per rank (merge_by_rank)
          for (size_t k = 0; k < std::min(theirs.size(), mine_post.size()); ++k) {
            const XSeg &a = pl.h_pre[theirs[k]], &b = pl.h_post[mine_post[k]];
            segs.push_back(P2PSeg{a.src, b.dst, a.sidx, b.didx, std::min(a.n, b.n), std::min(a.inner, b.inner), ix});
          }
          continue;
        }
        const p2p_wire::PullMsg* from = nullptr;  // src's message to this rank
        for (const p2p_wire::PullMsg& pm : recs[src].points[ip])
          if (pm.dest == me && !from) from = &pm;
        if (!from || from->segs.size() != mine_post.size()) {
          ctx->err = "MPAS_DYCORE_P2P: rank " + std::to_string(src) + "'s message to rank " + std::to_string(me) +
                     " does not match this rank's receive lists";
          return MPAS_DYC_ECOMM;
        }
        for (size_t k = 0; k < mine_post.size(); ++k) {
          const p2p_wire::PullSeg& a = from->segs[k];
          const XSeg& b = pl.h_post[mine_post[k]];
          if (a.n != b.n || a.inner != b.inner) {
            ctx->err = "MPAS_DYCORE_P2P: rank " + std::to_string(src) + " sends " + std::to_string(a.n) +
                       " elements where rank " + std::to_string(me) + " receives " + std::to_string(b.n);
            return MPAS_DYC_ECOMM;
          }
          if (pl.skip_pull) {  // each halo column onto itself: the protocol runs, the halo stays stale
            segs.push_back(P2PSeg{b.dst, b.dst, b.didx, b.didx, a.n, a.inner, ix});
            continue;
          }
          const double* base = nullptr;
          CHK(p2p_map_field(ctx, src, recs[src].bufs[a.buf], base));
          const int* sidx = nullptr;  // the peer's send list, copied to this device
          CHK(plan_upload(ctx, pl, sidx, a.idx, sizeof(int32_t) * (size_t)a.n));
          segs.push_back(P2PSeg{(const double*)((const char*)base + a.off), b.dst, sidx, b.didx, a.n, a.inner, ix});
        }
      }
      if (ctx->loopback)
        for (const XMsg& m : pl.rsend) (void)peer_of(m.peer_rank);
      std::vector<int2> chunks;
      for (size_t k = 0; k < segs.size(); ++k)
        for (int c = 0; c < segs[k].n; c += P2P_PULL_COLS) {
          chunks.push_back(make_int2((int)k, c));
          peers[segs[k].peer].nwg += 1;
        }
      pl.nchunk = (int)chunks.size();
      pl.npeer_work = 0;
      for (const P2PPeer& pr : peers) pl.npeer_work += pr.nwg ? 1 : 0;
      // loopback: ready to every emulated peer, in rank order; its emulated readers are the peers with
      // segments here
      std::vector<int> loop_ready(peer_rank), loop_cons;
      std::sort(loop_ready.begin(), loop_ready.end());
      for (size_t j = 0; j < peers.size(); ++j)
        if (peers[j].nwg) loop_cons.push_back(peer_rank[j]);
      // [0] uses, [1] finished workgroups of k_p2p_pull, [2 + i] workgroups done for peer i
      CHK(p2p_flags_and_counters(ctx, pl, 2 + peers.size(), loop_ready, loop_cons));
      for (size_t j = 0; j < peers.size(); ++j) peers[j].done = pl.p2p_cnt + 2 + j;
      CHK(plan_upload(ctx, pl, pl.d_pseg, segs.data(), segs.size() * sizeof(P2PSeg)));
      CHK(plan_upload(ctx, pl, pl.d_chunk, chunks.data(), chunks.size() * sizeof(int2)));
      CHK(plan_upload(ctx, pl, pl.d_peer, peers.data(), peers.size() * sizeof(P2PPeer)));
    }
    return MPAS_DYC_OK;
  }();
  return p2p_vote(ctx, built, "mapping the peers' fields");
}

// Sets up the exchange points built since the last call (p2p_id < 0).  Every rank builds the same
// exchange points in the same (plan key) order; the counts are checked here, and every message's
// size against its sender's in the two set-ups.
int p2p_setup(mpas_dyc_ctx* ctx) {
  std::vector<XPlan*> bufs, pulls;
  for (auto& kv : ctx->plans)
    if (kv.second.p2p && kv.second.p2p_id < 0) {
      // MPAS_DYCORE_P2P_SKIP=key[,key...]: the pull plans whose plan key contains one of the substrings
      kv.second.skip_pull = kv.second.pull && key_in_list(getenv("MPAS_DYCORE_P2P_SKIP"), kv.first);
      (kv.second.pull ? pulls : bufs).push_back(&kv.second);
    }
  // nothing to map and no peer process to agree with (a single block, or only in-process copies)
  if (bufs.empty() && pulls.empty() && ctx->nranks == 1) return MPAS_DYC_OK;
  CHK(p2p_init(ctx));
  // every rank must set up the same exchange points, split the same way into pull and buffer plans,
  // with the same next flag slot: pulls and buffers take different all-gathers below (a rank whose
  // environment -- MPAS_DYCORE_P2P_PULL / _BUFFERS / _OVERLAP -- or lists differ would pair its
  // all-gathers with other ones), and the slot numbers name the flags the peers wait on
  const int64_t n[3] = {(int64_t)pulls.size(), (int64_t)bufs.size(), (int64_t)ctx->p2p_next};
  std::vector<char> all;
  CHK(allgather_bytes(ctx, n, sizeof(n), all));
  for (int r = 0; r < ctx->nranks; ++r) {
    const int64_t* o = (const int64_t*)all.data() + 3 * (size_t)r;
    if (o[0] != n[0] || o[1] != n[1] || o[2] != n[2]) {
      ctx->err = "MPAS_DYCORE_P2P: rank " + std::to_string(r) + " sets up " + std::to_string(o[0]) + " pull and " +
                 std::to_string(o[1]) + " buffer exchange points from flag slot " + std::to_string(o[2]) + ", rank " +
                 std::to_string(ctx->rank) + " " + std::to_string(n[0]) + " and " + std::to_string(n[1]) +
                 " from slot " + std::to_string(n[2]) + " (every rank must run the same exchange sequence with the "
                 "same MPAS_DYCORE_P2P_* settings)";
      return MPAS_DYC_ECOMM;
    }
  }
  CHK(p2p_setup_pull(ctx, pulls));
  return p2p_setup_buffers(ctx, bufs);
}

// the one-sided transfer dropped on every rank (P2P_UNAVAILABLE): its plans, mappings and arena
// freed, the plans rebuilt for RCCL by the caller
void p2p_fallback(mpas_dyc_ctx* ctx) {
  fprintf(stderr, "mpas_dycore rank %d: %s; halo exchanges go through RCCL\n", ctx->rank, ctx->err.c_str());
  invalidate_plans(ctx);
  p2p_teardown(ctx);
  ctx->p2p = 0;
}

// p2p_status: a wait of k_p2p_get that timed out
int p2p_check(mpas_dyc_ctx* ctx) {
  if (!ctx->p2p_status) return MPAS_DYC_OK;
  int st = 0;
  HIPCHK(hipMemcpy(&st, ctx->p2p_status, sizeof(int), hipMemcpyDeviceToHost));
  if (st) {
    ctx->err = std::string("MPAS_DYCORE_P2P: a peer's halo message did not arrive within 30 s (last exchange: ") +
               ctx->last_key + ")";
    return MPAS_DYC_ECOMM;
  }
  return MPAS_DYC_OK;
}

// pm_group.cpp — batched multi-session serving on the host: the shared step
// of a StepGroup, the sharded exchange, the lock-step team loop
// (run_batched_team), pm_batchpir_group_*, the pooled loop (run_batched_pool)
// and pm_search_loop_sharded.  Needs pm_ctx.cpp, pm_engine.cpp and
// pm_search.cpp.
#include "pm_engine.h"
#include "pm_gvi_offs.h"

// ---------------------------------------------------------------------------
// Batched multi-session serving: S client sessions in
// lock-step, every batch-PIR round of all of them ONE step over S x 16
// partitions (k_match -> k_resolve -> [k_gather] -> k_answer), so a round
// costs one launch sequence for all clients instead of one per client.  Each
// session keeps its own keys, hint state, cache, counters, search state and
// maintenance; the shared step only concatenates their sub-queries (a
// session's partition p is the step's partition s * 16 + p) and scores each
// decoded row against its own session's query (PmPart::qv).  Host work (the
// sessions' searches) runs on a pool of worker threads between steps.
// ---------------------------------------------------------------------------
struct SpinBarrier {
  std::atomic<uint32_t> count{0}, gen{0};
  uint32_t n = 1;
  void wait() {
    const uint32_t g0 = gen.load(std::memory_order_acquire);
    if (count.fetch_add(1, std::memory_order_acq_rel) + 1 == n) {
      count.store(0, std::memory_order_relaxed);
      gen.fetch_add(1, std::memory_order_release);
    } else {
      while (gen.load(std::memory_order_acquire) == g0) std::this_thread::yield();
    }
  }
};

// The sharded loop's exchange: the caller's combine (an in-place SUM
// all-reduce of a team's records over the ranks, ordered on the given stream),
// issued in one global order (round-major, then team) on every rank so the
// ranks' collectives match; or model_peers: the partitions this rank does not
// hold are answered from the synthetic graph's spec on the device (a shard
// layout wider than the job, measured one shard per GPU).
struct ShardComb {
  pm_combine_fn fn = nullptr;   // include/pacmann.h
  void* user = nullptr;
  bool model_peers = false;
  uint32_t NG = 1;
  uint64_t* const* bufs = nullptr;   // the caller's device buffers, one per team (null: the library's)
  std::atomic<uint64_t> ticket{0};
  std::atomic<bool> abort{false};
};

static int group_upload_parts(StepGroup& G) {
  std::vector<PmPart> v;
  v.reserve((size_t)G.S * G.P);
  for (uint32_t s = 0; s < G.S; ++s) {
    Engine* e = G.es[s];
    for (uint32_t p : G.lp) {
      PmPart d = e->parts[p].d;
      d.qv = G.qv.empty() ? nullptr : G.qv[s];
      v.push_back(d);
    }
  }
  HIPCHK(hipMemcpyAsync(G.parts_d.p, v.data(), v.size() * sizeof(PmPart), hipMemcpyHostToDevice, G.c->stream));
  HIPCHK(hipStreamSynchronize(G.c->stream));
  G.gen.resize(G.S);
  for (uint32_t s = 0; s < G.S; ++s) G.gen[s] = G.es[s]->prep_gen;
  return 0;
}

// Common setup of a step group over clients of one server (same DB, shard
// and parameters): device buffers and the clients' parts.
static int group_init(StepGroup& G, pm_ctx* c) {
  G.c = c;
  G.S = (uint32_t)G.es.size();
  const Engine& e = *G.es[0];
  G.P = (uint32_t)e.P; G.maxPH = e.maxPH; G.ph8 = e.ph8; G.maxSS = e.maxSS; G.E = (uint32_t)e.E;
  G.lp = e.owned_list;
  G.Pl = (uint32_t)G.lp.size();
  HIPCHK(hipSetDevice(c->device));
  CHK(G.parts_d.reserve(std::max<size_t>(1, (size_t)G.S * G.Pl) * sizeof(PmPart)));
  CHK(G.done.reserve(4 * (3 + 65536)));
  const uint32_t init[3] = {1u << 31, 0, 0};
  HIPCHK(hipMemcpy(G.done.p, init, sizeof init, hipMemcpyHostToDevice));
  return group_upload_parts(G);
}

// Session s's sub-queries for the next shared step into its stage slot (the
// session's own task, after gvi_pre: the data is in this core's cache).  A
// session with more than `stride` sub-queries leaves its slot invalid and the
// step is built the general way (group_step raises the stride).
static void group_stage_session(StepGroup& G, uint32_t s) {
  StepGroup::SessStage& ss = G.stg[s];
  ss.ok = false;
  if (!G.stage_on || !G.stride) return;
  const Engine* e = G.es[s];
  PmSub* dst = G.stage_h.as<PmSub>() + (uint64_t)s * G.stride;
  uint32_t n = 0, nreal = 0, maxpp = 0, live = 0;
  double bytes = 0;
  ss.pc.resize(G.Pl);
  for (uint32_t li = 0; li < G.Pl; ++li) {
    const uint32_t p = G.lp[li], a = e->sb[p], b = e->sb[p + 1];
    if (n + (b - a) > G.stride) { ss.n = n + (b - a); return; }
    const double ab = answer_bytes(e->parts[p].d, G.E);
    for (uint32_t j = a; j < b; ++j) {
      PmSub x = e->subs[j];
      x.part = s * G.Pl + li;
      dst[n++] = x;
      if (x.kind == SUB_REAL || x.kind == SUB_DUMMY) bytes += ab;
      nreal += x.kind == SUB_REAL;
    }
    ss.pc[li] = b - a;
    maxpp = std::max(maxpp, b - a);
    live += b > a;
  }
  ss.n = n; ss.nreal = nreal; ss.maxpp = maxpp; ss.live = live; ss.bytes = bytes;
  ss.step = G.nstep;
  ss.ok = true;
}

namespace pmh {
// The kernels of one shared step whose descriptor S is complete (step_chain);
// the completion event unless the records go to a combine.  kind: STEP_SHARED
// (group_step) or STEP_DEVICE (the device loop's steps, run_batched_dev).
int group_step_launch(StepGroup& G, PmStep& S, int kind, uint32_t max_per_part, uint32_t nreal, double ans_bytes) {
  pm_ctx* c = G.c;
  auto t0 = Clock::now();
  pmk::StepShape shape{};
  shape.np = S.np; shape.nsub = S.nsub; shape.np_live = S.np_live; shape.max_per_part = max_per_part;
  shape.maxPH = G.maxPH; shape.maxSS = G.maxSS; shape.E = G.E; shape.ph8 = G.ph8;
  shape.of_caller(kind, false);
  shape.unfused = c->no_fuse || c->debug_sync; shape.no_split = c->no_split; shape.no_guess = c->no_guess;
  CHK(step_chain(c, G.buf, S, shape, nreal, ans_bytes));
  if (!G.comb) G.seq = c->record_done(c->stream);   // sharded: group_exchange publishes the records
  HIPCHK(hipGetLastError());
  c->host_add(HT_STEP_LAUNCH, ms_since(t0));
  G.pf_w0 = S.pf_w0; G.pf_w1 = S.pf_w1;
  return 0;
}
}  // namespace pmh

// One shared step over the clients whose sub-queries are ready (in[s]).
static int group_step(StepGroup& G, const std::vector<char>& in) {
  pm_ctx* c = G.c;
  hipStream_t st = c->stream;
  // timing 3: events on every kSampleSteps-th shared step of this stream (7: coprime
  // with the 20 rounds of a search, so every round position is sampled); the
  // events' dispatch-packet and completion handling cost ~5 % of the serving
  // rate when every launch carries them
  constexpr uint64_t kSampleSteps = 7;
  c->sample_now = c->sample_ctr++ % kSampleSteps == 0;
  bool stale = false;   // a client re-preprocessed since its parts were copied
  for (uint32_t s = 0; s < G.S; ++s) stale |= G.es[s]->prep_gen != G.gen[s];
  if (stale) CHK(group_upload_parts(G));
  G.sb.assign(1, 0);
  G.base.assign(G.S, 0);
  uint32_t max_per_part = 0, np_live = 0, nreal = 0, nsub = 0;
  double ans_bytes = 0;
  const uint32_t np = G.S * G.Pl;
  // the sessions' staged slots (group_stage_session), if every one is current
  bool staged = G.stage_on && G.stride > 0 && G.stg.size() == G.S;
  uint32_t need = 0;   // the largest session's sub-queries (the next stride)
  for (uint32_t s = 0; staged && s < G.S; ++s) {
    const StepGroup::SessStage& ss = G.stg[s];
    if (!in[s]) continue;
    need = std::max(need, ss.n);
    if (!ss.ok || ss.step != G.nstep) staged = false;
    nsub += ss.n;
  }
  if (staged && pmk::step_args_fit(nsub, np)) staged = false;   // kernel-argument descriptors: the general way
  G.nstep++;
  PmSub* const stage = G.stage_h.as<PmSub>();
  if (staged) {   // compact the slots in place; the partition offsets follow the subs
    uint32_t off = 0;
    for (uint32_t s = 0; s < G.S; ++s) {
      const StepGroup::SessStage& ss = G.stg[s];
      G.base[s] = off;
      const uint32_t n = in[s] ? ss.n : 0;
      if (n && off != s * G.stride) memmove(stage + off, stage + (uint64_t)s * G.stride, (size_t)n * sizeof(PmSub));
      for (uint32_t li = 0; li < G.Pl; ++li) G.sb.push_back(G.sb.back() + (in[s] ? ss.pc[li] : 0));
      if (in[s]) {
        max_per_part = std::max(max_per_part, ss.maxpp);
        np_live += ss.live;
        ans_bytes += ss.bytes;
        nreal += ss.nreal;
      }
      off += n;
    }
  } else {
    G.subs.clear();
    for (uint32_t s = 0; s < G.S; ++s) {
      Engine* e = G.es[s];
      G.base[s] = (uint32_t)G.subs.size();
      for (uint32_t li = 0; li < G.Pl; ++li) {
        const uint32_t p = G.lp[li];
        if (in[s]) {
          for (uint32_t j = e->sb[p]; j < e->sb[p + 1]; ++j) {
            PmSub x = e->subs[j];
            x.part = s * G.Pl + li;
            G.subs.push_back(x);
            if (x.kind == SUB_REAL || x.kind == SUB_DUMMY) ans_bytes += answer_bytes(e->parts[p].d, G.E);
            nreal += x.kind == SUB_REAL;
          }
          const uint32_t n = e->sb[p + 1] - e->sb[p];
          max_per_part = std::max(max_per_part, n);
          np_live += n > 0;
        }
        G.sb.push_back((uint32_t)G.subs.size());
      }
      need = std::max(need, in[s] ? (uint32_t)G.subs.size() - G.base[s] : 0u);
    }
    nsub = (uint32_t)G.subs.size();
  }
  G.nsub = nsub;
  if (G.stage_on && need > G.stride) {   // slots for the next step's staging (the tasks write them after this step)
    G.stride = (need + 7) & ~7u;
    CHK(G.stage_h.reserve((size_t)G.S * G.stride * sizeof(PmSub) + (size_t)(np + 1) * 4));
    if (G.stg.size() != G.S) G.stg.resize(G.S);
  }
  if (nsub == 0) return 0;
  const uint32_t words = (G.maxPH + 63) / 64, cblk = pmk::step_match_blocks(G.maxPH);
  StepBufs& B = G.buf;
  CHK(B.reserve(nsub, np, words, cblk, G.E));
  const size_t dsub = nsub * sizeof(PmSub);
  char* dh;
  if (staged) {   // the compacted slots are the descriptor; the offsets right after them
    dh = G.stage_h.as<char>();
    memcpy(dh + dsub, G.sb.data(), (np + 1) * 4);
  } else {
    CHK(B.desc_h.reserve(dsub + (np + 1) * 4));
    dh = B.desc_h.as<char>();
    memcpy(dh, G.subs.data(), dsub);
    memcpy(dh + dsub, G.sb.data(), (np + 1) * 4);
  }
  PmStep S{};
  S.parts = G.parts_d.as<PmPart>();
  S.subs_h = (const PmSub*)dh;
  S.sb_h = (const uint32_t*)(dh + dsub);
  B.fill(S, words, cblk);
  if (!pmk::step_args_fit(nsub, np)) {
    // a large descriptor crosses PCIe once, by DMA, instead of as thousands of
    // zero-copy reads by the match workgroups; k_match* stage it from here
    CHK(G.desc_d.reserve(dsub + (np + 1) * 4));
    HIPCHK(hipMemcpyAsync(G.desc_d.p, dh, dsub + (np + 1) * 4, hipMemcpyHostToDevice, st));
    S.subs_h = G.desc_d.as<PmSub>();
    S.sb_h = (const uint32_t*)(G.desc_d.as<char>() + dsub);
    S.subs = const_cast<PmSub*>(S.subs_h);   // the DMA'd descriptor is the device copy
    S.sb = const_cast<uint32_t*>(S.sb_h);
  }
  S.done = G.done.as<uint32_t>();
  Engine* e0 = G.es[0];
  e0->step_db(S);
  S.q = nullptr;   // each partition's PmPart::qv
  if (G.comb) {   // sharded: results stay on the device for group_exchange's records
    CHK(G.out_d.reserve(step_out_bytes(nsub, G.E)));
    step_out(S, G.out_d.p, nsub);
  } else {
    CHK(B.out_h.reserve(step_out_bytes(nsub, G.E)));
    step_out(S, B.out_h.p, nsub);
  }
  S.E = G.E; S.dim = G.dim; S.nsub = nsub; S.np = np;
  S.np_live = np_live;
  if (pmk::step_args_fit(nsub, np)) {   // (never the staged form)
    memcpy(S.subs_a, G.subs.data(), dsub);
    memcpy(S.sb_a, G.sb.data(), (np + 1) * 4);
  }
  S.token = next_token(G.token);
  step_read_window(S, e0->pf_off, e0->pf_len, G.E);
  S.rows_partial = host_rows_partial(c, G.rows_partial);
  return group_step_launch(G, S, pmk::STEP_SHARED, max_per_part, nreal, ans_bytes);
}

// The lines session s's collect will read (its result headers and the row
// words the host reads, its localCache slots, its ids' ground-truth rows),
// requested one task ahead by the worker that will most likely take it: the
// misses then resolve while the worker serves the session before it.
static void prefetch_session(StepGroup& G, uint32_t s, const pm_graph* g) {
  const Engine* e = G.es[s];
  const uint32_t n = (uint32_t)e->subs.size();
  const PmOutHdr* hdr = G.buf.out_h.as<PmOutHdr>() + G.base[s];
  const char* rows = G.buf.out_h.as<char>() + (size_t)G.nsub * sizeof(PmOutHdr) + (size_t)G.base[s] * G.E * 8;
  for (uint32_t j = 0; j < n; j += 2) __builtin_prefetch(hdr + j);
  for (uint32_t j = 0; j < n; ++j)
    for (uint32_t w = G.pf_w0; w < G.pf_w1; w += 8) __builtin_prefetch(rows + ((size_t)j * G.E + w) * 8);
  // (not its localCache slots: that session's collect may be rehashing its
  // FlatMap on another worker right now; group_collect prefetches them itself)
  if (g->graph)
    for (size_t b = 0; b < g->batch.size(); ++b) __builtin_prefetch(&g->graph[(uint64_t)g->batch[b] * g->m]);
}

// Session s's share of the last shared step: wait for its results (tokens and
// row checksums, polled by the session's own worker, so a team checks its
// sub-queries in parallel) and update its host mirrors.
static int group_collect(StepGroup& G, uint32_t s) {
  Engine* e = G.es[s];
  const uint32_t n = (uint32_t)e->subs.size();
  for (uint32_t j = 0; j < n; ++j)   // the localCache slots post_results fills, requested ahead
    if (e->subs[j].kind == SUB_REAL) e->parts[e->subs[j].part].cache.prefetch(e->subs[j].idx);
  PmOutHdr* hdr = G.buf.out_h.as<PmOutHdr>();
  uint64_t* rows = (uint64_t*)(G.buf.out_h.as<char>() + (size_t)G.nsub * sizeof(PmOutHdr));
  auto t_wait = Clock::now();
  CHK(wait_step(e->ctx, hdr + G.base[s], n, G.token, (const char*)(rows + (uint64_t)G.base[s] * G.E),
                (size_t)G.E * 8, (size_t)G.pf_w0 * 8, (size_t)(G.pf_w1 - G.pf_w0) * 8, G.seq, G.c));
  e->ctx->host_add(HT_STEP_WAIT, ms_since(t_wait));
  auto tp = Clock::now();
  post_results(e, hdr, rows, n, G.base[s], G.token);
  e->ctx->host_add(HT_STEP_POST, ms_since(tp));
  return 0;
}

// The team's queries (staged in G.qstage) to the device and every session's
// start-set distances (search.go:130-146) in one k_l2_rows launch: over the
// device copy of all vectors by start id, or (sharded / synthetic graphs)
// over the sessions' start vectors themselves.
static int group_start_dist(StepGroup& G, pm_graph** gs) {
  hipStream_t st = G.c->stream;
  float* qst = G.qstage.as<float>();
  HIPCHK(hipMemcpyAsync(G.qbuf.p, qst, (uint64_t)G.S * G.dim * 4, hipMemcpyHostToDevice, st));
  const uint64_t nrows = (uint64_t)G.S * G.ns;
  if (nrows) {
    const bool ids = gs[0]->dvec->p != nullptr;
    G.c->timed("l2_rows", (double)nrows * G.dim * 4, [&] {
      pmk::l2_rows(st, ids ? gs[0]->dvec->as<float>() : G.start_vec.as<float>(), G.dim, nrows,
                   ids ? G.start_ids.as<uint32_t>() : nullptr, G.qbuf.as<float>(), G.dim, G.start_dist.as<float>(),
                   G.ns);
    });
    HIPCHK(hipMemcpyAsync(qst + (uint64_t)G.S * G.dim, G.start_dist.p, nrows * 4, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

namespace pmh {
// SimpleBatchPianoPIR.Preprocessing (batch-pir.go:119-155) of the clients
// `who` (batch PIR engines of one server: same DB and parameters, partitions
// lp), as ONE launch set over all their partitions on c's stream, with its
// parts staged in pbuf.  Each client's maintenance time is the set's wall time
// (added to *mt[i] when given).
// Async form (stage non-null): the parts go up from the pinned `stage` (its
// previous copy waited for through *stage_ev), nothing waits for the launch
// set, and the caller times it with events (mt unused).
int prep_clients(pm_ctx* c, DevBuf& pbuf, const std::vector<uint32_t>& lp, const std::vector<Engine*>& who,
                        const std::vector<double*>* mt, HostBuf* stage, hipEvent_t* stage_ev) {
  if (who.empty()) return 0;
  // one fold form for the set, chosen from who[0]: a client created without the
  // fold image ("fold_rot" 0) has the chunk-major table the pipelined fold reads,
  // one created with it does not (checked before any client's state changes)
  for (Engine* e : who)
    if ((e->img->p != nullptr) != (who[0]->img->p != nullptr))
      return fail(PM_EINVAL, "grouped clients were created with and without the fold image");
  auto t0 = Clock::now();
  std::vector<PmPart> hp;
  std::vector<uint64_t> todo;
  for (Engine* e : who) {
    e->FBN = 0; e->QMIP = 0;
    CHK(engine_prep_host(e, 0, e->P, todo, c->stream));   // ordered before the launch set below
  }
  // partition-major: the clients' folds of one partition run side by side and
  // share its DB rows through the caches instead of re-reading them per client
  for (uint32_t p : lp)
    for (Engine* e : who) hp.push_back(e->parts[p].d);
  const Engine* e0 = who[0];
  bool skip = false;
  for (Engine* e : who) skip |= e->skipPrep != e0->skipPrep;
  if (skip) return fail(PM_EINVAL, "batched sessions mix Preprocessing and DummyPreprocessing");
  CHK(pbuf.reserve(hp.size() * sizeof(PmPart)));
  if (stage) {
    if (*stage_ev) HIPCHK(hipEventSynchronize(*stage_ev));
    else HIPCHK(hipEventCreateWithFlags(stage_ev, hipEventDisableTiming));
    CHK(stage->reserve(hp.size() * sizeof(PmPart)));
    memcpy(stage->p, hp.data(), hp.size() * sizeof(PmPart));
    HIPCHK(hipMemcpyAsync(pbuf.p, stage->p, hp.size() * sizeof(PmPart), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(*stage_ev, c->stream));
  } else {
    HIPCHK(hipMemcpyAsync(pbuf.p, hp.data(), hp.size() * sizeof(PmPart), hipMemcpyHostToDevice, c->stream));
  }
  CHK(engine_prep_launch(c, e0, pbuf.as<PmPart>(), (int)hp.size(), hp.data(), (uint32_t)who.size(), !stage));
  c->host_add(HT_PREP_SETS, (double)who.size());
  const double t = std::chrono::duration<double>(Clock::now() - t0).count();
  for (size_t i = 0; i < who.size(); ++i) {
    who[i]->prepCount++;
    record_stats(who[i], t);
    if (mt) *(*mt)[i] += t;
  }
  return 0;
}
}  // namespace pmh
// The clients of team G with need[s], as one launch set on the team's stream.
static int group_prep(StepGroup& G, const std::vector<char>& need, std::vector<double>* mt) {
  std::vector<Engine*> who;
  std::vector<double*> mts;
  for (uint32_t s = 0; s < G.S; ++s)
    if (need[s]) {
      who.push_back(G.es[s]);
      if (mt) mts.push_back(&(*mt)[s]);
    }
  return prep_clients(G.c, G.prep_parts, G.lp, who, mt ? &mts : nullptr);
}

// ---- sharded private search (pm_search_loop_sharded) --------------------
// Every rank runs the same sessions (same seeds, same queries) over its shard
// of the graph DB.  A round: each session's GetVertexInfo batch is bucketed
// (bq_prepare: the global decisions, identical on every rank) and its
// sub-queries on this rank's partitions join the team's shared step; the step's
// answers become per-id records [session][position] = {neighbour words, dist |
// ok << 32}, zero where this rank holds no answer; ONE combine per shared step
// sums the records over the ranks; every rank then reads all records back and
// continues the identical searches.  Host mirrors (FinishedQueryNum, the local
// cache, counters, the maintenance trigger) are per rank and per partition, as
// in the single-rank engine, so each rank's partitions evolve exactly as the
// unsharded engine's do.

// Bucket session s's batch (rank-local sub-queries) and fill its rows of the
// record map: the answering sub-query (client-local index) of each position,
// -1 (no local answer) or -2 (answered by a modelled peer).  A batch that
// needs several steps here (a partition at its query budget) is served now on
// the session's own stream and its records packed on the host.
static int gvi_pre_sharded(pm_graph* g, StepGroup& G, uint32_t s, bool* fast) {
  const uint64_t n = g->batch.size(), m = g->m;
  if (n != G.npos) return fail(PM_EINVAL, "sharded search: every round must fetch parallel * m ids");
  g->total += n;
  g->nb.resize(n * m);
  g->dist.assign(n, 0.0f);
  Engine* e = &g->pir->e;
  g->qids.assign(g->batch.begin(), g->batch.end());
  auto t = Clock::now();
  e->rows_partial = true;
  CHK(bq_prepare(e, g->qids.data(), n, fast));
  int32_t* map = G.map_h.as<int32_t>() + (uint64_t)s * G.npos;
  if (*fast) {
    e->resp_map.clear();
    for (size_t j = 0; j < e->subs.size(); ++j) {
      const uint32_t k = e->subs[j].kind;
      if (k == SUB_REAL || k == SUB_HOSTCACHE) e->resp_map.put(e->sub_gid[j], (uint32_t)j);   // last wins
    }
  } else {
    g->rowp.resize(n);
    g->okv.assign(n, 0);
    CHK(batch_query_impl(e, g->qids.data(), n, nullptr, g->qdev(), (uint32_t)g->dim, g->dist.data(), g->rowp.data(),
                         g->okv.data()));
    uint64_t* rec = G.slow_h.as<uint64_t>() + (uint64_t)s * G.npos * G.W;
    for (uint64_t i = 0; i < n; ++i) {
      uint64_t* r = rec + i * G.W;
      const bool own = e->parts[g->qids[i] / e->PS].owned;
      for (uint32_t w = 0; w + 1 < G.W; ++w) r[w] = own && g->okv[i] ? g->rowp[i][G.w0 + w] : 0;
      uint32_t db;
      memcpy(&db, &g->dist[i], 4);
      r[G.W - 1] = own && g->okv[i] ? (1ull << 32) | db : 0;
    }
  }
  uint64_t* ids = G.ids_h.as<uint64_t>() + (uint64_t)s * G.npos;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t id = g->qids[i], p = id / e->PS;
    int32_t v = -1;
    if (e->parts[p].owned) {
      if (*fast)
        if (const uint32_t* j = e->resp_map.find(id)) v = (int32_t)*j;
    } else if (G.comb->model_peers) {   // answered by its partition's holder unless dropped (batch-pir.go:195-200)
      for (uint64_t j = 0; j < e->qn && j < e->pq[p].size(); ++j)
        if (e->pq[p][j] == id) { v = -2; break; }
    }
    map[i] = v;
    ids[i] = id;
  }
  G.slow[s] = !*fast;
  e->ctx->host_add(HT_BATCH_QUERY, ms_since(t));
  return 0;
}

// After the shared step (group_step): the records of this rank's answers, the
// multi-step sessions' host-packed records, the modelled peers' records, the
// combine, and one copy of all records (and the step's statuses) to the host.
//
// Failure protocol (every rank must issue the same collectives): the team's
// records end in ONE error word, 0 from a healthy rank.  A rank whose team (or
// another team of the same rank: ShardComb::abort) failed still takes the
// team's next combine turn, with zero records and the error word 1 (poison);
// every rank then reads a nonzero sum in that turn's records and stops the
// team there (group_collect_sharded).  So all ranks issue each team's
// collectives up to the same turn and none is left waiting in a collective.
static int group_exchange(StepGroup& G, const std::vector<char>& in, bool poison) {
  pm_ctx* c = G.c;
  hipStream_t st = c->stream;
  const uint32_t nrec = G.S * G.npos;
  const uint64_t nw = (uint64_t)nrec * G.W;
  uint32_t* st2 = G.st_d.as<uint32_t>();
  uint32_t nsub = poison ? 0u : G.nsub;
  // this rank's records (map, pack, multi-step sessions, modelled peers)
  auto pack = [&]() -> int {
    int32_t* map = G.map_h.as<int32_t>();
    for (uint32_t s = 0; s < G.S; ++s)   // client-local sub-query indices -> the shared step's
      for (uint32_t i = 0; i < G.npos; ++i) {
        int32_t& v = map[(uint64_t)s * G.npos + i];
        if (poison) v = -1;
        else if (v >= 0) v = in[s] ? v + (int32_t)G.base[s] : -1;
      }
    HIPCHK(hipMemcpyAsync(G.map_d.p, map, (uint64_t)nrec * 4, hipMemcpyHostToDevice, st));
    const PmOutHdr* hdr = G.out_d.as<PmOutHdr>();
    const uint64_t* rows = (const uint64_t*)(G.out_d.as<char>() + (uint64_t)G.nsub * sizeof(PmOutHdr));
    c->timed("pack_records", (double)nw * 8, [&] {
      pmk::pack_records(st, G.map_d.as<int32_t>(), nrec, hdr, rows, G.E, G.w0, G.W, G.rec_d, nsub, st2,
                        poison ? 1u : 0u); });
    for (uint32_t s = 0; s < G.S && !poison; ++s)
      if (G.slow[s])
        HIPCHK(hipMemcpyAsync(G.rec_d + (uint64_t)s * G.npos * G.W, G.slow_h.as<uint64_t>() + (uint64_t)s * G.npos * G.W,
                              (uint64_t)G.npos * G.W * 8, hipMemcpyHostToDevice, st));
    if (G.comb->model_peers && !poison) {
      HIPCHK(hipMemcpyAsync(G.ids_d.p, G.ids_h.p, (uint64_t)nrec * 8, hipMemcpyHostToDevice, st));
      const pm_graph* g0 = G.gs[0];
      c->timed("synth_records", 0, [&] {
        pmk::synth_records(st, G.map_d.as<int32_t>(), G.ids_d.as<uint64_t>(), nrec, G.npos, G.qbuf.as<float>(), G.dim,
                           (uint32_t)g0->m, g0->n, g0->data_seed, G.w0, G.W, G.rec_d); });
    }
    HIPCHK(hipGetLastError());
    return 0;
  };
  const int pre = pack();
  std::string pre_msg;
  if (pre) {
    // a failure before the collective: the turn is still owed to the peers.
    // Take it poisoned (zero records, error word 1) if the device still
    // accepts work; otherwise no further turn can match the peers' (they are
    // then bounded by their own RCCL / torch.distributed timeout).
    pre_msg = pm_last_error();
    poison = true;
    nsub = 0;
    const uint64_t one = 1;
    if (!G.comb->fn || hipMemsetAsync(G.rec_d, 0, nw * 8, st) != hipSuccess ||
        hipMemcpyAsync(G.rec_d + nw, &one, 8, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      G.combine_dead = true;
      return fail(pre, pre_msg);
    }
  }
  if (G.comb->fn) {   // the collective, in the global (round, team) order on every rank
    ShardComb* cb = G.comb;
    const uint64_t turn = G.round * cb->NG + G.team;
    auto tw = Clock::now();
    // no early exit on cb->abort: a failed team still takes its turn (poisoned);
    // bounded so a rank whose peer died ends instead of spinning forever
    static const double limit_s = [] { const char* e = getenv("PM_COMBINE_TIMEOUT_S"); return e ? atof(e) : 600.0; }();
    uint32_t spins = 0;
    while (cb->ticket.load(std::memory_order_acquire) != turn) {
      if (++spins % 1024 == 0 && ms_since(tw) > limit_s * 1e3) {
        G.combine_dead = true;
        return fail(PM_EHIP, "sharded search: combine turn " + std::to_string(turn) + " not reached in " +
                                 std::to_string(limit_s) + " s");
      }
      std::this_thread::yield();
    }
    c->host_add(HT_COMBINE_TURN, ms_since(tw));
    auto t0 = Clock::now();
    int rc = 0;
    c->timed("combine", (double)nw * 8, [&] { rc = cb->fn(cb->user, G.team, G.rec_d, nw + 1, (void*)st); });
    c->host_add(HT_COMBINE, ms_since(t0));
    cb->ticket.fetch_add(1, std::memory_order_acq_rel);
    G.round++;
    if (rc) {   // the collective itself failed: no further turn of this team can match the peers'
      G.combine_dead = true;
      return fail(PM_EHIP, "sharded search: the combine callback failed (" + std::to_string(rc) + ")");
    }
    if (pre) { G.peer_failed.store(true); return fail(pre, pre_msg); }   // the turn taken poisoned; this team stops
  } else {
    G.round++;
  }
  HIPCHK(hipMemcpyAsync(G.rec_h.p, G.rec_d, (nw + 1) * 8, hipMemcpyDeviceToHost, st));
  if (nsub) HIPCHK(hipMemcpyAsync(G.rec_h.as<uint64_t>() + nw + 1, st2, (uint64_t)nsub * 8, hipMemcpyDeviceToHost, st));
  G.seq = c->record_done(st);
  return 0;
}

// L2Dist in the reference's order (l2_distance_amd64.s:4-36 via
// build_graph.go:119-127): eight lane sums of separately rounded sub / mul /
// add, ((l0+l1)+(l2+l3))+((l4+l5)+(l6+l7)), then the scalar tail.  Host-side
// check of the GPU's records only (the translation unit is built without FMA
// contraction).
static float l2_reference_order(const float* a, const float* b, uint64_t dim) {
  const uint64_t dimS = dim & ~7ull;
  float l[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint64_t t = 0; t < dimS; t += 8)
    for (int k = 0; k < 8; ++k) {
      const float d = a[t + k] - b[t + k];
      const float sq = d * d;
      l[k] = l[k] + sq;
    }
  float d = dimS ? ((l[0] + l[1]) + (l[2] + l[3])) + ((l[4] + l[5]) + (l[6] + l[7])) : 0.0f;
  for (uint64_t i = dimS; i < dim; ++i) {
    const float x = a[i] - b[i];
    const float sq = x * x;
    d = d + sq;
  }
  return d;
}

// The record check (pm_set_option "verify_records"): every answered record of
// session s's batch against the graph itself (the synthetic spec or the host
// arrays) — neighbour words bit for bit, and the distance bits against
// l2_reference_order of the vertex's vector and the session's query — and
// every unanswered id against its explanation (private-search.go:441-506 over
// batch-pir.go:170-248).  Counts go to the session's host counters.
static void verify_records(StepGroup& G, uint32_t s, bool fast, const uint64_t* rec, const uint32_t* st2) {
  pm_graph* g = G.gs[s];
  Engine* e = G.es[s];
  const uint64_t dim = g->dim, m = g->m;
  const float* q = G.qstage.as<float>() + (uint64_t)s * dim;
  const uint64_t kv = sm64(g->data_seed + DOM_SYNTH_VEC);
  std::vector<float> vec(dim);
  uint32_t tmp[64];
  for (uint64_t i = 0; i < G.npos; ++i) {
    const uint64_t* r = rec + ((uint64_t)s * G.npos + i) * G.W;
    const uint64_t id = (uint64_t)g->batch[i], p = id / e->PS;
    const bool ok = (r[G.W - 1] >> 32) & 1;
    if (ok) {
      const uint32_t* nb = g->true_nb(id, tmp);
      if (g->synth) for (uint64_t j = 0; j < dim; ++j) vec[j] = graph_synth_vec(kv, id, (uint32_t)dim, (uint32_t)j);
      else memcpy(vec.data(), g->vectors + id * dim, dim * 4);
      const float d = l2_reference_order(vec.data(), q, dim);
      uint32_t dbits;
      memcpy(&dbits, &d, 4);
      const bool good = memcmp((const char*)r + G.nb_off, nb, m * 4) == 0 && (uint32_t)r[G.W - 1] == dbits;
      g->ctx->host_add(good ? HT_REC_VERIFIED : HT_REC_BAD, 0.0);
      continue;
    }
    bool made = false;   // was a sub-query made for it (among the first qn of its partition, batch-pir.go:195-200)?
    for (uint64_t j = 0; j < e->qn && j < e->pq[p].size(); ++j) made |= e->pq[p][j] == id;
    HostTimer why = HT_REC_UNEXPLAINED;
    if (!made) {
      why = HT_REC_DROPPED;
    } else if (!e->parts[p].owned) {
      why = G.comb->model_peers ? HT_REC_UNEXPLAINED : HT_REC_PEER;   // a modelled peer always answers
    } else if (!fast) {
      why = HT_REC_FAILED;   // the multi-step path: its sub-queries' statuses stay on the host path
    } else if (const uint32_t* j = e->resp_map.find(id)) {
      const uint32_t st = st2[2 * ((uint64_t)G.base[s] + *j)];
      if (st == ST_ENOHIT || st == ST_ECHUNK || st == ST_EBUDGET) why = HT_REC_FAILED;
    }
    g->ctx->host_add(why, 0.0);
  }
}

// Session s's share of the exchanged records: host mirrors of its sub-queries
// on this rank (post_results), the batch's counters and trigger (bq_tail), and
// the neighbour lists and distances of all its ids (Entry2VectorAndNeighbors,
// private-search.go:418-439, with the success check :483-497).
static int group_collect_sharded(StepGroup& G, uint32_t s, bool fast) {
  pm_graph* g = G.gs[s];
  Engine* e = G.es[s];
  auto t_wait = Clock::now();
  if (G.c->publish_wait) CHK(wait_done(G.c, G.seq));
  else HIPCHK(hipStreamSynchronize(G.c->stream));
  e->ctx->host_add(HT_STEP_WAIT, ms_since(t_wait));
  const uint64_t nw = (uint64_t)G.S * G.npos * G.W, m = g->m;
  const uint64_t* rec = G.rec_h.as<uint64_t>();
  if (rec[nw]) {   // the error word: rec[nw] ranks poisoned this turn (group_exchange)
    G.peer_failed.store(true);
    return fail(PM_EHIP, "sharded search: " + std::to_string(rec[nw]) + " rank(s) failed; this team stops at the "
                         "same combine turn on every rank");
  }
  const uint32_t* st2 = (const uint32_t*)(rec + nw + 1);
  if (fast) {
    auto tp = Clock::now();
    for (size_t j = 0; j < e->subs.size(); ++j) {
      const uint64_t k = G.base[s] + j;
      if (st2[2 * k] == ST_OK) {
        PartHost& ph = e->parts[e->subs[j].part];
        ph.fqn++;
        ph.cache.put(e->subs[j].idx, st2[2 * k + 1]);
      }
    }
    e->ctx->host_add(HT_STEP_POST, ms_since(tp));
    CHK(bq_tail(e, G.npos));
  }
  auto t_parse = Clock::now();
  uint32_t tmp[64];
  for (uint64_t i = 0; i < G.npos; ++i) {
    const uint64_t* r = rec + ((uint64_t)s * G.npos + i) * G.W;
    uint32_t* nbi = &g->nb[i * m];
    memcpy(nbi, (const char*)r + G.nb_off, m * 4);
    const uint32_t db = (uint32_t)r[G.W - 1];
    memcpy(&g->dist[i], &db, 4);
    if (memcmp(nbi, g->true_nb((uint64_t)g->batch[i], tmp), m * 4) == 0) g->succ++;
  }
  if (G.verify_every && (G.round - 1) % G.verify_every == 0) verify_records(G, s, fast, rec, st2);
  e->rows_partial = false;
  g->ctx->host_add(HT_GVI_PARSE, ms_since(t_parse));
  return 0;
}

// Buffers of a sharded team (after group_init).
static int group_shard_init(StepGroup& G, pm_graph** gs, uint32_t S, int parallel, ShardComb* comb, uint32_t team) {
  G.comb = comb;
  G.team = team;
  G.round = 0;
  G.verify_every = (uint32_t)g_verify_records.load();
  G.gs.assign(gs, gs + S);
  const Engine& e = gs[0]->pir->e;
  G.npos = (uint32_t)(parallel * gs[0]->m);
  G.w0 = (uint32_t)(gs[0]->dim * 4 / 8);
  const uint32_t w1 = (uint32_t)((gs[0]->dim * 4 + gs[0]->m * 4 + 7) / 8);
  G.W = w1 - G.w0 + 1;
  G.nb_off = (uint32_t)(gs[0]->dim * 4 - (uint64_t)G.w0 * 8);
  if (e.pf_off != (size_t)gs[0]->dim * 4) return fail(PM_EINVAL, "sharded search: entries are not PIRGraphInfo's");
  const uint64_t nrec = (uint64_t)S * G.npos, nw = nrec * G.W;
  if (comb->bufs) {
    G.rec_d = comb->bufs[team];
    if (!G.rec_d) return fail(PM_EINVAL, "sharded search: NULL team buffer");
  } else {
    CHK(G.rec_own.reserve((nw + 1) * 8));
    G.rec_d = G.rec_own.as<uint64_t>();
  }
  CHK(G.st_d.reserve(std::max<uint64_t>(8, nrec * 8)));   // at most one sub-query per position
  CHK(G.map_d.reserve(nrec * 4));
  CHK(G.ids_d.reserve(nrec * 8));
  CHK(G.map_h.reserve(nrec * 4));
  CHK(G.ids_h.reserve(nrec * 8));
  CHK(G.slow_h.reserve(nw * 8));
  CHK(G.rec_h.reserve((nw + 1) * 8 + nrec * 8));
  G.slow.assign(S, 0);
  if (!gs[0]->dvec->p) {   // the sessions' start vectors side by side for the team's one k_l2_rows launch
    const uint64_t per = (uint64_t)G.ns * G.dim;
    CHK(G.start_vec.reserve(std::max<uint64_t>(4, S * per * 4)));
    for (uint32_t i = 0; i < S; ++i)
      if (per) HIPCHK(hipMemcpyAsync(G.start_vec.as<float>() + i * per, gs[i]->dstartvec.p, per * 4,
                                     hipMemcpyDeviceToDevice, G.c->stream));
    HIPCHK(hipStreamSynchronize(G.c->stream));
  }
  return 0;
}

namespace pmh {
// A lock-step team's device setup over sessions gs[0..S) (gs[0]'s stream):
// start ids, query slots (each session's query pointer points into G.qbuf
// until team_release), the clients' parts.
int team_init(StepGroup& G, pm_graph** gs, uint32_t S) {
  G.dim = (uint32_t)gs[0]->dim;
  G.rows_partial = true;   // GetVertexInfo reads the neighbour lists only
  for (uint32_t i = 0; i < S; ++i) G.es.push_back(&gs[i]->pir->e);
  HIPCHK(hipSetDevice(gs[0]->ctx->device));
  for (uint32_t i = 0; i < S; ++i) HIPCHK(hipStreamSynchronize(gs[i]->ctx->stream));
  G.ns = (uint32_t)gs[0]->start.size();
  for (uint32_t i = 0; i < S; ++i)
    if (gs[i]->start.size() != G.ns) return fail(PM_EINVAL, "sessions with different start-set sizes");
  CHK(G.qbuf.reserve((uint64_t)S * G.dim * 4));
  CHK(G.start_ids.reserve(std::max<uint64_t>(4, (uint64_t)S * G.ns * 4)));
  CHK(G.start_dist.reserve(std::max<uint64_t>(4, (uint64_t)S * G.ns * 4)));
  CHK(G.qstage.reserve((uint64_t)S * (G.dim + G.ns) * 4));
  {
    std::vector<uint32_t> ids;
    for (uint32_t i = 0; i < S; ++i) ids.insert(ids.end(), gs[i]->start.begin(), gs[i]->start.end());
    if (!ids.empty()) HIPCHK(hipMemcpy(G.start_ids.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
  }
  for (uint32_t i = 0; i < S; ++i) {
    gs[i]->q_shared = G.qbuf.as<float>() + (uint64_t)i * G.dim;
    G.qv.push_back(gs[i]->qdev());
  }
  return group_init(G, gs[0]->ctx);
}
void team_release(pm_graph** gs, uint32_t S) {
  for (uint32_t i = 0; i < S; ++i) gs[i]->q_shared = nullptr;
}

// One lock-step team: sessions gs[0..S) share one step stream (gs[0]'s) and T
// worker threads; maintenance seconds into mt[0..S).  Runs on the calling thread.
int run_batched_team(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k, int step,
                            int parallel, uint32_t T, int64_t* answers, double* mt_out, ShardComb* comb,
                            uint32_t team) {
  StepGroup G;
  struct Unshare {   // the sessions' query pointers point into G.qbuf until the team ends
    pm_graph** gs; uint32_t S;
    ~Unshare() { team_release(gs, S); }
  } unshare{gs, S};
  CHK(team_init(G, gs, S));
  if (comb) CHK(group_shard_init(G, gs, S, parallel, comb, team));
  T = std::max(1u, std::min(T, S));
  std::vector<char> fast(S, 0), need_prep(S, 0);
  std::vector<double> mt(S, 0.0);
  std::atomic<int> err{0};
  std::string err_msg;
  std::atomic<bool> stop{false};
  SpinBarrier bar;
  bar.n = T;
  auto set_err = [&](int rc, uint32_t s) {
    int z = 0;
    if (rc && err.compare_exchange_strong(z, rc)) err_msg = "session " + std::to_string(s) + ": " + pm_last_error();
    if (rc && comb) comb->abort.store(true);   // the other teams stop waiting for this one's turns
  };
  std::vector<int64_t> steps_buf((size_t)T * std::max(k, 1));
  // worker w serves sessions s = w, w + T, ...; worker 0 (this thread) also launches the shared steps
  auto worker = [&](uint32_t w) {
    if (hipSetDevice(G.c->device) != hipSuccess) set_err(PM_EHIP, w);
    int64_t* stp = &steps_buf[(size_t)w * std::max(k, 1)];
    for (uint64_t qi = 0; qi < q; ++qi) {
      // SearchKNN begin: every session's query and start-set distances in one
      // upload, one k_l2_rows launch and one download for the team
      float* qst = G.qstage.as<float>();
      for (uint32_t s = w; s < S; s += T) {
        pm_graph* g = gs[s];
        knn_reset(g);
        g->t_init = Clock::now();
        memcpy(qst + (uint64_t)s * G.dim, queries + ((uint64_t)s * q + qi) * g->dim, G.dim * 4);
      }
      bar.wait();
      if (w == 0 && !err.load()) {
        const int rc = group_start_dist(G, gs);
        if (rc) set_err(rc, 0);
      }
      bar.wait();
      for (uint32_t s = w; s < S && !err.load(); s += T)
        knn_begin_finish(gs[s], parallel, 0, qst + (uint64_t)S * G.dim + (uint64_t)s * G.ns);
      for (int st = 0; st < step; ++st) {
        for (uint32_t s = w; s < S && !err.load(); s += T) {   // this round's ids -> sub-queries
          pm_graph* g = gs[s];
          knn_batch(g, parallel, 0);
          bool f = false;
          const int rc = comb ? gvi_pre_sharded(g, G, s, &f) : gvi_pre(g, true, &f);
          fast[s] = f;
          if (rc) set_err(rc, s);
        }
        bar.wait();
        if (w == 0) {
          if (comb && comb->fn) {   // sharded: this round's combine is taken on every rank (see group_exchange)
            if (G.peer_failed.load() || G.combine_dead) {
              stop.store(true);
            } else {
              bool poison = err.load() != 0 || comb->abort.load();
              // fault seam (tests/test_shard_search_gpu.py): team 0 fails at shared step PM_FAULT_ROUND
              static const long fault_round = [] { const char* e = getenv("PM_FAULT_ROUND"); return e ? atol(e) : -1L; }();
              if (!poison && team == 0 && fault_round >= 0 && G.round == (uint64_t)fault_round) {
                set_err(fail(PM_EHIP, "injected fault (PM_FAULT_ROUND)"), 0);
                poison = true;
              }
              if (!poison) {
                const int rc = group_step(G, fast);
                if (rc) set_err(rc, 0);
                poison = rc != 0;
              }
              const int rx = group_exchange(G, fast, poison);   // records, combine, read-back
              if (rx) set_err(rx, 0);
              stop.store(poison || rx != 0);
            }
          } else {
            if (!err.load()) {
              int rc = group_step(G, fast);
              if (!rc && comb) rc = group_exchange(G, fast, false);   // records, read-back (no collective)
              if (rc) set_err(rc, 0);
            }
            stop.store(err.load() != 0);
          }
        }
        bar.wait();
        if (stop.load()) return;
        for (uint32_t s = w; s < S && !err.load(); s += T) {   // rows -> neighbours, known set
          pm_graph* g = gs[s];
          if (comb) {   // every id's record, combined over the shards
            const int rw = group_collect_sharded(G, s, fast[s]);
            if (rw) { set_err(rw, s); break; }
          } else {
            if (fast[s]) {   // this client's share of the shared step's results
              const int rw = group_collect(G, s);
              if (rw) { set_err(rw, s); break; }
            }
            const int rc = gvi_post(g, true, fast[s]);
            if (rc) { set_err(rc, s); break; }
          }
          knn_update(g, st);
        }
      }
      for (uint32_t s = w; s < S && !err.load(); s += T) {   // top k, maintenance trigger (private-search.go:226-232)
        pm_graph* g = gs[s];
        knn_end(g, k, answers + ((uint64_t)s * q + qi) * k, stp);
        Engine* e = &g->pir->e;
        need_prep[s] = e->FBN + (uint64_t)step * (uint64_t)parallel + 10 >= e->Support;
      }
      bar.wait();
      if (w == 0) {   // the triggered clients' preprocessings as one launch set
        if (!err.load()) {
          const int rc = group_prep(G, need_prep, &mt);
          if (rc) set_err(rc, 0);
        }
        stop.store(err.load() != 0);
        // a sharded team that failed here still owes its peers its next combine turn, poisoned
        if (stop.load() && comb && comb->fn && !G.peer_failed.load() && !G.combine_dead && qi + 1 < q)
          (void)group_exchange(G, fast, true);
      }
      bar.wait();
      if (stop.load()) return;
    }
  };
  std::vector<std::thread> th;
  for (uint32_t w = 1; w < T; ++w) th.emplace_back(worker, w);
  worker(0);
  for (auto& t : th) t.join();
  if (err.load()) return fail(err.load(), err_msg);
  HIPCHK(hipStreamSynchronize(G.c->stream));
  for (uint32_t s = 0; s < S; ++s) mt_out[s] = mt[s];
  return 0;
}
}  // namespace pmh

// ---- SimpleBatchPianoPIR clients served together (the batch API) --------
// S clients of one server (pm_batchpir_create_client): every call answers one
// batch of n ids per client (SimpleBatchPianoPIR.Query, batch-pir.go:170-248,
// per client) with ONE shared step over all their partitions.
struct pm_batchpir_group {
  StepGroup G;
  std::vector<char> fast;
};
extern "C" int pm_batchpir_group_create(pm_batchpir** clients, uint32_t S, pm_batchpir_group** out) {
  if (!clients || !S || !out) return fail(PM_EINVAL, "NULL argument");
  for (uint32_t i = 0; i < S; ++i) {
    if (!clients[i]) return fail(PM_EINVAL, "NULL client");
    CHK(db_guard(&clients[i]->e));
    const Engine& a = clients[0]->e;
    const Engine& b = clients[i]->e;
    if (a.db.get() != b.db.get() || a.P != b.P || a.E != b.E || a.N != b.N || a.shard != b.shard ||
        a.nshards != b.nshards || b.ctx->device != a.ctx->device || !b.is_batch)
      return fail(PM_EINVAL, "grouped clients must be batch PIR clients of one server on one device");
    for (uint32_t j = 0; j < i; ++j)
      if (clients[j] == clients[i]) return fail(PM_EINVAL, "a client appears twice");
  }
  pm_batchpir_group* h = new pm_batchpir_group();
  for (uint32_t i = 0; i < S; ++i) h->G.es.push_back(&clients[i]->e);
  h->fast.assign(S, 0);
  for (uint32_t i = 0; i < S; ++i) {
    const hipError_t e = hipStreamSynchronize(clients[i]->e.ctx->stream);
    if (e != hipSuccess) { delete h; return fail(PM_EHIP, hipGetErrorString(e)); }
  }
  if (int r = group_init(h->G, clients[0]->e.ctx)) { delete h; return r; }
  *out = h;
  return 0;
}
extern "C" void pm_batchpir_group_destroy(pm_batchpir_group* h) { delete h; }
extern "C" int pm_batchpir_group_preprocessing(pm_batchpir_group* h) {
  if (!h) return fail(PM_EINVAL, "NULL argument");
  for (Engine* e : h->G.es) CHK(client_guard(e));
  // SimpleBatchPianoPIR.Preprocessing (batch-pir.go:119-155) of every client,
  // as ONE launch set: each partition's K clients fold side by side
  return group_prep(h->G, std::vector<char>(h->G.S, 1), nullptr);
}
extern "C" int pm_batchpir_group_query(pm_batchpir_group* h, const uint64_t* ids, uint64_t n, uint64_t* out,
                                       uint8_t* ok) {
  if (!h || (!ids && n) || (!out && n)) return fail(PM_EINVAL, "NULL argument");
  StepGroup& G = h->G;
  const uint64_t E = G.E;
  for (uint32_t s = 0; s < G.S; ++s) CHK(client_guard(G.es[s]));   // before any client's state moves
  for (uint32_t s = 0; s < G.S; ++s) {   // bucketing; clients at a partition's budget go alone
    Engine* e = G.es[s];
    bool f = false;
    CHK(bq_prepare(e, ids + (uint64_t)s * n, n, &f));
    h->fast[s] = f;
    if (!f)
      CHK(batch_query_impl(e, ids + (uint64_t)s * n, n, out + (uint64_t)s * n * E, nullptr, 0, nullptr, nullptr,
                           ok ? ok + (uint64_t)s * n : nullptr));
  }
  CHK(group_step(G, h->fast));
  for (uint32_t s = 0; s < G.S; ++s) {
    if (!h->fast[s]) continue;
    Engine* e = G.es[s];
    CHK(group_collect(G, s));
    bq_emit_fast(e, ids + (uint64_t)s * n, n, out + (uint64_t)s * n * E, nullptr, nullptr,
                 ok ? ok + (uint64_t)s * n : nullptr);
    CHK(bq_tail(e, n));
  }
  return 0;
}

// ---- GetVertexInfo of many graph sessions served together (the plugin API) --
// S private sessions of one server DB (pm_graph_create_session): every
// pm_graph_group_get_vertex_info call makes, for each session s, exactly the
// pm_graph_get_vertex_info call of its own ids and query (GetVertexInfo,
// private-search.go:441-506: ONE SimpleBatchPianoPIR.Query of all its ids, the
// decode, the success count), with all sessions' sub-queries in ONE shared
// step on sessions[0]'s stream and each row scored against its own session's
// query (PmPart::qv pointing into the group's query buffer).  A session whose
// bucketing leaves the one-step path (a partition at its query budget, fewer
// ids than partitions, more than step_max_sub_per_part() per partition) is
// served alone by batch_query_impl, as pm_graph_get_vertex_info serves it.
// The rows come back whole (rows_partial = false: the caller reads the vectors
// too) in the step's pinned result buffer and the distances and statuses in
// its headers, so the call adds one copy to the step: the S queries, up.
struct pm_graph_group {
  StepGroup G;
  std::vector<pm_graph*> gs;
  std::vector<uint64_t> uid;   // Engine::uid of each session's client when its parts were copied
  std::vector<char> fast;
  std::vector<uint8_t> okv;
  std::vector<float> dv;
};
// A session re-preprocessed by pm_graph_preprocess has a new client: its parts replace the old one's.
static int gvi_group_refresh(pm_graph_group* h) {
  StepGroup& G = h->G;
  bool changed = false;
  for (uint32_t s = 0; s < G.S; ++s) {
    pm_graph* g = h->gs[s];
    CHK(check_session(g));
    if (!g->pir) return fail(PM_EINVAL, "session " + std::to_string(s) + " is not preprocessed");
    Engine* e = &g->pir->e;
    if (e->uid == h->uid[s]) continue;
    if (e->P != G.P || e->E != G.E || e->maxPH != G.maxPH || e->maxSS != G.maxSS || e->nshards != 1)
      return fail(PM_EINVAL, "session " + std::to_string(s) + " is no longer a client of the group's server DB");
    G.es[s] = e;
    h->uid[s] = e->uid;
    changed = true;
  }
  if (changed) CHK(group_upload_parts(G));
  return 0;
}
// Entry2VectorAndNeighbors (private-search.go:418-439) + the success count (:483-497) of session g's n ids
static void gvi_group_decode(pm_graph* g, const uint64_t* ids, uint64_t n, const uint8_t* okv, const float* dv,
                             float* vecs, uint32_t* nbrs, uint8_t* ok, float* dist) {
  const uint64_t dim = g->dim, m = g->m;
  uint32_t tmp[64];
  for (uint64_t i = 0; i < n; ++i) {
    const char* r = (const char*)g->rowp[i];
    if (vecs) memcpy(vecs + i * dim, r, dim * 4);
    if (nbrs) memcpy(nbrs + i * m, r + dim * 4, m * 4);
    if (memcmp(r + dim * 4, g->true_nb(ids[i], tmp), m * 4) == 0) g->succ++;
    if (ok) ok[i] = okv[i];
    if (dist) dist[i] = dv[i];
  }
}
extern "C" int pm_graph_group_create(pm_graph** sessions, uint32_t S, pm_graph_group** out) {
  if (!sessions || !S || !out) return fail(PM_EINVAL, "NULL argument");
  for (uint32_t i = 0; i < S; ++i) {   // by address first: nothing is read through a pointer given twice
    if (!sessions[i]) return fail(PM_EINVAL, "NULL session");
    for (uint32_t j = 0; j < i; ++j)
      if (sessions[j] == sessions[i]) return fail(PM_EINVAL, "a session appears twice");
  }
  for (uint32_t i = 0; i < S; ++i) {
    const pm_graph* g = sessions[i];
    const std::string who = "session " + std::to_string(i);
    if (g->nonprivate) return fail(PM_EINVAL, who + " is not private: a group fetches through the batch PIR");
    if (g->nshards > 1) return fail(PM_EINVAL, who + " is sharded: a sharded graph searches through pm_search_loop_sharded");
    if (!g->lost.empty()) return fail(PM_EINVAL, who + ": session state lost: " + g->lost);
    if (!g->pir) return fail(PM_EINVAL, who + " is not preprocessed");
    if (g->ctx->device != sessions[0]->ctx->device) return fail(PM_EINVAL, "grouped sessions must be on one device");
    const Engine& a = sessions[0]->pir->e;
    const Engine& b = g->pir->e;
    if (a.db.get() != b.db.get() || a.P != b.P || a.E != b.E || a.N != b.N || g->n != sessions[0]->n ||
        g->dim != sessions[0]->dim || g->m != sessions[0]->m || b.nshards != 1 || !b.is_batch)
      return fail(PM_EINVAL, "grouped sessions must be clients of one server DB");
    for (uint32_t j = 0; j < i; ++j)
      if (sessions[j]->ctx == g->ctx) return fail(PM_EINVAL, "grouped sessions need distinct contexts");
  }
  pm_graph_group* h = new pm_graph_group();
  StepGroup& G = h->G;
  h->gs.assign(sessions, sessions + S);
  h->fast.assign(S, 0);
  G.dim = (uint32_t)sessions[0]->dim;
  G.rows_partial = false;   // whole rows: the caller reads the vectors too
  auto init = [&]() -> int {
    HIPCHK(hipSetDevice(sessions[0]->ctx->device));
    for (uint32_t i = 0; i < S; ++i) HIPCHK(hipStreamSynchronize(sessions[i]->ctx->stream));
    const uint64_t qbytes = (uint64_t)S * G.dim * 4;
    CHK(G.qbuf.reserve(qbytes));
    CHK(G.qstage.reserve(qbytes));
    HIPCHK(hipMemset(G.qbuf.p, 0, qbytes));   // the rows of a call without queries are scored against zeros, unread
    for (uint32_t i = 0; i < S; ++i) {
      G.es.push_back(&sessions[i]->pir->e);
      h->uid.push_back(sessions[i]->pir->e.uid);
      G.qv.push_back(G.qbuf.as<float>() + (uint64_t)i * G.dim);
    }
    return group_init(G, sessions[0]->ctx);
  };
  if (int r = init()) { delete h; return r; }
  *out = h;
  return 0;
}
extern "C" void pm_graph_group_destroy(pm_graph_group* h) { delete h; }

extern "C" int pm_graph_group_get_vertex_info(pm_graph_group* h, const uint64_t* ids, const uint64_t* offs, float* vecs,
                                              uint32_t* nbrs, uint8_t* ok, const float* queries, float* dist) {
  if (dist && !queries) return fail(PM_EINVAL, "dist needs the queries");
  if (!h || !offs) return fail(PM_EINVAL, "NULL argument");
  StepGroup& G = h->G;
  const uint32_t S = G.S;
  uint32_t live = 0, bad_s = 0;
  uint64_t max_n = 0, end = 0, bad_i = 0;
  if (pmgvi::walk(offs, S, &live, &max_n, &end, &bad_s) != pmgvi::OFFS_OK)
    return fail(PM_EINVAL, "offs descends at session " + std::to_string(bad_s));
  if (live && !ids) return fail(PM_EINVAL, "NULL argument");
  // every refusal comes before any session's state moves
  for (uint32_t s = 0; s < S; ++s) {
    CHK(check_session(h->gs[s]));
    if (!h->gs[s]->pir) return fail(PM_EINVAL, "session " + std::to_string(s) + " is not preprocessed");
  }
  if (pmgvi::check_ids(ids, offs, S, h->gs[0]->n, &bad_s, &bad_i) != pmgvi::OFFS_OK)
    return fail(PM_EINVAL, "session " + std::to_string(bad_s) + ": vertex id " + std::to_string(ids[bad_i]) + " out of range");
  if (!live) return 0;
  auto t_call = Clock::now();
  pm_ctx* c = G.c;
  HIPCHK(hipSetDevice(c->device));
  CHK(gvi_group_refresh(h));
  const uint64_t dim = G.dim, m = h->gs[0]->m;
  if (queries) {   // all sessions' queries in one copy, ahead of the step on its stream
    memcpy(G.qstage.p, queries, (uint64_t)S * dim * 4);
    HIPCHK(hipMemcpyAsync(G.qbuf.p, G.qstage.p, (uint64_t)S * dim * 4, hipMemcpyHostToDevice, c->stream));
  }
  h->okv.resize(max_n);
  h->dv.resize(max_n);
  bool q_landed = !queries;   // a session served alone reads its query on its own stream
  for (uint32_t s = 0; s < S; ++s) {   // bucketing; sessions off the one-step path go alone, now
    const pmgvi::Slice sl = pmgvi::slice(offs, s);
    h->fast[s] = 0;
    if (!sl.n) continue;   // sits the call out
    pm_graph* g = h->gs[s];
    Engine* e = G.es[s];
    const uint64_t* sid = ids + sl.off;
    g->total += sl.n;   // totalQueryNum (:443)
    g->rowp.resize(sl.n);
    e->rows_partial = false;
    bool f = false;
    CHK(bq_prepare(e, sid, sl.n, &f));
    h->fast[s] = f;
    if (f) continue;
    if (!q_landed) { HIPCHK(hipStreamSynchronize(c->stream)); q_landed = true; }
    CHK(batch_query_impl(e, sid, sl.n, nullptr, queries ? G.qv[s] : nullptr, (uint32_t)dim, queries ? h->dv.data() : nullptr,
                         g->rowp.data(), h->okv.data()));
    gvi_group_decode(g, sid, sl.n, h->okv.data(), h->dv.data(), vecs ? vecs + sl.off * dim : nullptr,
                     nbrs ? nbrs + sl.off * m : nullptr, ok ? ok + sl.off : nullptr, dist ? dist + sl.off : nullptr);
  }
  if (pmgvi::shared_steps(h->fast.data(), S)) {
    CHK(group_step(G, h->fast));
    c->host_add(HT_GVI_GROUP_STEPS, 0.0);
    for (uint32_t s = 0; s < S; ++s) {
      if (!h->fast[s]) continue;
      const pmgvi::Slice sl = pmgvi::slice(offs, s);
      pm_graph* g = h->gs[s];
      Engine* e = G.es[s];
      const uint64_t* sid = ids + sl.off;
      CHK(group_collect(G, s));
      bq_emit_fast(e, sid, sl.n, nullptr, h->dv.data(), g->rowp.data(), h->okv.data());
      CHK(bq_tail(e, sl.n));
      gvi_group_decode(g, sid, sl.n, h->okv.data(), h->dv.data(), vecs ? vecs + sl.off * dim : nullptr,
                       nbrs ? nbrs + sl.off * m : nullptr, ok ? ok + sl.off : nullptr, dist ? dist + sl.off : nullptr);
    }
  }
  c->host_add(HT_GVI_GROUP, ms_since(t_call));
  return 0;
}

// pm_graph_preprocess (PIRGraphInfo.Preprocess, private-search.go:355-412, then
// GetStartVertex, :508-531) of every session: the sessions that are clients of
// a base get their new clients first and are folded as ONE launch set
// (prep_clients, as pm_batchpir_group_preprocessing); a base, which packs and
// uploads its own server DB, and DummyPreprocessing sessions go through
// pm_graph_preprocess itself.
extern "C" int pm_graph_group_preprocess(pm_graph_group* h) {
  if (!h) return fail(PM_EINVAL, "NULL argument");
  StepGroup& G = h->G;
  for (uint32_t s = 0; s < G.S; ++s) CHK(check_session(h->gs[s]));
  HIPCHK(hipSetDevice(G.c->device));
  std::vector<Engine*> who;
  std::vector<pm_graph*> folded, alone;
  for (pm_graph* g : h->gs) {
    if (!g->server || g->skipPrep) { alone.push_back(g); continue; }
    delete g->pir; g->pir = nullptr;
    CHK(pm_batchpir_create_client(g->ctx, g->server, g->pir_seed, &g->pir));
    who.push_back(&g->pir->e);
    folded.push_back(g);
  }
  CHK(prep_clients(G.c, G.prep_parts, G.lp, who, nullptr));
  for (pm_graph* g : folded) CHK(graph_start_set(g));
  for (pm_graph* g : alone) {
    const pm_batchpir* old = g->pir;
    CHK(pm_graph_preprocess(g));
    if (!g->server)   // a base: the group's sessions follow it to its new server
      for (pm_graph* x : h->gs)
        if (x->server == old) x->server = g->pir;
  }
  return gvi_group_refresh(h);
}

// pm_search_loop_batched with the host work pooled (the default; PM_BATCH_POOL=0:
// one worker subset per team, run_batched_team).  The NG lock-step teams keep
// their shared steps (one stream each, the same launches), but every worker
// serves every team: when a team's step has completed, all workers take its
// sessions' host work (results, GetVertexInfo's post-processing, the search
// update, the next round's ids and bucketing), one session at a time off an
// atomic counter, and the worker that finishes the team's last session
// launches its next step -- or, at the end of a query, runs its maintenance
// and the next query's start (search.go:130-146).  A team's host phase then
// takes about 1/T of its sessions' host time instead of NG/T, so the GPU is not
// left waiting while a fixed subset of workers works through one team, and
// teams that fall behind get more of the workers.  Every session performs the
// same operations in the same order as in run_batched_team.
// PM_TEAM_TRACE=<file> (diagnostics): the pooled loop's host spans, one CSV row
// each: team, kind (0 session task, 1 step launch, 2 maintenance, 3 query
// start, 4 step in flight until seen complete), worker, start and end in us.
// Host trace of the pooled loop (PM_TEAM_TRACE=<file>): one record per task,
// launch, maintenance, query start and step flight, kept per worker (no lock
// on the serving path) and written when the loop ends.
struct TeamTrace {
  struct Rec { double t0, t1; uint32_t team, kind, worker; };
  const char* file = getenv("PM_TEAM_TRACE");
  Clock::time_point base = Clock::now();
  std::vector<std::vector<Rec>> recs;   // [worker]
  explicit TeamTrace(uint32_t workers) { if (file) { recs.resize(workers); for (auto& v : recs) v.reserve(1 << 16); } }
  double now() const { return std::chrono::duration<double, std::micro>(Clock::now() - base).count(); }
  static inline thread_local uint32_t tl_worker = 0;   // the calling worker (set when it starts)
  void add(double t0, uint32_t team, uint32_t kind, uint32_t /*worker*/) {
    if (!file) return;
    recs[tl_worker].push_back({t0, now(), team, kind, tl_worker});
  }
  ~TeamTrace() {
    if (!file) return;
    if (FILE* f = fopen(file, "w")) {
      fprintf(f, "team,kind,worker,t0_us,t1_us\n");
      for (auto& v : recs)
        for (auto& r : v) fprintf(f, "%u,%u,%u,%.2f,%.2f\n", r.team, r.kind, r.worker, r.t0, r.t1);
      fclose(f);
    }
  }
};
enum : int { kTeamStart, kTeamOpen, kTeamBusy, kTeamFlight, kTeamPrep, kTeamDone };
constexpr uint32_t kNoSession = ~0u;
struct PoolTeam {
  StepGroup G;
  pm_graph** gs = nullptr;
  uint32_t S = 0, s0 = 0;
  std::vector<char> fast, need_prep;
  std::vector<double> mt;
  std::atomic<uint64_t> qi{0};     // the team's current query (read by the merged maintenance's worker)
  int st = 0;                      // its current round
  bool begin = false;              // the open phase: a query's start (true) or a round's results
  std::atomic<int> state{kTeamStart};
  std::unique_ptr<std::atomic<uint32_t>[]> lane;   // per worker w: sessions w, w + T, ... taken so far
  std::atomic<uint32_t> ndone{0};
  Clock::time_point launched, prep_since;
  double launched_us = 0;
  uint32_t id = 0;
};
namespace pmh {
// Streams of the lock-step teams.  A team's steps ran on its first session's
// context stream, and every session context creates its stream when it is
// made: HIP maps streams onto the process's GPU_MAX_HW_QUEUES (4) hardware
// queues in creation order, so with 72 sessions per team the four teams'
// streams (sessions 0, 72, 144, 216) could all land on ONE hardware queue,
// whose in-order packets serialise the teams' kernels.  The teams get streams
// of their own instead, created back to back once per device (so they take
// distinct hardware queues), swapped into the team's context for the loop
// (the context streams where none can be created).
hipStream_t team_stream(int dev, uint32_t t) {
  static std::mutex mu;
  static std::vector<hipStream_t> pool[64];
  if (dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  std::vector<hipStream_t>& v = pool[dev];
  if (v.empty()) {
    for (int i = 0; i < 8; ++i) {
      hipStream_t st = nullptr;
      if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) st = nullptr;
      if (!st) break;
      v.push_back(st);
    }
  }
  return v.empty() ? nullptr : v[t % v.size()];
}

int run_batched_pool(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k, int step, int parallel,
                            uint32_t NG, uint32_t T, int64_t* answers, double* mt_out) {
  std::vector<StreamSwap> swaps(NG);   // destroyed after `teams` (declared first): streams drained, restored
  std::vector<std::unique_ptr<PoolTeam>> teams;
  DevBuf prep_buf;   // the merged maintenance's parts
  std::mutex prep_mu;
  // Maintenance (the end-of-query re-preprocessing, private-search.go:226-232)
  // of the teams that need it at the same query runs as ONE launch set: a team
  // whose clients need it after query Q waits (kTeamPrep) until every other
  // team has finished query Q (it waits at Q too, has moved past Q, or is
  // done); the teams waiting at Q are then re-preprocessed together.  The set
  // is a function of the sessions' triggers alone (no timeout: the bench's
  // 256 sessions always fold in one launch, which the headline parity test
  // asserts), and no wait is unbounded: every other team is running its query
  // Q.  The maintenance kernels fill the GPU, so teams' maintenances run one
  // after another either way; merged, the teams also resume together instead
  // of finishing the timed work one after another with the GPU partly idle.
  struct Release {
    std::vector<std::unique_ptr<PoolTeam>>& t;
    ~Release() { for (auto& x : t) team_release(x->gs, x->S); }
  } release{teams};
  for (uint32_t g = 0; g < NG; ++g) {
    const uint32_t s0 = (uint32_t)((uint64_t)S * g / NG), s1 = (uint32_t)((uint64_t)S * (g + 1) / NG);
    teams.emplace_back(new PoolTeam());
    PoolTeam& t = *teams.back();
    t.gs = gs + s0; t.S = s1 - s0; t.s0 = s0; t.id = g;
    t.fast.assign(t.S, 0); t.need_prep.assign(t.S, 0); t.mt.assign(t.S, 0.0);
    t.lane.reset(new std::atomic<uint32_t>[T]);
    for (uint32_t w = 0; w < T; ++w) t.lane[w].store(0);
    CHK(team_init(t.G, t.gs, t.S));
    swaps[g].swap_in(t.G.c, team_stream(t.G.c->device, g));
    static const int stage = [] { const char* e = getenv("PM_DESC_STAGE"); return e ? atoi(e) : 1; }();
    t.G.stage_on = stage != 0;
    t.G.stg.resize(t.S);
  }
  const uint32_t dim = (uint32_t)gs[0]->dim;
  TeamTrace tr(T);
  std::atomic<int> err{0};
  std::atomic<uint32_t> finished{0};
  std::string err_msg;
  std::mutex err_mu;
  auto set_err = [&](int rc, uint32_t s) {
    std::lock_guard<std::mutex> lk(err_mu);
    int z = 0;
    if (rc && err.compare_exchange_strong(z, rc)) err_msg = "session " + std::to_string(s) + ": " + pm_last_error();
  };
  // the team's phase opens: its sessions' tasks become available
  auto open = [&](PoolTeam& t, bool begin) {
    t.begin = begin;
    t.ndone.store(0, std::memory_order_relaxed);
    for (uint32_t w = 0; w < T; ++w) t.lane[w].store(0, std::memory_order_release);
    t.state.store(kTeamOpen, std::memory_order_release);
  };
  // a session of the open phase: worker w's own lane first (sessions i = w mod
  // T: the same worker, hence core, serves a session every round and finds its
  // search state and prefetched rows in cache), then the other lanes' leftovers
  auto claim = [&](PoolTeam& t, uint32_t w) -> uint32_t {
    for (uint32_t j = 0; j < T; ++j) {
      const uint32_t l = (w + j) % T;
      if (l >= t.S) continue;
      if (t.lane[l].load(std::memory_order_relaxed) * T + l >= t.S) continue;
      const uint32_t i = t.lane[l].fetch_add(1, std::memory_order_acq_rel) * T + l;
      if (i < t.S) return i;
    }
    return kNoSession;
  };
  // SearchKNN begin for every session of the team: queries and start-set
  // distances in one upload, one k_l2_rows launch and one download
  auto start_query = [&](PoolTeam& t) -> int {
    const double t0 = tr.now();
    float* qst = t.G.qstage.as<float>();
    for (uint32_t i = 0; i < t.S; ++i) {
      pm_graph* g = t.gs[i];
      knn_reset(g);
      g->t_init = Clock::now();
      memcpy(qst + (uint64_t)i * dim, queries + ((uint64_t)(t.s0 + i) * q + t.qi) * dim, (size_t)dim * 4);
    }
    CHK(group_start_dist(t.G, t.gs));
    tr.add(t0, t.id, 3, 0);
    open(t, true);
    return 0;
  };
  // one session's share of the open phase (run_batched_team's per-session work)
  auto task = [&](PoolTeam& t, uint32_t i, int64_t* stp) -> int {
    pm_graph* g = t.gs[i];
    if (t.begin) {
      knn_begin_finish(g, parallel, 0, t.G.qstage.as<float>() + (uint64_t)t.S * dim + (uint64_t)i * t.G.ns);
    } else {
      // the next session of this worker's lane, one task ahead (prefetch_session)
      if (i + T < t.S && t.fast[i + T] && !t.G.comb) prefetch_session(t.G, i + T, t.gs[i + T]);
      if (g->graph) {   // the ground-truth rows of the success check (gvi_post), requested before the results' reads
        const uint64_t m = g->m;
        for (size_t b = 0; b < g->batch.size(); ++b) {
          const char* gr = (const char*)&g->graph[(uint64_t)g->batch[b] * m];
          __builtin_prefetch(gr);
          __builtin_prefetch(gr + m * 4 - 1);
        }
      }
      if (t.fast[i]) CHK(group_collect(t.G, i));   // complete: only the tokens and host mirrors
      CHK(gvi_post(g, true, t.fast[i]));
      knn_update(g, t.st);
      if (t.st + 1 == step) {   // top k, maintenance trigger (private-search.go:226-232)
        knn_end(g, k, answers + ((uint64_t)(t.s0 + i) * q + t.qi) * k, stp);
        Engine* e = &g->pir->e;
        t.need_prep[i] = e->FBN + (uint64_t)step * (uint64_t)parallel + 10 >= e->Support;
        return 0;
      }
    }
    knn_batch(g, parallel, 0);   // the next round's ids -> sub-queries
    bool f = false;
    CHK(gvi_pre(g, true, &f));
    t.fast[i] = f;
    if (f) group_stage_session(t.G, i);
    return 0;
  };
  // the worker that completed the phase's last session moves the team on
  auto advance = [&](PoolTeam& t) -> int {
    if (t.begin || t.st + 1 < step) {   // a round's ids are bucketed: its shared step
      t.st = t.begin ? 0 : t.st + 1;
      const double t0 = tr.now();
      CHK(group_step(t.G, t.fast));
      tr.add(t0, t.id, 1, 0);
      t.launched = Clock::now();
      t.launched_us = tr.now();
      t.state.store(kTeamFlight, std::memory_order_release);
      return 0;
    }
    const double t0 = tr.now();
    bool any = false;
    for (char c : t.need_prep) any |= c != 0;
    if (any) {   // with the other teams' (above)
      t.prep_since = Clock::now();
      t.state.store(kTeamPrep, std::memory_order_release);
      return 0;
    }
    CHK(group_prep(t.G, t.need_prep, &t.mt));   // the triggered clients' preprocessings as one launch set
    tr.add(t0, t.id, 2, 0);
    if (++t.qi == q) {
      t.state.store(kTeamDone, std::memory_order_release);
      finished.fetch_add(1);
      return 0;
    }
    return start_query(t);
  };
  std::vector<int64_t> steps_buf((size_t)T * std::max(k, 1));
  const int dev = gs[0]->ctx->device;
  auto worker = [&](uint32_t w) {
    TeamTrace::tl_worker = w;
    if (hipSetDevice(dev) != hipSuccess) { set_err(PM_EHIP, 0); return; }
    int64_t* stp = &steps_buf[(size_t)w * std::max(k, 1)];
    uint32_t idle = 0;
    while (!err.load(std::memory_order_relaxed) && finished.load(std::memory_order_acquire) < NG) {
      bool did = false;
      for (uint32_t j = 0; j < NG && !did; ++j) {
        PoolTeam& t = *teams[(w + j) % NG];
        int cur = t.state.load(std::memory_order_acquire);
        if (cur == kTeamOpen) {
          const uint32_t i = claim(t, w);
          if (i == kNoSession) continue;
          did = true;
          const double t0 = tr.now();
          int rc = task(t, i, stp);
          tr.add(t0, t.id, 0, w);
          if (rc) set_err(rc, t.s0 + i);
          if (t.ndone.fetch_add(1, std::memory_order_acq_rel) + 1 == t.S && !err.load()) {
            t.state.store(kTeamBusy, std::memory_order_relaxed);
            rc = advance(t);
            if (rc) set_err(rc, t.s0);
          }
        } else if (cur == kTeamPrep) {
          if (!prep_mu.try_lock()) continue;   // one worker runs the merged maintenance
          std::lock_guard<std::mutex> lk(prep_mu, std::adopt_lock);
          // Q: the earliest query a team waits at; the set: the teams waiting at Q,
          // once every team still running has finished query Q
          uint64_t Q = ~0ull;
          for (auto& u : teams)
            if (u->state.load(std::memory_order_acquire) == kTeamPrep) Q = std::min(Q, u->qi.load(std::memory_order_acquire));
          if (Q == ~0ull) continue;
          bool all = true;
          for (auto& u : teams) {
            const int us = u->state.load(std::memory_order_acquire);
            if (us != kTeamPrep && us != kTeamDone && u->qi.load(std::memory_order_acquire) <= Q) all = false;
          }
          if (!all) continue;
          std::vector<PoolTeam*> ts;
          for (auto& u : teams) {
            int e = kTeamPrep;
            if (u->qi.load(std::memory_order_acquire) == Q &&
                u->state.compare_exchange_strong(e, kTeamBusy, std::memory_order_acq_rel))
              ts.push_back(u.get());
          }
          if (ts.empty()) continue;
          did = true;
          const double t0 = tr.now();
          std::vector<Engine*> who;
          std::vector<double*> mts;
          for (PoolTeam* u : ts)
            for (uint32_t s = 0; s < u->S; ++s)
              if (u->need_prep[s]) { who.push_back(u->G.es[s]); mts.push_back(&u->mt[s]); }
          const int rc = prep_clients(ts[0]->G.c, prep_buf, ts[0]->G.lp, who, &mts);
          if (rc) { set_err(rc, ts[0]->s0); break; }
          for (PoolTeam* u : ts) {
            tr.add(t0, u->id, 2, w);
            if (++u->qi == q) {
              u->state.store(kTeamDone, std::memory_order_release);
              finished.fetch_add(1);
            } else {
              u->state.store(kTeamStart, std::memory_order_release);   // a worker starts its next query
            }
          }
        } else if (cur == kTeamStart || cur == kTeamFlight) {
          bool ready = cur == kTeamStart;
          if (!ready) {
            const int rc = poll_done(t.G.c, t.G.seq, &ready);
            if (rc) { set_err(rc, t.s0); break; }
            if (!ready && std::chrono::duration<double>(Clock::now() - t.launched).count() > 10.0) {
              set_err(fail(PM_EHIP, "shared step not complete after 10 s"), t.s0);
              break;
            }
          }
          if (ready && t.state.compare_exchange_strong(cur, kTeamBusy, std::memory_order_acq_rel)) {
            did = true;
            if (cur == kTeamFlight) tr.add(t.launched_us, t.id, 4, w);
            const int rc = cur == kTeamStart ? start_query(t) : (open(t, false), 0);
            if (rc) set_err(rc, t.s0);
          }
        }
      }
      if (did) {
        idle = 0;
      } else if (++idle > 32) {   // nothing to do: give the core to the workers that have work
        std::this_thread::yield();
      } else {
        __builtin_ia32_pause();   // spin politely (an SMT sibling may be a working worker)
      }
    }
  };
  std::vector<std::thread> th;
  for (uint32_t w = 1; w < T; ++w) th.emplace_back(worker, w);
  worker(0);
  for (auto& t : th) t.join();
  for (auto& t : teams) HIPCHK(hipStreamSynchronize(t->G.c->stream));
  if (err.load()) return fail(err.load(), err_msg);
  for (auto& t : teams)
    for (uint32_t s = 0; s < t->S; ++s) mt_out[t->s0 + s] = t->mt[s];
  return 0;
}

// What pm_search_loop_batched and pm_search_loop_sharded ask of their
// sessions: usable preprocessed private graphs, distinct, all clients of one
// server DB (sharded: of one shard's) on one device.
int check_loop_sessions(pm_graph** gs, uint32_t S, bool sharded) {
  for (uint32_t i = 0; i < S; ++i) {
    if (!gs[i] || !gs[i]->pir || gs[i]->nonprivate) return fail(PM_EINVAL, "sessions must be preprocessed private graphs");
    CHK(check_session(gs[i]));
    const Engine& a = gs[0]->pir->e;
    const Engine& b = gs[i]->pir->e;
    const bool shards_differ = sharded ? b.shard != a.shard || b.nshards != a.nshards : b.nshards != 1;
    if (a.db.get() != b.db.get() || a.P != b.P || a.E != b.E || gs[i]->dim != gs[0]->dim || gs[i]->m != gs[0]->m ||
        shards_differ || gs[i]->ctx->device != gs[0]->ctx->device)
      return fail(PM_EINVAL, sharded ? "sharded sessions must be clients of one shard's server DB on one device"
                                     : "batched sessions must be clients of one server DB on one device");
    for (uint32_t j = 0; j < i; ++j)
      if (gs[j] == gs[i] || gs[j]->ctx == gs[i]->ctx) return fail(PM_EINVAL, "sessions need distinct graphs and contexts");
  }
  return 0;
}

// The teams of a serving call, run concurrently: fn(g, s0, s1, Tg) serves team
// g's sessions [s0, s1) of the S with its Tg of the TT threads, on a thread of
// its own bound to the sessions' device.  Returns once every team has ended,
// with the first failed team's error.
int run_teams(pm_graph** gs, uint32_t S, uint32_t NG, uint32_t TT, const TeamFn& fn) {
  std::vector<int> rc(NG, 0);
  std::vector<std::string> msg(NG);
  std::vector<std::thread> teams;
  for (uint32_t g = 0; g < NG; ++g) {
    const uint32_t s0 = (uint32_t)((uint64_t)S * g / NG), s1 = (uint32_t)((uint64_t)S * (g + 1) / NG);
    const uint32_t Tg = std::max(1u, std::min(s1 - s0, (uint32_t)((uint64_t)TT * (g + 1) / NG - (uint64_t)TT * g / NG)));
    teams.emplace_back([&, g, s0, s1, Tg] {
      if (hipSetDevice(gs[0]->ctx->device) != hipSuccess) { rc[g] = PM_EHIP; msg[g] = "hipSetDevice"; return; }
      rc[g] = fn(g, s0, s1, Tg);
      if (rc[g]) msg[g] = pm_last_error();
    });
  }
  for (auto& t : teams) t.join();
  for (uint32_t g = 0; g < NG; ++g)
    if (rc[g]) return fail(rc[g], "group " + std::to_string(g) + ": " + msg[g]);
  return 0;
}
}  // namespace pmh

// Words of one team's records in pm_search_loop_sharded: sessions x (parallel
// x m) ids x W, W = the row words holding the neighbour list + 1.
extern "C" uint64_t pm_sharded_record_words(pm_graph* g, uint32_t sessions, int parallel) {
  if (!g || parallel <= 0) return 0;
  const uint64_t w0 = g->dim * 4 / 8, w1 = (g->dim * 4 + g->m * 4 + 7) / 8;
  return (uint64_t)sessions * (uint64_t)parallel * g->m * (w1 - w0 + 1) + 1;   // + the error word
}

// The batched serving loop over a sharded graph DB (every rank calls it with
// its own shard's sessions, the same seeds and queries).  Teams are
// pm_search_loop_batched's; each shared step ends in ONE combine of the team's
// records (see group_exchange).  combine NULL: no exchange (one shard holds
// every partition), or model_peers (synthetic graphs): the partitions of the
// other shards are answered from the graph's spec.  team_bufs (NULL: the
// library allocates): one device buffer per team of pm_sharded_record_words
// words, the tensors a torch.distributed combine all-reduces in place.
extern "C" int pm_search_loop_sharded(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k, int step,
                                      int parallel, uint32_t ngroups, uint32_t nthreads, pm_combine_fn combine,
                                      void* user, uint64_t* const* team_bufs, int model_peers, int64_t* answers,
                                      double* wall_s, double* online_s, double* maint_s) {
  if (!gs || !S || (!queries && q) || (!answers && q)) return fail(PM_EINVAL, "NULL argument");
  CHK(check_loop_sessions(gs, S, true));
  if (model_peers && !gs[0]->synth) return fail(PM_EINVAL, "modelled peers need the synthetic graph (its rows are computable)");
  if (model_peers && combine) return fail(PM_EINVAL, "pass a combine or model_peers, not both");
  if (gs[0]->pir->e.nshards > 1 && !combine && !model_peers)
    return fail(PM_EINVAL, "a sharded graph needs a combine (or model_peers)");
  if (gs[0]->m > 64) return fail(PM_EINVAL, "sharded search: m <= 64");
  const uint32_t NG = std::max(1u, std::min(ngroups ? ngroups : 1u, S));
  const uint32_t TT = std::max(NG, nthreads ? nthreads : std::min<uint32_t>(S, 16u));
  ShardComb comb;
  comb.fn = combine;
  comb.user = user;
  comb.model_peers = model_peers != 0;
  comb.NG = NG;
  comb.bufs = team_bufs;
  std::vector<double> mt(S, 0.0);
  auto t0 = Clock::now();
  const int rc = run_teams(gs, S, NG, TT, [&](uint32_t g, uint32_t s0, uint32_t s1, uint32_t Tg) {
    const int r = run_batched_team(gs + s0, s1 - s0, queries + (uint64_t)s0 * q * gs[0]->dim, q, k, step, parallel, Tg,
                                   answers + (uint64_t)s0 * q * (uint64_t)k, mt.data() + s0, &comb, g);
    if (r) comb.abort.store(true);
    return r;
  });
  const double wall = std::chrono::duration<double>(Clock::now() - t0).count();
  if (rc) return rc;
  if (wall_s) *wall_s = wall;
  for (uint32_t s = 0; s < S; ++s) {
    if (online_s) online_s[s] = wall - mt[s];
    if (maint_s) maint_s[s] = mt[s];
  }
  return 0;
}

// pm_devloop.cpp — the device loop (pm_drl.hip) and pm_search_loop_batched,
// which chooses between it, the pooled loop and the team loop.  Needs
// pm_ctx.cpp, pm_engine.cpp, pm_search.cpp and pm_group.cpp.
#include "pm_engine.h"

// ---- the device loop (pm_drl.hip) -------------------------
// The batched serving loop with each team's rounds chained on the GPU: per
// query and team, [queries -> qbuf, start-set L2, k_team_round BEGIN], then per
// round [k_match_resolve_s, k_answer_p, k_team_round MID / END] on the team's
// stream, enqueued ahead; the host only decides the maintenance between
// queries (its schedule is a function of the counters alone) and runs it as
// one launch set of every triggered client, like run_batched_pool.  Taken when
// drl_plan shows that every round of the call would take the host's one-step
// path (no partition at its query budget, no batch-layer re-preprocessing);
// otherwise, or with pm_set_option("device_loop", 0) / PM_DEVICE_LOOP=0, the
// host loop serves the call.  Every session's answers, counters and state
// equal the host loop's and the oracle's: every branch of the round kernel
// and every limit of drl_plan at its smallest shape in
// tests/test_gpu_devloop_rounds.py (cases and the oracle's evidence that each
// reaches its branch: tests/devloop_cases.py, test_devloop_cases.py), the
// headline shape in tests/test_gpu_parity.py and test_gpu_headline.py.
static bool device_loop_on() {
  const int o = g_device_loop.load();
  if (o >= 0) return o != 0;
  static const int env = [] { const char* e = getenv("PM_DEVICE_LOOP"); return e ? atoi(e) : 1; }();
  return env != 0;
}
static uint32_t pow2_at_least(uint64_t x) { uint32_t c = 1; while (c < x) c *= 2; return c; }

struct DrlShape { uint32_t n = 0, qn = 0, kcap = 0, cmask = 0; };
// Whether the device loop can serve the call, and its shape.  The counters
// FinishedBatchNum / QueriesMadeInPartition advance by fixed amounts per round
// (n / B, queryNumToMake) and reset at the harness's maintenance
// (private-search.go:226-232), so the whole call's schedule is known here: a
// query is chained on the device only if no round of it can reach a
// partition's budget (FinishedQueryNum + real sub-queries >= MaxQueryNum:
// bq_prepare's slow path; FinishedQueryNum <= QueriesMadeInPartition always)
// or the batch layer's trigger (QueriesMadeInPartition >= MaxQueryNum - 2).
static bool drl_plan(pm_graph** gs, uint32_t S, uint64_t q, int k, int step, int parallel, DrlShape* sh) {
  if (!device_loop_on() || S == 0 || step <= 0 || parallel <= 0 || k <= 0 || (uint32_t)parallel > pmk::kDrlMaxParallel)
    return false;
  const pm_graph* g0 = gs[0];
  const Engine& e0 = g0->pir->e;
  const uint64_t m = g0->m, n = (uint64_t)parallel * m, P = e0.P;
  if (m == 0 || m > 64 || n > pmk::kDrlMaxN || n * m > pmk::kDrlMaxNM || P == 0 || P > 64) return false;
  const uint64_t qn = n / P;
  if (qn == 0 || qn > pmk::step_max_sub_per_part() || e0.B == 0) return false;
  const uint64_t kcap = pow2_at_least((uint64_t)parallel + (uint64_t)step * n);
  if (kcap > pmk::kDrlMaxKcap || (uint64_t)k > kcap || pmk::team_round_lds(kcap, n, m) > 64 * 1024) return false;
  uint64_t maxq = ~0ull;
  for (uint32_t i = 0; i < S; ++i) {
    const pm_graph* g = gs[i];
    const Engine& e = g->pir->e;
    if (g->nonprivate || g->synth || !g->graph || !g->dvec->p || e.nshards != 1 || e.P != P || e.B != e0.B ||
        e.pf_off != g->dim * 4 || g->dim > 0xffffffffull || g->n >= 0xffffffffull || e.PS >= 0xffffffffull)
      return false;
    uint64_t mq = ~0ull;
    for (const PartHost& ph : e.parts) {
      mq = std::min(mq, ph.maxq64);
      maxq = std::max<uint64_t>(maxq == ~0ull ? 0 : maxq, ph.maxq64);   // localCache entries per partition <= MaxQueryNum
      if (ph.fqn > e.QMIP) return false;   // the bound below needs FinishedQueryNum <= QueriesMadeInPartition
    }
    uint64_t fbn = e.FBN, qmip = e.QMIP;
    for (uint64_t qi = 0; qi < q; ++qi) {
      if (qmip + (uint64_t)step * qn >= mq || qmip + (uint64_t)(step - 1) * qn + 2 >= e.parts[0].maxq64) return false;
      fbn += (uint64_t)step * (n / e.B);
      qmip += (uint64_t)step * qn;
      if (fbn + (uint64_t)step * (uint64_t)parallel + 10 >= e.Support) fbn = qmip = 0;
    }
  }
  sh->n = (uint32_t)n; sh->qn = (uint32_t)qn; sh->kcap = (uint32_t)kcap;
  sh->cmask = pow2_at_least(2 * std::max<uint64_t>(maxq, 1)) - 1;
  return true;
}

// The localCache indexes on the device for the loop: the device copy is made
// from the host's FlatMaps where it is not current (empty after a
// maintenance: a memset), and from then on the device copy is the truth.
static int ensure_dev_cache(Engine* e, uint32_t cmask, hipStream_t st) {
  const uint64_t cap = (uint64_t)cmask + 1, words = e->P * cap;
  if (e->dcache_cmask != cmask || !e->dcache.p) {
    if (e->cache_on_dev) CHK(ensure_host_cache(e));
    CHK(e->dcache.reserve(words * 8));
    e->dcache_cmask = cmask;
    e->dcache_valid = false;
  }
  if (!e->dcache_valid) {
    bool any = false;
    for (const PartHost& ph : e->parts) any |= ph.cache.count > 0;
    if (!any) {
      HIPCHK(hipMemsetAsync(e->dcache.p, 0, words * 8, st));
    } else {
      std::vector<uint64_t> t(words, 0);
      for (uint64_t p = 0; p < e->P; ++p)
        e->parts[p].cache.for_each([&](uint64_t key, uint32_t val) {
          uint64_t* tp = &t[p * cap];
          for (uint32_t i = pm::drl_hash((uint32_t)key) & cmask;; i = (i + 1) & cmask)
            if (!tp[i]) { tp[i] = ((uint64_t)val << 32) | (uint64_t)((uint32_t)key + 1u); break; }
        });
      HIPCHK(hipStreamSynchronize(st));
      HIPCHK(hipMemcpy(e->dcache.p, t.data(), words * 8, hipMemcpyHostToDevice));
    }
    e->dcache_valid = true;
  }
  e->cache_on_dev = true;
  return 0;
}

struct DrlTeam {
  StepGroup G;
  pm_graph** gs = nullptr;
  uint32_t S = 0, s0 = 0, nsub = 0;
  DevBuf sess, dummy, batch, heap, ktab, knb, kdist, kid, ctabp, answers, gid, out, allq, part_bytes, step_bytes,
      step_real, stamps;
  DrlArgs A{};
  hipEvent_t ev_end = nullptr;
  HostBuf prep_stage, parts_stage;               // pinned stages of the asynchronous maintenance (run_batched_dev)
  hipEvent_t prep_stage_ev = nullptr, parts_stage_ev = nullptr;
  DevBuf prep_buf;
  uint32_t seq = 0;                              // shared steps built so far (step_bytes rows)
  std::vector<std::pair<size_t, uint32_t>> tl;   // timed "answer" / "match_resolve" launches: (index, step)
  std::vector<char> need;
  std::vector<double> mt;
  ~DrlTeam() {
    for (hipEvent_t e : {ev_end, prep_stage_ev, parts_stage_ev})
      if (e) (void)hipEventDestroy(e);
  }
};

// The team's parts (new keys after a maintenance) up from a pinned stage on
// stream st, nothing waiting (the stage's previous copy is waited for first).
static int group_upload_parts_async(StepGroup& G, hipStream_t st, HostBuf& stage, hipEvent_t& ev) {
  if (ev) HIPCHK(hipEventSynchronize(ev));
  else HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  const size_t np = (size_t)G.S * G.Pl;
  CHK(stage.reserve(std::max<size_t>(1, np) * sizeof(PmPart)));
  PmPart* v = stage.as<PmPart>();
  for (uint32_t s = 0; s < G.S; ++s)
    for (uint32_t li = 0; li < G.Pl; ++li) {
      PmPart d = G.es[s]->parts[G.lp[li]].d;
      d.qv = G.qv.empty() ? nullptr : G.qv[s];
      v[(size_t)s * G.Pl + li] = d;
    }
  HIPCHK(hipMemcpyAsync(G.parts_d.p, v, np * sizeof(PmPart), hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ev, st));
  G.gen.resize(G.S);
  for (uint32_t s = 0; s < G.S; ++s) G.gen[s] = G.es[s]->prep_gen;
  return 0;
}

static int drl_team_init(DrlTeam& T, pm_graph** gs, uint32_t S, uint32_t s0, const float* queries, uint64_t q, int k,
                         int step, int parallel, const DrlShape& sh) {
  T.gs = gs; T.S = S; T.s0 = s0;
  StepGroup& G = T.G;
  CHK(team_init(G, gs, S));
  hipStream_t st = G.c->stream;
  const pm_graph* g0 = gs[0];
  const Engine& e0 = g0->pir->e;
  const uint32_t P = (uint32_t)e0.P, m = (uint32_t)g0->m, n = sh.n, kcap = sh.kcap, dim = (uint32_t)g0->dim;
  T.nsub = S * P * sh.qn;
  if (!g0->dgraph->p) {   // the true neighbour lists (success count, start set) on the device, once per graph
    CHK(g0->dgraph->reserve(g0->n * m * 4));
    HIPCHK(hipMemcpy(g0->dgraph->p, g0->graph, g0->n * m * 4, hipMemcpyHostToDevice));
  }
  CHK(T.sess.reserve(S * sizeof(DrlSess)));
  CHK(T.dummy.reserve((uint64_t)S * P * 8));
  CHK(T.batch.reserve((uint64_t)S * n * 4));
  CHK(T.heap.reserve((uint64_t)S * kcap * 8));
  CHK(T.ktab.reserve((uint64_t)S * 2 * kcap * 8));
  CHK(T.knb.reserve((uint64_t)S * kcap * m * 4));
  CHK(T.kdist.reserve((uint64_t)S * kcap * 4));
  CHK(T.kid.reserve((uint64_t)S * kcap * 4));
  CHK(T.ctabp.reserve(S * 8));
  CHK(T.answers.reserve(std::max<uint64_t>(8, (uint64_t)S * q * k * 8)));
  // the step buffers of group_step for nsub sub-queries; the descriptor in them
  // (subs_d, sb_d) is the one the round kernels build
  CHK(G.buf.reserve(T.nsub, S * P, (G.maxPH + 63) / 64, pmk::step_match_blocks(G.maxPH), G.E));
  CHK(T.gid.reserve((uint64_t)T.nsub * 8));
  CHK(T.out.reserve(step_out_bytes(T.nsub, G.E)));
  CHK(T.allq.reserve(std::max<uint64_t>(4, (uint64_t)S * q * dim * 4)));
  CHK(T.part_bytes.reserve(P * 8));
  // host state -> device: search streams and counters, dummy counters, localCache indexes
  std::vector<DrlSess> hs(S);
  std::vector<uint64_t> dmy((uint64_t)S * P), ctp(S);
  for (uint32_t i = 0; i < S; ++i) {
    pm_graph* g = gs[i];
    Engine* e = &g->pir->e;
    hs[i] = DrlSess{g->rng.s, g->succ, 0, 0, 0, 0};
    for (uint32_t p = 0; p < P; ++p) dmy[(uint64_t)i * P + p] = e->parts[p].dummy_ctr;
    CHK(ensure_dev_cache(e, sh.cmask, st));
    ctp[i] = (uint64_t)(uintptr_t)e->dcache.p;
  }
  std::vector<uint32_t> sbv(S * P + 1);
  for (uint32_t j = 0; j <= S * P; ++j) sbv[j] = j * sh.qn;
  std::vector<double> pb(P);
  for (uint32_t p = 0; p < P; ++p) pb[p] = answer_bytes(e0.parts[p].d, G.E);
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipMemcpy(T.sess.p, hs.data(), S * sizeof(DrlSess), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(T.dummy.p, dmy.data(), dmy.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(T.ctabp.p, ctp.data(), S * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(G.buf.sb_d.p, sbv.data(), sbv.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(T.part_bytes.p, pb.data(), P * 8, hipMemcpyHostToDevice));
  if (q) HIPCHK(hipMemcpy(T.allq.p, queries + (uint64_t)s0 * q * dim, (uint64_t)S * q * dim * 4, hipMemcpyHostToDevice));
  if (G.c->timing >= 2) {   // each step's answer bytes and real sub-queries, counted by the round that builds it
    const uint64_t steps = q * (uint64_t)step;
    CHK(T.step_bytes.reserve(std::max<uint64_t>(8, steps * S * 8)));
    CHK(T.step_real.reserve(std::max<uint64_t>(4, steps * S * 4)));
    HIPCHK(hipMemsetAsync(T.step_bytes.p, 0, std::max<uint64_t>(8, steps * S * 8), st));   // accumulated by the rounds
    HIPCHK(hipMemsetAsync(T.step_real.p, 0, std::max<uint64_t>(4, steps * S * 4), st));
  }
  HIPCHK(hipEventCreateWithFlags(&T.ev_end, hipEventDisableTiming));
  if (getenv("PM_DRL_STAMPS")) {   // diagnostics: per-phase shader clocks of the MID rounds (printed at the end)
    CHK(T.stamps.reserve(16 * 8));
    HIPCHK(hipMemset(T.stamps.p, 0, 16 * 8));
  }
  DrlArgs& A = T.A;
  A.S = S; A.P = P; A.qn = sh.qn; A.n = n; A.m = m; A.parallel = (uint32_t)parallel; A.k = (uint32_t)k;
  A.E = G.E; A.dim = dim; A.kcap = kcap; A.cmask = sh.cmask; A.ns = G.ns; A.q = (uint32_t)q;
  A.N = g0->n; A.PS = e0.PS;
  A.vec16 = (G.E % 2 == 0 && dim % 4 == 0 && m % 4 == 0 && ((m / 4) & (m / 4 - 1)) == 0) ? 1u : 0u;
  A.hdr = T.out.as<PmOutHdr>();
  A.rows = (const uint64_t*)(T.out.as<char>() + (uint64_t)T.nsub * sizeof(PmOutHdr));
  A.subs = G.buf.subs_d.as<PmSub>(); A.gid = T.gid.as<uint64_t>();
  A.graph = g0->dgraph->as<uint32_t>();
  A.start_dist = G.start_dist.as<float>(); A.start_ids = G.start_ids.as<uint32_t>();
  A.sess = T.sess.as<DrlSess>(); A.dummy = T.dummy.as<uint64_t>(); A.batch = T.batch.as<uint32_t>();
  A.heap = T.heap.as<uint64_t>(); A.ktab = T.ktab.as<uint64_t>(); A.knb = T.knb.as<uint32_t>();
  A.kdist = T.kdist.as<float>(); A.kid = T.kid.as<uint32_t>(); A.ctab = T.ctabp.as<uint64_t*>();
  A.answers = T.answers.as<int64_t>(); A.part_bytes = T.part_bytes.as<double>();
  A.step_bytes = T.step_bytes.p ? T.step_bytes.as<double>() : nullptr;
  A.step_real = T.step_real.p ? T.step_real.as<uint32_t>() : nullptr;
  A.stamps = T.stamps.p ? T.stamps.as<uint64_t>() : nullptr;
  T.need.assign(S, 0);
  T.mt.assign(S, 0.0);
  return 0;
}

// One shared step of the device loop: the descriptor the last round kernel
// built, results into device memory.
static int drl_step(DrlTeam& T, const DrlShape& sh) {
  StepGroup& G = T.G;
  pm_ctx* c = G.c;
  const Engine* e0 = G.es[0];
  c->sample_now = c->sample_ctr++ % 7 == 0;   // timing level 3: group_step's sample
  PmStep S{};
  S.parts = G.parts_d.as<PmPart>();
  G.buf.fill(S, (G.maxPH + 63) / 64, pmk::step_match_blocks(G.maxPH));
  S.subs_h = S.subs;   // the descriptor is on the device already
  S.sb_h = S.sb;
  S.done = G.done.as<uint32_t>();
  e0->step_db(S);
  S.q = nullptr;   // each partition's PmPart::qv
  step_out(S, T.out.p, T.nsub);
  S.E = G.E; S.dim = G.dim; S.nsub = T.nsub; S.np = T.S * G.Pl;
  S.np_live = S.np;
  S.token = next_token(G.token);
  step_read_window(S, e0->pf_off, e0->pf_len, G.E);
  S.rows_partial = 1;   // the rows stay on the device: no host diagnostic re-reads them
  const size_t before = c->launches.size();
  // bytes: every sub-query answered (patched with the round's exact count in timing runs)
  double ans_bytes = 0;
  for (uint32_t li = 0; li < G.Pl; ++li) ans_bytes += answer_bytes(e0->parts[G.lp[li]].d, G.E) * sh.qn * T.S;
  CHK(group_step_launch(G, S, pmk::STEP_DEVICE, sh.qn, T.nsub, ans_bytes));
  for (size_t i = before; i < c->launches.size(); ++i)
    if (c->launches[i].name == "answer" || c->launches[i].name == "match_resolve" || c->launches[i].name == "hint_match")
      T.tl.emplace_back(i, T.seq - 1);   // the step the last BEGIN / MID round built (drl_round advanced seq)
  c->host_add(HT_DEV_STEPS, 0.0);
  return 0;
}

static void drl_round(DrlTeam& T, uint32_t mode, uint64_t qi) {
  pm_ctx* c = T.G.c;
  DrlArgs A = T.A;
  A.mode = mode;
  A.qi = (uint32_t)qi;
  A.seq = T.seq;   // the step this round builds (BEGIN / MID)
  if (mode != DRL_END) T.seq++;
  c->timed_ext("team_round", 0, [&](pmk::PmEvents ev) { pmk::team_round(c->stream, A, ev); }, 2);
}

// Query qi of every team, enqueued round by round across the teams (so that
// teams whose streams share a hardware queue still interleave their rounds):
// per team the queries into qbuf, the start set's distances and BEGIN, then
// per round the shared step and the round kernel (MID, END after the last).
static int drl_begin(DrlTeam& T, uint64_t qi, uint64_t q) {
  StepGroup& G = T.G;
  hipStream_t st = G.c->stream;
  const uint32_t dim = G.dim;
  HIPCHK(hipMemcpy2DAsync(G.qbuf.p, (size_t)dim * 4, T.allq.as<float>() + qi * dim, (size_t)q * dim * 4,
                          (size_t)dim * 4, T.S, hipMemcpyDeviceToDevice, st));
  const uint64_t nrows = (uint64_t)T.S * G.ns;
  if (nrows)
    G.c->timed("l2_rows", (double)nrows * G.dim * 4, [&] {
      pmk::l2_rows(st, T.gs[0]->dvec->as<float>(), G.dim, nrows, G.start_ids.as<uint32_t>(), G.qbuf.as<float>(), G.dim,
                   G.start_dist.as<float>(), G.ns);
    });
  drl_round(T, DRL_BEGIN, qi);
  return 0;
}
static int drl_query_all(std::vector<std::unique_ptr<DrlTeam>>& teams, const DrlShape& sh, uint64_t qi, uint64_t q,
                         int step) {
  for (auto& t : teams) CHK(drl_begin(*t, qi, q));
  for (int r = 0; r < step; ++r)
    for (auto& t : teams) {
      CHK(drl_step(*t, sh));
      drl_round(*t, r + 1 == step ? DRL_END : DRL_MID, qi);
    }
  HIPCHK(hipGetLastError());
  for (auto& t : teams) {
    for (uint32_t i = 0; i < t->S; ++i) {   // the host's deterministic mirrors of the rounds (bq_tail, gvi_pre)
      pm_graph* g = t->gs[i];
      Engine* e = &g->pir->e;
      e->FBN += (uint64_t)step * (sh.n / e->B);
      e->QMIP += (uint64_t)step * sh.qn;
      g->total += (uint64_t)step * sh.n;
    }
    t->G.c->host_add(HT_DEV_QUERIES, (double)t->S);
  }
  return 0;
}

// Device state -> host at the end of the call: answers, search streams and
// counters, dummy counters, FinishedQueryNum; the timed launches' bytes.
static int drl_team_finish(DrlTeam& T, uint64_t q, int k, int64_t* answers) {
  StepGroup& G = T.G;
  HIPCHK(hipStreamSynchronize(G.c->stream));
  const uint32_t S = T.S, P = (uint32_t)G.es[0]->P;
  if (q) HIPCHK(hipMemcpy(answers + (uint64_t)T.s0 * q * k, T.answers.p, (uint64_t)S * q * k * 8, hipMemcpyDeviceToHost));
  std::vector<DrlSess> hs(S);
  std::vector<uint64_t> dmy((uint64_t)S * P);
  HIPCHK(hipMemcpy(hs.data(), T.sess.p, S * sizeof(DrlSess), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(dmy.data(), T.dummy.p, dmy.size() * 8, hipMemcpyDeviceToHost));
  std::vector<uint32_t> fq(P);
  for (uint32_t i = 0; i < S; ++i) {
    pm_graph* g = T.gs[i];
    Engine* e = &g->pir->e;
    g->rng.s = hs[i].rng;
    g->succ = hs[i].succ;
    HIPCHK(hipMemcpy(fq.data(), e->fqn.p, P * 4, hipMemcpyDeviceToHost));
    for (uint32_t p = 0; p < P; ++p) {
      e->parts[p].dummy_ctr = dmy[(uint64_t)i * P + p];
      e->parts[p].fqn = fq[p];
    }
  }
  if (T.stamps.p) {
    uint64_t st[16];
    HIPCHK(hipMemcpy(st, T.stamps.p, sizeof st, hipMemcpyDeviceToHost));
    if (st[15])
      fprintf(stderr, "[pm] team_round MID phases (shader clocks per launch, %lu launches): load %.0f respond %.0f decode %.0f "
              "[ballot %.0f known %.0f rows %.0f push %.0f fence %.0f] pop+gather %.0f bucket %.0f store %.0f\n",
              (unsigned long)st[15], st[1] / (double)st[15], st[2] / (double)st[15], st[3] / (double)st[15],
              st[8] / (double)st[15], st[9] / (double)st[15], st[10] / (double)st[15], st[11] / (double)st[15],
              st[4] / (double)st[15], st[5] / (double)st[15], st[6] / (double)st[15], st[7] / (double)st[15]);
  }
  pm_ctx* c = G.c;
  if (!T.tl.empty() && T.step_bytes.p) {   // the timed steps' exact answer bytes / real sub-queries
    std::vector<double> by((uint64_t)T.seq * S);
    std::vector<uint32_t> nr((uint64_t)T.seq * S);
    HIPCHK(hipMemcpy(by.data(), T.step_bytes.p, by.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(nr.data(), T.step_real.p, nr.size() * 4, hipMemcpyDeviceToHost));
    for (auto& [idx, sq] : T.tl) {
      if (idx >= c->launches.size() || sq >= T.seq) continue;
      double b = 0, r = 0;
      for (uint32_t i = 0; i < S; ++i) { b += by[(uint64_t)sq * S + i]; r += nr[(uint64_t)sq * S + i]; }
      if (c->launches[idx].name == "answer") c->launches[idx].bytes = b;
      else c->launches[idx].bytes = r * G.maxPH;
    }
  }
  return 0;
}

static int run_batched_dev_body(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k, int step,
                                int parallel, uint32_t NG, int64_t* answers, double* mt_out, const DrlShape& sh,
                                std::vector<std::unique_ptr<DrlTeam>>& teams) {
  std::vector<StreamSwap> swaps(NG);   // (destroyed after the teams: drained, restored)
  struct Release {
    std::vector<std::unique_ptr<DrlTeam>>& t;
    ~Release() { for (auto& x : t) if (x->gs) team_release(x->gs, x->S); }
  } release{teams};
  for (uint32_t g = 0; g < NG; ++g) {
    const uint32_t s0 = (uint32_t)((uint64_t)S * g / NG), s1 = (uint32_t)((uint64_t)S * (g + 1) / NG);
    teams.emplace_back(new DrlTeam());
    CHK(drl_team_init(*teams.back(), gs + s0, s1 - s0, s0, queries, q, k, step, parallel, sh));
    swaps[g].swap_in(teams.back()->G.c, team_stream(teams.back()->G.c->device, g));
  }
  // Maintenance launch sets, timed by events around them on the leader's stream
  struct PrepSet { hipEvent_t a = nullptr, b = nullptr; std::vector<std::pair<DrlTeam*, uint32_t>> members; };
  std::vector<PrepSet> sets;
  struct SetsRelease {
    std::vector<PrepSet>& v;
    ~SetsRelease() { for (auto& x : v) { if (x.a) (void)hipEventDestroy(x.a); if (x.b) (void)hipEventDestroy(x.b); } }
  } sets_release{sets};
  for (uint64_t qi = 0; qi < q; ++qi) {
    if ((int64_t)g_fault_drl_query.load() == (int64_t)qi) return fail(PM_EHIP, "injected fault (fault_drl_query)");
    CHK(drl_query_all(teams, sh, qi, q, step));
    // the harness's maintenance trigger (private-search.go:226-232) per session:
    // the triggered clients of every team as ONE launch set after the query
    std::vector<Engine*> who;
    std::vector<double*> mts;
    std::vector<DrlTeam*> involved;
    for (auto& t : teams) {
      bool any = false;
      for (uint32_t i = 0; i < t->S; ++i) {
        Engine* e = &t->gs[i]->pir->e;
        t->need[i] = e->FBN + (uint64_t)step * (uint64_t)parallel + 10 >= e->Support;
        if (t->need[i]) { who.push_back(e); mts.push_back(&t->mt[i]); any = true; }
      }
      if (any) involved.push_back(t.get());
    }
    if (who.empty()) continue;
    // ONE launch set of every triggered client, on the first involved team's
    // stream after every involved team's query; nothing on the host waits for
    // it (the other teams keep running what is queued), and the involved
    // teams' next rounds wait for it on the device
    DrlTeam* L = involved[0];
    hipStream_t const sl = L->G.c->stream;
    for (DrlTeam* t : involved)
      if (t != L) {
        HIPCHK(hipEventRecord(t->ev_end, t->G.c->stream));
        HIPCHK(hipStreamWaitEvent(sl, t->ev_end, 0));
      }
    sets.emplace_back();
    PrepSet& ps = sets.back();
    HIPCHK(hipEventCreate(&ps.a));
    HIPCHK(hipEventCreate(&ps.b));
    HIPCHK(hipEventRecord(ps.a, sl));
    CHK(prep_clients(L->G.c, L->prep_buf, L->G.lp, who, nullptr, &L->prep_stage, &L->prep_stage_ev));
    for (DrlTeam* t : involved) {   // the new keys into the team's parts; the emptied localCache indexes
      CHK(group_upload_parts_async(t->G, sl, t->parts_stage, t->parts_stage_ev));
      for (uint32_t i = 0; i < t->S; ++i)
        if (t->need[i]) {
          CHK(ensure_dev_cache(&t->gs[i]->pir->e, sh.cmask, sl));
          ps.members.emplace_back(t, i);
        }
    }
    HIPCHK(hipEventRecord(ps.b, sl));
    for (DrlTeam* t : involved)
      if (t != L) HIPCHK(hipStreamWaitEvent(t->G.c->stream, ps.b, 0));
  }
  for (auto& t : teams) CHK(drl_team_finish(*t, q, k, answers));
  for (PrepSet& ps : sets) {   // each triggered client's maintenance time: its launch set's span on the GPU
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ps.a, ps.b));
    for (auto& [t, i] : ps.members) {
      t->mt[i] += ms / 1e3;
      record_stats(&t->gs[i]->pir->e, ms / 1e3);   // PreprocessingTime: the set's GPU span
    }
  }
  for (auto& t : teams)
    for (uint32_t i = 0; i < t->S; ++i) mt_out[t->s0 + i] = t->mt[i];
  return 0;
}

// The device loop; on a failure after the teams started, their streams are
// drained (nothing left running on the buffers being freed) and every session
// is marked lost: its host mirrors were advanced for queries whose device state
// was never read back.
static int run_batched_dev(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k, int step, int parallel,
                           uint32_t NG, int64_t* answers, double* mt_out, const DrlShape& sh) {
  std::vector<std::unique_ptr<DrlTeam>> teams;
  const int rc = run_batched_dev_body(gs, S, queries, q, k, step, parallel, NG, answers, mt_out, sh, teams);
  if (rc == 0) return 0;
  const std::string why = pm_last_error();
  for (auto& t : teams)
    if (t && t->G.c) (void)hipStreamSynchronize(t->G.c->stream);
  (void)hipDeviceSynchronize();
  for (uint32_t i = 0; i < S; ++i) gs[i]->lost = "device loop failed: " + why;
  return fail(rc, why);
}

extern "C" int pm_search_loop_batched(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k, int step,
                                      int parallel, uint32_t ngroups, uint32_t nthreads, int64_t* answers,
                                      double* wall_s, double* online_s, double* maint_s) {
  if (!gs || !S || (!queries && q) || (!answers && q)) return fail(PM_EINVAL, "NULL argument");
  CHK(check_loop_sessions(gs, S, false));
  // teams: sessions split into `ngroups` lock-step groups with their own step
  // streams, run concurrently (one group's shared step on the GPU while the
  // others' searches run on the host); threads split evenly
  const uint32_t NG = std::max(1u, std::min(ngroups ? ngroups : 1u, S));
  const uint32_t TT = std::max(NG, nthreads ? nthreads : std::min<uint32_t>(S, 16u));
  std::vector<double> mt(S, 0.0);
  auto t0 = Clock::now();
  DrlShape sh;
  if (drl_plan(gs, S, q, k, step, parallel, &sh)) {   // every round on the GPU (run_batched_dev)
    CHK(run_batched_dev(gs, S, queries, q, k, step, parallel, NG, answers, mt.data(), sh));
  } else {
    static const int pool = [] { const char* e = getenv("PM_BATCH_POOL"); return e ? atoi(e) : 1; }();
    if (pool && NG > 1) {   // the pooled workers (run_batched_pool); one team: the workers serve it alone anyway
      CHK(run_batched_pool(gs, S, queries, q, k, step, parallel, NG, TT, answers, mt.data()));
    } else {
      CHK(run_teams(gs, S, NG, TT, [&](uint32_t, uint32_t s0, uint32_t s1, uint32_t Tg) {
        return run_batched_team(gs + s0, s1 - s0, queries + (uint64_t)s0 * q * gs[0]->dim, q, k, step, parallel, Tg,
                                answers + (uint64_t)s0 * q * (uint64_t)k, mt.data() + s0);
      }));
    }
  }
  const double wall = std::chrono::duration<double>(Clock::now() - t0).count();
  if (wall_s) *wall_s = wall;
  for (uint32_t s = 0; s < S; ++s) {
    if (online_s) online_s[s] = wall - mt[s];
    if (maint_s) maint_s[s] = mt[s];
  }
  return 0;
}

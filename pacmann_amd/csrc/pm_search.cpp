// pm_search.cpp — the graphann beam search over PIRGraphInfo / BasicGraphInfo:
// pm_graph_*, GetVertexInfo (gvi_*), SearchKNN (knn_*), pm_search_knn,
// pm_search_knn_batch and the per-session loops pm_search_loop /
// pm_search_loop_sessions.  Needs pm_ctx.cpp and pm_engine.cpp.
#include "pm_engine.h"

// ---------------------------------------------------------------------------
// graphann: GraphANNFrontend over PIRGraphInfo / BasicGraphInfo
// ---------------------------------------------------------------------------
namespace pmh {
int check_session(const pm_graph* g) {
  if (!g->lost.empty()) return fail(PM_EINVAL, "session state lost: " + g->lost);
  if (g->pir) CHK(client_guard(&g->pir->e));
  return 0;
}
}  // namespace pmh

// PIRGraphInfo over one shard of the graph DB (multi-GPU private search,
// SURVEY.md §8e): host vectors and graph as pm_graph_create, but only the
// partitions p % nshards == shard are uploaded and served by this handle.
extern "C" int pm_graph_create_shard(pm_ctx* ctx, uint64_t n, uint64_t dim, uint64_t m, const float* vectors,
                                     const uint32_t* graph, uint32_t shard, uint32_t nshards, uint64_t pir_seed,
                                     uint64_t search_seed, pm_graph** out) {
  if (!ctx || !out || !vectors || !graph) return fail(PM_EINVAL, "NULL argument");
  if (n == 0 || dim == 0 || m == 0) return fail(PM_EINVAL, "n, dim, m must be > 0");
  if ((dim * 4 + m * 4) % 8) return fail(PM_EINVAL, "(4*dim + 4*m) must be a multiple of 8");
  if (nshards == 0 || shard >= nshards) return fail(PM_EINVAL, "shard must be < nshards");
  HIPCHK(hipSetDevice(ctx->device));
  pm_graph* g = new pm_graph();
  g->ctx = ctx; g->n = n; g->dim = dim; g->m = m;
  g->pir_seed = pir_seed; g->rng.s = search_seed;
  g->shard = shard; g->nshards = nshards;
  g->vec_own = std::make_shared<const std::vector<float>>(vectors, vectors + n * dim);
  g->graph_own = std::make_shared<const std::vector<uint32_t>>(graph, graph + n * m);
  g->vectors = g->vec_own->data();
  g->graph = g->graph_own->data();
  if (int r = g->dq.reserve(dim * 4)) { delete g; return r; }
  *out = g;
  return 0;
}
// The same over the synthetic graph (graph_synth_elem of data_seed, the
// reference's -input synthetic mode) generated on the device: BIGANN-scale
// graph DBs that cannot be built or shipped (BASELINE.json configs[3]/[4]).
extern "C" int pm_graph_create_synth(pm_ctx* ctx, uint64_t n, uint64_t dim, uint64_t m, uint64_t data_seed,
                                     uint32_t shard, uint32_t nshards, uint64_t pir_seed, uint64_t search_seed,
                                     pm_graph** out) {
  if (!ctx || !out) return fail(PM_EINVAL, "NULL argument");
  if (n <= 1 || dim == 0 || m == 0 || m > 64 || n > 0xffffffffull)
    return fail(PM_EINVAL, "need 1 < n < 2^32, dim > 0, 0 < m <= 64");
  if ((dim + m) % 2) return fail(PM_EINVAL, "(4*dim + 4*m) must be a multiple of 8");
  if (nshards == 0 || shard >= nshards) return fail(PM_EINVAL, "shard must be < nshards");
  HIPCHK(hipSetDevice(ctx->device));
  pm_graph* g = new pm_graph();
  g->ctx = ctx; g->n = n; g->dim = dim; g->m = m;
  g->pir_seed = pir_seed; g->rng.s = search_seed;
  g->shard = shard; g->nshards = nshards;
  g->synth = true; g->data_seed = data_seed;
  if (int r = g->dq.reserve(dim * 4)) { delete g; return r; }
  *out = g;
  return 0;
}
// Host restatement of the synthetic graph's rows (tests, checks): vec[i*dim..]
// and nb[i*m..] of vertex ids[i]; either output may be NULL.
extern "C" int pm_graph_synth_rows(uint64_t n, uint64_t dim, uint64_t m, uint64_t data_seed, const uint64_t* ids,
                                   uint64_t k, float* vec, uint32_t* nb) {
  if (k && !ids) return fail(PM_EINVAL, "NULL argument");
  const uint64_t kv = sm64(data_seed + DOM_SYNTH_VEC), kg = sm64(data_seed + DOM_SYNTH_NB);
  for (uint64_t i = 0; i < k; ++i) {
    if (ids[i] >= n) return fail(PM_EINVAL, "id out of range");
    if (vec) for (uint64_t j = 0; j < dim; ++j) vec[i * dim + j] = graph_synth_vec(kv, ids[i], (uint32_t)dim, (uint32_t)j);
    if (nb) for (uint64_t j = 0; j < m; ++j) nb[i * m + j] = graph_synth_nb(kg, n, ids[i], (uint32_t)m, (uint32_t)j);
  }
  return 0;
}

extern "C" int pm_graph_create(pm_ctx* ctx, uint64_t n, uint64_t dim, uint64_t m, const float* vectors,
                               const uint32_t* graph, int nonprivate, int skip_prep, uint64_t pir_seed,
                               uint64_t search_seed, pm_graph** out) {
  if (!ctx || !out || !vectors || !graph) return fail(PM_EINVAL, "NULL argument");
  if (n == 0 || dim == 0 || m == 0) return fail(PM_EINVAL, "n, dim, m must be > 0");
  if ((dim * 4 + m * 4) % 8) return fail(PM_EINVAL, "(4*dim + 4*m) must be a multiple of 8");
  HIPCHK(hipSetDevice(ctx->device));
  pm_graph* g = new pm_graph();
  g->ctx = ctx; g->n = n; g->dim = dim; g->m = m; g->nonprivate = nonprivate; g->skipPrep = skip_prep;
  g->pir_seed = pir_seed; g->rng.s = search_seed;
  g->vec_own = std::make_shared<const std::vector<float>>(vectors, vectors + n * dim);
  g->graph_own = std::make_shared<const std::vector<uint32_t>>(graph, graph + n * m);
  g->vectors = g->vec_own->data();
  g->graph = g->graph_own->data();
  int r = g->dvec->reserve(n * dim * 4);
  if (!r) r = g->dq.reserve(dim * 4);
  if (r) { delete g; return r; }
  hipError_t e = hipMemcpy(g->dvec->p, vectors, n * dim * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { delete g; return fail(PM_EHIP, hipGetErrorString(e)); }
  *out = g;
  return 0;
}
// A second client session over the same graph and server: shares the host
// vectors/graph, their device copy and (after pm_graph_preprocess) the server
// DB of `base`'s batch PIR, with its own context, keys, hint state, start set
// and id stream.  `base` must be preprocessed and outlive its sessions' preprocessing.
extern "C" int pm_graph_create_session(pm_ctx* ctx, pm_graph* base, uint64_t pir_seed, uint64_t search_seed,
                                       pm_graph** out) {
  if (!ctx || !base || !out) return fail(PM_EINVAL, "NULL argument");
  if (!base->nonprivate && !base->pir) return fail(PM_EINVAL, "base graph not preprocessed");
  if (base->ctx->device != ctx->device) return fail(PM_EINVAL, "a session shares its base's device");
  HIPCHK(hipSetDevice(ctx->device));
  pm_graph* g = new pm_graph();
  g->ctx = ctx; g->n = base->n; g->dim = base->dim; g->m = base->m;
  g->nonprivate = base->nonprivate; g->skipPrep = base->skipPrep;
  g->pir_seed = pir_seed; g->rng.s = search_seed;
  g->vec_own = base->vec_own; g->graph_own = base->graph_own;
  g->vectors = base->vectors; g->graph = base->graph;
  g->dvec = base->dvec;
  g->dgraph = base->dgraph;
  g->shard = base->shard; g->nshards = base->nshards;
  g->synth = base->synth; g->data_seed = base->data_seed;
  g->server = base->pir;
  if (int r = g->dq.reserve(g->dim * 4)) { delete g; return r; }
  *out = g;
  return 0;
}
extern "C" void pm_graph_destroy(pm_graph* g) { delete g; }
extern "C" pm_batchpir* pm_graph_pir(pm_graph* g) { return g->pir; }
extern "C" int pm_graph_counts(pm_graph* g, uint64_t* t, uint64_t* s) { *t = g->total; *s = g->succ; return 0; }

// PIRGraphInfo.Preprocess (private-search.go:355-412) + GetStartVertex (:508-531)
extern "C" int pm_graph_preprocess(pm_graph* g) {
  if (g->server) {   // session: a new client over the base's server DB
    delete g->pir; g->pir = nullptr;
    CHK(pm_batchpir_create_client(g->ctx, g->server, g->pir_seed, &g->pir));
    if (g->skipPrep) CHK(pm_batchpir_dummy_preprocessing(g->pir));
    else CHK(pm_batchpir_preprocessing(g->pir));
  } else if (g->synth) {   // the synthetic graph's entries generated on the device, this shard's partitions
    const uint64_t ebytes = g->dim * 4 + g->m * 4;
    delete g->pir; g->pir = nullptr;
    pm_batchpir* h = new pm_batchpir();
    const DbGen gen{1, g->data_seed, (uint32_t)g->dim, (uint32_t)g->m};
    if (int r = engine_create(g->ctx, &h->e, g->n, ebytes, g->m, nullptr, 8, g->pir_seed, true, g->shard, g->nshards,
                              nullptr, &gen, (uint32_t)g->dim)) { delete h; return r; }
    g->pir = h;
    g->pir->e.pf_off = g->dim * 4;
    g->pir->e.pf_len = g->m * 4;
    if (g->skipPrep) CHK(pm_batchpir_dummy_preprocessing(g->pir));
    else CHK(pm_batchpir_preprocessing(g->pir));
  } else {   // the PIR is built in non-private mode too (private-search.go:405)
    const uint64_t ebytes = g->dim * 4 + g->m * 4, E = ebytes / 8;
    std::vector<uint64_t> raw(g->n * E);
    for (uint64_t i = 0; i < g->n; ++i) {
      uint8_t* e = (uint8_t*)&raw[i * E];
      memcpy(e, &g->vectors[i * g->dim], g->dim * 4);
      memcpy(e + g->dim * 4, &g->graph[i * g->m], g->m * 4);
    }
    delete g->pir; g->pir = nullptr;
    // as pm_batchpir_create_shard, with the entry layout: words [0, dim) are the coordinates
    pm_batchpir* h = new pm_batchpir();
    if (int r = engine_create(g->ctx, &h->e, g->n, ebytes, g->m, raw.data(), 8, g->pir_seed, true, g->shard, g->nshards,
                              nullptr, nullptr, (uint32_t)g->dim)) { delete h; return r; }
    g->pir = h;
    g->pir->e.pf_off = g->dim * 4;   // the search reads the neighbour lists of the rows
    g->pir->e.pf_len = g->m * 4;
    if (g->skipPrep) CHK(pm_batchpir_dummy_preprocessing(g->pir));
    else CHK(pm_batchpir_preprocessing(g->pir));
  }
  return graph_start_set(g);
}
// GetStartVertex (private-search.go:508-531): the second half of pm_graph_preprocess, on its own for
// pm_graph_group_preprocess, which folds the sessions' hints as one launch set first.
int pmh::graph_start_set(pm_graph* g) {
  const uint64_t target = (uint64_t)std::sqrt((double)g->n);
  std::unordered_map<uint64_t, bool> added;
  g->start.clear();
  for (uint64_t i = 0; i < target; ++i) {
    uint64_t x = g->rng.intn(g->n);
    while (added.count(x)) x = g->rng.intn(g->n);
    added[x] = true;
    g->start.push_back(x);
  }
  std::vector<uint32_t> ids(g->start.begin(), g->start.end());
  CHK(g->dstart.reserve(std::max<size_t>(4, ids.size() * 4)));
  if (!ids.empty()) HIPCHK(hipMemcpy(g->dstart.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
  if (!g->dvec->p && !g->nonprivate) {   // the start set's vectors themselves (GetStartVertex, non-private)
    const uint64_t ns = g->start.size();
    CHK(g->dstartvec.reserve(std::max<uint64_t>(4, ns * g->dim * 4)));
    if (g->synth) {
      DevBuf did;
      CHK(did.reserve(std::max<uint64_t>(8, ns * 8)));
      HIPCHK(hipMemcpy(did.p, g->start.data(), ns * 8, hipMemcpyHostToDevice));
      pmk::graph_synth_vecs(g->ctx->stream, did.as<uint64_t>(), ns, (uint32_t)g->dim, g->data_seed,
                            g->dstartvec.as<float>());
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(g->ctx->stream));
    } else {
      std::vector<float> sv(ns * g->dim);
      for (uint64_t i = 0; i < ns; ++i) memcpy(&sv[i * g->dim], g->vectors + g->start[i] * g->dim, g->dim * 4);
      if (ns) HIPCHK(hipMemcpy(g->dstartvec.p, sv.data(), sv.size() * 4, hipMemcpyHostToDevice));
    }
  }
  return 0;
}

// container/heap (Go stdlib) restated: up / down / Push / Pop on a min-heap.
static void heap_up(std::vector<VD>& h, int64_t j) {
  for (;;) { int64_t i = (j - 1) / 2; if (i == j || !(h[j].dist < h[i].dist)) break; std::swap(h[i], h[j]); j = i; }
}
static void heap_down(std::vector<VD>& h, int64_t i0, int64_t n) {
  int64_t i = i0;
  for (;;) {
    int64_t j1 = 2 * i + 1; if (j1 >= n || j1 < 0) break;
    int64_t j = j1, j2 = j1 + 1;
    if (j2 < n && h[j2].dist < h[j1].dist) j = j2;
    if (!(h[j].dist < h[i].dist)) break;
    std::swap(h[i], h[j]); i = j;
  }
}
static void heap_push(std::vector<VD>& h, VD x) { h.push_back(x); heap_up(h, (int64_t)h.size() - 1); }
static VD heap_pop(std::vector<VD>& h) {
  int64_t n = (int64_t)h.size() - 1; std::swap(h[0], h[n]); heap_down(h, 0, n);
  VD r = h.back(); h.pop_back(); return r;
}

// GetVertexInfo (private-search.go:441-506) for g->batch, with the L2 distance
// of every returned vector to the resident query computed on the GPU next to
// the decode (k_answer).  Fills g->nb and g->dist.  In two halves around the
// batch-PIR step, so that several sessions' steps can share one launch
// (pm_search_loop_batched): gvi_pre buckets the ids into this session's
// sub-queries (*fast: they are ready for a shared step; otherwise the step
// has already been served on this session's own stream), gvi_post maps the
// published rows back and parses them.
static int gvi_nonprivate(pm_graph* g, bool with_q) {
  const uint64_t n = g->batch.size(), m = g->m;
  for (uint64_t i = 0; i < n; ++i)
    memcpy(&g->nb[i * m], &g->graph[(uint64_t)g->batch[i] * m], m * 4);
  if (with_q && n) {
    hipStream_t st = g->ctx->stream;
    std::vector<uint32_t> u(g->batch.begin(), g->batch.end());
    CHK(g->dids.reserve(n * 4)); CHK(g->ddist.reserve(n * 4));
    HIPCHK(hipMemcpyAsync(g->dids.p, u.data(), n * 4, hipMemcpyHostToDevice, st));
    g->ctx->timed("l2_rows", (double)n * g->dim * 4, [&] {
      pmk::l2_rows(st, g->dvec->as<float>(), g->dim, n, g->dids.as<uint32_t>(), g->qdev(), (uint32_t)g->dim, g->ddist.as<float>());
    });
    HIPCHK(hipMemcpyAsync(g->dist.data(), g->ddist.p, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return 0;
}
namespace pmh {
int gvi_pre(pm_graph* g, bool with_q, bool* fast) {
  const uint64_t n = g->batch.size(), m = g->m;
  g->total += n;
  g->nb.resize(n * m);
  g->dist.assign(n, 0.0f);
  *fast = false;
  if (g->nonprivate) return gvi_nonprivate(g, with_q);
  Engine* e = &g->pir->e;
  // the ground-truth rows of the success check (private-search.go:483-497) are
  // pulled into the cache while the GPU answers
  for (uint64_t i = 0; g->graph && i < n; ++i) {
    const char* gr = (const char*)&g->graph[(uint64_t)g->batch[i] * m];
    for (uint64_t b = 0; b < m * 4; b += 64) __builtin_prefetch(gr + b);
    __builtin_prefetch(gr + m * 4 - 1);
  }
  g->qids.assign(g->batch.begin(), g->batch.end());
  g->rowp.resize(n);
  auto t = Clock::now();
  e->rows_partial = true;   // Entry2VectorAndNeighbors reads the neighbour list (the distance is in the header)
  CHK(bq_prepare(e, g->qids.data(), n, fast));
  if (!*fast)   // a partition at its query budget: the general path, served now
    CHK(batch_query_impl(e, g->qids.data(), n, nullptr, with_q ? g->qdev() : nullptr, (uint32_t)g->dim,
                         with_q ? g->dist.data() : nullptr, g->rowp.data(), nullptr));
  e->ctx->host_add(HT_BATCH_QUERY, ms_since(t));
  return 0;
}
int gvi_post(pm_graph* g, bool with_q, bool fast) {
  if (g->nonprivate) return 0;
  const uint64_t n = g->batch.size(), m = g->m;
  Engine* e = &g->pir->e;
  if (fast) {
    auto t = Clock::now();
    bq_emit_fast(e, g->qids.data(), n, nullptr, with_q ? g->dist.data() : nullptr, g->rowp.data(), nullptr);
    CHK(bq_tail(e, n));
    e->ctx->host_add(HT_BATCH_QUERY, ms_since(t));
  }
  auto t_parse = Clock::now();
  const uint64_t nb_off = g->dim * 4;   // Entry2VectorAndNeighbors (private-search.go:418-439)
  for (uint64_t i = 0; i < n; ++i) {
    const char* r = (const char*)g->rowp[i] + nb_off;
    for (uint64_t b = 0; b < m * 4; b += 64) __builtin_prefetch(r + b);
  }
  uint32_t tmp[64];
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t* nbi = &g->nb[i * m];
    memcpy(nbi, (const char*)g->rowp[i] + nb_off, m * 4);
    if (memcmp(nbi, g->true_nb((uint64_t)g->batch[i], tmp), m * 4) == 0) g->succ++;
  }
  e->rows_partial = false;
  g->ctx->host_add(HT_GVI_PARSE, ms_since(t_parse));
  return 0;
}
}  // namespace pmh
static int get_vertex_info(pm_graph* g, bool with_q) {
  if (g->nshards > 1) return fail(PM_EINVAL, "a sharded graph searches through pm_search_loop_sharded (the shards' combine)");
  bool fast = false;
  CHK(gvi_pre(g, with_q, &fast));
  if (fast) {
    Engine* e = &g->pir->e;
    auto t = Clock::now();
    CHK(engine_step(e, with_q ? g->qdev() : nullptr, (uint32_t)g->dim));
    e->ctx->host_add(HT_BATCH_QUERY, ms_since(t));
  }
  return gvi_post(g, with_q, fast);
}

// ---- the GetGraphInfo plugin surface (graphann/search.go:20-25) ----------
// PIRGraphInfo's methods (private-search.go:441-531) as batch calls, so a
// caller that keeps its own beam search (graphann.SearchKNN in Go) still gets
// the private fetch, the decode and the L2 on the GPU.
extern "C" int pm_graph_get_metadata(pm_graph* g, uint64_t* n, uint64_t* dim, uint64_t* m) {
  if (!g) return fail(PM_EINVAL, "NULL argument");
  if (n) *n = g->n;
  if (dim) *dim = g->dim;
  if (m) *m = g->m;
  return 0;
}

extern "C" int pm_graph_get_vertex_info(pm_graph* g, const uint64_t* ids, uint64_t n, float* vecs, uint32_t* nbrs,
                                        uint8_t* ok, const float* query, float* dist) {
  if (!g || (n && !ids)) return fail(PM_EINVAL, "NULL argument");
  CHK(check_session(g));
  if (dist && !query) return fail(PM_EINVAL, "dist needs a query");
  if (g->nshards > 1) return fail(PM_EINVAL, "a sharded graph searches through pm_search_loop_sharded (the shards' combine)");
  if (!g->nonprivate && !g->pir) return fail(PM_EINVAL, "graph not preprocessed");
  for (uint64_t i = 0; i < n; ++i)
    if (ids[i] >= g->n) return fail(PM_EINVAL, "vertex id " + std::to_string(ids[i]) + " out of range");
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(g->ctx->device));
  if (query) HIPCHK(hipMemcpy(g->dq.p, query, g->dim * 4, hipMemcpyHostToDevice));
  const uint64_t dim = g->dim, m = g->m;
  uint32_t tmp[64];
  g->total += n;   // totalQueryNum (:443)
  if (g->nonprivate) {   // :445-455, BasicGraphInfo-style direct access
    for (uint64_t i = 0; i < n; ++i) {
      if (vecs) {
        if (g->synth) for (uint64_t j = 0; j < dim; ++j) vecs[i * dim + j] = graph_synth_vec(sm64(g->data_seed + DOM_SYNTH_VEC), ids[i], (uint32_t)dim, (uint32_t)j);
        else memcpy(vecs + i * dim, g->vectors + ids[i] * dim, dim * 4);
      }
      if (nbrs) memcpy(nbrs + i * m, g->true_nb(ids[i], tmp), m * 4);
      if (ok) ok[i] = 1;
    }
    if (dist) {
      g->batch.assign(ids, ids + n);
      g->nb.resize(n * m);
      g->dist.assign(n, 0.0f);
      CHK(gvi_nonprivate(g, true));
      memcpy(dist, g->dist.data(), n * 4);
    }
    return 0;
  }
  Engine* e = &g->pir->e;
  g->rowp.resize(n);
  std::vector<uint8_t> okv(n);
  std::vector<float> dv(n);
  e->rows_partial = false;   // whole rows: the caller reads the vectors too
  CHK(batch_query(e, ids, n, nullptr, query ? g->qdev() : nullptr, (uint32_t)dim, query ? dv.data() : nullptr,
                  g->rowp.data(), okv.data()));
  for (uint64_t i = 0; i < n; ++i) {   // Entry2VectorAndNeighbors (:418-439) + the success count (:483-497)
    const char* r = (const char*)g->rowp[i];
    if (vecs) memcpy(vecs + i * dim, r, dim * 4);
    if (nbrs) memcpy(nbrs + i * m, r + dim * 4, m * 4);
    if (memcmp(r + dim * 4, g->true_nb(ids[i], tmp), m * 4) == 0) g->succ++;
    if (ok) ok[i] = okv[i];
    if (dist) dist[i] = dv[i];
  }
  return 0;
}

extern "C" int pm_graph_get_start_vertex(pm_graph* g, uint64_t cap, uint64_t* ids, float* vecs, uint32_t* nbrs,
                                         uint64_t* count) {
  if (!g) return fail(PM_EINVAL, "NULL argument");
  if (!g->nonprivate && !g->pir) return fail(PM_EINVAL, "graph not preprocessed");
  const uint64_t ns = g->start.size(), dim = g->dim, m = g->m;
  if (count) *count = ns;
  uint32_t tmp[64];
  const uint64_t kv = sm64(g->data_seed + DOM_SYNTH_VEC);
  for (uint64_t i = 0; i < ns && i < cap; ++i) {   // non-private (:508-531)
    const uint64_t x = g->start[i];
    if (ids) ids[i] = x;
    if (vecs) {
      if (g->synth) for (uint64_t j = 0; j < dim; ++j) vecs[i * dim + j] = graph_synth_vec(kv, x, (uint32_t)dim, (uint32_t)j);
      else memcpy(vecs + i * dim, g->vectors + x * dim, dim * 4);
    }
    if (nbrs) memcpy(nbrs + i * m, g->true_nb(x, tmp), m * 4);
  }
  return 0;
}

// SearchKNN (graphann/search.go:114-234).  Same tie rules as oracle/pm_oracle.cpp.
static int search_knn_impl(pm_graph* g, const float* query, int k, int max_step, int parallel,
                           int benchmarking, int64_t* ids_out, int64_t* steps_out);
extern "C" int pm_search_knn(pm_graph* g, const float* query, int k, int max_step, int parallel,
                             int benchmarking, int64_t* ids_out, int64_t* steps_out) {
  if (g) CHK(check_session(g));
  auto t = Clock::now();
  int r = search_knn_impl(g, query, k, max_step, parallel, benchmarking, ids_out, steps_out);
  g->ctx->host_add(HT_SEARCH_KNN, ms_since(t));
  return r;
}
// SearchKNN in parts (the loop of search_knn_impl; pm_search_loop_batched
// interleaves them across sessions):
//   knn_begin  reset; unless benchmarking, the start set's distances to the
//              query (GPU, k_l2_rows) and the first `parallel` of them on the heap;
//   knn_batch  the ids of one step (search.go:150-172);
//   knn_update the returned vertices with a non-empty neighbour list become
//              known (search.go:185-218);
//   knn_end    top k by (dist, id) (search.go:222-233).
static void knn_add_known(pm_graph* g, int64_t id, const uint32_t* nb, float d, int64_t reach) {
  const uint64_t m = g->m;
  const uint32_t slot = (uint32_t)g->known_id.size();
  g->known.put((uint64_t)id, slot);
  g->known_nb.insert(g->known_nb.end(), nb, nb + m);
  g->known_dist.push_back(d);
  g->known_id.push_back(id);
  g->known_reach.push_back(reach);
}
namespace pmh {
// first half: reset + enqueue the start-set distances (async on the session's
// stream); knn_begin_finish completes it after the stream is synchronised
void knn_reset(pm_graph* g) {
  g->known.clear();
  g->known_nb.clear(); g->known_dist.clear(); g->known_id.clear(); g->known_reach.clear();
  g->heap.clear();
}
}  // namespace pmh
static int knn_begin_enqueue(pm_graph* g, const float* query, int benchmarking) {
  if (!g->pir && !g->nonprivate) return fail(PM_EINVAL, "pm_graph_preprocess not called");
  hipStream_t st = g->ctx->stream;
  knn_reset(g);
  if (benchmarking) return 0;
  g->t_init = Clock::now();
  // the query stays resident for every distance this search computes; it and
  // the start-vertex distances move through pinned staging (async, no bounce)
  const uint64_t ns = g->start.size();
  CHK(g->stage_h.reserve(g->dim * 4 + ns * 4));
  float* qh = g->stage_h.as<float>();
  memcpy(qh, query, g->dim * 4);
  HIPCHK(hipMemcpyAsync(g->dq.p, qh, g->dim * 4, hipMemcpyHostToDevice, st));
  if (ns) {
    CHK(g->ddist.reserve(ns * 4));
    const bool ids = g->dvec->p != nullptr;   // all vectors on the device, or the start set's own (sharded / synthetic)
    g->ctx->timed("l2_rows", (double)ns * g->dim * 4, [&] {
      pmk::l2_rows(st, ids ? g->dvec->as<float>() : g->dstartvec.as<float>(), g->dim, ns,
                   ids ? g->dstart.as<uint32_t>() : nullptr, g->dq.as<float>(), (uint32_t)g->dim, g->ddist.as<float>());
    });
    HIPCHK(hipMemcpyAsync(qh + g->dim, g->ddist.p, ns * 4, hipMemcpyDeviceToHost, st));
  }
  return 0;
}
namespace pmh {
// sdh: the start set's distances (null: where knn_begin_enqueue put them)
void knn_begin_finish(pm_graph* g, int parallel, int benchmarking, const float* sdh) {
  if (benchmarking) return;
  const uint64_t ns = g->start.size();
  if (!sdh) sdh = g->stage_h.as<float>() + g->dim;
  // the first `parallel` start vertices in stable distance order (search.go:130-146):
  // a partial sort on (dist, position) selects exactly those
  g->fs.clear();
  for (uint64_t i = 0; i < ns; ++i) g->fs.push_back({{sdh[i], (int64_t)g->start[i]}, (uint32_t)i});
  const size_t take = std::min<size_t>(g->fs.size(), (size_t)std::max(parallel, 0));
  std::partial_sort(g->fs.begin(), g->fs.begin() + take, g->fs.end(), [](const auto& a, const auto& b) {
    return a.first.dist < b.first.dist || (a.first.dist == b.first.dist && a.second < b.second); });
  g->fs.resize(take);   // start ids are distinct: none of the first `parallel` is skipped as known
  g->ctx->host_add(HT_KNN_INIT, ms_since(g->t_init));
  for (size_t i = 0; (int64_t)g->heap.size() < parallel && i < g->fs.size(); ++i) {
    const int64_t id = g->fs[i].first.id;
    if (g->known.find((uint64_t)id)) continue;
    uint32_t tmp[64];   // GetStartVertex returns the start vertices' neighbour lists (non-private)
    knn_add_known(g, id, g->true_nb((uint64_t)id, tmp), g->fs[i].first.dist, 0);
    heap_push(g->heap, g->fs[i].first);
  }
}
void knn_batch(pm_graph* g, int parallel, int benchmarking) {
  auto t_batch = Clock::now();
  const uint64_t m = g->m, n = g->n;
  g->batch.clear();
  for (int r = 0; r < parallel; ++r) {
    if (g->heap.empty() || benchmarking) {
      for (uint64_t i = 0; i < m; ++i) g->batch.push_back((int64_t)g->rng.intn(n));
    } else {
      const VD it = heap_pop(g->heap);
      const uint32_t* nb = &g->known_nb[(size_t)*g->known.find((uint64_t)it.id) * m];
      for (uint64_t i = 0; i < m; ++i) g->batch.push_back((int64_t)nb[i]);
    }
  }
  g->ctx->host_add(HT_KNN_BATCH, ms_since(t_batch));
}
void knn_update(pm_graph* g, int step) {
  auto t_round = Clock::now();
  const uint64_t m = g->m;
  for (size_t i = 0; i < g->batch.size(); ++i) g->known.prefetch((uint64_t)g->batch[i]);
  if (g->known_id.capacity() < 4096) {   // a search keeps ~2,000 known vertices (20 steps x 96 ids)
    g->known_id.reserve(4096); g->known_dist.reserve(4096); g->known_reach.reserve(4096);
    g->known_nb.reserve(4096 * m);
  }
  for (size_t i = 0; i < g->batch.size(); ++i) {
    const int64_t id = g->batch[i];
    if (g->known.find((uint64_t)id)) continue;
    const uint32_t* nb = &g->nb[i * m];
    bool ok = false;
    for (uint64_t j = 0; j < m; ++j) if (nb[j] != 0) { ok = true; break; }
    if (!ok) continue;
    knn_add_known(g, id, nb, g->dist[i], step);
    heap_push(g->heap, {g->dist[i], id});
  }
  g->ctx->host_add(HT_KNN_UPDATE, ms_since(t_round));
}
void knn_end(pm_graph* g, int k, int64_t* ids_out, int64_t* steps_out) {
  auto t_fin = Clock::now();
  g->all.clear();
  for (size_t i = 0; i < g->known_id.size(); ++i) g->all.push_back({g->known_dist[i], g->known_id[i]});
  // top k in (dist, id) order (search.go:222-233); ids are unique, so a partial sort is exact
  std::partial_sort(g->all.begin(), g->all.begin() + std::min<size_t>(g->all.size(), (size_t)std::max(k, 0)),
                    g->all.end(), [](const VD& a, const VD& b) {
    return a.dist < b.dist || (a.dist == b.dist && a.id < b.id); });
  for (int i = 0; i < k; ++i) {
    if (i >= (int)g->all.size()) { ids_out[i] = -1; if (steps_out) steps_out[i] = -1; }
    else { ids_out[i] = g->all[i].id; if (steps_out) steps_out[i] = g->known_reach[*g->known.find((uint64_t)g->all[i].id)]; }
  }
  g->ctx->host_add(HT_KNN_FINAL, ms_since(t_fin));
}
}  // namespace pmh
static int search_knn_impl(pm_graph* g, const float* query, int k, int max_step, int parallel,
                           int benchmarking, int64_t* ids_out, int64_t* steps_out) {
  CHK(knn_begin_enqueue(g, query, benchmarking));
  if (!benchmarking) HIPCHK(hipStreamSynchronize(g->ctx->stream));
  knn_begin_finish(g, parallel, benchmarking);
  for (int step = 0; step < max_step; ++step) {
    knn_batch(g, parallel, benchmarking);
    CHK(get_vertex_info(g, !benchmarking));
    if (benchmarking) continue;
    knn_update(g, step);
  }
  knn_end(g, k, ids_out, steps_out);
  return 0;
}

// GraphANNFrontend.SearchKNNBatch (graphann/search.go:236-245): SearchKNN of
// queries[i] for i = 0 .. nq-1 in order.  Defined as that loop over
// search_knn_impl (same ids, steps, counters and id stream afterwards); a
// non-private in-memory graph whose shape fits k_knn_batch (pm_knnb.hip) is
// searched on the device instead, one workgroup per query, a chunk of queries
// per launch.  A search draws from the id stream only where a pop finds its
// heap empty (search.go:155-159); the kernel flags such a query instead of
// answering it, and the flagged queries are re-run here in ascending order, so
// the stream is consumed exactly as by the loop.
extern "C" int pm_search_knn_batch(pm_graph* g, const float* queries, uint64_t nq, int k, int max_step, int parallel,
                                   int benchmarking, int64_t* ids, int64_t* steps, uint64_t* device_queries) {
  if (!g) return fail(PM_EINVAL, "NULL argument");
  CHK(check_session(g));
  if (device_queries) *device_queries = 0;
  if (nq && (!queries || !ids)) return fail(PM_EINVAL, "NULL argument");
  pm_ctx* c = g->ctx;
  const uint64_t dim = g->dim, m = g->m, ns = g->start.size(), kk = (uint64_t)std::max(k, 0);
  auto host_query = [&](uint64_t i) {
    return search_knn_impl(g, queries + i * dim, k, max_step, parallel, benchmarking, ids + i * kk,
                           steps ? steps + i * kk : nullptr);
  };
  bool dev = nq && g->nonprivate && !g->synth && g->nshards == 1 && !benchmarking && g->dvec->p && g->graph &&
             g->n < 0xffffffffull && k > 0 && max_step >= 0 && parallel > 0 &&
             pmk::knn_batch_ok(dim, m, ns, (uint64_t)max_step, (uint64_t)parallel);
  if (dev && g->graph_ids_ok < 0) {   // the kernel follows the graph's ids without a host in between
    g->graph_ids_ok = 1;
    for (uint64_t i = 0; i < g->n * m; ++i)
      if (g->graph[i] >= g->n) { g->graph_ids_ok = 0; break; }
  }
  if (!dev || !g->graph_ids_ok) {
    for (uint64_t i = 0; i < nq; ++i) CHK(host_query(i));
    return 0;
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  if (!g->dgraph->p) {   // the neighbour lists on the device, once per graph
    CHK(g->dgraph->reserve(g->n * m * 4));
    HIPCHK(hipMemcpy(g->dgraph->p, g->graph, g->n * m * 4, hipMemcpyHostToDevice));
  }
  const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>({nq, 1u << 15, (256ull << 20) / (kk * 16)}));
  std::vector<uint32_t> flags(nq);
  pmk::KnbArgs A{};
  A.vec = g->dvec->as<float>();
  A.graph = g->dgraph->as<uint32_t>();
  A.start = g->dstart.as<uint32_t>();
  A.ns = (uint32_t)ns; A.dim = (uint32_t)dim; A.m = (uint32_t)m; A.k = (uint32_t)k;
  A.max_step = (uint32_t)max_step; A.parallel = (uint32_t)parallel;
  A.kcap = pmk::knn_batch_kcap((uint64_t)parallel, (uint64_t)max_step, m);
  for (uint64_t q0 = 0; q0 < nq; q0 += chunk) {
    const uint64_t cn = std::min(chunk, nq - q0);
    CHK(g->kb_q.reserve(cn * dim * 4)); CHK(g->kb_ids.reserve(cn * kk * 8));
    CHK(g->kb_steps.reserve(cn * kk * 8)); CHK(g->kb_flags.reserve(cn * 4));
    HIPCHK(hipMemcpyAsync(g->kb_q.p, queries + q0 * dim, cn * dim * 4, hipMemcpyHostToDevice, st));
    A.queries = g->kb_q.as<float>(); A.nq = (uint32_t)cn;
    A.ids = g->kb_ids.as<int64_t>(); A.steps = g->kb_steps.as<int64_t>(); A.needs_host = g->kb_flags.as<uint32_t>();
    c->timed("knn_batch", (double)cn * (double)(ns + (uint64_t)max_step * parallel * m) * (double)(dim + m) * 4.0,
             [&] { pmk::knn_batch(st, A); });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ids + q0 * kk, g->kb_ids.p, cn * kk * 8, hipMemcpyDeviceToHost, st));
    if (steps) HIPCHK(hipMemcpyAsync(steps + q0 * kk, g->kb_steps.p, cn * kk * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(flags.data() + q0, g->kb_flags.p, cn * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  uint64_t nhost = 0;
  for (uint64_t i = 0; i < nq; ++i) nhost += flags[i] != 0;
  g->total += (nq - nhost) * (uint64_t)max_step * (uint64_t)parallel * m;   // totalQueryNum of the device's queries
  if (device_queries) *device_queries = nq - nhost;
  if (nhost) {
    auto t = Clock::now();
    for (uint64_t i = 0; i < nq; ++i)
      if (flags[i]) CHK(host_query(i));
    c->host_add(HT_KNN_BATCH_FALLBACK, ms_since(t));
  }
  return 0;
}

// private-search.go:216-240
extern "C" int pm_search_loop(pm_graph* g, const float* queries, uint64_t q, int k, int step, int parallel,
                              int benchmarking, int64_t* answers, double* online_s, double* maint_s) {
  if (g) CHK(check_session(g));
  std::vector<int64_t> steps(k);
  double maint = 0;
  auto t0 = std::chrono::steady_clock::now();
  for (uint64_t i = 0; i < q; ++i) {
    CHK(pm_search_knn(g, queries + i * g->dim, k, step, parallel, benchmarking, answers + i * k, steps.data()));
    if (g->pir) {
      Engine* e = &g->pir->e;
      if (e->FBN + (uint64_t)step * (uint64_t)parallel + 10 >= e->Support) {
        auto a = std::chrono::steady_clock::now();
        CHK(batch_prep(e));
        maint += std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count();
      }
    }
  }
  double total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (online_s) *online_s = total - maint;
  if (maint_s) *maint_s = maint;
  return 0;
}

// S client sessions served concurrently on one GPU: session i runs the
// private-search.go:216-240 loop (search + its own maintenance trigger) over
// queries[i*q .. (i+1)*q) on its own host thread and stream.  The sessions'
// step kernels overlap each other's host work.  online_s / maint_s: S entries.
extern "C" int pm_search_loop_sessions(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k,
                                       int step, int parallel, int64_t* answers, double* wall_s,
                                       double* online_s, double* maint_s) {
  if (!gs || !S || (!queries && q) || (!answers && q)) return fail(PM_EINVAL, "NULL argument");
  for (uint32_t i = 0; i < S; ++i)
    if (gs[i]) CHK(check_session(gs[i]));
  for (uint32_t i = 0; i < S; ++i) {
    if (!gs[i]) return fail(PM_EINVAL, "NULL session");
    for (uint32_t j = 0; j < i; ++j)
      if (gs[j] == gs[i] || gs[j]->ctx == gs[i]->ctx) return fail(PM_EINVAL, "sessions need distinct graphs and contexts");
  }
  std::vector<int> rc(S, 0);
  std::vector<std::string> msg(S);
  std::vector<double> on(S, 0.0), mt(S, 0.0);
  std::atomic<uint32_t> ready{0};
  std::atomic<bool> go{false};
  std::vector<std::thread> th;
  th.reserve(S);
  for (uint32_t i = 0; i < S; ++i) {
    th.emplace_back([&, i] {
      pm_graph* g = gs[i];
      if (hipSetDevice(g->ctx->device) != hipSuccess) { rc[i] = PM_EHIP; msg[i] = "hipSetDevice"; ready++; return; }
      ready++;
      while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
      rc[i] = pm_search_loop(g, queries + i * q * g->dim, q, k, step, parallel, 0, answers + i * q * (uint64_t)k,
                             &on[i], &mt[i]);
      if (rc[i]) msg[i] = pm_last_error();
      else if (hipStreamSynchronize(g->ctx->stream) != hipSuccess) { rc[i] = PM_EHIP; msg[i] = "stream sync"; }
    });
  }
  while (ready.load() < S) std::this_thread::yield();
  auto t0 = std::chrono::steady_clock::now();
  go.store(true, std::memory_order_release);
  for (auto& t : th) t.join();
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (wall_s) *wall_s = wall;
  for (uint32_t i = 0; i < S; ++i) {
    if (online_s) online_s[i] = on[i];
    if (maint_s) maint_s[i] = mt[i];
  }
  for (uint32_t i = 0; i < S; ++i)
    if (rc[i]) return fail(rc[i], "session " + std::to_string(i) + ": " + msg[i]);
  return 0;
}

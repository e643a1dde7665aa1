// pm_build.cpp — graph construction and the exact kNN ground truth
// (pm_knn, pm_build_graph), for float rows and for uint8 rows (pm_knn_u8,
// pm_build_graph_u8).
#include "pm_host.h"

// ---------------------------------------------------------------------------
// Graph construction and exact kNN ground truth.
// CreateGraphBasedOnNGT (graphann/build_graph.go:314-523) with the NGT
// candidate search replaced by exact kNN: GPU bf16 MFMA prefilter (top 64) and
// an exact re-rank in L2Dist order (pm_graph.hip); robustPrune on the GPU;
// reverse edges, sampling and the random fill on host threads (O(n m)).
// Randomness (the reference's per-thread math/rand, :455,473-475) comes from
// hash4 domains 7 (edge sampling) and 8 (fill), so any thread split gives the
// same graph.  oracle/pm_oracle.cpp (or_build_graph) restates the same spec.
// ---------------------------------------------------------------------------
enum : uint64_t { DOM_GRAPH_SAMPLE = 7, DOM_GRAPH_FILL = 8 };

template <class F> static void par_for(uint64_t n, F&& f) {
  const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (n < 4096 || nt == 1) { f(0, n); return; }
  std::vector<std::thread> th;
  const uint64_t per = (n + nt - 1) / nt;
  for (unsigned t = 0; t < nt; ++t) {
    const uint64_t a = t * per, b = std::min(n, a + per);
    if (a < b) th.emplace_back([&, a, b] { f(a, b); });
  }
  for (auto& t : th) t.join();
}

// KnnDev (pm_host.h): device copies for the prefilter + re-rank.
// The "_wide" entry points: rows up to 1,024 wide.  Rows that are not pmk::knn_wide
// take the narrow path unchanged; the others the chunked kernels.
const char* const kWideDimText = "dim must be in [1, 1024]";
// The "_k128" entry points: the wide ones with 128 prefilter keys per query row.
static const char* const kK128KText = "k must be in [1, 128]";
bool wide_dim_ok(uint64_t dim) { return pmk::knn_pad_dim_wide((uint32_t)std::min<uint64_t>(dim, UINT32_MAX)) != 0; }
// exact: the split rows of pm_knn_exact (hi + lo, norms of the f32 values);
// wide (exact only): rows above knn_pad_dim's widths are padded by knn_pad_dim_wide;
// kind: where v lies (pm_kmeans' centroids are already on the device)
int knn_upload(pm_ctx* c, const float* v, uint64_t n, uint32_t dim, KnnDev& d, bool exact, bool wide,
               hipMemcpyKind kind) {
  d.dp = wide && pmk::knn_wide(dim) ? pmk::knn_pad_dim_wide(dim) : pmk::knn_pad_dim(dim);
  if (!d.dp) return fail(PM_EINVAL, "kNN supports dim <= 192");
  CHK(d.x.reserve(std::max<uint64_t>(4, n * dim * 4)));
  CHK(d.xb.reserve(std::max<uint64_t>(4, n * d.dp * 2)));
  CHK(d.xn.reserve(std::max<uint64_t>(4, n * 4)));
  HIPCHK(hipMemcpyAsync(d.x.p, v, n * dim * 4, kind, c->stream));
  if (!exact) {
    c->timed("to_bf16", (double)n * dim * 4, [&] { pmk::to_bf16(c->stream, d.x.as<float>(), n, dim, d.dp, d.xb.p, d.xn.as<float>()); });
    return 0;
  }
  CHK(d.xl.reserve(std::max<uint64_t>(4, n * d.dp * 2)));
  CHK(d.mx.reserve(4));
  HIPCHK(hipMemsetAsync(d.mx.p, 0, 4, c->stream));
  c->timed("to_bf16", (double)n * dim * 4, [&] {
    pmk::to_bf16x2(c->stream, d.x.as<float>(), n, dim, d.dp, d.xb.p, d.xl.p, d.xn.as<float>(), d.mx.as<uint32_t>()); });
  return 0;
}

// The first K of every query row's (L2Dist, id) ranking of the base rows, self
// dropped when self_base (Q is B): out [nq][K] with len [nq] valid entries each,
// dist [nq][K] when want_dist.  Prefilter (64 candidates per row) and exact
// re-rank; exact: the three-product prefilter, the certificate in the re-rank
// and the brute-force pass over the rows it did not certify, whose number goes
// to *fallback (pm_knn_exact).  Enqueued on c->stream; exact synchronises it.
// stages (pm_knn_stages): the kernels also store what they otherwise drop: the
// candidates' prefilter distances (pref [nq][64]) and, exact, each row's eps
// (NaN bits where no row was judged: n <= 64); tau and the uncertified list
// (nl rows, unordered) stay in the struct either way.
// top: the keys kept per query row, knn_top() or, for the _k128 entry points
// (exact only), knn_top_k128(): cand and pref [nq][128], no row judged for
// n <= 128.  pmk picks every stage's kernel from (B.dp or dim, top); the host
// only names the prefilter's timing entry after the same two.
// KnnOut is in pm_host.h.
int knn_device(pm_ctx* c, const KnnDev& B, uint64_t n, const KnnDev& Q, uint64_t nq, uint32_t dim, uint32_t K,
               bool self_base, bool want_dist, bool exact, KnnOut& o, uint64_t* fallback, uint32_t top) {
  hipStream_t st = c->stream;
  const bool k128 = top == pmk::knn_top_k128();
  CHK(o.cand.reserve(std::max<uint64_t>(4, nq * top * 4)));
  CHK(o.out.reserve(std::max<uint64_t>(4, nq * K * 4)));
  if (want_dist) CHK(o.dist.reserve(std::max<uint64_t>(4, nq * K * 4)));
  CHK(o.len.reserve(std::max<uint64_t>(4, nq * 4)));
  if (o.stages) CHK(o.pref.reserve(std::max<uint64_t>(4, nq * top * 4)));
  uint32_t* pref = o.stages ? o.pref.as<uint32_t>() : nullptr;
  const double pre_bytes = (double)nq * n * B.dp * 2, rr_bytes = (double)nq * top * dim * 4;
  if (!exact) {
    c->timed("knn_prefilter", pre_bytes, [&] {
      pmk::knn_prefilter(st, B.xb.p, B.xn.as<float>(), n, Q.xb.p, Q.xn.as<float>(), nq, B.dp, o.cand.as<uint32_t>(),
                         pref); });
    c->timed("knn_rerank", rr_bytes, [&] {
      pmk::knn_rerank(st, B.x.as<float>(), n, dim, Q.x.as<float>(), nq, o.cand.as<uint32_t>(), K, self_base,
                      o.out.as<uint32_t>(), o.dist.as<float>(), o.len.as<uint32_t>()); });
    return 0;
  }
  CHK(o.tau.reserve(std::max<uint64_t>(4, nq * 4)));
  CHK(o.list.reserve(std::max<uint64_t>(8, nq * 8)));
  CHK(o.nlist.reserve(8));
  HIPCHK(hipMemsetAsync(o.nlist.p, 0, 8, st));
  if (o.stages) {
    CHK(o.eps.reserve(std::max<uint64_t>(4, nq * 4)));
    HIPCHK(hipMemsetAsync(o.eps.p, 0xff, std::max<uint64_t>(4, nq * 4), st));
  }
  const bool wide = pmk::knn_wide(B.dp);
  c->timed(k128 ? (wide ? "knn_prefilter_k128_w" : "knn_prefilter_k128") : (wide ? "knn_prefilter_w" : "knn_prefilter_x3"),
           2 * pre_bytes, [&] {
    pmk::knn_prefilter_x3(st, B.xb.p, B.xl.p, B.xn.as<float>(), n, Q.xb.p, Q.xl.p, Q.xn.as<float>(), nq, B.dp, top,
                          o.cand.as<uint32_t>(), o.tau.as<float>(), pref); });
  c->timed("knn_rerank", rr_bytes, [&] {
    pmk::knn_rerank_cert(st, B.x.as<float>(), n, dim, Q.x.as<float>(), nq, o.cand.as<uint32_t>(), K, self_base,
                         o.out.as<uint32_t>(), o.dist.as<float>(), o.len.as<uint32_t>(), Q.xn.as<float>(),
                         o.tau.as<float>(), B.mx.as<uint32_t>(), B.dp, top, o.list.as<uint64_t>(),
                         o.nlist.as<uint64_t>(), o.stages ? o.eps.as<float>() : nullptr); });
  uint64_t nl = 0;
  HIPCHK(hipMemcpyAsync(&nl, o.nlist.p, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  c->timed("knn_brute", (double)nl * n * dim * 4, [&] {
    pmk::knn_brute(st, B.x.as<float>(), n, dim, top, Q.x.as<float>(), o.list.as<uint64_t>(), nl, K, self_base,
                   o.out.as<uint32_t>(), o.dist.as<float>(), o.len.as<uint32_t>()); });
  HIPCHK(hipStreamSynchronize(st));
  o.nl = nl;
  if (fallback) *fallback = nl;
  return 0;
}

// pm_knn and pm_knn_exact: exact k nearest base rows of each query by (L2Dist,
// id), k <= 64 (the ground truth of ComputeRecall, build_graph.go:821-863);
// ids -1 padded.
static int knn_impl(pm_ctx* c, const float* base, uint64_t n, uint64_t dim, const float* queries, uint64_t nq,
                    uint32_t k, int64_t* ids, float* dists, bool exact, uint64_t* fallback, bool wide = false,
                    uint32_t top = pmk::knn_top()) {
  if (!c || !base || (!queries && nq) || (!ids && nq)) return fail(PM_EINVAL, "NULL argument");
  if (wide && !wide_dim_ok(dim)) return fail(PM_EINVAL, kWideDimText);
  if (k == 0 || k > top) return fail(PM_EINVAL, top == pmk::knn_top() ? "k must be in [1, 64]" : kK128KText);
  if (n == 0 || dim == 0 || n >= (1ull << 32) - 1) return fail(PM_EINVAL, "n must be in [1, 2^32-1)");
  if (exact && !wide && !pmk::knn_pad_dim((uint32_t)std::min<uint64_t>(dim, UINT32_MAX)))
    return fail(PM_EINVAL, "kNN supports dim <= 192");
  HIPCHK(hipSetDevice(c->device));
  KnnDev B, Q;
  CHK(knn_upload(c, base, n, (uint32_t)dim, B, exact, wide));
  CHK(knn_upload(c, queries, nq, (uint32_t)dim, Q, exact, wide));
  KnnOut o;
  CHK(knn_device(c, B, n, Q, nq, (uint32_t)dim, k, false, true, exact, o, fallback, top));
  std::vector<uint32_t> out(nq * k), l(nq);
  std::vector<float> dd(nq * k);
  HIPCHK(hipMemcpyAsync(out.data(), o.out.p, nq * k * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(dd.data(), o.dist.p, nq * k * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(l.data(), o.len.p, nq * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (uint64_t i = 0; i < nq; ++i)
    for (uint32_t j = 0; j < k; ++j) {
      ids[i * k + j] = j < l[i] ? (int64_t)out[i * k + j] : -1;
      if (dists) dists[i * k + j] = j < l[i] ? dd[i * k + j] : INFINITY;
    }
  return 0;
}
extern "C" int pm_knn(pm_ctx* c, const float* base, uint64_t n, uint64_t dim, const float* queries, uint64_t nq,
                      uint32_t k, int64_t* ids, float* dists) {
  return knn_impl(c, base, n, dim, queries, nq, k, ids, dists, false, nullptr);
}
extern "C" int pm_knn_exact(pm_ctx* c, const float* base, uint64_t n, uint64_t dim, const float* queries,
                            uint64_t nq, uint32_t k, int64_t* ids, float* dists, uint64_t* fallback_rows) {
  if (fallback_rows) *fallback_rows = 0;
  return knn_impl(c, base, n, dim, queries, nq, k, ids, dists, true, fallback_rows);
}
extern "C" int pm_knn_wide(pm_ctx* c, const float* base, uint64_t n, uint64_t dim, const float* queries, uint64_t nq,
                           uint32_t k, int64_t* ids, float* dists, uint64_t* fallback_rows) {
  if (fallback_rows) *fallback_rows = 0;
  return knn_impl(c, base, n, dim, queries, nq, k, ids, dists, true, fallback_rows, true);
}
extern "C" int pm_knn_k128(pm_ctx* c, const float* base, uint64_t n, uint64_t dim, const float* queries, uint64_t nq,
                           uint32_t k, int64_t* ids, float* dists, uint64_t* fallback_rows) {
  if (fallback_rows) *fallback_rows = 0;
  return knn_impl(c, base, n, dim, queries, nq, k, ids, dists, true, fallback_rows, true, pmk::knn_top_k128());
}
extern "C" uint32_t pm_knn_k128_top(void) { return pmk::knn_top_k128(); }

// pm_knn_stages and pm_knn_stages_wide: pm_knn's (exact: pm_knn_exact's, wide:
// pm_knn_wide's) own upload and launches (knn_upload, knn_device), with the
// intermediate values copied out.
static int knn_stages_impl(pm_ctx* c, const float* base, uint64_t n, uint64_t dim, const float* queries, uint64_t nq,
                           uint32_t k, int exact, pm_knn_stages_out* out, bool wide,
                           uint32_t top = pmk::knn_top()) {
  if (!c || !base || !queries || !out || !out->cand || !out->pref) return fail(PM_EINVAL, "NULL argument");
  if (wide && !wide_dim_ok(dim)) return fail(PM_EINVAL, kWideDimText);
  if (k == 0 || k > top) return fail(PM_EINVAL, top == pmk::knn_top() ? "k must be in [1, 64]" : kK128KText);
  if (n == 0 || dim == 0 || n >= (1ull << 32) - 1) return fail(PM_EINVAL, "n must be in [1, 2^32-1)");
  if (nq == 0) return fail(PM_EINVAL, "nq must be > 0");
  if (!wide && !pmk::knn_pad_dim((uint32_t)std::min<uint64_t>(dim, UINT32_MAX)))
    return fail(PM_EINVAL, "kNN supports dim <= 192");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  KnnDev B, Q;
  CHK(knn_upload(c, base, n, (uint32_t)dim, B, exact != 0, wide));
  CHK(knn_upload(c, queries, nq, (uint32_t)dim, Q, exact != 0, wide));
  KnnOut o;
  o.stages = true;
  CHK(knn_device(c, B, n, Q, nq, (uint32_t)dim, k, false, true, exact != 0, o, nullptr, top));
  auto get = [&](void* dst, const DevBuf& src, uint64_t bytes) {
    return dst ? hipMemcpyAsync(dst, src.p, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
  };
  out->dp = B.dp;
  out->n_uncertified = 0;
  HIPCHK(get(out->cand, o.cand, nq * top * 4));
  HIPCHK(get(out->pref, o.pref, nq * top * 4));
  std::vector<uint64_t> list;
  if (exact) {
    HIPCHK(get(out->tau, o.tau, nq * 4));
    HIPCHK(get(out->eps, o.eps, nq * 4));
    HIPCHK(get(out->qnorm, Q.xn, nq * 4));
    HIPCHK(get(out->bnorm, B.xn, n * 4));
    HIPCHK(get(out->maxnorm, B.mx, 4));
    HIPCHK(get(out->bhi, B.xb, n * B.dp * 2));
    HIPCHK(get(out->blo, B.xl, n * B.dp * 2));
    list.resize(o.nl);
    if (o.nl) HIPCHK(hipMemcpyAsync(list.data(), o.list.p, o.nl * 8, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  if (exact) {
    std::sort(list.begin(), list.end());   // the kernel appends in any order
    out->n_uncertified = list.size();
    if (out->uncertified) std::copy(list.begin(), list.end(), out->uncertified);
  }
  return 0;
}
extern "C" int pm_knn_stages(pm_ctx* c, const float* base, uint64_t n, uint64_t dim, const float* queries,
                             uint64_t nq, uint32_t k, int exact, pm_knn_stages_out* out) {
  return knn_stages_impl(c, base, n, dim, queries, nq, k, exact, out, false);
}
extern "C" int pm_knn_stages_wide(pm_ctx* c, const float* base, uint64_t n, uint64_t dim, const float* queries,
                                  uint64_t nq, uint32_t k, pm_knn_stages_out* out) {
  return knn_stages_impl(c, base, n, dim, queries, nq, k, 1, out, true);
}
extern "C" int pm_knn_stages_k128(pm_ctx* c, const float* base, uint64_t n, uint64_t dim, const float* queries,
                                  uint64_t nq, uint32_t k, pm_knn_stages_out* out) {
  return knn_stages_impl(c, base, n, dim, queries, nq, k, 1, out, true, pmk::knn_top_k128());
}

// robustPrune on the GPU of the listed vertices' lists (the second pass of the
// build, :464-466; pm_robust_prune): vertex u's candidates are conn[coff[u] ..
// coff[u] + clen[u]), X the device rows.  big: by k_prune's own LDS sort (lists
// up to prune_max_list()).  huge: lists above the kernel's LDS sort (hub
// vertices: every in-edge of a popular vertex is kept, :448-462 sample by the
// TARGET's inbounds) get their candidate distances on the GPU (k_cand_dist),
// their (L2Dist, position) order by a host sort of those exact keys, and the
// same greedy pass (presorted k_prune).  P [n][m] and PL [n] hold the listed
// vertices' results; *e the kernel's error flag (a big list above the limit).
static int prune_lists(pm_ctx* c, const float* X, uint64_t n, uint32_t dim, const std::vector<uint32_t>& big,
                       const std::vector<uint32_t>& huge, const std::vector<uint64_t>& coff,
                       const std::vector<uint32_t>& clen, const std::vector<uint32_t>& conn, uint32_t m, float alpha,
                       std::vector<uint32_t>& P, std::vector<uint32_t>& PL, uint32_t* e, bool wide = false) {
  *e = 0;
  if (big.empty() && huge.empty()) return 0;
  hipStream_t st = c->stream;
  DevBuf dv, dh, doff, dlen, dids, dout, dol, dd, dpos, err;
  CHK(dv.reserve(std::max<size_t>(1, big.size()) * 4));
  CHK(dh.reserve(std::max<size_t>(1, huge.size()) * 4));
  CHK(doff.reserve(n * 8));
  CHK(dlen.reserve(n * 4));
  CHK(dids.reserve(std::max<uint64_t>(4, conn.size() * 4)));
  CHK(dout.reserve(n * m * 4));
  CHK(dol.reserve(n * 4));
  CHK(err.reserve(4));
  HIPCHK(hipMemsetAsync(err.p, 0, 4, st));
  if (!big.empty()) HIPCHK(hipMemcpyAsync(dv.p, big.data(), big.size() * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(doff.p, coff.data(), n * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dlen.p, clen.data(), n * 4, hipMemcpyHostToDevice, st));
  if (!conn.empty()) HIPCHK(hipMemcpyAsync(dids.p, conn.data(), conn.size() * 4, hipMemcpyHostToDevice, st));
  c->timed("prune", 0.0, [&] {
    pmk::prune(st, X, dim, wide, dv.as<uint32_t>(), big.size(), doff.as<uint64_t>(), 0, dlen.as<uint32_t>(),
               dids.as<uint32_t>(), m, alpha, dout.as<uint32_t>(), dol.as<uint32_t>(), err.as<uint32_t>(), nullptr,
               nullptr); });
  if (!huge.empty()) {
    CHK(dd.reserve(std::max<uint64_t>(4, conn.size() * 4)));
    CHK(dpos.reserve(std::max<uint64_t>(4, conn.size() * 4)));
    HIPCHK(hipMemcpyAsync(dh.p, huge.data(), huge.size() * 4, hipMemcpyHostToDevice, st));
    pmk::cand_dist(st, X, dim, dh.as<uint32_t>(), huge.size(), doff.as<uint64_t>(), dlen.as<uint32_t>(),
                   dids.as<uint32_t>(), dd.as<float>());
    std::vector<float> hd(conn.size());
    if (!conn.empty()) HIPCHK(hipMemcpyAsync(hd.data(), dd.p, conn.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<uint32_t> pos(conn.size());
    par_for(huge.size(), [&](uint64_t a, uint64_t b) {
      std::vector<uint64_t> key;
      for (uint64_t i = a; i < b; ++i) {   // sort.Slice by distance; ties by position (as the LDS sort)
        const uint32_t u = huge[i];
        const uint64_t o = coff[u], len = clen[u];
        key.resize(len);
        for (uint64_t j = 0; j < len; ++j) {
          uint32_t bits;
          memcpy(&bits, &hd[o + j], 4);
          key[j] = ((uint64_t)bits << 32) | j;
        }
        std::sort(key.begin(), key.end());
        for (uint64_t j = 0; j < len; ++j) pos[o + j] = (uint32_t)key[j];
      }
    });
    if (!pos.empty()) HIPCHK(hipMemcpyAsync(dpos.p, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, st));
    c->timed("prune", 0.0, [&] {
      pmk::prune(st, X, dim, wide, dh.as<uint32_t>(), huge.size(), doff.as<uint64_t>(), 0, dlen.as<uint32_t>(),
                 dids.as<uint32_t>(), m, alpha, dout.as<uint32_t>(), dol.as<uint32_t>(), err.as<uint32_t>(),
                 dpos.as<uint32_t>(), dd.as<float>()); });
  }
  P.resize(n * m);
  PL.resize(n);
  HIPCHK(hipMemcpyAsync(P.data(), dout.p, n * m * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(PL.data(), dol.p, n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(e, err.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// What the candidate stage hands to the rest of the build: the device f32 rows
// and every vertex's candidates (out [n][K], len [n] valid each).
struct BuildCand {
  const float* x = nullptr;
  const uint32_t* out = nullptr;
  const uint32_t* len = nullptr;
};

// The build after its argument checks.  upload() puts the rows on the device,
// candidates(bc) enqueues the exact kNN of every vertex (K results, self
// dropped) and fills bc; everything else is the same for every entry point: the
// first robustPrune, the host edge work, prune_lists and the fill, all over
// bc.x.
template <class Up, class Cand>
static int build_graph_core(pm_ctx* c, uint64_t n, uint64_t dim, uint64_t m, float alpha, uint64_t seed,
                            uint32_t* graph, double* times, bool wide, uint32_t K, Up&& upload, Cand&& candidates) {
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  auto t0 = Clock::now();
  CHK(upload());
  DevBuf g1, len1, err;
  CHK(g1.reserve(n * m * 4));
  CHK(len1.reserve(n * 4));
  CHK(err.reserve(4));
  HIPCHK(hipMemsetAsync(err.p, 0, 4, st));
  // candidates: NGT.Search(u, 1.5m) with u removed (:398-410), exact here
  BuildCand bc;
  CHK(candidates(bc));
  HIPCHK(hipStreamSynchronize(st));
  auto t1 = Clock::now();
  // first pass: robustPrune(vectors, u, candidates, m, alpha) (:413-414)
  c->timed("prune", 0.0, [&] {
    pmk::prune(st, bc.x, (uint32_t)dim, wide, nullptr, n, nullptr, K, bc.len, bc.out, (uint32_t)m, alpha,
               g1.as<uint32_t>(), len1.as<uint32_t>(), err.as<uint32_t>(), nullptr, nullptr); });
  std::vector<uint32_t> G(n * m), L1(n);
  uint32_t e = 0;
  HIPCHK(hipMemcpyAsync(G.data(), g1.p, n * m * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(L1.data(), len1.p, n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&e, err.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (e) return fail(PM_EINVAL, "robustPrune: candidate list above the kernel's limit");
  auto t2 = Clock::now();
  // bi-directional edges (:421-430): biGraph[x] = [u < x with x in graph[u]] ++
  // graph[x] ++ [u > x with x in graph[u]], u ascending, with multiplicity
  std::vector<uint64_t> roff(n + 1, 0);
  for (uint64_t u = 0; u < n; ++u)
    for (uint32_t j = 0; j < L1[u]; ++j) roff[G[u * m + j] + 1]++;
  for (uint64_t x = 0; x < n; ++x) roff[x + 1] += roff[x];
  std::vector<uint32_t> rev(roff[n]);
  {
    std::vector<uint64_t> fillp(roff.begin(), roff.end() - 1);
    for (uint64_t u = 0; u < n; ++u)
      for (uint32_t j = 0; j < L1[u]; ++j) rev[fillp[G[u * m + j]]++] = (uint32_t)u;
  }
  std::vector<uint32_t> inb(n);   // inbounds = len(biGraph) (:433-436)
  for (uint64_t x = 0; x < n; ++x) inb[x] = (uint32_t)(L1[x] + roff[x + 1] - roff[x]);
  // sampling (:448-462): keep edge j of u with probability min(1.5m / inbounds[v], 1)
  std::vector<uint32_t> clen2(n);
  std::vector<uint64_t> coff(n + 1, 0);
  auto visit = [&](uint64_t x, auto&& fn) {   // biGraph[x] in order
    const uint32_t* r = rev.data() + roff[x];
    const uint64_t nr = roff[x + 1] - roff[x];
    uint64_t a = 0, j = 0;
    while (a < nr && r[a] < x) fn(j++, r[a++]);
    for (uint32_t i = 0; i < L1[x]; ++i) fn(j++, G[x * m + i]);
    while (a < nr) fn(j++, r[a++]);
  };
  auto keep = [&](uint64_t u, uint64_t j, uint32_t v) {
    const double prob = std::min(1.5 * (double)m / (double)inb[v], 1.0);
    const double r = (double)(hash4(seed, DOM_GRAPH_SAMPLE, u, j, 0) >> 11) * 0x1.0p-53;
    return r < prob;
  };
  par_for(n, [&](uint64_t a, uint64_t b) {
    for (uint64_t u = a; u < b; ++u) {
      uint32_t cnt = 0;
      visit(u, [&](uint64_t j, uint32_t v) { cnt += keep(u, j, v); });
      clen2[u] = cnt;
    }
  });
  for (uint64_t u = 0; u < n; ++u) coff[u + 1] = coff[u] + clen2[u];
  std::vector<uint32_t> conn(coff[n]);
  par_for(n, [&](uint64_t a, uint64_t b) {
    for (uint64_t u = a; u < b; ++u) {
      uint32_t* o = conn.data() + coff[u];
      visit(u, [&](uint64_t j, uint32_t v) { if (keep(u, j, v)) *o++ = v; });
    }
  });
  // second pass: robustPrune of the lists above m (:464-466) on the GPU
  // (prune_lists), those above the kernel's LDS sort presorted
  std::vector<uint32_t> big, huge;
  for (uint64_t u = 0; u < n; ++u)
    if (clen2[u] > pmk::prune_max_list()) huge.push_back((uint32_t)u);
    else if (clen2[u] > m) big.push_back((uint32_t)u);
  auto t3 = Clock::now();
  if (!big.empty() || !huge.empty()) {
    std::vector<uint32_t> P, PL;
    CHK(prune_lists(c, bc.x, n, (uint32_t)dim, big, huge, coff, clen2, conn, (uint32_t)m, alpha, P, PL, &e, wide));
    if (e) return fail(PM_EINVAL, "robustPrune: a connection list above the kernel's limit");
    for (const auto* lst : {&big, &huge})
      for (uint32_t u : *lst) {   // robustPrune of a list > m returns exactly m
        memcpy(conn.data() + coff[u], &P[(uint64_t)u * m], m * 4);
        clen2[u] = PL[u];
      }
  }
  auto t4 = Clock::now();
  // random fill to exactly m (:468-486)
  par_for(n, [&](uint64_t a, uint64_t b) {
    std::vector<uint32_t> cur;
    for (uint64_t u = a; u < b; ++u) {
      cur.assign(conn.data() + coff[u], conn.data() + coff[u] + std::min<uint64_t>(clen2[u], m));
      uint64_t t = 0;
      while (cur.size() < m) {
        const uint32_t v = (uint32_t)(hash4(seed, DOM_GRAPH_FILL, u, t++, 0) % n);
        if (v == u) continue;
        if (std::find(cur.begin(), cur.end(), v) != cur.end()) continue;
        cur.push_back(v);
      }
      memcpy(graph + u * m, cur.data(), m * 4);
    }
  });
  if (times) {
    times[0] = std::chrono::duration<double>(t1 - t0).count();   // kNN candidates
    times[1] = std::chrono::duration<double>(t2 - t1).count();   // first robustPrune
    times[2] = std::chrono::duration<double>(t3 - t2 + (Clock::now() - t4)).count();   // host edges, sampling, fill
    times[3] = std::chrono::duration<double>(t4 - t3).count();   // second robustPrune
  }
  return 0;
}

// pm_build_graph and pm_build_graph_exact
static int build_graph_impl(pm_ctx* c, const float* vectors, uint64_t n, uint64_t dim, uint64_t m, float alpha,
                            uint64_t seed, uint32_t* graph, double* times, bool exact, uint64_t* fallback,
                            bool wide = false, uint32_t top = pmk::knn_top()) {
  if (!c || !vectors || !graph) return fail(PM_EINVAL, "NULL argument");
  if (wide && !wide_dim_ok(dim)) return fail(PM_EINVAL, kWideDimText);
  const uint32_t K = (uint32_t)((float)m * 1.5f);   // int(float32(m)*1.5) NGT results (build_graph.go:398)
  if (m == 0 || m > pmk::prune_max_m() || K + 1 > top)
    return fail(PM_EINVAL, top == pmk::knn_top()
                               ? "m must be in [1, 42] (1.5 m candidates + self within the 64-key prefilter)"
                               : "m must be in [1, 64] (1.5 m candidates + self within the 128-key prefilter)");
  if (!wide && (dim == 0 || dim > pmk::prune_max_dim() || !pmk::knn_pad_dim((uint32_t)dim)))
    return fail(PM_EINVAL, "dim must be in [1, 192]");
  if (n <= m || n >= (1ull << 32) - 1) return fail(PM_EINVAL, "n must be > m (the random fill needs m other vertices)");
  KnnDev X;
  KnnOut kn;
  return build_graph_core(
      c, n, dim, m, alpha, seed, graph, times, wide, K,
      [&] { return knn_upload(c, vectors, n, (uint32_t)dim, X, exact, wide); },
      [&](BuildCand& bc) {
        CHK(knn_device(c, X, n, X, n, (uint32_t)dim, K, true, false, exact, kn, fallback, top));
        bc = {X.x.as<float>(), kn.out.as<uint32_t>(), kn.len.as<uint32_t>()};
        return 0;
      });
}
extern "C" int pm_build_graph(pm_ctx* c, const float* vectors, uint64_t n, uint64_t dim, uint64_t m, float alpha,
                              uint64_t seed, uint32_t* graph, double* times) {
  return build_graph_impl(c, vectors, n, dim, m, alpha, seed, graph, times, false, nullptr);
}
extern "C" int pm_build_graph_exact(pm_ctx* c, const float* vectors, uint64_t n, uint64_t dim, uint64_t m,
                                    float alpha, uint64_t seed, uint32_t* graph, double* times,
                                    uint64_t* fallback_rows) {
  if (fallback_rows) *fallback_rows = 0;
  return build_graph_impl(c, vectors, n, dim, m, alpha, seed, graph, times, true, fallback_rows);
}
extern "C" int pm_build_graph_wide(pm_ctx* c, const float* vectors, uint64_t n, uint64_t dim, uint64_t m, float alpha,
                                   uint64_t seed, uint32_t* graph, double* times, uint64_t* fallback_rows) {
  if (fallback_rows) *fallback_rows = 0;
  return build_graph_impl(c, vectors, n, dim, m, alpha, seed, graph, times, true, fallback_rows, true);
}
extern "C" int pm_build_graph_k128(pm_ctx* c, const float* vectors, uint64_t n, uint64_t dim, uint64_t m, float alpha,
                                   uint64_t seed, uint32_t* graph, double* times, uint64_t* fallback_rows) {
  if (fallback_rows) *fallback_rows = 0;
  return build_graph_impl(c, vectors, n, dim, m, alpha, seed, graph, times, true, fallback_rows, true,
                          pmk::knn_top_k128());
}

// ---------------------------------------------------------------------------
// uint8 rows (pm_knn_u8, pm_build_graph_u8; pm_graph_u8.hip):
// for values 0..255 and dim <= 256 the integer distance of the int8 matrix
// cores is L2Dist bit for bit, so the candidate stage is two kernels (k_u8_bias,
// k_knn_i8) with no re-rank, certificate or fallback.  The kNN call holds
// n dp + 4 n bytes of the base on the device (dp: dim padded to 64) and a
// staging buffer of at most kU8Stage bytes.  The build also holds the rows as
// f32 (n dim 4 bytes, k_u8_to_f32): robustPrune reads f32 rows.
// ---------------------------------------------------------------------------
static const char* const kU8DimText = "dim must be in [1, 256]";
constexpr uint64_t kU8Stage = 32ull << 20;   // bytes of raw rows on the device at a time
struct KnnDevU8 {
  DevBuf xb, xc, xf;   // biased padded rows, their constants, build: f32 rows
  uint32_t dp = 0;
};
// The rows go up in pieces of at most kU8Stage bytes through one staging buffer
// (the stream orders a piece's kernels before the next piece's copy).
static int knn_upload_u8(pm_ctx* c, const uint8_t* v, uint64_t n, uint32_t dim, KnnDevU8& d, bool want_f32) {
  hipStream_t st = c->stream;
  d.dp = pmk::knn_u8_pad_dim(dim);
  if (!d.dp) return fail(PM_EINVAL, kU8DimText);
  CHK(d.xb.reserve(std::max<uint64_t>(4, n * d.dp)));
  CHK(d.xc.reserve(std::max<uint64_t>(4, n * 4)));
  if (want_f32) CHK(d.xf.reserve(std::max<uint64_t>(4, n * dim * 4)));
  const uint64_t per = std::max<uint64_t>(1, kU8Stage / dim);
  DevBuf stage;
  CHK(stage.reserve(std::max<uint64_t>(4, std::min(n, per) * dim)));
  for (uint64_t r0 = 0; r0 < n; r0 += per) {
    const uint64_t rows = std::min(per, n - r0);
    HIPCHK(hipMemcpyAsync(stage.p, v + r0 * dim, rows * dim, hipMemcpyHostToDevice, st));
    c->timed("u8_bias", (double)rows * dim, [&] {
      pmk::u8_bias(st, stage.as<uint8_t>(), rows, dim, d.dp, d.xb.as<uint8_t>() + r0 * d.dp, d.xc.as<int32_t>() + r0); });
    if (want_f32)
      c->timed("u8_to_f32", (double)rows * dim * 5, [&] {
        pmk::u8_to_f32(st, stage.as<uint8_t>(), rows * dim, d.xf.as<float>() + r0 * dim); });
  }
  HIPCHK(hipStreamSynchronize(st));   // the staging buffer goes away here
  return 0;
}
static void knn_i8_timed(pm_ctx* c, const KnnDevU8& B, uint64_t n, const KnnDevU8& Q, uint64_t nq, uint32_t K,
                         bool self_base, uint32_t* out, float* dist, uint32_t* len) {
  c->timed("knn_prefilter_u8", (double)nq * n * B.dp, [&] {
    pmk::knn_i8(c->stream, B.xb.p, B.xc.as<int32_t>(), n, Q.xb.p, Q.xc.as<int32_t>(), nq, B.dp, K, self_base, out, dist,
                len); });
}

extern "C" uint32_t pm_knn_u8_max_dim(void) { return pmk::knn_u8_max_dim(); }

extern "C" int pm_knn_u8(pm_ctx* c, const uint8_t* base, uint64_t n, uint64_t dim, const uint8_t* queries, uint64_t nq,
                         uint32_t k, int64_t* ids, float* dists) {
  if (!c || !base || (!queries && nq) || (!ids && nq)) return fail(PM_EINVAL, "NULL argument");
  if (!pmk::knn_u8_pad_dim((uint32_t)std::min<uint64_t>(dim, UINT32_MAX))) return fail(PM_EINVAL, kU8DimText);
  if (k == 0 || k > pmk::knn_top_k128()) return fail(PM_EINVAL, kK128KText);
  if (n == 0 || n >= (1ull << 32) - 1) return fail(PM_EINVAL, "n must be in [1, 2^32-1)");
  HIPCHK(hipSetDevice(c->device));
  KnnDevU8 B, Q;
  CHK(knn_upload_u8(c, base, n, (uint32_t)dim, B, false));
  CHK(knn_upload_u8(c, queries, nq, (uint32_t)dim, Q, false));
  DevBuf out, dist, len;
  CHK(out.reserve(std::max<uint64_t>(4, nq * k * 4)));
  CHK(dist.reserve(std::max<uint64_t>(4, nq * k * 4)));
  CHK(len.reserve(std::max<uint64_t>(4, nq * 4)));
  knn_i8_timed(c, B, n, Q, nq, k, false, out.as<uint32_t>(), dist.as<float>(), len.as<uint32_t>());
  std::vector<uint32_t> o(nq * k), l(nq);
  std::vector<float> dd(nq * k);
  HIPCHK(hipMemcpyAsync(o.data(), out.p, nq * k * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(dd.data(), dist.p, nq * k * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(l.data(), len.p, nq * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (uint64_t i = 0; i < nq; ++i)
    for (uint32_t j = 0; j < k; ++j) {
      ids[i * k + j] = j < l[i] ? (int64_t)o[i * k + j] : -1;
      if (dists) dists[i * k + j] = j < l[i] ? dd[i * k + j] : INFINITY;
    }
  return 0;
}

extern "C" int pm_build_graph_u8(pm_ctx* c, const uint8_t* vectors, uint64_t n, uint64_t dim, uint64_t m, float alpha,
                                 uint64_t seed, uint32_t* graph, double* times) {
  if (!c || !vectors || !graph) return fail(PM_EINVAL, "NULL argument");
  if (!pmk::knn_u8_pad_dim((uint32_t)std::min<uint64_t>(dim, UINT32_MAX)) || dim > pmk::prune_max_dim())
    return fail(PM_EINVAL, kU8DimText);
  const uint32_t K = (uint32_t)((float)m * 1.5f);   // int(float32(m)*1.5) NGT results (build_graph.go:398)
  if (m == 0 || m > pmk::prune_max_m() || K + 1 > pmk::knn_top_k128())
    return fail(PM_EINVAL, "m must be in [1, 64] (1.5 m candidates + self within the 128-key list)");
  if (n <= m || n >= (1ull << 32) - 1) return fail(PM_EINVAL, "n must be > m (the random fill needs m other vertices)");
  KnnDevU8 X;
  DevBuf out, len;
  return build_graph_core(
      c, n, dim, m, alpha, seed, graph, times, false, K,
      [&] { return knn_upload_u8(c, vectors, n, (uint32_t)dim, X, true); },
      [&](BuildCand& bc) {
        CHK(out.reserve(std::max<uint64_t>(4, n * K * 4)));
        CHK(len.reserve(std::max<uint64_t>(4, n * 4)));
        knn_i8_timed(c, X, n, X, n, K, true, out.as<uint32_t>(), nullptr, len.as<uint32_t>());
        bc = {X.xf.as<float>(), out.as<uint32_t>(), len.as<uint32_t>()};
        return 0;
      });
}

// pm_robust_prune and pm_robust_prune_wide: k_prune (wide, rows above
// knn_pad_dim's: its form with one row in LDS) on given lists, through the build's own second pass (prune_lists);
// every list by the LDS sort, or every list presorted.
static int robust_prune_impl(pm_ctx* c, const float* vectors, uint64_t n, uint64_t dim, const uint32_t* verts,
                             uint64_t nverts, const uint64_t* offs, const uint32_t* lens, const uint32_t* ids,
                             uint64_t nids, uint32_t m, float alpha, int presorted, uint32_t* out, uint32_t* out_len,
                             uint32_t* err, bool wide) {
  if (!c || !vectors || !verts || !offs || !lens || (!ids && nids) || !out || !out_len || !err)
    return fail(PM_EINVAL, "NULL argument");
  if (wide && !wide_dim_ok(dim)) return fail(PM_EINVAL, kWideDimText);
  if (m == 0 || m > pmk::prune_max_m()) return fail(PM_EINVAL, "m must be in [1, 64]");
  if (!wide && (dim == 0 || dim > pmk::prune_max_dim())) return fail(PM_EINVAL, "dim must be in [1, 256]");
  if (n == 0 || n >= (1ull << 32) - 1) return fail(PM_EINVAL, "n must be in [1, 2^32-1)");
  if (nverts == 0 || nverts > n) return fail(PM_EINVAL, "nverts must be in [1, n]");
  for (uint64_t i = 0; i < nids; ++i)
    if (ids[i] >= n) return fail(PM_EINVAL, "candidate id out of range");
  // the kernel addresses lists and results by vertex: one list per vertex
  std::vector<uint64_t> coff(n + 1, 0);
  std::vector<uint32_t> clen(n, 0);
  std::vector<uint8_t> seen(n, 0);
  for (uint64_t b = 0; b < nverts; ++b) {
    const uint32_t u = verts[b];
    if (u >= n) return fail(PM_EINVAL, "vertex out of range");
    if (seen[u]) return fail(PM_EINVAL, "verts must be distinct");
    if (offs[b] > nids || lens[b] > nids - offs[b]) return fail(PM_EINVAL, "list outside ids");
    seen[u] = 1;
    coff[u] = offs[b];
    clen[u] = lens[b];
  }
  HIPCHK(hipSetDevice(c->device));
  DevBuf X;
  CHK(X.reserve(n * dim * 4));
  HIPCHK(hipMemcpyAsync(X.p, vectors, n * dim * 4, hipMemcpyHostToDevice, c->stream));
  const std::vector<uint32_t> vs(verts, verts + nverts), none, conn(ids, ids + nids);
  std::vector<uint32_t> P, PL;
  CHK(prune_lists(c, X.as<float>(), n, (uint32_t)dim, presorted ? none : vs, presorted ? vs : none, coff, clen, conn, m,
                  alpha, P, PL, err, wide));
  for (uint64_t b = 0; b < nverts; ++b) {
    const uint32_t u = verts[b];
    out_len[b] = PL[u];
    memcpy(out + b * m, &P[(uint64_t)u * m], (size_t)std::min<uint32_t>(PL[u], m) * 4);
  }
  return 0;
}
extern "C" int pm_robust_prune(pm_ctx* c, const float* vectors, uint64_t n, uint64_t dim, const uint32_t* verts,
                               uint64_t nverts, const uint64_t* offs, const uint32_t* lens, const uint32_t* ids,
                               uint64_t nids, uint32_t m, float alpha, int presorted, uint32_t* out,
                               uint32_t* out_len, uint32_t* err) {
  return robust_prune_impl(c, vectors, n, dim, verts, nverts, offs, lens, ids, nids, m, alpha, presorted, out, out_len,
                           err, false);
}
extern "C" int pm_robust_prune_wide(pm_ctx* c, const float* vectors, uint64_t n, uint64_t dim, const uint32_t* verts,
                                    uint64_t nverts, const uint64_t* offs, const uint32_t* lens, const uint32_t* ids,
                                    uint64_t nids, uint32_t m, float alpha, int presorted, uint32_t* out,
                                    uint32_t* out_len, uint32_t* err) {
  return robust_prune_impl(c, vectors, n, dim, verts, nverts, offs, lens, ids, nids, m, alpha, presorted, out, out_len,
                           err, true);
}

// pm_cluster.cpp — k-means and the cluster-search baseline (pm_kmeans,
// pm_cluster_*): the reference's cluster-search.py, the
// Tiptoe-style sqrt(n)-cluster search its headline comparison is made against.
// Every "nearest centroid" is the exact kNN device path of pm_build.cpp
// (knn_upload / knn_device: prefilter, certificate, re-rank, brute fallback)
// with the centroids as base; the member lists, the centroid update, the
// cluster-ordered copy and the ranged scan are the kernels of pm_cluster.hip.
#include "pm_host.h"

enum : uint64_t { DOM_KMEANS_INIT = 12 };   // hash4 stream of pm_kmeans' start

constexpr uint64_t kAssignChunk = 1ull << 18;   // rows per kNN call of an assignment (128 candidates of 4 B each)
constexpr uint64_t kSearchChunk = 1ull << 16;   // queries per pass of pm_cluster_search
constexpr uint64_t kScanPiece = 2048;           // rows per work item of k_cluster_scan

static const char* const kClusterNText = "n must be in [1, 2^32-1)";

// A KnnDev over rows [r0, r0 + rows) of another's buffers; owns nothing.
struct KnnRowsView {
  KnnDev v;
  KnnRowsView(const KnnDev& d, uint64_t r0, uint32_t dim) {
    v.dp = d.dp;
    v.x.p = d.x.as<float>() + r0 * dim;
    v.xb.p = d.xb.as<uint16_t>() + r0 * d.dp;
    v.xl.p = d.xl.as<uint16_t>() + r0 * d.dp;
    v.xn.p = d.xn.as<float>() + r0;
    v.mx.p = d.mx.p;
  }
  ~KnnRowsView() { v.x.p = v.xb.p = v.xl.p = v.xn.p = v.mx.p = nullptr; }
};

// The member lists of a labelling on the device: order [n] (ids by (label, id))
// and offs [nc + 1], with the sort's scratch.
struct ClusterLists {
  DevBuf keys, keys_out, temp, order, offs;
  size_t temp_bytes = 0;
  int reserve(uint64_t n, uint64_t nc) {
    temp_bytes = pmk::cluster_sort_temp(n, nc);
    CHK(keys.reserve(n * 8));
    CHK(keys_out.reserve(n * 8));
    CHK(temp.reserve(std::max<size_t>(8, temp_bytes)));
    CHK(order.reserve(n * 4));
    CHK(offs.reserve((nc + 1) * 8));
    return 0;
  }
  int run(pm_ctx* c, const char* name, const uint32_t* labels, uint64_t n, uint64_t nc) {
    hipError_t e = hipSuccess;
    c->timed(name, (double)n * 4, [&] {
      e = pmk::cluster_sort(c->stream, temp.p, temp_bytes, labels, n, nc, keys.as<uint64_t>(), keys_out.as<uint64_t>(),
                            order.as<uint32_t>(), offs.as<uint64_t>()); });
    HIPCHK(e);
    return 0;
  }
};

// labels [n] = the nearest centroid of every row by (L2Dist, c): pm_knn_k128's
// device path with k = 1, the rows walked in chunks of kAssignChunk.
static int kmeans_assign(pm_ctx* c, const KnnDev& R, uint64_t n, const float* cen, uint64_t nc, uint32_t dim,
                         KnnDev& Cn, KnnOut& o, uint32_t* labels) {
  CHK(knn_upload(c, cen, nc, dim, Cn, true, true, hipMemcpyDeviceToDevice));
  for (uint64_t r0 = 0; r0 < n; r0 += kAssignChunk) {
    const uint64_t rows = std::min(kAssignChunk, n - r0);
    KnnRowsView Q(R, r0, dim);
    CHK(knn_device(c, Cn, nc, Q.v, rows, dim, 1, false, false, true, o, nullptr, pmk::knn_top_k128()));
    HIPCHK(hipMemcpyAsync(labels + r0, o.out.p, rows * 4, hipMemcpyDeviceToDevice, c->stream));
  }
  return 0;
}

extern "C" int pm_kmeans(pm_ctx* c, const float* vectors, uint64_t n, uint64_t dim, uint64_t nc, uint32_t niter,
                         uint64_t seed, const float* init, float* centroids, uint32_t* labels, uint64_t* sizes,
                         uint64_t* moved) {
  if (!c || !vectors || !centroids || !labels) return fail(PM_EINVAL, "NULL argument");
  if (!wide_dim_ok(dim)) return fail(PM_EINVAL, kWideDimText);
  if (n == 0 || n >= (1ull << 32) - 1) return fail(PM_EINVAL, kClusterNText);
  if (nc == 0 || nc > n) return fail(PM_EINVAL, "nc must be in [1, n]");
  if (niter > 10000) return fail(PM_EINVAL, "niter must be in [0, 10000]");
  // the start: init, or rows pick[0 .. nc), the head of a Fisher-Yates shuffle of
  // 0 .. n-1 whose i-th swap partner is i + hash4(seed, 12, i, 0, 0) % (n - i);
  // only the touched entries of the permutation are kept
  std::vector<float> start(nc * dim);
  if (init) {
    memcpy(start.data(), init, nc * dim * 4);
  } else {
    std::unordered_map<uint64_t, uint64_t> perm;
    auto at = [&](uint64_t i) { auto it = perm.find(i); return it == perm.end() ? i : it->second; };
    for (uint64_t i = 0; i < nc; ++i) {
      const uint64_t j = i + hash4(seed, DOM_KMEANS_INIT, i, 0, 0) % (n - i);
      const uint64_t vi = at(i), vj = at(j);
      perm[j] = vi;
      perm[i] = vj;
      memcpy(&start[i * dim], vectors + vj * dim, dim * 4);
    }
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const uint32_t d = (uint32_t)dim;
  KnnDev R, Cn;
  KnnOut o;
  DevBuf cen, lab[2], cnt;
  ClusterLists L;
  CHK(knn_upload(c, vectors, n, d, R, true, true));   // the rows' halves and norms: once per call
  CHK(cen.reserve(nc * dim * 4));
  CHK(lab[0].reserve(n * 4));
  CHK(lab[1].reserve(n * 4));
  CHK(cnt.reserve(8));
  if (niter) CHK(L.reserve(n, nc));
  HIPCHK(hipMemcpyAsync(cen.p, start.data(), nc * dim * 4, hipMemcpyHostToDevice, st));
  if (moved) std::fill(moved, moved + niter + 1, 0);
  int cur = 0;
  CHK(kmeans_assign(c, R, n, cen.as<float>(), nc, d, Cn, o, lab[cur].as<uint32_t>()));
  if (moved) moved[0] = n;
  for (uint32_t t = 1; t <= niter; ++t) {
    CHK(L.run(c, "kmeans_sort", lab[cur].as<uint32_t>(), n, nc));
    c->timed("kmeans_update", (double)n * dim * 4, [&] {
      pmk::kmeans_update(st, R.x.as<float>(), d, L.order.as<uint32_t>(), L.offs.as<uint64_t>(), nc, cen.as<float>()); });
    cur ^= 1;
    CHK(kmeans_assign(c, R, n, cen.as<float>(), nc, d, Cn, o, lab[cur].as<uint32_t>()));
    HIPCHK(hipMemsetAsync(cnt.p, 0, 8, st));
    c->timed("kmeans_moved", (double)n * 8, [&] {
      pmk::kmeans_moved(st, lab[cur].as<uint32_t>(), lab[cur ^ 1].as<uint32_t>(), n, cnt.as<uint64_t>()); });
    uint64_t m = 0;
    HIPCHK(hipMemcpyAsync(&m, cnt.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (moved) moved[t] = m;
    if (m == 0) break;   // a fixed point: the next update would return these centroids
  }
  HIPCHK(hipMemcpyAsync(centroids, cen.p, nc * dim * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(labels, lab[cur].p, n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (sizes) {
    std::fill(sizes, sizes + nc, 0);
    for (uint64_t i = 0; i < n; ++i) sizes[labels[i]]++;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// The cluster-ordered index (cluster_search_index.build_index,
// cluster-search.py:118-131) and its search (:170-198).
// ---------------------------------------------------------------------------
struct pm_cluster {
  pm_ctx* c = nullptr;
  uint64_t n = 0, nc = 0;
  uint32_t dim = 0;
  DevBuf sorted, order;             // the rows in cluster order, their original ids
  KnnDev Cn;                        // the centroids with their halves and norms
  std::vector<uint64_t> offsets;    // [nc + 1]
  std::vector<uint32_t> order_h;    // [n]
  // per-search buffers, kept between calls
  KnnDev Q;
  KnnOut o;
  DevBuf work, woff, lists, out, dist, len;
};

extern "C" int pm_cluster_create(pm_ctx* c, const float* vectors, uint64_t n, uint64_t dim, const float* centroids,
                                 uint64_t nc, const uint32_t* labels, pm_cluster** out) {
  if (!c || !vectors || !centroids || !labels || !out) return fail(PM_EINVAL, "NULL argument");
  if (!wide_dim_ok(dim)) return fail(PM_EINVAL, kWideDimText);
  if (n == 0 || n >= (1ull << 32) - 1) return fail(PM_EINVAL, kClusterNText);
  if (nc == 0 || nc >= (1ull << 32) - 1) return fail(PM_EINVAL, "nc must be in [1, 2^32-1)");
  for (uint64_t i = 0; i < n; ++i)
    if (labels[i] >= nc) return fail(PM_EINVAL, "label out of range (>= nc)");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  std::unique_ptr<pm_cluster> h(new pm_cluster);
  h->c = c;
  h->n = n;
  h->nc = nc;
  h->dim = (uint32_t)dim;
  DevBuf x, lab;
  ClusterLists L;
  CHK(x.reserve(n * dim * 4));
  CHK(lab.reserve(n * 4));
  CHK(L.reserve(n, nc));
  CHK(h->sorted.reserve(n * dim * 4));
  HIPCHK(hipMemcpyAsync(x.p, vectors, n * dim * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(lab.p, labels, n * 4, hipMemcpyHostToDevice, st));
  CHK(L.run(c, "cluster_sort", lab.as<uint32_t>(), n, nc));
  c->timed("cluster_gather", (double)n * dim * 8, [&] {
    pmk::cluster_gather(st, x.as<float>(), n, h->dim, L.order.as<uint32_t>(), h->sorted.as<float>()); });
  CHK(knn_upload(c, centroids, nc, h->dim, h->Cn, true, true));
  h->offsets.resize(nc + 1);
  h->order_h.resize(n);
  HIPCHK(hipMemcpyAsync(h->offsets.data(), L.offs.p, (nc + 1) * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(h->order_h.data(), L.order.p, n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::swap(h->order.p, L.order.p);   // the index keeps order; the sort's scratch goes
  std::swap(h->order.n, L.order.n);
  *out = h.release();
  return 0;
}

extern "C" void pm_cluster_destroy(pm_cluster* h) { delete h; }

extern "C" int pm_cluster_info(pm_cluster* h, uint64_t* n, uint64_t* dim, uint64_t* nc, uint64_t* offsets,
                               uint32_t* order) {
  if (!h) return fail(PM_EINVAL, "NULL argument");
  if (n) *n = h->n;
  if (dim) *dim = h->dim;
  if (nc) *nc = h->nc;
  if (offsets) std::copy(h->offsets.begin(), h->offsets.end(), offsets);
  if (order) std::copy(h->order_h.begin(), h->order_h.end(), order);
  return 0;
}

extern "C" int pm_cluster_search(pm_cluster* h, const float* queries, uint64_t nq, uint32_t k, uint32_t nprobe,
                                 int64_t* ids, float* dists, uint32_t* probed, uint64_t* scanned) {
  if (!h || !queries || !ids) return fail(PM_EINVAL, "NULL argument");
  if (k == 0 || k > pmk::knn_top_k128()) return fail(PM_EINVAL, "k must be in [1, 128]");
  if (nq == 0) return fail(PM_EINVAL, "nq must be > 0");
  if (nprobe == 0 || nprobe > std::min<uint64_t>(h->nc, pmk::knn_top_k128()))
    return fail(PM_EINVAL, "nprobe must be in [1, min(nc, 128)]");
  pm_ctx* c = h->c;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const uint32_t dim = h->dim;
  std::vector<uint32_t> pr, oid, l;
  std::vector<float> dd;
  std::vector<pmk::ScanWork> work;
  std::vector<uint64_t> woff;
  for (uint64_t q0 = 0; q0 < nq; q0 += kSearchChunk) {
    const uint64_t qn = std::min(kSearchChunk, nq - q0);
    // step 1: the nprobe nearest centroids of every query by (L2Dist, c), exact
    CHK(knn_upload(c, queries + q0 * dim, qn, dim, h->Q, true, true));
    CHK(knn_device(c, h->Cn, h->nc, h->Q, qn, dim, nprobe, false, false, true, h->o, nullptr, pmk::knn_top_k128()));
    pr.resize(qn * nprobe);
    HIPCHK(hipMemcpyAsync(pr.data(), h->o.out.p, qn * nprobe * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // step 2: one work item per (query, probed cluster), a cluster above
    // kScanPiece rows in pieces; an empty cluster gives none
    work.clear();
    woff.assign(qn + 1, 0);
    uint64_t total = 0;
    for (uint64_t q = 0; q < qn; ++q) {
      uint64_t rows = 0;
      for (uint32_t p = 0; p < nprobe; ++p) {
        const uint32_t cl = pr[q * nprobe + p];
        const uint64_t a = h->offsets[cl], b = h->offsets[cl + 1];
        rows += b - a;
        for (uint64_t r = a; r < b; r += kScanPiece) work.push_back({r, std::min(b, r + kScanPiece), (uint32_t)q, 0});
      }
      woff[q + 1] = work.size();
      total += rows;
      if (scanned) scanned[q0 + q] = rows;
    }
    if (probed) std::copy(pr.begin(), pr.end(), probed + q0 * nprobe);
    CHK(h->work.reserve(std::max<size_t>(8, work.size() * sizeof(pmk::ScanWork))));
    CHK(h->woff.reserve((qn + 1) * 8));
    CHK(h->lists.reserve(std::max<size_t>(8, work.size() * k * 8)));
    CHK(h->out.reserve(qn * k * 4));
    CHK(h->dist.reserve(qn * k * 4));
    CHK(h->len.reserve(qn * 4));
    if (!work.empty())
      HIPCHK(hipMemcpyAsync(h->work.p, work.data(), work.size() * sizeof(pmk::ScanWork), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->woff.p, woff.data(), (qn + 1) * 8, hipMemcpyHostToDevice, st));
    c->timed("cluster_scan", (double)total * dim * 4, [&] {
      pmk::cluster_scan(st, h->sorted.as<float>(), h->order.as<uint32_t>(), dim, h->Q.x.as<float>(),
                        h->work.as<pmk::ScanWork>(), work.size(), k, h->lists.as<uint64_t>()); });
    c->timed("cluster_merge", (double)work.size() * k * 8, [&] {
      pmk::cluster_merge(st, h->lists.as<uint64_t>(), h->woff.as<uint64_t>(), qn, k, h->out.as<uint32_t>(),
                         h->dist.as<float>(), h->len.as<uint32_t>()); });
    oid.resize(qn * k);
    dd.resize(qn * k);
    l.resize(qn);
    HIPCHK(hipMemcpyAsync(oid.data(), h->out.p, qn * k * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(dd.data(), h->dist.p, qn * k * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(l.data(), h->len.p, qn * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint64_t i = 0; i < qn; ++i)
      for (uint32_t j = 0; j < k; ++j) {
        ids[(q0 + i) * k + j] = j < l[i] ? (int64_t)oid[i * k + j] : -1;
        if (dists) dists[(q0 + i) * k + j] = j < l[i] ? dd[i * k + j] : INFINITY;
      }
  }
  return 0;
}

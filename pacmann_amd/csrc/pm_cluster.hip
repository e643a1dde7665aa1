// pm_cluster.hip — the kernels of pm_kmeans and pm_cluster_* (DESIGN.md §10.5):
//
//   k_cluster_keys / k_cluster_unpack  the member lists: keys (label << idbits | id),
//                       sorted by rocPRIM's device radix sort (the keys are distinct,
//                       so the result is one fixed permutation), then order [n] and
//                       offs [nc + 1] from the label boundaries.  No atomics.
//   k_kmeans_update     the centroid update in a fixed f64 summation order
//   k_kmeans_moved      how many rows changed label (an integer count)
//   k_cluster_gather    the rows in cluster order
//   k_cluster_scan      the brute-force stream of pm_graph_dev.h over a row range of
//                       the cluster-ordered copy, keys carrying the original id
//   k_cluster_merge     a query's lists merged into its first K
//
// The distances of every assignment and probe come from the exact kNN kernels
// (pm_graph*.hip) with the centroids as base; nothing here computes one but
// k_cluster_scan, through l2_group8.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <cstring>

#include "pm_internal.h"
#include "pm_graph_dev.h"

namespace pm {

constexpr int kUpdDims = 64;                              // coordinates per workgroup of k_kmeans_update
constexpr int kUpdLanes = kUpdDims / 4;                   // threads along dim, four coordinates each
constexpr int kUpdParts = (int)pmk::kKmeansPartials;      // partial sums per coordinate
static_assert(kUpdLanes * kUpdParts == kBlock, "one thread per (partial, four coordinates)");
constexpr int kScanMaxDim = 1024;                         // the widest row (knn_pad_dim_wide)

__global__ void __launch_bounds__(kBlock) k_cluster_keys(const uint32_t* __restrict__ labels, uint64_t n,
                                                         uint32_t idbits, uint64_t* __restrict__ keys) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
    keys[i] = ((uint64_t)labels[i] << idbits) | i;
}

// order[r] = the id of sorted key r; offs[c] = the first r whose label is >= c
// (offs[nc] = n): position r writes offs for the labels in (label[r - 1],
// label[r]], the last position also those above its own.
__global__ void __launch_bounds__(kBlock) k_cluster_unpack(const uint64_t* __restrict__ keys, uint64_t n, uint64_t nc,
                                                           uint32_t idbits, uint32_t* __restrict__ order,
                                                           uint64_t* __restrict__ offs) {
  const uint64_t mask = (1ull << idbits) - 1;
  for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (uint64_t)gridDim.x * kBlock) {
    const uint64_t key = keys[r];
    const uint64_t lab = key >> idbits;
    order[r] = (uint32_t)(key & mask);
    const uint64_t from = r ? (keys[r - 1] >> idbits) + 1 : 0;
    for (uint64_t c = from; c <= lab; ++c) offs[c] = r;
    if (r + 1 == n)
      for (uint64_t c = lab + 1; c <= nc; ++c) offs[c] = n;
  }
}

// Centroid c = the mean of rows order[offs[c] .. offs[c + 1]) (ascending id), or
// unchanged when there is none.  Coordinate j: partial sum p of 16 adds members
// p, p + 16, ... in that order in f64 from +0.0; the total is partial 0 plus
// partials 1 .. 15 in order; the mean is total / size in f64, rounded once to
// f32.  A workgroup is one (cluster, 64 coordinates): thread (p, l) holds
// partial p of coordinates 4 l .. 4 l + 3, so the 16 threads of a partial read
// 256 contiguous bytes of a member row (16-byte loads when dim is a multiple
// of 4).  The order depends on the member list alone: a large cluster is
// shared among workgroups only along dim.
__global__ void __launch_bounds__(kBlock) k_kmeans_update(const float* __restrict__ rows, uint32_t dim,
                                                          const uint32_t* __restrict__ order,
                                                          const uint64_t* __restrict__ offs, uint64_t nc,
                                                          float* __restrict__ centroids) {
  __shared__ double part[kUpdParts][kUpdDims];
  const uint32_t tid = threadIdx.x, p = tid / kUpdLanes, l = tid % kUpdLanes;
  const uint32_t j0 = blockIdx.y * kUpdDims + 4 * l;
  const bool vec = (dim & 3) == 0;
  for (uint64_t c = blockIdx.x; c < nc; c += gridDim.x) {
    const uint64_t a = offs[c], b = offs[c + 1];
    if (a == b) continue;   // uniform: the empty cluster keeps its centroid
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (j0 < dim) {
      for (uint64_t m = a + p; m < b; m += kUpdParts) {
        const float* row = rows + (uint64_t)order[m] * dim + j0;
        if (vec) {
          const float4 v = *(const float4*)row;
          s[0] += (double)v.x;
          s[1] += (double)v.y;
          s[2] += (double)v.z;
          s[3] += (double)v.w;
        } else {
          #pragma unroll
          for (uint32_t i = 0; i < 4; ++i)
            if (j0 + i < dim) s[i] += (double)row[i];
        }
      }
    }
    #pragma unroll
    for (uint32_t i = 0; i < 4; ++i) part[p][4 * l + i] = s[i];
    __syncthreads();
    const uint32_t j = blockIdx.y * kUpdDims + tid;
    if (tid < kUpdDims && j < dim) {
      double t = part[0][tid];
      for (uint32_t q = 1; q < (uint32_t)kUpdParts; ++q) t += part[q][tid];
      centroids[c * dim + j] = (float)(t / (double)(b - a));
    }
    __syncthreads();   // part is reused by the next cluster
  }
}

__global__ void __launch_bounds__(kBlock) k_kmeans_moved(const uint32_t* __restrict__ cur,
                                                         const uint32_t* __restrict__ prev, uint64_t n,
                                                         unsigned long long* __restrict__ count) {
  uint32_t mine = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
    mine += cur[i] != prev[i];
  #pragma unroll
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, (unsigned long long)mine);   // an integer sum: any order
}

// One wave per row: out row r = rows[order[r]].
__global__ void __launch_bounds__(kBlock) k_cluster_gather(const float* __restrict__ rows, uint64_t n, uint32_t dim,
                                                           const uint32_t* __restrict__ order,
                                                           float* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint64_t r = (uint64_t)blockIdx.x * (kBlock / 64) + w; r < n; r += (uint64_t)gridDim.x * (kBlock / 64)) {
    const float* src = rows + (uint64_t)order[r] * dim;
    float* dst = out + r * dim;
    if ((dim & 3) == 0) {
      for (uint32_t j = 4 * lane; j < dim; j += 256) *(float4*)(dst + j) = *(const float4*)(src + j);
    } else {
      for (uint32_t j = lane; j < dim; j += 64) dst[j] = src[j];
    }
  }
}

// knn_brute_stream (pm_graph_dev.h) over the rows [r0, r1) of the
// cluster-ordered copy S, the key carrying order[r]: one workgroup per work
// item (a query and a probed cluster, or a piece of a large one); wave 0 writes
// the first K keys of the merged top-128.
__global__ void __launch_bounds__(kBlock) k_cluster_scan(const float* __restrict__ S,
                                                         const uint32_t* __restrict__ order, uint32_t dim,
                                                         const float* __restrict__ Q,
                                                         const pmk::ScanWork* __restrict__ work, uint64_t nwork,
                                                         uint32_t K, uint64_t* __restrict__ lists) {
  __shared__ BruteLds<kKnnTop2, kScanMaxDim> L;
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t e = blockIdx.x; e < nwork; e += gridDim.x) {
    const pmk::ScanWork wk = work[e];
    const TopKeys<kKnnTop2> t = knn_brute_stream(L, S, dim, Q + (uint64_t)wk.q * dim, wk.r0, wk.r1, order);
    if (threadIdx.x < 64) {
      #pragma unroll
      for (int i = 0; i < t.H; ++i)
        if (64 * i + lane < K) lists[e * K + 64 * i + lane] = t.v[i];
    }
    __syncthreads();   // L is reused by the next work item
  }
}

// One wave per query: the K smallest keys of its lists (each ascending, kNoKey
// padded), written as TopKeys::emit writes a row.
__global__ void __launch_bounds__(kBlock) k_cluster_merge(const uint64_t* __restrict__ lists,
                                                          const uint64_t* __restrict__ woff, uint64_t nq, uint32_t K,
                                                          uint32_t* __restrict__ out, float* __restrict__ dist_out,
                                                          uint32_t* __restrict__ len) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t q = (uint64_t)blockIdx.x * (kBlock / 64) + w;
  if (q >= nq) return;
  TopKeys<kKnnTop2> t = TopKeys<kKnnTop2>::empty();
  for (uint64_t e = woff[q]; e < woff[q + 1]; ++e)
    for (uint32_t i = 0; i < K; ++i) {
      const uint64_t key = lists[e * K + i];   // the same address in every lane
      if (key == kNoKey) break;
      t.insert(key, lane);
    }
  t.emit(q, K, 0, lane, out, dist_out, len);
}

}  // namespace pm

namespace pmk {
static inline unsigned cgrid(uint64_t items, uint64_t per) {
  const uint64_t b = (items + per - 1) / per;
  return (unsigned)(b < 1 ? 1 : b < (1u << 20) ? b : (1u << 20));
}
static inline uint32_t host_bits_for(uint64_t count) {
  uint32_t b = 1;
  while (b < 64 && (count - 1) >> b) ++b;
  return b;
}

size_t cluster_sort_temp(uint64_t n, uint64_t nc) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_keys(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)n, 0u,
                                 host_bits_for(n) + host_bits_for(nc));
  return bytes;
}

hipError_t cluster_sort(hipStream_t st, void* temp, size_t temp_bytes, const uint32_t* labels, uint64_t n, uint64_t nc,
                        uint64_t* keys, uint64_t* keys_out, uint32_t* order, uint64_t* offs) {
  const uint32_t idbits = host_bits_for(n), labbits = host_bits_for(nc);
  hipLaunchKernelGGL(k_cluster_keys, dim3(cgrid(n, kBlock)), dim3(kBlock), 0, st, labels, n, idbits, keys);
  const hipError_t e = rocprim::radix_sort_keys(temp, temp_bytes, (const uint64_t*)keys, keys_out, (size_t)n, 0u,
                                                idbits + labbits, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_cluster_unpack, dim3(cgrid(n, kBlock)), dim3(kBlock), 0, st, (const uint64_t*)keys_out, n, nc,
                     idbits, order, offs);
  return hipSuccess;
}

void kmeans_update(hipStream_t st, const float* rows, uint32_t dim, const uint32_t* order, const uint64_t* offs,
                   uint64_t nc, float* centroids) {
  hipLaunchKernelGGL(k_kmeans_update, dim3(cgrid(nc, 1), (dim + kUpdDims - 1) / kUpdDims), dim3(kBlock), 0, st, rows,
                     dim, order, offs, nc, centroids);
}

void kmeans_moved(hipStream_t st, const uint32_t* cur, const uint32_t* prev, uint64_t n, uint64_t* count) {
  hipLaunchKernelGGL(k_kmeans_moved, dim3(cgrid(n, 4 * kBlock)), dim3(kBlock), 0, st, cur, prev, n,
                     (unsigned long long*)count);
}

void cluster_gather(hipStream_t st, const float* rows, uint64_t n, uint32_t dim, const uint32_t* order, float* out) {
  hipLaunchKernelGGL(k_cluster_gather, dim3(cgrid(n, kBlock / 64)), dim3(kBlock), 0, st, rows, n, dim, order, out);
}

void cluster_scan(hipStream_t st, const float* S, const uint32_t* order, uint32_t dim, const float* Q,
                  const ScanWork* work, uint64_t nwork, uint32_t K, uint64_t* lists) {
  if (!nwork) return;
  hipLaunchKernelGGL(k_cluster_scan, dim3(cgrid(nwork, 1)), dim3(kBlock), 0, st, S, order, dim, Q, work, nwork, K,
                     lists);
}

void cluster_merge(hipStream_t st, const uint64_t* lists, const uint64_t* woff, uint64_t nq, uint32_t K, uint32_t* out,
                   float* dist, uint32_t* len) {
  if (!nq) return;
  hipLaunchKernelGGL(k_cluster_merge, dim3((unsigned)((nq + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, st,
                     lists, woff, nq, K, out, dist, len);
}
}  // namespace pmk

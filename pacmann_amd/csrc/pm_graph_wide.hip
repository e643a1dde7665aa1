// pm_graph_wide.hip — the exact kNN and robustPrune for rows of 193 to 1,024
// dimensions (pm_knn_wide, pm_build_graph_wide).  The kernels
// of pm_graph.hip keep a whole padded row in registers or LDS (a[KS],
// b[cols][DP + 8], acc[65][264], q[192]); these walk the row in pieces:
//
//   k_knn_bf16x3_w  k_knn_bf16x3 at a runtime row width dp (a multiple of 64):
//                   K is walked in chunks of 64, the hi and lo chunks of the
//                   64 query rows and the 64 base columns double-buffered in
//                   LDS, one accumulator carried across the whole K extent
//   k_knn_brute_w   k_knn_brute with a 1,024-float query row in LDS
//   k_prune_w       k_prune with only the candidate under test in LDS; the
//                   accepted rows are read from X by their ids
//
// k_to_bf16x2, k_knn_rerank_cert and k_cand_dist (pm_graph.hip) take any dim
// and dp and are launched as they are.
#include <hip/hip_runtime.h>

#include "pm_internal.h"
#include "pm_graph_dev.h"

namespace pm {

constexpr int kKnnWCols = 64;      // base rows per tile
constexpr int kKnnWThreads = 256;  // 4 waves: 2 row blocks x 2 column blocks of 32x32
constexpr int kKnnWChunk = 64;     // K extent held in LDS at a time
constexpr int kKnnWMaxDim = 1024;  // the widest row knn_pad_dim_wide() accepts

struct KnnWLds {
  uint64_t top[kKnnRows][kKnnTop];          // sorted ascending per row
  uint64_t buf[kKnnRows][kKnnWCols];        // this tile's keys below the row threshold
  uint32_t cnt[kKnnRows];
  uint32_t any[2];
  // one K chunk of the query rows and of the base tile, both halves, two
  // buffers; padded rows: conflict-free 16-B fragment reads
  __bf16 qh[2][kKnnRows][kKnnWChunk + 8];
  __bf16 ql[2][kKnnRows][kKnnWChunk + 8];
  __bf16 bh[2][kKnnWCols][kKnnWChunk + 8];
  __bf16 bl[2][kKnnWCols][kKnnWChunk + 8];
};
static_assert(sizeof(KnnWLds) <= 160 * 1024, "LDS of one CU");

// The contract of k_knn_bf16x3 (pm_graph.hip) for rows of dp bf16 values, dp a
// multiple of kKnnWChunk: per query row the 64 smallest (prefilter distance
// bits, id) keys over all base rows, sorted, the prefilter distance tau of the
// 64th (NaN bits while fewer than 64 keys exist) and, when out_hi is given, the
// keys' distances.  q.x = lo.hi' + hi.lo' + hi.hi' per k-step of 16 into one
// accumulator that lives across the row's dp / 64 chunks.  A step is one chunk
// of one tile; step s + 1's four chunk pieces travel from global memory to
// registers during step s's MFMAs and into the other LDS buffer behind them,
// so one barrier per step orders both buffers.  The query chunks are read again
// for every tile (they stay in L2); nothing is held for a whole row.
__global__ void __launch_bounds__(kKnnWThreads) k_knn_bf16x3_w(const __bf16* __restrict__ Xh,
                                                               const __bf16* __restrict__ Xl,
                                                               const float* __restrict__ xn, uint64_t N,
                                                               const __bf16* __restrict__ Qh,
                                                               const __bf16* __restrict__ Ql,
                                                               const float* __restrict__ qn, uint64_t M, uint32_t dp,
                                                               uint32_t* __restrict__ out, float* __restrict__ tau,
                                                               uint32_t* __restrict__ out_hi) {
  constexpr int PER = kKnnRows * kKnnWChunk / 8 / kKnnWThreads;   // 16-B pieces per thread and chunk half
  constexpr int MR = kKnnRows / (kKnnWThreads / 64);              // rows each wave merges
  static_assert(kKnnRows == kKnnWCols && PER * kKnnWThreads * 8 == kKnnRows * kKnnWChunk, "chunk pieces");
  __shared__ KnnWLds L;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t rb = 32 * (w & 1), cb = 32 * (w >> 1);
  const uint32_t r32 = lane & 31, h = lane >> 5;
  const uint64_t row0 = (uint64_t)blockIdx.x * kKnnRows;

  for (uint32_t i = tid; i < kKnnRows * kKnnTop; i += kKnnWThreads) (&L.top[0][0])[i] = kNoKey;
  if (tid < kKnnRows) L.cnt[tid] = 0;
  if (tid < 2) L.any[tid] = 0;

  float qnr[16];
  uint32_t thi[16];
  #pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint64_t qr = row0 + rb + (i & 3) + 8 * (i >> 2) + 4 * h;
    qnr[i] = qr < M ? qn[qr] : 0.0f;
    thi[i] = 0xffffffffu;
  }
  const uint32_t NC = dp / kKnnWChunk;                      // chunks per row
  const uint64_t T = (N + kKnnWCols - 1) / kKnnWCols;       // tiles
  const uint64_t S = T * NC;                                // steps
  uint4 pqh[PER], pql[PER], pbh[PER], pbl[PER];
  // step (t, c): chunk c of the query rows and of base tile t
  auto load_step = [&](uint64_t t, uint32_t c) {
    const uint64_t c0 = t * kKnnWCols;
    #pragma unroll
    for (int p = 0; p < PER; ++p) {
      const uint32_t q = tid + p * kKnnWThreads;
      const uint32_t j = q / (kKnnWChunk / 8);
      const uint64_t off = (uint64_t)c * kKnnWChunk + (q % (kKnnWChunk / 8)) * 8;
      if (row0 + j < M) {
        pqh[p] = *(const uint4*)(Qh + (row0 + j) * dp + off);
        pql[p] = *(const uint4*)(Ql + (row0 + j) * dp + off);
      } else {
        pqh[p] = make_uint4(0, 0, 0, 0);
        pql[p] = make_uint4(0, 0, 0, 0);
      }
      if (c0 + j < N) {
        pbh[p] = *(const uint4*)(Xh + (c0 + j) * dp + off);
        pbl[p] = *(const uint4*)(Xl + (c0 + j) * dp + off);
      } else {
        pbh[p] = make_uint4(0, 0, 0, 0);
        pbl[p] = make_uint4(0, 0, 0, 0);
      }
    }
  };
  auto store_step = [&](uint32_t b) {
    #pragma unroll
    for (int p = 0; p < PER; ++p) {
      const uint32_t q = tid + p * kKnnWThreads;
      const uint32_t j = q / (kKnnWChunk / 8), off = (q % (kKnnWChunk / 8)) * 8;
      *(uint4*)&L.qh[b][j][off] = pqh[p];
      *(uint4*)&L.ql[b][j][off] = pql[p];
      *(uint4*)&L.bh[b][j][off] = pbh[p];
      *(uint4*)&L.bl[b][j][off] = pbl[p];
    }
  };
  load_step(0, 0);
  store_step(0);
  __syncthreads();
  f32x16 acc = {};
  uint64_t t = 0;
  uint32_t c = 0;
  for (uint64_t s = 0; s < S; ++s) {
    const uint32_t b = (uint32_t)(s & 1);
    const bool more = s + 1 < S;
    const bool last = c + 1 == NC;          // the tile's last chunk
    if (more) load_step(last ? t + 1 : t, last ? 0 : c + 1);   // in flight during the MFMAs
    #pragma unroll
    for (int ks = 0; ks < kKnnWChunk / 16; ++ks) {
      const bf16x8 ah = *(const bf16x8*)&L.qh[b][rb + r32][16 * ks + 8 * h];
      const bf16x8 al = *(const bf16x8*)&L.ql[b][rb + r32][16 * ks + 8 * h];
      const bf16x8 bh = *(const bf16x8*)&L.bh[b][cb + r32][16 * ks + 8 * h];
      const bf16x8 bl = *(const bf16x8*)&L.bl[b][cb + r32][16 * ks + 8 * h];
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
    }
    if (!last) {
      if (more) store_step(b ^ 1);
      __syncthreads();
      ++c;
      continue;
    }
    // the row is complete: the threshold / insert / merge phase of k_knn_bf16x3
    const uint64_t col = t * kKnnWCols + cb + r32;
    if (col < N) {
      const float cn = xn[col];
      #pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint32_t lr = rb + (i & 3) + 8 * (i >> 2) + 4 * h;
        float d = __fsub_rn(__fadd_rn(qnr[i], cn), __fmul_rn(2.0f, acc[i]));
        d = d < 0.0f ? 0.0f : d;
        const uint32_t db = __float_as_uint(d);
        if (db <= thi[i]) {
          const uint64_t key = ((uint64_t)db << 32) | (uint32_t)col;
          if (db < thi[i] || key < L.top[lr][kKnnTop - 1]) {
            const uint32_t slot = atomicAdd(&L.cnt[lr], 1u);
            L.buf[lr][slot] = key;
            L.any[t & 1] = 1;
          }
        }
      }
    }
    #pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    if (tid == 0) L.any[(t + 1) & 1] = 0;
    __syncthreads();
    const bool merged = L.any[t & 1] != 0;   // uniform
    if (merged) {
      for (uint32_t r = w * MR; r < w * MR + MR; ++r) {
        const uint32_t n = L.cnt[r];
        if (n) knn_merge_row(L.top[r], L.buf[r], n, lane);
      }
    }
    if (more) store_step(b ^ 1);
    __syncthreads();
    if (merged) {
      if (lane < MR) L.cnt[w * MR + lane] = 0;
      #pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint32_t lr = rb + (i & 3) + 8 * (i >> 2) + 4 * h;
        thi[i] = (uint32_t)(L.top[lr][kKnnTop - 1] >> 32);
      }
    }
    // cnt resets must land before the next tile's inserts
    if (merged) __syncthreads();
    ++t;
    c = 0;
  }
  for (uint32_t r = w * MR; r < w * MR + MR; ++r) {
    const uint64_t qr = row0 + r;
    if (qr < M) {
      out[qr * kKnnTop + lane] = (uint32_t)L.top[r][lane];
      if (out_hi) out_hi[qr * kKnnTop + lane] = (uint32_t)(L.top[r][lane] >> 32);
      if (lane == kKnnTop - 1) tau[qr] = __uint_as_float((uint32_t)(L.top[r][lane] >> 32));
    }
  }
}

// k_knn_brute (pm_graph.hip) for rows up to kKnnWMaxDim wide: one workgroup per
// listed query row streams all N base rows, L2Dist in the reference order by
// 8-lane groups (the query row in LDS); each wave keeps the sorted 64 smallest
// (dist, id) keys of its rows in registers with the 64th as threshold, wave 0
// merges the four and writes the first K as k_knn_rerank does.
struct BruteWLds {
  uint64_t top[kBlock / 64][kKnnTop];
  float q[kKnnWMaxDim];
};

__global__ void __launch_bounds__(kBlock) k_knn_brute_w(const float* __restrict__ X, uint64_t N, uint32_t dim,
                                                        const float* __restrict__ Q,
                                                        const uint64_t* __restrict__ list, uint64_t nlist, uint32_t K,
                                                        int self_base, uint32_t* __restrict__ out,
                                                        float* __restrict__ dist_out, uint32_t* __restrict__ len) {
  __shared__ BruteWLds L;
  constexpr uint32_t W = kBlock / 64;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 3, k = lane & 7;
  for (uint64_t e = blockIdx.x; e < nlist; e += gridDim.x) {
    const uint64_t row = list[e];
    for (uint32_t i = tid; i < dim; i += kBlock) L.q[i] = Q[row * dim + i];
    __syncthreads();
    uint64_t t = kNoKey;
    for (uint64_t r0 = 8 * w; r0 < N; r0 += 8 * W) {   // uniform per wave: every lane stays active
      const uint64_t r = r0 + g;
      const bool ok = r < N;
      const float d = l2_group8(X + (ok ? r : 0) * dim, L.q, dim, k);
      const uint64_t key = ok ? (((uint64_t)__float_as_uint(d) << 32) | r) : kNoKey;
      uint64_t m = __ballot(k == 0 && key < readlane64(t, 63));
      while (m) {
        const int src = __builtin_ctzll(m);
        m &= m - 1;
        t = knn_insert(t, readlane64(key, src), lane);
      }
    }
    L.top[w][lane] = t;
    __syncthreads();
    if (w == 0) {
      for (uint32_t o = 1; o < W; ++o)
        for (uint32_t i = 0; i < kKnnTop; ++i) t = knn_insert(t, L.top[o][i], lane);
      knn_emit(t, row, K, self_base, lane, out, dist_out, len);
    }
    __syncthreads();   // L.q and L.top are reused by the next listed row
  }
}

constexpr int kPruneWMaxL = 4096;   // candidates per vertex held in LDS (k_prune's kPruneMaxL)
constexpr int kPruneWMaxM = 64;

struct PruneWLds {
  uint64_t key[kPruneWMaxL];        // (L2Dist to u, position): stable order
  float dist[kPruneWMaxL];          // by position
  uint32_t disc[kPruneWMaxL];       // discarded ids in order
  float cand[kKnnWMaxDim];          // the candidate under test
  uint32_t acc_id[kPruneWMaxM];
};

// k_prune (pm_graph.hip) for rows up to kKnnWMaxDim wide, same arguments, lists,
// sort, presorted form, discard cap and err flag.  Only the candidate under
// test lies in LDS; the accepted rows (at most m, read again for every
// candidate, so cache-hot) come from X by acc_id through the same l2_group8,
// whose operand order and sums do not depend on where the rows lie: every
// distance has k_prune's bits.
__global__ void __launch_bounds__(kBlock) k_prune_w(const float* __restrict__ X, uint32_t dim,
                                                    const uint32_t* __restrict__ verts, uint64_t nverts,
                                                    const uint64_t* __restrict__ offs, uint64_t stride,
                                                    const uint32_t* __restrict__ lens,
                                                    const uint32_t* __restrict__ ids, uint32_t m, float alpha,
                                                    uint32_t* __restrict__ out, uint32_t* __restrict__ out_len,
                                                    uint32_t* __restrict__ err,
                                                    const uint32_t* __restrict__ sorted_pos,
                                                    const float* __restrict__ dist_g) {
  __shared__ PruneWLds L;
  const uint64_t b = blockIdx.x;
  if (b >= nverts) return;
  const uint64_t u = verts ? verts[b] : b;
  const uint32_t tid = threadIdx.x, g = tid >> 3, k = tid & 7;
  const uint64_t off = offs ? offs[u] : u * stride;
  const uint32_t n = lens[u];
  const uint32_t* c = ids + off;
  if (n <= m) {
    for (uint32_t i = tid; i < n; i += kBlock) out[u * m + i] = c[i];
    if (tid == 0) out_len[u] = n;
    return;
  }
  const bool pre = sorted_pos != nullptr;
  if (n > kPruneWMaxL && !pre) {
    if (tid == 0) { atomicOr(err, 1u); out_len[u] = 0; }
    return;
  }
  const float* xu = X + u * dim;
  if (!pre) {
    // dist2u (:176-182) in L2Dist order; 32 candidates per round
    for (uint32_t r = 0; r < n; r += kBlock / 8) {
      const uint32_t i = r + g;
      const uint32_t id = i < n ? c[i] : 0;
      const float d = l2_group8(xu, X + (uint64_t)id * dim, dim, k);
      if (i < n && k == 0) {
        L.dist[i] = d;
        L.key[i] = ((uint64_t)__float_as_uint(d) << 32) | i;
      }
    }
    uint32_t np2 = 64;
    while (np2 < n) np2 <<= 1;
    for (uint32_t i = n + tid; i < np2; i += kBlock) L.key[i] = kNoKey;
    __syncthreads();
    // sort.Slice by distance (:184-186); ties by position (stable)
    for (uint32_t kk = 2; kk <= np2; kk <<= 1) {
      for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
        for (uint32_t i = tid; i < np2; i += kBlock) {
          const uint32_t p = i ^ j;
          if (p > i) {
            const uint64_t x = L.key[i], y = L.key[p];
            const bool up = (i & kk) == 0;
            if ((x > y) == up) { L.key[i] = y; L.key[p] = x; }
          }
        }
        __syncthreads();
      }
    }
  }   // !pre
  // the greedy pass (:188-212): candidate v is accepted unless an accepted a_j
  // has L2Dist(a_j, v) * alpha < dist(u, v); the a_j are tested 32 at a time
  uint32_t na = 0, nd = 0;
  for (uint32_t s = 0; s < n; ++s) {
    const uint32_t pos = pre ? sorted_pos[off + s] : (uint32_t)L.key[s];
    const uint32_t v = c[pos];
    const float duv = pre ? dist_g[off + pos] : L.dist[pos];
    const float* xv = X + (uint64_t)v * dim;
    for (uint32_t i = tid; i < dim; i += kBlock) L.cand[i] = xv[i];
    __syncthreads();   // also: acc_id[na - 1] of the accept before
    bool rej = false;
    for (uint32_t a = g; a < na; a += kBlock / 8) {   // 32 groups: two rounds once na > 32 (m up to 64)
      const float d = l2_group8(X + (uint64_t)L.acc_id[a] * dim, L.cand, dim, k);
      rej |= __fmul_rn(d, alpha) < duv;
    }
    const bool any = __syncthreads_or(rej);
    if (!any) {
      if (tid == 0) L.acc_id[na] = v;
      ++na;
      if (na == m) break;
    } else {
      if (tid == 0 && nd < kPruneWMaxL) L.disc[nd] = v;
      ++nd;
    }
  }
  __syncthreads();
  // too few accepted: the discarded ones in order (:216-223)
  for (uint32_t i = tid; i < na; i += kBlock) out[u * m + i] = L.acc_id[i];
  const uint32_t fill = na < m ? (m - na < nd ? m - na : nd) : 0;
  for (uint32_t i = tid; i < fill; i += kBlock) out[u * m + na + i] = L.disc[i];
  if (tid == 0) out_len[u] = na + fill;
}

}  // namespace pm

namespace pmk {
static inline unsigned gcdiv(uint64_t a, uint64_t b) { return (unsigned)((a + b - 1) / b); }

uint32_t knn_pad_dim_wide(uint32_t dim) {
  return dim == 0 || dim > (uint32_t)kKnnWMaxDim ? 0 : (dim + kKnnWChunk - 1) / kKnnWChunk * kKnnWChunk;
}
void knn_prefilter_x3_w(hipStream_t st, const void* Xh, const void* Xl, const float* xn, uint64_t N, const void* Qh,
                        const void* Ql, const float* qn, uint64_t M, uint32_t dp, uint32_t* out, float* tau,
                        uint32_t* out_hi) {
  if (!M) return;
  hipLaunchKernelGGL(k_knn_bf16x3_w, dim3(gcdiv(M, kKnnRows)), dim3(kKnnWThreads), 0, st, (const __bf16*)Xh,
                     (const __bf16*)Xl, xn, N, (const __bf16*)Qh, (const __bf16*)Ql, qn, M, dp, out, tau, out_hi);
}
void knn_brute_w(hipStream_t st, const float* X, uint64_t N, uint32_t dim, const float* Q, const uint64_t* list,
                 uint64_t nlist, uint32_t K, bool self_base, uint32_t* out, float* dist, uint32_t* len) {
  if (!nlist) return;
  hipLaunchKernelGGL(k_knn_brute_w, dim3((unsigned)(nlist < (1u << 20) ? nlist : (1u << 20))), dim3(kBlock), 0, st, X,
                     N, dim, Q, list, nlist, K, (int)self_base, out, dist, len);
}
void prune_w(hipStream_t st, const float* X, uint32_t dim, const uint32_t* verts, uint64_t nverts,
             const uint64_t* offs, uint64_t stride, const uint32_t* lens, const uint32_t* ids, uint32_t m,
             float alpha, uint32_t* out, uint32_t* out_len, uint32_t* err, const uint32_t* sorted_pos,
             const float* dist_g) {
  if (!nverts) return;
  hipLaunchKernelGGL(k_prune_w, dim3((unsigned)nverts), dim3(kBlock), 0, st, X, dim, verts, nverts, offs, stride,
                     lens, ids, m, alpha, out, out_len, err, sorted_pos, dist_g);
}
}  // namespace pmk

// pm_graph.hip — graph construction and ground truth on the GPU (SURVEY.md
// §8f rank 1: the reference builds its degree-m graph with NGT candidates,
// robustPrune (alpha = 1.2), reverse-edge sampling and a random fill,
// graphann/build_graph.go:169-236,314-523; NGT is not in the image, so the
// candidates here are the exact k nearest neighbours).
//
//   k_to_bf16     rows -> bf16 rows padded to DP (a multiple of 64) + f32 norms
//   k_knn_bf16    per query row, the 64 smallest (bf16 distance, id) keys over
//                 all base rows: MFMA 32x32x16 bf16 tiles, per-row thresholds,
//                 LDS insertion buffers merged into a sorted top-64 per row
//   k_knn_rerank  the 64 prefilter candidates re-ranked by the reference's own
//                 L2Dist (l2_distance_amd64.s order) and id: top K, self dropped
//   k_prune       robustPrune (build_graph.go:169-236) per vertex: candidate
//                 distances in L2Dist order, stable sort, the alpha test of each
//                 candidate against every accepted neighbour in parallel
//
// Integer-valued inputs up to 255 (SIFT bvecs semantics, loader.go:46-51) are
// exact in bf16 and every bf16 product/partial sum is an exact f32 integer, so
// the prefilter distances are exact and the top-64 holds the exact top-K: the
// result equals a brute-force L2Dist ranking bit for bit.  For general float
// data the prefilter ranks by bf16-rounded distances and keeps 64 candidates
// for the exact re-rank of the top K (K <= 48 in the graph build).
//
// The exact variants (pm_knn_exact, pm_build_graph_exact) are
// exact for every finite float input:
//   k_to_bf16x2        rows -> hi = bf16(x), lo = bf16(x - hi), f32 norms of x,
//                      the largest norm
//   k_knn_bf16x3       k_knn_bf16 with q.x = hi.hi' + hi.lo' + lo.hi' (three
//                      MFMAs per k-step, 64-column tiles); also the prefilter
//                      distance tau of each row's 64th key
//   k_knn_rerank_cert  k_knn_rerank plus the certificate: the row is exact if
//                      its K-th re-ranked distance < tau - eps; other rows go
//                      to a list
//   k_knn_brute        the listed rows by brute force in L2Dist order
#include <hip/hip_runtime.h>

#include "pm_internal.h"
#include "pm_graph_dev.h"

namespace pm {

constexpr int kKnnCols = 128;     // base rows per tile
constexpr int kKnnThreads = 512;  // 8 waves: 2 row blocks x 4 column blocks of 32x32
constexpr int kKnnMaxDim = 192;   // the widest row knn_pad_dim() accepts

// rows [n][dim] f32 -> out [n][dp] bf16 (zero padded), norms [n] = sum of the
// squared bf16 values in element order (exact for integer-valued rows)
__global__ void __launch_bounds__(kBlock) k_to_bf16(const float* __restrict__ rows, uint64_t n, uint32_t dim,
                                                    uint32_t dp, __bf16* __restrict__ out,
                                                    float* __restrict__ norms) {
  const uint64_t r = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (r >= n) return;
  float s = 0.0f;
  for (uint32_t c0 = 0; c0 < dp; c0 += 64) {
    const uint32_t c = c0 + lane;
    const float v = c < dim ? rows[r * dim + c] : 0.0f;
    const __bf16 b = (__bf16)v;
    out[r * dp + c] = b;
    const float f = (float)b;
    float sq = __fmul_rn(f, f);
    // fixed-order wave sum (xor tree), then chunk order
    for (int o = 1; o < 64; o <<= 1) sq = __fadd_rn(sq, __shfl_xor(sq, o));
    s = __fadd_rn(s, sq);
  }
  if (lane == 0) norms[r] = s;
}

// The split form of k_to_bf16: hi = bf16(x), lo = bf16(x - hi) (x - hi is exact
// in f32), both [n][dp] zero padded; norms [n] = sum of the squared f32 values
// in the same fixed order.  maxnorm (nullable) is raised to the largest norm:
// norms are >= +0, so their bit order is their value order and a NaN's bits
// lie above every number's.
__global__ void __launch_bounds__(kBlock) k_to_bf16x2(const float* __restrict__ rows, uint64_t n, uint32_t dim,
                                                      uint32_t dp, __bf16* __restrict__ hi, __bf16* __restrict__ lo,
                                                      float* __restrict__ norms, uint32_t* __restrict__ maxnorm) {
  const uint64_t r = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (r >= n) return;
  float s = 0.0f;
  for (uint32_t c0 = 0; c0 < dp; c0 += 64) {
    const uint32_t c = c0 + lane;
    const float v = c < dim ? rows[r * dim + c] : 0.0f;
    const __bf16 b = (__bf16)v;
    hi[r * dp + c] = b;
    lo[r * dp + c] = (__bf16)__fsub_rn(v, (float)b);
    float sq = __fmul_rn(v, v);
    for (int o = 1; o < 64; o <<= 1) sq = __fadd_rn(sq, __shfl_xor(sq, o));
    s = __fadd_rn(s, sq);
  }
  if (lane == 0) {
    norms[r] = s;
    if (maxnorm) atomicMax(maxnorm, __float_as_uint(s));
  }
}

template <int DP>
struct KnnLds {
  uint64_t top[kKnnRows][kKnnTop];          // sorted ascending per row
  uint64_t buf[kKnnRows][kKnnCols];         // this tile's keys below the row threshold
  uint32_t cnt[kKnnRows];
  uint32_t any[2];
  __bf16 b[kKnnCols][DP + 8];               // padded rows: conflict-free 16-B fragment reads
};

template <int DP>
__global__ void __launch_bounds__(kKnnThreads) k_knn_bf16(const __bf16* __restrict__ X, const float* __restrict__ xn,
                                                          uint64_t N, const __bf16* __restrict__ Q,
                                                          const float* __restrict__ qn, uint64_t M,
                                                          uint32_t* __restrict__ out,
                                                          uint32_t* __restrict__ out_hi) {
  constexpr int KS = DP / 16;                       // MFMA k-steps
  constexpr int CH = kKnnCols * DP / 8;             // 16-B chunks per tile
  constexpr int PER = CH / kKnnThreads;             // per thread
  static_assert(CH % kKnnThreads == 0, "tile chunks");
  __shared__ KnnLds<DP> L;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t rb = 32 * (w & 1), cb = 32 * (w >> 1);
  const uint32_t r32 = lane & 31, h = lane >> 5;
  const uint64_t row0 = (uint64_t)blockIdx.x * kKnnRows;

  for (uint32_t i = tid; i < kKnnRows * kKnnTop; i += kKnnThreads) (&L.top[0][0])[i] = kNoKey;
  if (tid < kKnnRows) L.cnt[tid] = 0;
  if (tid < 2) L.any[tid] = 0;

  // A fragments of this wave's 32 query rows (whole K), kept in registers
  bf16x8 a[KS];
  {
    const uint64_t qr = row0 + rb + r32;
    for (int s = 0; s < KS; ++s) {
      if (qr < M) a[s] = *(const bf16x8*)(Q + qr * DP + 16 * s + 8 * h);
      else for (int j = 0; j < 8; ++j) a[s][j] = (__bf16)0.0f;
    }
  }
  // query norms and thresholds of the lane's 16 output rows
  float qnr[16];
  uint32_t thi[16];
  for (int i = 0; i < 16; ++i) {
    const uint64_t qr = row0 + rb + (i & 3) + 8 * (i >> 2) + 4 * h;
    qnr[i] = qr < M ? qn[qr] : 0.0f;
    thi[i] = 0xffffffffu;
  }
  const uint64_t T = (N + kKnnCols - 1) / kKnnCols;
  uint4 pre[PER];
  auto load_tile = [&](uint64_t t) {
    const uint64_t c0 = t * kKnnCols;
    for (int p = 0; p < PER; ++p) {
      const uint32_t q = tid + p * kKnnThreads;
      const uint32_t j = q / (DP / 8), off = (q % (DP / 8)) * 8;
      if (c0 + j < N) pre[p] = *(const uint4*)(X + (c0 + j) * DP + off);
      else pre[p] = make_uint4(0, 0, 0, 0);
    }
  };
  auto store_tile = [&]() {
    for (int p = 0; p < PER; ++p) {
      const uint32_t q = tid + p * kKnnThreads;
      const uint32_t j = q / (DP / 8), off = (q % (DP / 8)) * 8;
      *(uint4*)&L.b[j][off] = pre[p];
    }
  };
  load_tile(0);
  store_tile();
  __syncthreads();
  for (uint64_t t = 0; t < T; ++t) {
    if (t + 1 < T) load_tile(t + 1);   // in flight during the MFMAs
    f32x16 acc = {};
    for (int s = 0; s < KS; ++s) {
      const bf16x8 bb = *(const bf16x8*)&L.b[cb + r32][16 * s + 8 * h];
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], bb, acc, 0, 0, 0);
    }
    const uint64_t col = t * kKnnCols + cb + r32;
    if (col < N) {
      const float cn = xn[col];
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
    if (tid == 0) L.any[(t + 1) & 1] = 0;
    __syncthreads();
    const bool merged = L.any[t & 1] != 0;   // uniform
    if (merged) {
      for (uint32_t r = w * 8; r < w * 8 + 8; ++r) {
        const uint32_t n = L.cnt[r];
        if (n) knn_merge_row(L.top[r], L.buf[r], n, lane);
      }
    }
    if (t + 1 < T) store_tile();
    __syncthreads();
    if (merged) {
      if (lane < 8) L.cnt[w * 8 + lane] = 0;   // every row of this wave's merge set
      for (int i = 0; i < 16; ++i) {
        const uint32_t lr = rb + (i & 3) + 8 * (i >> 2) + 4 * h;
        thi[i] = (uint32_t)(L.top[lr][kKnnTop - 1] >> 32);
      }
    }
    // cnt resets must land before the next tile's inserts
    if (merged) __syncthreads();
  }
  for (uint32_t r = w * 8; r < w * 8 + 8; ++r) {
    const uint64_t qr = row0 + r;
    if (qr < M) {
      out[qr * kKnnTop + lane] = (uint32_t)L.top[r][lane];
      if (out_hi) out_hi[qr * kKnnTop + lane] = (uint32_t)(L.top[r][lane] >> 32);
    }
  }
}

// The split form of k_knn_bf16 (pm_knn_exact): rows are hi + lo (k_to_bf16x2)
// and q.x is hi.hi' + hi.lo' + lo.hi', three MFMAs per k-step into one
// accumulator, the two small terms of every k-step before the hi.hi' terms.
// Both halves of a base tile lie in LDS, so the tile is 64 columns wide and the
// workgroup has 4 waves (2 row blocks x 2 column blocks of 32x32); each wave
// keeps both halves of its 32 query rows in registers.  Besides the 64
// candidate ids a row gets tau, the prefilter distance of its 64th key (NaN
// while fewer than 64 keys exist): every base row outside the candidates has
// a prefilter distance >= tau.  The fixed-count loops are unrolled by pragma:
// left alone, the compiler keeps some of them rolled at DP = 128 and indexes
// the register arrays through select chains (35,000 instructions).
constexpr int kKnn3Cols = 64;
constexpr int kKnn3Threads = 256;

template <int DP>
struct Knn3Lds {
  uint64_t top[kKnnRows][kKnnTop];
  uint64_t buf[kKnnRows][kKnn3Cols];
  uint32_t cnt[kKnnRows];
  uint32_t any[2];
  __bf16 bh[kKnn3Cols][DP + 8];
  __bf16 bl[kKnn3Cols][DP + 8];
};

template <int DP>
__global__ void __launch_bounds__(kKnn3Threads) k_knn_bf16x3(const __bf16* __restrict__ Xh,
                                                             const __bf16* __restrict__ Xl,
                                                             const float* __restrict__ xn, uint64_t N,
                                                             const __bf16* __restrict__ Qh,
                                                             const __bf16* __restrict__ Ql,
                                                             const float* __restrict__ qn, uint64_t M,
                                                             uint32_t* __restrict__ out, float* __restrict__ tau,
                                                             uint32_t* __restrict__ out_hi) {
  constexpr int KS = DP / 16;
  constexpr int CH = kKnn3Cols * DP / 8;            // 16-B chunks per tile half
  constexpr int PER = CH / kKnn3Threads;
  constexpr int MR = kKnnRows / (kKnn3Threads / 64);   // rows each wave merges
  static_assert(CH % kKnn3Threads == 0, "tile chunks");
  __shared__ Knn3Lds<DP> L;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t rb = 32 * (w & 1), cb = 32 * (w >> 1);
  const uint32_t r32 = lane & 31, h = lane >> 5;
  const uint64_t row0 = (uint64_t)blockIdx.x * kKnnRows;

  for (uint32_t i = tid; i < kKnnRows * kKnnTop; i += kKnn3Threads) (&L.top[0][0])[i] = kNoKey;
  if (tid < kKnnRows) L.cnt[tid] = 0;
  if (tid < 2) L.any[tid] = 0;

  bf16x8 ah[KS], al[KS];
  {
    const uint64_t qr = row0 + rb + r32;
    #pragma unroll
    for (int s = 0; s < KS; ++s) {
      if (qr < M) {
        ah[s] = *(const bf16x8*)(Qh + qr * DP + 16 * s + 8 * h);
        al[s] = *(const bf16x8*)(Ql + qr * DP + 16 * s + 8 * h);
      } else {
        #pragma unroll
        for (int j = 0; j < 8; ++j) ah[s][j] = (__bf16)0.0f;
        #pragma unroll
        for (int j = 0; j < 8; ++j) al[s][j] = (__bf16)0.0f;
      }
    }
  }
  float qnr[16];
  uint32_t thi[16];
  #pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint64_t qr = row0 + rb + (i & 3) + 8 * (i >> 2) + 4 * h;
    qnr[i] = qr < M ? qn[qr] : 0.0f;
    thi[i] = 0xffffffffu;
  }
  const uint64_t T = (N + kKnn3Cols - 1) / kKnn3Cols;
  uint4 preh[PER], prel[PER];
  auto load_tile = [&](uint64_t t) {
    const uint64_t c0 = t * kKnn3Cols;
    #pragma unroll
    for (int p = 0; p < PER; ++p) {
      const uint32_t q = tid + p * kKnn3Threads;
      const uint32_t j = q / (DP / 8), off = (q % (DP / 8)) * 8;
      if (c0 + j < N) {
        preh[p] = *(const uint4*)(Xh + (c0 + j) * DP + off);
        prel[p] = *(const uint4*)(Xl + (c0 + j) * DP + off);
      } else {
        preh[p] = make_uint4(0, 0, 0, 0);
        prel[p] = make_uint4(0, 0, 0, 0);
      }
    }
  };
  auto store_tile = [&]() {
    #pragma unroll
    for (int p = 0; p < PER; ++p) {
      const uint32_t q = tid + p * kKnn3Threads;
      const uint32_t j = q / (DP / 8), off = (q % (DP / 8)) * 8;
      *(uint4*)&L.bh[j][off] = preh[p];
      *(uint4*)&L.bl[j][off] = prel[p];
    }
  };
  load_tile(0);
  store_tile();
  __syncthreads();
  for (uint64_t t = 0; t < T; ++t) {
    if (t + 1 < T) load_tile(t + 1);   // in flight during the MFMAs
    f32x16 acc = {};
    #pragma unroll
    for (int s = 0; s < KS; ++s) {
      const bf16x8 bh = *(const bf16x8*)&L.bh[cb + r32][16 * s + 8 * h];
      const bf16x8 bl = *(const bf16x8*)&L.bl[cb + r32][16 * s + 8 * h];
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[s], bh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s], bl, acc, 0, 0, 0);
    }
    #pragma unroll
    for (int s = 0; s < KS; ++s) {
      const bf16x8 bh = *(const bf16x8*)&L.bh[cb + r32][16 * s + 8 * h];
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s], bh, acc, 0, 0, 0);
    }
    const uint64_t col = t * kKnn3Cols + cb + r32;
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
    if (tid == 0) L.any[(t + 1) & 1] = 0;
    __syncthreads();
    const bool merged = L.any[t & 1] != 0;   // uniform
    if (merged) {
      for (uint32_t r = w * MR; r < w * MR + MR; ++r) {
        const uint32_t n = L.cnt[r];
        if (n) knn_merge_row(L.top[r], L.buf[r], n, lane);
      }
    }
    if (t + 1 < T) store_tile();
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

// One wave per query row: exact L2Dist of the 64 candidates, keys (dist, id),
// sorted; the first K (self dropped when self_base) go to out[row][K], their
// count to len[row].
__global__ void __launch_bounds__(kBlock) k_knn_rerank(const float* __restrict__ X, uint64_t N, uint32_t dim,
                                                       const float* __restrict__ Q, uint64_t M,
                                                       const uint32_t* __restrict__ cand, uint32_t K,
                                                       int self_base, uint32_t* __restrict__ out,
                                                       float* __restrict__ dist_out, uint32_t* __restrict__ len) {
  __shared__ uint64_t keys[kBlock / 64][64];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t row = (uint64_t)blockIdx.x * (kBlock / 64) + w;
  if (row >= M) return;
  const uint64_t x = knn_rerank_keys(X, N, dim, Q + row * dim, cand + row * kKnnTop, keys[w], lane);
  knn_emit(x, row, K, self_base, lane, out, dist_out, len);
}

// k_knn_rerank with the certificate of pm_knn_exact.  The row's result is the
// brute-force one if N <= 64 (every base row is a candidate) or if the K-th
// re-ranked distance is < tau - eps: a base row outside the candidates has a
// prefilter distance >= tau, so an L2Dist >= tau - eps, strictly above all K
// kept keys.  A NaN or an infinity anywhere fails the comparison.  Uncertified
// rows are appended to list (their count in nlist) for k_knn_brute.
__global__ void __launch_bounds__(kBlock) k_knn_rerank_cert(const float* __restrict__ X, uint64_t N, uint32_t dim,
                                                            const float* __restrict__ Q, uint64_t M,
                                                            const uint32_t* __restrict__ cand, uint32_t K,
                                                            int self_base, uint32_t* __restrict__ out,
                                                            float* __restrict__ dist_out, uint32_t* __restrict__ len,
                                                            const float* __restrict__ qn,
                                                            const float* __restrict__ tau,
                                                            const uint32_t* __restrict__ maxnorm, float crel,
                                                            uint64_t* __restrict__ list,
                                                            unsigned long long* __restrict__ nlist,
                                                            float* __restrict__ eps_out) {
  __shared__ uint64_t keys[kBlock / 64][64];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t row = (uint64_t)blockIdx.x * (kBlock / 64) + w;
  if (row >= M) return;
  const uint64_t x = knn_rerank_keys(X, N, dim, Q + row * dim, cand + row * kKnnTop, keys[w], lane);
  knn_emit(x, row, K, self_base, lane, out, dist_out, len);
  if (lane == K - 1 && N > kKnnTop) {
    const float dk = __uint_as_float((uint32_t)(x >> 32));
    const float sum = __fadd_rn(qn[row], __uint_as_float(*maxnorm));
    // rounded up: the factor covers the two roundings of the product and the sum
    const float eps = __fadd_rn(__fmul_rn(__fmul_rn(sum, crel), 1.0f + 0x1.0p-20f), kCertAbs);
    if (eps_out) eps_out[row] = eps;
    const bool ok = x != kNoKey && sum <= kCertMaxSum && (double)dk < (double)tau[row] - (double)eps;
    if (!ok) list[atomicAdd(nlist, 1ull)] = row;
  }
}

// The exact fallback of pm_knn_exact: one workgroup per listed query row
// streams all N base rows, L2Dist in the reference order by 8-lane groups (the
// query row in LDS); each wave keeps the sorted 64 smallest (dist, id) keys of
// its rows in registers with the 64th as threshold, wave 0 merges the four and
// writes the first K as k_knn_rerank does.
struct BruteLds {
  uint64_t top[kBlock / 64][kKnnTop];
  float q[kKnnMaxDim];
};

__global__ void __launch_bounds__(kBlock) k_knn_brute(const float* __restrict__ X, uint64_t N, uint32_t dim,
                                                      const float* __restrict__ Q,
                                                      const uint64_t* __restrict__ list, uint64_t nlist, uint32_t K,
                                                      int self_base, uint32_t* __restrict__ out,
                                                      float* __restrict__ dist_out, uint32_t* __restrict__ len) {
  __shared__ BruteLds L;
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

constexpr int kPruneMaxL = 4096;   // candidates per vertex held in LDS
constexpr int kPruneMaxM = 64;
constexpr int kPruneMaxD = 256;

struct PruneLds {
  uint64_t key[kPruneMaxL];        // (L2Dist to u, position): stable order
  float dist[kPruneMaxL];          // by position
  uint32_t disc[kPruneMaxL];       // discarded ids in order
  float acc[kPruneMaxM + 1][kPruneMaxD + 8];   // accepted vectors; slot na = the candidate under test
  uint32_t acc_id[kPruneMaxM];
};

// robustPrune(vectors, u, candidates, m, alpha) (build_graph.go:169-236) for
// vertex verts[b] (or b): candidates ids[offs[u] .. offs[u] + lens[u]) (offs
// null: u * stride).  Lists of at most m are kept as they are (:170-172).
// Writes out[u][0..len) and out_len[u]; err = 1 if a list exceeds kPruneMaxL.
// Presorted mode (lists above kPruneMaxL, hub vertices): sorted_pos[off + s]
// is the position of the s-th candidate in (L2Dist, position) order and
// dist_g[off + pos] its distance (k_cand_dist, sorted on the host); only the
// first kPruneMaxL discards are kept (the top-up needs at most m).
__global__ void __launch_bounds__(kBlock) k_prune(const float* __restrict__ X, uint32_t dim,
                                                  const uint32_t* __restrict__ verts, uint64_t nverts,
                                                  const uint64_t* __restrict__ offs, uint64_t stride,
                                                  const uint32_t* __restrict__ lens,
                                                  const uint32_t* __restrict__ ids, uint32_t m, float alpha,
                                                  uint32_t* __restrict__ out, uint32_t* __restrict__ out_len,
                                                  uint32_t* __restrict__ err,
                                                  const uint32_t* __restrict__ sorted_pos,
                                                  const float* __restrict__ dist_g) {
  __shared__ PruneLds L;
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
  if (n > kPruneMaxL && !pre) {
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
    for (uint32_t i = tid; i < dim; i += kBlock) L.acc[na][i] = xv[i];
    __syncthreads();
    bool rej = false;
    for (uint32_t a = g; a < na; a += kBlock / 8) {   // 32 groups: two rounds once na > 32 (m up to 64)
      const float d = l2_group8(L.acc[a], L.acc[na], dim, k);
      rej |= __fmul_rn(d, alpha) < duv;
    }
    const bool any = __syncthreads_or(rej);
    if (!any) {
      if (tid == 0) L.acc_id[na] = v;
      ++na;
      if (na == m) break;
    } else {
      if (tid == 0 && nd < kPruneMaxL) L.disc[nd] = v;
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

// L2Dist(x_u, x_v) of every candidate v of vertex verts[b]'s list, in the
// reference's order (dist2u, build_graph.go:176-182), into dist_g[offs[u] + i]:
// the keys the host sorts for the presorted k_prune of hub vertices.
__global__ void __launch_bounds__(kBlock) k_cand_dist(const float* __restrict__ X, uint32_t dim,
                                                      const uint32_t* __restrict__ verts,
                                                      const uint64_t* __restrict__ offs,
                                                      const uint32_t* __restrict__ lens,
                                                      const uint32_t* __restrict__ ids, float* __restrict__ dist_g) {
  const uint64_t u = verts[blockIdx.x];
  const uint32_t g = threadIdx.x >> 3, k = threadIdx.x & 7, n = lens[u];
  const uint64_t off = offs[u];
  const float* xu = X + u * dim;
  for (uint32_t i = g; i < n; i += kBlock / 8) {
    const float d = l2_group8(xu, X + (uint64_t)ids[off + i] * dim, dim, k);
    if (k == 0) dist_g[off + i] = d;
  }
}

}  // namespace pm

namespace pmk {
static inline unsigned gcdiv(uint64_t a, uint64_t b) { return (unsigned)((a + b - 1) / b); }

uint32_t knn_pad_dim(uint32_t dim) { return dim <= 128 ? 128 : (dim <= 192 ? 192 : 0); }
uint32_t knn_top() { return kKnnTop; }
uint32_t prune_max_list() { return kPruneMaxL; }
uint32_t prune_max_dim() { return kPruneMaxD; }
uint32_t prune_max_m() { return kPruneMaxM; }

void to_bf16(hipStream_t st, const float* rows, uint64_t n, uint32_t dim, uint32_t dp, void* out, float* norms) {
  if (!n) return;
  hipLaunchKernelGGL(k_to_bf16, dim3(gcdiv(n, kBlock / 64)), dim3(kBlock), 0, st, rows, n, dim, dp, (__bf16*)out,
                     norms);
}
void knn_prefilter(hipStream_t st, const void* X, const float* xn, uint64_t N, const void* Q, const float* qn,
                   uint64_t M, uint32_t dp, uint32_t* out, uint32_t* out_hi) {
  if (!M) return;
  const dim3 grid(gcdiv(M, kKnnRows));
  if (dp == 128)
    hipLaunchKernelGGL(k_knn_bf16<128>, grid, dim3(kKnnThreads), 0, st, (const __bf16*)X, xn, N, (const __bf16*)Q,
                       qn, M, out, out_hi);
  else
    hipLaunchKernelGGL(k_knn_bf16<192>, grid, dim3(kKnnThreads), 0, st, (const __bf16*)X, xn, N, (const __bf16*)Q,
                       qn, M, out, out_hi);
}
void knn_rerank(hipStream_t st, const float* X, uint64_t N, uint32_t dim, const float* Q, uint64_t M,
                const uint32_t* cand, uint32_t K, bool self_base, uint32_t* out, float* dist, uint32_t* len) {
  if (!M) return;
  hipLaunchKernelGGL(k_knn_rerank, dim3(gcdiv(M, kBlock / 64)), dim3(kBlock), 0, st, X, N, dim, Q, M, cand, K,
                     (int)self_base, out, dist, len);
}
void to_bf16x2(hipStream_t st, const float* rows, uint64_t n, uint32_t dim, uint32_t dp, void* hi, void* lo,
               float* norms, uint32_t* maxnorm) {
  if (!n) return;
  hipLaunchKernelGGL(k_to_bf16x2, dim3(gcdiv(n, kBlock / 64)), dim3(kBlock), 0, st, rows, n, dim, dp, (__bf16*)hi,
                     (__bf16*)lo, norms, maxnorm);
}
void knn_prefilter_x3(hipStream_t st, const void* Xh, const void* Xl, const float* xn, uint64_t N, const void* Qh,
                      const void* Ql, const float* qn, uint64_t M, uint32_t dp, uint32_t* out, float* tau,
                      uint32_t* out_hi) {
  if (!M) return;
  const dim3 grid(gcdiv(M, kKnnRows));
  if (dp == 128)
    hipLaunchKernelGGL(k_knn_bf16x3<128>, grid, dim3(kKnn3Threads), 0, st, (const __bf16*)Xh, (const __bf16*)Xl, xn,
                       N, (const __bf16*)Qh, (const __bf16*)Ql, qn, M, out, tau, out_hi);
  else
    hipLaunchKernelGGL(k_knn_bf16x3<192>, grid, dim3(kKnn3Threads), 0, st, (const __bf16*)Xh, (const __bf16*)Xl, xn,
                       N, (const __bf16*)Qh, (const __bf16*)Ql, qn, M, out, tau, out_hi);
}
// the prefilter's 3 dp products summed with at most 2^-23
// relative error per add, doubled for whatever order and alignment the matrix
// core uses; 2^-16 (1 + 2^-6) for the lo residues and the lo.lo' term; 2^-17 for
// the norm sums, the final qn + xn - 2 acc and L2Dist's own rounding.
float knn_cert_rel(uint32_t dp) {
  return (float)(2.0 * (3.0 * dp + 8.0) * 0x1.0p-23 + 0x1.0p-16 * (1.0 + 0x1.0p-6) + 0x1.0p-17);
}
void knn_rerank_cert(hipStream_t st, const float* X, uint64_t N, uint32_t dim, const float* Q, uint64_t M,
                     const uint32_t* cand, uint32_t K, bool self_base, uint32_t* out, float* dist, uint32_t* len,
                     const float* qn, const float* tau, const uint32_t* maxnorm, uint32_t dp, uint64_t* list,
                     uint64_t* nlist, float* eps_out) {
  if (!M) return;
  hipLaunchKernelGGL(k_knn_rerank_cert, dim3(gcdiv(M, kBlock / 64)), dim3(kBlock), 0, st, X, N, dim, Q, M, cand, K,
                     (int)self_base, out, dist, len, qn, tau, maxnorm, knn_cert_rel(dp), list,
                     (unsigned long long*)nlist, eps_out);
}
void knn_brute(hipStream_t st, const float* X, uint64_t N, uint32_t dim, const float* Q, const uint64_t* list,
               uint64_t nlist, uint32_t K, bool self_base, uint32_t* out, float* dist, uint32_t* len) {
  if (!nlist) return;
  hipLaunchKernelGGL(k_knn_brute, dim3((unsigned)(nlist < (1u << 20) ? nlist : (1u << 20))), dim3(kBlock), 0, st, X, N, dim,
                     Q, list, nlist, K, (int)self_base, out, dist, len);
}
void prune(hipStream_t st, const float* X, uint32_t dim, const uint32_t* verts, uint64_t nverts,
           const uint64_t* offs, uint64_t stride, const uint32_t* lens, const uint32_t* ids, uint32_t m,
           float alpha, uint32_t* out, uint32_t* out_len, uint32_t* err, const uint32_t* sorted_pos,
           const float* dist_g) {
  if (!nverts) return;
  hipLaunchKernelGGL(k_prune, dim3((unsigned)nverts), dim3(kBlock), 0, st, X, dim, verts, nverts, offs, stride, lens,
                     ids, m, alpha, out, out_len, err, sorted_pos, dist_g);
}
void cand_dist(hipStream_t st, const float* X, uint32_t dim, const uint32_t* verts, uint64_t nverts,
               const uint64_t* offs, const uint32_t* lens, const uint32_t* ids, float* dist_g) {
  if (!nverts) return;
  hipLaunchKernelGGL(k_cand_dist, dim3((unsigned)nverts), dim3(kBlock), 0, st, X, dim, verts, offs, lens, ids, dist_g);
}
}  // namespace pmk

// pm_graph_k128.hip — the exact kNN with 128 prefilter keys per query row
// (pm_knn_k128, pm_build_graph_k128): k up to 128 and, in the
// build, m up to 64 (int(1.5 m) + self = 97 keys).  The kernels of pm_graph.hip
// and pm_graph_wide.hip keep 64 keys per row, one per lane of the merging wave;
// these keep 128, two per lane (pm_graph_dev.h: Key2, knn_insert128,
// wave_sort128):
//
//   k_knn128_bf16x3     k_knn_bf16x3 (dp 128 / 192) with top lists of 128
//   k_knn128_bf16x3_w   k_knn_bf16x3_w (dp 256 .. 1,024) with top lists of 128;
//                       K is walked in chunks of 32 so that the lists fit
//   k_knn128_rerank_cert  L2Dist of the 128 candidates, sort, the first K, the
//                       certificate against the 128th prefilter distance
//   k_knn128_brute      k_knn_brute / k_knn_brute_w with 128 keys per wave
//
// The MFMA sequence of a (query row, base row) pair is the 64-key kernels':
// every prefilter distance has their bits, so the eps of the certificate is
// theirs.  k_to_bf16x2, k_prune, k_prune_w and k_cand_dist are launched as they
// are.
#include <hip/hip_runtime.h>

#include "pm_internal.h"
#include "pm_graph_dev.h"

namespace pm {

constexpr int kK2Cols = 64;       // base rows per tile
constexpr int kK2Threads = 256;   // 4 waves: 2 row blocks x 2 column blocks of 32x32
constexpr int kK2Chunk = 32;      // wide: K extent held in LDS at a time
constexpr int kK2MaxDim = 1024;   // the widest row (knn_pad_dim_wide)

// The threshold / insert phase shared by both prefilters (k_knn_bf16x3's): the
// lane's 16 distances of base row col against its query rows; keys below the
// row's threshold go to the row's insertion buffer of tile t.
template <class Lds>
__device__ __forceinline__ void knn128_insert_tile(Lds& L, const f32x16& acc, const float (&qnr)[16],
                                                   const uint32_t (&thi)[16], float cn, uint64_t col, uint64_t t,
                                                   uint32_t rb, uint32_t h) {
  #pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t lr = rb + (i & 3) + 8 * (i >> 2) + 4 * h;
    float d = __fsub_rn(__fadd_rn(qnr[i], cn), __fmul_rn(2.0f, acc[i]));
    d = d < 0.0f ? 0.0f : d;
    const uint32_t db = __float_as_uint(d);
    if (db <= thi[i]) {
      const uint64_t key = ((uint64_t)db << 32) | (uint32_t)col;
      if (db < thi[i] || key < L.top[lr][kKnnTop2 - 1]) {
        const uint32_t slot = atomicAdd(&L.cnt[lr], 1u);
        L.buf[lr][slot] = key;
        L.any[t & 1] = 1;
      }
    }
  }
}

template <int DP>
struct Knn128Lds {
  uint64_t top[kKnnRows][kKnnTop2];         // sorted ascending per row
  uint64_t buf[kKnnRows][kK2Cols];          // this tile's keys below the row threshold
  uint32_t cnt[kKnnRows];
  uint32_t any[2];
  __bf16 bh[kK2Cols][DP + 8];               // padded rows: conflict-free 16-B fragment reads
  __bf16 bl[kK2Cols][DP + 8];
};
static_assert(sizeof(Knn128Lds<128>) == 133384 && sizeof(Knn128Lds<192>) == 149768, "LDS budget of DESIGN.md §10.3");
static_assert(sizeof(Knn128Lds<192>) <= 160 * 1024, "LDS of one CU");

// k_knn_bf16x3 (pm_graph.hip) with 128 keys per query row: per row the 128
// smallest (prefilter distance bits, id) keys over all base rows, sorted, tau =
// the prefilter distance of the 128th (NaN bits while fewer exist) and, when
// out_hi is given, the keys' distances.  Tile walk, MFMA order (lo.hi' and
// hi.lo' of every k-step, then the hi.hi' terms, one accumulator), insert,
// merge and cnt reset ordering are k_knn_bf16x3's; thi is read from entry 127.
template <int DP>
__global__ void __launch_bounds__(kK2Threads) k_knn128_bf16x3(const __bf16* __restrict__ Xh,
                                                              const __bf16* __restrict__ Xl,
                                                              const float* __restrict__ xn, uint64_t N,
                                                              const __bf16* __restrict__ Qh,
                                                              const __bf16* __restrict__ Ql,
                                                              const float* __restrict__ qn, uint64_t M,
                                                              uint32_t* __restrict__ out, float* __restrict__ tau,
                                                              uint32_t* __restrict__ out_hi) {
  constexpr int KS = DP / 16;
  constexpr int CH = kK2Cols * DP / 8;              // 16-B chunks per tile half
  constexpr int PER = CH / kK2Threads;
  constexpr int MR = kKnnRows / (kK2Threads / 64);  // rows each wave merges
  static_assert(CH % kK2Threads == 0, "tile chunks");
  __shared__ Knn128Lds<DP> L;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t rb = 32 * (w & 1), cb = 32 * (w >> 1);
  const uint32_t r32 = lane & 31, h = lane >> 5;
  const uint64_t row0 = (uint64_t)blockIdx.x * kKnnRows;

  for (uint32_t i = tid; i < kKnnRows * kKnnTop2; i += kK2Threads) (&L.top[0][0])[i] = kNoKey;
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
  const uint64_t T = (N + kK2Cols - 1) / kK2Cols;
  uint4 preh[PER], prel[PER];
  auto load_tile = [&](uint64_t t) {
    const uint64_t c0 = t * kK2Cols;
    #pragma unroll
    for (int p = 0; p < PER; ++p) {
      const uint32_t q = tid + p * kK2Threads;
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
      const uint32_t q = tid + p * kK2Threads;
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
    const uint64_t col = t * kK2Cols + cb + r32;
    if (col < N) knn128_insert_tile(L, acc, qnr, thi, xn[col], col, t, rb, h);
    if (tid == 0) L.any[(t + 1) & 1] = 0;
    __syncthreads();
    const bool merged = L.any[t & 1] != 0;   // uniform
    if (merged) {
      for (uint32_t r = w * MR; r < w * MR + MR; ++r) {
        const uint32_t n = L.cnt[r];
        if (n) knn_merge_row128(L.top[r], L.buf[r], n, lane);
      }
    }
    if (t + 1 < T) store_tile();
    __syncthreads();
    if (merged) {
      if (lane < MR) L.cnt[w * MR + lane] = 0;
      #pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint32_t lr = rb + (i & 3) + 8 * (i >> 2) + 4 * h;
        thi[i] = (uint32_t)(L.top[lr][kKnnTop2 - 1] >> 32);
      }
    }
    // cnt resets must land before the next tile's inserts
    if (merged) __syncthreads();
  }
  for (uint32_t r = w * MR; r < w * MR + MR; ++r) {
    const uint64_t qr = row0 + r;
    if (qr < M) {
      #pragma unroll
      for (uint32_t e = lane; e < kKnnTop2; e += 64) {
        out[qr * kKnnTop2 + e] = (uint32_t)L.top[r][e];
        if (out_hi) out_hi[qr * kKnnTop2 + e] = (uint32_t)(L.top[r][e] >> 32);
      }
      if (lane == 63) tau[qr] = __uint_as_float((uint32_t)(L.top[r][kKnnTop2 - 1] >> 32));
    }
  }
}

// k_knn_bf16x3_w's layout with top lists of 128 would take 172,296 B of the
// 160 KB; here a step is a K chunk of 32 (two k-steps), so the four
// double-buffered chunk pieces take 40 KB instead of 72 KB.  A padded chunk row
// is 80 B = 20 banks: 16 consecutive rows start on 16 distinct multiples of 4
// banks (5 r mod 16 is a bijection), so a 16-lane group of a 16-B fragment read
// covers the 64 banks once, as the 144-B rows of k_knn_bf16x3_w do.
struct Knn128WLds {
  uint64_t top[kKnnRows][kKnnTop2];         // sorted ascending per row
  uint64_t buf[kKnnRows][kK2Cols];          // this tile's keys below the row threshold
  uint32_t cnt[kKnnRows];
  uint32_t any[2];
  __bf16 qh[2][kKnnRows][kK2Chunk + 8];
  __bf16 ql[2][kKnnRows][kK2Chunk + 8];
  __bf16 bh[2][kK2Cols][kK2Chunk + 8];
  __bf16 bl[2][kK2Cols][kK2Chunk + 8];
};
static_assert(sizeof(Knn128WLds) == 139528, "LDS budget of DESIGN.md §10.3");

// The contract of k_knn128_bf16x3 for rows of dp bf16 values, dp a multiple of
// 64 (so of kK2Chunk).  q.x = lo.hi' + hi.lo' + hi.hi' per k-step of 16 in row
// order into one accumulator that lives across the row's dp / 32 chunks: the
// MFMA sequence of k_knn_bf16x3_w, whatever the chunk width.  Steps, prefetch
// and the one barrier per step are k_knn_bf16x3_w's.
__global__ void __launch_bounds__(kK2Threads) k_knn128_bf16x3_w(const __bf16* __restrict__ Xh,
                                                                const __bf16* __restrict__ Xl,
                                                                const float* __restrict__ xn, uint64_t N,
                                                                const __bf16* __restrict__ Qh,
                                                                const __bf16* __restrict__ Ql,
                                                                const float* __restrict__ qn, uint64_t M,
                                                                uint32_t dp, uint32_t* __restrict__ out,
                                                                float* __restrict__ tau,
                                                                uint32_t* __restrict__ out_hi) {
  constexpr int PER = kKnnRows * kK2Chunk / 8 / kK2Threads;   // 16-B pieces per thread and chunk half
  constexpr int MR = kKnnRows / (kK2Threads / 64);            // rows each wave merges
  static_assert(kKnnRows == kK2Cols && PER * kK2Threads * 8 == kKnnRows * kK2Chunk, "chunk pieces");
  __shared__ Knn128WLds L;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t rb = 32 * (w & 1), cb = 32 * (w >> 1);
  const uint32_t r32 = lane & 31, h = lane >> 5;
  const uint64_t row0 = (uint64_t)blockIdx.x * kKnnRows;

  for (uint32_t i = tid; i < kKnnRows * kKnnTop2; i += kK2Threads) (&L.top[0][0])[i] = kNoKey;
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
  const uint32_t NC = dp / kK2Chunk;                      // chunks per row
  const uint64_t T = (N + kK2Cols - 1) / kK2Cols;         // tiles
  const uint64_t S = T * NC;                              // steps
  uint4 pqh[PER], pql[PER], pbh[PER], pbl[PER];
  // step (t, c): chunk c of the query rows and of base tile t
  auto load_step = [&](uint64_t t, uint32_t c) {
    const uint64_t c0 = t * kK2Cols;
    #pragma unroll
    for (int p = 0; p < PER; ++p) {
      const uint32_t q = tid + p * kK2Threads;
      const uint32_t j = q / (kK2Chunk / 8);
      const uint64_t off = (uint64_t)c * kK2Chunk + (q % (kK2Chunk / 8)) * 8;
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
      const uint32_t q = tid + p * kK2Threads;
      const uint32_t j = q / (kK2Chunk / 8), off = (q % (kK2Chunk / 8)) * 8;
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
    for (int ks = 0; ks < kK2Chunk / 16; ++ks) {
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
    // the row is complete: the threshold / insert / merge phase of k_knn128_bf16x3
    const uint64_t col = t * kK2Cols + cb + r32;
    if (col < N) knn128_insert_tile(L, acc, qnr, thi, xn[col], col, t, rb, h);
    #pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    if (tid == 0) L.any[(t + 1) & 1] = 0;
    __syncthreads();
    const bool merged = L.any[t & 1] != 0;   // uniform
    if (merged) {
      for (uint32_t r = w * MR; r < w * MR + MR; ++r) {
        const uint32_t n = L.cnt[r];
        if (n) knn_merge_row128(L.top[r], L.buf[r], n, lane);
      }
    }
    if (more) store_step(b ^ 1);
    __syncthreads();
    if (merged) {
      if (lane < MR) L.cnt[w * MR + lane] = 0;
      #pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint32_t lr = rb + (i & 3) + 8 * (i >> 2) + 4 * h;
        thi[i] = (uint32_t)(L.top[lr][kKnnTop2 - 1] >> 32);
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
      #pragma unroll
      for (uint32_t e = lane; e < kKnnTop2; e += 64) {
        out[qr * kKnnTop2 + e] = (uint32_t)L.top[r][e];
        if (out_hi) out_hi[qr * kKnnTop2 + e] = (uint32_t)(L.top[r][e] >> 32);
      }
      if (lane == 63) tau[qr] = __uint_as_float((uint32_t)(L.top[r][kKnnTop2 - 1] >> 32));
    }
  }
}

// k_knn_rerank_cert (pm_graph.hip) for 128 candidates and K up to 128: one wave
// per query row.  The row's result is the brute-force one if N <= 128 (every
// base row is a candidate) or if the K-th re-ranked distance is < tau - eps,
// tau the 128th prefilter distance and eps as in k_knn_rerank_cert.
__global__ void __launch_bounds__(kBlock) k_knn128_rerank_cert(const float* __restrict__ X, uint64_t N, uint32_t dim,
                                                               const float* __restrict__ Q, uint64_t M,
                                                               const uint32_t* __restrict__ cand, uint32_t K,
                                                               int self_base, uint32_t* __restrict__ out,
                                                               float* __restrict__ dist_out,
                                                               uint32_t* __restrict__ len,
                                                               const float* __restrict__ qn,
                                                               const float* __restrict__ tau,
                                                               const uint32_t* __restrict__ maxnorm, float crel,
                                                               uint64_t* __restrict__ list,
                                                               unsigned long long* __restrict__ nlist,
                                                               float* __restrict__ eps_out) {
  __shared__ uint64_t keys[kBlock / 64][kKnnTop2];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t row = (uint64_t)blockIdx.x * (kBlock / 64) + w;
  if (row >= M) return;
  const Key2 t = knn_rerank_keys128(X, N, dim, Q + row * dim, cand + row * kKnnTop2, keys[w], lane);
  knn_emit128(t, row, K, self_base, lane, out, dist_out, len);
  if (N <= kKnnTop2) return;
  const uint32_t e = K - 1;   // the K-th key: entry e, in a of lane e or in b of lane e - 64
  if (lane == (e & 63)) {
    const uint64_t x = e < 64 ? t.a : t.b;
    const float dk = __uint_as_float((uint32_t)(x >> 32));
    const float sum = __fadd_rn(qn[row], __uint_as_float(*maxnorm));
    // rounded up: the factor covers the two roundings of the product and the sum
    const float eps = __fadd_rn(__fmul_rn(__fmul_rn(sum, crel), 1.0f + 0x1.0p-20f), kCertAbs);
    if (eps_out) eps_out[row] = eps;
    const bool ok = x != kNoKey && sum <= kCertMaxSum && (double)dk < (double)tau[row] - (double)eps;
    if (!ok) list[atomicAdd(nlist, 1ull)] = row;
  }
}

// k_knn_brute (MAXD 192) and k_knn_brute_w (MAXD 1,024) with 128 keys: one
// workgroup per listed query row streams all N base rows, L2Dist in the
// reference order by 8-lane groups (the query row in LDS); each wave keeps the
// sorted 128 smallest (dist, id) keys of its rows in registers, two per lane,
// with the 128th as threshold; wave 0 merges the four and writes the first K.
template <int MAXD>
struct Brute128Lds {
  uint64_t top[kBlock / 64][kKnnTop2];
  float q[MAXD];
};

template <int MAXD>
__global__ void __launch_bounds__(kBlock) k_knn128_brute(const float* __restrict__ X, uint64_t N, uint32_t dim,
                                                         const float* __restrict__ Q,
                                                         const uint64_t* __restrict__ list, uint64_t nlist,
                                                         uint32_t K, int self_base, uint32_t* __restrict__ out,
                                                         float* __restrict__ dist_out, uint32_t* __restrict__ len) {
  __shared__ Brute128Lds<MAXD> L;
  constexpr uint32_t W = kBlock / 64;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 3, k = lane & 7;
  for (uint64_t e = blockIdx.x; e < nlist; e += gridDim.x) {
    const uint64_t row = list[e];
    for (uint32_t i = tid; i < dim; i += kBlock) L.q[i] = Q[row * dim + i];
    __syncthreads();
    Key2 t = {kNoKey, kNoKey};
    for (uint64_t r0 = 8 * w; r0 < N; r0 += 8 * W) {   // uniform per wave: every lane stays active
      const uint64_t r = r0 + g;
      const bool ok = r < N;
      const float d = l2_group8(X + (ok ? r : 0) * dim, L.q, dim, k);
      const uint64_t key = ok ? (((uint64_t)__float_as_uint(d) << 32) | r) : kNoKey;
      uint64_t m = __ballot(k == 0 && key < readlane64(t.b, 63));
      while (m) {
        const int src = __builtin_ctzll(m);
        m &= m - 1;
        t = knn_insert128(t, readlane64(key, src), lane);
      }
    }
    L.top[w][lane] = t.a;
    L.top[w][64 + lane] = t.b;
    __syncthreads();
    if (w == 0) {
      for (uint32_t o = 1; o < W; ++o)
        for (uint32_t i = 0; i < kKnnTop2; ++i) t = knn_insert128(t, L.top[o][i], lane);
      knn_emit128(t, row, K, self_base, lane, out, dist_out, len);
    }
    __syncthreads();   // L.q and L.top are reused by the next listed row
  }
}

}  // namespace pm

namespace pmk {
static inline unsigned gcdiv(uint64_t a, uint64_t b) { return (unsigned)((a + b - 1) / b); }

uint32_t knn_top_k128() { return kKnnTop2; }

// dp: 128 or 192 (knn_pad_dim) or a multiple of 64 up to 1,024 (knn_pad_dim_wide)
void knn_prefilter_k128(hipStream_t st, const void* Xh, const void* Xl, const float* xn, uint64_t N, const void* Qh,
                        const void* Ql, const float* qn, uint64_t M, uint32_t dp, uint32_t* out, float* tau,
                        uint32_t* out_hi) {
  if (!M) return;
  const dim3 grid(gcdiv(M, kKnnRows));
  if (dp == 128)
    hipLaunchKernelGGL(k_knn128_bf16x3<128>, grid, dim3(kK2Threads), 0, st, (const __bf16*)Xh, (const __bf16*)Xl, xn,
                       N, (const __bf16*)Qh, (const __bf16*)Ql, qn, M, out, tau, out_hi);
  else if (dp == 192)
    hipLaunchKernelGGL(k_knn128_bf16x3<192>, grid, dim3(kK2Threads), 0, st, (const __bf16*)Xh, (const __bf16*)Xl, xn,
                       N, (const __bf16*)Qh, (const __bf16*)Ql, qn, M, out, tau, out_hi);
  else
    hipLaunchKernelGGL(k_knn128_bf16x3_w, grid, dim3(kK2Threads), 0, st, (const __bf16*)Xh, (const __bf16*)Xl, xn, N,
                       (const __bf16*)Qh, (const __bf16*)Ql, qn, M, dp, out, tau, out_hi);
}
void knn_rerank_cert_k128(hipStream_t st, const float* X, uint64_t N, uint32_t dim, const float* Q, uint64_t M,
                          const uint32_t* cand, uint32_t K, bool self_base, uint32_t* out, float* dist, uint32_t* len,
                          const float* qn, const float* tau, const uint32_t* maxnorm, uint32_t dp, uint64_t* list,
                          uint64_t* nlist, float* eps_out) {
  if (!M) return;
  hipLaunchKernelGGL(k_knn128_rerank_cert, dim3(gcdiv(M, kBlock / 64)), dim3(kBlock), 0, st, X, N, dim, Q, M, cand, K,
                     (int)self_base, out, dist, len, qn, tau, maxnorm, knn_cert_rel(dp), list,
                     (unsigned long long*)nlist, eps_out);
}
// dim <= 192: the query row of k_knn_brute; above: k_knn_brute_w's
void knn_brute_k128(hipStream_t st, const float* X, uint64_t N, uint32_t dim, const float* Q, const uint64_t* list,
                    uint64_t nlist, uint32_t K, bool self_base, uint32_t* out, float* dist, uint32_t* len) {
  if (!nlist) return;
  const dim3 grid((unsigned)(nlist < (1u << 20) ? nlist : (1u << 20)));
  if (dim <= 192)
    hipLaunchKernelGGL(k_knn128_brute<192>, grid, dim3(kBlock), 0, st, X, N, dim, Q, list, nlist, K, (int)self_base,
                       out, dist, len);
  else
    hipLaunchKernelGGL(k_knn128_brute<kK2MaxDim>, grid, dim3(kBlock), 0, st, X, N, dim, Q, list, nlist, K,
                       (int)self_base, out, dist, len);
}
}  // namespace pmk

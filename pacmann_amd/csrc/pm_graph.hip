// pm_graph.hip — graph construction and ground truth on the GPU (SURVEY.md
// §8f rank 1: the reference builds its degree-m graph with NGT candidates,
// robustPrune (alpha = 1.2), reverse-edge sampling and a random fill,
// graphann/build_graph.go:169-236,314-523; NGT is not in the image, so the
// candidates here are the exact k nearest neighbours).  Every float kernel of
// the family is here, each phase once; the lists, the tile epilogue and the
// brute-force stream they share are in pm_graph_dev.h.
//
//   k_to_bf16, k_to_bf16x2   rows -> padded bf16 rows (x2: hi = bf16(x), lo =
//                      bf16(x - hi)), f32 norms, x2 also the largest norm
//   k_knn_bf16<DP>     per query row the 64 smallest (bf16 distance, id) keys
//                      over all base rows: 128-column MFMA tiles, 512 threads
//   k_knn_bf16x3<DP, TOP>    the exact prefilter for padded rows of 128 / 192:
//                      q.x = hi.hi' + hi.lo' + lo.hi', 64-column tiles, the
//                      query fragments in registers, TOP (64 or 128) keys per
//                      row and the distance tau of the last one
//   k_knn_bf16x3_w<TOP, CHUNK>   the same for rows of 256 .. 1,024: K walked
//                      in chunks, query and base chunks double-buffered in LDS
//   k_knn_rerank, k_knn_rerank_cert<TOP>   the candidates re-ranked by the
//                      reference's own L2Dist (l2_distance_amd64.s order) and
//                      id: the first K, self dropped; cert: the row is exact if
//                      its K-th distance < tau - eps, other rows go to a list
//   k_knn_brute<TOP, MAXD>   the listed rows by brute force in L2Dist order
//   k_prune<ACC_IN_LDS>      robustPrune (build_graph.go:169-236) per vertex
//   k_cand_dist        the candidate distances of hub vertices' lists
//
// Integer-valued inputs up to 255 (SIFT bvecs semantics, loader.go:46-51) are
// exact in bf16 and every bf16 product/partial sum is an exact f32 integer, so
// k_knn_bf16's distances are exact and its top-64 holds the exact top-K.  For
// general float data it ranks by bf16-rounded distances and keeps 64 candidates
// for the re-rank of the top K (K <= 48 in the graph build).  The exact
// variants (pm_knn_exact, _wide, _k128) are exact for every
// finite float input.  pmk (below) picks the instantiation of every stage from
// (dp or dim, top); the narrow / wide boundary kKnnNarrowMax lives here alone.
#include <hip/hip_runtime.h>

#include "pm_internal.h"
#include "pm_graph_dev.h"

namespace pm {

constexpr int kKnnCols = 128;       // k_knn_bf16: base rows per tile
constexpr int kKnnThreads = 512;    // 8 waves: 2 row blocks x 4 column blocks of 32x32
constexpr int kKnn3Cols = 64;       // the exact prefilters: base rows per tile
constexpr int kKnn3Threads = 256;   // 4 waves: 2 row blocks x 2 column blocks of 32x32
constexpr int kKnnNarrowMax = 192;  // the widest row held whole in registers / LDS (knn_pad_dim)
constexpr int kKnnWMaxDim = 1024;   // the widest row at all (knn_pad_dim_wide)
constexpr int kKnnWPad = 64;        // wide rows are padded to a multiple of this

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

// ---- the prefilters.  All follow one plan: the lists of pm_graph_dev.h
// (knn_lists_init, knn_rows_init), a walk over the base tiles with tile t + 1
// travelling from global memory to registers during tile t's MFMAs and into LDS
// behind the merge, knn_tile_end after each tile, knn_lists_write at the end.
//
// Every operand row in LDS is padded by 8 bf16 (16 B).  A padded chunk row of
// CHUNK 32 is 80 B = 20 banks: 16 consecutive rows start on 16 distinct
// multiples of 4 banks (5 r mod 16 is a bijection), so a 16-lane group of a
// 16-B fragment read covers the 64 banks once.  The 144-B rows of CHUNK 64 do
// the same (36 banks, 9 r mod 16), and so do the whole rows of the narrow
// kernels.
//
// The fixed-count loops are unrolled by pragma: left alone, the compiler keeps
// some of them rolled at DP = 128 and indexes the register arrays through
// select chains (35,000 instructions).

template <int DP>
struct KnnLds : KnnLists<kKnnTop, kKnnCols> {
  __bf16 b[kKnnCols][DP + 8];
};

// Per query row the 64 smallest (bf16 distance bits, id) keys over all base
// rows: out [M][64], out_hi (nullable) their distance bits.
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
  knn_lists_init<kKnnThreads>(L, tid);

  // A fragments of this wave's 32 query rows (whole K), kept in registers
  bf16x8 a[KS];
  {
    const uint64_t qr = row0 + rb + r32;
    for (int s = 0; s < KS; ++s) {
      if (qr < M) a[s] = *(const bf16x8*)(Q + qr * DP + 16 * s + 8 * h);
      else for (int j = 0; j < 8; ++j) a[s][j] = (__bf16)0.0f;
    }
  }
  float qnr[16];
  uint32_t thi[16];
  knn_rows_init(qn, row0, M, rb, h, qnr, thi);
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
  uint32_t par = 0;   // t & 1, carried by knn_tile_end
  for (uint64_t t = 0; t < T; ++t) {
    if (t + 1 < T) load_tile(t + 1);   // in flight during the MFMAs
    f32x16 acc = {};
    for (int s = 0; s < KS; ++s) {
      const bf16x8 bb = *(const bf16x8*)&L.b[cb + r32][16 * s + 8 * h];
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], bb, acc, 0, 0, 0);
    }
    const uint64_t col = t * kKnnCols + cb + r32;
    knn_tile_end<kKnnThreads>(
        L, par, col, N, xn, rb, h, thi, [=](int i, float cn) { return knn_dist_bits(qnr[i], cn, acc[i]); },
        [&] { if (t + 1 < T) store_tile(); });
  }
  knn_lists_write<kKnnThreads>(L, row0, M, out, out_hi, nullptr);
}

// The split form of k_knn_bf16 (pm_knn_exact, pm_knn_k128): rows are hi + lo
// (k_to_bf16x2) and q.x is hi.hi' + hi.lo' + lo.hi', three MFMAs per k-step
// into one accumulator, the two small terms of every k-step before the hi.hi'
// terms: the order the certificate's eps is proved for (knn_cert_rel, DESIGN.md
// §10.1).  Both halves of a base tile lie in LDS, so the tile is 64 columns
// wide and the workgroup has 4 waves; each wave keeps both halves of its 32
// query rows in registers.  Besides the TOP candidate ids a row gets tau, the
// prefilter distance of its last key: every base row outside the candidates
// has a prefilter distance >= tau.
template <int DP, int TOP>
struct Knn3Lds : KnnLists<TOP, kKnn3Cols> {
  __bf16 bh[kKnn3Cols][DP + 8];
  __bf16 bl[kKnn3Cols][DP + 8];
};
static_assert(sizeof(Knn3Lds<128, 64>) == 100616 && sizeof(Knn3Lds<192, 64>) == 117000, "LDS budget of DESIGN.md §10.1");
static_assert(sizeof(Knn3Lds<128, 128>) == 133384 && sizeof(Knn3Lds<192, 128>) == 149768,
              "LDS budget of DESIGN.md §10.3");
static_assert(sizeof(Knn3Lds<192, 128>) <= 160 * 1024, "LDS of one CU");

template <int DP, int TOP>
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
  static_assert(CH % kKnn3Threads == 0, "tile chunks");
  __shared__ Knn3Lds<DP, TOP> L;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t rb = 32 * (w & 1), cb = 32 * (w >> 1);
  const uint32_t r32 = lane & 31, h = lane >> 5;
  const uint64_t row0 = (uint64_t)blockIdx.x * kKnnRows;
  knn_lists_init<kKnn3Threads>(L, tid);

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
  knn_rows_init(qn, row0, M, rb, h, qnr, thi);
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
  uint32_t par = 0;   // t & 1, carried by knn_tile_end
  for (uint64_t t = 0; t < T; ++t) {
    if (t + 1 < T) load_tile(t + 1);   // in flight during the MFMAs
    f32x16 acc = {};
    bf16x8 bh[KS];   // read once, used by both loops
    #pragma unroll
    for (int s = 0; s < KS; ++s) {
      bh[s] = *(const bf16x8*)&L.bh[cb + r32][16 * s + 8 * h];
      const bf16x8 bl = *(const bf16x8*)&L.bl[cb + r32][16 * s + 8 * h];
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[s], bh[s], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s], bl, acc, 0, 0, 0);
    }
    #pragma unroll
    for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s], bh[s], acc, 0, 0, 0);
    const uint64_t col = t * kKnn3Cols + cb + r32;
    knn_tile_end<kKnn3Threads>(
        L, par, col, N, xn, rb, h, thi, [=](int i, float cn) { return knn_dist_bits(qnr[i], cn, acc[i]); },
        [&] { if (t + 1 < T) store_tile(); });
  }
  knn_lists_write<kKnn3Threads>(L, row0, M, out, out_hi, tau);
}

// The contract of k_knn_bf16x3 for rows of dp bf16 values, dp a multiple of
// kKnnWPad (so of CHUNK).  q.x = lo.hi' + hi.lo' + hi.hi' per k-step of 16 in
// row order into one accumulator that lives across the row's dp / CHUNK
// chunks: the MFMA sequence does not depend on the chunk width.  A step is one
// chunk of one tile; step s + 1's four chunk pieces travel from global memory
// to registers during step s's MFMAs and into the other LDS buffer behind them,
// so one barrier per step orders both buffers.  The query chunks are read again
// for every tile (they stay in L2); nothing is held for a whole row.  With 64
// keys per row the chunk is 64 wide; with 128 that would take 172,296 B of the
// 160 KB, so the chunk is 32 (two k-steps) and the four double-buffered pieces
// take 40 KB instead of 72 KB.
template <int TOP, int CHUNK>
struct KnnWLds : KnnLists<TOP, kKnn3Cols> {
  __bf16 qh[2][kKnnRows][CHUNK + 8];
  __bf16 ql[2][kKnnRows][CHUNK + 8];
  __bf16 bh[2][kKnn3Cols][CHUNK + 8];
  __bf16 bl[2][kKnn3Cols][CHUNK + 8];
};
static_assert(sizeof(KnnWLds<64, 64>) == 139528, "LDS budget of DESIGN.md §10.2");
static_assert(sizeof(KnnWLds<128, 32>) == 139528, "LDS budget of DESIGN.md §10.3");
static_assert(sizeof(KnnWLds<64, 64>) <= 160 * 1024, "LDS of one CU");

template <int TOP, int CHUNK>
__global__ void __launch_bounds__(kKnn3Threads) k_knn_bf16x3_w(const __bf16* __restrict__ Xh,
                                                               const __bf16* __restrict__ Xl,
                                                               const float* __restrict__ xn, uint64_t N,
                                                               const __bf16* __restrict__ Qh,
                                                               const __bf16* __restrict__ Ql,
                                                               const float* __restrict__ qn, uint64_t M, uint32_t dp,
                                                               uint32_t* __restrict__ out, float* __restrict__ tau,
                                                               uint32_t* __restrict__ out_hi) {
  constexpr int PER = kKnnRows * CHUNK / 8 / kKnn3Threads;   // 16-B pieces per thread and chunk half
  static_assert(kKnnRows == kKnn3Cols && PER * kKnn3Threads * 8 == kKnnRows * CHUNK, "chunk pieces");
  static_assert(kKnnWPad % CHUNK == 0, "a padded row is whole chunks");
  __shared__ KnnWLds<TOP, CHUNK> L;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t rb = 32 * (w & 1), cb = 32 * (w >> 1);
  const uint32_t r32 = lane & 31, h = lane >> 5;
  const uint64_t row0 = (uint64_t)blockIdx.x * kKnnRows;
  knn_lists_init<kKnn3Threads>(L, tid);

  float qnr[16];
  uint32_t thi[16];
  knn_rows_init(qn, row0, M, rb, h, qnr, thi);
  const uint32_t NC = dp / CHUNK;                           // chunks per row
  const uint64_t T = (N + kKnn3Cols - 1) / kKnn3Cols;       // tiles
  const uint64_t S = T * NC;                                // steps
  uint4 pqh[PER], pql[PER], pbh[PER], pbl[PER];
  // step (t, c): chunk c of the query rows and of base tile t
  auto load_step = [&](uint64_t t, uint32_t c) {
    const uint64_t c0 = t * kKnn3Cols;
    #pragma unroll
    for (int p = 0; p < PER; ++p) {
      const uint32_t q = tid + p * kKnn3Threads;
      const uint32_t j = q / (CHUNK / 8);
      const uint64_t off = (uint64_t)c * CHUNK + (q % (CHUNK / 8)) * 8;
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
      const uint32_t q = tid + p * kKnn3Threads;
      const uint32_t j = q / (CHUNK / 8), off = (q % (CHUNK / 8)) * 8;
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
  uint32_t c = 0, par = 0;   // par: t & 1, carried by knn_tile_end
  for (uint64_t s = 0; s < S; ++s) {
    const uint32_t b = (uint32_t)(s & 1);
    const bool more = s + 1 < S;
    const bool last = c + 1 == NC;          // the tile's last chunk
    if (more) load_step(last ? t + 1 : t, last ? 0 : c + 1);   // in flight during the MFMAs
    #pragma unroll
    for (int ks = 0; ks < CHUNK / 16; ++ks) {
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
    // the row is complete
    const uint64_t col = t * kKnn3Cols + cb + r32;
    knn_tile_end<kKnn3Threads>(
        L, par, col, N, xn, rb, h, thi, [=](int i, float cn) { return knn_dist_bits(qnr[i], cn, acc[i]); },
        [&] { if (more) store_step(b ^ 1); });
    #pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    ++t;
    c = 0;
  }
  knn_lists_write<kKnn3Threads>(L, row0, M, out, out_hi, tau);
}

// ---- the re-rank: one wave per query row, exact L2Dist of the TOP candidates,
// keys (dist, id) sorted; the first K (self dropped when self_base) go to
// out[row][K], their count to len[row].  Returns the sorted keys.
template <int TOP>
__device__ __forceinline__ TopKeys<TOP> knn_rerank_row(const float* __restrict__ X, uint64_t N, uint32_t dim,
                                                       const float* __restrict__ Q, uint64_t row,
                                                       const uint32_t* __restrict__ cand, uint32_t K, int self_base,
                                                       uint64_t* keys, uint32_t lane, uint32_t* __restrict__ out,
                                                       float* __restrict__ dist_out, uint32_t* __restrict__ len) {
  const TopKeys<TOP> t = TopKeys<TOP>::rerank_keys(X, N, dim, Q + row * dim, cand + row * TOP, keys, lane);
  t.emit(row, K, self_base, lane, out, dist_out, len);
  return t;
}

__global__ void __launch_bounds__(kBlock) k_knn_rerank(const float* __restrict__ X, uint64_t N, uint32_t dim,
                                                       const float* __restrict__ Q, uint64_t M,
                                                       const uint32_t* __restrict__ cand, uint32_t K,
                                                       int self_base, uint32_t* __restrict__ out,
                                                       float* __restrict__ dist_out, uint32_t* __restrict__ len) {
  __shared__ uint64_t keys[kBlock / 64][kKnnTop];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t row = (uint64_t)blockIdx.x * (kBlock / 64) + w;
  if (row >= M) return;
  knn_rerank_row<kKnnTop>(X, N, dim, Q, row, cand, K, self_base, keys[w], lane, out, dist_out, len);
}

// k_knn_rerank with the certificate of pm_knn_exact.  The row's result is the
// brute-force one if N <= TOP (every base row is a candidate) or if the K-th
// re-ranked distance is < tau - eps: a base row outside the candidates has a
// prefilter distance >= tau, so an L2Dist >= tau - eps, strictly above all K
// kept keys.  A NaN or an infinity anywhere fails the comparison.  Uncertified
// rows are appended to list (their count in nlist) for k_knn_brute.
template <int TOP>
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
  __shared__ uint64_t keys[kBlock / 64][TOP];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t row = (uint64_t)blockIdx.x * (kBlock / 64) + w;
  if (row >= M) return;
  const TopKeys<TOP> t = knn_rerank_row<TOP>(X, N, dim, Q, row, cand, K, self_base, keys[w], lane, out, dist_out, len);
  if (N <= TOP) return;
  const uint32_t e = K - 1;   // the K-th key
  if (lane == (e & 63)) {
    const uint64_t x = t.at(e);
    const float dk = __uint_as_float((uint32_t)(x >> 32));
    const float sum = __fadd_rn(qn[row], __uint_as_float(*maxnorm));
    // rounded up: the factor covers the two roundings of the product and the sum
    const float eps = __fadd_rn(__fmul_rn(__fmul_rn(sum, crel), 1.0f + 0x1.0p-20f), kCertAbs);
    if (eps_out) eps_out[row] = eps;
    const bool ok = x != kNoKey && sum <= kCertMaxSum && (double)dk < (double)tau[row] - (double)eps;
    if (!ok) list[atomicAdd(nlist, 1ull)] = row;
  }
}

// The exact fallback of pm_knn_exact: one workgroup per listed query row ranks
// all N base rows (knn_brute_stream; the query row of up to MAXD floats in LDS)
// and writes the first K as k_knn_rerank does.
template <int TOP, int MAXD>
__global__ void __launch_bounds__(kBlock) k_knn_brute(const float* __restrict__ X, uint64_t N, uint32_t dim,
                                                      const float* __restrict__ Q,
                                                      const uint64_t* __restrict__ list, uint64_t nlist, uint32_t K,
                                                      int self_base, uint32_t* __restrict__ out,
                                                      float* __restrict__ dist_out, uint32_t* __restrict__ len) {
  __shared__ BruteLds<TOP, MAXD> L;
  for (uint64_t e = blockIdx.x; e < nlist; e += gridDim.x) {
    const uint64_t row = list[e];
    const TopKeys<TOP> t = knn_brute_stream(L, X, dim, Q + row * dim, 0, N, nullptr);
    if (threadIdx.x < 64) t.emit(row, K, self_base, threadIdx.x, out, dist_out, len);
    __syncthreads();   // L is reused by the next listed row
  }
}

constexpr int kPruneMaxL = 4096;   // candidates per vertex held in LDS
constexpr int kPruneMaxM = 64;
constexpr int kPruneMaxD = 256;    // the widest row of the ACC_IN_LDS form

// ACC_IN_LDS: the accepted vectors lie in LDS, row na being the candidate under
// test (rows up to kPruneMaxD).  Otherwise (rows up to kKnnWMaxDim) only the
// candidate lies there, in row 0; the accepted rows (at most m, read again for
// every candidate, so cache-hot) come from X by acc_id through the same
// l2_group8, whose operand order and sums do not depend on where the rows lie:
// both forms give the same bits.
template <bool ACC_IN_LDS>
struct PruneLds {
  uint64_t key[kPruneMaxL];        // (L2Dist to u, position): stable order
  float dist[kPruneMaxL];          // by position
  uint32_t disc[kPruneMaxL];       // discarded ids in order
  float row[ACC_IN_LDS ? kPruneMaxM + 1 : 1][ACC_IN_LDS ? kPruneMaxD + 8 : kKnnWMaxDim];
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
template <bool ACC_IN_LDS>
__global__ void __launch_bounds__(kBlock) k_prune(const float* __restrict__ X, uint32_t dim,
                                                  const uint32_t* __restrict__ verts, uint64_t nverts,
                                                  const uint64_t* __restrict__ offs, uint64_t stride,
                                                  const uint32_t* __restrict__ lens,
                                                  const uint32_t* __restrict__ ids, uint32_t m, float alpha,
                                                  uint32_t* __restrict__ out, uint32_t* __restrict__ out_len,
                                                  uint32_t* __restrict__ err,
                                                  const uint32_t* __restrict__ sorted_pos,
                                                  const float* __restrict__ dist_g) {
  __shared__ PruneLds<ACC_IN_LDS> L;
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
    float* cand = L.row[ACC_IN_LDS ? na : 0];
    for (uint32_t i = tid; i < dim; i += kBlock) cand[i] = xv[i];
    __syncthreads();   // also: acc_id[na - 1] of the accept before
    bool rej = false;
    for (uint32_t a = g; a < na; a += kBlock / 8) {   // 32 groups: two rounds once na > 32 (m up to 64)
      float d;
      if constexpr (ACC_IN_LDS) d = l2_group8(L.row[a], cand, dim, k);
      else d = l2_group8(X + (uint64_t)L.acc_id[a] * dim, cand, dim, k);
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

uint32_t knn_pad_dim(uint32_t dim) { return dim <= 128 ? 128 : (dim <= (uint32_t)kKnnNarrowMax ? kKnnNarrowMax : 0); }
uint32_t knn_pad_dim_wide(uint32_t dim) {
  return dim == 0 || dim > (uint32_t)kKnnWMaxDim ? 0 : (dim + kKnnWPad - 1) / kKnnWPad * kKnnWPad;
}
bool knn_wide(uint32_t width) { return width > (uint32_t)kKnnNarrowMax; }
uint32_t knn_top() { return kKnnTop; }
uint32_t knn_top_k128() { return kKnnTop2; }
uint32_t prune_max_list() { return kPruneMaxL; }
uint32_t prune_max_dim() { return kPruneMaxD; }
uint32_t prune_max_m() { return kPruneMaxM; }

void to_bf16(hipStream_t st, const float* rows, uint64_t n, uint32_t dim, uint32_t dp, void* out, float* norms) {
  if (!n) return;
  hipLaunchKernelGGL(k_to_bf16, dim3(gcdiv(n, kBlock / 64)), dim3(kBlock), 0, st, rows, n, dim, dp, (__bf16*)out,
                     norms);
}
void to_bf16x2(hipStream_t st, const float* rows, uint64_t n, uint32_t dim, uint32_t dp, void* hi, void* lo,
               float* norms, uint32_t* maxnorm) {
  if (!n) return;
  hipLaunchKernelGGL(k_to_bf16x2, dim3(gcdiv(n, kBlock / 64)), dim3(kBlock), 0, st, rows, n, dim, dp, (__bf16*)hi,
                     (__bf16*)lo, norms, maxnorm);
}
void knn_prefilter(hipStream_t st, const void* X, const float* xn, uint64_t N, const void* Q, const float* qn,
                   uint64_t M, uint32_t dp, uint32_t* out, uint32_t* out_hi) {
  if (!M) return;
  const auto k = dp == 128 ? k_knn_bf16<128> : k_knn_bf16<192>;
  hipLaunchKernelGGL(k, dim3(gcdiv(M, kKnnRows)), dim3(kKnnThreads), 0, st, (const __bf16*)X, xn, N, (const __bf16*)Q,
                     qn, M, out, out_hi);
}
void knn_rerank(hipStream_t st, const float* X, uint64_t N, uint32_t dim, const float* Q, uint64_t M,
                const uint32_t* cand, uint32_t K, bool self_base, uint32_t* out, float* dist, uint32_t* len) {
  if (!M) return;
  hipLaunchKernelGGL(k_knn_rerank, dim3(gcdiv(M, kBlock / 64)), dim3(kBlock), 0, st, X, N, dim, Q, M, cand, K,
                     (int)self_base, out, dist, len);
}

template <int TOP>
static void prefilter_x3(hipStream_t st, const __bf16* Xh, const __bf16* Xl, const float* xn, uint64_t N,
                         const __bf16* Qh, const __bf16* Ql, const float* qn, uint64_t M, uint32_t dp, uint32_t* out,
                         float* tau, uint32_t* out_hi) {
  const dim3 grid(gcdiv(M, kKnnRows)), block(kKnn3Threads);
  if (knn_wide(dp))
    hipLaunchKernelGGL((k_knn_bf16x3_w<TOP, TOP == kKnnTop ? 64 : 32>), grid, block, 0, st, Xh, Xl, xn, N, Qh, Ql, qn,
                       M, dp, out, tau, out_hi);
  else
    hipLaunchKernelGGL((dp == 128 ? k_knn_bf16x3<128, TOP> : k_knn_bf16x3<192, TOP>), grid, block, 0, st, Xh, Xl, xn,
                       N, Qh, Ql, qn, M, out, tau, out_hi);
}
void knn_prefilter_x3(hipStream_t st, const void* Xh, const void* Xl, const float* xn, uint64_t N, const void* Qh,
                      const void* Ql, const float* qn, uint64_t M, uint32_t dp, uint32_t top, uint32_t* out,
                      float* tau, uint32_t* out_hi) {
  if (!M) return;
  (top == kKnnTop2 ? prefilter_x3<kKnnTop2> : prefilter_x3<kKnnTop>)(
      st, (const __bf16*)Xh, (const __bf16*)Xl, xn, N, (const __bf16*)Qh, (const __bf16*)Ql, qn, M, dp, out, tau,
      out_hi);
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
                     const float* qn, const float* tau, const uint32_t* maxnorm, uint32_t dp, uint32_t top,
                     uint64_t* list, uint64_t* nlist, float* eps_out) {
  if (!M) return;
  hipLaunchKernelGGL((top == kKnnTop2 ? k_knn_rerank_cert<kKnnTop2> : k_knn_rerank_cert<kKnnTop>),
                     dim3(gcdiv(M, kBlock / 64)), dim3(kBlock), 0, st, X, N, dim, Q, M, cand, K, (int)self_base, out,
                     dist, len, qn, tau, maxnorm, knn_cert_rel(dp), list, (unsigned long long*)nlist, eps_out);
}
void knn_brute(hipStream_t st, const float* X, uint64_t N, uint32_t dim, uint32_t top, const float* Q,
               const uint64_t* list, uint64_t nlist, uint32_t K, bool self_base, uint32_t* out, float* dist,
               uint32_t* len) {
  if (!nlist) return;
  const bool wide = knn_wide(dim);
  const auto k = top == kKnnTop2
                     ? (wide ? k_knn_brute<kKnnTop2, kKnnWMaxDim> : k_knn_brute<kKnnTop2, kKnnNarrowMax>)
                     : (wide ? k_knn_brute<kKnnTop, kKnnWMaxDim> : k_knn_brute<kKnnTop, kKnnNarrowMax>);
  hipLaunchKernelGGL(k, dim3(gclamp(nlist)), dim3(kBlock), 0, st, X, N, dim, Q, list, nlist, K, (int)self_base, out,
                     dist, len);
}
void prune(hipStream_t st, const float* X, uint32_t dim, bool wide, const uint32_t* verts, uint64_t nverts,
           const uint64_t* offs, uint64_t stride, const uint32_t* lens, const uint32_t* ids, uint32_t m,
           float alpha, uint32_t* out, uint32_t* out_len, uint32_t* err, const uint32_t* sorted_pos,
           const float* dist_g) {
  if (!nverts) return;
  hipLaunchKernelGGL((wide && knn_wide(dim) ? k_prune<false> : k_prune<true>), dim3((unsigned)nverts), dim3(kBlock), 0,
                     st, X, dim, verts, nverts, offs, stride, lens, ids, m, alpha, out, out_len, err, sorted_pos,
                     dist_g);
}
void cand_dist(hipStream_t st, const float* X, uint32_t dim, const uint32_t* verts, uint64_t nverts,
               const uint64_t* offs, const uint32_t* lens, const uint32_t* ids, float* dist_g) {
  if (!nverts) return;
  hipLaunchKernelGGL(k_cand_dist, dim3((unsigned)nverts), dim3(kBlock), 0, st, X, dim, verts, offs, lens, ids, dist_g);
}
}  // namespace pmk

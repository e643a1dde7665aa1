// pm_graph_dev.h — the device code shared by the exact kNN / robustPrune
// kernels of pm_graph.hip, pm_graph_u8.hip and pm_cluster.hip, each piece once:
//
//   TopKeys<TOP>       a wave's sorted list of TOP (distance bits, id) keys
//   l2_group8          the 8-lane L2Dist in the reference's order
//   KnnLists and the   the per-row top lists of a prefilter workgroup: init,
//   knn_* phases       per-lane set-up, the tile epilogue, the write-out
//   knn_brute_stream   one query against a row range, four waves
//   the certificate's constants
//
// Include from HIP translation units only, after pm_internal.h.
#pragma once
#include <hip/hip_runtime.h>

#include "pm_internal.h"

namespace pm {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kKnnRows = 64;      // query rows per workgroup
constexpr int kKnnTop = 64;       // prefilter keys kept per query row
constexpr int kKnnTop2 = 128;     // ... by the _k128 and u8 entry points
constexpr uint64_t kNoKey = ~0ull;

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) {
  const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
  return ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(v >> 32), l) << 32) |
         __builtin_amdgcn_readlane((uint32_t)v, l);
}

// 8-lane L2Dist of a (global f32) and b (global f32) in the reference order;
// every lane of the group returns the distance.
__device__ __forceinline__ float l2_group8(const float* __restrict__ a, const float* __restrict__ b, uint32_t dim,
                                           uint32_t k) {
  const uint32_t dimS = dim & ~7u;
  float acc = 0.0f;
  for (uint32_t t = k; t < dimS; t += 8) {
    const float d = __fsub_rn(a[t], b[t]);
    acc = __fadd_rn(acc, __fmul_rn(d, d));
  }
  acc = __fadd_rn(acc, __shfl_xor(acc, 1));
  acc = __fadd_rn(acc, __shfl_xor(acc, 2));
  acc = __fadd_rn(acc, __shfl_xor(acc, 4));
  float d = dimS ? acc : 0.0f;
  for (uint32_t i = dimS; i < dim; ++i) {   // build_graph.go:122-125 scalar tail
    const float t = __fsub_rn(a[i], b[i]);
    d = __fadd_rn(d, __fmul_rn(t, t));
  }
  return d;
}

// A wave's sorted list of TOP u64 keys, ascending: entry 64 i + lane lives in
// v[i] of that lane, so every part v[i] is ascending by lane and the list is
// v[0], v[1], ...  Every loop over the parts has a fixed count and is unrolled:
// v stays in registers.
template <int TOP>
struct TopKeys {
  static_assert(TOP >= 64 && TOP % 64 == 0, "whole parts of 64 keys");
  static constexpr int H = TOP / 64;
  uint64_t v[H];

  static __device__ __forceinline__ TopKeys empty() {
    TopKeys t;
    #pragma unroll
    for (int i = 0; i < H; ++i) t.v[i] = kNoKey;
    return t;
  }
  // a row of TOP keys in LDS
  static __device__ __forceinline__ TopKeys load(const uint64_t* row, uint32_t lane) {
    TopKeys t;
    #pragma unroll
    for (int i = 0; i < H; ++i) t.v[i] = row[64 * i + lane];
    return t;
  }
  __device__ __forceinline__ void store(uint64_t* row, uint32_t lane) const {
    #pragma unroll
    for (int i = 0; i < H; ++i) row[64 * i + lane] = v[i];
  }
  // entry TOP - 1 (wave-uniform): the threshold of the list
  __device__ __forceinline__ uint64_t last() const { return readlane64(v[H - 1], 63); }
  // entry e, valid in lane e & 63
  __device__ __forceinline__ uint64_t at(uint32_t e) const {
    uint64_t x = v[0];
    #pragma unroll
    for (int i = 1; i < H; ++i) x = e >= 64u * i ? v[i] : x;
    return x;
  }

  // Insert the wave-uniform key x.  The parts are sorted, so the keys below x
  // are a prefix of the list and pos is x's entry; every branch is uniform.
  __device__ __forceinline__ void insert(uint64_t x, uint32_t lane) {
    if (x >= last()) return;
    uint32_t pos = 0;
    #pragma unroll
    for (int i = 0; i < H; ++i) pos += __popcll(__ballot(v[i] < x));
    uint64_t up[H];   // the list shifted up by one entry
    #pragma unroll
    for (int i = 0; i < H; ++i) {
      up[i] = shfl_up64(v[i], 1);
      if (i) up[i] = lane == 0 ? readlane64(v[i - 1], 63) : up[i];
    }
    if constexpr (H == 2) {   // the generic chain below, written as one two-way branch
      if (pos < 64) {
        v[0] = lane < pos ? v[0] : (lane == pos ? x : up[0]);
        v[1] = up[1];
      } else {
        const uint32_t p = pos - 64;
        v[1] = lane < p ? v[1] : (lane == p ? x : up[1]);
      }
    } else {
      #pragma unroll
      for (int i = 0; i < H; ++i) {
        const uint32_t p = pos - 64u * i;
        if (i + 1 < H && pos >= 64u * (i + 1)) continue;   // x lands in a later part
        if (i && pos < 64u * i) v[i] = up[i];
        else v[i] = lane < p ? v[i] : (lane == p ? x : up[i]);
      }
    }
  }
  // Merge n keys of an insertion buffer into the sorted LDS row top.
  static __device__ __forceinline__ void merge_row(uint64_t* top, const uint64_t* buf, uint32_t n, uint32_t lane) {
    TopKeys t = load(top, lane);
    for (uint32_t e = 0; e < n; ++e) t.insert(buf[e], lane);
    t.store(top, lane);
  }

  // Bitonic sort of the TOP keys, ascending by entry: partners less than 64
  // entries apart meet by a lane exchange, the others within the lane.
  __device__ __forceinline__ void sort(uint32_t lane) {
    for (int k = 2; k <= 64; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) sort_lanes(k, j, lane);
    #pragma unroll
    for (int k = 128; k <= TOP; k <<= 1) {   // the part indices are constants: v is never indexed by a variable
      #pragma unroll
      for (int j = k >> 1; j >= 64; j >>= 1) {
        #pragma unroll
        for (int i = 0; i < H; ++i) {
          const int o = i ^ (j >> 6);
          if (o < i) continue;
          const bool up = ((64 * i) & k) == 0;
          const uint64_t mn = v[i] < v[o] ? v[i] : v[o], mx = v[i] < v[o] ? v[o] : v[i];
          v[i] = up ? mn : mx;
          v[o] = up ? mx : mn;
        }
      }
      for (int j = 32; j > 0; j >>= 1) sort_lanes(k, j, lane);
    }
  }
  // one compare-exchange step of the network at distance j < 64: entry idx
  // against entry idx ^ j in lane ^ j
  __device__ __forceinline__ void sort_lanes(int k, int j, uint32_t lane) {
    #pragma unroll
    for (int i = 0; i < H; ++i) {
      const uint32_t idx = 64 * i + lane;
      const uint64_t x = v[i];
      const uint32_t lo = __shfl_xor((uint32_t)x, j), hi = __shfl_xor((uint32_t)(x >> 32), j);
      const uint64_t y = ((uint64_t)hi << 32) | lo;
      const bool up = (idx & k) == 0, lower = (idx & j) == 0;
      const uint64_t mn = x < y ? x : y, mx = x < y ? y : x;
      v[i] = (up == lower) ? mn : mx;
    }
  }

  // One wave's re-rank of a query row: exact L2Dist of the TOP candidates in
  // TOP / 8 rounds of eight, keys (dist, id) in the wave's LDS row, sorted.
  static __device__ __forceinline__ TopKeys rerank_keys(const float* __restrict__ X, uint64_t N, uint32_t dim,
                                                        const float* __restrict__ q,
                                                        const uint32_t* __restrict__ cand, uint64_t* keys,
                                                        uint32_t lane) {
    const uint32_t g = lane >> 3, k = lane & 7;
    for (uint32_t r = 0; r < TOP / 8; ++r) {
      const uint32_t c = r * 8 + g;
      const uint32_t id = cand[c];
      const bool ok = id < N;
      const float d = l2_group8(X + (ok ? (uint64_t)id : 0) * dim, q, dim, k);
      if (k == 0) keys[c] = ok ? (((uint64_t)__float_as_uint(d) << 32) | id) : kNoKey;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // this wave's LDS keys visible to its lanes
    __builtin_amdgcn_wave_barrier();
    TopKeys t = load(keys, lane);
    t.sort(lane);
    return t;
  }

  // The first K of the sorted keys (self dropped when self_base: the reference
  // removes u from NGT's K results) go to out[row][K], their distances to
  // dist_out when given, their count to len[row].
  __device__ __forceinline__ void emit(uint64_t row, uint32_t K, int self_base, uint32_t lane,
                                       uint32_t* __restrict__ out, float* __restrict__ dist_out,
                                       uint32_t* __restrict__ len) const {
    bool keep[H];
    uint64_t m[H];
    #pragma unroll
    for (int i = 0; i < H; ++i) {
      keep[i] = 64 * i + lane < K && v[i] != kNoKey && !(self_base && (uint32_t)v[i] == (uint32_t)row);
      m[i] = __ballot(keep[i]);
    }
    uint32_t base = 0;
    #pragma unroll
    for (int i = 0; i < H; ++i) {
      if (keep[i]) {
        const uint32_t pos = base + __popcll(m[i] & ((1ull << lane) - 1));
        out[row * K + pos] = (uint32_t)v[i];
        if (dist_out) dist_out[row * K + pos] = __uint_as_float((uint32_t)(v[i] >> 32));
      }
      base += __popcll(m[i]);
    }
    if (lane == 0) len[row] = base;
  }
};

// ---- the prefilter workgroup's lists.  A workgroup of
// THREADS threads holds kKnnRows query rows against tiles of COLS base rows;
// wave w computes the 32x32 block of rows rb = 32 (w & 1) and columns
// cb = 32 (w >> 1), and merges the MR = kKnnRows / waves rows from w MR on.
// A kernel's LDS struct derives from KnnLists and appends its operand tiles.
template <int TOP, int COLS>
struct KnnLists {
  uint64_t top[kKnnRows][TOP];    // sorted ascending per row
  uint64_t buf[kKnnRows][COLS];   // this tile's keys below the row threshold
  uint32_t cnt[kKnnRows];
  uint32_t any[2];                // tile t inserted something: parity t & 1
};

// The query row of element i of a lane's 32x32 accumulator (h = lane >> 5).
__device__ __forceinline__ uint32_t knn_acc_row(uint32_t rb, uint32_t h, int i) {
  return rb + (i & 3) + 8 * (i >> 2) + 4 * h;
}

template <int THREADS, int TOP, int COLS>
__device__ __forceinline__ void knn_lists_init(KnnLists<TOP, COLS>& L, uint32_t tid) {
  for (uint32_t i = tid; i < kKnnRows * TOP; i += THREADS) (&L.top[0][0])[i] = kNoKey;
  if (tid < kKnnRows) L.cnt[tid] = 0;
  if (tid < 2) L.any[tid] = 0;
}

// The constants (norms, or the u8 form's int32 constants) and the thresholds of
// the lane's 16 accumulator rows.
template <class T>
__device__ __forceinline__ void knn_rows_init(const T* __restrict__ qn, uint64_t row0, uint64_t M, uint32_t rb,
                                              uint32_t h, T (&qnr)[16], uint32_t (&thi)[16]) {
  #pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint64_t qr = row0 + knn_acc_row(rb, h, i);
    qnr[i] = qr < M ? qn[qr] : T(0);
    thi[i] = 0xffffffffu;
  }
}

// The end of tile t, after its MFMAs.  par is t & 1, a variable the caller
// starts at 0 and this function flips: carried through the loop it stays one
// scalar; derived from t here, the compiler recomputes it on both sides of the
// col < N branch and the insert block moves out of line (k_knn_i8 1 to 2 % slower).
// col is the lane's base row, xn[col] its
// constant (norm) when col < N; dist(i, cn) gives the bits of the distance of
// base row col to the lane's accumulator row i (ordered as unsigned).  The
// constant is loaded here, behind the col < N test and after the MFMAs: a load
// the compiler can move up to the tile's start makes the MFMAs wait for the
// next tile's prefetch.  A key at or below its row's threshold (thi: the distance bits of
// the row's last entry) goes to the row's insertion buffer; the owning wave
// merges the buffers into the sorted lists; stage() runs between the merge and
// the barrier behind it (the kernels store the next tile's operands there).
// The ordering rules, for every kernel that calls this:
//  * any has two parities.  Tile t's inserts raise any[t & 1] while thread 0
//    clears any[(t + 1) & 1], both before the first barrier; nobody writes
//    any[t & 1] again before tile t + 2, so every thread reads the same
//    `merged` after that barrier and the branches on it, the third barrier
//    included, are uniform over the workgroup.
//  * The merge reads cnt and buf after the first barrier; cnt is reset and thi
//    re-read only after the second, when every merge has been stored.
//  * The cnt resets must land before the next tile's inserts: the third
//    barrier, needed only when a merge happened.
template <int THREADS, int TOP, int COLS, class T, class Dist, class Stage>
__device__ __forceinline__ void knn_tile_end(KnnLists<TOP, COLS>& L, uint32_t& par, uint64_t col, uint64_t N,
                                             const T* __restrict__ xn, uint32_t rb, uint32_t h,
                                             uint32_t (&thi)[16], Dist&& dist, Stage&& stage) {
  constexpr uint32_t MR = kKnnRows / (THREADS / 64);
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (col < N) {
    const T cn = xn[col];
    #pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t lr = knn_acc_row(rb, h, i);
      const uint32_t db = dist(i, cn);
      if (db <= thi[i]) {
        const uint64_t key = ((uint64_t)db << 32) | (uint32_t)col;
        if (db < thi[i] || key < L.top[lr][TOP - 1]) {
          const uint32_t slot = atomicAdd(&L.cnt[lr], 1u);
          L.buf[lr][slot] = key;
          L.any[par] = 1;
        }
      }
    }
  }
  if (tid == 0) L.any[par ^ 1] = 0;
  __syncthreads();
  const bool merged = L.any[par] != 0;
  if (merged) {
    for (uint32_t r = w * MR; r < w * MR + MR; ++r) {
      const uint32_t n = L.cnt[r];
      if (n) TopKeys<TOP>::merge_row(L.top[r], L.buf[r], n, lane);
    }
  }
  stage();
  __syncthreads();
  if (merged) {
    if (lane < MR) L.cnt[w * MR + lane] = 0;
    #pragma unroll
    for (int i = 0; i < 16; ++i) thi[i] = (uint32_t)(L.top[knn_acc_row(rb, h, i)][TOP - 1] >> 32);
  }
  if (merged) __syncthreads();
  par ^= 1;
}

// The float distance of the prefilters, max(0, qn + cn - 2 acc), as bits.
__device__ __forceinline__ uint32_t knn_dist_bits(float qn, float cn, float acc) {
  float d = __fsub_rn(__fadd_rn(qn, cn), __fmul_rn(2.0f, acc));
  d = d < 0.0f ? 0.0f : d;
  return __float_as_uint(d);
}

// Every row's list to out [M][TOP] (ids) and out_hi (distance bits, when
// given), and to tau (when given) the distance of its last entry (NaN bits
// while fewer than TOP keys exist).
template <int THREADS, int TOP, int COLS>
__device__ __forceinline__ void knn_lists_write(const KnnLists<TOP, COLS>& L, uint64_t row0, uint64_t M,
                                                uint32_t* __restrict__ out, uint32_t* __restrict__ out_hi,
                                                float* __restrict__ tau) {
  constexpr uint32_t MR = kKnnRows / (THREADS / 64);
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint32_t r = w * MR; r < w * MR + MR; ++r) {
    const uint64_t qr = row0 + r;
    if (qr < M) {
      #pragma unroll
      for (uint32_t e = lane; e < TOP; e += 64) {
        out[qr * TOP + e] = (uint32_t)L.top[r][e];
        if (out_hi) out_hi[qr * TOP + e] = (uint32_t)(L.top[r][e] >> 32);
      }
      if (tau && lane == 63) tau[qr] = __uint_as_float((uint32_t)(L.top[r][TOP - 1] >> 32));
    }
  }
}

// ---- the brute-force stream: one workgroup of kBlock threads ranks the rows
// [r0, r1) of X against the query row q (copied to LDS) by (L2Dist bits, id),
// L2Dist in the reference order by 8-lane groups.  Each wave strides the rows
// eight at a time and keeps its TOP smallest keys sorted in registers with the
// last as threshold; wave 0 merges the four and returns the result (the other
// waves' return value is their own list).  The id of row r is idmap[r], or r
// without a map.  The caller puts a barrier before L is used again.
template <int TOP, int MAXD>
struct BruteLds {
  uint64_t top[kBlock / 64][TOP];
  float q[MAXD];
};

template <int TOP, int MAXD>
__device__ __forceinline__ TopKeys<TOP> knn_brute_stream(BruteLds<TOP, MAXD>& L, const float* __restrict__ X,
                                                         uint32_t dim, const float* __restrict__ q, uint64_t r0,
                                                         uint64_t r1, const uint32_t* __restrict__ idmap) {
  constexpr uint32_t W = kBlock / 64;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 3, k = lane & 7;
  for (uint32_t i = tid; i < dim; i += kBlock) L.q[i] = q[i];
  __syncthreads();
  TopKeys<TOP> t = TopKeys<TOP>::empty();
  for (uint64_t s = r0 + 8 * w; s < r1; s += 8 * W) {   // uniform per wave: every lane stays active
    const uint64_t r = s + g;
    const bool ok = r < r1;
    const uint64_t rr = ok ? r : r0;
    const float d = l2_group8(X + rr * dim, L.q, dim, k);
    const uint64_t key = ok ? (((uint64_t)__float_as_uint(d) << 32) | (idmap ? idmap[rr] : rr)) : kNoKey;
    uint64_t m = __ballot(k == 0 && key < t.last());
    while (m) {
      const int src = __builtin_ctzll(m);
      m &= m - 1;
      t.insert(readlane64(key, src), lane);
    }
  }
  t.store(L.top[w], lane);
  __syncthreads();
  if (w == 0)
    for (uint32_t o = 1; o < W; ++o)
      for (uint32_t i = 0; i < TOP; ++i) t.insert(L.top[o][i], lane);
  return t;
}

// Bounds of the certificate: eps = crel (qn + maxnorm) +
// kCertAbs bounds |prefilter distance - L2Dist| of k_knn_bf16x3 and
// k_knn_bf16x3_w for every base row while qn + maxnorm <= kCertMaxSum (no
// overflow in the products or sums).
constexpr float kCertAbs = 0x1.0p-50f;
constexpr float kCertMaxSum = 0x1.0p126f;

}  // namespace pm

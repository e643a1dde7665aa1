// pm_graph_dev.h — device helpers shared by the kNN / robustPrune kernels of
// pm_graph.hip (rows up to 192 wide) and pm_graph_wide.hip (rows up to 1,024):
// the sorted top-64 list of a wave, the 8-lane L2Dist in the reference's order,
// the re-rank of a row's 64 candidates and the certificate's constants; and the
// two-keys-per-lane top-128 list of pm_graph_k128.hip.
// Include from HIP translation units only, after pm_internal.h.
#pragma once
#include <hip/hip_runtime.h>

#include "pm_internal.h"

namespace pm {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kKnnRows = 64;      // query rows per workgroup
constexpr int kKnnTop = 64;       // prefilter keys kept per query row
constexpr uint64_t kNoKey = ~0ull;

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) {
  const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
  return ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(v >> 32), l) << 32) |
         __builtin_amdgcn_readlane((uint32_t)v, l);
}

// Insert the wave-uniform key x into the sorted top-64 t (lane i holds entry i).
__device__ __forceinline__ uint64_t knn_insert(uint64_t t, uint64_t x, uint32_t lane) {
  if (x >= readlane64(t, 63)) return t;   // uniform: x and the last key are wave-uniform
  const uint32_t pos = __popcll(__ballot(t < x));
  const uint64_t up = shfl_up64(t, 1);
  return lane < pos ? t : (lane == pos ? x : up);
}

// Merge the row's insertion buffer into its sorted top-64 (lane i holds entry i).
__device__ __forceinline__ void knn_merge_row(uint64_t* top, const uint64_t* buf, uint32_t n, uint32_t lane) {
  uint64_t t = top[lane];
  for (uint32_t e = 0; e < n; ++e) t = knn_insert(t, buf[e], lane);
  top[lane] = t;
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

// Bitonic sort of 64 u64 keys held one per lane (ascending by lane).
__device__ __forceinline__ uint64_t wave_sort64(uint64_t x, uint32_t lane) {
  for (int k = 2; k <= 64; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)x, j), hi = __shfl_xor((uint32_t)(x >> 32), j);
      const uint64_t y = ((uint64_t)hi << 32) | lo;
      const bool up = (lane & k) == 0, lower = (lane & j) == 0;
      const uint64_t mn = x < y ? x : y, mx = x < y ? y : x;
      x = (up == lower) ? mn : mx;
    }
  }
  return x;
}

// One wave's re-rank of a query row: exact L2Dist of the 64 candidates, keys
// (dist, id) in the wave's LDS row, sorted; lane i returns the i-th key.
__device__ __forceinline__ uint64_t knn_rerank_keys(const float* __restrict__ X, uint64_t N, uint32_t dim,
                                                    const float* __restrict__ q, const uint32_t* __restrict__ cand,
                                                    uint64_t* keys, uint32_t lane) {
  const uint32_t g = lane >> 3, k = lane & 7;
  for (uint32_t r = 0; r < 8; ++r) {
    const uint32_t c = r * 8 + g;
    const uint32_t id = cand[c];
    const bool ok = id < N;
    const float d = l2_group8(X + (ok ? (uint64_t)id : 0) * dim, q, dim, k);
    if (k == 0) keys[c] = ok ? (((uint64_t)__float_as_uint(d) << 32) | id) : kNoKey;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // this wave's LDS keys visible to its lanes
  __builtin_amdgcn_wave_barrier();
  return wave_sort64(keys[lane], lane);
}

// The first K of a row's sorted keys x (self dropped when self_base: the
// reference removes u from NGT's K results) go to out[row][K], their count to
// len[row].
__device__ __forceinline__ void knn_emit(uint64_t x, uint64_t row, uint32_t K, int self_base, uint32_t lane,
                                         uint32_t* __restrict__ out, float* __restrict__ dist_out,
                                         uint32_t* __restrict__ len) {
  const uint32_t id = (uint32_t)x;
  const bool in = lane < K && x != kNoKey;
  const bool self = self_base && id == (uint32_t)row;
  const uint64_t keep = __ballot(in && !self);
  const uint32_t pos = __popcll(keep & ((1ull << lane) - 1));
  if (in && !self) {
    out[row * K + pos] = id;
    if (dist_out) dist_out[row * K + pos] = __uint_as_float((uint32_t)(x >> 32));
  }
  if (lane == 0) len[row] = __popcll(keep);
}

// ---- the 128-key list of pm_graph_k128.hip: a wave holds a
// sorted top-128 as two keys per lane, entry `lane` in a and entry 64 + lane
// in b, so the list is a then b, each half ascending by lane.
constexpr int kKnnTop2 = 128;     // prefilter keys kept per query row by the _k128 entry points

struct Key2 {
  uint64_t a, b;
};

// Insert the wave-uniform key x into the sorted top-128 t.
__device__ __forceinline__ Key2 knn_insert128(Key2 t, uint64_t x, uint32_t lane) {
  if (x >= readlane64(t.b, 63)) return t;   // uniform: x and entry 127 are wave-uniform
  // the halves are sorted: once a key of a is >= x, every key of b is
  const uint32_t pos = __popcll(__ballot(t.a < x)) + __popcll(__ballot(t.b < x));
  const uint64_t carry = readlane64(t.a, 63);
  const uint64_t ua = shfl_up64(t.a, 1);
  uint64_t ub = shfl_up64(t.b, 1);
  ub = lane == 0 ? carry : ub;
  Key2 r;
  if (pos < 64) {   // uniform
    r.a = lane < pos ? t.a : (lane == pos ? x : ua);
    r.b = ub;
  } else {
    const uint32_t p = pos - 64;
    r.a = t.a;
    r.b = lane < p ? t.b : (lane == p ? x : ub);
  }
  return r;
}

// Merge the row's insertion buffer into its sorted top-128.
__device__ __forceinline__ void knn_merge_row128(uint64_t* top, const uint64_t* buf, uint32_t n, uint32_t lane) {
  Key2 t = {top[lane], top[64 + lane]};
  for (uint32_t e = 0; e < n; ++e) t = knn_insert128(t, buf[e], lane);
  top[lane] = t.a;
  top[64 + lane] = t.b;
}

// One compare-exchange step of the 128-key bitonic network on the entry idx
// held in x (partner idx ^ j in lane ^ j, j < 64).
__device__ __forceinline__ uint64_t sort128_step(uint64_t x, uint32_t idx, int k, int j) {
  const uint32_t lo = __shfl_xor((uint32_t)x, j), hi = __shfl_xor((uint32_t)(x >> 32), j);
  const uint64_t y = ((uint64_t)hi << 32) | lo;
  const bool up = (idx & k) == 0, lower = (idx & j) == 0;
  const uint64_t mn = x < y ? x : y, mx = x < y ? y : x;
  return (up == lower) ? mn : mx;
}

// Bitonic sort of 128 u64 keys held two per lane (entries lane and 64 + lane),
// ascending by entry.
__device__ __forceinline__ Key2 wave_sort128(Key2 t, uint32_t lane) {
  for (int k = 2; k <= 128; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j == 64) {   // k = 128: entry lane against entry 64 + lane, ascending
        const uint64_t mn = t.a < t.b ? t.a : t.b, mx = t.a < t.b ? t.b : t.a;
        t.a = mn;
        t.b = mx;
      } else {
        t.a = sort128_step(t.a, lane, k, j);
        t.b = sort128_step(t.b, 64 + lane, k, j);
      }
    }
  }
  return t;
}

// knn_rerank_keys for 128 candidates: 16 rounds of 8, keys in the wave's LDS
// row of 128, sorted; the lane returns entries lane and 64 + lane.
__device__ __forceinline__ Key2 knn_rerank_keys128(const float* __restrict__ X, uint64_t N, uint32_t dim,
                                                   const float* __restrict__ q, const uint32_t* __restrict__ cand,
                                                   uint64_t* keys, uint32_t lane) {
  const uint32_t g = lane >> 3, k = lane & 7;
  for (uint32_t r = 0; r < kKnnTop2 / 8; ++r) {
    const uint32_t c = r * 8 + g;
    const uint32_t id = cand[c];
    const bool ok = id < N;
    const float d = l2_group8(X + (ok ? (uint64_t)id : 0) * dim, q, dim, k);
    if (k == 0) keys[c] = ok ? (((uint64_t)__float_as_uint(d) << 32) | id) : kNoKey;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // this wave's LDS keys visible to its lanes
  __builtin_amdgcn_wave_barrier();
  const Key2 t = {keys[lane], keys[64 + lane]};
  return wave_sort128(t, lane);
}

// knn_emit for a sorted top-128 and K up to 128: two ballots, the kept entries
// of a before those of b.
__device__ __forceinline__ void knn_emit128(Key2 t, uint64_t row, uint32_t K, int self_base, uint32_t lane,
                                            uint32_t* __restrict__ out, float* __restrict__ dist_out,
                                            uint32_t* __restrict__ len) {
  const bool ka = lane < K && t.a != kNoKey && !(self_base && (uint32_t)t.a == (uint32_t)row);
  const bool kb = 64 + lane < K && t.b != kNoKey && !(self_base && (uint32_t)t.b == (uint32_t)row);
  const uint64_t ma = __ballot(ka), mb = __ballot(kb);
  const uint64_t below = (1ull << lane) - 1;
  const uint32_t na = __popcll(ma);
  if (ka) {
    const uint32_t pos = __popcll(ma & below);
    out[row * K + pos] = (uint32_t)t.a;
    if (dist_out) dist_out[row * K + pos] = __uint_as_float((uint32_t)(t.a >> 32));
  }
  if (kb) {
    const uint32_t pos = na + __popcll(mb & below);
    out[row * K + pos] = (uint32_t)t.b;
    if (dist_out) dist_out[row * K + pos] = __uint_as_float((uint32_t)(t.b >> 32));
  }
  if (lane == 0) len[row] = na + __popcll(mb);
}

// Bounds of the certificate: eps = crel (qn + maxnorm) +
// kCertAbs bounds |prefilter distance - L2Dist| of k_knn_bf16x3 and
// k_knn_bf16x3_w for every base row while qn + maxnorm <= kCertMaxSum (no
// overflow in the products or sums).
constexpr float kCertAbs = 0x1.0p-50f;
constexpr float kCertMaxSum = 0x1.0p126f;

}  // namespace pm

// pm_search_dev.h — device helpers of the on-device beam search, shared by the
// team round of the batched serving loop (pm_drl.hip) and the batched
// non-private search (pm_knnb.hip): the knownVertices table, Go's
// container/heap Push and Pop on a one-wave min-heap, and the wave-wide
// selections.  Device code only (included by .hip units).
#pragma once
#include <hip/hip_runtime.h>

#include "pm_internal.h"

namespace pm {

struct HeapE { float d; uint32_t slot; };

// Open-addressing tables of u64 entries {key + 1 | value << 32} (0 = empty).
// A session's tables are only touched by its own workgroup (one CU) within a
// launch, and across launches through the stream's kernel boundaries, so
// workgroup-scope atomics suffice (no L2 write-back or invalidate: MI355X's
// L2s are per XCD, and an agent-scope fence would write one back).
__device__ __forceinline__ bool tab_find(const uint64_t* t, uint32_t mask, uint32_t key, uint32_t* val) {
  for (uint32_t i = drl_hash(key) & mask;; i = (i + 1) & mask) {
    const uint64_t e = __hip_atomic_load(const_cast<uint64_t*>(t) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (e == 0) return false;
    if ((uint32_t)e == key + 1u) { *val = (uint32_t)(e >> 32); return true; }
  }
}
__device__ __forceinline__ void tab_put(uint64_t* t, uint32_t mask, uint32_t key, uint32_t val) {
  const uint64_t ne = ((uint64_t)val << 32) | (uint64_t)(key + 1u);
  for (uint32_t i = drl_hash(key) & mask;; i = (i + 1) & mask) {
    uint64_t e = 0;
    if (__hip_atomic_compare_exchange_strong(t + i, &e, ne, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_WORKGROUP))
      return;
    if ((uint32_t)e == key + 1u) {   // insert or overwrite (FlatMap::put)
      __hip_atomic_store(t + i, ne, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      return;
    }
  }
}

// container/heap.Push: append, then up().  up() swaps the new element with its
// parent while it is strictly Less (dist <); the ancestors on its path are
// non-increasing upward (heap order), so the elements it passes are exactly the
// c nearest ancestors with dist > x.  Lane l >= 1 holds the ancestor l levels
// up (0-based index ((n + 1) >> l) - 1): one LDS read per lane, one ballot, and
// the c passed ancestors move one level down while x lands at ancestor c.
__device__ __forceinline__ void heap_push(HeapE* hp, uint32_t& nh, HeapE x, uint32_t lane) {
  const uint32_t j1 = nh + 1;   // 1-based position of the new element
  const bool valid = lane >= 1 && lane < 32 && (j1 >> lane) >= 1u;
  HeapE a{0.0f, 0u};
  if (valid) a = hp[(j1 >> lane) - 1];
  const uint64_t b = __ballot(valid && x.d < a.d);
  const uint32_t c = (uint32_t)__builtin_ctzll(~(b >> 1));   // consecutive passed ancestors from lane 1
  if (lane >= 1 && lane <= c) hp[(j1 >> (lane - 1)) - 1] = a;
  if (lane == c) hp[(j1 >> c) - 1] = x;
  nh = j1;   // (one wave: its LDS operations complete in order, so the next push reads these stores)
}
// A run of container/heap.Push calls with the insertion path cached in
// registers (lane l >= 1: the value of ancestor level l of the next insertion
// position j, 1-based, node (j >> l) - 1), so a push costs one ballot and its
// stores, not an LDS round trip: after a push the next position j + 1 shares
// every ancestor above the lowest zero bit of j, whose new values are known
// (shifted down one level through c, x at level c); only the levels below
// it are read from LDS (after this push's stores; none of them is on j's path,
// except the root when j = 2^t - 1, also taken from the registers).  The same
// result as heap_push push by push (restated and checked against Go's
// container/heap with ties in tools/sim_heap_path.py).
__device__ __forceinline__ HeapE dpp_from_up(HeapE v) {   // lane l <- lane l + 1 (wave_shl:1)
  HeapE r;
  r.d = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v.d), 0x130, 0xf, 0xf, true));
  r.slot = (uint32_t)__builtin_amdgcn_mov_dpp((int)v.slot, 0x130, 0xf, 0xf, true);
  return r;
}
__device__ __forceinline__ HeapE dpp_from_down(HeapE v) {   // lane l <- lane l - 1 (wave_shr:1)
  HeapE r;
  r.d = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v.d), 0x138, 0xf, 0xf, true));
  r.slot = (uint32_t)__builtin_amdgcn_mov_dpp((int)v.slot, 0x138, 0xf, 0xf, true);
  return r;
}
__device__ __forceinline__ HeapE path_load(const HeapE* hp, uint32_t j, uint32_t lane) {
  const uint32_t a = lane >= 1 && lane < 32 ? j >> lane : 0u;
  return a ? hp[a - 1] : HeapE{0.0f, 0u};
}
__device__ __forceinline__ void path_push(HeapE* hp, uint32_t& j, HeapE& pv, HeapE x, uint32_t lane) {
  const uint32_t jn = j + 1;
  const uint32_t aj = lane >= 1 && lane < 32 ? j >> lane : 0u;
  const uint64_t b = __ballot(aj >= 1 && x.d < pv.d);
  const uint32_t c = (uint32_t)__builtin_ctzll(~(b >> 1));
  if (lane >= 1 && lane <= c) hp[(j >> (lane - 1)) - 1] = pv;
  if (lane == c) hp[(j >> c) - 1] = x;
  const HeapE up = dpp_from_up(pv), dn = dpp_from_down(pv);
  const uint32_t an = lane >= 1 && lane < 32 ? jn >> lane : 0u;
  HeapE nv{0.0f, 0u};
  if (an >= 1) {
    if (an == aj) nv = lane < c ? up : (lane == c ? x : pv);
    else if (an == (j >> (lane - 1))) nv = lane - 1 < c ? pv : (lane - 1 == c ? x : dn);
    else nv = hp[an - 1];
  }
  pv = nv;
  j = jn;
}

// container/heap.Pop: swap(0, n-1), down(0, n-1), remove the last.  down()
// moves the larger-index child only when strictly Less than the smaller-index
// one, and stops when the chosen child is not Less than the element.
__device__ __forceinline__ HeapE heap_pop(HeapE* hp, uint32_t& nh, uint32_t lane) {
  const uint32_t n1 = nh - 1;
  const HeapE top = hp[0];
  const HeapE x = hp[n1];
  uint32_t i = 0;
  for (;;) {
    const uint32_t j1 = 2 * i + 1;
    if (j1 >= n1) break;
    uint32_t j = j1;
    HeapE e = hp[j1];
    if (j1 + 1 < n1) {
      const HeapE e2 = hp[j1 + 1];
      if (e2.d < e.d) { j = j1 + 1; e = e2; }
    }
    if (!(e.d < x.d)) break;
    if (lane == 0) hp[i] = e;
    i = j;
  }
  if (lane == 0) hp[i] = x;
  nh = n1;
  return top;
}

// wave-wide lexicographic minimum of (d, id)
__device__ __forceinline__ void wave_min2(float& d, uint32_t& id) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float od = __shfl_xor(d, o);
    const uint32_t oi = __shfl_xor(id, o);
    if (od < d || (od == d && oi < id)) { d = od; id = oi; }
  }
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
__device__ __forceinline__ double wave_sumd(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// Occurrences of x among a[0 .. len) (LDS, 16-B aligned): 4 ids per read,
// no early exit, so the reads of the loop pipeline.
__device__ __forceinline__ uint32_t lds_count(const uint32_t* a, uint32_t len, uint32_t x) {
  const uint4* a4 = (const uint4*)a;
  uint32_t c = 0;
  const uint32_t n4 = len / 4;
#pragma unroll 4
  for (uint32_t j = 0; j < n4; ++j) {
    const uint4 v = a4[j];
    c += (v.x == x) + (v.y == x) + (v.z == x) + (v.w == x);
  }
  for (uint32_t j = n4 * 4; j < len; ++j) c += a[j] == x;
  return c;
}

}  // namespace pm

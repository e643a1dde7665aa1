// pm_knnb.hip — the batched non-private beam search (pm_search_knn_batch,
// GraphANNFrontend.SearchKNNBatch, graphann/search.go:236-245).
//
// One launch answers a batch of queries over a non-private in-memory graph:
// one kKnbThreads (256-thread) workgroup runs a whole SearchKNN
// (search.go:114-234) of one query against the device's vectors [n][dim] and
// graph [n][m], with no host round trip.  Same operations in the same order as
// the host loop (pm_engine.cpp search_knn_impl), the oracle
// (oracle/pm_oracle.cpp or_search_knn) and the team round (pm_drl.hip), with
// their tie rules:
//   * begin (search.go:129-148): the L2 of the start set to the query; the
//     first min(parallel, ns) start vertices by (distance, position) become
//     known with reach step 0 and are pushed in that order;
//   * a round (search.go:150-207): wave 0 pops `parallel` vertices
//     (container/heap's exact Pop); their m neighbours each, read from the
//     graph, are the round's parallel x m positions; in position order an id
//     that is known, repeated at an earlier position or whose neighbour list
//     is all zero is skipped, the rest become known with reach = step and
//     their L2 to the query (8 lanes per row, 32 rows per pass), and wave 0
//     pushes them in position order (container/heap's exact Push);
//   * end (search.go:211-233): the top k by (distance, id), -1 padded, with
//     their reach steps.
// A pop that finds the heap empty would draw m ids from the graph's id stream
// (search.go:155-159), which is sequential across the queries of a batch: the
// workgroup then sets needs_host[query] and stops, and the host re-runs that
// query in order.
//
// The whole search state stays in LDS: the heap (8 B per slot), the known
// table (2 x 8 B), and per known slot its distance, id and reach step (12 B),
// 36 B per slot of kcap = the next power of two >= parallel (1 + max_step m);
// the known vertices' neighbour lists are the graph's own rows.
#include <hip/hip_runtime.h>

#include "pm_internal.h"
#include "pm_search_dev.h"

namespace pm {

constexpr uint32_t kKnbThreads = 256, kKnbRows = kKnbThreads / 8;

// L2Dist of a global row against the query in LDS, one 8-lane group, bit-exact
// in the reference's order (k_l2_rows, l2_distance_amd64.s:4-36): lane k owns
// the running sum over elements 8t + k (subtract, multiply, add, each rounded:
// no FMA), then the xor-1/2/4 tree, then the scalar tail of dim % 8.  The
// loads of 16 terms are issued ahead of the (ordered) sum.  Every lane of the
// wave calls it (the shuffles); a group without a row passes live = false.
__device__ __forceinline__ float l2_row8(const float* __restrict__ row, const float* q, uint32_t dim, uint32_t k,
                                         bool live) {
  const uint32_t dimS = dim & ~7u;
  float acc = 0.0f;
  if (live) {
    uint32_t t = k;
    for (; t + 120 < dimS; t += 128) {
      float r[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) r[u] = row[t + 8 * u];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const float d = __fsub_rn(r[u], q[t + 8 * u]);
        acc = __fadd_rn(acc, __fmul_rn(d, d));
      }
    }
#pragma unroll 4
    for (; t < dimS; t += 8) {
      const float d = __fsub_rn(row[t], q[t]);
      acc = __fadd_rn(acc, __fmul_rn(d, d));
    }
  }
  acc = __fadd_rn(acc, __shfl_xor(acc, 1));
  acc = __fadd_rn(acc, __shfl_xor(acc, 2));
  acc = __fadd_rn(acc, __shfl_xor(acc, 4));
  float d = dimS ? acc : 0.0f;
  if (live)
    for (uint32_t i = dimS; i < dim; ++i) {
      const float t = __fsub_rn(row[i], q[i]);
      d = __fadd_rn(d, __fmul_rn(t, t));
    }
  return d;
}

__global__ void __launch_bounds__(kKnbThreads) k_knn_batch(const KnbArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const uint32_t qi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t k8 = tid & 7, grp = tid >> 3;
  const uint32_t m = A.m, dim = A.dim, kcap = A.kcap, ns = A.ns, nb = A.parallel * m;
  const uint32_t nb4 = (nb + 3) & ~3u, dim4 = (dim + 3) & ~3u;
  // (kcap is a multiple of 4: bat starts 16-B aligned for lds_count)
  HeapE* hp = (HeapE*)lds;                                  // [kcap] the heap
  uint64_t* ktab = (uint64_t*)(lds + (size_t)kcap * 8);     // [2 kcap] knownVertices: id -> slot
  float* kdist = (float*)(lds + (size_t)kcap * 24);         // [kcap] known slot's distance
  uint32_t* kid = (uint32_t*)(kdist + kcap);                // [kcap] ... id
  uint32_t* kreach = kid + kcap;                            // [kcap] ... reach step
  uint32_t* bat = kreach + kcap;                            // [nb] the round's ids
  uint32_t* nlist = bat + nb4;                              // [nb] the round's new ids by rank
  float* qv = (float*)(nlist + nb4);                        // [dim] the query
  float* sd = qv + dim4;                                    // [ns] the start set's distances
  __shared__ uint32_t s_wcnt[kKnbThreads / 64];
  __shared__ uint32_t s_stop;
  __shared__ float s_seld[2][kKnbThreads / 64];
  __shared__ uint32_t s_seli[2][kKnbThreads / 64], s_selj[2][kKnbThreads / 64];
  const uint32_t kmask = 2 * kcap - 1;

  // ---- begin: an empty known set, the query, the start set's distances
  for (uint32_t i = tid; i < 2 * kcap; i += kKnbThreads) ktab[i] = 0;
  for (uint32_t i = tid; i < dim; i += kKnbThreads) qv[i] = A.queries[(uint64_t)qi * dim + i];
  __syncthreads();
  for (uint32_t r0 = 0; r0 < ns; r0 += kKnbRows) {
    const uint32_t r = r0 + grp;
    const bool live = r < ns;
    const float d = l2_row8(A.vec + (uint64_t)(live ? A.start[r] : 0u) * dim, qv, dim, k8, live);
    if (live && k8 == 0) sd[r] = d;
  }
  __syncthreads();
  uint32_t nknown = min(A.parallel, ns);   // (start ids are distinct: none of them is skipped as known)
  uint32_t nheap = 0, pend = 0;            // wave 0: the heap's size; new vertices not pushed yet
  if (wave == 0) {
    // the first `parallel` start vertices in (distance, position) order (search.go:130-146)
    float pd = 0.0f;
    uint32_t ppos = 0;
    for (uint32_t t = 0; t < nknown; ++t) {
      float bd = __builtin_inff();
      uint32_t bp = 0xffffffffu;
      for (uint32_t j = lane; j < ns; j += 64) {
        const float d = sd[j];
        const bool after = t == 0 || d > pd || (d == pd && j > ppos);
        if (after && (d < bd || (d == bd && j < bp))) { bd = d; bp = j; }
      }
      wave_min2(bd, bp);
      if (bp >= ns) bp = ppos;   // (a NaN distance: never selected; keep the reads in bounds)
      pd = bd; ppos = bp;
      const uint32_t id = A.start[bp];
      if (lane == 0) {
        kdist[t] = bd;
        kid[t] = id;
        kreach[t] = 0;
        tab_put(ktab, kmask, id, t);
      }
      heap_push(hp, nheap, HeapE{bd, t}, lane);
    }
  }
  __syncthreads();

  // ---- the rounds
  bool stopped = false;
  for (uint32_t step = 0; step < A.max_step; ++step) {
    if (wave == 0) {
      if (pend) {   // the previous round's new vertices, in position order (slots nknown - pend ..)
        const uint32_t base = nknown - pend;
        uint32_t j = nheap + 1;
        HeapE pv = path_load(hp, j, lane);
        for (uint32_t r0 = 0; r0 < pend; r0 += 64) {
          const float dl = r0 + lane < pend ? kdist[base + r0 + lane] : 0.0f;
          const uint32_t cnt = min(64u, pend - r0);
          for (uint32_t r = 0; r < cnt; ++r) {
            const float d = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dl), (int)r));
            path_push(hp, j, pv, HeapE{d, base + r0 + r}, lane);
          }
        }
        nheap = j - 1;
      }
      // the next batch (search.go:153-171): each pop's neighbour row is loaded while the next pops run
      bool empty = false;
      for (uint32_t r0 = 0; r0 < A.parallel; r0 += 4) {
        uint32_t v[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
          v[u] = 0;
          if (r0 + u < A.parallel && !empty) {
            if (nheap) {
              const uint32_t id = kid[heap_pop(hp, nheap, lane).slot];
              if (lane < m) v[u] = A.graph[(uint64_t)id * m + lane];
            } else {
              empty = true;   // the reference draws from the id stream here: the host's
            }
          }
        }
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u)
          if (r0 + u < A.parallel && lane < m) bat[(r0 + u) * m + lane] = v[u];
      }
      if (lane == 0) s_stop = empty ? 1u : 0u;
    }
    __syncthreads();
    if (s_stop) { stopped = true; break; }
    // ---- each position: known, repeated at an earlier position, or an all-zero neighbour list
    bool nw = false;
    uint32_t myid = 0;
    if (tid < nb) {
      myid = bat[tid];
      bool known = lds_count(bat, tid, myid) != 0;
      uint32_t v;
      if (!known) known = tab_find(ktab, kmask, myid, &v);
      if (!known) {
        const uint32_t* row = A.graph + (uint64_t)myid * m;
        uint32_t o = 0;
        if ((m & 3u) == 0) {
          for (uint32_t j = 0; j < m / 4; ++j) {
            const uint4 x = ((const uint4*)row)[j];
            o |= x.x | x.y | x.z | x.w;
          }
        } else {
          for (uint32_t j = 0; j < m; ++j) o |= row[j];
        }
        nw = o != 0;
      }
    }
    // ---- the new vertices in position order (search.go:185-207): slots, ids, reach steps, the table
    const uint64_t bal = __ballot(nw);
    if (lane == 0) s_wcnt[wave] = (uint32_t)__builtin_popcountll(bal);
    __syncthreads();
    uint32_t before = 0, total_new = 0;
    for (uint32_t w = 0; w < kKnbThreads / 64; ++w) {
      if (w < wave) before += s_wcnt[w];
      total_new += s_wcnt[w];
    }
    if (nw) {
      const uint32_t rank = before + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
      const uint32_t slot = nknown + rank;
      kid[slot] = myid;
      kreach[slot] = step;
      nlist[rank] = myid;
      tab_put(ktab, kmask, myid, slot);
    }
    __syncthreads();
    // ---- their distances: 8 lanes per row, 32 rows per pass, a pass's gathers in flight together
    for (uint32_t r0 = 0; r0 < total_new; r0 += kKnbRows) {
      const uint32_t r = r0 + grp;
      const bool live = r < total_new;
      const float d = l2_row8(A.vec + (uint64_t)(live ? nlist[r] : 0u) * dim, qv, dim, k8, live);
      if (live && k8 == 0) kdist[nknown + r] = d;
    }
    nknown += total_new;
    pend = total_new;   // (not pushed after the last round: the end reads the known set only)
    __syncthreads();
  }
  if (tid == 0) A.needs_host[qi] = stopped ? 1u : 0u;
  if (stopped) return;

  // ---- end: the top k by (distance, id) (search.go:211-233), -1 padded, with the reach steps
  int64_t* oid = A.ids + (uint64_t)qi * A.k;
  int64_t* ost = A.steps + (uint64_t)qi * A.k;
  float pd = 0.0f;
  uint32_t pi = 0;
  for (uint32_t t = 0; t < A.k; ++t) {
    const uint32_t par = t & 1u;
    float bd = __builtin_inff();
    uint32_t bi = 0xffffffffu, bj = 0xffffffffu;
#pragma unroll 2
    for (uint32_t j = tid; j < nknown; j += kKnbThreads) {
      const float d = kdist[j];
      const uint32_t id = kid[j];
      const bool after = t == 0 || d > pd || (d == pd && id > pi);
      if (after && (d < bd || (d == bd && id < bi))) { bd = d; bi = id; bj = j; }
    }
    float wd = bd;
    uint32_t wi = bi;
    wave_min2(wd, wi);   // lanes without a candidate hold (inf, ~0): never below a real one
    if (wd == bd && wi == bi) { s_seld[par][wave] = bd; s_seli[par][wave] = bi; s_selj[par][wave] = bj; }
    __syncthreads();
    bd = __builtin_inff(); bi = 0xffffffffu; bj = 0xffffffffu;
    for (uint32_t w = 0; w < kKnbThreads / 64; ++w) {
      const float d = s_seld[par][w];
      const uint32_t id = s_seli[par][w], j = s_selj[par][w];
      if (j != 0xffffffffu && (d < bd || (d == bd && id < bi))) { bd = d; bi = id; bj = j; }
    }
    if (bj == 0xffffffffu) {   // the known set is exhausted
      for (uint32_t u = t + tid; u < A.k; u += kKnbThreads) { oid[u] = -1; ost[u] = -1; }
      break;
    }
    if (tid == 0) { oid[t] = (int64_t)bi; ost[t] = (int64_t)kreach[bj]; }
    pd = bd; pi = bi;
  }
}

}  // namespace pm

namespace pmk {
uint32_t knn_batch_kcap(uint64_t parallel, uint64_t max_step, uint64_t m) {
  if (parallel == 0 || parallel > kKnbMaxBatch || m == 0 || m > kKnbMaxM || max_step > (1u << 16)) return 0;
  const uint64_t need = parallel * (1 + max_step * m);
  uint64_t kc = 4;
  while (kc < need) kc <<= 1;
  return kc > (1u << 16) ? 0u : (uint32_t)kc;
}
uint64_t knn_batch_lds(uint32_t kcap, uint32_t dim, uint32_t nb, uint32_t ns) {
  const uint64_t nb4 = ((uint64_t)nb + 3) & ~3ull, dim4 = ((uint64_t)dim + 3) & ~3ull, ns4 = ((uint64_t)ns + 3) & ~3ull;
  return (uint64_t)kcap * 36 + (2 * nb4 + dim4 + ns4) * 4;
}
bool knn_batch_ok(uint64_t dim, uint64_t m, uint64_t ns, uint64_t max_step, uint64_t parallel) {
  if (dim == 0 || dim > (1u << 20) || ns == 0 || ns > (1u << 20)) return false;
  if (m == 0 || m > kKnbMaxM || parallel == 0 || parallel * m > kKnbMaxBatch) return false;
  const uint32_t kcap = knn_batch_kcap(parallel, max_step, m);
  if (!kcap) return false;
  return knn_batch_lds(kcap, (uint32_t)dim, (uint32_t)(parallel * m), (uint32_t)ns) <= kKnbMaxLds;
}
void knn_batch(hipStream_t st, const KnbArgs& A) {
  if (!A.nq) return;
  const uint32_t lds = (uint32_t)knn_batch_lds(A.kcap, A.dim, A.parallel * A.m, A.ns);
  // (dynamic LDS above the default 64 KB limit of a launch)
  if (hipFuncSetAttribute((const void*)pm::k_knn_batch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kKnbMaxLds) !=
      hipSuccess)
    (void)hipGetLastError();
  hipLaunchKernelGGL(pm::k_knn_batch, dim3(A.nq), dim3(pm::kKnbThreads), lds, st, A);
}
}  // namespace pmk

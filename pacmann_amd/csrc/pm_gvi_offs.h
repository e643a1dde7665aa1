// pm_gvi_offs.h — the argument arithmetic of pm_graph_group_get_vertex_info
// (pm_group.cpp): the walk over the caller's offs[0 .. S], each session's slice
// of ids, and the id range check.  Plain C++ without HIP, so that a stand-alone
// host program can run it under the sanitizers (tests/host/gvi_offs_check.cpp).
#pragma once
#include <cstdint>

namespace pmgvi {
enum : int { OFFS_OK = 0, OFFS_DESCENDING = 1, OFFS_ID_RANGE = 2 };

struct Slice { uint64_t off, n; };   // session s's ids are ids[off .. off + n)

// Session s's slice.  offs has S + 1 entries.
inline Slice slice(const uint64_t* offs, uint32_t s) { return {offs[s], offs[s + 1] - offs[s]}; }

// offs must not descend (offs[0] may be > 0: the ids before it belong to no
// session).  *live: sessions with a non-empty slice, *max_n: the longest
// slice, *end: offs[S], one past the last id any session reads.  On
// OFFS_DESCENDING *bad is the first s with offs[s + 1] < offs[s].
inline int walk(const uint64_t* offs, uint32_t S, uint32_t* live, uint64_t* max_n, uint64_t* end, uint32_t* bad) {
  *live = 0; *max_n = 0; *end = offs[0]; *bad = 0;
  for (uint32_t s = 0; s < S; ++s) {
    if (offs[s + 1] < offs[s]) { *bad = s; return OFFS_DESCENDING; }
    const uint64_t n = offs[s + 1] - offs[s];
    *live += n != 0;
    if (n > *max_n) *max_n = n;
  }
  *end = offs[S];
  return OFFS_OK;
}

// Every id a session reads must be a vertex (< nvert).  On OFFS_ID_RANGE *bad_s
// and *bad_i name the first offender (session, index into ids).
inline int check_ids(const uint64_t* ids, const uint64_t* offs, uint32_t S, uint64_t nvert, uint32_t* bad_s,
                     uint64_t* bad_i) {
  for (uint32_t s = 0; s < S; ++s)
    for (uint64_t i = offs[s]; i < offs[s + 1]; ++i)
      if (ids[i] >= nvert) { *bad_s = s; *bad_i = i; return OFFS_ID_RANGE; }
  return OFFS_OK;
}

// The shared steps of one call: every session makes ONE SimpleBatchPianoPIR.Query
// of its whole slice (as pm_graph_get_vertex_info does), so a call has one
// shared step if any session's bucketing took the one-step path, else none.
inline uint32_t shared_steps(const char* fast, uint32_t S) {
  for (uint32_t s = 0; s < S; ++s)
    if (fast[s]) return 1;
  return 0;
}
}  // namespace pmgvi

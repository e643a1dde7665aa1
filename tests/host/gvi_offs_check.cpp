// gvi_offs_check.cpp — the argument arithmetic of pm_graph_group_get_vertex_info
// (pacmann_amd/csrc/pm_gvi_offs.h) as a stand-alone host program, to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_host_gvi_offs.py):
// the offs walk, the ragged slices, the id range check and the step count, over
// buffers allocated at their exact sizes so that a read past an end is caught.
#include "../../pacmann_amd/csrc/pm_gvi_offs.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#define EXPECT(x)                                                      \
  do {                                                                 \
    if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } \
  } while (0)

int main() {
  using namespace pmgvi;
  uint32_t live = 0, bad = 0, bad_s = 0;
  uint64_t max_n = 0, end = 0, bad_i = 0;
  {   // 0, 1, one batch, one batch + 1, three batches (m = 8)
    const uint64_t counts[5] = {0, 1, 8, 9, 24};
    std::unique_ptr<uint64_t[]> offs(new uint64_t[6]);
    offs[0] = 0;
    for (int s = 0; s < 5; ++s) offs[s + 1] = offs[s] + counts[s];
    EXPECT(walk(offs.get(), 5, &live, &max_n, &end, &bad) == OFFS_OK);
    EXPECT(live == 4 && max_n == 24 && end == 42);
    std::unique_ptr<uint64_t[]> ids(new uint64_t[end]);
    for (uint64_t i = 0; i < end; ++i) ids[i] = i * 47 % 2000;
    EXPECT(check_ids(ids.get(), offs.get(), 5, 2000, &bad_s, &bad_i) == OFFS_OK);
    uint64_t seen = 0;
    for (uint32_t s = 0; s < 5; ++s) {   // the slices tile [0, end) in order
      const Slice sl = slice(offs.get(), s);
      EXPECT(sl.off == seen && sl.n == counts[s]);
      for (uint64_t i = 0; i < sl.n; ++i) EXPECT(ids[sl.off + i] < 2000);
      seen += sl.n;
    }
    EXPECT(seen == end);
    ids[41] = 2000;   // the last id of the last session
    EXPECT(check_ids(ids.get(), offs.get(), 5, 2000, &bad_s, &bad_i) == OFFS_ID_RANGE && bad_s == 4 && bad_i == 41);
    ids[41] = 0; ids[8] = ~0ull;   // session 1's single id is ids[0]; ids[8] is session 2's last
    EXPECT(check_ids(ids.get(), offs.get(), 5, 2000, &bad_s, &bad_i) == OFFS_ID_RANGE && bad_s == 2 && bad_i == 8);
  }
  {   // all empty: no id is read (ids may be NULL)
    const uint64_t offs[4] = {7, 7, 7, 7};
    EXPECT(walk(offs, 3, &live, &max_n, &end, &bad) == OFFS_OK && live == 0 && max_n == 0 && end == 7);
    EXPECT(check_ids(nullptr, offs, 3, 10, &bad_s, &bad_i) == OFFS_OK);
  }
  {   // a first offset above zero: the ids before it belong to nobody and are not checked
    const uint64_t offs[3] = {2, 3, 5};
    const uint64_t ids[5] = {99, 99, 1, 2, 3};
    EXPECT(walk(offs, 2, &live, &max_n, &end, &bad) == OFFS_OK && live == 2 && max_n == 2 && end == 5);
    EXPECT(check_ids(ids, offs, 2, 10, &bad_s, &bad_i) == OFFS_OK);
    EXPECT(slice(offs, 0).off == 2 && slice(offs, 0).n == 1 && slice(offs, 1).off == 3 && slice(offs, 1).n == 2);
  }
  {   // descending, also by wrap-around sized values
    const uint64_t a[4] = {0, 4, 2, 9};
    EXPECT(walk(a, 3, &live, &max_n, &end, &bad) == OFFS_DESCENDING && bad == 1);
    const uint64_t b[3] = {~0ull, 0, 1};
    EXPECT(walk(b, 2, &live, &max_n, &end, &bad) == OFFS_DESCENDING && bad == 0);
    const uint64_t c[2] = {0, ~0ull};   // one huge slice is not descending; the id check is what bounds a caller
    EXPECT(walk(c, 1, &live, &max_n, &end, &bad) == OFFS_OK && max_n == ~0ull);
  }
  {   // the step count: one shared step if any session took the one-step path
    std::vector<char> fast{0, 0, 0};
    EXPECT(shared_steps(fast.data(), 3) == 0);
    fast[2] = 1;
    EXPECT(shared_steps(fast.data(), 3) == 1);
    fast[0] = 1;
    EXPECT(shared_steps(fast.data(), 3) == 1);
    EXPECT(shared_steps(nullptr, 0) == 0);
  }
  std::printf("gvi_offs_check: ok\n");
  return 0;
}

// pm_stream.hip — gfx950 kernels of the streamed hint preprocessing
// (pm_batchpir_prep_stream_*): PianoPIRClient.UpdatePreprocessing
// (pir.go:303-352) of a window of whole chunks whose rows were just uploaded,
// for a client that keeps no DB.  The window is the only row source: row i of
// it is partition row c0 * CS + i, and nothing at or past `nrows` is read.
#include "pm_internal.h"

namespace pm {

// The fold of one sub-window into every hint of one partition.  Lane = (hint h
// of the concatenated space [0, H): primaries then backups, 16-B or 8-B segment
// of the entry), as k_prep_fold: the hint's tag-major tiles (tabT, 8 chunks per
// 16-B load) give its offset in every chunk of the window, the selected window
// rows are XORed in registers, and the parity gets ONE read-modify-write per
// sub-window (it was zeroed when the stream began; words [E & ~3, E) stay
// zero, as xorSlices leaves them).
//
// The window is at most max(8 MiB, one chunk), so the gather is served by L2 /
// the Infinity Cache.  The traffic to mind is the parity's read-modify-write: 2 H
// DBEntryByteNum bytes per sub-window whatever the window holds.  At SIFT1M's
// partition (H ~ 23,000 hints of 640 B) that is ~30 MB per sub-window and ~5
// sub-windows, against 15 MB for the one write of the whole-DB fold; with
// single-chunk windows it would be 124 times 30 MB.  That is why the host cuts
// sub-windows by MiB and not by chunk.  A hint that selects nothing in the
// window (every chunk its own or past the staged rows) touches no parity.
template <int W>   // 64-bit words per lane segment: 2 (even E) or 1
__global__ void __launch_bounds__(kBlock) k_stream_fold(const PmPart* __restrict__ parts, uint32_t part,
                                                        const uint64_t* __restrict__ win, uint32_t c0, uint32_t nc,
                                                        uint32_t nrows, uint32_t E) {
  const PmPart& P = parts[part];
  const uint32_t NSEG = (E & ~3u) / W;   // > 0: E < 4 launches nothing
  const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t H = P.H;
  const uint32_t h = (uint32_t)(e / NSEG), seg = (uint32_t)(e % NSEG);
  if (h >= H) return;
  const uint64_t* base = win + (uint64_t)seg * W;
  const uint32_t CS = P.CS, c1 = c0 + nc;
  uint64_t a0 = 0, a1 = 0;
  for (uint32_t t = c0 >> 3; t <= (c1 - 1) >> 3; ++t) {   // tabT pads SetSize to whole tiles
    const uint4 t4 = *reinterpret_cast<const uint4*>(P.tabT + tabT_index(H, h, t * 8));
    const uint32_t tw[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const uint32_t c = t * 8 + u;
      const uint16_t v = (uint16_t)(tw[u >> 1] >> (16 * (u & 1)));
      const uint32_t r = (c - c0) * CS + v;   // row of the window
      if (c >= c0 && c < c1 && v != kSkip && r < nrows) {
        const uint64_t* p = base + (uint64_t)r * E;
        if (W == 2) {
          const uint4 x = *reinterpret_cast<const uint4*>(p);
          a0 ^= ((uint64_t)x.y << 32) | x.x;
          a1 ^= ((uint64_t)x.w << 32) | x.z;
        } else {
          a0 ^= *p;
        }
      }
    }
  }
  if ((a0 | a1) == 0) return;
  PM_G uint64_t* dst = P.parity + (uint64_t)h * E + (uint64_t)seg * W;
  dst[0] ^= a0;
  if (W == 2) dst[1] ^= a1;
}

// k_prep_repl restricted to the window's slots [c0 * Qpc, (c0 + nc) * Qpc), the
// window as source: the same hash4(seed, DOM_REPL, idx, epoch, slot) offsets,
// ridx written for every slot (chunks wholly past the partition's end too) and
// zero values for rows at or past nrows.
constexpr uint32_t kStreamReplRows = 32, kStreamReplIt = 8;   // 8 x 256 16-B pieces: 32 rows of 128 words per pass
template <int W>
__global__ void __launch_bounds__(kBlock) k_stream_repl(const PmPart* __restrict__ parts, uint32_t part,
                                                        const uint64_t* __restrict__ win, uint32_t c0, uint32_t nc,
                                                        uint32_t nrows, uint32_t E) {
  typedef uint64_t vec __attribute__((ext_vector_type(W)));
  __shared__ uint32_t rrow[kStreamReplRows];   // window row of each slot, ~0u past the staged rows
  const PmPart& P = parts[part];
  const uint32_t s_end = (c0 + nc) * P.Qpc;
  const uint32_t s0 = c0 * P.Qpc + blockIdx.x * kStreamReplRows;
  if (s0 >= s_end) return;   // block-uniform
  const uint32_t ns = min(kStreamReplRows, s_end - s0);
  if (threadIdx.x < ns) {
    const uint32_t slot = s0 + threadIdx.x, c = slot / P.Qpc;
    const uint32_t off = (uint32_t)(hash4(P.seed, DOM_REPL, P.idx, P.epoch, slot) & (P.CS - 1));
    P.ridx[slot] = c * P.CS + off;
    const uint32_t r = (c - c0) * P.CS + off;
    rrow[threadIdx.x] = r < nrows ? r : ~0u;
  }
  __syncthreads();
  const uint32_t nseg = E / W, tot = ns * nseg;
  PM_G uint64_t* const dst = P.rval + (uint64_t)s0 * E;
  for (uint32_t x0 = 0; x0 < tot; x0 += kStreamReplIt * kBlock) {
    vec v[kStreamReplIt];
    uint32_t at[kStreamReplIt];
#pragma unroll
    for (uint32_t u = 0; u < kStreamReplIt; ++u) {
      const uint32_t x = x0 + u * kBlock + threadIdx.x;
      at[u] = ~0u;
      v[u] = vec{};
      if (x < tot) {
        const uint32_t i = x / nseg, sg = x - i * nseg, r = rrow[i];
        at[u] = i * E + sg * W;
        if (r != ~0u) v[u] = *reinterpret_cast<const vec*>(win + (uint64_t)r * E + sg * W);
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < kStreamReplIt; ++u)
      if (at[u] != ~0u) *reinterpret_cast<PM_G vec*>(dst + at[u]) = v[u];
  }
}

}  // namespace pm

namespace pmk {
static inline unsigned cdiv(uint64_t a, uint64_t b) { return (unsigned)((a + b - 1) / b); }

void stream_fold(hipStream_t st, const PmPart* parts, uint32_t part, uint32_t H, const uint64_t* win, uint32_t c0,
                 uint32_t nc, uint32_t nrows, uint32_t E) {
  const uint32_t EX = E & ~3u;
  if (EX == 0 || nrows == 0) return;   // xorSlices folds nothing / no row to fold
  if (E % 2 == 0)
    hipLaunchKernelGGL(k_stream_fold<2>, dim3(cdiv((uint64_t)H * (EX / 2), kBlock)), dim3(kBlock), 0, st, parts, part, win,
                       c0, nc, nrows, E);
  else
    hipLaunchKernelGGL(k_stream_fold<1>, dim3(cdiv((uint64_t)H * EX, kBlock)), dim3(kBlock), 0, st, parts, part, win, c0,
                       nc, nrows, E);
}
void stream_repl(hipStream_t st, const PmPart* parts, uint32_t part, uint32_t Qpc, const uint64_t* win, uint32_t c0,
                 uint32_t nc, uint32_t nrows, uint32_t E) {
  const dim3 grid(cdiv((uint64_t)nc * Qpc, kStreamReplRows));
  if (E % 2 == 0)
    hipLaunchKernelGGL(k_stream_repl<2>, grid, dim3(kBlock), 0, st, parts, part, win, c0, nc, nrows, E);
  else
    hipLaunchKernelGGL(k_stream_repl<1>, grid, dim3(kBlock), 0, st, parts, part, win, c0, nc, nrows, E);
}
}  // namespace pmk

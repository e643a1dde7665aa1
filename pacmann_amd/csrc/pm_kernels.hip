// pm_kernels.hip — gfx950 kernels of the PianoPIR XOR fold / answer path and
// the graphann distance path.  See DESIGN.md §5 for the roofline of each.
#include <atomic>
#include "pm_aes.h"
#include "pm_aes_bs.h"
#include "pm_internal.h"

namespace pm {
#ifndef PM_PREP_NT
#define PM_PREP_NT 0   // the maintenance's bulk stores (tabT tiles, the CS-512 fold's parities) nontemporal
#endif


__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}
__device__ __forceinline__ uint4 xor4(uint4 a, uint4 b) {
  return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w);
}

// ---------------------------------------------------------------------------
// Client hint preprocessing (pir.go:267-352), split in two kernels:
//   prep_offsets: tab[c][h] = PRF(tag_h, c) & (CS-1) for every hint h and
//                 chunk c (HOT LOOP A/B's PRF), kSkip for a backup hint's own
//                 chunk (pir.go:332-334).  AES-bound.  The table stays resident
//                 and serves every online PRF (PmPart::tab).
//   prep_fold:    parity[h] = XOR_c chunk_c[off[c][h]]  (HOT LOOP A/B's
//                 EntryXor), one lane per (hint, 16-B segment), parity held in
//                 a register for the whole chunk sweep.  Gather-bound.
// ---------------------------------------------------------------------------
#ifndef PM_OFFS_CHUNKS
#define PM_OFFS_CHUNKS 8
#endif
constexpr int kOffsChunksPerBlock = PM_OFFS_CHUNKS;
constexpr int kOffsBlock = 1024;   // 64 KiB of replicated table per workgroup: 16 waves share it

// Initial PRF tables of every hint h < H (its tag is h) at 8 chunks per
// workgroup, written chunk-major (hint search) and hint-major (set
// expansion).  Bound by the AES: its VALU issue (238 per PRF) and its T-table
// lookups in LDS (114) are both 0.83-0.87 busy.  The hint-major stores
// are scattered 2-B writes (every lane on its own line, ~5x their bytes in
// HBM write traffic), yet staging them through LDS made the kernel 20-25 %
// slower (375 -> 450-470 us at SIFT1M shape), so they stay direct (without
// them the kernel is only 2 % faster).  1,024-thread workgroups share one 64 KiB
// table copy (the LDS init is 4 B per PRF, not 16) and keep 16 waves per CU
// for the lookups' latency: 0.370 -> 0.335 ms at SIFT1M shape.
#ifndef PM_OFFS_TILES
#define PM_OFFS_TILES 1   // 8-chunk tiles per workgroup sharing one 64 KiB table fill (2 and 4 measured no faster: 244 / 268 vs 240 us per client alone)
#endif
constexpr int kOffsTiles = PM_OFFS_TILES;

// a 2-B store at a wave-uniform row plus a lane's fixed 32-bit byte offset: the
// row is scalar arithmetic, the store's address one 64-bit VALU add
__device__ __forceinline__ void store16_row(PM_G uint16_t* row, uint32_t lane_bytes, uint32_t v) {
  *reinterpret_cast<PM_G uint16_t*>(reinterpret_cast<PM_G char*>(row) + lane_bytes) = (uint16_t)v;
}

// The tiles of one workgroup.  The kernel is bound by VALU issue (DESIGN.md
// §5.6), so everything that is not AES is decided outside the chunk loop: the
// AES form (R2: SetSize <= 256, pm_aes.h r2_hint) and the chunk-major table
// (TAB: only where the fold reads it) are template parameters, a lane's
// offsets into a cur row and a tab row are computed once and the rows advance
// in SGPRs, two chunks share one pack / mask / key step and one register (its
// halves are stored with global_store_short and _d16_hi), and a backup hint's
// own chunk is patched after the tile instead of being compared against every
// chunk.  SetSize is a multiple of 4 (part_params): a pair of chunks is whole.
template <bool R2, bool TAB>
__device__ __forceinline__ void prep_offsets_tiles(const PmPart& P, const AesLane& A,
                                                   const R1Uniform (&r1u)[kOffsTiles][kOffsChunksPerBlock],
                                                   const uint32_t (&r1u0)[kOffsTiles][kOffsChunksPerBlock],
                                                   uint32_t cb, uint32_t h) {
  const uint32_t H = P.H, SS = P.SS, PH = P.PH, K = P.curk;
  const uint32_t m = P.CS - 1, m2 = m | (m << 16);
  const uint32_t k2 = (P.rk[40] & 0xffffu) * 0x10001u;   // rk[40]'s low half in both halves
  const bool prim = h < PH;
  const uint32_t own = prim ? 0xffffffffu : (h - PH) / P.Qpc;
  const uint32_t lcur = cur_row_off(K, h) * 2, ltab = h * 2;   // bytes; H < 2^29 (engine_create)
  const uint64_t cur_group = (uint64_t)cur_blocks(PH) * K * 8;   // cur words per K chunks (cur_index)
  const R1Lane r1v = r1_lane(A, P.rk, h);   // initial tag of hint h is h
  R2Hint r2k{0, 0, 0, 0};
  if (R2) r2k = r2_hint(A, P.rk, r1u[0][0], r1v);
  for (int tl = 0; tl < kOffsTiles; ++tl) {
    const uint32_t c0 = cb + tl * kOffsChunksPerBlock;
    if (c0 >= SS) break;
    const uint32_t c1 = min(SS, c0 + kOffsChunksPerBlock);
    // chunk c0's cur row as (group, chunk in group); next_cur steps it without a division
    const uint32_t cq = K == 2 ? c0 >> 1 : K == 1 ? c0 : c0 / K;
    uint32_t cr = c0 - cq * K;
    uint64_t crow = cq * cur_group + cr * 8;
    auto next_cur = [&] {
      if (++cr == K) { cr = 0; crow += cur_group - (K - 1) * 8; }
      else crow += 8;
    };
    uint64_t trow = (uint64_t)c0 * H;   // chunk c0's tab row
    uint32_t w[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};   // chunks past SetSize: kSkip padding
    uint32_t u0[kOffsChunksPerBlock];   // R2: the tile's round-1 words, two 16-B LDS reads
#pragma unroll
    for (int i = 0; i < kOffsChunksPerBlock; ++i) u0[i] = R2 ? r1u0[tl][i] : 0u;
#pragma unroll
    for (int p = 0; p < 4; ++p) {   // chunks c, c + 1: word p of the tile
      const uint32_t c = c0 + 2 * p;
      if (c >= c1) break;   // block-uniform, like everything about c below
      const Lo16Words a = R2 ? prf_lo16_r2(A, P.rk, u0[2 * p], r1v, r2k) : prf_lo16_split(A, P.rk, r1u[tl][2 * p], r1v);
      const Lo16Words b = R2 ? prf_lo16_r2(A, P.rk, u0[2 * p + 1], r1v, r2k) : prf_lo16_split(A, P.rk, r1u[tl][2 * p + 1], r1v);
      const uint32_t kx = k2 ^ (c | ((c + 1) << 16));   // rk[40] ^ x of both chunks: a scalar
      const uint32_t v = lo16_pair(a, b, kx) & m2;
      w[p] = v;
      if (TAB) {   // chunk-major (only the folds that stage it read it)
        store16_row(P.tab + trow, ltab, v);
        store16_row(P.tab + trow + H, ltab, v >> 16);
        trow += 2 * (uint64_t)H;
      }
      const uint64_t crow_a = crow;
      next_cur();
      const uint64_t crow_b = crow;
      next_cur();
      if (prim) {   // hint search (tags start at h)
        store16_row(P.cur + crow_a, lcur, v);
        store16_row(P.cur + crow_b, lcur, v >> 16);
      }
    }
    // a backup hint's own chunk (pir.go:332-334), if it is one of this tile's: kSkip
    const uint32_t j = own - c0;
    if (j < c1 - c0) {
      const uint32_t half = (j & 1) ? 0xffff0000u : 0x0000ffffu;
#pragma unroll
      for (uint32_t p = 0; p < 4; ++p) w[p] |= (j >> 1) == p ? half : 0u;
      if (TAB) P.tab[(uint64_t)own * H + h] = kSkip;   // after this lane's store of the PRF value above
    }
    // tag-major tile (set expansion): one 16-B store
    if (PM_PREP_NT) {
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      __builtin_nontemporal_store(u32x4{w[0], w[1], w[2], w[3]}, reinterpret_cast<u32x4*>(P.tabT + tabT_index(H, h, c0)));
    } else {
      *reinterpret_cast<uint4*>(P.tabT + tabT_index(H, h, c0)) = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}

__global__ void __launch_bounds__(kOffsBlock, 1) k_prep_offsets(const PmPart* __restrict__ parts) {
  __shared__ uint32_t te[kTeLdsWords];
  __shared__ R1Uniform r1u[kOffsTiles][kOffsChunksPerBlock];
  __shared__ __attribute__((aligned(16))) uint32_t r1u0[kOffsTiles][kOffsChunksPerBlock];   // their u0 words, side by side
  const PmPart& P = parts[blockIdx.z];
  const uint32_t H = P.H, SS = P.SS;
  const uint32_t cb = blockIdx.y * kOffsChunksPerBlock * kOffsTiles;
  if (blockIdx.x * kOffsBlock >= H || cb >= SS) return;   // block-uniform
  aes_lds_init<kOffsBlock>(te, g_aes.te0);
  __syncthreads();
  const AesLane A(te, threadIdx.x);
  const uint32_t cend = min(SS, cb + kOffsChunksPerBlock * kOffsTiles);
  // round 1's chunk-dependent half, once per chunk for the workgroup (pm_aes.h)
  if (threadIdx.x < cend - cb) {
    const R1Uniform u = r1_uniform(A, P.rk, cb + threadIdx.x);
    r1u[threadIdx.x / kOffsChunksPerBlock][threadIdx.x % kOffsChunksPerBlock] = u;
    r1u0[threadIdx.x / kOffsChunksPerBlock][threadIdx.x % kOffsChunksPerBlock] = u.u0;
  }
  __syncthreads();
  const uint32_t h = blockIdx.x * kOffsBlock + threadIdx.x;
  if (h >= H) return;
  static_assert(kOffsChunksPerBlock == 8, "one 16-B tabT tile of 8 chunks per thread");
  // SetSize <= 256: round 2's hint-only part once per hint (pm_aes.h r2_hint)
  if (SS <= 256) {
    if (P.tab) prep_offsets_tiles<true, true>(P, A, r1u, r1u0, cb, h);
    else prep_offsets_tiles<true, false>(P, A, r1u, r1u0, cb, h);
  } else {
    if (P.tab) prep_offsets_tiles<false, true>(P, A, r1u, r1u0, cb, h);
    else prep_offsets_tiles<false, false>(P, A, r1u, r1u0, cb, h);
  }
}

// Bitsliced form of k_prep_offsets (round 6, pm_aes_bs.h): the same tables
// (tabT, cur, tab) bit for bit, the AES on the VALU instead of LDS T-table
// lookups.  A lane owns 32 consecutive hints (one bitsliced block set) and one
// tile group of 8 chunks; it evaluates the chunks in pairs, transposes each
// pair's 2 x 16 output planes into 32 words (hint j: chunk c | chunk c+1 << 16,
// i.e. one 4-B word of the hint's tabT tile) and stores them.  LDS holds only
// the per-key setup (Te0 for rounds 1-2, the folded round constants, W's
// planes): 2.7 KB.
constexpr int kBsThreads = 256;
#ifndef PM_BS_WAVES
#define PM_BS_WAVES 2
#endif
__global__ void __launch_bounds__(kBsThreads, PM_BS_WAVES) k_prep_offsets_bs(const PmPart* __restrict__ parts) {
  __shared__ uint32_t bs_te0[256];
  __shared__ uint32_t bs_kx[32];
  __shared__ uint32_t bs_wv[32][4];
  __shared__ __attribute__((aligned(16))) uint32_t bs_wp[128];
  __shared__ __attribute__((aligned(16))) uint32_t bs_stash[16 * kBsThreads];
  const PmPart& P = parts[blockIdx.y];
  const uint32_t H = P.H, SS = P.SS, PH = P.PH;
  const uint32_t nm = (H + 31) / 32, ng = (SS + 7) / 8;
  if (blockIdx.x * kBsThreads >= nm * ng) return;   // block-uniform
  bs_te0[threadIdx.x] = g_aes.te0[threadIdx.x];
  __syncthreads();
  bs_setup_a(bs_te0, P.rk, bs_kx, bs_wv);
  __syncthreads();
  bs_setup_b(bs_wv, bs_wp);
  __syncthreads();
  const uint32_t task = blockIdx.x * kBsThreads + threadIdx.x;
  if (task >= nm * ng) return;
  const uint32_t m = task % nm, g = task / nm, h0 = 32 * m;
  const uint32_t nb = P.log2CS, Qpc = P.Qpc;
  const uint32_t keep = nb >= 16 ? 0xffffu : (1u << nb) - 1u;   // planes past log2(CS): masked off
  auto lowmask = [](int n) { return n <= 0 ? 0u : n >= 32 ? ~0u : (1u << n) - 1u; };
  // chunks in pairs: the first chunk's 16 planes wait in LDS (64 B per lane)
  // while the second is evaluated, so one copy of the AES code serves both and
  // no planes stay pinned in VGPRs across it
  uint4* stash = reinterpret_cast<uint4*>(bs_stash) + threadIdx.x;
#pragma unroll 1
  for (uint32_t q = 0; q < 8; ++q) {
    const uint32_t cc = 8 * g + q, c = cc & ~1u;
    uint32_t T[32];
    if (c < SS) {   // SetSize is a multiple of 4: a pair is whole
      uint32_t o[16];
      bs_prf16(bs_te0, P.rk, bs_kx, bs_wp, m, cc, o);
      // backup hints whose own chunk is cc (pir.go:332-334): kSkip (all 16 bits set)
      const int lo = (int)(PH + cc * Qpc) - (int)h0, hi = lo + (int)Qpc;
      const uint32_t own = lowmask(hi) & ~lowmask(lo);
#pragma unroll
      for (int b = 0; b < 16; ++b) o[b] = (((keep >> b) & 1u) ? o[b] : 0u) | own;
      if ((q & 1) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) stash[i * kBsThreads] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
        continue;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint4 v = stash[i * kBsThreads];
        T[4 * i] = v.x; T[4 * i + 1] = v.y; T[4 * i + 2] = v.z; T[4 * i + 3] = v.w;
      }
#pragma unroll
      for (int b = 0; b < 16; ++b) T[16 + b] = o[b];
      bs_transpose32(T);
    } else {
      if ((q & 1) == 0) continue;
#pragma unroll
      for (int j = 0; j < 32; ++j) T[j] = 0xffffffffu;   // tile padding past SetSize
    }
    // tag-major tiles: word (c & 7) / 2 of hint h0 + j's tile
    uint32_t* tt = reinterpret_cast<uint32_t*>(P.tabT + tabT_index(H, h0, c));
    if (h0 + 32 <= H) {
#pragma unroll
      for (int j = 0; j < 32; ++j) tt[4 * j] = T[j];
    } else {
#pragma unroll
      for (int j = 0; j < 32; ++j)
        if (h0 + j < H) tt[4 * j] = T[j];
    }
    if (c >= SS) continue;
    // 8-hint blocks of chunks c and c + 1 (cur: primary hints only; tab: every tag)
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      const uint32_t hb = h0 + 8 * jb;
      uint4 wlo, whi;
      wlo.x = __builtin_amdgcn_perm(T[8 * jb + 1], T[8 * jb + 0], 0x05040100u);
      wlo.y = __builtin_amdgcn_perm(T[8 * jb + 3], T[8 * jb + 2], 0x05040100u);
      wlo.z = __builtin_amdgcn_perm(T[8 * jb + 5], T[8 * jb + 4], 0x05040100u);
      wlo.w = __builtin_amdgcn_perm(T[8 * jb + 7], T[8 * jb + 6], 0x05040100u);
      whi.x = __builtin_amdgcn_perm(T[8 * jb + 1], T[8 * jb + 0], 0x07060302u);
      whi.y = __builtin_amdgcn_perm(T[8 * jb + 3], T[8 * jb + 2], 0x07060302u);
      whi.z = __builtin_amdgcn_perm(T[8 * jb + 5], T[8 * jb + 4], 0x07060302u);
      whi.w = __builtin_amdgcn_perm(T[8 * jb + 7], T[8 * jb + 6], 0x07060302u);
      if (hb < PH) {
        *reinterpret_cast<uint4*>(P.cur + cur_index(PH, P.curk, c, hb)) = wlo;
        *reinterpret_cast<uint4*>(P.cur + cur_index(PH, P.curk, c + 1, hb)) = whi;
      }
      if (P.tab && hb < H) {
        *reinterpret_cast<uint4*>(P.tab + (uint64_t)c * H + hb) = wlo;
        *reinterpret_cast<uint4*>(P.tab + (uint64_t)(c + 1) * H + hb) = whi;
      }
    }
  }
}

#ifndef PM_FOLD_NT
#define PM_FOLD_NT 1   // k_prep_fold's (BIGANN's gather fold) row loads nontemporal: 221-222 -> 210-212 ms per
                       // 100M client = 0.83 of HBM peak (profiles/r05/ab/fold_nt_100m)
#endif
template <int W>   // 64-bit words per lane segment: 2 (16-B loads) or 1
__global__ void __launch_bounds__(kBlock) k_prep_fold(const PmPart* __restrict__ parts,
                                                      const uint64_t* __restrict__ db, uint32_t E) {
  const PmPart& P = parts[blockIdx.y];
  const uint32_t EX = E & ~3u, NSEG = EX / W;
  const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t H = P.H;
  if (NSEG == 0) {   // xorSlices does nothing: every parity word stays zero
    if (e < (uint64_t)H * E) P.parity[e] = 0;
    return;
  }
  const uint32_t h = (uint32_t)(e / NSEG), seg = (uint32_t)(e % NSEG);
  if (h >= H) return;
  const uint64_t* base = db + (P.row0 * E) + (uint64_t)seg * W;
  const uint32_t CS = P.CS, SS = P.SS;
  const uint64_t N = P.N;
  uint64_t a0 = 0, a1 = 0;
  uint32_t c = 0;
  for (; c + 4 <= SS; c += 4) {   // chunks c .. c+3 of hint h: 8 B of its tag-major tile (tabT)
    const uint64_t t4 = *reinterpret_cast<const uint64_t*>(P.tabT + tabT_index(H, h, c));
    uint16_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = (uint16_t)(t4 >> (16 * u));
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint64_t r = (uint64_t)(c + u) * CS + v[u];
      if (v[u] != kSkip && r < N) {
        const uint64_t* p = base + r * E;
        if (W == 2) {
          typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
          const u32x4 x = PM_FOLD_NT ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p))
                                     : *reinterpret_cast<const u32x4*>(p);
          a0 ^= ((uint64_t)x.y << 32) | x.x;
          a1 ^= ((uint64_t)x.w << 32) | x.z;
        } else {
          a0 ^= PM_FOLD_NT ? __builtin_nontemporal_load(p) : *p;
        }
      }
    }
  }
  for (; c < SS; ++c) {
    uint16_t v = P.tabT[tabT_index(H, h, c)];
    const uint64_t r = (uint64_t)c * CS + v;
    if (v != kSkip && r < N) {
      const uint64_t* p = base + r * E;
      a0 ^= p[0];
      if (W == 2) a1 ^= p[1];
    }
  }
  uint64_t* dst = P.parity + (uint64_t)h * E + (uint64_t)seg * W;
  dst[0] = a0;
  if (W == 2) dst[1] = a1;
  if (seg == 0)
    for (uint32_t w = EX; w < E; ++w) P.parity[(uint64_t)h * E + w] = 0;
}

// Cache-blocked fold (same result as k_prep_fold): a workgroup owns one
// partition, one SW-word column slice of every entry and one group of hints.
// For each chunk it stages the slice of all CS entries of the chunk into LDS
// with direct global->LDS loads (double-buffered, one barrier per chunk) and
// XORs the entry each of its hints selects into parity accumulators held in
// registers, so a DB byte is read from HBM once per hint group instead of once
// per hint that selects it.  Entry CS of a staged chunk is a zero row (kSkip
// selects it); rows past N are staged from a 16-byte zero source.
constexpr int kFoldThreads = 1024, kFoldHPT = 7;   // hints per thread: pipelined fold
constexpr int kFoldHPTBlk = 4;                      // hints per thread: double-buffered fold (up to 8-word slices)
constexpr uint32_t kFoldMaxItems = 4;   // 16-B staging items per thread per chunk
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void g_cvoid_t;

// LDS-DMA of 16 B per lane (global_load_lds_dwordx4: lane l's bytes land at
// m0 + 16 l) issued by inline asm.  With __builtin_amdgcn_global_load_lds the
// compiler counts the DMA as a pending write to all of LDS and puts an
// s_waitcnt vmcnt(0) before the next ds_read of ANY buffer: a double buffer's
// staging of block b + 1 then completes before the fold of block b reads its
// first byte (k_prep_fold_rot's loop was serialised that way).  Issued here,
// the DMA is invisible to the compiler's wait insertion, so the caller waits
// for it (s_waitcnt vmcnt) before the buffer it fills is read.  The compiler's
// own counted waits for other loads stay correct: an extra operation in flight
// only makes a counted wait stricter.
__device__ __forceinline__ void lds_dma16(const void* src, const void* lds_wave_base) {
  const uint32_t m = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void_t*)lds_wave_base);
  asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "{m0}"(m) : "memory");
}

template <int SW>   // 64-bit words per column slice: 8, 4 or 2
__global__ void __launch_bounds__(kFoldThreads) k_prep_fold_blk(const PmPart* __restrict__ parts,
                                                                const uint64_t* __restrict__ db,
                                                                const uint64_t* __restrict__ zero16,
                                                                uint32_t E, uint32_t w0) {
  extern __shared__ __attribute__((aligned(16))) uint64_t fold_lds[];   // [2][(CS+1)*SW]
  typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
  constexpr uint32_t IPE = SW / 2;   // 16-B items per entry slice
  const PmPart& P = parts[blockIdx.z];
  const uint32_t H = P.H, CS = P.CS, SS = P.SS, tid = threadIdx.x;
  const uint32_t ng = (H + kFoldThreads * kFoldHPTBlk - 1) / (kFoldThreads * kFoldHPTBlk);
  if (blockIdx.x >= ng) return;   // block-uniform
  const uint32_t hb = (H + ng - 1) / ng, h0 = blockIdx.x * hb, h1 = min(H, h0 + hb);
  const uint32_t w = w0 + blockIdx.y * SW;
  const uint64_t N = P.N;
  const PM_G uint64_t* base = (const PM_G uint64_t*)db + P.row0 * E + w;
  const PM_G uint16_t* tab = P.tab;
  const uint32_t rowWords = (CS + 1) * SW, items = CS * IPE;
  const uint32_t wave_item0 = tid & ~63u;
  uint32_t hk[kFoldHPTBlk];
  uint64_t acc[kFoldHPTBlk][SW];
#pragma unroll
  for (int k = 0; k < kFoldHPTBlk; ++k) {
    hk[k] = h0 + tid + k * kFoldThreads;
#pragma unroll
    for (int x = 0; x < SW; ++x) acc[k][x] = 0;
  }
  uint32_t v[kFoldHPTBlk], nv[kFoldHPTBlk];
  // item it of chunk c: entry it / IPE, 16-B piece it % IPE, LDS byte offset it * 16
  auto stage = [&](uint32_t c, uint32_t buf) {
    uint64_t* L = fold_lds + buf * rowWords;
#pragma unroll
    for (uint32_t i = 0; i < kFoldMaxItems; ++i) {
      const uint32_t it = tid + i * kFoldThreads;
      if (i * kFoldThreads + wave_item0 < items && it < items) {
        const uint64_t r = (uint64_t)c * CS + it / IPE;
        const PM_G uint64_t* src = r < N ? base + r * E + (it % IPE) * 2 : (const PM_G uint64_t*)zero16;
        __builtin_amdgcn_global_load_lds((g_cvoid_t*)src, (lds_void_t*)(L + (i * kFoldThreads + wave_item0) * 2),
                                         16, 0, 0);
      }
    }
  };
  auto load_tab = [&](uint32_t c, uint32_t* out) {
#pragma unroll
    for (int k = 0; k < kFoldHPTBlk; ++k) out[k] = hk[k] < h1 ? tab[(uint64_t)c * H + hk[k]] : kSkip;
  };
  stage(0, 0);
  load_tab(0, v);
  for (uint32_t x = tid; x < 2 * SW; x += kFoldThreads) fold_lds[(x / SW) * rowWords + CS * SW + x % SW] = 0;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (uint32_t c = 0; c < SS; ++c) {
    const bool more = c + 1 < SS;
    if (more) { stage(c + 1, (c + 1) & 1); load_tab(c + 1, nv); }
    const uint64_t* L = fold_lds + (c & 1) * rowWords;
#pragma unroll
    for (int k = 0; k < kFoldHPTBlk; ++k) {
      const uint32_t o = v[k] == kSkip ? CS : v[k];
      const uint64_t* row = L + o * SW;
#pragma unroll
      for (int x = 0; x < SW; x += 2) {
        const u64x2 y = *reinterpret_cast<const u64x2*>(row + x);
        acc[k][x] ^= y.x;
        acc[k][x + 1] ^= y.y;
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kFoldHPTBlk; ++k) v[k] = nv[k];
  }
#pragma unroll
  for (int k = 0; k < kFoldHPTBlk; ++k) {
    if (hk[k] >= h1) continue;
    PM_G uint64_t* dst = P.parity + (uint64_t)hk[k] * E + w;
#pragma unroll
    for (int x = 0; x < SW; x += 2) *reinterpret_cast<PM_G u64x2*>(dst + x) = u64x2{acc[k][x], acc[k][x + 1]};
    if (w == 0)   // xorSlices leaves the words past len&~3 zero
      for (uint32_t t = E & ~3u; t < E; ++t) P.parity[(uint64_t)hk[k] * E + t] = 0;
  }
}

// Pipelined form of k_prep_fold_blk for CS * SW == 2048 * G (every
// partition): three LDS buffers, two chunks in flight, and the PRF-table row
// of the chunk staged through LDS too, so every load of the loop is a direct
// global->LDS load and the waits are counted per wave (G or G+1 loads per
// chunk), never vmcnt(0).  One extern __shared__ array; raw s_barrier.
constexpr uint32_t kPipeTabWords = kFoldThreads * kFoldHPT / 4;   // the group's table row: one u16 per hint

// s_waitcnt vmcnt(n) for a runtime n, n <= 15.  n must be wave-uniform, and is
// made visibly so: s_waitcnt is a scalar instruction, and in a switch lowered
// as divergent (exec-masked) branches every case's wait would execute.
__device__ __forceinline__ void wait_vmcnt(uint32_t n) {
  switch (__builtin_amdgcn_readfirstlane(n)) {
#define PM_VMC(i) case i: asm volatile("s_waitcnt vmcnt(" #i ")" ::: "memory"); break;
    PM_VMC(1) PM_VMC(2) PM_VMC(3) PM_VMC(4) PM_VMC(5) PM_VMC(6) PM_VMC(7) PM_VMC(8)
    PM_VMC(9) PM_VMC(10) PM_VMC(11) PM_VMC(12) PM_VMC(13) PM_VMC(14) PM_VMC(15)
#undef PM_VMC
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}

// G = 16-B staging loads per thread per chunk; NB LDS buffers; D chunks folded
// between two workgroup barriers
template <int SW, int G, int NB, int D = 1>
__global__ void __launch_bounds__(kFoldThreads) k_prep_fold_pipe(const PmPart* __restrict__ parts,
                                                                 const uint64_t* __restrict__ db,
                                                                 const uint64_t* __restrict__ zero16,
                                                                 uint32_t E, uint32_t ngmax, uint32_t nsl,
                                                                 uint32_t npg, uint32_t K) {
  extern __shared__ __attribute__((aligned(16))) uint64_t fold_lds[];   // [NB][(CS+1)*SW + 1024]
  typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
  constexpr uint32_t IPE = SW / 2, CS = G * kFoldThreads / IPE;
  // XCD-aware order (workgroups b and b + 8 share an XCD, MI355X_MICROARCH.md
  // § Workgroup dispatch).  parts holds K clients of each partition, partition-
  // major; pg = (partition, hint group) runs on XCD pg % 8.  There, for each
  // group of LW column slices that split one 128-B line of every row, the
  // workgroups of all K clients follow each other, so the lines they stage are
  // fetched into that XCD's L2 once for K x LW workgroups instead of once per
  // client (the same DB, read by every client's fold).
  constexpr uint32_t LW = 16 / SW;   // slices per 128-B line
  const uint32_t ngl = (nsl + LW - 1) / LW, per_pg = K * ngl * LW;
  const uint32_t xcd = blockIdx.x % 8, k = blockIdx.x / 8;
  const uint32_t pg = xcd + 8 * (k / per_pg), r = k % per_pg;
  const uint32_t client = (r / LW) % K, slice = (r / (K * LW)) * LW + r % LW;
  if (pg >= npg || slice >= nsl) return;   // block-uniform
  const PmPart& P = parts[(pg / ngmax) * K + client];
  const uint32_t H = P.H, SS = P.SS, tid = threadIdx.x;
  const uint32_t ng = (H + kFoldThreads * kFoldHPT - 1) / (kFoldThreads * kFoldHPT);
  const uint32_t grp = pg % ngmax;
  if (grp >= ng) return;   // block-uniform
  const uint32_t hb = (((H + ng - 1) / ng) + 7) & ~7u, h0 = grp * hb, h1 = min(H, h0 + hb);
  const uint32_t w = slice * SW;
  const uint64_t N = P.N;
  const PM_G uint64_t* base = (const PM_G uint64_t*)db + P.row0 * E + w;
  const PM_G uint16_t* tab = P.tab;
  constexpr uint32_t TABW = (CS + 1) * SW, BUFW = TABW + kPipeTabWords;
  const uint32_t wave_item0 = tid & ~63u;
  const bool tab_wave = tid < kPipeTabWords / 2;   // these waves stage the table row (8 entries per lane)
  uint32_t hk[kFoldHPT];
  uint64_t acc[kFoldHPT][SW];
#pragma unroll
  for (int k = 0; k < kFoldHPT; ++k) {
    hk[k] = h0 + tid + k * kFoldThreads;
#pragma unroll
    for (int x = 0; x < SW; ++x) acc[k][x] = 0;
  }
  auto stage = [&](uint32_t c, uint32_t buf) {
    uint64_t* L = fold_lds + buf * BUFW;
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)G; ++i) {
      const uint32_t it = tid + i * kFoldThreads;
      const uint64_t r = (uint64_t)c * CS + it / IPE;
      const PM_G uint64_t* src = r < N ? base + r * E + (it % IPE) * 2 : (const PM_G uint64_t*)zero16;
      __builtin_amdgcn_global_load_lds((g_cvoid_t*)src, (lds_void_t*)(L + (i * kFoldThreads + wave_item0) * 2),
                                       16, 0, 0);
    }
    if (tab_wave) {   // 8 table entries (16 B) per lane; h0 and H are multiples of 8
      const uint32_t hh = h0 + tid * 8;
      const PM_G uint64_t* src = hh < h1 ? (const PM_G uint64_t*)(tab + (uint64_t)c * H + hh)
                                         : (const PM_G uint64_t*)zero16;
      __builtin_amdgcn_global_load_lds((g_cvoid_t*)src, (lds_void_t*)(L + TABW + wave_item0 * 2), 16, 0, 0);
    }
  };
  for (uint32_t x = tid; x < NB * SW; x += kFoldThreads) fold_lds[(x / SW) * BUFW + CS * SW + x % SW] = 0;
  // chunks 0 .. NB-D-1 in flight; chunks c+NB-D .. c+NB-1 are issued while
  // chunks c .. c+D-1 are folded
  static_assert(NB > D, "fold pipeline: more buffers than chunks per barrier");
  for (uint32_t c = 0; c + D < (uint32_t)NB && c < SS; ++c) stage(c, c);
  const uint32_t ops = G + (tab_wave ? 1 : 0);   // loads per chunk of this wave
  auto wait_chunks = [&](uint32_t next, uint32_t issued) {   // chunks next .. next+D-1 landed
    const uint32_t need = min(SS, next + D);
    wait_vmcnt(issued > need ? (issued - need) * ops : 0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };
  wait_chunks(0, min(SS, (uint32_t)(NB - D)));
  // LDS banking: a ds_read_b128 is served in 16-lane groups, and a SW = 4 row
  // (32 B) starts on one of 8 of the 16 16-B slots of the 256-B bank row, so 16
  // random rows pile up ~4.4-deep on 8 slots.  Odd lanes read the row's halves
  // in the other order (their accumulator holds words 2-3 first): each group's
  // 8 even and 8 odd lanes then fall on disjoint slot sets (~3.1-deep).
  const uint32_t fl = SW == 4 ? ((tid & 1u) << 1) : 0u;
  for (uint32_t c0 = 0; c0 < SS; c0 += D) {
#pragma unroll
    for (int j = 0; j < D; ++j)
      if (c0 + NB - D + j < SS) stage(c0 + NB - D + j, (c0 + NB - D + j) % NB);
#pragma unroll
    for (int j = 0; j < D; ++j) {
    const uint32_t c = c0 + j;
    if (D > 1 && c >= SS) break;
    const uint64_t* L = fold_lds + (c % NB) * BUFW;
    const uint16_t* T = reinterpret_cast<const uint16_t*>(L + TABW);
#pragma unroll
    for (int k = 0; k < kFoldHPT; ++k) {
      const uint32_t t = hk[k] < h1 ? T[hk[k] - h0] : kSkip;
      const uint64_t* row = L + (t == kSkip ? CS : t) * SW;
#pragma unroll
      for (int x = 0; x < SW; x += 2) {
        const u64x2 y = *reinterpret_cast<const u64x2*>(row + (x ^ fl));
        acc[k][x] ^= y.x;
        acc[k][x + 1] ^= y.y;
      }
    }
    }
    if (c0 + D < SS) wait_chunks(c0 + D, min(SS, c0 + NB));
  }
#pragma unroll
  for (int k = 0; k < kFoldHPT; ++k) {
    if (hk[k] >= h1) continue;
    PM_G uint64_t* dst = P.parity + (uint64_t)hk[k] * E + w;
#pragma unroll
    for (int x = 0; x < SW; x += 2)
      *reinterpret_cast<PM_G u64x2*>(dst + (x ^ fl)) = u64x2{acc[k][x], acc[k][x + 1]};
    if (w == 0)   // xorSlices leaves the words past len&~3 zero
      for (uint32_t t = E & ~3u; t < E; ++t) P.parity[(uint64_t)hk[k] * E + t] = 0;
  }
}

// Bank-rotated fold for CS = 512 (same result as k_prep_fold): a workgroup
// owns (partition, 32-B column slice, group of <= 5,120 hints), one hint per
// lane slot (5 per lane), and folds the slice of every chunk into its hints'
// parities, like k_prep_fold_pipe.  What differs is how a chunk reaches LDS
// and is read there.  k_prep_fold_pipe has each lane read its hint's 32-B row
// with ds_read_b128: random rows land on random bank slots, ~3 rows pile up
// per slot in a 16-lane group, and the LDS array bounds the fold.  Here four
// chunks are staged side by side: LDS line k (128 B) holds row k of chunks
// 4b..4b+3, one 32-B slot each.  Lane l reads chunk slot (s + phase) % 4 and
// there the 16-B halves f, then f ^ 1, of its row (s = l % 4, f = (l / 4) & 1):
// a 16-lane ds_read_b128 group holds each (slot, half) twice, whatever rows
// its hints select.  Accumulator t of a lane always holds the same word of
// its slice (XOR order does not matter) and is stored there at the end.
// The staged bytes come from the partition's fold image (PmPart::img: the
// same 64 KB LDS image per (slice, 4 chunks), contiguous, rows past N zero),
// a second, server-side copy of the DB laid out for this kernel (640 MB for
// SIFT1M: HBM capacity traded for whole-line sequential staging instead of
// 32-B pieces at 640-B stride).  Hint offsets come from the tag-major table
// (tabT: 8 chunks in 16 B per tag; hint h's initial tag is h).
// Two buffers of (CS + 1) lines (line CS is zero: kSkip), 128.3 KB.
// CS = 1,024 (MS-MARCO's 200K-row partitions): two chunks per block instead
// of four (64-B lines, the same 64 KB per block, nbuf = SS / 2), so the double
// buffer still fits (131.2 KB).  A 16-lane ds_read_b128 group then holds each
// (slot, half) four times and its lanes collide when their rows agree mod 4
// (about 2.6 instead of 2 LDS cycles per group for random rows).
// npk != 0 (CS 512 only, FOLD_ROT512P): the image is packed (k_fold_image).  Its
// first npk slices each hold the high halves of 16 coordinate words, whose low
// halves are zero in every row of the DB and so in every parity; the id slices
// follow.  The fold itself does not differ: a lane's 8 accumulators of a packed
// slice are 16 half-words, which the epilogue expands to 16 parity dwords (64 B).
// qf != 0 (CS 512 only, FOLD_ROT512Q): the image is bit-packed (fold_bits_*
// below, k_fold_image_bits).  The fold does not differ either; the epilogue
// takes the fields of a lane's 256 accumulated bits apart and stores each quad
// of four as four whole parity dwords.
//
// The bit-packed image.  A row's folded 32-bit words are taken four at a time
// (a quad: one aligned 16-B store of the parity): first n1 coordinate quads of
// w1-bit fields, then n2 quads of w2-bit fields for the words that follow (the
// neighbour ids).  A field is a selection of its word's bits, the others being
// the same in every row of the DB (k_row_bits_or), so the same in every XOR of
// rows:
//   w1 = 12  half-word bits 14 (exponent bit 7), 10 (exponent bit 3, which bits
//            4..6 copy) and 9..0; the sign and the low half are zero
//   w1 = 16  the high half-word (the fields of FOLD_ROT512P)
//   w2 = 20  bits 19..0 (ids below 2^20)      w2 = 32  the whole word
// A 32-B slice holds whole quads, so that every parity dword is written by one
// workgroup: 64 / w1 coordinate quads per slice from bit 0 up (quad i, field t
// at bit (4 i + t) w1), then one slice with the coordinate quads left over and
// as many of the others as still fit, then 64 / w2 of the others per slice.
// Those lie from bit 256 down (quad i, field t at bit 256 - 4 w2 (i + 1) + t
// w2): every field sits at a place known when the kernel is compiled, whatever
// the slice holds.  SIFT1M (12, 20): 6 slices of 20 coordinates, one of 8
// coordinates and 8 ids, two of 12 ids: 9 slices where FOLD_ROT512P has 12.
// qf = w1 | w2 << 8 | n1 << 16; n2 follows from the folded words.
struct FoldBits { uint32_t w1, n1, w2, n2; };
struct FoldBitsSlice { uint32_t q1, c1, q2, c2; };   // first quad and quads of each kind in a slice
__host__ __device__ inline FoldBits fold_bits_of(uint32_t qf, uint32_t E) {
  FoldBits f;
  f.w1 = qf & 0xffu; f.w2 = (qf >> 8) & 0xffu; f.n1 = qf >> 16;
  f.n2 = (E & ~3u) / 2 - f.n1;
  return f;
}
__host__ __device__ inline FoldBitsSlice fold_bits_slice(const FoldBits& f, uint32_t s) {
  const uint32_t per1 = 64 / f.w1, per2 = 64 / f.w2, nf1 = f.n1 / per1, r1 = f.n1 % per1;
  const uint32_t fit = r1 ? (64 - r1 * f.w1) / f.w2 : 0u, cm = fit < f.n2 ? fit : f.n2;   // the others beside the left-over coordinates
  FoldBitsSlice o;
  if (s < nf1) { o.q1 = s * per1; o.c1 = per1; o.q2 = 0; o.c2 = 0; return o; }
  if (r1 && s == nf1) { o.q1 = nf1 * per1; o.c1 = r1; o.q2 = 0; o.c2 = cm; return o; }
  o.q1 = f.n1; o.c1 = 0;
  o.q2 = cm + (s - nf1 - (r1 ? 1 : 0)) * per2;
  o.c2 = o.q2 >= f.n2 ? 0u : f.n2 - o.q2 < per2 ? f.n2 - o.q2 : per2;
  return o;
}
__host__ __device__ inline uint32_t fold_bits_nsl(const FoldBits& f) {
  const uint32_t per1 = 64 / f.w1, per2 = 64 / f.w2, nf1 = f.n1 / per1, r1 = f.n1 % per1;
  const uint32_t fit = r1 ? (64 - r1 * f.w1) / f.w2 : 0u, cm = fit < f.n2 ? fit : f.n2;
  return nf1 + (r1 ? 1 : 0) + (f.n2 - cm + per2 - 1) / per2;
}
template <int W> __host__ __device__ __forceinline__ uint32_t fold_field_pack(uint32_t x) {
  if constexpr (W == 12) return ((x >> 16) & 0x7ffu) | ((x >> 19) & 0x800u);
  else if constexpr (W == 16) return x >> 16;
  else if constexpr (W == 20) return x & 0xfffffu;
  else return x;
}
template <int W> __host__ __device__ __forceinline__ uint32_t fold_field_expand(uint32_t f) {
  if constexpr (W == 12) return ((f & 0x7ffu) | ((f & 0x400u) * 14u) | ((f & 0x800u) << 3)) << 16;
  else if constexpr (W == 16) return f << 16;
  else return f;
}
// field of W bits at bit p of a slice's eight dwords (p: a constant once the callers' loops are unrolled)
template <int W> __device__ __forceinline__ uint32_t fold_bits_get(const uint32_t (&d)[8], int p) {
  const int i = p >> 5, sh = p & 31;
  uint32_t v = d[i] >> sh;
  if (sh + W > 32) v |= d[i + 1] << (32 - sh);
  if constexpr (W < 32) v &= (1u << W) - 1u;
  return v;
}
template <int W> __device__ __forceinline__ void fold_bits_put(uint32_t (&d)[8], int p, uint32_t f) {
  const int i = p >> 5, sh = p & 31;
  d[i] |= f << sh;
  if (sh + W > 32) d[i + 1] |= f >> (32 - sh);
}
__host__ __device__ constexpr int fold_bits_pos1(int w1, int i, int t) { return (4 * i + t) * w1; }
__host__ __device__ constexpr int fold_bits_pos2(int w2, int i, int t) { return 256 - 4 * w2 * (i + 1) + t * w2; }
// the epilogue of a bit-packed slice: d, the slice's accumulated dwords in the image's order
template <int W1, int W2>
__device__ __forceinline__ void fold_bits_store(const uint32_t (&d)[8], const FoldBitsSlice& sl, uint32_t n1,
                                                PM_G uint32_t* par) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
  for (int i = 0; i < 64 / W1; ++i) {
    if ((uint32_t)i >= sl.c1) break;   // block-uniform
    u32x4 x;
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = fold_field_expand<W1>(fold_bits_get<W1>(d, fold_bits_pos1(W1, i, t)));
    PM_G u32x4* const dst = reinterpret_cast<PM_G u32x4*>(par + (sl.q1 + i) * 4);
    if (PM_PREP_NT) __builtin_nontemporal_store(x, dst);
    else *dst = x;
  }
#pragma unroll
  for (int i = 0; i < 64 / W2; ++i) {
    if ((uint32_t)i >= sl.c2) break;   // block-uniform
    u32x4 x;
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = fold_field_expand<W2>(fold_bits_get<W2>(d, fold_bits_pos2(W2, i, t)));
    PM_G u32x4* const dst = reinterpret_cast<PM_G u32x4*>(par + (n1 + sl.q2 + i) * 4);
    if (PM_PREP_NT) __builtin_nontemporal_store(x, dst);
    else *dst = x;
  }
}
#ifndef PM_ROT_HPL
#define PM_ROT_HPL 5
#endif
#ifndef PM_ROT_GB
#define PM_ROT_GB 4   // XCD tile: GB (partition, group) pairs x SB slices
#endif                // (64 clients, one box: 4 x 8 19.4 ms, 8 x 4 20.2, 16 x 2 +2 %)
#ifndef PM_ROT_SB
#define PM_ROT_SB 8
#endif
#ifndef PM_ROTQ_GB
#define PM_ROTQ_GB 4   // the bit-packed image's tile (SIFT1M's 9 slices in one slice block; 288 clients, one box:
#endif                // 4 x 9 51.6 ms, 4 x 8 51.8, 3 x 9 52.6, 6 x 5 52.8, 11 x 3 55.1; profiles/r14)
#ifndef PM_ROTQ_SB
#define PM_ROTQ_SB 9
#endif
#ifndef PM_ROT_HPL2
#define PM_ROT_HPL2 7   // hints per lane at CS 1,024 (2-B tiles; 128 VGPRs, no spills): 140 / 126 / 118 ms at 5 / 6 / 7
#endif
constexpr int kRotHPL = PM_ROT_HPL;   // hints per lane (SIFT1M's 12,512 hints: 3 groups of 4,171)
__host__ __device__ constexpr int rot_hpl(uint32_t cs) { return cs == 512 ? kRotHPL : PM_ROT_HPL2; }
constexpr uint32_t kRotBufBytes = 512 * 128;   // one image block per (slice, 4 chunks of 512 / 2 of 1,024 rows)
__host__ __device__ constexpr uint32_t rot_nch(uint32_t cs) { return cs == 512 ? 4 : 2; }   // chunks per block
template <int CS>
__global__ void __launch_bounds__(kFoldThreads) k_prep_fold_rot(const PmPart* __restrict__ parts, uint32_t E,
                                                                uint32_t nvg, uint32_t nsl, uint32_t npv,
                                                                uint32_t npk_arg, uint32_t K, uint32_t ngc,
                                                                uint32_t qf_arg, uint32_t GB, uint32_t SB) {
  constexpr uint32_t NCH = rot_nch(CS), LINE = NCH * 8, BUFW = (CS + 1) * LINE;
  constexpr int HPL = rot_hpl(CS);
  static_assert(CS == 512 || CS == 1024, "4 chunks of 512 rows or 2 of 1,024 per block");
  static_assert(CS * LINE * 4 == kRotBufBytes, "64 KB blocks");
  // static (not extern) LDS: its address is a constant the reads fold into
  // their offsets
  __shared__ __attribute__((aligned(16))) uint32_t rot_lds[2 * BUFW];
  constexpr uint32_t ITEMS = CS * NCH * 2;   // 16-B staging items per buffer (NCH chunks x CS rows x 2)
  static_assert(ITEMS % kFoldThreads == 0, "whole staging items per thread");
  constexpr uint32_t G = ITEMS / kFoldThreads;
  // Virtual hint groups: the K clients' hint lists of a partition, concatenated
  // (client c's hint h is virtual hint c * H + h), cut into groups of HB =
  // 1,024 x HPL lane slots.  A group spans at most two clients (HB <= H),
  // and only the partition's last group has idle slots: 157 workgroups per
  // (partition, slice) for 64 SIFT1M clients instead of 3 per client (192),
  // each staging the slice's image once.  ngc != 0: partitions with fewer
  // than HB hints (small configs) keep ngc groups per client instead (no
  // mixing).
  constexpr uint32_t HB = kFoldThreads * HPL;
  const uint32_t npk = CS == 512 ? npk_arg : 0u;   // packed coordinate slices (nsl counts packed slices)
  const uint32_t qf = CS == 512 ? qf_arg : 0u;     // the bit-packed image's fields (nsl counts its slices; npk is 0)
  const uint32_t xcd = blockIdx.x % 8, kq = blockIdx.x / 8;
  // Order: tiles of GB consecutive (partition, group) pairs x SB consecutive slices
  // (GB and SB: kernel arguments, prep_fold chooses them by form), one tile per XCD at a time (GB * SB: about
  // its 32 CUs): a group's tabT rows are
  // read by SB workgroups and a slice's image blocks by GB workgroups out of
  // the XCD's L2.  The eight XCDs take eight consecutive pair blocks of the
  // SAME slice block, so the partition's image slices are shared through the
  // Infinity Cache; then the next slice block of the same pairs (their tabT
  // again, from the Infinity Cache).
  // Tile T = (its index on the XCD) * 8 + XCD; a last group of fewer than 8
  // pair blocks is dealt over the XCDs the same way (small launches, e.g. one
  // client's 48 pairs, keep every XCD busy).
  const uint32_t nsb = (nsl + SB - 1) / SB, ngb = (npv + GB - 1) / GB;
  const uint32_t T = (kq / (GB * SB)) * 8 + xcd, wt = kq % (GB * SB);
  if (T >= ngb * nsb) return;   // block-uniform
  const uint32_t gsup = T / (8 * nsb), m = min(8u, ngb - gsup * 8), r = T - gsup * 8 * nsb;
  const uint32_t pgv = (gsup * 8 + r % m) * GB + wt % GB;
  const uint32_t slice = (r / m) * SB + wt / GB;
  if (pgv >= npv || slice >= nsl) return;   // block-uniform
  const uint32_t part = pgv / nvg, vg = pgv % nvg;
  const PmPart& P = parts[part * K];   // H, SS and the fold image are the same for every client
  const uint32_t H = P.H, SS = P.SS, tid = threadIdx.x;
  const uint32_t vend = K * H;
  uint32_t v0, v1;
  if (ngc == 0) {
    v0 = vg * HB;
    if (v0 >= vend) return;   // block-uniform (a partition with fewer hints than maxH)
    v1 = min(v0 + HB, vend);
  } else {
    const uint32_t c = vg / ngc, g = vg % ngc;
    if (c >= K || g * HB >= H) return;   // block-uniform
    v0 = c * H + g * HB;
    v1 = min(v0 + HB, (c + 1) * H);
  }
  const uint32_t cA = v0 / H, cB = min(cA + 1, K - 1), vb = (cA + 1) * H;
  const PmPart& PA = parts[part * K + cA];
  const PmPart& PB = parts[part * K + cB];
  const PM_G uint16_t* const tabA = PA.tabT;
  const PM_G uint16_t* const tabB = PB.tabT;
  const uint32_t hA = cA * H;
  // first parity word of the slice: a packed slice covers two 32-B slices of the row
  const uint32_t w = slice < npk ? slice * 8 : (slice + npk) * 4;
  const uint32_t nbuf = SS / NCH;   // SetSize is a multiple of 4 (pir.go:497)
  const PM_G char* img = (const PM_G char*)P.img + (uint64_t)slice * nbuf * kRotBufBytes;
  // 16-B reads: lane l reads chunk slot (s + phase) % NCH, halves f then f ^ 1
  // (s = l % NCH, f = (l / NCH) & 1: every ds_read_b128 lane group of 16 holds
  // each (slot, half) 8 / NCH times, MI355X_MICROARCH.md §LDS)
  const uint32_t lane = tid & 63, j = (lane / NCH) & 1, ks = lane & (NCH - 1);
  const uint32_t vl = v0 + tid;   // virtual hint of lane slot k: vl + k * kFoldThreads
  uint32_t acc[HPL][8];
#pragma unroll
  for (int k = 0; k < HPL; ++k)
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[k][t] = 0;
  const uint32_t wave_item0 = tid & ~63u;
  auto stage = [&](uint32_t b, uint32_t buf) {   // one contiguous 64 KB block of the image
    uint32_t* L = rot_lds + buf * BUFW;
    const PM_G char* src = img + (uint64_t)b * kRotBufBytes;
#pragma unroll
    for (uint32_t i = 0; i < G; ++i)
      lds_dma16(src + (tid + i * kFoldThreads) * 16u, L + (i * kFoldThreads + wave_item0) * 4);
  };
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  using Tile = std::conditional_t<NCH == 4, u32x2, uint32_t>;   // the NCH 2-B offsets of a hint's block
  auto load_tab = [&](uint32_t b, Tile* out) {   // chunks NCH b .. of each hint: 2 NCH B of its tabT tile
#pragma unroll
    for (int k = 0; k < HPL; ++k) {
      const uint32_t v = min(vl + k * kFoldThreads, vend - 1);
      const bool inB = v >= vb;
      const PM_G char* src = (const PM_G char*)(inB ? tabB : tabA) + (uint32_t)tabT_index(H, v - (inB ? vb : hA), NCH * b) * 2u;
      out[k] = *reinterpret_cast<const PM_G Tile*>(src);
    }
  };
  for (uint32_t x = tid; x < 2 * LINE; x += kFoldThreads) rot_lds[(x / LINE) * BUFW + CS * LINE + x % LINE] = 0;
  Tile tv[HPL], tn[HPL];
  stage(0, 0);
  // lane slots past the group read the zero line (kSkip).  Applied when a tile
  // is taken into use, not at its load: a select on the loaded value right
  // after the load made every iteration wait for its prefetched staging and
  // tabT loads before folding the current buffer (the double buffer's
  // overlap lost)
  auto skip_idle = [&](Tile* t) {
#pragma unroll
    for (int k = 0; k < HPL; ++k)
      if (vl + k * kFoldThreads >= v1) t[k] = ~Tile{};
  };
  load_tab(0, tv);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  skip_idle(tv);
  const char* lds0 = reinterpret_cast<const char*>(rot_lds);
  for (uint32_t b = 0; b < nbuf; ++b) {
    if (b + 1 < nbuf) { stage(b + 1, (b + 1) & 1); load_tab(b + 1, tn); }
    const uint32_t lb = (b & 1) * BUFW * 4;   // byte offset of this buffer
    uint32_t cso[NCH], psel[NCH];
#pragma unroll
    for (uint32_t ph = 0; ph < NCH; ++ph) {
      const uint32_t sl = (ks + ph) & (NCH - 1);
      cso[ph] = lb + sl * 32 + 16 * j;
      psel[ph] = 0x0c0c0000u | ((2 * sl + 1) << 8) | (2 * sl);   // v_perm: tile word sl, zero-extended
    }
#pragma unroll
    for (int k = 0; k < HPL; ++k) {
#pragma unroll
      for (uint32_t p0 = 0; p0 < NCH; p0 += 2) {   // two phases' rows in flight (16 VGPRs), then their XOR
        uint32_t v[2][8];
#pragma unroll
        for (uint32_t pp = 0; pp < 2; ++pp) {
          const uint32_t ph = p0 + pp;
          uint32_t o;
          if constexpr (NCH == 4) o = __builtin_amdgcn_perm(tv[k].y, tv[k].x, psel[ph]);
          else o = __builtin_amdgcn_perm(0u, tv[k], psel[ph]);
          o = min(o, (uint32_t)CS);   // kSkip -> zero line
          const uint32_t a = o * (LINE * 4) + cso[ph];
          const uint4 x0 = *reinterpret_cast<const uint4*>(lds0 + a);
          const uint4 x1 = *reinterpret_cast<const uint4*>(lds0 + (a ^ 16u));
          v[pp][0] = x0.x; v[pp][1] = x0.y; v[pp][2] = x0.z; v[pp][3] = x0.w;
          v[pp][4] = x1.x; v[pp][5] = x1.y; v[pp][6] = x1.z; v[pp][7] = x1.w;
        }
#pragma unroll
        for (int t = 0; t < 8; ++t)   // v_bitop3_b32 0x96 = a ^ b ^ c (gfx950): two XORs per instruction
          acc[k][t] = xor3(acc[k][t], v[0][t], v[1][t]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int k = 0; k < HPL; ++k) tv[k] = tn[k];
    skip_idle(tv);
  }
#pragma unroll
  for (int k = 0; k < HPL; ++k) {
    const uint32_t v = vl + k * kFoldThreads;
    if (v >= v1) continue;
    const bool inB = v >= vb;
    PM_G uint64_t* const par = (inB ? PB.parity : PA.parity) + (uint64_t)(v - (inB ? vb : hA)) * E;
    PM_G uint32_t* dst = reinterpret_cast<PM_G uint32_t*>(par + w);
    if (qf) {   // block-uniform: the slice's 256 bits in the image's order, then field by field
      uint32_t d[8];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        d[t] = j ? acc[k][4 + t] : acc[k][t];
        d[4 + t] = j ? acc[k][t] : acc[k][4 + t];
      }
      const FoldBits fb = fold_bits_of(qf, E);
      const FoldBitsSlice sl = fold_bits_slice(fb, slice);
      PM_G uint32_t* const p32 = reinterpret_cast<PM_G uint32_t*>(par);
      if (fb.w1 == 12 && fb.w2 == 20) fold_bits_store<12, 20>(d, sl, fb.n1, p32);
      else if (fb.w1 == 16) fold_bits_store<16, 20>(d, sl, fb.n1, p32);
      else fold_bits_store<12, 32>(d, sl, fb.n1, p32);
    } else if (slice < npk) {   // block-uniform: half-word i of the slice is the high half of parity dword i
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
      for (int t = 0; t < 8; t += 2) {   // accumulators t, t + 1: dwords 2 p .. 2 p + 3 of the 16, p the word's place
        PM_G u32x4* const d = reinterpret_cast<PM_G u32x4*>(dst + 8 * (j ^ (t >> 2)) + 2 * (t & 3));
        const u32x4 x = {acc[k][t] << 16, acc[k][t] & 0xffff0000u, acc[k][t + 1] << 16, acc[k][t + 1] & 0xffff0000u};
        if (PM_PREP_NT) __builtin_nontemporal_store(x, d);
        else *d = x;
      }
    } else {
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        PM_G uint32_t* const d = dst + 4 * (j ^ (t >> 2)) + (t & 3);
        if (PM_PREP_NT) __builtin_nontemporal_store(acc[k][t], d);
        else *d = acc[k][t];
      }
    }
    if (slice == 0)   // xorSlices leaves the words past len&~3 zero
      for (uint32_t t = E & ~3u; t < E; ++t) par[t] = 0;
  }
}

// One partition's fold image: 16-B item it of block (slice s, chunks NCH b..)
// = line it / (2 NCH), chunk slot (it / 2) % NCH, half it % 2 of row
// (NCH b + slot) CS + line (NCH = rot_nch(CS); 4,096 items per block).
// npk != 0, the packed image of a DB whose coordinate words have zero low
// halves: slice s < npk holds, as 16 consecutive half-words, the high halves of
// the row's 32-bit words 16 s .. 16 s + 15 (an item: those of 8 words); slice
// s >= npk is the row's 32-B slice s + npk, whole.  fold_image_src is that map.
__host__ __device__ inline FoldImageSrc fold_image_src(uint64_t x, uint32_t nbuf, uint32_t CS, uint32_t npk) {
  const uint32_t lg = CS == 512 ? 2 : 1;   // log2 NCH
  const uint32_t it = (uint32_t)(x % (kRotBufBytes / 16));
  const uint64_t blk = x / (kRotBufBytes / 16);
  const uint32_t b = (uint32_t)(blk % nbuf), s = (uint32_t)(blk / nbuf);
  FoldImageSrc o;
  o.row = (uint64_t)((b << lg) + ((it >> 1) & ((1u << lg) - 1))) * CS + (it >> (lg + 1));
  o.packed = s < npk;
  o.word = o.packed ? 16 * s + 8 * (it & 1) : 8 * (s + npk) + 4 * (it & 1);
  return o;
}
__global__ void __launch_bounds__(kBlock) k_fold_image(uint4* __restrict__ img, const uint64_t* __restrict__ rows,
                                                      uint64_t N, uint32_t nbuf, uint32_t E, uint64_t nitems,
                                                      uint32_t CS, uint32_t npk) {
  for (uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x; x < nitems; x += (uint64_t)gridDim.x * kBlock) {
    const FoldImageSrc src = fold_image_src(x, nbuf, CS, npk);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (src.row < N) {
      const uint4* const p = reinterpret_cast<const uint4*>(reinterpret_cast<const uint32_t*>(rows + src.row * E) + src.word);
      v = p[0];
      if (src.packed) {
        const uint4 u = p[1];
        v = make_uint4((v.x >> 16) | (v.y & 0xffff0000u), (v.z >> 16) | (v.w & 0xffff0000u),
                       (u.x >> 16) | (u.y & 0xffff0000u), (u.z >> 16) | (u.w & 0xffff0000u));
      }
    }
    img[x] = v;
  }
}
// The bit-packed image (fold_bits_*): the same blocks, lines, chunk slots and
// halves; a thread packs its row's slice and keeps its item's half of it.
template <int W1, int W2>
__device__ __forceinline__ void fold_bits_pack(const uint32_t* __restrict__ row, const FoldBitsSlice& sl, uint32_t n1,
                                               uint32_t (&d)[8]) {
#pragma unroll
  for (int i = 0; i < 64 / W1; ++i) {
    if ((uint32_t)i >= sl.c1) break;
    const uint4 v = *reinterpret_cast<const uint4*>(row + (sl.q1 + i) * 4);
    const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) fold_bits_put<W1>(d, fold_bits_pos1(W1, i, t), fold_field_pack<W1>(x[t]));
  }
#pragma unroll
  for (int i = 0; i < 64 / W2; ++i) {
    if ((uint32_t)i >= sl.c2) break;
    const uint4 v = *reinterpret_cast<const uint4*>(row + (n1 + sl.q2 + i) * 4);
    const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) fold_bits_put<W2>(d, fold_bits_pos2(W2, i, t), fold_field_pack<W2>(x[t]));
  }
}
__global__ void __launch_bounds__(kBlock) k_fold_image_bits(uint4* __restrict__ img, const uint64_t* __restrict__ rows,
                                                           uint64_t N, uint32_t nbuf, uint32_t E, uint64_t nitems,
                                                           uint32_t qf) {
  const FoldBits fb = fold_bits_of(qf, E);
  for (uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x; x < nitems; x += (uint64_t)gridDim.x * kBlock) {
    const uint32_t it = (uint32_t)(x % (kRotBufBytes / 16));
    const uint64_t blk = x / (kRotBufBytes / 16);
    const uint32_t b = (uint32_t)(blk % nbuf), s = (uint32_t)(blk / nbuf);
    const uint64_t r = (uint64_t)(4 * b + ((it >> 1) & 3)) * 512 + (it >> 3);
    uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (r < N) {
      const uint32_t* const row = reinterpret_cast<const uint32_t*>(rows + r * E);
      const FoldBitsSlice sl = fold_bits_slice(fb, s);
      if (fb.w1 == 12 && fb.w2 == 20) fold_bits_pack<12, 20>(row, sl, fb.n1, d);
      else if (fb.w1 == 16) fold_bits_pack<16, 20>(row, sl, fb.n1, d);
      else fold_bits_pack<12, 32>(row, sl, fb.n1, d);
    }
    img[x] = (it & 1) ? make_uint4(d[4], d[5], d[6], d[7]) : make_uint4(d[0], d[1], d[2], d[3]);
  }
}
// The answer's packed row image (pmk::answer_pack_image): item x = 16-B segment
// x % nseg of row x / nseg.  The first cseg segments hold the high halves of
// eight coordinate words each (the packing of k_fold_image), the others four
// whole words from 32-bit word 8 cseg on.
__global__ void __launch_bounds__(kBlock) k_answer_pack_image(uint4* __restrict__ img, const uint64_t* __restrict__ rows,
                                                             uint64_t nitems, uint32_t E, uint32_t nseg, uint32_t cseg) {
  for (uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x; x < nitems; x += (uint64_t)gridDim.x * kBlock) {
    const uint64_t r = x / nseg;
    const uint32_t s = (uint32_t)(x - r * nseg);
    const uint32_t* const row = reinterpret_cast<const uint32_t*>(rows + r * E);
    uint4 v;
    if (s < cseg) {
      const uint4* const p = reinterpret_cast<const uint4*>(row + 8 * s);
      const uint4 a = p[0], u = p[1];
      v = make_uint4((a.x >> 16) | (a.y & 0xffff0000u), (a.z >> 16) | (a.w & 0xffff0000u),
                     (u.x >> 16) | (u.y & 0xffff0000u), (u.z >> 16) | (u.w & 0xffff0000u));
    } else {
      v = *reinterpret_cast<const uint4*>(row + 8 * cseg + 4 * (s - cseg));
    }
    img[x] = v;
  }
}
// One pass over the rows for the bits that the packed images leave out (32-bit
// words [0, dim) of every E-word row are coordinates, the others ids; dim % 4 ==
// 0, E even).  *out gets kRowLowHalf if a coordinate word has a non-zero low
// half, kRowCoordBits if one has its sign set or exponent bits 6..3 not all
// equal (an f32 holding 0..255 has neither: its exponent is 0 or 127..134), and
// kRowIdBits if another word has one of bits 31..20 set.
__device__ inline uint32_t coord_bits_or(uint32_t x) {
  const uint32_t e6 = x >> 29;
  return (x >> 31) | ((((e6 ^ (x >> 28)) | (e6 ^ (x >> 27)) | (e6 ^ (x >> 26))) & 1u));
}
__global__ void __launch_bounds__(kBlock) k_row_bits_or(const uint64_t* __restrict__ rows, uint64_t nrows, uint32_t E,
                                                       uint32_t dim, uint32_t* __restrict__ out) {
  const uint32_t per = E / 2;
  const uint64_t nitems = nrows * per;
  uint32_t low = 0, cb = 0, ib = 0;
  for (uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x; x < nitems; x += (uint64_t)gridDim.x * kBlock) {
    const uint64_t r = x / per;
    const uint32_t i = (uint32_t)(x - r * per);
    const uint4 v = reinterpret_cast<const uint4*>(rows + r * E)[i];
    if (4 * i < dim) {
      low |= v.x | v.y | v.z | v.w;
      cb |= coord_bits_or(v.x) | coord_bits_or(v.y) | coord_bits_or(v.z) | coord_bits_or(v.w);
    } else {
      ib |= v.x | v.y | v.z | v.w;
    }
  }
  const uint32_t f = ((low & 0xffffu) ? pmk::kRowLowHalf : 0u) | (cb ? pmk::kRowCoordBits : 0u) | ((ib >> 20) ? pmk::kRowIdBits : 0u);
  if (f) atomicOr(out, f);
}

// Replacement rows (pir.go:345-350): Qpc random offsets per chunk, idx + copy.
// One workgroup per kReplRows slots: their offsets are hashed once per row
// (not once per word) into LDS, then the rows are copied in 16-B pieces with
// every piece of a thread in flight together (32-bit index math throughout).
constexpr uint32_t kReplRows = 32, kReplIt = (kReplRows * 1024 / 16 + kBlock - 1) / kBlock;   // E <= 128 words
template <int W>
__global__ void __launch_bounds__(kBlock) k_prep_repl(const PmPart* __restrict__ parts,
                                                      const uint64_t* __restrict__ db, uint32_t E) {
  typedef uint64_t vec __attribute__((ext_vector_type(W)));
  __shared__ uint32_t rrow[kReplRows];   // partition row of each slot, ~0u past the partition's end
  const PmPart& P = parts[blockIdx.y];
  const uint32_t nslot = P.SS * P.Qpc;
  const uint32_t s0 = blockIdx.x * kReplRows;
  if (s0 >= nslot) return;   // block-uniform
  const uint32_t ns = min(kReplRows, nslot - s0);
  if (threadIdx.x < ns) {
    const uint32_t slot = s0 + threadIdx.x, c = slot / P.Qpc;
    const uint64_t off = hash4(P.seed, DOM_REPL, P.idx, P.epoch, slot) & (P.CS - 1);
    const uint64_t r = (uint64_t)c * P.CS + off;
    P.ridx[slot] = (uint32_t)r;
    rrow[threadIdx.x] = r < P.N ? (uint32_t)r : ~0u;
  }
  __syncthreads();
  const uint32_t nseg = E / W, tot = ns * nseg;
  const uint64_t* const src = db + P.row0 * E;
  uint64_t* const dst = P.rval + (uint64_t)s0 * E;
  for (uint32_t x0 = 0; x0 < tot; x0 += kReplIt * kBlock) {
    vec v[kReplIt];
    uint32_t at[kReplIt];
#pragma unroll
    for (uint32_t u = 0; u < kReplIt; ++u) {
      const uint32_t x = x0 + u * kBlock + threadIdx.x;
      at[u] = ~0u;
      v[u] = vec{};
      if (x < tot) {
        const uint32_t i = x / nseg, sg = x - i * nseg, r = rrow[i];
        at[u] = i * E + sg * W;
        if (r != ~0u) v[u] = *reinterpret_cast<const vec*>(src + (uint64_t)r * E + sg * W);
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < kReplIt; ++u)
      if (at[u] != ~0u) *reinterpret_cast<vec*>(dst + at[u]) = v[u];
  }
}

// Initialization (pir.go:203-255): tags 0..H-1, program points, histogram.
__global__ void __launch_bounds__(kBlock) k_prep_init(const PmPart* __restrict__ parts) {
  const PmPart& P = parts[blockIdx.y];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < P.H) P.tag[i] = i;
  if (i < P.PH) P.pp[i] = kDefaultProgramPoint;
  if (i < P.SS) P.hist[i] = 0;
  if (i < P.SS * P.Qpc) P.ridx[i] = kDefaultProgramPoint;
  if (i == 0) *P.fqn = 0;
}

// PianoPIRServer.PrivateQuery (pir.go:65-88) for nq client-supplied offset
// sets: XOR of SetSize gathered rows.  One workgroup per offset set: lanes =
// (row slice, 16-B segment); slices are XOR-combined through LDS.
template <int W>
__global__ void __launch_bounds__(kBlock) k_server_answer(const PmPart* __restrict__ parts,
                                                          const uint32_t* __restrict__ qoffs,
                                                          uint32_t maxSS,
                                                          const uint64_t* __restrict__ db, uint32_t E,
                                                          uint64_t* __restrict__ ans) {
  __shared__ uint64_t red[kBlock * 2];
  const uint32_t s = blockIdx.x;
  const PmPart& P = parts[0];
  const uint32_t EX = E & ~3u, NSEG = EX / W;
  const uint32_t* qo = qoffs + (uint64_t)s * maxSS;
  const uint64_t* base = db + P.row0 * E;
  uint64_t* out = ans + (uint64_t)s * E;
  for (uint32_t seg0 = 0; seg0 < NSEG; seg0 += kBlock) {
    const uint32_t nseg = min(NSEG - seg0, (uint32_t)kBlock);
    const uint32_t nsl = kBlock / nseg;
    const uint32_t sl = threadIdx.x / nseg, seg = seg0 + threadIdx.x % nseg;
    uint64_t a0 = 0, a1 = 0;
    if (sl < nsl) {
      for (uint32_t i = sl; i < P.SS; i += nsl) {
        const uint64_t r = (uint64_t)i * P.CS + qo[i];
        if (r < P.N) {
          const uint64_t* p = base + r * E + (uint64_t)seg * W;
          if (W == 2) {
            uint4 x = *reinterpret_cast<const uint4*>(p);
            a0 ^= ((uint64_t)x.y << 32) | x.x;
            a1 ^= ((uint64_t)x.w << 32) | x.z;
          } else {
            a0 ^= *p;
          }
        }
      }
    }
    red[threadIdx.x * 2] = a0;
    red[threadIdx.x * 2 + 1] = a1;
    __syncthreads();
    if (threadIdx.x < nseg) {
      uint64_t x0 = 0, x1 = 0;
      for (uint32_t k = 0; k < nsl; ++k) {
        x0 ^= red[(k * nseg + threadIdx.x) * 2];
        x1 ^= red[(k * nseg + threadIdx.x) * 2 + 1];
      }
      out[(uint64_t)seg * W] = x0;
      if (W == 2) out[(uint64_t)seg * W + 1] = x1;
    }
    __syncthreads();
  }
  for (uint32_t w = EX + threadIdx.x; w < E; w += kBlock) out[w] = 0;
}

// The same for a batch PIR's partitions (pm_batchpir_server_answer): set s is
// answered over partition qpart[s], whose DB-side parameters (PmSrvPart: no
// client state) it looks up itself, so one launch serves sets of partitions of
// different length.  One workgroup per set, lanes = (row slice, 16-B segment)
// as above, with kSrvFlight rows in flight per lane: a set is SetSize rows of
// one partition (245 of 640 B at SIFT1M), enough for 256 lanes, and a remote
// client's batch can be as small as one set per partition, which one wave per
// set would leave with a quarter of the loads in flight.
// rows / rw: the stored rows and their length in 64-bit words.  PK: the packed
// row image (k_answer_pack_image; NSEG segments per row, the first cseg of
// them eight coordinate high halves each, E % 4 == 0): the XOR of packed rows
// is the packed XOR since every dropped half is zero, and the reducing lane
// widens its segment back into the answer's words.
constexpr uint32_t kSrvFlight = 4;
template <int W, bool PK>
__global__ void __launch_bounds__(kBlock) k_server_answer_parts(const PmSrvPart* __restrict__ sp,
                                                                const uint32_t* __restrict__ qpart,
                                                                const uint32_t* __restrict__ qoffs, uint32_t stride,
                                                                const uint64_t* __restrict__ rows, uint32_t rw,
                                                                uint32_t NSEG, uint32_t cseg, uint32_t E,
                                                                uint64_t* __restrict__ ans) {
  static_assert(!PK || W == 2, "packed rows are whole 16-B segments");
  __shared__ uint64_t red[kBlock * 2];
  const uint32_t s = blockIdx.x;
  const PmSrvPart P = sp[qpart[s]];
  const uint32_t* qo = qoffs + (uint64_t)s * stride;
  const uint64_t* base = rows + P.row0 * rw;
  uint64_t* out = ans + (uint64_t)s * E;
  for (uint32_t seg0 = 0; seg0 < NSEG; seg0 += kBlock) {
    const uint32_t nseg = min(NSEG - seg0, (uint32_t)kBlock);
    const uint32_t nsl = kBlock / nseg;
    const uint32_t sl = threadIdx.x / nseg, seg = seg0 + threadIdx.x % nseg;
    uint64_t a0 = 0, a1 = 0;
    if (sl < nsl) {
      for (uint32_t i0 = sl; i0 < P.SS; i0 += kSrvFlight * nsl) {
        uint64_t x0[kSrvFlight], x1[kSrvFlight];
#pragma unroll
        for (uint32_t u = 0; u < kSrvFlight; ++u) {
          const uint32_t i = i0 + u * nsl;
          x0[u] = 0; x1[u] = 0;
          if (i >= P.SS) continue;
          const uint64_t r = (uint64_t)i * P.CS + qo[i];
          if (r >= P.N) continue;   // pir.go:75-77
          const uint64_t* p = base + r * rw + (uint64_t)seg * W;
          if (W == 2) {
            const uint4 x = *reinterpret_cast<const uint4*>(p);
            x0[u] = ((uint64_t)x.y << 32) | x.x;
            x1[u] = ((uint64_t)x.w << 32) | x.z;
          } else {
            x0[u] = *p;
          }
        }
#pragma unroll
        for (uint32_t u = 0; u < kSrvFlight; ++u) { a0 ^= x0[u]; a1 ^= x1[u]; }
      }
    }
    red[threadIdx.x * 2] = a0;
    red[threadIdx.x * 2 + 1] = a1;
    __syncthreads();
    if (threadIdx.x < nseg) {
      uint64_t x0 = 0, x1 = 0;
      for (uint32_t k = 0; k < nsl; ++k) {
        x0 ^= red[(k * nseg + threadIdx.x) * 2];
        x1 ^= red[(k * nseg + threadIdx.x) * 2 + 1];
      }
      if (PK && seg < cseg) {   // half-word pair k of the segment: the high halves of 32-bit words 8 seg + 2 k, + 1
        const uint32_t v[4] = {(uint32_t)x0, (uint32_t)(x0 >> 32), (uint32_t)x1, (uint32_t)(x1 >> 32)};
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
          out[4 * seg + k] = ((uint64_t)(v[k] & 0xffff0000u) << 32) | (uint64_t)(uint32_t)(v[k] << 16);
      } else if (PK) {
        out[4 * cseg + 2 * (seg - cseg)] = x0;
        out[4 * cseg + 2 * (seg - cseg) + 1] = x1;
      } else {
        out[(uint64_t)seg * W] = x0;
        if (W == 2) out[(uint64_t)seg * W + 1] = x1;
      }
    }
    __syncthreads();
  }
  for (uint32_t w = (E & ~3u) + threadIdx.x; w < E; w += kBlock) out[w] = 0;
}

// ---------------------------------------------------------------------------
// Distance kernels (graphann/l2_distance_amd64.s).
// ---------------------------------------------------------------------------
// L2Dist, bit-exact: lane k of an 8-lane group owns running sum s_k over
// elements 8t+k (VSUBPS/VMULPS/VADDPS, each rounded: no FMA), then the
// VHADDPS tree ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)) as xor-1/2/4 shuffles, then
// the scalar tail of build_graph.go:123-125 on lane 0.
// seglen > 0: rows [j*seglen, (j+1)*seglen) are scored against query j at
// q + j*dim (several clients' start sets in one launch, pm_search_loop_batched)
__global__ void __launch_bounds__(kBlock) k_l2_rows(const float* __restrict__ rows,
                                                    uint64_t stride, uint64_t nrows,
                                                    const uint32_t* __restrict__ ids,
                                                    const float* __restrict__ q, uint32_t dim,
                                                    float* __restrict__ out, uint64_t seglen) {
  const uint64_t g = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 3;
  const uint32_t k = threadIdx.x & 7;
  const bool live = g < nrows;
  const float* r = rows + (live ? (ids ? (uint64_t)ids[g] : g) : 0) * stride;
  if (seglen && live) q += (g / seglen) * dim;
  const uint32_t dimS = dim & ~7u;
  float acc = 0.0f;
  if (live)
    for (uint32_t t = k; t < dimS; t += 8) {
      const float d = __fsub_rn(r[t], q[t]);
      acc = __fadd_rn(acc, __fmul_rn(d, d));
    }
  acc = __fadd_rn(acc, __shfl_xor(acc, 1));
  acc = __fadd_rn(acc, __shfl_xor(acc, 2));
  acc = __fadd_rn(acc, __shfl_xor(acc, 4));
  if (live && k == 0) {
    float d = dimS ? acc : 0.0f;
    for (uint32_t i = dimS; i < dim; ++i) {
      const float t = __fsub_rn(r[i], q[i]);
      d = __fadd_rn(d, __fmul_rn(t, t));
    }
    out[g] = d;
  }
}

// InnerProduct per row (mod 2^32): 16 lanes per row, shuffle-reduced; the
// wrapping sum of all rows is atomically accumulated (order-independent).
__global__ void __launch_bounds__(kBlock) k_ip_rows(const uint32_t* __restrict__ rows, uint64_t nrows,
                                                    const uint32_t* __restrict__ q, uint32_t dim,
                                                    uint32_t* __restrict__ per_row,
                                                    uint32_t* __restrict__ sum) {
  const uint64_t g = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 4;
  const uint32_t l = threadIdx.x & 15;
  uint32_t acc = 0;
  if (g < nrows) {
    const uint32_t* r = rows + g * dim;
    for (uint32_t j = l; j < dim; j += 16) acc += r[j] * q[j];
  }
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) acc += __shfl_xor(acc, m);
  if (g < nrows && l == 0 && per_row) per_row[g] = acc;
  uint32_t w = (l == 0 && g < nrows) ? acc : 0;
#pragma unroll
  for (int m = 16; m < 64; m <<= 1) w += __shfl_xor(w, m);
  if ((threadIdx.x & 63) == 0) atomicAdd(sum, w);
}

// Streaming sum-only scan (the TestInnerProduct loop): 16-B loads, query
// element j = flat index mod dim from LDS, per-thread partial sums.
__global__ void __launch_bounds__(kBlock) k_ip_scan(const uint4* __restrict__ rows, uint64_t n4,
                                                    const uint32_t* __restrict__ q, uint32_t dim,
                                                    uint32_t* __restrict__ sum) {
  __shared__ uint32_t qs[4096];
  for (uint32_t j = threadIdx.x; j < dim; j += kBlock) qs[j] = q[j];
  __syncthreads();
  uint32_t acc = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  const uint32_t dim4 = dim / 4;
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const u32x4* r4 = reinterpret_cast<const u32x4*>(rows);
  uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (stride % dim4 == 0) {
    // the grid stride is whole rows: a thread's column (and query slice) is
    // fixed, and kU 16-B nontemporal loads are in flight per thread
    const uint32_t j = (uint32_t)(f % dim4) * 4;
    const uint32_t q0 = qs[j], q1 = qs[j + 1], q2 = qs[j + 2], q3 = qs[j + 3];
    constexpr int kU = 8;
    for (; f + (kU - 1) * stride < n4; f += kU * stride) {
      u32x4 t[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) t[u] = __builtin_nontemporal_load(r4 + f + u * stride);
#pragma unroll
      for (int u = 0; u < kU; ++u) acc += t[u].x * q0 + t[u].y * q1 + t[u].z * q2 + t[u].w * q3;
    }
    for (; f < n4; f += stride) {
      const u32x4 t = __builtin_nontemporal_load(r4 + f);
      acc += t.x * q0 + t.y * q1 + t.z * q2 + t.w * q3;
    }
  } else {
    for (; f < n4; f += stride) {
      const u32x4 t = __builtin_nontemporal_load(r4 + f);
      const uint32_t j = (uint32_t)(f % dim4) * 4;
      acc += t.x * qs[j] + t.y * qs[j + 1] + t.z * qs[j + 2] + t.w * qs[j + 3];
    }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m);
  if ((threadIdx.x & 63) == 0) atomicAdd(sum, acc);
}

__global__ void __launch_bounds__(kBlock) k_ip_fill(uint4* __restrict__ rows, uint64_t n4, uint32_t dim,
                                                    uint64_t r0) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x; f < n4; f += stride) {
    const uint64_t e = f * 4;
    const uint32_t i = (uint32_t)(r0 + e / dim), j = (uint32_t)(e % dim);   // global row (uint32 as in Go)
    rows[f] = make_uint4(i + j, i + j + 1, i + j + 2, i + j + 3);
  }
}

// Synthetic DB fill (BIGANN-scale benchmarks: the rows never cross PCIe).
// Grid-stride over the words of rows [r0, r0 + rows) of the global DB.
__global__ void __launch_bounds__(kBlock) k_db_synth(uint64_t* __restrict__ dst, uint64_t r0, uint64_t nw,
                                                     uint32_t E, uint64_t k) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock, x0 = r0 * E;
  for (uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x; f < nw; f += stride)
    __builtin_nontemporal_store(sm64(k ^ (x0 + f)), dst + f);
}

__global__ void __launch_bounds__(kBlock) k_prf_batch(const uint32_t* __restrict__ rk,
                                                      const uint64_t* __restrict__ tags,
                                                      const uint64_t* __restrict__ xs, uint64_t n,
                                                      uint64_t* __restrict__ out) {
  __shared__ uint32_t te[kTeLdsWords];
  __shared__ uint32_t srk[44];
  aes_lds_init<kBlock>(te, g_aes.te0);
  if (threadIdx.x < 44) srk[threadIdx.x] = rk[threadIdx.x];
  __syncthreads();
  const AesLane A(te, threadIdx.x);
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
    out[i] = prf64(A, srk, tags[i], xs[i]);
}

// Device-resident batch responses (pm_batchpir_query_dev): row i of out
// (E + 1 words) = the entry at src[i] (a row of a partition's localCache arena
// in HBM; the pointer list sits in pinned host memory) and the success flag,
// or zeros.  One workgroup per response; E <= 2048.
__global__ void __launch_bounds__(kBlock) k_gather_rows(const uint64_t* const* __restrict__ src, uint32_t E,
                                                         uint64_t* __restrict__ out) {
  const uint64_t i = blockIdx.x;
  const uint64_t* r = src[i];
  uint64_t* o = out + i * (E + 1);
  for (uint32_t w = threadIdx.x; w < E; w += kBlock) o[w] = r ? r[w] : 0;
  if (threadIdx.x == 0) o[E] = r ? 1 : 0;
}

}  // namespace pm

// ---------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------
namespace pmk {
static inline unsigned cdiv(uint64_t a, uint64_t b) { return (unsigned)((a + b - 1) / b); }

void prep_init(hipStream_t st, const PmPart* d, int np, uint32_t maxH, uint32_t maxRepl, uint32_t,
               bool) {
  const uint32_t n = maxH > maxRepl ? maxH : maxRepl;
  hipLaunchKernelGGL(k_prep_init, dim3(cdiv(n, kBlock), np), dim3(kBlock), 0, st, d);
}
void prep_offsets_tt(hipStream_t st, const PmPart* d, int np, uint32_t maxH, uint32_t maxSS) {
  hipLaunchKernelGGL(k_prep_offsets, dim3(cdiv(maxH, kOffsBlock), cdiv(maxSS, kOffsChunksPerBlock * kOffsTiles), np),
                     dim3(kOffsBlock), 0, st, d);
}
void prep_offsets_bs(hipStream_t st, const PmPart* d, int np, uint32_t maxH, uint32_t maxSS) {
  hipLaunchKernelGGL(k_prep_offsets_bs, dim3(cdiv((uint64_t)cdiv(maxH, 32) * cdiv(maxSS, 8), kBsThreads), np),
                     dim3(kBsThreads), 0, st, d);
}
static std::atomic<int> g_aes_bs{-1};
void set_aes_bs(int v) { g_aes_bs.store(v < 0 ? -1 : (v ? 1 : 0)); }
bool prep_offsets_bitsliced() {
  static const bool env = [] { const char* e = getenv("PM_AES_BS"); return e && e[0] == '1'; }();
  const int v = g_aes_bs.load();
  return v < 0 ? env : v == 1;
}
void prep_offsets(hipStream_t st, const PmPart* d, int np, uint32_t maxH, uint32_t maxSS) {
  if (prep_offsets_bitsliced()) prep_offsets_bs(st, d, np, maxH, maxSS);
  else prep_offsets_tt(st, d, np, maxH, maxSS);
}
static std::atomic<int> g_fold_rot{-1};
void set_fold_rot(int v) { g_fold_rot.store(v < 0 ? -1 : (v ? 1 : 0)); }
// the shapes k_prep_fold_rot folds: one ChunkSize of 512 or 1,024, whole 32-B slices
static bool fold_rot_shape(uint32_t minCS, uint32_t maxCS, uint32_t E) {
  return minCS == maxCS && (maxCS == 512 || maxCS == 1024) && E % 2 == 0 && E >= 4;
}
// The "fold_rot" option (else PM_FOLD_ROT, default on) is read HERE ONLY, and
// this is called only while an engine is created: that is where the image is
// built, shared or skipped and where the chunk-major table is allocated or not
// (fold_needs_tab).  Every later launch decides from what its engine was
// created with (have_img) and the shape (fold_form), never from the option: an
// engine created with the image has no chunk-major table, and the pipelined
// fold launched on it after the option changed would read PmPart::tab == null.
bool fold_image_ok(uint32_t minCS, uint32_t maxCS, uint32_t E) {
  static const bool env = [] { const char* e = getenv("PM_FOLD_ROT"); return !e || e[0] != '0'; }();
  const int v = g_fold_rot.load();
  return (v < 0 ? env : v == 1) && fold_rot_shape(minCS, maxCS, E);
}
// the double-buffered fold's column-slice width: the widest of 8, 4, 2 words
// whose two chunk buffers fit in LDS and whose staging fits kFoldMaxItems 16-B
// items per thread; 0: none does (very wide chunks)
static uint32_t fold_blk_sw(uint32_t maxCS) {
  auto fits = [&](uint32_t sw) {
    return 2ull * (maxCS + 1) * sw * 8 <= 150u * 1024 &&
           (uint64_t)maxCS * (sw / 2) <= (uint64_t)kFoldMaxItems * kFoldThreads;
  };
  uint32_t sw = 8;
  while (sw > 2 && !fits(sw)) sw /= 2;
  return fits(sw) ? sw : 0;
}
int fold_form(uint32_t minCS, uint32_t maxCS, uint32_t E, bool have_img, uint32_t npk, uint32_t qf) {
  if ((E & ~3u) == 0) return FOLD_GATHER;   // xorSlices folds nothing: zero parities
  if (have_img && fold_rot_shape(minCS, maxCS, E))
    return maxCS == 512 ? (qf ? FOLD_ROT512Q : npk ? FOLD_ROT512P : FOLD_ROT512) : FOLD_ROT1024;
  if (minCS == maxCS && (maxCS == 512 || maxCS == 1024 || maxCS == 2048) && E % 2 == 0) return FOLD_PIPE;
  if (E % 2 || !fold_blk_sw(maxCS)) return FOLD_GATHER;   // odd entries or very wide chunks
  return FOLD_BLK;
}
bool fold_needs_tab(uint32_t minCS, uint32_t maxCS, uint32_t E, bool have_img) {
  // the folds that stage a chunk-major PRF table row through LDS (k_prep_fold_pipe
  // / _blk); the rotated fold and the unblocked gather read the tag-major one
  const int form = fold_form(minCS, maxCS, E, have_img);
  return form == FOLD_PIPE || form == FOLD_BLK;
}
static std::atomic<int> g_fold_pack{-1};
void set_fold_pack(int v) { g_fold_pack.store(v < 0 ? -1 : (v ? 1 : 0)); }
static std::atomic<int> g_fold_bits{-1};
void set_fold_bits(int v) { g_fold_bits.store(v < 0 ? -1 : (v ? 1 : 0)); }
// Like "fold_rot", "fold_pack" (else PM_FOLD_PACK, default on) and "fold_bits"
// (else PM_FOLD_BITS, default on) are read here only, while a server's image is
// built; its clients share the image and so the decision.  Level 0: the plain
// image ("fold_pack" off); 1: the packed one (FOLD_ROT512P) where the DB
// qualifies ("fold_bits" off); 2: the bit-packed one (FOLD_ROT512Q) too.
static int fold_pack_level() {
  static const bool env = [] { const char* e = getenv("PM_FOLD_PACK"); return !e || e[0] != '0'; }();
  static const bool envb = [] { const char* e = getenv("PM_FOLD_BITS"); return !e || e[0] != '0'; }();
  const int v = g_fold_pack.load(), b = g_fold_bits.load();
  if (!(v < 0 ? env : v == 1)) return 0;
  return (b < 0 ? envb : b == 1) ? 2 : 1;
}
// Whole packed slices: 16 coordinate words each, inside the folded E & ~3 words.
uint32_t fold_pack_slices(uint32_t minCS, uint32_t maxCS, uint32_t E, uint32_t dim) {
  if (fold_pack_level() < 1 || fold_form(minCS, maxCS, E, true) != FOLD_ROT512) return 0;
  return fold_pack_shape(E, dim);
}
// The shape rule of the bit-packed image: a DB that takes the packed image (npk
// != 0: FOLD_ROT512's shape, dim % 16 == 0, zero low halves), whose constant
// bits (row_bits_or's flags) allow 12-bit coordinate fields, 20-bit id fields
// or both, takes the fields that give the fewest slices, if those are fewer
// than the packed image's; otherwise 0 (also where "fold_bits" is off).  Quads of four words: dim % 4 == 0 and
// (E & ~3) % 2 == 0 hold for every such shape.
uint32_t fold_bits_form(uint32_t E, uint32_t dim, uint32_t npk, uint32_t flags) {
  if (fold_pack_level() < 2 || !npk || (flags & kRowLowHalf)) return 0;
  const bool cq = !(flags & kRowCoordBits), iq = !(flags & kRowIdBits);
  uint32_t best = 0, best_nsl = (E & ~3u) / 4 - npk;
  auto offer = [&](uint32_t w1, uint32_t w2) {
    const uint32_t qf = w1 | (w2 << 8) | ((dim / 4) << 16), nsl = fold_bits_nsl(fold_bits_of(qf, E));
    if (nsl < best_nsl) { best = qf; best_nsl = nsl; }
  };
  if (iq) offer(16, 20);
  if (cq) offer(12, 32);
  if (cq && iq) offer(12, 20);
  return best;
}
uint32_t fold_bits_slices(uint32_t qf, uint32_t E) { return qf ? fold_bits_nsl(fold_bits_of(qf, E)) : 0; }
uint32_t fold_pack_shape(uint32_t E, uint32_t dim) {
  return dim && dim % 16 == 0 && dim / 8 <= E / 4 ? dim / 16 : 0;
}
static std::atomic<int> g_answer_pack{-1};
void set_answer_pack(int v) { g_answer_pack.store(v < 0 ? -1 : (v ? 1 : 0)); }
uint32_t answer_pack_shape(uint32_t E, uint32_t dim) {
  if (!dim || E % 4 || E > 256 || dim % 8 || dim >= 2 * E) return 0;
  const uint32_t stride = 2 * dim + 4 * (2 * E - dim);   // bytes
  return stride % 16 ? 0 : stride / 16;
}
// "answer_pack" (else PM_ANSWER_PACK, default on) is read here only, while a
// server is created; its clients share the image and so the decision.
uint32_t answer_pack_segs(uint32_t E, uint32_t dim) {
  static const bool env = [] { const char* e = getenv("PM_ANSWER_PACK"); return !e || e[0] != '0'; }();
  const int v = g_answer_pack.load();
  return (v < 0 ? env : v == 1) ? answer_pack_shape(E, dim) : 0;
}
void answer_pack_image(hipStream_t st, uint64_t* img, const uint64_t* rows, uint64_t nrows, uint32_t E, uint32_t dim) {
  const uint32_t nseg = answer_pack_shape(E, dim);
  const uint64_t nitems = nrows * nseg;
  unsigned grid = cdiv(nitems, kBlock);
  if (grid > 256 * 32) grid = 256 * 32;
  if (grid) hipLaunchKernelGGL(k_answer_pack_image, dim3(grid), dim3(kBlock), 0, st, (uint4*)img, rows, nitems, E, nseg, dim / 8);
}
uint32_t row_bits_or(hipStream_t st, const uint64_t* rows, uint64_t nrows, uint32_t E, uint32_t dim, uint32_t* flag) {
  const uint32_t all = kRowLowHalf | kRowCoordBits | kRowIdBits;
  if (hipMemsetAsync(flag, 0, 4, st) != hipSuccess) return all;
  unsigned grid = cdiv(nrows * (E / 2), kBlock);
  if (grid > 256 * 32) grid = 256 * 32;
  if (grid) hipLaunchKernelGGL(k_row_bits_or, dim3(grid), dim3(kBlock), 0, st, rows, nrows, E, dim, flag);
  uint32_t h = all;
  if (hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return all;
  return h;
}
uint64_t fold_image_words(uint32_t SS, uint32_t E, uint32_t CS, uint32_t npk, uint32_t qf) {
  const uint32_t nsl = qf ? fold_bits_slices(qf, E) : E / 4 - npk;
  return (uint64_t)nsl * (SS / rot_nch(CS)) * (kRotBufBytes / 8);
}
void fold_image(hipStream_t st, uint64_t* img, const uint64_t* rows, uint64_t N, uint32_t SS, uint32_t E, uint32_t CS,
                uint32_t npk, uint32_t qf) {
  const uint64_t nitems = fold_image_words(SS, E, CS, npk, qf) / 2;
  unsigned grid = cdiv(nitems, kBlock);
  if (grid > 256 * 32) grid = 256 * 32;
  if (qf)   // CS 512 only (fold_bits_form)
    hipLaunchKernelGGL(k_fold_image_bits, dim3(grid), dim3(kBlock), 0, st, (uint4*)img, rows, N, SS / rot_nch(CS), E, nitems, qf);
  else
    hipLaunchKernelGGL(k_fold_image, dim3(grid), dim3(kBlock), 0, st, (uint4*)img, rows, N, SS / rot_nch(CS), E, nitems,
                       CS, npk);
}
void fold_image_map(uint32_t CS, uint32_t SS, uint32_t npk, uint64_t x0, uint64_t n, uint64_t* row, uint32_t* word,
                    uint8_t* packed) {
  for (uint64_t i = 0; i < n; ++i) {
    const FoldImageSrc s = fold_image_src(x0 + i, SS / rot_nch(CS), CS, npk);
    row[i] = s.row; word[i] = s.word; packed[i] = s.packed;
  }
}
int prep_fold(hipStream_t st, const PmPart* d, int np, uint32_t maxH, const uint64_t* db, uint32_t E,
              uint32_t minCS, uint32_t maxCS, const uint64_t* zero16, uint32_t clients, bool have_img,
               uint32_t minH, uint32_t npk, uint32_t qf) {
  // the form follows from what the engine was created with (have_img) and the
  // shape alone (fold_form): the same inputs that decided whether PmPart::tab exists
  const int form = fold_form(minCS, maxCS, E, have_img, npk, qf);
  const uint32_t EX = E & ~3u;
  if (EX == 0) {
    hipLaunchKernelGGL(k_prep_fold<2>, dim3(cdiv((uint64_t)maxH * E, kBlock), np), dim3(kBlock), 0,
                       st, d, db, E);
    return form;
  }
  const uint32_t ng = cdiv(maxH, (uint64_t)kFoldThreads * kFoldHPT);      // pipelined fold
  const uint32_t ngb = cdiv(maxH, (uint64_t)kFoldThreads * kFoldHPTBlk);  // double-buffered fold
  auto launch = [&](uint32_t sw, uint32_t w0, uint32_t nsl) {
    const size_t lds = 2ull * (maxCS + 1) * sw * 8;
    const dim3 grid(ngb, nsl, np), blk(kFoldThreads);
    if (sw == 8) hipLaunchKernelGGL(k_prep_fold_blk<8>, grid, blk, lds, st, d, db, zero16, E, w0);
    else if (sw == 4) hipLaunchKernelGGL(k_prep_fold_blk<4>, grid, blk, lds, st, d, db, zero16, E, w0);
    else hipLaunchKernelGGL(k_prep_fold_blk<2>, grid, blk, lds, st, d, db, zero16, E, w0);
  };
  if (form == FOLD_ROT512 || form == FOLD_ROT512P || form == FOLD_ROT512Q || form == FOLD_ROT1024 || form == FOLD_PIPE) {
    // (SW, G): CS 512 -> (4, 1), 1024 -> (4, 2), 2048 -> (2, 2); EX % SW == 0
    // the packed image: npk slices in place of the 2 npk coordinate slices
    // the bit-packed image: its own slice count
    const uint32_t psw = maxCS == 2048 ? 2 : 4;
    const uint32_t nsl = form == FOLD_ROT512Q ? fold_bits_slices(qf, E) : EX / psw - (form == FOLD_ROT512P ? npk : 0);
    const uint32_t K = clients && np % clients == 0 ? clients : 1, npg = (np / K) * ng;
    const uint32_t lw = 16 / psw, per_pg = K * cdiv(nsl, lw) * lw;
#ifndef PM_FOLD_NB512
#define PM_FOLD_NB512 4
#endif
#ifndef PM_FOLD_D512
#define PM_FOLD_D512 1
#endif
    if (form != FOLD_PIPE) {   // the bank-rotated fold (same slices and block order)
      // virtual hint groups over the K clients of each partition (see the kernel)
      const uint64_t HB = (uint64_t)kFoldThreads * rot_hpl(maxCS);
      const uint32_t ngc = minH >= HB ? 0u : (uint32_t)cdiv(maxH, HB);
      const uint32_t nvg = ngc ? K * ngc : (uint32_t)cdiv((uint64_t)K * maxH, HB), npv = (np / K) * nvg;
      // whole tiles of GB pairs x SB slices, dealt over the 8 XCDs (the kernel's sixth parameter: the packed
      // coordinate slices, 0 for the plain image; its ninth: the bit-packed image's fields)
      const uint32_t GB = form == FOLD_ROT512Q ? PM_ROTQ_GB : PM_ROT_GB, SB = form == FOLD_ROT512Q ? PM_ROTQ_SB : PM_ROT_SB;
      const uint32_t grid = 8 * cdiv((uint64_t)cdiv(npv, GB) * cdiv(nsl, SB), 8) * GB * SB;
      if (form != FOLD_ROT1024)
        hipLaunchKernelGGL(k_prep_fold_rot<512>, dim3(grid), dim3(kFoldThreads), 0, st, d, E, nvg, nsl, npv,
                           form == FOLD_ROT512P ? npk : 0u, K, ngc, form == FOLD_ROT512Q ? qf : 0u, GB, SB);
      else
        hipLaunchKernelGGL(k_prep_fold_rot<1024>, dim3(grid), dim3(kFoldThreads), 0, st, d, E, nvg, nsl, npv, 0u, K, ngc,
                           0u, GB, SB);
      return form;
    }
    const uint32_t nb = maxCS == 512 ? PM_FOLD_NB512 : 3;   // LDS buffers: <= 150 KB
    const size_t lds = (size_t)nb * ((maxCS + 1) * psw + kPipeTabWords) * 8;
    const dim3 grid(cdiv(npg, 8) * 8 * per_pg), blk(kFoldThreads);
    if (maxCS == 512)
      hipLaunchKernelGGL((k_prep_fold_pipe<4, 1, PM_FOLD_NB512, PM_FOLD_D512>), grid, blk, lds, st, d, db, zero16, E, ng, nsl,
                         npg, K);
    else if (maxCS == 1024)
      hipLaunchKernelGGL((k_prep_fold_pipe<4, 2, 3>), grid, blk, lds, st, d, db, zero16, E, ng, nsl, npg, K);
    else
      hipLaunchKernelGGL((k_prep_fold_pipe<2, 2, 3>), grid, blk, lds, st, d, db, zero16, E, ng, nsl, npg, K);
    return form;
  }
  if (form == FOLD_GATHER) {   // very wide chunks or odd entries: the unblocked gather
    if (E % 2 == 0)
      hipLaunchKernelGGL(k_prep_fold<2>, dim3(cdiv((uint64_t)maxH * (EX / 2), kBlock), np),
                         dim3(kBlock), 0, st, d, db, E);
    else
      hipLaunchKernelGGL(k_prep_fold<1>, dim3(cdiv((uint64_t)maxH * EX, kBlock), np), dim3(kBlock), 0,
                         st, d, db, E);
    return form;
  }
  const uint32_t sw = fold_blk_sw(maxCS);          // FOLD_BLK: sw != 0
  const uint32_t nfull = EX / sw, rem = EX % sw;   // EX is a multiple of 4
  if (nfull) launch(sw, 0, nfull);
  if (rem) launch(rem, nfull * sw, 1);
  return form;
}
void prep_repl(hipStream_t st, const PmPart* d, int np, uint32_t maxRepl, const uint64_t* db,
               uint32_t E) {
  if (E % 2 == 0)
    hipLaunchKernelGGL(k_prep_repl<2>, dim3(cdiv(maxRepl, kReplRows), np), dim3(kBlock), 0, st, d, db, E);
  else
    hipLaunchKernelGGL(k_prep_repl<1>, dim3(cdiv(maxRepl, kReplRows), np), dim3(kBlock), 0, st, d, db, E);
}
void server_answer(hipStream_t st, const PmPart* d, const uint32_t* offs, uint32_t nq, uint32_t SS,
                   const uint64_t* db, uint32_t E, uint64_t* out) {
  if (E % 2 == 0)
    hipLaunchKernelGGL(k_server_answer<2>, dim3(nq), dim3(kBlock), 0, st, d, offs, SS, db, E, out);
  else
    hipLaunchKernelGGL(k_server_answer<1>, dim3(nq), dim3(kBlock), 0, st, d, offs, SS, db, E, out);
}
void server_answer_parts(hipStream_t st, const PmSrvPart* sp, const uint32_t* qpart, const uint32_t* offs,
                         uint32_t nq, uint32_t stride, const uint64_t* db, const uint64_t* dbp, uint32_t pk_nseg,
                         uint32_t pk_cseg, uint32_t E, uint64_t* out) {
  const uint32_t EX = E & ~3u;
  if (dbp)
    hipLaunchKernelGGL((k_server_answer_parts<2, true>), dim3(nq), dim3(kBlock), 0, st, sp, qpart, offs, stride, dbp,
                       2 * pk_nseg, pk_nseg, pk_cseg, E, out);
  else if (E % 2 == 0)
    hipLaunchKernelGGL((k_server_answer_parts<2, false>), dim3(nq), dim3(kBlock), 0, st, sp, qpart, offs, stride, db,
                       E, EX / 2, 0u, E, out);
  else
    hipLaunchKernelGGL((k_server_answer_parts<1, false>), dim3(nq), dim3(kBlock), 0, st, sp, qpart, offs, stride, db,
                       E, EX, 0u, E, out);
}
void l2_rows(hipStream_t st, const float* rows, uint64_t stride, uint64_t nrows, const uint32_t* ids,
             const float* q, uint32_t dim, float* out, uint64_t seglen) {
  if (!nrows) return;
  hipLaunchKernelGGL(k_l2_rows, dim3(cdiv(nrows * 8, kBlock)), dim3(kBlock), 0, st, rows, stride, nrows,
                     ids, q, dim, out, seglen);
}
void ip_rows(hipStream_t st, const uint32_t* rows, uint64_t nrows, const uint32_t* q, uint32_t dim,
             uint32_t* per_row, uint32_t* sum) {
  if (!per_row && dim % 4 == 0 && dim <= 4096) {
    const uint64_t n4 = nrows * dim / 4;
    unsigned grid = cdiv(n4, kBlock);
    if (grid > 256 * 8) grid = 256 * 8;   // 8 workgroups per CU: 2,048 x 256 threads, 16 waves per CU
    if (grid == 0) return;
    hipLaunchKernelGGL(k_ip_scan, dim3(grid), dim3(kBlock), 0, st, (const uint4*)rows, n4, q, dim, sum);
    return;
  }
  if (!nrows) return;
  hipLaunchKernelGGL(k_ip_rows, dim3(cdiv(nrows * 16, kBlock)), dim3(kBlock), 0, st, rows, nrows, q, dim,
                     per_row, sum);
}
void ip_fill(hipStream_t st, uint32_t* rows, uint64_t N, uint32_t D, uint64_t r0) {
  const uint64_t n4 = N * D / 4;
  unsigned grid = cdiv(n4, kBlock);
  if (grid > 256 * 16) grid = 256 * 16;
  if (grid == 0) return;
  hipLaunchKernelGGL(k_ip_fill, dim3(grid), dim3(kBlock), 0, st, (uint4*)rows, n4, D, r0);
}
void db_synth(hipStream_t st, uint64_t* dst, uint64_t r0, uint64_t rows, uint32_t E, uint64_t db_seed) {
  const uint64_t nw = rows * E;
  unsigned grid = cdiv(nw, kBlock);
  if (grid > 256 * 32) grid = 256 * 32;
  if (grid == 0) return;
  hipLaunchKernelGGL(k_db_synth, dim3(grid), dim3(kBlock), 0, st, dst, r0, nw, E, sm64(db_seed + DOM_SYNTH_DB));
}
void gather_rows(hipStream_t st, const uint64_t* const* src, uint64_t n, uint32_t E, uint64_t* out) {
  if (n) hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)n), dim3(kBlock), 0, st, src, E, out);
}
void prf_batch(hipStream_t st, const uint32_t* rk, const uint64_t* tags, const uint64_t* xs, uint64_t n,
               uint64_t* out) {
  unsigned grid = cdiv(n, kBlock * 16);
  if (grid == 0) return;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(k_prf_batch, dim3(grid), dim3(kBlock), 0, st, rk, tags, xs, n, out);
}
}  // namespace pmk
